"""Window placement of the any-size sliding-window evaluation (segpost.slide_windows, DESIGN.md "Sliding windows on any image size") and
the pixel-resolution stitch it is defined by, written here as the explicit numpy loop that the GPU kernels are tested against
(tests/test_gpu_slide_ragged.py)."""
import numpy as np
import pytest

SIDES = (1, 15, 96, 97, 375, 427, 480, 500, 512, 640, 683, 1023, 2048)
GEOMS = ((96, 48), (512, 256), (512, 512), (512, 384))


def stitch_pixels_ref(win_maps, offsets, H, W, win):
    """win_maps [Nw, n*n, C] float32 (one image's windows, in window order), offsets [(y0, x0)] -> S [H, W, C] float32: per source pixel the
    sum, in window order, of cell ((y - y0) // 16, (x - x0) // 16) of every window that covers it, divided once by their count."""
    n = win // 16
    C = win_maps.shape[-1]
    acc = np.zeros((H, W, C), np.float32)
    cnt = np.zeros((H, W), np.int32)
    for m, (y0, x0) in zip(win_maps, offsets):
        px = np.repeat(np.repeat(m.reshape(n, n, C).astype(np.float32), 16, 0), 16, 1)      # [win, win, C]
        h, w = min(win, H - y0), min(win, W - x0)
        acc[y0:y0 + h, x0:x0 + w] += px[:h, :w]
        cnt[y0:y0 + h, x0:x0 + w] += 1
    return acc / cnt[..., None].astype(np.float32)


def normalise_ref(S):
    """min-max over the image (float32), binary = prob > 0.5 (a constant map gives NaN, hence 0) -> (prob, mask uint8 0 / 255)."""
    mn, mx = S.min(), S.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        prob = (S - mn) / (mx - mn)
    return prob, (prob > 0.5).astype(np.uint8) * 255


def test_exact_tilings_match_window_grid():
    from simseg_amd import segpost
    for win, stride in GEOMS + ((32, 16), (64, 16)):
        for wy in range(1, 5):
            for wx in range(1, 5):
                H, W = win + (wy - 1) * stride, win + (wx - 1) * stride
                assert segpost.window_grid(H, W, win, stride) == (wy, wx)
                want = [(i * stride, j * stride) for i in range(wy) for j in range(wx)]
                assert segpost.slide_windows(H, W, win, stride) == want


@pytest.mark.parametrize("win,stride", GEOMS)
def test_any_size_geometry(win, stride):
    from simseg_amd import segpost
    for H in SIDES:
        for W in SIDES:
            offs = segpost.slide_windows(H, W, win, stride)
            ny = max(H - win + stride - 1, 0) // stride + 1
            nx = max(W - win + stride - 1, 0) // stride + 1
            assert len(offs) == ny * nx
            ys, xs = sorted({y for y, _ in offs}), sorted({x for _, x in offs})
            assert offs == [(y, x) for y in ys for x in xs]                      # row-major
            assert len(ys) == ny and len(xs) == nx                                # strictly increasing offsets
            for L, o in ((H, ys), (W, xs)):
                if L < win:
                    assert o == [0]                                               # one window at the origin, padded past the border
                else:
                    assert o[-1] + win == L and o[0] == 0                          # flush with both borders
                cov = np.zeros(L, np.int32)
                for v in o:
                    cov[v:v + win] += 1
                assert cov.min() >= 1 and cov.max() <= -(-win // stride) + 1       # every pixel covered


def test_slide_windows_rejects_bad_geometry():
    from simseg_amd import segpost
    for bad in ((100, 50), (512, 0), (256, 512), (512, 264)):
        with pytest.raises(ValueError):
            segpost.slide_windows(600, 600, *bad)
    with pytest.raises(ValueError):
        segpost.slide_windows(0, 10)


@pytest.mark.parametrize("H,W,win,stride", [(80, 80, 96, 48), (131, 257, 96, 48), (96, 192, 96, 48), (97, 97, 32, 16), (40, 170, 48, 32)])
def test_pixel_stitch_partition_of_unity(H, W, win, stride):
    """Constant per-window maps stitch to the same constant everywhere; with an exact tiling the pixel map is the patch-grid stitch of
    the oracle (oracle/segpost_ref.stitch_windows) repeated x16."""
    from oracle import segpost_ref as SR
    from simseg_amd import segpost
    n, C = win // 16, 3
    offs = segpost.slide_windows(H, W, win, stride)
    maps = np.full((len(offs), n * n, C), 0.75, np.float32)                 # (a dyadic constant: the window sums are exact)
    np.testing.assert_array_equal(stitch_pixels_ref(maps, offs, H, W, win), np.full((H, W, C), 0.75, np.float32))
    np.testing.assert_allclose(stitch_pixels_ref(maps * np.float32(0.7 / 0.75), offs, H, W, win), np.full((H, W, C), 0.7), rtol=1e-6)
    if H >= win and W >= win and (H - win) % stride == 0 and (W - win) % stride == 0:
        rng = np.random.default_rng(1)
        maps = rng.standard_normal(maps.shape).astype(np.float32)
        wy, wx = segpost.window_grid(H, W, win, stride)
        patch = SR.stitch_windows(maps, wy, wx, n, stride // 16).reshape(H // 16, W // 16, C)
        np.testing.assert_array_equal(stitch_pixels_ref(maps, offs, H, W, win), np.repeat(np.repeat(patch, 16, 0), 16, 1))


def test_plan_tables():
    """ops.slide_plan's host side: windows grouped per image in list order, 16-aligned output planes."""
    import torch
    from simseg_amd import ops, segpost
    sizes = [(96, 150), (80, 80), (131, 257)]
    plan = ops.slide_plan(sizes, 96, 48, "cpu")
    want = [(b, y, x) for b, (H, W) in enumerate(sizes) for y, x in segpost.slide_windows(H, W, 96, 48)]
    assert plan["windows"] == want
    it = plan["img_tab"]
    assert it.dtype == torch.int64 and tuple(it.shape) == (3, 8)
    assert [int(v) for v in it[:, 4]] == [0, 3, 4] and [int(v) for v in it[:, 5] * it[:, 6]] == [3, 1, 10]
    assert all(o % 16 == 0 for o in plan["out_off"]) and plan["src_off"] == [0, 3 * 96 * 150, 3 * 96 * 150 + 3 * 80 * 80]
