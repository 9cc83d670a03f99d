"""The PAMR kernels (csrc/pamr.hip: simseg_pamr; ops.pamr, segpost.pamr_masks, the `refiner` keyword) against the float64 statement of
the definition (tests/_pamr_ref.py pamr_np), on the smallest shapes at which they can still go wrong.

Refined map: |m - m_ref| <= 2e-4 everywhere.  Weights whose logit lies more than ~88 below the row maximum are zero in fp32; the
hardware exponential's relative error on the rest is at most ~1e-5; an averaging step is a convex combination, so that adds at most 1e-5
per step, 1e-4 over 10 steps; the allowance is twice that.
Masks: equal to the float64 masks on every pixel whose float64 value is farther than 2e-4 from 0.5, and the pixels left out are at most
2 % of a case's pixels (a condition on the case, asserted).
Every case prints one `pamr |` line before it asserts; profiles/pamr_tests.txt is that table."""
import functools

import numpy as np
import pytest
import torch

import _pamr_ref as P

pytestmark = pytest.mark.gpu

TOL, BAND, CAP = 2e-4, 2e-4, 0.02

#        name              H    W   B  K  dilations      iters  visited slots per image (None = no candidate table: all of them)
CASES = [("16x16",         16,  16, 1, 2, P.DILATIONS,   10, None),              # every dilation above 8 clamps on all sides
         ("17x50",         17,  50, 1, 2, P.DILATIONS,   10, None),              # odd sizes, no multiple of any tile
         ("40x56",         40,  56, 1, 2, P.DILATIONS,   10, None),
         ("64x64-b3k5",    64,  64, 3, 5, P.DILATIONS,   10, [(), (1, 3), (0, 1, 2, 3, 4)]),        # 0 / 2 / 5 of 5 slots visited
         ("40x56-d1",      40,  56, 1, 2, (1,),          10, None),
         ("40x56-d3-64",   40,  56, 1, 2, (3, 64),       10, None),              # the 64-pixel dilation is wider than the image
         ("40x56-it0",     40,  56, 1, 2, P.DILATIONS,   0,  None),
         ("40x56-it1",     40,  56, 1, 2, P.DILATIONS,   1,  None),
         ("128x96",        128, 96, 1, 3, P.DILATIONS,   10, [(0, 2)])]          # crosses block boundaries in both directions


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (rgb [B,H,W,3] uint8, maps [B,K,H,W] float32, cand [B,K] int32 or None, m_ref [B,K,H,W] float64 (zero for unvisited slots),
    dilations, iters): computed once per case and shared."""
    _, H, W, B, K, dil, iters, visited = next(c for c in CASES if c[0] == name)
    scenes = [P.scene(H, W, K, seed=1000 * H + 10 * W + b) for b in range(B)]
    rgb, maps = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    cand = None
    if visited is not None:
        cand = np.full((B, K), -1, np.int32)
        for b, ks in enumerate(visited):
            cand[b, list(ks)] = [7 + 3 * k for k in ks]
    ref = np.zeros((B, K, H, W), np.float64)
    for b in range(B):
        ks = list(range(K)) if visited is None else list(visited[b])
        if ks:
            ref[b, ks] = P.pamr_np(rgb[b], maps[b, ks], dil, iters)
    for a in (rgb, maps, ref):
        a.setflags(write=False)
    return rgb, maps, cand, ref, dil, iters


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()         # (a copy: the cached arrays are read-only)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_refined_map_and_masks_vs_float64(name):
    from simseg_amd import ops
    rgb, maps, cand, ref, dil, iters = _case(name)
    mask, m = ops.pamr(_dev(rgb), _dev(maps), _dev(cand), dilations=dil, iters=iters, want_m=True)
    mask, m = mask.cpu().numpy(), m.cpu().numpy()
    err = float(np.abs(m - ref).max())
    visited = np.ones(ref.shape[:2], bool) if cand is None else cand >= 0
    near = (np.abs(ref - 0.5) <= BAND) & visited[:, :, None, None]
    want = np.where(ref > 0.5, 255, 0).astype(np.uint8)
    wrong = int(((mask != want) & ~near).sum())
    left, total = int(near.sum()), int(visited.sum()) * ref.shape[2] * ref.shape[3]
    print(f"pamr | {name:<12} | max |m - m_ref| {err:.3e} (allowance {TOL:.1e}) | pixels within {BAND:.0e} of 0.5 left out {left} of {total} = "
          f"{100.0 * left / total:.3f} % (cap {100 * CAP:.0f} %) | masks differing elsewhere {wrong}")
    assert err <= TOL
    assert left <= CAP * total
    assert wrong == 0
    if cand is not None:                                              # unvisited slots (and the image without any) come back exactly zero
        assert not mask[~visited].any() and not m[~visited].any()
    if iters == 0:                                                    # the unary decision, bit for bit
        assert np.array_equal(mask[visited], np.where(maps > 0.5, 255, 0).astype(np.uint8)[visited]) and np.array_equal(m[visited], maps[visited])
    m_only = ops.pamr(_dev(rgb), _dev(maps), _dev(cand), dilations=dil, iters=iters)
    assert m_only[1] is None and np.array_equal(m_only[0].cpu().numpy(), mask)


@pytest.mark.parametrize("iters", [0, 1, 10])
def test_scale16_equals_the_upsampled_map(iters):
    """scale=16 on a 4x4 grid == scale=1 on the repeat_interleave'd map, bit for bit."""
    from simseg_amd import ops
    rgb = _dev(P.scene(64, 64, 1, seed=3)[0])[None]
    g = torch.Generator().manual_seed(iters)
    lo = torch.rand(1, 3, 4, 4, generator=g).cuda()
    cand = torch.tensor([[4, -1, 9]], dtype=torch.int32).cuda()
    up = lo.repeat_interleave(16, 2).repeat_interleave(16, 3).contiguous()
    a = ops.pamr(rgb, lo, cand, iters=iters, scale=16, want_m=True)
    b = ops.pamr(rgb, up, cand, iters=iters, scale=1, want_m=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0][0, 0].any() and not a[0][0, 1].any() and not a[1][0, 1].any()


def test_batch_equals_per_image_calls_and_chunking():
    from simseg_amd import ops, segpost
    rgb, maps, cand, _, dil, iters = _case("64x64-b3k5")
    rgb, maps, cand = _dev(rgb), _dev(maps), _dev(cand)
    mask, m = ops.pamr(rgb, maps, cand, want_m=True)
    for b in range(rgb.shape[0]):
        m1, q1 = ops.pamr(rgb[b], maps[b], cand[b], want_m=True)
        assert torch.equal(mask[b], m1) and torch.equal(m[b], q1)
    whole = segpost.pamr_masks(maps, cand, rgb)
    assert torch.equal(whole, mask)
    assert torch.equal(segpost.pamr_masks(maps, cand, rgb, chunk=1), whole)
    assert torch.equal(segpost.pamr_masks(maps, cand, rgb, chunk=2), whole)
    few = segpost.pamr_masks(maps, cand, rgb, iters=2, dilations=(1, 2))
    assert torch.equal(few, ops.pamr(rgb, maps, cand, iters=2, dilations=(1, 2))[0]) and not torch.equal(few, whole)


def test_flat_image_is_the_uniform_average():
    from simseg_amd import ops
    H, W = 40, 56
    rgb = torch.full((H, W, 3), 77, dtype=torch.uint8).cuda()
    maps = P.scene(H, W, 2, seed=9)[1]
    _, m = ops.pamr(rgb, _dev(maps), iters=1, want_m=True)
    want = P.propagate_np(np.full((48, H, W), 1.0 / 48.0), maps.astype(np.float64))
    err = float(np.abs(m.cpu().numpy() - want).max())
    print(f"pamr | flat 40x56   | one step vs the float64 uniform average: {err:.3e} (allowance 1.0e-06)")
    assert err <= 1e-6


def test_refusals_leave_the_outputs_untouched():
    from simseg_amd import lib, ops
    import ctypes
    B, K, H, W = 1, 2, 32, 32
    rgb = torch.zeros(B, H, W, 3, dtype=torch.uint8).cuda()
    prob = torch.rand(B, 9, H, W).cuda()
    mask = torch.full((B, 9, H, W), 7, dtype=torch.uint8).cuda()
    m = torch.full((B, 9, H, W), 7.0).cuda()
    ws = torch.empty(lib.raw("simseg_pamr_workspace_bytes", B, 8, H, W, 8), dtype=torch.uint8).cuda()
    need = lib.raw("simseg_pamr_workspace_bytes", B, K, H, W, 6)
    assert need == 4 * B * H * W * (48 + 2 * K)
    assert lib.raw("simseg_pamr_workspace_bytes", B, 9, H, W, 6) < 0 and lib.raw("simseg_pamr_workspace_bytes", B, K, H, W, 9) < 0

    def go(K=K, dil=P.DILATIONS, n_dil=None, iters=10, ws_bytes=None, scale=1):
        arr = (ctypes.c_int * max(len(dil), 1))(*dil)
        lib.call("simseg_pamr", rgb.data_ptr(), prob.data_ptr(), None, mask.data_ptr(), m.data_ptr(), B, K, H, W, arr, len(dil) if n_dil is None else n_dil,
                 iters, scale, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, ops.stream())

    for kw in [dict(n_dil=0), dict(dil=(1,) * 9), dict(dil=(1, 0)), dict(dil=(65,)), dict(iters=-1), dict(iters=65), dict(K=0), dict(K=9),
               dict(ws_bytes=need - 1), dict(scale=5)]:
        with pytest.raises(RuntimeError, match="pamr"):
            go(**kw)
    torch.cuda.synchronize()
    assert bool((mask == 7).all()) and bool((m == 7.0).all())
    go()                                                              # and the same call with everything in range runs
    torch.cuda.synchronize()
    n = B * K * H * W                                                 # ... and writes its B x K planes, nothing behind them
    assert not bool((mask.reshape(-1)[:n] == 7).any()) and bool((mask.reshape(-1)[n:] == 7).all())
    assert not bool((m.reshape(-1)[:n] == 7.0).any()) and bool((m.reshape(-1)[n:] == 7.0).all())


def _tiny_route(monkeypatch, B=2, size=96, C=21):
    from test_gpu_miou_gate import MEAN, STD, _build, _voc_like
    from test_gpu_slide_ragged import _Memo, _memo_ops
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    model = _build("vit_test_patch16", 128, "bert-test", 128, size, seed=5).eval().cuda()
    g = torch.Generator().manual_seed(3)
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=g), dim=-1).cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    memo = _Memo(model)                       # (the towers' split-K sums differ in the last bits from call to call: both sides get one call's outputs)
    _memo_ops(monkeypatch, memo, text)
    return memo, text, mean, std, g, _voc_like


def test_eval_batch_with_pamr_equals_the_refine_hook(monkeypatch):
    from simseg_amd import ops, segpost
    B, S, C = 2, 96, 21
    memo, text, mean, std, g, voc = _tiny_route(monkeypatch, B, S, C)
    x = voc(B, S, seed=23)[1].cuda()
    labels = torch.randint(0, C, (B, 80, 120), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    u8 = (((x * std) + mean) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    seen = []

    def hook(up, cand_idx, cand_score):
        seen.append(int((cand_idx >= 0).sum()))
        return ops.pamr(u8, up.contiguous(), cand_idx)[0]

    with torch.no_grad():
        a = segpost.eval_batch(memo, x, labels, text, 10, mean=mean, std=std, refiner="pamr", want_pred=True)
        b = segpost.eval_batch(memo, x, labels, text, 10, mean=mean, std=std, refine=hook, want_pred=True)
        c = segpost.eval_batch(memo, x, labels, text, 10, mean=mean, std=std, refiner=("pamr", {"iters": 10, "chunk": 1}), want_pred=True)
        raw = segpost.eval_batch(memo, x, labels, text, 10, crf=False, want_pred=True)
    assert seen and seen[0] >= B
    for other in (b, c):
        assert torch.equal(a["masks"], other["masks"]) and torch.equal(a["pred"], other["pred"]) and torch.equal(a["hist"], other["hist"])
    assert not torch.equal(a["masks"], raw["masks"])                  # the refinement did something


def test_finish_sliding_with_pamr_equals_per_image_calls(monkeypatch):
    from simseg_amd import ops, segpost
    C, win, stride = 21, 96, 48
    memo, text, mean, std, g, voc = _tiny_route(monkeypatch, 2, win, C)
    sizes = [(96, 150), (80, 80)]
    xs = [voc(1, 160, seed=31 + i)[1][0, :, :h, :w].contiguous().cuda() for i, (h, w) in enumerate(sizes)]
    labs = [torch.randint(0, C, (h + 7, w - 5), generator=g, dtype=torch.int64).to(torch.uint8).cuda() for h, w in sizes]
    hist = torch.zeros(3, C, device="cuda", dtype=torch.int64)
    with torch.no_grad():
        st = segpost.encode_images_sliding(memo, xs, text, 10, win=win, stride=stride, mean=mean, std=std, refiner="pamr")
        out = segpost.finish_sliding(st, labs, hist=hist, want_pred=True)
    assert st["refiner"] == ("pamr", {}) and int((st["cand_idx"] >= 0).sum()) >= 2
    want_hist = torch.zeros_like(hist)
    for b, (h, w) in enumerate(sizes):
        u8 = (((xs[b][None] * std) + mean) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        cand, score = st["cand_idx"][b:b + 1], st["cand_score"][b:b + 1]
        maps = ops.slide_planes(st["prob"], st["plan"], b).contiguous()
        m, _ = ops.pamr(u8[0], maps, cand[0])
        closed = ops.close7(m[None], cand.reshape(-1))
        pred, want_hist = ops.seg_predict(closed, cand, score, labs[b][None].contiguous(), C, 255, hist=want_hist, want_pred=True)
        assert torch.equal(out["masks"][b], closed[0]) and torch.equal(out["pred"][b], pred[0])
    assert torch.equal(hist, want_hist)


def test_default_refiner_is_still_the_crf(monkeypatch):
    """refiner=None / "crf" is today's route under crf=True: the DenseCRF is called, PAMR is not, and the result equals the call without the
    keyword bit for bit in the same process."""
    from simseg_amd import segpost
    B, S, C = 2, 96, 21
    memo, text, mean, std, g, voc = _tiny_route(monkeypatch, B, S, C)
    x = voc(B, S, seed=23)[1].cuda()
    labels = torch.randint(0, C, (B, 80, 120), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    calls = {"crf": 0, "pamr": 0}
    crf, pamr = segpost.crf_masks, segpost.pamr_masks
    monkeypatch.setattr(segpost, "crf_masks", lambda *a, **k: (calls.__setitem__("crf", calls["crf"] + 1), crf(*a, **k))[1])
    monkeypatch.setattr(segpost, "pamr_masks", lambda *a, **k: (calls.__setitem__("pamr", calls["pamr"] + 1), pamr(*a, **k))[1])
    with torch.no_grad():
        base = segpost.eval_batch(memo, x, labels, text, 10, mean=mean, std=std, want_pred=True)
        for refiner in (None, "crf"):
            got = segpost.eval_batch(memo, x, labels, text, 10, mean=mean, std=std, want_pred=True, refiner=refiner)
            assert torch.equal(base["masks"], got["masks"]) and torch.equal(base["pred"], got["pred"]) and torch.equal(base["hist"], got["hist"])
    assert calls == {"crf": 3, "pamr": 0}


def test_graph_capture_and_replay_give_the_eager_bits():
    """The whole call is a fixed sequence of launches with no host read: one capture, one replay.  (Last test of the file, default queue
    configuration.)"""
    from simseg_amd import ops
    rgb, maps, cand, _, _, _ = _case("64x64-b3k5")
    rgb, maps, cand = _dev(rgb), _dev(maps), _dev(cand)
    eager = ops.pamr(rgb, maps, cand, want_m=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keys = set(ops._PAMR_WS)
    with torch.cuda.graph(graph):
        mask, m = ops.pamr(rgb, maps, cand, want_m=True)
    mask.fill_(3)
    m.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mask, eager[0]) and torch.equal(m, eager[1])
    for k in set(ops._PAMR_WS) - keys:                                # the workspace of the capture stream lives in the graph's pool
        ops._PAMR_WS.pop(k)
