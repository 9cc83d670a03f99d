"""The full training grammar on the device (simseg_amd/pipeline.py parse_chain(full=True), csrc/augment.hip simseg_train_chain) against
apply_pipeline_pil, Pillow's own calls in list order: zero differing bytes in the uint8 output and torch.equal on the fp32 planes
(test_gpu_train_pipeline._check), for the Gaussian blur, the hue shift, the grayscale, the distortion in every order and whole chains, at
S = 32 (the smallest), 96 (in LDS) and 288 (in global memory)."""
import itertools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import REPO
from test_gpu_train_augment import _edge_images, _synth
from test_gpu_train_pipeline import _check, _raws, _run

pytestmark = pytest.mark.gpu

SIMCLR = ["random_resize_crop", "random_flip", "color_distortion", "gaussian_blur"]
ALL11 = ["resize", "autoaug", "color_jitter", "gaussian_blur", "color_distortion"]
OLD_LISTS = [["random_resize_crop", "autoaug"], ["resize_bicubic", "random_crop", "random_flip", "color_jitter"], ["random_crop", "random_flip"],
             ["resize", "random_flip", "autoaug", "color_jitter"], ["random_flip", "random_resize_crop"],
             ["resize_bicubic", "center_crop", "color_jitter", "autoaug"], ["resize"], ["random_resize_crop", "random_flip", "color_jitter", "autoaug"]]
RADII = (0.1, 1.0, 1.41, 1.42, 2.0, 4.0)
NO_JITTER = (0, (0, 1, 2, 3), 1.0, 1.0, 1.0, 0.0, 0)              # a distortion that does nothing


def _cfg(names, S, extra=(), distortion=None, blur=None):
    """The shipped config with train_transforms = names, every size set so that the list ends at S x S, and the SimCLR keys given."""
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    argv = [f"transforms.train_transforms=[{','.join(names)}]", f"transforms.resize.size={S}", f"transforms.resize_bicubic.size={S}",
            f"transforms.random_crop.size={S}", f"transforms.center_crop.size={S}", f"transforms.random_resize_crop.size={S}"] + list(extra)
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), argv, update_clip_config)
    for key, val in (("color_distortion", distortion), ("gaussian_blur", blur)):
        dict.pop(cfg.transforms, key, None)
        if val is not None:
            dict.__setitem__(cfg.transforms, key, dict(val))
    return cfg


def _chain(names, S, extra=(), **kw):
    from simseg_amd import pipeline as P
    cfg = _cfg(names, S, extra, **kw)
    return P.parse_chain(cfg.transforms.train_transforms, cfg, full=True)


def _noise(S, seed):
    return np.random.default_rng(seed).integers(0, 256, (S, S, 3), dtype=np.uint8)


def _border(S):
    """Constant but for its border rows and columns: what the clamp at a line's ends reads."""
    a = np.full((S, S, 3), 60, np.uint8)
    a[0], a[-1], a[:, 0], a[:, -1] = (250, 10, 0), (0, 255, 30), (5, 200, 255), (255, 255, 0)
    return a


@pytest.mark.parametrize("S", [32, 96, 288])
def test_blur_alone(S):
    """Square S x S images under [resize] (the identity) and raw images, every radius: l goes 0 -> 1 between 1.41 and 1.42, radius 4
    has the box radius 3."""
    from simseg_amd import pipeline as P
    chain = _chain(["resize", "gaussian_blur"], S, blur={"radius_max": 4.0})
    raws = [_noise(S, 1), _noise(S, 2), _border(S)] + _edge_images(S) + _raws()[:3]
    for r in RADII:
        p = P.explicit_pipeline_params(chain, len(raws), blur=(1, r))
        assert P.op_chain(chain, p, 0)[0][0] == P.OP_BLUR
        _, u8 = _check(raws, p, chain, label=f"blur radius {r}")
        assert np.array_equal(u8[0], P.gaussian_blur_ref(raws[0], r))                  # (the numpy twin, on the identity resize)
    p = P.explicit_pipeline_params(chain, len(raws), blur=[(i % 2, 2.0) for i in range(len(raws))])       # applied and not, in one batch
    _, u8 = _check(raws, p, chain, label="blur on every other image")
    assert np.array_equal(u8[0], raws[0]) and not np.array_equal(u8[1], raws[1])


@pytest.mark.parametrize("S", [32, 96, 288])
def test_hue_alone(S):
    """The byte shifts 0, 1, 128, 255 (the last from a negative hue factor) and -0.3; brightness, contrast and saturation at 1 are exact
    identities, so the hue is the one op that changes bytes.  Shift 0 still makes the round trip through HSV."""
    from simseg_amd import pipeline as P
    chain = _chain(["resize", "color_distortion"], S)
    raws = [_noise(S, 3), _border(S)] + _edge_images(S) + _raws()[:3]
    for hue, shift in ((0.0, 0), (0.004, 1), (0.502, 128), (-0.004, 255), (-0.3, 180)):
        assert P.hue_shift(hue) == shift
        p = P.explicit_pipeline_params(chain, len(raws), distort=(1, (3, 0, 1, 2), 1.0, 1.0, 1.0, hue, 0))
        assert [op for op, _ in P.op_chain(chain, p, 0)][0] == P.OP_HUE
        _, u8 = _check(raws, p, chain, label=f"hue {hue}")
        assert np.array_equal(u8[0], P.hue_ref(raws[0], shift))
        assert shift or not np.array_equal(u8[0], raws[0])                              # the round trip is lossy


@pytest.mark.parametrize("shift, hue", [(0, 0.0), (77, 0.302)])
def test_hue_on_all_colours(shift, hue):
    """All 2^24 colours as 114 raw 384 x 384 images through [center_crop] at 384 + the hue shift, in batches of 16."""
    from simseg_amd import pipeline as P
    assert P.hue_shift(hue) == shift
    S = 384
    c = np.arange(114 * S * S, dtype=np.uint32) & 0xFFFFFF
    rgb = np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=-1).astype(np.uint8).reshape(114, S, S, 3)
    chain = _chain(["center_crop", "color_distortion"], S)
    for k in range(0, 114, 16):
        raws = list(rgb[k:k + 16])
        p = P.explicit_pipeline_params(chain, len(raws), distort=(1, (3, 0, 1, 2), 1.0, 1.0, 1.0, hue, 0))
        _check(raws, p, chain, label=f"colours {k * S * S} ..")


@pytest.mark.parametrize("S", [32, 96, 288])
def test_grayscale_alone(S):
    from simseg_amd import pipeline as P
    chain = _chain(["resize", "color_distortion"], S)
    raws = [_noise(S, 4)] + _edge_images(S) + _raws()[:3]
    p = P.explicit_pipeline_params(chain, len(raws), distort=(0, (0, 1, 2, 3), 0.5, 0.5, 0.5, 0.1, 1))
    assert [op for op, _ in P.op_chain(chain, p, 0)] == [P.OP_GRAY]
    _, u8 = _check(raws, p, chain, label="grayscale")
    assert (u8[0][..., 0] == u8[0][..., 1]).all() and (u8[0][..., 0] == u8[0][..., 2]).all()


@pytest.mark.parametrize("gray", [0, 1])
def test_all_24_distortion_orders(gray):
    from simseg_amd import pipeline as P
    S = 96
    chain = _chain(["resize", "color_distortion"], S)
    base = [_synth(120, 90, 5)] + _edge_images(S)[:2]
    orders = list(itertools.permutations(range(4)))
    assert len(orders) == 24
    for k in range(0, 24, 4):
        raws = [r for _ in orders[k:k + 4] for r in base]
        d = [(1, o, 0.73, 1.31, 0.64, 0.17, gray) for o in orders[k:k + 4] for _ in base]
        p = P.explicit_pipeline_params(chain, len(raws), distort=d)
        assert len(P.op_chain(chain, p, 0)) == 4 + gray
        _check(raws, p, chain, label=f"orders {k}..{k + 3} gray {gray}")


@pytest.mark.parametrize("S", [96, 288])
def test_full_chains(S):
    """The SimCLR list with sampled parameters, and the list with every op of the registry: 11 ops applied."""
    from simseg_amd import pipeline as P
    raws = _raws() + [_synth(33, 41, 15)]
    sizes = [r.shape[:2] for r in raws]
    chain = _chain(SIMCLR, S, blur={"p": 0.7, "radius_max": 3.0})
    for seed in (1, 2):
        p = P.sample_pipeline_params(sizes, np.random.default_rng(seed), chain)
        _check(raws, p, chain, label=f"SimCLR seed {seed}")
    chain = _chain(ALL11, S, blur={"radius_max": 4.0})
    for j, aa in enumerate([("sharpness", 0.7, 1, "rotate", 30.0, 1), ("shearX", 1 / 6, -1, "equalize", 0, 1)]):
        order = list(itertools.permutations(range(4)))[7 * j + 2]
        p = P.explicit_pipeline_params(chain, len(raws), aa=aa, jitter=(order, 0.8, 1.25, 0.45), blur=(1, (1.3, 3.7)[j]),
                                       distort=(1, order[::-1], 1.2, 0.7, 1.4, (-0.13, 0.21)[j], 1 - j))
        assert len(P.op_chain(chain, p, 0)) == 11 - j and P.plan_pipeline(sizes, p, chain, "cpu")["img_tab_host"][0, P.T_NOPS] == 11 - j
        _check(raws, p, chain, label=f"11 ops {aa[0]}+{aa[3]}")


@pytest.mark.parametrize("S", [96, 288])
def test_full_chain_with_pixel_erasing(S):
    """The SimCLR list + random erasing, mode pixel: the bytes and everything outside the boxes are the oracle's exactly; inside, the
    noise is erase_noise_ref's within 1e-5 (test_gpu_train_pipeline states why)."""
    from simseg_amd import pipeline as P
    extra = ["transforms.random_erasing.reprob=1.0", "transforms.random_erasing.remode=pixel", "transforms.random_erasing.recount=3"]
    chain = _chain(SIMCLR, S, extra, blur={"p": 1.0})
    raws = _raws()
    p = P.sample_pipeline_params([r.shape[:2] for r in raws], np.random.default_rng(4), chain)
    assert p["erase_n"].sum() > 0 and p["blur_apply"].all()
    f32, u8 = _run(raws, p, chain)
    for i, r in enumerate(raws):
        want_f, want_u = P.apply_pipeline_pil(Image.fromarray(r), p, i, chain)
        inside = torch.zeros(S, S, dtype=torch.bool)
        for t, l, h, w in p["erase_box"][i][:int(p["erase_n"][i])]:
            inside[t:t + h, l:l + w] = True
        assert np.array_equal(u8[i], want_u) and torch.equal(f32[i][:, ~inside], want_f[:, ~inside]), i
        if inside.any():
            assert float((f32[i] - want_f)[:, inside].abs().max()) <= 1e-5, i


@pytest.mark.parametrize("names", OLD_LISTS)
def test_old_lists_are_bit_for_bit_the_old_route(names):
    from simseg.transforms import build_train_pipeline, build_train_views
    S = 96
    extra = ["transforms.random_erasing.reprob=0.5", "transforms.random_erasing.remode=pixel", "transforms.random_erasing.recount=2"]
    _, old = build_train_pipeline(_cfg(names, S, extra))
    _, new = build_train_views(_cfg(names, S, extra))
    raws = [torch.from_numpy(r) for r in _raws() if names[0] != "random_crop" or min(r.shape[:2]) >= S] * 2
    a = old(raws, np.random.default_rng(21), want_u8=True)
    b = new(raws, np.random.default_rng(21), want_u8=True)
    torch.cuda.synchronize()
    assert not a["plan"]["full"] and b["plan"]["full"] and b["plan"]["img_tab_host"].shape[1] == 144
    assert torch.equal(a["images"], b["images"]) and torch.equal(a["u8"], b["u8"])


def test_corrupted_chain_tables_are_refused():
    """Every corrupted field of the new table is refused under the new entry point's name before anything is launched."""
    from simseg_amd import ops, pipeline as P, preproc
    S = 96
    chain = _chain(ALL11, S, blur={"radius_max": 4.0})
    raws = _raws()
    p = P.explicit_pipeline_params(chain, len(raws), aa=("posterize", 4, 1, "solarize", 2, 1), jitter=((0, 1, 2, 3), 0.9, 1.1, 1.2),
                                   distort=(1, (3, 0, 1, 2), 0.8, 1.1, 0.9, 0.1, 1), blur=(1, 2.0))
    pl = P.plan_pipeline([r.shape[:2] for r in raws], p, chain, "cuda")
    lut = preproc.make_lut(chain["mean"], chain["std"]).cuda()
    src = preproc._pack([torch.from_numpy(r) for r in raws], pl, "cuda")
    out, _ = ops.train_chain(src, pl, lut)                                            # the untouched plan runs
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    row = pl["img_tab_host"][1]
    assert row[P.T_NOPS] == 11 and row[P.TC_OP + 5] == P.OP_BLUR and row[P.TC_OP + 6] == P.OP_HUE and row[P.TC_OP + 10] == P.OP_GRAY
    blur_p, hue_p = P.TC_P + 5 * 8, P.TC_P + 6 * 8
    R, ww, fw = (int(v) for v in row[blur_p:blur_p + 3])
    assert (R, ww, fw) == P.blur_weights(2.0) and R == 1
    nan_bits = int(np.array([np.nan], np.float32).view(np.int32)[0])
    for col, val, what in [(P.T_NOPS, 13, "chain"), (P.TC_OP, 15, "code"), (P.TC_OP + 10, -1, "code"), (hue_p, 256, "hue shift"),
                           (hue_p, -1, "hue shift"), (blur_p + 1, 0, "blur weights"), (blur_p + 1, ww + 1, "blur weights"),
                           (blur_p + 2, fw - 1, "blur weights"), (blur_p + 2, -1, "blur weights"), (blur_p, -1, "blur box radius"),
                           (blur_p, 8, "blur box radius"), (blur_p, 0, "blur weights"), (P.TC_P + 2 * 8, nan_bits, "blend factor"),
                           (P.T_WTOP, 10_000, "output window"), (P.T_FLIP, 2, "flip"), (P.T_NERASE, 5, "erase boxes")]:
        bad = dict(pl)
        bad["img_tab_host"] = pl["img_tab_host"].copy()
        bad["img_tab_host"][1, col] = val
        with pytest.raises(RuntimeError, match=f"train_chain.*{what}"):
            ops.train_chain(src, bad, lut)
    with pytest.raises(RuntimeError, match="train_chain.*output size"):
        ops.train_chain(src, dict(pl, size=17), lut)
    old = P.parse_chain(["resize"], _cfg(["resize"], S))
    old_pl = P.plan_pipeline([r.shape[:2] for r in raws], P.explicit_pipeline_params(old, len(raws)), old, "cuda")
    with pytest.raises(ValueError, match="144 columns"):
        ops.train_chain(src, old_pl, lut)
