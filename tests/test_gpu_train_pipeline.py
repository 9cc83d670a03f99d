"""Device-side training transforms (simseg_amd/pipeline.py, csrc/augment.hip simseg_train_transforms) against apply_pipeline_pil, Pillow's
own calls in list order: zero differing bytes in the uint8 output and torch.equal on the fp32 planes, for every case.  The erase noise
is compared with erase_noise_ref, the float64 restatement of the hash and Box-Muller, within 1e-5 (u1 has 24 bits, so the radius is at
most sqrt(48 ln 2) = 5.77; a few fp32 ulp of log, sqrt and cos and the rounding of the angle stay under 1e-5 absolute)."""
import itertools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import REPO
from test_gpu_train_augment import RAW_SIZES, _edge_images, _synth

pytestmark = pytest.mark.gpu

SIZES = RAW_SIZES + [(33, 41)]
V = 0.4                                                          # the shipped colour jitter


def _cfg(names, S, extra=()):
    """The shipped config with train_transforms = names and every size set so that the list ends at S x S."""
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    argv = [f"transforms.train_transforms=[{','.join(names)}]", f"transforms.resize.size={S}", f"transforms.resize_bicubic.size={S}",
            f"transforms.random_crop.size={S}", f"transforms.center_crop.size={S}", f"transforms.random_resize_crop.size={S}"] + list(extra)
    return update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), argv, update_clip_config)


def _chain(names, S, extra=()):
    from simseg_amd import pipeline as P
    cfg = _cfg(names, S, extra)
    return P.parse_chain(cfg.transforms.train_transforms, cfg)


def _raws(sizes=SIZES):
    return [_synth(H, W, 10 + i) for i, (H, W) in enumerate(sizes)]


def _run(raws, params, chain):
    from simseg_amd import pipeline as P
    assert len(raws) <= 16
    res = P.run_pipeline([torch.from_numpy(r) for r in raws], params, chain, want_u8=True)
    torch.cuda.synchronize()
    return res["images"].cpu(), res["u8"].cpu().numpy()


def _check(raws, params, chain, label=""):
    """Device result == apply_pipeline_pil for every image: uint8 bytes and fp32 values."""
    from simseg_amd import pipeline as P
    f32, u8 = _run(raws, params, chain)
    bad = []
    for i, r in enumerate(raws):
        want_f, want_u = P.apply_pipeline_pil(Image.fromarray(r), params, i, chain)
        nd = int((u8[i] != want_u).sum())
        if nd or not torch.equal(f32[i], want_f):
            bad.append((i, r.shape[:2], nd, float((f32[i] - want_f).abs().max())))
    print(f"{label} {chain['names']} S={chain['size']}: {len(raws)} images, {len(bad)} differ", bad[:8])
    assert not bad, f"{label} {chain['names']}: images differ (index, raw extent, differing bytes, max fp32 error): {bad[:8]}"
    return f32, u8


def _extent_before_crop(chain, H, W):
    """The extent a trailing random_crop of [.., random_crop] sees (lists of these tests: an optional resize_bicubic before it)."""
    from simseg_amd import pipeline as P
    if chain["geom"][0][0] == "resize_bicubic":
        return P.short_side(H, W, chain["geom"][0][1])
    return H, W


@pytest.mark.parametrize("S", [32, 96, 224, 288])
def test_random_crop_alone(S):
    """random_crop at the corner, at the far corner and at full extent, with and without a resample before it."""
    from simseg_amd import pipeline as P
    for names in (["random_crop"], ["resize_bicubic", "random_crop"]):
        chain = _chain(names, S)
        sizes = [hw for hw in SIZES if names[0] != "random_crop" or min(hw) >= S] + [(S, S)]            # (S, S): the crop is the whole extent
        raws = _raws(sizes)
        ext = [_extent_before_crop(chain, H, W) for H, W in sizes]
        assert ext[-1] == (S, S)
        for where in ("corner", "far corner", "inside"):
            tl = [[(0, 0)] if where == "corner" else [(h - S, w - S)] if where == "far corner" else [((h - S) // 3, (w - S) * 2 // 3)]
                  for h, w in ext]
            _check(raws, P.explicit_pipeline_params(chain, len(raws), rcrop=tl), chain, label=where)


@pytest.mark.parametrize("S", [32, 96, 224, 288])
def test_center_crop_after_resize_bicubic(S):
    """The short side goes to S + 10 and S + 11, so the centre crop's margin is even and odd (and odd / even on the long side)."""
    from simseg_amd import pipeline as P
    raws = _raws()
    for short in (S + 10, S + 11):
        chain = _chain(["resize_bicubic", "center_crop"], S, [f"transforms.resize_bicubic.size={short}"])
        _check(raws, P.explicit_pipeline_params(chain, len(raws)), chain, label=f"short side {short}")


@pytest.mark.parametrize("S", [32, 96, 224, 288])
def test_flip_positions(S):
    """A flip before and after the resample, before and after a post-resample crop and a pre-resample box, with off-centre boxes (drawn,
    then the flip forced on and off)."""
    from simseg_amd import pipeline as P
    raws = _raws()
    sizes = [r.shape[:2] for r in raws]
    big = [f"transforms.resize_bicubic.size={S + 13}"]
    for names, extra in ((["random_flip", "resize_bicubic", "random_crop"], big), (["resize_bicubic", "random_flip", "random_crop"], big),
                         (["resize_bicubic", "random_crop", "random_flip"], big), (["random_flip", "random_resize_crop"], ()),
                         (["random_resize_crop", "random_flip"], ()), (["random_flip", "resize"], ()), (["resize", "random_flip"], ()),
                         (["random_resize_crop", "random_flip", "random_crop"], [f"transforms.random_resize_crop.size={S + 7}"])):
        chain = _chain(names, S, extra)
        p = P.sample_pipeline_params(sizes, np.random.default_rng(S), chain)
        for flip in (1, 0):
            p["flip"][:] = flip
            _check(raws, p, chain, label=f"flip={flip}")
    # no resample at all: launch 1 copies the (mirrored) box
    chain = _chain(["random_crop", "random_flip"], S)
    keep = [r for r in raws if min(r.shape[:2]) >= S] + [_synth(S, S, 3)]
    p = P.sample_pipeline_params([r.shape[:2] for r in keep], np.random.default_rng(1), chain)
    p["flip"][:] = 1
    _check(keep, p, chain, label="copy + flip")


@pytest.mark.parametrize("S", [32, 96, 224, 288])
def test_each_jitter_op_alone(S):
    """Brightness, contrast and saturation, each alone (the two other factors are 1, an exact identity) at f in {0, 1 - v, 1, 1 + v} and
    one irrational-looking f, on resized raw images and the edge images."""
    from simseg_amd import pipeline as P
    chain = _chain(["resize", "color_jitter"], S)
    raws = _raws() + _edge_images(S)
    for which in range(3):
        for f in (0.0, 1 - V, 1.0, 1 + V, 0.7368421052631579):
            fac = [1.0, 1.0, 1.0]
            fac[which] = f
            _check(raws, P.explicit_pipeline_params(chain, len(raws), jitter=((0, 1, 2, 3), *fac)), chain,
                   label=f"{('brightness', 'contrast', 'saturation')[which]} f={f}")


def test_all_24_jitter_orders():
    from simseg_amd import pipeline as P
    S = 96
    chain = _chain(["resize", "color_jitter"], S)
    base = [_synth(120, 90, 5)] + _edge_images(S)[:2]
    orders = list(itertools.permutations(range(4)))
    assert len(orders) == 24
    for k in range(0, 24, 4):
        raws = [r for _ in orders[k:k + 4] for r in base]
        jit = [(o, 0.73, 1.31, 0.64) for o in orders[k:k + 4] for _ in base]
        _check(raws, P.explicit_pipeline_params(chain, len(raws), jitter=jit), chain, label=f"orders {k}..{k + 3}")


@pytest.mark.parametrize("S", [224, 288])
def test_chains(S):
    """The CLIP-style list with sampled parameters; AutoAugment ops that read neighbours after and before the jitter, all five ops
    applied, in LDS (S = 224) and in global memory (S = 288, where every gather swaps the two slots)."""
    from simseg_amd import pipeline as P
    raws = _raws()
    sizes = [r.shape[:2] for r in raws]
    chain = _chain(["resize_bicubic", "random_crop", "random_flip", "color_jitter"], S)
    for seed in (1, 2):
        _check(raws, P.sample_pipeline_params(sizes, np.random.default_rng(seed), chain), chain, label=f"sampled seed {seed}")
    combos = [("sharpness", 0.7, 1, "rotate", 30.0, 1), ("shearX", 1 / 6, -1, "sharpness", 0.5, -1), ("rotate", 20.0, 1, "shearX", 0.3, 1),
              ("equalize", 0, 1, "contrast", 0.8, -1)]
    for names in (["resize", "random_flip", "autoaug", "color_jitter"], ["resize", "random_flip", "color_jitter", "autoaug"]):
        chain = _chain(names, S)
        for j, aa in enumerate(combos):
            order = list(itertools.permutations(range(4)))[5 * j + 1]
            p = P.explicit_pipeline_params(chain, len(raws), flip=[i % 2 for i in range(len(raws))], aa=aa, jitter=(order, 0.8, 1.25, 0.45))
            assert len(P.op_chain(chain, p, 0)) == 5
            _check(raws, p, chain, label=f"{aa[0]}+{aa[3]} order {order}")


def _erase_cases(S):
    """Per image a list of boxes: none, one (count 1), two that overlap, one that touches the far border, four (count 4, one touching
    the near border, two overlapping)."""
    q = S // 4
    return [[], [(q, q + 1, q, q + 3)], [(2, 3, 2 * q, 2 * q), (q, q, 2 * q, q + 5)], [(S - q, S - q - 2, q, q + 2)],
            [(0, 0, q, q), (q // 2, q // 2, q, q), (3 * q - 1, 1, 5, S - 1), (1, 3 * q, S - 1, 7)], [(S // 2, 0, 1, 1)]]


@pytest.mark.parametrize("S", [96, 224])
def test_erasing_const_is_exact(S):
    from simseg_amd import pipeline as P
    chain = _chain(["resize", "random_flip", "color_jitter"], S, ["transforms.random_erasing.reprob=0.5", "transforms.random_erasing.remode=const",
                                                                  "transforms.random_erasing.recount=4"])
    raws = _raws()
    p = P.explicit_pipeline_params(chain, len(raws), jitter=((2, 0, 3, 1), 0.9, 1.2, 0.7), erase=_erase_cases(S))
    assert list(p["erase_n"]) == [0, 1, 2, 1, 4, 1]
    f32, _ = _check(raws, p, chain, label="const")
    assert (f32[4][:, :S // 4, :S // 4] == 0).all() and (f32[0] != 0).any()


@pytest.mark.parametrize("mode", ["rand", "pixel"])
@pytest.mark.parametrize("S", [96, 224])
def test_erasing_noise(S, mode):
    """Outside the boxes: the un-erased output, exactly.  Inside: |device - erase_noise_ref| <= 1e-5, the last box that holds a pixel
    wins.  The same seed gives the same planes, another seed does not."""
    from simseg_amd import pipeline as P
    chain = _chain(["resize", "color_jitter"], S, ["transforms.random_erasing.reprob=0.5", f"transforms.random_erasing.remode={mode}",
                                                   "transforms.random_erasing.recount=4"])
    raws = _raws()
    boxes = _erase_cases(S)
    seed = 0x9E3779B97F4A7C15
    p = P.explicit_pipeline_params(chain, len(raws), jitter=((0, 1, 2, 3), 1.1, 0.9, 1.2), erase=boxes, seed=seed)
    plain = P.explicit_pipeline_params(chain, len(raws), jitter=((0, 1, 2, 3), 1.1, 0.9, 1.2))
    base, base_u8 = _check(raws, plain, chain, label="un-erased")                  # the un-erased output is the oracle's
    got, got_u8 = _run(raws, p, chain)
    assert np.array_equal(got_u8, base_u8)                                         # u8: the bytes before normalisation and erasing
    worst = 0.0
    for i, bx in enumerate(boxes):
        want = base[i].double()
        inside = torch.zeros(S, S, dtype=torch.bool)
        for k, (t, l, h, w) in enumerate(bx):
            want[:, t:t + h, l:l + w] = torch.from_numpy(P.erase_noise_ref(seed, i, k, (t, l, h, w), mode))
            inside[t:t + h, l:l + w] = True
        assert torch.equal(got[i][:, ~inside], base[i][:, ~inside]), f"image {i}: pixels outside the boxes changed"
        if bx:
            err = float((got[i].double() - want)[:, inside].abs().max())
            worst = max(worst, err)
            assert err <= 1e-5, f"image {i}: noise differs from erase_noise_ref by {err}"
            if mode == "rand":                                                      # one value per (box, channel)
                t, l, h, w = bx[-1]
                assert (got[i][:, t:t + h, l:l + w] == got[i][:, t:t + 1, l:l + 1]).all()
    print(f"{mode} S={S}: worst |device - erase_noise_ref| = {worst:.3e}")
    again, _ = _run(raws, p, chain)
    assert torch.equal(again, got)
    other, _ = _run(raws, P.explicit_pipeline_params(chain, len(raws), jitter=((0, 1, 2, 3), 1.1, 0.9, 1.2), erase=boxes, seed=seed + 1), chain)
    assert not torch.equal(other, got)
    assert torch.equal(other[0], got[0])                                           # (image 0 has no box)


def test_interchangeable_with_train_augment_on_shipped_config():
    from simseg.transforms import build_train_augmentation, build_train_pipeline
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"), [], update_clip_config)
    _, aug = build_train_augmentation(cfg)
    _, pipe = build_train_pipeline(cfg)
    raws = [torch.from_numpy(r) for r in _raws()] * 2
    a = aug(raws, np.random.default_rng(77), want_u8=True)
    b = pipe(raws, np.random.default_rng(77), want_u8=True)
    torch.cuda.synchronize()
    assert torch.equal(a["images"], b["images"]) and torch.equal(a["u8"], b["u8"])
    assert (a["params"]["apply1"] | a["params"]["apply2"]).any()


def test_build_train_pipeline_end_to_end():
    """From a config with overrides and PIL images through host_op to the device batch: equal to the oracle."""
    from simseg.transforms import build_train_pipeline
    from simseg_amd import pipeline as P
    cfg = _cfg(["resize_bicubic", "random_crop", "random_flip", "color_jitter", "autoaug"], 96,
               ["transforms.resize_bicubic.size=110", "transforms.color_jitter=0.3", "transforms.random_erasing.reprob=0.6",
                "transforms.random_erasing.remode=const", "transforms.random_erasing.recount=3"])
    host_op, pipe = build_train_pipeline(cfg)
    assert isinstance(pipe, P.TrainPipeline) and pipe.size == 96
    pil = [Image.fromarray(r) for r in _raws()] * 2
    res = pipe([host_op(im) for im in pil], np.random.default_rng(5), want_u8=True)
    torch.cuda.synchronize()
    p = res["params"]
    assert 0 < p["erase_n"].sum() and 0 < p["flip"].sum() < len(pil)
    for i, im in enumerate(pil):
        want_f, want_u = P.apply_pipeline_pil(im, p, i, pipe.chain)
        assert np.array_equal(res["u8"][i].cpu().numpy(), want_u) and torch.equal(res["images"][i].cpu(), want_f), i


def test_corrupted_tables_are_refused():
    """Every corrupted field of the host table is refused under the entry point's name before anything is launched."""
    from simseg_amd import ops, pipeline as P, preproc
    S = 96
    chain = _chain(["resize_bicubic", "center_crop", "color_jitter"], S, ["transforms.resize_bicubic.size=100", "transforms.random_erasing.reprob=1.0",
                                                                          "transforms.random_erasing.remode=pixel", "transforms.random_erasing.recount=2"])
    raws = _raws()
    p = P.explicit_pipeline_params(chain, len(raws), jitter=((0, 1, 2, 3), 0.9, 1.1, 1.2), erase=[(1, 2, 30, 40), (50, 50, 46, 46)], seed=9)
    pl = P.plan_pipeline([r.shape[:2] for r in raws], p, chain, "cuda")
    lut = preproc.make_lut(chain["mean"], chain["std"]).cuda()
    src = preproc._pack([torch.from_numpy(r) for r in raws], pl, "cuda")
    out, _ = ops.train_transforms(src, pl, lut)                                       # the untouched plan runs
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert pl["img_tab_host"][1, P.T_OP] == P.OP_BRIGHTNESS and pl["img_tab_host"][1, P.T_NOPS] == 3
    nan_bits = int(np.array([np.nan], np.float32).view(np.int32)[0])
    inf_bits = int(np.array([np.inf], np.float32).view(np.int32)[0])
    for col, val, what in [(P.T_WTOP, 10_000, "output window"), (P.T_WLEFT, -1, "output window"), (P.T_RW, S - 1, "output window"),
                           (P.T_NOPS, 6, "chain"), (P.T_OP, 99, "code"), (P.T_OP + 2, -1, "code"), (P.T_BOX + 2, S, "erase box"),
                           (P.T_BOX + 5, S - 45, "erase box"), (P.T_NERASE, 5, "erase boxes"), (P.T_MODE, 3, "erase mode"),
                           (P.T_P, nan_bits, "blend factor"), (P.T_P + 8, inf_bits, "blend factor"), (P.T_FLIP, 2, "flip"),
                           (P.T_TOP, 10_000, "crop box"), (P.T_SRC, 1 << 40, "source offset"), (P.T_HOFF, -5, "axis table")]:
        bad = dict(pl)
        bad["img_tab_host"] = pl["img_tab_host"].copy()
        bad["img_tab_host"][1, col] = val
        with pytest.raises(RuntimeError, match=f"train_transforms.*{what}"):
            ops.train_transforms(src, bad, lut)
    with pytest.raises(RuntimeError, match="train_transforms.*output size"):
        ops.train_transforms(src, dict(pl, size=17), lut)
