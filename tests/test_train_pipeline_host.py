"""Host side of the training transforms (simseg_amd/pipeline.py): the grammar, the sampling law, the facts about Pillow that the device
route rests on (flip and resize commute; brightness is a truncated float32 product), the oracle, the plan and the C header.  No GPU
needed: plans are built for the CPU device, where the axis arena lives on the host."""
import itertools
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from conftest import REPO

SHIPPED = ["random_resize_crop", "autoaug"]
CLIP = ["resize_bicubic", "random_crop", "random_flip", "color_jitter"]
SIZES = [(375, 500), (500, 333), (224, 224), (300, 1203), (250, 600), (1200, 240)]


def _cfg(names=None, extra=(), path="configs/clip/simseg.vit-b.yaml"):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    argv = ([] if names is None else [f"transforms.train_transforms=[{','.join(names)}]"]) + list(extra)
    return update_cfg(task_cfg_init_fn, os.path.join(REPO, path), argv, update_clip_config)


def _chain(names=None, extra=()):
    from simseg_amd import pipeline as P
    cfg = _cfg(names, extra)
    return P.parse_chain(cfg.transforms.train_transforms, cfg)


@pytest.mark.parametrize("names", [SHIPPED, CLIP, ["random_crop", "random_flip"], ["resize", "random_flip", "autoaug", "color_jitter"],
                                   ["random_flip", "random_resize_crop"], ["resize_bicubic", "center_crop", "color_jitter", "autoaug"]])
def test_grammar_accepts(names):
    from simseg.transforms import build_train_pipeline
    from simseg_amd import pipeline as P
    host_op, pipe = build_train_pipeline(_cfg(names, ["transforms.resize.size=224"]))
    assert isinstance(pipe, P.TrainPipeline) and pipe.size == 224 and pipe.chain["names"] == names
    assert pipe.chain["colour"] == [n for n in names if n in P.COLOUR] and pipe.chain["erase"] is None
    assert pipe.chain["lut"].shape == (3, 256) and torch.equal(pipe.chain["lut"], P.preproc.make_lut(pipe.chain["mean"], pipe.chain["std"]))
    a = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    assert np.array_equal(host_op(Image.fromarray(a)).numpy(), a)


@pytest.mark.parametrize("names, rule", [(["resize", "random_resize_crop"], "at most one resample"),
                                         (["resize_bicubic", "resize"], "at most one resample"),
                                         (["resize", "color_jitter", "random_flip"], "geometry\\+ colour\\*"),
                                         (["autoaug", "resize"], "geometry\\+ colour\\*"),
                                         (["resize_bicubic"], "final extent"), (["resize_bicubic", "random_flip"], "final extent"),
                                         (["autoaug"], "geometry\\+ colour\\*"), (["random_flip"], "final extent"),
                                         (["random_flip", "resize", "random_flip"], "random_flip at most once"),
                                         (["resize", "color_jitter", "autoaug", "color_jitter"], "color_jitter at most once"),
                                         (["resize", "autoaug", "autoaug"], "autoaug at most once"),
                                         (["resize", "gaussian_blur"], "geometry \\| colour")])
def test_grammar_refuses_naming_the_rule(names, rule):
    from simseg.transforms import build_train_pipeline
    with pytest.raises(NotImplementedError, match=rule):
        build_train_pipeline(_cfg(names))


def test_grammar_sizes_and_erasing_config():
    from simseg_amd import pipeline as P
    with pytest.raises(NotImplementedError, match="final extent"):
        _chain(["resize"], ["transforms.resize.size=31"])
    with pytest.raises(NotImplementedError, match="final extent"):
        _chain(["resize_bicubic", "random_crop"], ["transforms.random_crop.size=385"])
    assert _chain(["resize"], ["transforms.resize.size=32"])["size"] == 32 and _chain(["resize"], ["transforms.resize.size=384"])["size"] == 384
    with pytest.raises(ValueError, match="recount"):
        _chain(CLIP, ["transforms.random_erasing.reprob=0.25", "transforms.random_erasing.recount=5"])
    with pytest.raises(ValueError, match="recount"):
        _chain(CLIP, ["transforms.random_erasing.reprob=0.25", "transforms.random_erasing.recount=0"])
    with pytest.raises(NotImplementedError, match="remode"):
        _chain(CLIP, ["transforms.random_erasing.reprob=0.25", "transforms.random_erasing.remode=noise"])
    assert _chain(CLIP, ["transforms.random_erasing.recount=5"])["erase"] is None                 # reprob = 0: erasing is off, nothing to refuse
    for mode in P.ERASE_MODES:
        er = _chain(CLIP, ["transforms.random_erasing.reprob=0.25", f"transforms.random_erasing.remode={mode}", "transforms.random_erasing.recount=4"])["erase"]
        assert er == {"reprob": 0.25, "mode": mode, "recount": 4}


@pytest.mark.parametrize("path", ["configs/clip/simseg.vit-b.yaml", "configs/clip/simseg.vit-s.yaml"])
def test_pinned_refusals_of_the_other_builders(path):
    """The four lists tests/test_train_augment_host.py expects build_train_augmentation to refuse are still refused by it, and
    build_transforms / build_device_transforms still refuse the training lists."""
    from simseg.transforms import build_device_transforms, build_train_augmentation, build_transforms
    for names in (["autoaug"], ["random_resize_crop", "autoaug", "resize"], ["resize"], ["autoaug", "random_resize_crop"]):
        with pytest.raises(NotImplementedError):
            build_train_augmentation(_cfg(names, path=path))
    for names in (None, CLIP):
        with pytest.raises(NotImplementedError):
            build_transforms(_cfg(names, path=path), "train")
        with pytest.raises(NotImplementedError):
            build_device_transforms(_cfg(names, path=path), "train")


def test_sampling_of_the_shipped_list_is_sample_params():
    from simseg_amd import augment as A, pipeline as P
    chain = _chain()
    assert chain["names"] == SHIPPED and chain["scale"] == (0.6, 1.0)
    sizes = [(375, 500), (500, 333), (224, 224), (97, 1203), (8, 600), (1200, 40)] * 20
    a = A.sample_params(sizes, np.random.default_rng(11))
    b = P.sample_pipeline_params(sizes, np.random.default_rng(11), chain)
    for f in A.FIELDS:
        assert np.array_equal(a[f], b[f]), f
    assert not b["flip"].any() and not b["erase_n"].any() and b["seed"] == 0


@pytest.fixture(scope="module")
def draws():
    from simseg_amd import pipeline as P
    chain = _chain(CLIP + ["autoaug"], ["transforms.random_erasing.reprob=0.25", "transforms.random_erasing.remode=pixel",
                                        "transforms.random_erasing.recount=4"])
    sizes = [SIZES[i % len(SIZES)] for i in range(20000)]
    return chain, sizes, P.sample_pipeline_params(sizes, np.random.default_rng(2025), chain)


def test_sampling_law(draws):
    from simseg_amd import pipeline as P
    chain, sizes, p = draws
    n, S, v = len(sizes), chain["size"], chain["jitter"]
    assert (S, v) == (224, 0.4)
    se = math.sqrt(0.25 / n)
    assert abs(p["flip"].mean() - 0.5) <= 5 * se, p["flip"].mean()
    rate = (p["erase_n"] > 0).mean()                 # (a drawn erase keeps at least one box unless all ten tries of every box fail)
    assert abs(rate - 0.25) <= 5 * math.sqrt(0.25 * 0.75 / n), rate
    for f in ("jb", "jc", "js"):
        assert (p[f] >= 1 - v).all() and (p[f] <= 1 + v).all() and p[f].std() > 0.2
    assert {tuple(o) for o in p["order"]} == set(itertools.permutations(range(4)))
    assert set(np.unique(p["erase_n"])) == {0, 1, 2, 3, 4}
    for k in range(P.MAX_ERASE):
        sel = p["erase_n"] > k
        t, l, h, w = (p["erase_box"][sel, k, j] for j in range(4))
        assert (h > 0).all() and (w > 0).all() and (h < S).all() and (w < S).all()
        assert (t >= 0).all() and (l >= 0).all() and (t + h <= S).all() and (l + w <= S).all()
        assert (p["erase_box"][~sel, k] == 0).all()
    # the random crop: inside the resized extent, and uniform enough to reach both ends of the long side
    for i in (0, 1):
        rh, rw = P.short_side(*sizes[i], 224)
        sel = np.arange(i, n, len(SIZES))
        assert (rh, rw) == ((224, 299), (336, 224))[i]
        assert (p["rcrop"][sel, 0, 0].min(), p["rcrop"][sel, 0, 0].max()) == (0, rh - 224)
        assert (p["rcrop"][sel, 0, 1].min(), p["rcrop"][sel, 0, 1].max()) == (0, rw - 224)
    assert p["seed"] != 0 and p["policy"].min() == 0 and p["policy"].max() == 24
    q = P.sample_pipeline_params(sizes[:600], np.random.default_rng(2025), chain)
    r = P.sample_pipeline_params(sizes[:600], np.random.default_rng(2026), chain)
    assert all(np.array_equal(q[f], p[f][:600]) for f in P.FIELDS)              # the same state, the same per-image draws
    assert not all(np.array_equal(q[f], r[f]) for f in P.FIELDS) and q["seed"] != r["seed"]
    q2 = P.sample_pipeline_params(sizes[:600], np.random.default_rng(2025), chain)
    assert q2["seed"] == q["seed"]


def test_flip_and_resize_commute_in_this_pillow():
    """What lets a flip be a mirrored column index in launch 1: over 240 random extents and both filters, resize then FLIP_LEFT_RIGHT
    equals FLIP_LEFT_RIGHT then resize, byte for byte."""
    rng = np.random.default_rng(8)
    bad = []
    for k in range(240):
        H, W, oh, ow = (int(v) for v in rng.integers(1, 90, 4))
        if k % 4 == 0:
            oh, ow = H + int(rng.integers(0, 3)), W                                     # (one axis unchanged: the pass Pillow skips)
        img = Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        for filt in (Image.BILINEAR, Image.BICUBIC):
            a = np.asarray(img.resize((ow, oh), filt).transpose(Image.FLIP_LEFT_RIGHT))
            b = np.asarray(img.transpose(Image.FLIP_LEFT_RIGHT).resize((ow, oh), filt))
            if not np.array_equal(a, b):
                bad.append((H, W, oh, ow, filt))
    assert not bad, bad[:8]


def test_brightness_is_a_truncated_float32_product():
    """ImageEnhance.Brightness(img).enhance(f) == clamp(trunc(float32(f) * v)): the kernel's ag_blend(0, v, f)."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)
    a[0, :, 0] = np.arange(48) * 5
    a.reshape(-1)[:256] = np.arange(256)
    for f in (0.0, 0.6, 1.0, 1.4):
        got = np.asarray(ImageEnhance.Brightness(Image.fromarray(a)).enhance(f))
        prod = (np.float32(0.0) + np.float32(f) * a.astype(np.float32)).astype(np.float32)       # float32 deg + f * (im - deg), deg = 0
        want = np.clip(np.trunc(prod), 0, 255).astype(np.uint8)
        assert np.array_equal(got, want), f


def test_oracle_on_the_shipped_list_is_apply_pil():
    from simseg_amd import augment as A, pipeline as P
    chain = _chain()
    rng = np.random.default_rng(4)
    raws = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in [(120, 160), (97, 203), (8, 600), (224, 224)]] * 3
    p = P.sample_pipeline_params([r.shape[:2] for r in raws], np.random.default_rng(21), chain)
    assert (p["apply1"] | p["apply2"]).any()
    for i, r in enumerate(raws):
        wf, wu = A.apply_pil(Image.fromarray(r), p, i, 224, chain["mean"], chain["std"])
        gf, gu = P.apply_pipeline_pil(Image.fromarray(r), p, i, chain)
        assert np.array_equal(gu, wu) and torch.equal(gf, wf), i


def test_folded_geometry_is_pillows_calls_in_list_order():
    """The fold (one source box, one resample, one window, one flip flag), evaluated with resample_ref on the host, equals Pillow's calls
    in list order for lists with crops and flips on both sides of the resample."""
    from simseg_amd import pipeline as P, preproc
    rng = np.random.default_rng(6)
    sizes = [(150, 200), (200, 133), (97, 203), (100, 100), (81, 80)]
    extra = ["transforms.random_crop.size=60", "transforms.center_crop.size=48", "transforms.resize_bicubic.size=80", "transforms.resize.size=64",
             "transforms.random_resize_crop.size=72"]
    for names in (["resize_bicubic", "random_crop", "random_flip"], ["random_crop", "random_flip"], ["random_flip", "random_resize_crop"],
                  ["center_crop", "random_flip", "resize_bicubic", "random_crop", "center_crop"],
                  ["random_resize_crop", "random_crop", "random_flip", "center_crop"], ["random_crop", "random_flip", "random_crop", "resize"]):
        chain = _chain(names, extra)
        S = chain["size"]
        for _ in range(3):
            p = P.sample_pipeline_params(sizes, rng, chain)
            pl = P.plan_pipeline(sizes, p, chain, "cpu")
            for i, (H, W) in enumerate(sizes):
                raw = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                g = pl["geometry"][i]
                t, l, h, w = g["box"]
                r = preproc.resample_ref(np.ascontiguousarray(raw[t:t + h, l:l + w]), (g["RH"], g["RW"]), g["filter"])
                r = r[g["wtop"]:g["wtop"] + S, g["wleft"]:g["wleft"] + S]
                if g["flip"]:
                    r = r[:, ::-1]
                assert np.array_equal(r, np.asarray(P.apply_pipeline_pil_u8(Image.fromarray(raw), p, i, chain))), (names, i)


def test_plan_rows_tables_and_refusals():
    from simseg_amd import augment as A, pipeline as P, preproc
    chain = _chain(["resize_bicubic", "random_crop"])
    sizes = [(375, 500), (500, 333), (97, 1203)]
    p = P.explicit_pipeline_params(chain, 3, rcrop=[[(0, 10)], [(100, 0)], [(0, 2554)]])
    pl = P.plan_pipeline(sizes, p, chain, "cpu")
    it = pl["img_tab_host"]
    assert it.shape == (3, P.TT_COLS) and it.dtype == np.int64 and np.array_equal(pl["img_tab"].numpy(), it)
    # the same axis-table entries as preproc's plan of the same resize
    pp = preproc.plan(sizes, preproc.make_spec("short", 224, "bicubic"), "cpu")
    assert pp["tab_host"] is pl["tab_host"]
    assert np.array_equal(it[:, P.T_HOFF:P.T_VKS + 1], pp["img_tab_host"][:, 8:12]) and np.array_equal(it[:, P.T_RH:P.T_RW + 1], pp["img_tab_host"][:, 12:14])
    assert [list(r) for r in it[:, P.T_TOP:P.T_CW + 1]] == [[0, 0, 375, 500], [0, 0, 500, 333], [0, 0, 97, 1203]]
    assert [list(r) for r in it[:, P.T_WTOP:P.T_FLIP + 1]] == [[0, 10, 0], [100, 0, 0], [0, 2554, 0]] and (it[:, P.T_NOPS:] == 0).all()
    assert list(it[:, P.T_SRC]) == pl["src_off"] == [0, 375 * 500 * 3, 375 * 500 * 3 + 500 * 333 * 3]
    # a crop outside the current extent: ValueError at plan time (and when it is drawn)
    with pytest.raises(ValueError, match="random_crop"):
        P.plan_pipeline(sizes, P.explicit_pipeline_params(chain, 3, rcrop=[(0, 76)]), chain, "cpu")         # image 0 is 299 wide there: left <= 75
    with pytest.raises(ValueError, match="random_crop"):
        P.plan_pipeline(sizes, P.explicit_pipeline_params(chain, 3, rcrop=[(-1, 0)]), chain, "cpu")
    small = _chain(["random_crop", "random_flip"])
    with pytest.raises(ValueError, match="random_crop"):
        P.sample_pipeline_params([(300, 200)], np.random.default_rng(0), small)
    with pytest.raises(ValueError, match="center_crop"):
        P.plan_pipeline([(300, 200)], P.explicit_pipeline_params(_chain(["center_crop"]), 1), _chain(["center_crop"]), "cpu")
    with pytest.raises(ValueError, match="random_resize_crop"):
        P.plan_pipeline([(300, 200)], P.explicit_pipeline_params(_chain(), 1, rrc=(0, 0, 301, 10)), _chain(), "cpu")
    # a flipped pre-resample crop is mirrored inside the current extent; the op chain and the erase boxes land in their columns
    chain = _chain(["random_flip", "random_crop", "resize", "color_jitter", "autoaug"],
                   ["transforms.random_crop.size=100", "transforms.resize.size=224", "transforms.random_erasing.reprob=1.0", "transforms.random_erasing.remode=rand",
                    "transforms.random_erasing.recount=2"])
    p = P.explicit_pipeline_params(chain, 1, rcrop=[(5, 20)], flip=1, aa=("rotate", 30.0, 1, "posterize", 5, 1), jitter=((3, 2, 0, 1), 0.5, 1.5, 1.25),
                                   erase=[(1, 2, 3, 4), (10, 20, 30, 40)], seed=2 ** 64 - 2)
    it = P.plan_pipeline([(300, 500)], p, chain, "cpu")["img_tab_host"][0]
    assert list(it[P.T_TOP:P.T_CW + 1]) == [5, 500 - 20 - 100, 100, 100] and list(it[P.T_RH:P.T_NERASE + 1]) == [224, 224, 0, 0, 1, 5, 2]
    assert it[P.T_MODE] == 1 and it[P.T_SEED] == -2 and list(it[P.T_BOX:P.T_BOX + 8]) == [1, 2, 3, 4, 10, 20, 30, 40] and (it[P.T_BOX + 8:P.T_OP] == 0).all()
    assert list(it[P.T_OP:P.T_P]) == [A.OP_CODE["color"], P.OP_BRIGHTNESS, A.OP_CODE["contrast"], A.OP_CODE["rotate"], A.OP_CODE["posterize"]]
    f = [np.int32(it[P.T_P + 8 * k]).view(np.float32) for k in range(3)]
    assert f == [np.float32(1.25), np.float32(0.5), np.float32(1.5)]
    assert list(it[P.T_P + 24:P.T_P + 32]) == A.op_slots(A.OP_CODE["rotate"], 30.0, 1, 224) and it[P.T_P + 32] == 0b11111000


def test_erase_noise_ref_is_the_stated_hash_and_transform():
    """erase_noise_ref against a scalar restatement in Python integers, and as a distribution."""
    from simseg_amd import pipeline as P

    def h32(seed, idx):
        M = 0xFFFFFFFF
        x = ((idx & M) * 0x9E3779B1 + (idx >> 32) * 0x85EBCA77 + (seed & M) + (seed >> 32) * 0xC2B2AE3D) & M
        x ^= x >> 16
        x = x * 0x21F0AAAD & M
        x ^= x >> 15
        x = x * 0x735A2D97 & M
        return x ^ (x >> 15)

    def normal(seed, i):
        u1 = ((h32(seed, 2 * i) >> 8) + 1) * 2.0 ** -24
        u2 = (h32(seed, 2 * i + 1) >> 8) * 2.0 ** -24
        return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)

    seed, b, k, box = 0xFEDCBA9876543210, 70000, 3, (5, 9, 4, 6)
    z = P.erase_noise_ref(seed, b, k, box, "pixel")
    assert z.shape == (3, 4, 6) and z.dtype == np.float64
    for c, y, x in ((0, 0, 0), (1, 2, 3), (2, 3, 5)):
        i = (((b * 4 + k) * 3 + c) << 18) + (5 + y) * 512 + 9 + x
        assert z[c, y, x] == pytest.approx(normal(seed, i), abs=1e-12)
    r = P.erase_noise_ref(seed, b, k, box, "rand")
    assert all((r[c] == r[c, 0, 0]).all() and r[c, 0, 0] == pytest.approx(normal(seed, ((b * 4 + k) * 3 + c) << 18), abs=1e-12) for c in range(3))
    assert not P.erase_noise_ref(seed, b, k, box, "const").any()
    big = P.erase_noise_ref(7, 1, 0, (0, 0, 300, 300), "pixel")
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01 and np.abs(big).max() <= math.sqrt(48 * math.log(2))
    assert abs(np.corrcoef(big[0].ravel(), big[1].ravel())[0, 1]) < 0.01 and abs(np.corrcoef(big[0, :, :-1].ravel(), big[0, :, 1:].ravel())[0, 1]) < 0.01


def test_header_declares_and_library_exports_the_entries():
    import ctypes
    from simseg_amd import lib
    protos = lib.parse_header()
    assert "simseg_train_transforms" in protos and "simseg_train_transforms_scratch_bytes" in protos
    assert [a for _, a in protos["simseg_train_transforms"][1]] == [a for _, a in protos["simseg_train_augment"][1]]
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, "simseg_train_transforms") and hasattr(so, "simseg_train_transforms_scratch_bytes")
    assert lib.raw("simseg_train_transforms_scratch_bytes", 3, 224) == 3 * 150528 and lib.raw("simseg_train_transforms_scratch_bytes", 3, 31) == 0
    assert lib.raw("simseg_train_transforms_scratch_bytes", 2, 288) == 2 * 2 * 248832
