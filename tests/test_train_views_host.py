"""Host side of the full training grammar (simseg_amd/pipeline.py parse_chain(full=True), simseg.transforms.build_train_views): the three
numpy restatements of Pillow's arithmetic (Gaussian blur, RGB -> HSV, HSV -> RGB) against Pillow's own calls with zero differences, the
grammar and its refusals, the sampling law, the 144-column table and the C header.  No GPU needed."""
import os

import numpy as np
import pytest
from PIL import Image, ImageFilter

from conftest import REPO

SIMCLR = ["random_resize_crop", "random_flip", "color_distortion", "gaussian_blur"]
ALL11 = ["resize", "autoaug", "color_jitter", "gaussian_blur", "color_distortion"]
OLD_LISTS = [["random_resize_crop", "autoaug"], ["resize_bicubic", "random_crop", "random_flip", "color_jitter"], ["random_crop", "random_flip"],
             ["resize", "random_flip", "autoaug", "color_jitter"], ["random_flip", "random_resize_crop"],
             ["resize_bicubic", "center_crop", "color_jitter", "autoaug"]]              # test_train_pipeline_host.test_grammar_accepts'
SIZES = [(375, 500), (500, 333), (224, 224), (300, 1203), (250, 600), (1200, 240)]


def _cfg(names, extra=(), distortion=None, blur=None):
    """The shipped config with train_transforms = names; distortion / blur: dicts put under transforms.color_distortion /
    transforms.gaussian_blur (the task defaults have no such keys: parse_chain then takes the registry's defaults)."""
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"),
                     [f"transforms.train_transforms=[{','.join(names)}]"] + list(extra), update_clip_config)
    for key, val in (("color_distortion", distortion), ("gaussian_blur", blur)):
        dict.pop(cfg.transforms, key, None)                                             # (update_cfg hands out one shared object)
        if val is not None:
            dict.__setitem__(cfg.transforms, key, dict(val))
    return cfg


def _chain(names, extra=(), **kw):
    from simseg_amd import pipeline as P
    cfg = _cfg(names, extra, **kw)
    return P.parse_chain(cfg.transforms.train_transforms, cfg, full=True)


# ---- the three numpy twins against Pillow ---------------------------------------------------------------------------------------------------
def _blur_cases():
    rng = np.random.default_rng(7)
    extents = [(3, 40), (40, 3), (33, 41), (64, 64), (96, 50), (224, 224)]
    radii = [0.1, 0.5, 1.0, 1.41, 1.42, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0]
    cases = [(e, r) for e in extents[:5] for r in radii + [float(v) for v in rng.uniform(0.1, 6.0, 30)]]
    return cases + [(extents[5], r) for r in (0.1, 1.0, 1.41, 1.42, 2.0, 5.0)]


def test_gaussian_blur_twin_is_pillow():
    from simseg_amd import pipeline as P
    cases = _blur_cases()
    assert len(cases) >= 200 and {1.0, 1.41, 1.42, 2.0, 5.0} <= {r for _, r in cases} and ((3, 40), 1.0) in cases
    assert P.blur_weights(1.41)[0] == 0 and P.blur_weights(1.42)[0] == 1               # l goes 0 -> 1 between them
    rng = np.random.default_rng(8)
    bad = []
    for k, ((h, w), r) in enumerate(cases):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 3 == 0:                                                                  # flat with a bright border: the clamp at the ends
            a[1:-1, 1:-1] = 40
        want = np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(r)))
        nd = int((P.gaussian_blur_ref(a, r) != want).sum())
        if nd:
            bad.append(((h, w), r, nd))
    assert not bad, f"(extent, radius, differing bytes): {bad[:8]}"


@pytest.fixture(scope="module")
def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def test_rgb_to_hsv_twin_is_pillow_on_all_colours(all_colours):
    from simseg_amd import pipeline as P
    want = np.asarray(Image.fromarray(all_colours).convert("HSV"))
    assert int((P.rgb_to_hsv_ref(all_colours) != want).any(axis=-1).sum()) == 0


def test_hsv_to_rgb_twin_is_pillow_on_all_triples(all_colours):
    from simseg_amd import pipeline as P
    want = np.asarray(Image.fromarray(all_colours, "HSV").convert("RGB"))
    assert int((P.hsv_to_rgb_ref(all_colours) != want).any(axis=-1).sum()) == 0


def test_hue_shift_and_oracle_agree_with_the_twins():
    from simseg_amd import pipeline as P
    assert [P.hue_shift(v) for v in (0.0, 0.5, -0.5, 0.3, -0.3, 0.004, -0.004, 0.0039)] == [0, 127, 129, 76, 180, 1, 255, 0]
    chain = _chain(["resize", "color_distortion"], ["transforms.resize.size=32"])
    a = np.random.default_rng(3).integers(0, 256, (32, 32, 3), dtype=np.uint8)
    for hue in (0.0, 0.31, -0.2):
        p = P.explicit_pipeline_params(chain, 1, distort=(1, (3, 0, 1, 2), 1.0, 1.0, 1.0, hue, 0))
        got = np.asarray(P.apply_pipeline_pil_u8(Image.fromarray(a), p, 0, chain))
        assert np.array_equal(got, P.hue_ref(a, P.hue_shift(hue))), hue
    p = P.explicit_pipeline_params(chain, 1, distort=(0, (0, 1, 2, 3), 0.5, 0.5, 0.5, 0.1, 1))     # jitter not applied, gray applied
    got = np.asarray(P.apply_pipeline_pil_u8(Image.fromarray(a), p, 0, chain))
    assert np.array_equal(got, np.repeat(np.asarray(Image.fromarray(a).convert("L"))[:, :, None], 3, axis=2))


# ---- the grammar ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [SIMCLR, ALL11, ["resize", "gaussian_blur"], ["random_crop", "color_distortion"],
                                   ["resize_bicubic", "center_crop", "gaussian_blur", "autoaug", "color_distortion", "color_jitter"]])
def test_full_grammar_accepts(names):
    from simseg.transforms import build_train_views
    from simseg_amd import pipeline as P
    host_op, pipe = build_train_views(_cfg(names, ["transforms.resize.size=224"]))
    ch = pipe.chain
    assert isinstance(pipe, P.TrainPipeline) and pipe.size == 224 and ch["names"] == names and ch["full"]
    assert ch["colour"] == [n for n in names if n in P.PIXEL] and P.COLOUR == ("autoaug", "color_jitter")
    assert ch["distort"] == ({"strength": 1.0} if "color_distortion" in names else None)
    assert ch["blur"] == ({"p": 0.5, "radius_min": 0.1, "radius_max": 2.0} if "gaussian_blur" in names else None)


def test_config_keys_are_read():
    ch = _chain(SIMCLR, distortion={"strength": 0.5}, blur={"p": 1.0, "radius_min": 0.3, "radius_max": 4.0})
    assert ch["distort"] == {"strength": 0.5} and ch["blur"] == {"p": 1.0, "radius_min": 0.3, "radius_max": 4.0}
    assert _chain(SIMCLR, blur={"p": 0.25})["blur"] == {"p": 0.25, "radius_min": 0.1, "radius_max": 2.0}


@pytest.mark.parametrize("names, kw, rule", [
    (["resize", "color_distortion", "random_flip"], {}, "geometry\\+ pixel\\*"),
    (["gaussian_blur"], {}, "geometry\\+ pixel\\*"),
    (["resize", "gaussian_blur", "gaussian_blur"], {}, "gaussian_blur at most once"),
    (["resize", "color_distortion", "autoaug", "color_distortion"], {}, "color_distortion at most once"),
    (["resize", "random_augment"], {}, "geometry \\| pixel"),
    (["resize", "color_distortion"], {"distortion": {"strength": 0.0}}, "strength in \\(0, 2.5\\]"),
    (["resize", "color_distortion"], {"distortion": {"strength": 2.6}}, "strength in \\(0, 2.5\\]"),
    (["resize", "gaussian_blur"], {"blur": {"p": 1.5}}, "gaussian_blur.p in \\[0, 1\\]"),
    (["resize", "gaussian_blur"], {"blur": {"p": -0.1}}, "gaussian_blur.p in \\[0, 1\\]"),
    (["resize", "gaussian_blur"], {"blur": {"radius_min": 0.0}}, "0 < radius_min <= radius_max"),
    (["resize", "gaussian_blur"], {"blur": {"radius_min": 2.5, "radius_max": 2.0}}, "0 < radius_min <= radius_max"),
    (["resize", "gaussian_blur"], {"blur": {"radius_max": 9.0}}, "box radius of radius_max is at most 7")])
def test_full_grammar_refuses_naming_the_rule(names, kw, rule):
    from simseg.transforms import build_train_views
    with pytest.raises(NotImplementedError, match=rule):
        build_train_views(_cfg(names, **kw))


def test_the_radius_cap_admits_pillow_radius_4_and_more():
    from simseg_amd import pipeline as P
    assert P.blur_weights(4.0)[0] == 3 and P.blur_weights(8.4)[0] == 7 and P.blur_weights(8.6)[0] == 8 and P.BLUR_MAX_R == 7
    assert _chain(SIMCLR, blur={"radius_max": 8.4})["blur"]["radius_max"] == 8.4
    assert _chain(SIMCLR, distortion={"strength": 2.5})["distort"]["strength"] == 2.5


def test_the_old_builder_and_the_old_grammar_still_refuse_both_names():
    from simseg.transforms import build_train_pipeline
    from simseg_amd import pipeline as P
    for names in (["resize", "gaussian_blur"], ["resize", "color_distortion"], SIMCLR):
        with pytest.raises(NotImplementedError, match="geometry \\| colour"):
            build_train_pipeline(_cfg(names))
        cfg = _cfg(names)
        with pytest.raises(NotImplementedError, match="geometry \\| colour"):
            P.parse_chain(cfg.transforms.train_transforms, cfg)


@pytest.mark.parametrize("names", OLD_LISTS)
def test_old_lists_sample_the_same_through_both_builders(names):
    from simseg.transforms import build_train_pipeline, build_train_views
    from simseg_amd import pipeline as P
    extra = ["transforms.resize.size=224", "transforms.random_erasing.reprob=0.3", "transforms.random_erasing.recount=3"]
    _, new = build_train_views(_cfg(names, extra))
    _, old = build_train_pipeline(_cfg(names, extra))
    assert new.chain["full"] and not old.chain["full"] and new.chain["names"] == old.chain["names"] == names
    sizes = [SIZES[i % len(SIZES)] for i in range(60)]
    a, b = old.sample(sizes, np.random.default_rng(31)), new.sample(sizes, np.random.default_rng(31))
    assert set(a) == set(b) and a["seed"] == b["seed"]
    for f in P.FIELDS + P.FULL_FIELDS:
        assert np.array_equal(a[f], b[f]), f
    for i in range(len(sizes)):
        assert P.op_chain(old.chain, a, i) == P.op_chain(new.chain, b, i)
    pa, pb = P.plan_pipeline(sizes, a, old.chain, "cpu"), P.plan_pipeline(sizes, b, new.chain, "cpu")
    ta, tb = pa["img_tab_host"], pb["img_tab_host"]
    assert ta.shape == (60, 81) and tb.shape == (60, 144) and not pa["full"] and pb["full"]
    assert np.array_equal(ta[:, :P.T_OP + 5], tb[:, :P.T_OP + 5]) and not tb[:, P.T_OP + 5:P.TC_P].any()
    assert np.array_equal(ta[:, P.T_P:], tb[:, P.TC_P:P.TC_P + 40]) and not tb[:, P.TC_P + 40:].any()


# ---- the sampling law -----------------------------------------------------------------------------------------------------------------------
def test_sampling_law_of_a_fixed_seed():
    """The draws of one image, restated: list order; everything is drawn whether or not it applies."""
    from simseg_amd import pipeline as P
    st = 0.5
    chain = _chain(["resize", "random_flip", "gaussian_blur", "color_distortion"], distortion={"strength": st},
                   blur={"p": 0.3, "radius_min": 0.2, "radius_max": 3.0})
    p = P.sample_pipeline_params([(100, 120)] * 3, np.random.default_rng(99), chain)
    rng = np.random.default_rng(99)
    for i in range(3):
        assert p["flip"][i] == int(rng.random() < 0.5)
        assert p["blur_apply"][i] == int(rng.random() <= 0.3) and p["blur_radius"][i] == rng.uniform(0.2, 3.0)
        assert p["d_apply"][i] == int(rng.random() <= 0.8) and list(p["d_order"][i]) == [int(j) for j in rng.permutation(4)]
        assert [p[f][i] for f in ("db", "dc", "ds")] == [rng.uniform(1 - 0.8 * st, 1 + 0.8 * st) for _ in range(3)]
        assert p["dh"][i] == rng.uniform(-0.2 * st, 0.2 * st) and p["d_gray"][i] == int(rng.random() < 0.2)
    assert p["seed"] == 0


def test_sampling_ranges_and_rates():
    from simseg_amd import pipeline as P
    n = 20000
    chain = _chain(SIMCLR, distortion={"strength": 2.0})
    p = P.sample_pipeline_params([(64, 64)] * n, np.random.default_rng(5), chain)
    for f, rate in (("d_apply", 0.8), ("d_gray", 0.2), ("blur_apply", 0.5), ("flip", 0.5)):
        assert abs(p[f].mean() - rate) <= 5 * np.sqrt(rate * (1 - rate) / n), (f, p[f].mean())
    for f in ("db", "dc", "ds"):
        assert p[f].min() >= 0.0 and p[f].max() <= 2.6 and p[f].min() < 0.05 and p[f].max() > 2.55        # max(0, 1 - 1.6) = 0
    assert -0.4 <= p["dh"].min() < -0.39 and 0.39 < p["dh"].max() <= 0.4
    assert 0.1 <= p["blur_radius"].min() < 0.11 and 1.99 < p["blur_radius"].max() <= 2.0
    assert len({tuple(o) for o in p["d_order"]}) == 24


def test_streams_stay_aligned_whether_or_not_an_op_applies():
    """p = 0 against p = 1 for the blur: every other draw of every image is the same, and so is the generator's state afterwards."""
    from simseg_amd import pipeline as P
    sizes = [SIZES[i % len(SIZES)] for i in range(200)]
    names = ["random_resize_crop", "random_flip", "gaussian_blur", "color_distortion", "autoaug"]
    ra, rb = np.random.default_rng(17), np.random.default_rng(17)
    a = P.sample_pipeline_params(sizes, ra, _chain(names, blur={"p": 0.0}))
    b = P.sample_pipeline_params(sizes, rb, _chain(names, blur={"p": 1.0}))
    assert not a["blur_apply"].any() and b["blur_apply"].all() and 0 < a["d_apply"].sum() < 200 and 0 < a["d_gray"].sum() < 200
    for f in P.FIELDS + P.FULL_FIELDS:
        assert f == "blur_apply" or np.array_equal(a[f], b[f]), f
    assert ra.random() == rb.random()
    off = a["d_apply"] == 0                                       # a distortion that is not applied still drew its factors
    assert off.any() and (a["db"][off] != 1.0).all() and (a["dh"][off] != 0.0).all()


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_blur_weights_of_radius_one():
    from simseg_amd import pipeline as P
    assert P.blur_weights(1.0) == (0, 11184811, 2796202)
    for r in (0.1, 0.7, 1.0, 1.41, 1.42, 2.0, 3.3, 4.0, 8.4):
        R, ww, fw = P.blur_weights(r)
        assert 0 <= R <= 7 and ww > 0 and fw >= 0 and (1 << 24) - (2 * R + 1) * ww - 2 * fw in (0, 1), r


def test_table_of_a_row_with_all_eleven_ops():
    from simseg_amd import augment as A, pipeline as P
    chain = _chain(ALL11, ["transforms.resize.size=96", "transforms.random_erasing.reprob=1.0", "transforms.random_erasing.recount=2"])
    f32 = lambda v: int(np.array([v], np.float32).view(np.int32)[0])                   # noqa: E731
    p = P.explicit_pipeline_params(chain, 2, aa=("posterize", 4, 1, "solarize", 2, 1), jitter=((2, 3, 0, 1), 0.9, 1.1, 1.2),
                                   distort=[(1, (3, 1, 0, 2), 0.6, 0.7, 0.8, -0.1, 1), (0, (0, 1, 2, 3), 0.6, 0.7, 0.8, 0.1, 0)],
                                   blur=[(1, 1.0), (0, 2.0)], erase=[(1, 2, 30, 40)], seed=9)
    pl = P.plan_pipeline([(100, 120), (50, 70)], p, chain, "cpu")
    t = pl["img_tab_host"]
    assert t.shape == (2, 144) and t.dtype == np.int64 and pl["full"] and (P.TC_COLS, P.TC_OP, P.TC_P, P.FULL_MAX_OPS) == (144, 36, 48, 12)
    assert t[0, P.T_NOPS] == 11 and t[1, P.T_NOPS] == 5 and list(t[:, P.T_NERASE]) == [1, 1] and list(t[0, P.T_BOX:P.T_BOX + 4]) == [1, 2, 30, 40]
    codes = [A.OP_CODE["posterize"], A.OP_CODE["solarize"], A.OP_CODE["color"], P.OP_BRIGHTNESS, A.OP_CODE["contrast"], P.OP_BLUR,
             P.OP_HUE, A.OP_CODE["contrast"], P.OP_BRIGHTNESS, A.OP_CODE["color"], P.OP_GRAY]
    assert list(t[0, 36:48]) == codes + [0] and (P.OP_GRAY, P.OP_HUE, P.OP_BLUR) == (12, 13, 14)
    slot = lambda k: list(t[0, 48 + 8 * k:56 + 8 * k])                                  # noqa: E731
    assert slot(2) == [f32(1.2)] + [0] * 7 and slot(3) == [f32(0.9)] + [0] * 7 and slot(4) == [f32(1.1)] + [0] * 7
    assert slot(5) == [0, 11184811, 2796202, 0, 0, 0, 0, 0]
    assert slot(6) == [P.hue_shift(-0.1)] + [0] * 7 and P.hue_shift(-0.1) == 231
    assert slot(7) == [f32(0.7)] + [0] * 7 and slot(8) == [f32(0.6)] + [0] * 7 and slot(9) == [f32(0.8)] + [0] * 7
    assert slot(10) == [0] * 8 and slot(11) == [0] * 8
    assert list(t[1, 36:48]) == codes[:5] + [0] * 7                                     # neither the distortion nor the blur applied
    with pytest.raises(ValueError, match="blur radius"):
        P.plan_pipeline([(100, 120)], P.explicit_pipeline_params(chain, 1, blur=(1, 9.0)), chain, "cpu")


def test_header_declares_and_library_exports_the_chain_entries():
    import ctypes
    from simseg_amd import lib
    protos = lib.parse_header()
    assert "simseg_train_chain" in protos and "simseg_train_chain_scratch_bytes" in protos
    assert [a for _, a in protos["simseg_train_chain"][1]] == [a for _, a in protos["simseg_train_transforms"][1]]
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, "simseg_train_chain") and hasattr(so, "simseg_train_chain_scratch_bytes")
    assert lib.raw("simseg_train_chain_scratch_bytes", 3, 224) == 3 * 150528 and lib.raw("simseg_train_chain_scratch_bytes", 3, 31) == 0
    assert lib.raw("simseg_train_chain_scratch_bytes", 2, 288) == 2 * 2 * 248832
