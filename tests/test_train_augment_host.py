"""Host side of the training augmentation (simseg_amd/augment.py): the parameter sampler, the policy table, the plan and the public
builder.  No GPU needed: plans are built for the CPU device, where the axis arena lives on the host."""
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _cfg(path, argv=()):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, os.path.join(REPO, path), list(argv), update_clip_config)


SIZES = [(375, 500), (500, 333), (224, 224), (97, 1203), (8, 600), (1200, 40)]


@pytest.fixture(scope="module")
def draws():
    from simseg_amd import augment as A
    sizes = [SIZES[i % len(SIZES)] for i in range(20000)]
    return sizes, A.sample_params(sizes, np.random.default_rng(2024))


def test_boxes_inside_and_distributions(draws):
    sizes, p = draws
    H = np.array([s[0] for s in sizes]); W = np.array([s[1] for s in sizes])
    t, l, h, w = p["top"], p["left"], p["h"], p["w"]
    assert (t >= 0).all() and (l >= 0).all() and (h > 0).all() and (w > 0).all() and (t + h <= H).all() and (l + w <= W).all()
    tried = p["fallback"] == 0
    assert tried.sum() > 9000                        # (three of the six shapes are too extreme for most tries)
    # area fraction in scale, up to the rounding of w and h (each within 0.5 of its real value)
    lo = (np.maximum(w - 0.5, 0) * np.maximum(h - 0.5, 0)) / (H * W)
    hi = ((w + 0.5) * (h + 0.5)) / (H * W)
    assert (hi[tried] >= 0.6).all() and (lo[tried] <= 1.0).all()
    # aspect w / h in [3/4, 4/3], up to the same rounding
    assert ((w[tried] + 0.5) / np.maximum(h[tried] - 0.5, 1e-9) >= 0.75).all()
    assert ((np.maximum(w[tried] - 0.5, 0) / (h[tried] + 0.5)) <= 4 / 3).all()


def test_fallback_on_extreme_shapes():
    from simseg_amd import augment as A
    rng = np.random.default_rng(0)
    for H, W in [(8, 600), (600, 8), (1, 1000)]:
        p = A.sample_params([(H, W)] * 200, rng, autoaug=False)
        assert p["fallback"].all(), (H, W)
        # torchvision's centre crop: aspect clamped into [3/4, 4/3]
        in_ratio = W / H
        if in_ratio < 3 / 4:
            w, h = W, int(round(W / (3 / 4)))
        else:
            h, w = H, int(round(H * (4 / 3)))
        assert (p["h"] == h).all() and (p["w"] == w).all()
        assert (p["top"] == (H - h) // 2).all() and (p["left"] == (W - w) // 2).all()
    # a square image can take a ten-try crop, and with scale (1, 1) the ratio 1 window is the whole image
    p = A.sample_params([(50, 50)] * 50, rng, scale=(1.0, 1.0), autoaug=False)
    assert ((p["h"] <= 50) & (p["w"] <= 50)).all()


def test_policy_coverage_and_apply_rates(draws):
    from simseg_amd import augment as A
    _, p = draws
    k = p["policy"]
    assert set(np.unique(k)) == set(range(25))
    for j in (1, 2):
        for pi, row in enumerate(A.POLICY):
            prob = row[0] if j == 1 else row[3]
            sel = k == pi
            n = int(sel.sum())
            rate = p[f"apply{j}"][sel].mean()
            se = math.sqrt(max(prob * (1 - prob), 1e-12) / n)
            assert abs(rate - prob) <= 4 * se + 1e-12, (pi, j, rate, prob, n)
            # op code and magnitude are the policy's; signs only on applied signed ops
            name, mi = (row[1], row[2]) if j == 1 else (row[4], row[5])
            assert (p[f"op{j}"][sel] == A.OP_CODE[name]).all()
            assert (p[f"mag{j}"][sel] == float(A.MAGNITUDES[name][mi])).all()
            s = p[f"sign{j}"][sel]
            assert set(np.unique(s)) <= {-1, 1}
            if name not in A.SIGNED:
                assert (s == 1).all()
    signed = np.isin(p["op1"], [A.OP_CODE[o] for o in A.SIGNED]) & (p["apply1"] == 1)
    assert abs((p["sign1"][signed] == 1).mean() - 0.5) < 4 * math.sqrt(0.25 / signed.sum())


def test_same_seed_same_parameters():
    from simseg_amd import augment as A
    a = A.sample_params(SIZES * 10, np.random.default_rng(5))
    b = A.sample_params(SIZES * 10, np.random.default_rng(5))
    c = A.sample_params(SIZES * 10, np.random.default_rng(6))
    assert all(np.array_equal(a[f], b[f]) for f in A.FIELDS)
    assert not all(np.array_equal(a[f], c[f]) for f in A.FIELDS)


def test_policy_table_matches_design_doc():
    """The 25 rows and the magnitude ranges in augment.py are the ones DESIGN.md states."""
    from simseg_amd import augment as A
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    sec = text[text.index("## Device-side training augmentation"):]
    rows = re.findall(r"^\| *(\d+) *\| *([\d.]+) *\| *(\w+) *\| *(\d) *\| *([\d.]+) *\| *(\w+) *\| *(\d) *\|", sec, re.M)
    assert len(rows) == 25
    for (i, p1, o1, m1, p2, o2, m2), want in zip(rows, A.POLICY):
        assert (float(p1), o1, int(m1), float(p2), o2, int(m2)) == want, i
    mags = dict(re.findall(r"^- `(\w+)`: magnitudes `([^`]*)`", sec, re.M))
    assert set(mags) == set(A.MAGNITUDES)
    for op, spec in mags.items():
        got = [float(v) for v in A.MAGNITUDES[op]]
        want = [float(v) for v in eval(spec, {"linspace": lambda a, b, n: np.linspace(a, b, n), "rnd": lambda v: [int(x) for x in np.round(v)]})]
        assert got == want, op
    assert [int(v) for v in A.MAGNITUDES["posterize"]] == [8, 8, 7, 7, 6, 6, 5, 5, 4, 4]
    assert A.MAGNITUDES["shearX"][5] == pytest.approx(1 / 6) and A.MAGNITUDES["rotate"][9] == 30.0


def test_plan_rows_and_tables():
    from simseg_amd import augment as A, preproc
    sizes = [(375, 500), (8, 600), (97, 1203)]
    p = A.explicit_params([(10, 20, 300, 400), (0, 294, 8, 11), (0, 537, 97, 129)], "rotate", 30.0, 1, "color", 0.4, -1)
    p["apply2"][1] = 0
    pl = A.plan(sizes, p, 224, "cpu")
    it = pl["img_tab_host"]
    assert it.shape == (3, A.AUG_COLS) and it.dtype == np.int64 and np.array_equal(pl["img_tab"].numpy(), it)
    assert pl["src_off"] == [0, 375 * 500 * 3, 375 * 500 * 3 + 8 * 600 * 3] and pl["src_bytes"] == sum(h * w * 3 for h, w in sizes)
    assert list(it[:, A.C_SRC]) == pl["src_off"] and list(it[:, A.C_H]) == [375, 8, 97] and list(it[:, A.C_W]) == [500, 600, 1203]
    assert list(it[0, A.C_TOP:A.C_CW + 1]) == [10, 20, 300, 400]
    assert list(it[:, A.C_OP1]) == [A.OP_CODE["rotate"]] * 3 and list(it[:, A.C_OP2]) == [A.OP_CODE["color"], 0, A.OP_CODE["color"]]
    # the axis tables: in the arena at the row's offsets, host mirror == device copy, equal to preproc.axis_coefficients
    for r, (t, l, h, w) in enumerate([(10, 20, 300, 400), (0, 294, 8, 11), (0, 537, 97, 129)]):
        for off_col, ks_col, n_in in ((A.C_HOFF, A.C_HKS, w), (A.C_VOFF, A.C_VKS, h)):
            b, c = preproc.axis_coefficients(n_in, 224, "bilinear")
            off, ks = int(it[r, off_col]), int(it[r, ks_col])
            assert ks == c.shape[1]
            assert np.array_equal(pl["tab_host"][off:off + b.size], b.reshape(-1))
            assert np.array_equal(pl["tab_host"][off + b.size:off + b.size + c.size], c.reshape(-1))
    assert np.array_equal(pl["tab"].numpy()[:len(pl["tab_host"])], pl["tab_host"])
    # op parameters: rotate in Pillow's 16.16 fixed point, the colour factor as float bits
    m = A.rotate_matrix(30.0, 224)
    rot = [int(math.floor(v * 65536.0 + 0.5)) for v in (m[0], m[1], m[3], m[4], m[2] + m[1] * 0.5 + m[0] * 0.5, m[5] + m[4] * 0.5 + m[3] * 0.5)]
    assert list(it[0, A.C_P1:A.C_P1 + 6]) == rot and (it[0, A.C_P1 + 6:A.C_P2] == 0).all()
    assert np.int32(it[0, A.C_P2]).view(np.float32) == np.float32(1 + 0.4 * -1)
    assert (it[1, A.C_P2:] == 0).all()
    # posterize / solarize / shear slots
    assert A.op_slots(A.OP_CODE["posterize"], 5, 1, 224)[0] == 0b11111000
    assert A.op_slots(A.OP_CODE["solarize"], 113.77777777777777, 1, 224)[0] == 114
    assert A.op_slots(A.OP_CODE["solarize"], 256.0, 1, 224)[0] == 256
    sh = A.op_slots(A.OP_CODE["shearX"], 1 / 6, -1, 224)
    assert list(np.array(sh[:6], np.int64).view(np.float64)) == [1.0, -1 / 6, 0.0, 0.0, 1.0, 0.0]


def test_plan_refuses_bad_input():
    from simseg_amd import augment as A
    with pytest.raises(ValueError):
        A.plan([(8, 600)], A.explicit_params([(0, 0, 9, 10)]), 224, "cpu")
    with pytest.raises(ValueError):
        A.plan([(80, 600)], A.explicit_params([(0, 0, 9, 10)]), 31, "cpu")
    with pytest.raises(ValueError):
        A.plan([(80, 600)], A.explicit_params([(0, 0, 9, 10)]), 385, "cpu")
    with pytest.raises(ValueError):
        A.plan([(80, 600), (80, 600)], A.explicit_params([(0, 0, 9, 10)]), 224, "cpu")
    with pytest.raises(NotImplementedError):
        A.plan([(80, 600)], A.explicit_params([(0, 0, 9, 10)], "rotate", 90.0), 224, "cpu")


def test_shared_resample_cases_on_the_host():
    """The (image, box) cases of tests/test_gpu_resample_shared.py without a GPU: augment.plan takes the four boxes, the preprocessing
    plan of the four crops reads the very same axis tables, and Pillow's crop + resize is resample_ref of the crop."""
    import test_gpu_resample_shared as T
    from simseg_amd import augment as A, preproc
    ap = A.plan([hw for hw, _ in T.CASES], A.explicit_params([box for _, box in T.CASES]), T.S, "cpu")
    pp = T.crop_plan("cpu")
    assert pp["out_sizes"] == [(T.S, T.S)] * len(T.CASES) and pp["tab_host"] is ap["tab_host"]
    a, p = ap["img_tab_host"], pp["img_tab_host"]
    assert np.array_equal(a[:, A.C_HOFF:A.C_VKS + 1], p[:, 8:12]) and np.array_equal(a[:, A.C_CH:A.C_CW + 1], p[:, 1:3])
    raws = T._raws()
    for raw, want, (_, (t, l, h, w)) in zip(raws, T.pillow_route(raws), T.CASES):
        assert np.array_equal(preproc.resample_ref(np.ascontiguousarray(raw[t:t + h, l:l + w]), (T.S, T.S), "bilinear"), want)


@pytest.mark.parametrize("path", ["configs/clip/simseg.vit-b.yaml", "configs/clip/simseg.vit-s.yaml"])
def test_build_train_augmentation_on_shipped_configs(path):
    import torch
    from PIL import Image
    from simseg.transforms import build_device_transforms, build_train_augmentation, build_transforms
    from simseg_amd.augment import TrainAugment
    host_op, aug = build_train_augmentation(_cfg(path))
    assert isinstance(aug, TrainAugment) and aug.size == 224 and aug.scale == (0.6, 1.0) and aug.autoaug
    assert aug.lut.shape == (3, 256) and aug.lut.dtype == torch.float32
    a = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    t = host_op(Image.fromarray(a))
    assert t.dtype == torch.uint8 and np.array_equal(t.numpy(), a)
    _, only_crop = build_train_augmentation(_cfg(path, ["transforms.train_transforms=[random_resize_crop]"]))
    assert not only_crop.autoaug
    p = only_crop.sample([(100, 120)], np.random.default_rng(0))
    assert p["apply1"][0] == 0 and p["apply2"][0] == 0
    for names in ("[autoaug]", "[random_resize_crop,autoaug,resize]", "[resize]", "[autoaug,random_resize_crop]"):
        with pytest.raises(NotImplementedError):
            build_train_augmentation(_cfg(path, [f"transforms.train_transforms={names}"]))
    # the existing builders still refuse the training transforms
    with pytest.raises(NotImplementedError):
        build_transforms(_cfg(path), "train")
    with pytest.raises(NotImplementedError):
        build_device_transforms(_cfg(path), "train")
