"""Mixup / CutMix, host side: the sampler's invariants, the two host statements, the config builder, the loss registry, and the model's
choice between the hard and the soft head.  No GPU."""
import os

import numpy as np
import pytest
import torch

from _mix_ref import dense_target64, mix_exact, soft_ce64
from conftest import REPO

YAML = os.path.join(REPO, "configs/linear_prob/imagenet.yaml")
SIZES = [(1, 1), (7, 5), (224, 224)]
CONFIGS = {"mixup_only": dict(mixup_alpha=0.8, cutmix_alpha=0.0), "cutmix_only": dict(mixup_alpha=0.0, cutmix_alpha=1.0),
           "both": dict(mixup_alpha=0.8, cutmix_alpha=1.0), "uncorrected": dict(mixup_alpha=0.8, cutmix_alpha=1.0, correct_lam=False),
           "minmax": dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8)), "half": dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5)}


def _cols(p):
    t = p["table"]
    return t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 5].copy().view(np.float32), t[:, 6].copy().view(np.float32)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_sampling_invariants(mode, name, H, W):
    from simseg_amd.mixup import Mixup
    kw = CONFIGS[name]
    mix = Mixup(mode=mode, label_smoothing=0.1, num_classes=10, **kw)
    rng = np.random.default_rng(1000 + 17 * SIZES.index((H, W)))
    B = 8
    kinds_seen, distinct = set(), 0
    for _ in range(100):
        p = mix.sample(B, H, W, rng)
        t = p["table"]
        assert t.dtype == np.int32 and t.shape == (B, 8) and t.flags.c_contiguous and p["smoothing"] == 0.1
        kind, yl, yh, xl, xh, lam, om = _cols(p)
        assert np.array_equal(p["lam"], lam) and p["lam"].dtype == np.float32
        assert ((kind >= 0) & (kind <= 2)).all() and (t[:, 7] == 0).all()
        assert ((lam >= 0) & (lam <= 1)).all() and np.array_equal(om, (1.0 - lam.astype(np.float64)).astype(np.float32))
        assert ((0 <= yl) & (yl <= yh) & (yh <= H) & (0 <= xl) & (xl <= xh) & (xh <= W)).all()
        assert (lam[kind == 0] == 1).all() and (lam[kind == 1] < 1).all()
        cut = kind == 2
        if kw.get("correct_lam", True) or "cutmix_minmax" in kw:                   # lam = 1 - area / (H W), in double, rounded to fp32
            area = (yh - yl).astype(np.float64) * (xh - xl)
            assert np.array_equal(lam[cut], (1.0 - area[cut] / float(H * W)).astype(np.float32))
        if "cutmix_minmax" in kw and cut.any():
            lo, hi = kw["cutmix_minmax"]
            ch, cw = (yh - yl)[cut], (xh - xl)[cut]
            assert (ch >= int(H * lo)).all() and (ch <= max(int(H * hi) - 1, int(H * lo))).all()
            assert (cw >= int(W * lo)).all() and (cw <= max(int(W * hi) - 1, int(W * lo))).all()
        if kw["mixup_alpha"] == 0:
            assert not (kind == 1).any()
        if kw["cutmix_alpha"] == 0:
            assert not cut.any()
        if mode == "batch":
            assert (t == t[0]).all()
        if mode in ("batch", "pair"):
            assert np.array_equal(t, t[::-1])                                        # row i equals row B - 1 - i
        distinct = max(distinct, len({r.tobytes() for r in t}))
        kinds_seen |= set(kind.tolist())
    if mode == "pair" and (H, W) == (224, 224):
        assert distinct > 1                                                          # pairs differ from each other
    if mode == "elem" and (H, W) == (224, 224):
        assert distinct > B // 2                                                     # rows differ, also inside a pair
    if name == "both" and (H, W) != (1, 1):
        assert kinds_seen >= {1, 2}
    if name == "half":
        assert 0 in kinds_seen and len(kinds_seen) > 1


def test_prob_zero_zero_alphas_and_odd_batches():
    from simseg_amd.mixup import Mixup
    rng = np.random.default_rng(3)
    for mode in ("batch", "pair", "elem"):
        p = Mixup(0.8, 1.0, prob=0.0, mode=mode).sample(6, 7, 5, rng)
        assert (p["table"][:, 0] == 0).all() and (p["lam"] == 1).all() and (p["table"][:, 1:5] == 0).all()
        with pytest.raises(ValueError, match="even"):
            Mixup(0.8, 1.0, mode=mode).sample(5, 7, 5, rng)
    assert (Mixup(0.0, 0.0).sample(4, 7, 5, rng)["table"][:, 0] == 0).all()
    with pytest.raises(ValueError, match="mode"):
        Mixup(0.8, 1.0, mode="half")
    # the same generator state gives the same table; the documented order: u, then v (both alphas positive), then lam, then the box
    a = Mixup(0.8, 1.0, mode="elem").sample(8, 32, 32, np.random.default_rng(5))
    b = Mixup(0.8, 1.0, mode="elem").sample(8, 32, 32, np.random.default_rng(5))
    assert np.array_equal(a["table"], b["table"])
    r = np.random.default_rng(11)
    u, v = r.random(), r.random()
    lam = np.float32(r.beta(1.0, 1.0) if v < 0.5 else r.beta(0.8, 0.8))
    got = Mixup(0.8, 1.0, mode="batch", correct_lam=False).sample(2, 32, 32, np.random.default_rng(11))
    assert u < 1.0 and got["table"][0, 0] == (2 if v < 0.5 else 1) and got["lam"][0] == lam


def _elem_case(dtype):
    from simseg_amd.mixup import explicit_params
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(4, 3, 5, 7, generator=g) * 2).to(dtype)
    # pair (0, 3): a mixup row whose partner is a cutmix row; pair (1, 2): two cutmix rows with different, overlapping boxes
    p = explicit_params([1, 2, 2, 2], [0.3, 0.5, 0.25, 0.75], [(0, 0, 0, 0), (1, 4, 2, 6), (0, 3, 0, 4), (2, 5, 3, 7)])
    return x, p


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_mix_ref_mixes_from_the_originals(dtype):
    from simseg_amd.mixup import mix_ref
    x, p = _elem_case(dtype)
    keep = x.clone()
    got = mix_ref(x, p)
    assert torch.equal(x, keep) and got.dtype == dtype                               # the input is not touched
    want = torch.from_numpy(mix_exact(x.float().numpy(), p["table"])).to(dtype)      # (one rounding to the storage type)
    assert torch.equal(got.view(torch.int16 if dtype != torch.float32 else torch.int32), want.view(torch.int16 if dtype != torch.float32 else torch.int32))
    # both rows of a pair see the other's ORIGINAL values: row 3 takes row 0's untouched pixels, row 0 blends row 3's untouched ones
    assert torch.equal(got[3, :, 2:5, 3:7], keep[0, :, 2:5, 3:7])
    if dtype == torch.float32:                                                       # torch's own statement, with Python scalars
        lam = float(np.float32(0.3))
        assert torch.equal(got[0], keep[0] * lam + keep[3] * (1 - lam))
    assert torch.equal(got[1, :, 1:4, 2:6], keep[2, :, 1:4, 2:6]) and torch.equal(got[2, :, 0:3, 0:4], keep[1, :, 0:3, 0:4])
    # a sequential in-place mix would have read row 0's blended pixels into row 3
    assert not torch.equal(got[0], keep[0]) and not torch.equal(got[3, :, 2:5, 3:7], got[0, :, 2:5, 3:7])


def test_soft_target_ref_is_timms_mixup_target():
    from simseg_amd.mixup import explicit_params, soft_target_ref
    C = 7
    labels = torch.tensor([0, 3, 6, 3, 2, 5])
    p = explicit_params([1, 2, 0, 0, 2, 1], [0.3, 0.75, 1.0, 1.0, 0.75, 2.0 ** -24], smoothing=0.1)
    got = soft_target_ref(labels, p, C)
    want = dense_target64(labels, labels.flip(0), p["lam"], 0.1, C)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert torch.allclose(got.sum(1), torch.ones(6, dtype=torch.float64), atol=1e-15)
    # timm's on / off values, spelled out on one row: labels 0 and 5, lam 0.3
    off, on, lam = 0.1 / C, 1.0 - 0.1 + 0.1 / C, float(np.float32(0.3))
    row = [off * lam + off * (1 - lam)] * C
    row[0] = on * lam + off * (1 - lam)
    row[5] = off * lam + on * (1 - lam)
    assert got[0].tolist() == row
    assert torch.equal(soft_target_ref(labels, p, C, smoothing=0.0)[2], torch.nn.functional.one_hot(labels, C)[2].double())


def _cfg(argv=()):
    from simseg.core.config import update_cfg
    from simseg.tasks.linear_prob.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, YAML, list(argv), update_clip_config)


def test_build_mixup_reads_every_key():
    from simseg.transforms import build_mixup
    assert build_mixup(_cfg(["transforms.mixup=0.0", "transforms.cutmix=0.0"])) is None
    mix = build_mixup(_cfg([]))                                                      # the task defaults: mixup 0.8, cutmix 1.0, batch mode
    assert (mix.mixup_alpha, mix.cutmix_alpha, mix.cutmix_minmax, mix.prob, mix.switch_prob, mix.mode) == (0.8, 1.0, None, 1.0, 0.5, "batch")
    assert mix.correct_lam and mix.label_smoothing == 0.0 and mix.num_classes == 1000
    mix = build_mixup(_cfg(["transforms.mixup=0.2", "transforms.cutmix=0.6", "transforms.cutmix_minmax=[0.25,0.5]", "transforms.mixup_prob=0.7",
                            "transforms.mixup_switch_prob=0.3", "transforms.mixup_mode=elem", "loss.smoothing=0.1",
                            "model.classifier.num_classes=10"]))
    assert (mix.mixup_alpha, mix.cutmix_alpha, mix.cutmix_minmax, mix.prob, mix.switch_prob, mix.mode) == (0.2, 0.6, (0.25, 0.5), 0.7, 0.3, "elem")
    assert mix.label_smoothing == 0.1 and mix.num_classes == 10
    assert "elem" in repr(mix)
    only_cut = build_mixup(_cfg(["transforms.mixup=0.0"]))
    assert only_cut.mixup_alpha == 0.0 and only_cut.cutmix_alpha == 1.0


def test_loss_registry_and_the_unfused_soft_target_loss():
    from simseg.models.criteria.losses import LOSS
    ls = LOSS.get("LabelSmoothingCrossEntropy")(None, 0)
    assert ls.smoothing == 0.1 and ls.reduction == "mean"
    assert LOSS.get("LabelSmoothingCrossEntropy")(None, 0, smoothing=0.2, reduction="none").confidence == 0.8
    with pytest.raises(AssertionError):
        LOSS.get("LabelSmoothingCrossEntropy")(None, 0, smoothing=1.0)
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(6, 9, generator=g) * 3).requires_grad_(True)
    a, b = torch.randint(0, 9, (6,), generator=g), torch.randint(0, 9, (6,), generator=g)
    t64 = dense_target64(a, b, np.linspace(0.0, 1.0, 6), 0.1, 9)
    rows64, grad64 = soft_ce64(x.detach().double(), t64)
    rows = LOSS.get("SoftTargetCrossEntropy")(None, 0, reduction="none")(x, t64.float())
    mean = LOSS.get("SoftTargetCrossEntropy")(None, 0)(x, t64.float())
    assert rows.shape == (6,) and mean.shape == ()
    # fp32 torch ops on the CPU against float64: a few ulps of values of order 10
    assert (rows.detach().double() - rows64).abs().max() < 1e-5 and abs(mean.item() - rows64.mean().item()) < 1e-5
    mean.backward()
    assert (x.grad.double() - grad64).abs().max() < 1e-6
    assert "unfused" in " ".join(LOSS.get("SoftTargetCrossEntropy").__doc__.lower().split())


def test_header_declares_the_new_symbols():
    from simseg_amd.lib import parse_header
    protos = parse_header()
    assert [n for _, n in protos["simseg_mix_batch"][1]] == ["images", "dt", "table", "table_host", "B", "C", "H", "W", "stream"]
    assert [n for _, n in protos["simseg_soft_ce_rows"][1]] == ["logits", "dt", "labels_a", "labels_b", "lam", "smoothing", "loss_rows", "ranks",
                                                               "dlogits", "out3", "B", "C", "gscale", "write_grad", "stream"]
    from simseg_amd import build
    import glob
    objs = [os.path.basename(o) for o in glob.glob(os.path.join(REPO, "simseg_amd", "build", "mixup*.o"))]
    assert not getattr(build, "TWICE", ()) and objs in ([], ["mixup.o"])     # the type is a template argument: ONE object (none here when the library was built elsewhere)
    assert os.path.exists(os.path.join(REPO, "simseg_amd/csrc/mixup.hip"))


def test_model_takes_the_soft_head_only_for_a_mixed_batch(monkeypatch):
    """A batch without label_b / lam goes to ProbeHeadFn in forward, forward(valid=True) and eval_counts, and never near the soft path;
    a batch with them goes to SoftProbeHeadFn with the batch's smoothing (default 0)."""
    import simseg_amd.probe as probe
    from simseg.models import PIPELINE
    from simseg.utils import build_from_cfg
    from simseg_amd import ops
    cfg = _cfg(["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
                "model.classifier.num_classes=10"])
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    feats = torch.randn(4, 128)
    calls = []

    def boom(*a, **k):
        raise AssertionError("the soft-target path was reached by a batch without label_b / lam")

    def hard(x, w, b, y):
        calls.append(("hard", y))
        return torch.zeros(()), torch.tensor([0.5, 1.0, 2.0]), torch.zeros(4, 10)

    def soft(x, w, b, ya, yb, lam, eps):
        calls.append(("soft", ya, yb, lam, eps))
        return torch.zeros(()), torch.tensor([0.5, 1.0, 2.0]), torch.zeros(4, 10)

    monkeypatch.setattr(model, "forward_image_feature", lambda image: feats)
    monkeypatch.setattr(probe.ProbeHeadFn, "apply", staticmethod(hard))
    monkeypatch.setattr(probe.SoftProbeHeadFn, "apply", staticmethod(boom))
    monkeypatch.setattr(probe.SoftCEFn, "apply", staticmethod(boom))
    monkeypatch.setattr(ops, "soft_ce_rows", boom)
    monkeypatch.setattr(ops, "mix_batch", boom)
    batch = {"image": torch.zeros(4, 3, 96, 96), "label": torch.tensor([1, 2, 3, 4])}
    loss_dict, acc1, acc5 = model(batch)
    assert list(loss_dict) == ["crossentropy_loss"] and acc1.tolist() == [25.0] and acc5.tolist() == [50.0]
    _, pred, label = model(batch, valid=True)
    assert pred.shape == (4, 10) and label is batch["label"]
    assert model.eval_counts(batch).tolist() == [2.0, 1.0, 2.0]
    assert [c[0] for c in calls] == ["hard"] * 3
    # only ONE of the two keys is not a mixed batch either
    model({**batch, "lam": torch.ones(4)})
    assert [c[0] for c in calls] == ["hard"] * 4
    monkeypatch.setattr(probe.SoftProbeHeadFn, "apply", staticmethod(soft))
    mixed = {**batch, "label_b": batch["label"].flip(0), "lam": torch.full((4,), 0.25)}
    loss_dict, acc1, acc5 = model(mixed)
    assert calls[-1][0] == "soft" and calls[-1][1] is batch["label"] and calls[-1][2] is mixed["label_b"] and calls[-1][3] is mixed["lam"]
    assert calls[-1][4] == 0.0 and list(loss_dict) == ["crossentropy_loss"] and acc1.tolist() == [25.0]
    model({**mixed, "smoothing": 0.1})
    assert calls[-1][0] == "soft" and calls[-1][4] == 0.1
