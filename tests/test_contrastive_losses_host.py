"""Triplet and MixUpNCE, host side: the loss registry, the constructors' and keyword errors, the float64 statements of
tests/_contrastive_ref.py against the reference's own lines (restated in torch float64 with autograd), the per-element bits claim of the
max mode, the C ABI, and the conditions of the input tables the GPU tests use.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _contrastive_ref as R
from conftest import REPO

YAML = os.path.join(REPO, "configs/clip/simseg.vit-s.yaml")


def _cfg(argv=()):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, YAML, list(argv), update_clip_config)


def _loss(name, argv=()):
    from simseg.models.criteria.losses.builder import LOSS
    return LOSS.get(name)(_cfg([f"loss.name={name}"] + list(argv)), 0)


def test_registry_holds_the_three_contrastive_objectives():
    import simseg.models  # noqa: F401
    from simseg.models.criteria.losses.builder import LOSS
    assert LOSS.has("NCE") and LOSS.has("Triplet") and LOSS.has("MixUpNCE")


def test_triplet_constructor():
    t = _loss("Triplet")
    assert t.margin == 0.2 and t.reduce == "max" and t.global_reduce and t.group is None and t.rank == 0 and not hasattr(t, "both")
    t = _loss("Triplet", ["loss.triplet_loss.reduce_mode=mean", "loss.triplet_loss.margin=0.1", "loss.global_reduce=False"])
    assert t.margin == 0.1 and t.reduce == "mean" and not t.global_reduce
    with pytest.raises(NotImplementedError, match="Reduce method sum is not implemented yet"):
        _loss("Triplet", ["loss.triplet_loss.reduce_mode=sum"])


def test_mixupnce_constructor_and_keyword_errors():
    with pytest.raises(NotImplementedError):
        _loss("MixUpNCE", ["loss.global_reduce=False"])
    with pytest.raises(NotImplementedError):
        _loss("MixUpNCE", ["loss.temperature.name=schedule"])
    m = _loss("MixUpNCE", ["loss.temperature.name=parameter", "loss.smoothing=0.1"])
    assert isinstance(m.temperature, torch.nn.Parameter) and m.smoothing == 0.1 and m.group is None and not hasattr(m, "both")
    assert "temperature" in dict(m.named_parameters())
    c = _loss("MixUpNCE", ["loss.temperature.name=constant"])
    assert not list(c.parameters()) and float(c.temperature) == pytest.approx(0.02)
    f = torch.zeros(4, 8)
    for kw in ({}, {"image_alpha": 0.3, "text_alpha": 0.3}):
        with pytest.raises(NotImplementedError, match="only supports mixing up one modal"):
            m(f, f, **kw)
    with pytest.raises(ValueError, match="alpha holds 3 values"):
        m(f, f, image_alpha=torch.ones(3))


def test_forward_loss_hands_keywords_to_both_calls_and_skips_both():
    from simseg.models.pipelines.clip import CLIPModel
    calls = []

    class Loss:
        def both(self, a, b):
            calls.append("both")
            return torch.zeros(()), 0, 0

        def __call__(self, a, b, ignore_mask=None, **kw):
            calls.append(kw)
            return torch.ones(()), 0

    class M:
        global_reduce, loss = True, Loss()
        cfg = _cfg(["loss.name=MixUpNCE"])

    class Emb:
        is_cuda = True

    out, _, _ = CLIPModel.forward_loss(M(), Emb(), Emb(), image_alpha=0.25)
    assert calls == [{"image_alpha": 0.25}, {"image_alpha": 0.25}] and list(out) == ["mixupnce_loss"]
    del calls[:]
    CLIPModel.forward_loss(M(), Emb(), Emb())
    assert calls == ["both"]


# ---- the float64 statements against the reference's lines -----------------------------------------------------------------------------
def _reference_triplet(scores, rank, margin, reduce, global_reduce):
    """mml_loss.py:285-347 of the reference on a given score matrix: the dense statements, no process group."""
    N1 = scores.shape[0]
    if global_reduce:
        diagonal = scores[:, N1 * rank: N1 * (rank + 1)].diag().view(N1, 1)
        d1 = diagonal.expand_as(scores)
        loss = (margin + scores - d1).clamp(min=0)
        mask = torch.zeros_like(loss)
        mask[:, N1 * rank: N1 * (rank + 1)] += 1
        loss = loss.masked_fill(mask.bool(), 0)
        loss = loss.sum(1) / (N1 - 1) if reduce == "mean" else loss.max(1)[0]
        return loss
    diagonal = scores.diag().view(N1, 1)
    d1 = diagonal.expand_as(scores)
    d2 = diagonal.t().expand_as(scores)
    loss_1to2 = (margin + scores - d1).clamp(min=0)
    loss_2to1 = (margin + scores - d2).clamp(min=0)
    mask = torch.eye(N1) > 0.5
    loss_1to2 = loss_1to2.masked_fill(mask, 0)
    loss_2to1 = loss_2to1.masked_fill(mask, 0)
    if reduce == "mean":
        return loss_1to2.sum(1) / (N1 - 1), loss_2to1.sum(0) / (N1 - 1)
    return loss_1to2.max(1)[0], loss_2to1.max(0)[0]


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", [(5, 5, 0), (3, 9, 3), (33, 99, 33), (64, 256, 128)])
def test_triplet_ref_is_the_reference_global_branch(N1, N2, target0, family, reduce):
    s = R.sim_block(family, N1, N2, target0, 1).double().requires_grad_(True)
    m = R.margin32(R.MARGIN)
    rows = _reference_triplet(s, target0 // N1, m, reduce, True)
    rows.sum().backward()
    got_rows, total, ds, _ = R.triplet_ref(s.detach(), target0, R.MARGIN, 0 if reduce == "mean" else 1, 1)
    assert torch.equal(got_rows, rows.detach()) and total == rows.sum()
    torch.testing.assert_close(ds, s.grad, rtol=1e-13, atol=0)          # (autograd adds count times -1 / (N1 - 1) at the target column)
    assert torch.equal(ds != 0, s.grad != 0)
    if N2 == N1:
        assert total == 0 and not ds.any()          # one rank: every column is masked


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N1", [2, 5, 33, 97])
def test_triplet_ref_is_the_reference_local_branch(N1, family, reduce):
    """One matrix reduced along rows and along columns = the local statement on S and on S^T, and dS = dS_0 + dS_1^T."""
    s = R.sim_block(family, N1, N1, 0, 1).double().requires_grad_(True)
    m = R.margin32(R.MARGIN)
    r12, r21 = _reference_triplet(s, 0, m, reduce, False)
    (r12 + r21).sum().backward()
    code = 0 if reduce == "mean" else 1
    rows0, t0, ds0, _ = R.triplet_ref(s.detach(), 0, R.MARGIN, code, 0)
    rows1, t1, ds1, _ = R.triplet_ref(s.detach().T.contiguous(), 0, R.MARGIN, code, 0)
    assert torch.equal(rows0, r12.detach())
    torch.testing.assert_close(rows1, r21.detach(), rtol=0, atol=1e-15)          # (a column sum and a row sum of the same numbers)
    torch.testing.assert_close(t0 + t1, (r12 + r21).sum().detach(), rtol=0, atol=1e-13)
    torch.testing.assert_close(ds0 + ds1.T, s.grad, rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("alpha", [1.0, 0.0, 0.3, "vector"])
@pytest.mark.parametrize("N1,N2,target0", [(5, 5, 0), (3, 9, 3), (33, 99, 33)])
def test_mix_nce_ref_is_the_reference(N1, N2, target0, alpha, masked, smoothing):
    """mml_loss.py:154-191 of the reference on a given similarity matrix (the ignore mask's zeroing of feat2_global happens before the
    matrix and is the autograd node's business)."""
    s = R.sim_block("aligned", N1, N2, target0, 1).double().requires_grad_(True)
    T = torch.tensor(0.05, dtype=torch.float32).double().requires_grad_(True)
    # (fp32 values: the kernel reads alpha as fp32, and the statement under test rounds what it is given to fp32)
    al = (torch.rand(N1, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.05).double() if alpha == "vector" else float(np.float32(alpha))
    ign = torch.zeros(N1, dtype=torch.float64)
    if masked:
        ign[N1 // 2], ign[0] = 1.0, 0.25
    logits = s / torch.clamp(T, 0.001, 0.5)
    targets = torch.arange(target0, target0 + N1)

    def ce(x, t):           # nn.CrossEntropyLoss(reduction="none") / LabelSmoothingCrossEntropy(reduction="none"), :350-376
        logp = torch.log_softmax(x, -1)
        return (1 - smoothing) * -logp.gather(1, t[:, None])[:, 0] + smoothing * -logp.mean(-1)

    loss = al * ce(logits, targets) + (1 - al) * ce(logits, targets.flip(0))
    loss = loss * (1 - ign)
    loss.mean().backward()
    r = R.mix_nce_eval(s.detach(), 0.05, target0, al, smoothing, ign if masked else None)
    torch.testing.assert_close(r["rows"], loss.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r["total"], loss.mean().detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r["ds"], s.grad, rtol=1e-10, atol=1e-14)
    torch.testing.assert_close(r["dt"], T.grad, rtol=1e-10, atol=1e-14)


def test_max_mode_elements_are_two_rounded_fp32_operations():
    """fl32(fl32(margin + s) - d) with numpy float32 operations equals torch CPU's (margin + scores - d1) on fp32 inputs, element for
    element: the statement the kernel makes (no contraction) is the reference's fp32 arithmetic."""
    for family in R.FAMILIES:
        for N1, N2, target0 in R.SHAPES:
            s = R.sim_blocks(family, N1, N2, target0)[0]
            d1 = s[:, target0:target0 + N1].diag().view(N1, 1).expand_as(s)
            want = (R.MARGIN + s - d1).numpy()
            sn = s.numpy()
            got = (np.float32(R.MARGIN) + sn).astype(np.float32) - sn[np.arange(N1), target0 + np.arange(N1)][:, None]
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_c_abi_declares_and_exports_the_new_entries():
    from simseg_amd import lib
    protos = lib.parse_header()
    assert [n for _, n in protos["simseg_triplet_rows"][1]] == ["sims", "row_loss", "row_correct", "out", "N1", "N2", "target0", "margin", "reduce",
                                                                "mask_block", "blocks", "write_grad", "stream"]
    assert [n for _, n in protos["simseg_mix_nce_rows"][1]] == ["sims", "temperature", "ignore_mask", "alpha", "alpha_stride", "row_loss",
                                                                "row_correct", "row_tdot", "out3", "N1", "N2", "target0", "smoothing",
                                                                "write_grad", "stream"]
    so = ctypes.CDLL(lib.LIB_PATH)          # (the built library: the suite runs after the build)
    from simseg_amd import build
    import glob
    objs = [os.path.basename(o) for o in glob.glob(os.path.join(REPO, "simseg_amd", "build", "loss*.o"))]
    assert not getattr(build, "TWICE", ()) and objs in ([], ["loss.o"])     # fp32 rows, one entry point each: ONE object (none here when the library was built elsewhere)
    src = open(os.path.join(REPO, "simseg_amd/csrc/loss.hip")).read()
    for name in ("simseg_triplet_rows", "simseg_mix_nce_rows"):
        assert f'extern "C" int {name}(' in src, f"{name} is not defined in loss.hip"
        assert hasattr(so, name), f"{name} is not exported"
        assert not hasattr(so, name + "_h16"), f"{name}_h16 is exported"
    # the same for the row kernels these losses sit next to in a step: one object, the 16-bit type chosen per call
    objs = [os.path.basename(o) for o in glob.glob(os.path.join(REPO, "simseg_amd", "build", "rowops*.o"))]
    assert not getattr(build, "TWICE", ()) and objs in ([], ["rowops.o"])     # the type is a template argument: ONE object (none here when the library was built elsewhere)
    src = open(os.path.join(REPO, "simseg_amd/csrc/rowops.hip")).read()
    for name in ("simseg_layernorm_fwd", "simseg_layernorm_bwd", "simseg_layernorm_bwd_workspace_bytes", "simseg_colsum_accum",
                 "simseg_vit_im2col", "simseg_topk_pool_workspace_bytes", "simseg_topk_pool_l2norm_fwd", "simseg_topk_pool_l2norm_bwd",
                 "simseg_row_rnorm", "simseg_cast", "simseg_dropout_apply"):
        assert src.count(f" {name}(") == 1, f"{name} is not defined exactly once in rowops.hip"
        assert hasattr(so, name), f"{name} is not exported"
        assert not hasattr(so, name + "_h16"), f"{name}_h16 is exported"


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", R.SHAPES)
def test_input_tables_satisfy_their_conditions(N1, N2, target0, family):
    s2 = R.sim_blocks(family, N1, N2, target0)
    for k in range(2):
        assert R.case_ok(s2[k], target0) == [], f"{family} {N1}x{N2}+{target0} block {k}: pick another seed"


def test_families_differ_as_described():
    """"random" violates the margin in most rows; "aligned" leaves a share of rows without a violation (and not all of them)."""
    viol = {}
    for family in R.FAMILIES:
        rows = torch.cat([R.triplet_eval(R.sim_blocks(family, N1, N2, t0)[0], t0, R.MARGIN, 1, 0)["rows"]
                          for N1, N2, t0 in R.SHAPES])
        viol[family] = (rows > 0).double().mean().item()
    assert viol["random"] > 0.9 and 0.1 < viol["aligned"] < 0.9, viol


@pytest.mark.parametrize("N1,P", R.HEAD_SHAPES)
def test_head_tables_satisfy_their_conditions(N1, P):
    for name, s, t0 in R.head_cases(N1, P):
        assert R.case_ok(s, t0) == [], f"head {name} N1={N1} P={P}: pick another seed"
