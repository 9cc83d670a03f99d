"""Triplet and MixUpNCE on MI355X: ops.triplet_rows / ops.mix_nce_rows, the autograd nodes TripletFn / TripletLocalFn / MixNCEFn, and
the two losses driven through CLIPModel and Trainer.

What the header states exactly is compared exactly: the max-mode row losses bit for bit against fp32 CPU torch on the same similarities,
both gradient layouts, the accuracies, and MixUpNCE at alpha = 1 against ops.nce_rows.  Everything else follows the yardstick rule of
tests/test_gpu_loss_head.py, unchanged (its _check): the kernel's error against the float64 statements of tests/_contrastive_ref.py is
at most 8 x the error of the same formula in fp32 torch on the device + 4 fp32 ulps of the largest reference magnitude.  Every such
check prints one `loss-head |` line; profiles/contrastive_losses_tests.txt is that table.  Every case first ASSERTS, in float64, the
conditions under which its exact comparisons are well posed (_contrastive_ref.case_ok); none is skipped."""
import os

import numpy as np
import pytest
import torch

import _contrastive_ref as R
from conftest import REPO, tt
from test_gpu_loss_head import _check, _ignore_mask, _margin_ok

pytestmark = pytest.mark.gpu

MARGIN = R.MARGIN
REDUCE = {"mean": 0, "max": 1}


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _blocks(family, N1, N2, target0):
    s2 = R.sim_blocks(family, N1, N2, target0)
    for k in range(2):
        bad = R.case_ok(s2[k], target0)
        assert bad == [], f"{family} {N1}x{N2}+{target0} block {k}: {bad} - pick another seed"
    return s2


def _mean_ds_exact(ev, N1):
    """The mean mode's gradient as the kernel forms it: fl32(1 / (N1 - 1)) where the float64 statement has a positive entry and
    fl32(-count / (N1 - 1)) at the target column - each ONE rounded fp32 division."""
    pos = ev["ds"] > 0
    count = pos.sum(1).float()
    den = torch.tensor(float(N1 - 1), dtype=torch.float32)
    want = pos.float() * (torch.tensor(1.0) / den)
    neg = ev["ds"] < 0
    want[neg] = (-count / den)[neg.any(1)]
    return want


def _triplet_case(ops, case, s, target0, reduce, mask_block):
    """One block through ops.triplet_rows against the float64 statement and fp32 CPU torch."""
    N1, N2 = s.shape
    ev = R.triplet_eval(s, target0, MARGIN, reduce, mask_block)
    sims = s.cuda().clone()
    out, rows = ops.triplet_rows(sims, target0, MARGIN, reduce, mask_block)
    assert out.shape == (2,) and rows.shape == (N1,)
    assert out[1].item() == ev["acc"], f"{case}: top-1 accuracy {out[1].item()} vs {ev['acc']}"
    if reduce == 1:
        # the reference's own statements in fp32 on the CPU: max is order-free, so the row losses are its bits
        d1 = s[:, target0:target0 + N1].diag().view(N1, 1).expand_as(s)
        cost = (MARGIN + s - d1).clamp(min=0)
        mask = torch.zeros_like(cost)
        if mask_block:
            mask[:, target0:target0 + N1] += 1
        else:
            mask[torch.arange(N1), target0 + torch.arange(N1)] = 1
        want_rows = cost.masked_fill(mask.bool(), 0).max(1)[0]
        assert torch.equal(rows.cpu().view(torch.int32), want_rows.view(torch.int32)), f"{case}: max row losses are not fp32 torch's bits"
        assert torch.equal(sims.cpu(), ev["ds"].float()), f"{case}: max dS is not {{0, +1 at the first arg, -1 at the target}}"
    else:
        yard = R.triplet_eval(s, target0, MARGIN, reduce, mask_block, dtype=torch.float32, device="cuda")
        _check(case, "rows", rows, ev["rows"], yard["rows"])
        assert torch.equal(sims.cpu(), _mean_ds_exact(ev, N1)), f"{case}: mean dS is not k / (N1 - 1) as documented"
    yard = R.triplet_eval(s, target0, MARGIN, reduce, mask_block, dtype=torch.float32, device="cuda")
    _check(case, "total", out[0], ev["total"], yard["total"])
    if mask_block and N2 == N1:
        assert out[0].item() == 0.0 and not sims.any(), f"{case}: one rank - every column masked - must give exactly zero"
    # write_grad = False: the similarities survive bit for bit, the outputs are the same numbers
    kept = s.cuda().clone()
    o2, r2 = ops.triplet_rows(kept, target0, MARGIN, reduce, mask_block, write_grad=False)
    assert torch.equal(kept.cpu(), s) and torch.equal(o2, out) and torch.equal(r2, rows), f"{case}: write_grad=False"
    return out.cpu(), rows.cpu(), sims.cpu()


@pytest.mark.parametrize("mask_block", [0, 1])
@pytest.mark.parametrize("reduce", ["max", "mean"])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", R.SHAPES)
def test_triplet_rows(ops, N1, N2, target0, family, reduce, mask_block):
    s2 = _blocks(family, N1, N2, target0)
    case = f"triplet {family} {N1}x{N2}+{target0} {reduce} mask_block={mask_block}"
    one = [_triplet_case(ops, f"{case} b{k}", s2[k], target0, REDUCE[reduce], mask_block) for k in range(2)]
    # the stacked form: one launch over both blocks gives each block's rows and gradient bit for bit, the sum over both, both accuracies
    sims = s2.cuda().clone()
    out, rows = ops.triplet_rows(sims, target0, MARGIN, reduce, mask_block)
    assert out.shape == (3,) and rows.shape == (2, N1)
    for k in range(2):
        assert torch.equal(rows[k].cpu(), one[k][1]) and torch.equal(sims[k].cpu(), one[k][2]), f"{case}: stacked block {k}"
        assert out[1 + k].item() == one[k][0][1].item(), f"{case}: stacked accuracy {k}"
    ev = [R.triplet_eval(s2[k], target0, MARGIN, REDUCE[reduce], mask_block) for k in range(2)]
    yard = [R.triplet_eval(s2[k], target0, MARGIN, REDUCE[reduce], mask_block, dtype=torch.float32, device="cuda") for k in range(2)]
    _check(case + " x2", "total", out[0], ev[0]["total"] + ev[1]["total"], yard[0]["total"] + yard[1]["total"])


def _grid_block(N1, N2, target0, seed):
    """Similarities on the 1/8 grid in [-1, 7/8]: with margin 0.25 every pre is exact in fp32 (and in the yardstick), ties and zeros are
    real ties and real zeros."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 8, (N1, N2), generator=g).float() / 8


@pytest.mark.parametrize("mask_block", [0, 1])
def test_triplet_documented_rules_on_exact_inputs(ops, mask_block):
    N1, N2, target0, m = 33, 257, 100, 0.25
    s = _grid_block(N1, N2, target0, 7)
    idx = torch.arange(N1)
    s[idx, target0 + idx] = 0.5                                   # d = 0.5: pre = s - 0.25
    hi, lo = target0 + N1 + 70, 20                                # unmasked in both modes, in other threads and waves than the target
    s[:, lo], s[:, hi] = 1.0, 1.0                                 # the maximum cost 0.75 twice: the FIRST index (20) is the arg
    s[0::3, 5] = 0.25                                             # pre == 0 exactly: costs 0 and passes no gradient
    rows_none = torch.arange(N1) % 4 == 1                         # rows without a violation: every unmasked s <= 0.25
    s[rows_none] = torch.minimum(s[rows_none], torch.tensor(0.25))
    s[idx, target0 + idx] = 0.5
    for reduce in (1, 0):
        ev = R.triplet_eval(s, target0, m, reduce, mask_block)
        assert bool(((ev["pre"] == 0) & ev["unmasked"]).any()) and bool((ev["rows"] == 0).any()) and bool((ev["rows"] > 0).any())
        sims = s.cuda().clone()
        out, rows = ops.triplet_rows(sims, target0, m, reduce, mask_block)
        got = sims.cpu()
        assert torch.equal(rows.cpu(), ev["rows"].float()), f"reduce {reduce}: row losses"       # (exact: multiples of 1/8 over 32)
        if reduce == 1:
            assert torch.equal(got.double(), ev["ds"])
            viol = ~rows_none
            assert bool((got[viol, lo] == 1).all()) and bool((got[viol, hi] == 0).all()), "a tie for the maximum goes to the first index"
            assert not got[rows_none].any(), "a row without a violation has a zero gradient row"
        else:
            assert torch.equal(got, _mean_ds_exact(ev, N1))
            assert not got[0::3, 5].any(), "pre == 0 passes no gradient"
        assert out[0].item() == ev["total"].item()


@pytest.mark.parametrize("mask_block,N1,N2,reduce", [(1, 33, 33, 1), (1, 33, 33, 0), (1, 2, 2, 0), (0, 1, 1, 1)])
def test_triplet_all_masked_rows_give_zero(ops, mask_block, N1, N2, reduce):
    """Fully masked rows in both mask modes: the block mask over N2 == N1 (one rank), and the target mask over a one-column row (max mode:
    the mean refuses N1 = 1).  Zero loss, zero gradient - the similarities are large, so anything that leaked would show."""
    s = _grid_block(N1, N2, 0, 8) * 8
    sims = s.cuda().clone()
    out, rows = ops.triplet_rows(sims, 0, 0.25, reduce, mask_block)
    assert out[0].item() == 0.0 and not rows.any() and not sims.any()


@pytest.mark.parametrize("what", ["mean_N1_1", "targets_outside", "bad_reduce"])
def test_triplet_refusals_launch_nothing(ops, what):
    s = torch.randn(4, 9, generator=torch.Generator().manual_seed(5)).cuda()
    before = s.clone()
    if what == "mean_N1_1":
        with pytest.raises(ValueError, match="N1 >= 2"):
            ops.triplet_rows(s[:1], 0, MARGIN, "mean", 0)
        from simseg_amd.lib import call, ptr, stream
        scratch, out = torch.zeros(2, 1).cuda(), torch.zeros(2).cuda()
        with pytest.raises(RuntimeError, match="triplet_rows.*N1 >= 2"):                 # the C entry refuses on its own too
            call("simseg_triplet_rows", ptr(s), ptr(scratch[0]), ptr(scratch[1]), ptr(out), 1, 9, 0, MARGIN, 0, 0, 1, 1, stream())
    elif what == "targets_outside":
        with pytest.raises(RuntimeError, match="triplet_rows: targets"):
            ops.triplet_rows(s, 6, MARGIN, "max", 1)
    else:
        with pytest.raises(RuntimeError, match="triplet_rows: reduce 2"):
            ops.triplet_rows(s, 0, MARGIN, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(s, before)


# ------------------------------------------------------------------------------------------------------------------------------------------
# MixUpNCE rows
# ------------------------------------------------------------------------------------------------------------------------------------------
def _alpha_vec(N1, seed=3):
    return torch.rand(N1, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.05          # in (0, 1)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N1,N2,target0", R.SHAPES)
def test_mix_nce_rows_at_alpha_one_is_nce_rows(ops, N1, N2, target0, masked, smoothing):
    s = _blocks("aligned", N1, N2, target0)[0]
    t = torch.tensor([0.05]).cuda()
    ign = _ignore_mask(N1).cuda() if masked else None
    from simseg_amd.lib import call, ptr, stream
    want_s = s.cuda().clone()
    scratch = torch.empty(3, N1, device="cuda")
    want3 = torch.empty(3, device="cuda")
    call("simseg_nce_rows", ptr(want_s), ptr(t), ptr(ign), ptr(scratch[0]), ptr(scratch[1]), ptr(scratch[2]), ptr(want3), N1, N2, target0,
         smoothing, 1, stream())
    ref3 = ops.nce_rows(s.cuda().clone(), t, target0, ign, smoothing)
    assert torch.equal(ref3.view(torch.int32), want3.view(torch.int32))
    for alpha in (torch.ones(1), torch.ones(N1)):
        got_s = s.cuda().clone()
        out3, rows = ops.mix_nce_rows(got_s, t, target0, alpha.cuda(), ign, smoothing)
        assert torch.equal(out3.view(torch.int32), want3.view(torch.int32)), f"out3 {out3.tolist()} vs nce_rows {want3.tolist()}"
        assert torch.equal(rows.view(torch.int32), scratch[0].view(torch.int32)), "row losses"
        assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)), "dS"


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("alpha", ["0", "0.3", "vector"])
@pytest.mark.parametrize("N1,N2,target0", R.SHAPES)
def test_mix_nce_rows_vs_float64(ops, N1, N2, target0, alpha, masked, smoothing):
    s = _blocks("aligned", N1, N2, target0)[0]
    al = _alpha_vec(N1) if alpha == "vector" else torch.tensor([float(alpha)])
    ign = _ignore_mask(N1) if masked else None
    T = 0.05
    case = f"mix_nce {N1}x{N2}+{target0} alpha={alpha} eps={smoothing}" + (" ignore" if masked else "")
    ref = R.mix_nce_eval(s, T, target0, al, smoothing, ign)
    yard = R.mix_nce_eval(s, T, target0, al, smoothing, ign, dtype=torch.float32, device="cuda")
    assert _margin_ok(ref["z"]), f"{case}: top two logits too close for an exact accuracy check - pick another seed"
    sims = s.cuda().clone()
    out3, rows = ops.mix_nce_rows(sims, torch.tensor([T]).cuda(), target0, al.cuda(), None if ign is None else ign.cuda(), smoothing)
    _check(case, "loss", out3[0], ref["total"], yard["total"])
    _check(case, "rows", rows, ref["rows"], yard["rows"])
    _check(case, "dsims", sims, ref["ds"], yard["ds"])
    _check(case, "dT", out3[2], ref["dt"], yard["dt"])
    assert out3[1].item() == ref["acc"], f"{case}: top-1 accuracy {out3[1].item()} vs {ref['acc']}"
    kept = s.cuda().clone()
    o2, _ = ops.mix_nce_rows(kept, torch.tensor([T]).cuda(), target0, al.cuda(), None if ign is None else ign.cuda(), smoothing, write_grad=False)
    assert torch.equal(kept.cpu(), s) and torch.equal(o2[:2], out3[:2])


def test_mix_nce_rows_argument_checks(ops):
    s = torch.randn(4, 9, generator=torch.Generator().manual_seed(5)).cuda()
    t = torch.tensor([0.05]).cuda()
    before = s.clone()
    with pytest.raises(ValueError, match="alpha holds one element"):
        ops.mix_nce_rows(s, t, 0, torch.ones(3).cuda())
    with pytest.raises(TypeError, match="alpha must be fp32"):
        ops.mix_nce_rows(s, t, 0, torch.ones(4, dtype=torch.float64).cuda())
    with pytest.raises(RuntimeError, match="mix_nce_rows: targets"):
        ops.mix_nce_rows(s, t, 6, torch.ones(1).cuda())
    torch.cuda.synchronize()
    assert torch.equal(s, before)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the autograd nodes against float64 autograd of the restated reference
# ------------------------------------------------------------------------------------------------------------------------------------------
UP = 3.0          # the upstream gradient


def _triplet_torch(f1, f2g, rank, margin, reduce, local):
    """The reference's statements (mml_loss.py:285-347) on embeddings, in their dtype on their device -> (loss, scores)."""
    N1 = f1.shape[0]
    scores = f1.mm(f2g.t())
    if local:
        diagonal = scores.diag().view(N1, 1)
        d1, d2 = diagonal.expand_as(scores), diagonal.t().expand_as(scores)
        mask = torch.eye(N1, device=scores.device) > 0.5
        l12 = (margin + scores - d1).clamp(min=0).masked_fill(mask, 0)
        l21 = (margin + scores - d2).clamp(min=0).masked_fill(mask, 0)
        l12, l21 = (l12.sum(1) / (N1 - 1), l21.sum(0) / (N1 - 1)) if reduce == "mean" else (l12.max(1)[0], l21.max(0)[0])
        return (l12 + l21).sum(), scores
    diagonal = scores[:, N1 * rank: N1 * (rank + 1)].diag().view(N1, 1)
    loss = (margin + scores - diagonal.expand_as(scores)).clamp(min=0)
    mask = torch.zeros_like(loss)
    mask[:, N1 * rank: N1 * (rank + 1)] += 1
    loss = loss.masked_fill(mask.bool(), 0)
    loss = loss.sum(1) / (N1 - 1) if reduce == "mean" else loss.max(1)[0]
    return loss.sum(), scores


def _triplet_head_eval(a32, b32, rank, reduce, local, dtype, device):
    a = a32.to(device=device, dtype=dtype).requires_grad_(True)
    b = b32.to(device=device, dtype=dtype).requires_grad_(True)
    loss, scores = _triplet_torch(a, b, rank, R.margin32(MARGIN), reduce, local)
    (UP * loss).backward()
    return {"loss": loss.detach(), "da": a.grad, "db": b.grad, "s": scores.detach()}


@pytest.mark.parametrize("reduce", ["max", "mean"])
@pytest.mark.parametrize("N1,P", R.HEAD_SHAPES)
def test_triplet_fn_vs_float64(ops, N1, P, reduce):
    """rank 1 of 3 with a hand-built gathered matrix; gradients w.r.t. both embeddings (the gathered rows of other ranks included)."""
    from simseg_amd import heads
    img, _, gathered = R.head_embeddings(N1, P, R.HEAD_SEEDS[N1, P])
    for name, s, t0 in R.head_cases(N1, P):
        assert R.case_ok(s, t0) == [], f"head {name} N1={N1} P={P}: pick another seed"
    ref = _triplet_head_eval(img, gathered, 1, reduce, False, torch.float64, "cpu")
    yard = _triplet_head_eval(img, gathered, 1, reduce, False, torch.float32, "cuda")
    a, b = img.cuda().requires_grad_(True), gathered.cuda().requires_grad_(True)
    loss, acc = heads.TripletFn.apply(a, b, 1, MARGIN, REDUCE[reduce])
    (loss * UP).backward()
    case = f"TripletFn N1={N1} P={P} {reduce} rank 1/3"
    _check(case, "loss", loss, ref["loss"], yard["loss"])
    _check(case, "dfeat1", a.grad, ref["da"], yard["da"])
    _check(case, "dfeat2", b.grad, ref["db"], yard["db"])
    assert acc.item() == R.acc32(ref["s"], N1)
    assert ref["loss"].item() > 0


@pytest.mark.parametrize("reduce", ["max", "mean"])
@pytest.mark.parametrize("N1,P", R.HEAD_SHAPES)
def test_triplet_local_fn_vs_float64(ops, N1, P, reduce):
    from simseg_amd import heads
    img, txt, _ = R.head_embeddings(N1, P, R.HEAD_SEEDS[N1, P])
    for name, s, t0 in R.head_cases(N1, P):
        assert R.case_ok(s, t0) == [], f"head {name} N1={N1} P={P}: pick another seed"
    ref = _triplet_head_eval(img, txt, 0, reduce, True, torch.float64, "cpu")
    yard = _triplet_head_eval(img, txt, 0, reduce, True, torch.float32, "cuda")
    a, b = img.cuda().requires_grad_(True), txt.cuda().requires_grad_(True)
    loss, a1, a2 = heads.TripletLocalFn.apply(a, b, MARGIN, REDUCE[reduce])
    (loss * UP).backward()
    case = f"TripletLocalFn N1={N1} P={P} {reduce}"
    _check(case, "loss", loss, ref["loss"], yard["loss"])
    _check(case, "dfeat1", a.grad, ref["da"], yard["da"])
    _check(case, "dfeat2", b.grad, ref["db"], yard["db"])
    assert a1.item() == R.acc32(ref["s"], 0) and a2.item() == R.acc32(ref["s"].T.contiguous(), 0)
    assert ref["loss"].item() > 0


def _mix_head_eval(a32, b32, t32, rank, al32, smoothing, dtype, device):
    """mml_loss.py:154-191 of the reference on embeddings (no ignore mask)."""
    a = a32.to(device=device, dtype=dtype).requires_grad_(True)
    b = b32.to(device=device, dtype=dtype).requires_grad_(True)
    t = t32.to(device=device, dtype=dtype).requires_grad_(True)
    al = al32.to(device=device, dtype=dtype)
    N1 = a.shape[0]
    logits = (a @ b.T) / torch.clamp(t, 0.001, 0.5)
    targets = torch.arange(N1 * rank, N1 * (rank + 1), device=device)
    logp = torch.log_softmax(logits, -1)

    def ce(tg):
        return (1 - smoothing) * -logp.gather(1, tg[:, None])[:, 0] + smoothing * -logp.mean(-1)

    loss = (al * ce(targets) + (1 - al) * ce(targets.flip(0))).mean()
    (UP * loss).backward()
    return {"loss": loss.detach(), "da": a.grad, "db": b.grad, "dt": t.grad, "z": logits.detach()}


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("alpha", ["0.3", "vector"])
@pytest.mark.parametrize("N1,P", R.HEAD_SHAPES)
def test_mix_nce_fn_vs_float64(ops, N1, P, alpha, smoothing):
    from simseg_amd import heads
    img, _, gathered = R.head_embeddings(N1, P, R.HEAD_SEEDS[N1, P])
    al = _alpha_vec(N1) if alpha == "vector" else torch.tensor([float(alpha)])
    t32 = torch.tensor(0.05)
    ref = _mix_head_eval(img, gathered, t32, 1, al, smoothing, torch.float64, "cpu")
    yard = _mix_head_eval(img, gathered, t32, 1, al, smoothing, torch.float32, "cuda")
    assert _margin_ok(ref["z"])
    a, b, t = (x.cuda().requires_grad_(True) for x in (img, gathered, t32))
    loss, acc = heads.MixNCEFn.apply(a, b, t, al.cuda(), None, None, 1, smoothing)
    (loss * UP).backward()
    case = f"MixNCEFn N1={N1} P={P} alpha={alpha} eps={smoothing} rank 1/3"
    _check(case, "loss", loss, ref["loss"], yard["loss"])
    _check(case, "dfeat1", a.grad, ref["da"], yard["da"])
    _check(case, "dfeat2", b.grad, ref["db"], yard["db"])
    _check(case, "dT", t.grad, ref["dt"], yard["dt"])
    assert acc.item() == R.acc32(ref["z"], N1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# end to end through CLIPModel and Trainer
# ------------------------------------------------------------------------------------------------------------------------------------------
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False", "epoch=1", "optim.lr.init=1e-3"]


def _model(golden, extra):
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), TINY + list(extra), update_clip_config)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    g = golden("clip_glue")
    model.load_state_dict({k[3:]: tt(g[k]) for k in g.files if k.startswith("sd.")}, strict=False)
    return model.cuda().eval()                      # (eval: no dropout, so that two runs see the same numbers)


def _batch(golden):
    g = golden("clip_train_ws1")
    return {"image": tt(g["r0.image"]).cuda(), "input_ids": tt(g["r0.input_ids"]).cuda(), "attention_mask": tt(g["r0.attention_mask"]).cuda()}


@pytest.mark.parametrize("reduce", ["max", "mean"])
def test_model_with_the_triplet_loss(golden, reduce):
    from simseg_amd import heads, trainer as T
    batch = _batch(golden)
    extra = ["loss.name=Triplet", f"loss.triplet_loss.reduce_mode={reduce}"]
    # the local symmetric form
    m = _model(golden, extra + ["loss.global_reduce=False"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_dict, a1, a2 = m(batch)
        assert list(loss_dict) == ["triplet_loss"]
        with torch.no_grad():
            img, txt = m(batch, embeddings="all")
            want, w1, w2 = heads.TripletLocalFn.apply(img, txt, 0.2, REDUCE[reduce])
    assert loss_dict["triplet_loss"].item() == want.item() and a1.item() == w1.item() and a2.item() == w2.item()
    assert want.item() > 0
    tr = T.Trainer(m, m.cfg, steps_per_epoch=40)
    out = tr.train_step(batch)
    assert np.isfinite(float(out["loss"])) and tr.optimizer.steps_taken() == 1
    # global_reduce with no process group = ONE rank: every column is masked (the reference's behaviour): exactly zero
    m = _model(golden, extra + ["loss.global_reduce=True"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        img, txt = m(batch, embeddings="all")
        img.retain_grad()
        txt.retain_grad()
        loss_dict, a1, a2 = m.forward_loss(img, txt)
    assert list(loss_dict) == ["triplet_loss"] and loss_dict["triplet_loss"].item() == 0.0
    loss_dict["triplet_loss"].backward()
    assert not img.grad.any() and not txt.grad.any()
    assert 0.0 <= a1.item() <= 1.0 and 0.0 <= a2.item() <= 1.0
    tr = T.Trainer(m, m.cfg, steps_per_epoch=40)
    assert float(tr.train_step(batch)["loss"]) == 0.0


def test_model_with_the_mixupnce_loss(golden):
    from simseg_amd import trainer as T
    batch = _batch(golden)
    B = batch["image"].shape[0]
    mixed = dict(batch, image_alpha=_alpha_vec(B).cuda())
    m = _model(golden, ["loss.name=MixUpNCE"])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_dict, a1, a2 = m(mixed)
        assert list(loss_dict) == ["mixupnce_loss"] and np.isfinite(loss_dict["mixupnce_loss"].item())
        with torch.no_grad():
            img, txt = m(batch, embeddings="all")
            l1, w1 = m.loss(img, txt, image_alpha=mixed["image_alpha"])
            l2, w2 = m.loss(txt, img, image_alpha=mixed["image_alpha"])
        assert loss_dict["mixupnce_loss"].item() == (0.5 * (l1 + l2)).item() and a1.item() == w1.item() and a2.item() == w2.item()
        with pytest.raises(NotImplementedError, match="only supports mixing up one modal"):
            m(batch)
    tr = T.Trainer(m, m.cfg, steps_per_epoch=40)
    assert np.isfinite(float(tr.train_step(mixed)["loss"])) and tr.optimizer.steps_taken() == 1
    # under NCE the key is ignored: the same bits as today's batch
    n = _model(golden, ["loss.name=NCE"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        plain, p1, p2 = n(batch)
        keyed, k1, k2 = n(mixed)
    assert list(keyed) == ["nce_loss"] and torch.equal(plain["nce_loss"], keyed["nce_loss"]) and torch.equal(p1, k1) and torch.equal(p2, k2)
