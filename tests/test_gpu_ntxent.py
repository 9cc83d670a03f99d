"""The NT-Xent loss on MI355X: ops.ntxent_rows, the autograd node heads.NTXentFn and LOSS.NTXent.

Toleranced checks follow the yardstick rule of tests/test_gpu_loss_head.py, unchanged (its _check): the kernel's error against the float64
statement of tests/_ntxent_ref.py is at most 8 x the error of the same formula in fp32 torch on the device + 4 fp32 ulps of the largest
reference magnitude.  Every such check prints one `loss-head |` line; profiles/ntxent_loss_tests.txt is that table.  What the header states
exactly is compared exactly: the two accuracies, dLoss/dT = 0 outside the clamp, the zero gradient of the own column, the one-column case,
write_grad = 0, run-to-run bits, exact zeros at saturation.  Every case first ASSERTS the top-1 margin in float64
(tests/test_ntxent_host.py asserts it on the CPU too); none is skipped."""
import numpy as np
import pytest
import torch

import _ntxent_ref as N
from test_gpu_loss_head import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _dev(v):
    return torch.tensor([v], dtype=torch.float32).cuda()


def _own(N1, target0):
    return torch.arange(N1), target0 + torch.arange(N1)


def _rows_case(ops, case, s, T, target0):
    N1, N2 = s.shape
    ref = N.ntxent_eval(s, T, target0)
    assert N.margin_ok(ref["z"]), f"{case}: top-1 margin - pick another seed"
    yard = N.ntxent_eval(s, T, target0, dtype=torch.float32, device="cuda")
    sims = s.cuda().clone()
    out4, rows = ops.ntxent_rows(sims, _dev(T), target0)
    assert out4.shape == (4,) and rows.shape == (N1,)
    _check(case, "rows", rows, ref["rows"], yard["rows"])
    _check(case, "total", out4[0], ref["total"], yard["total"])
    _check(case, "dsims", sims, ref["ds"], yard["ds"])
    _check(case, "dT", out4[3], ref["dt"], yard["dt"])
    assert out4[1].item() == ref["acc_a"] and out4[2].item() == ref["acc_b"], \
        f"{case}: top-1 accuracies {out4[1].item()}, {out4[2].item()} vs {ref['acc_a']}, {ref['acc_b']}"
    if not (N.T_LO <= float(np.float32(T)) <= N.T_HI):
        assert out4[3].item() == 0.0, f"{case}: dLoss/dT outside the clamp must be exactly 0"
    elif N2 > 2:
        assert out4[3].item() != 0.0, f"{case}: dLoss/dT"
    g = sims.cpu()
    assert not g[_own(N1, target0)].any(), f"{case}: the gradient in the own column must be exactly 0"
    if N2 == 2:          # one non-self column: p = 1 exactly
        assert out4[0].item() == 0.0 and not rows.any() and not g.any() and out4[3].item() == 0.0
        assert out4[1].item() == 1.0 and out4[2].item() == 1.0
    return out4, rows, sims


@pytest.mark.parametrize("T", N.SETTINGS)
@pytest.mark.parametrize("family", N.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", N.SHAPES)
def test_ntxent_rows_vs_float64(ops, N1, N2, target0, family, T):
    s2 = N.blocks(family, N1, N2, target0)
    for k in range(2):
        _rows_case(ops, f"ntxent {family} {N1}x{N2}+{target0} T={T:g} b{k}", s2[k], T, target0)


@pytest.mark.parametrize("T", [0.1, 0.7])
@pytest.mark.parametrize("N1,N2,target0", N.SHAPES)
def test_ntxent_rows_without_the_gradient_and_twice(ops, N1, N2, target0, T):
    s = N.blocks("aligned", N1, N2, target0)[0]
    sims = s.cuda().clone()
    out4, rows = ops.ntxent_rows(sims, _dev(T), target0)
    # write_grad = False: the similarities survive bit for bit; loss, both accuracies and the row losses are the same bits
    kept = s.cuda().clone()
    o2, r2 = ops.ntxent_rows(kept, _dev(T), target0, write_grad=False)
    assert torch.equal(kept.cpu().view(torch.int32), s.view(torch.int32)), "write_grad=False touched the similarities"
    assert torch.equal(o2[:3].view(torch.int32), out4[:3].view(torch.int32)) and torch.equal(r2.view(torch.int32), rows.view(torch.int32))
    # no atomics: a second run on the same input gives the same bits
    again = s.cuda().clone()
    o3, r3 = ops.ntxent_rows(again, _dev(T), target0)
    assert torch.equal(o3.view(torch.int32), out4.view(torch.int32)) and torch.equal(r3.view(torch.int32), rows.view(torch.int32))
    assert torch.equal(again.view(torch.int32), sims.view(torch.int32))


def test_ntxent_rows_own_column_is_never_read_as_a_value(ops):
    """Whatever stands in the own column - NaN here - nothing changes: it is in no maximum, no sum and no product."""
    N1, N2, target0 = 34, 257, 102
    s = N.blocks("aligned", N1, N2, target0)[0]
    a = s.cuda().clone()
    o1, r1 = ops.ntxent_rows(a, _dev(0.1), target0)
    p = s.clone()
    p[_own(N1, target0)] = float("nan")
    b = p.cuda()
    o2, r2 = ops.ntxent_rows(b, _dev(0.1), target0)
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(r1.view(torch.int32), r2.view(torch.int32))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_ntxent_rows_saturation(ops):
    """T = 1e-3 with s in {-1, +1}: |z| = 1000, exp(-2000) underflows to 0 - finite everywhere, and dS is exactly 0 at every non-self
    column holding -1 in a row that has a +1 among its non-self columns."""
    N1, N2, target0, T = 6, 64, 20, 1e-3
    B = N1 // 2
    g = torch.Generator().manual_seed(11)
    s = torch.randint(0, 2, (N1, N2), generator=g).float() * 2 - 1
    idx, own = _own(N1, target0)
    pos = target0 + (idx + B) % N1
    s[idx, own] = 1.0
    s[idx, pos] = 1.0               # every positive is among its row's maxima: ties, and the first index decides the hit
    s[0, :target0] = -1.0           # row 0: no +1 before its positive's column...
    s[0, target0 + 1:pos[0]] = -1.0         # ...(its own column, target0, is skipped): a hit
    s[1, 0] = 1.0                   # row 1: a +1 in column 0: a miss
    s[5] = -1.0                     # row 5 (view b): no +1 at all among its non-self columns - a uniform softmax, outside the zero rule
    s[5, own[5]] = 1.0
    ref = N.ntxent_eval(s, T, target0)
    yard = N.ntxent_eval(s, T, target0, dtype=torch.float32, device="cuda")
    sims = s.cuda().clone()
    out4, rows = ops.ntxent_rows(sims, _dev(T), target0)
    assert bool(torch.isfinite(out4).all()) and bool(torch.isfinite(rows).all()) and bool(torch.isfinite(sims).all())
    assert out4[1].item() == ref["acc_a"] and out4[2].item() == ref["acc_b"]          # (exact ties on exact inputs: the first index wins on both sides)
    assert 0.0 < ref["acc_a"] < 1.0
    case = "ntxent saturation 6x64+20 T=0.001"
    _check(case, "rows", rows, ref["rows"], yard["rows"])
    _check(case, "total", out4[0], ref["total"], yard["total"])
    _check(case, "dsims", sims, ref["ds"], yard["ds"])
    # (dLoss/dT is a rounding residue here - sum_j p_j s_j = s_pos in every row, whose non-self maxima all hold s_pos - and is not compared)
    d = sims.cpu()
    nonself = torch.ones(N1, N2, dtype=torch.bool)
    nonself[idx, own] = False
    has_plus = ((s == 1.0) & nonself).any(1)
    assert has_plus.tolist() == [True] * 5 + [False]
    zero = (s == -1.0) & nonself & has_plus[:, None]
    assert bool(zero.any()) and not d[zero].any(), "dS must be exactly 0 at the -1 columns of a row that holds a +1"
    assert not d[idx, own].any() and bool((d[5][nonself[5]] != 0).all())


@pytest.mark.parametrize("what", ["odd_rows", "no_rows", "block_past_the_columns", "negative_target0", "bf16_sims", "two_element_temperature",
                                  "columns_past_int32"])
def test_ntxent_rows_refusals_launch_nothing(ops, what):
    s = torch.randn(4, 9, generator=torch.Generator().manual_seed(5)).cuda()
    before = s.clone()
    t = _dev(0.1)
    if what == "odd_rows":
        with pytest.raises(ValueError, match="ntxent_rows: N1 = 3 is odd"):
            ops.ntxent_rows(s[:3], t, 0)
    elif what == "no_rows":
        with pytest.raises(RuntimeError, match="ntxent_rows: N1 = 0 rows"):
            ops.ntxent_rows(s[:0], t, 0)
    elif what == "block_past_the_columns":
        with pytest.raises(RuntimeError, match="ntxent_rows: own block"):
            ops.ntxent_rows(s, t, 6)
    elif what == "negative_target0":
        with pytest.raises(RuntimeError, match="ntxent_rows: own block"):
            ops.ntxent_rows(s, t, -1)
    elif what == "bf16_sims":
        h = s.bfloat16()
        hb = h.clone()
        with pytest.raises(TypeError, match="ntxent_rows: sims must be fp32"):
            ops.ntxent_rows(h, t, 0)
        torch.cuda.synchronize()
        assert torch.equal(h, hb)
    elif what == "two_element_temperature":
        with pytest.raises(ValueError, match="ntxent_rows: temperature holds one element"):
            ops.ntxent_rows(s, torch.tensor([0.1, 0.1]).cuda(), 0)
    else:
        # the C entry itself: an odd row count, and a column count the kernel's 32-bit indices cannot hold (refused before any launch)
        from simseg_amd.lib import call, ptr, stream
        scratch, out4 = torch.zeros(3, 4).cuda(), torch.zeros(4).cuda()
        with pytest.raises(RuntimeError, match="ntxent_rows: N1 = 3 is odd"):
            call("simseg_ntxent_rows", ptr(s), ptr(t), ptr(scratch[0]), ptr(scratch[1]), ptr(scratch[2]), ptr(out4), 3, 9, 0, 1, stream())
        with pytest.raises(RuntimeError, match="ntxent_rows: N2 = 2147483648 columns"):
            call("simseg_ntxent_rows", ptr(s), ptr(t), ptr(scratch[0]), ptr(scratch[1]), ptr(scratch[2]), ptr(out4), 4, 2 ** 31, 0, 1, stream())
    torch.cuda.synchronize()
    assert torch.equal(s, before)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the autograd node against float64 autograd of the torch statement
# ------------------------------------------------------------------------------------------------------------------------------------------
UP = 3.0          # the upstream gradient


def _head_eval(z32, g32, T, rank, dtype, device):
    """g32 None: single process, the same tensor in both roles."""
    z = z32.to(device=device, dtype=dtype).requires_grad_(True)
    g = z if g32 is None else g32.to(device=device, dtype=dtype).requires_grad_(True)
    t = torch.tensor(T, dtype=torch.float32).to(device=device, dtype=dtype).requires_grad_(True)
    s = z @ g.T
    loss = N.ntxent_torch(s, t, rank * z.shape[0])
    (UP * loss).backward()
    return {"loss": loss.detach(), "dz": z.grad, "dg": None if g32 is None else g.grad, "dt": t.grad, "s": s.detach()}


def _accs(s64, T, target0):
    r = N.ntxent_eval(s64, T, target0)
    assert N.margin_ok(r["z"]), "pick another seed"
    return r["acc_a"], r["acc_b"]


@pytest.mark.parametrize("T", [0.1, 0.05])
@pytest.mark.parametrize("B,P", N.HEAD_SHAPES)
def test_ntxent_fn_vs_float64(ops, B, P, T):
    """rank 1 of 3 with a hand-built gathered matrix; gradients w.r.t. the stacked local embeddings, the gathered ones (other ranks' rows
    included) and the temperature."""
    from simseg_amd import heads
    a, b, gathered = N.head_embeddings(B, P, N.HEAD_SEEDS[B, P])
    z32 = torch.cat([a, b])
    ref = _head_eval(z32, gathered, T, 1, torch.float64, "cpu")
    yard = _head_eval(z32, gathered, T, 1, torch.float32, "cuda")
    acc = _accs(ref["s"], T, 2 * B)
    z, g = z32.cuda().requires_grad_(True), gathered.cuda().requires_grad_(True)
    t = torch.tensor(T).cuda().requires_grad_(True)
    loss, acc_a, acc_b = heads.NTXentFn.apply(z, g, t, 1)
    assert not acc_a.requires_grad and not acc_b.requires_grad
    (loss * UP).backward()
    case = f"NTXentFn B={B} P={P} T={T:g} rank 1/3"
    _check(case, "loss", loss, ref["loss"], yard["loss"])
    _check(case, "dz", z.grad, ref["dz"], yard["dz"])
    _check(case, "dzg", g.grad, ref["dg"], yard["dg"])
    _check(case, "dT", t.grad, ref["dt"], yard["dt"])
    assert (acc_a.item(), acc_b.item()) == acc
    assert t.grad.shape == () and loss.shape == ()


@pytest.mark.parametrize("B,P", N.HEAD_SHAPES)
def test_ntxent_fn_single_process(ops, B, P):
    """No process group: the same tensor in both roles, autograd adds the two gradients."""
    from simseg_amd import heads
    T = 0.1
    a, b, _ = N.head_embeddings(B, P, N.HEAD_SEEDS[B, P])
    z32 = torch.cat([a, b])
    ref = _head_eval(z32, None, T, 0, torch.float64, "cpu")
    yard = _head_eval(z32, None, T, 0, torch.float32, "cuda")
    acc = _accs(ref["s"], T, 0)
    z = z32.cuda().requires_grad_(True)
    t = torch.tensor(T).cuda().requires_grad_(True)
    loss, acc_a, acc_b = heads.NTXentFn.apply(z, z, t, 0)
    (loss * UP).backward()
    case = f"NTXentFn B={B} P={P} T={T:g} single"
    _check(case, "loss", loss, ref["loss"], yard["loss"])
    _check(case, "dz", z.grad, ref["dz"], yard["dz"])
    _check(case, "dT", t.grad, ref["dt"], yard["dt"])
    assert (acc_a.item(), acc_b.item()) == acc
    if B == 1:          # one other row: nothing to learn
        assert loss.item() == 0.0 and not z.grad.any() and t.grad.item() == 0.0


def test_ntxent_fn_returns_none_for_inputs_that_need_no_gradient(ops):
    from simseg_amd import heads
    a, b, gathered = N.head_embeddings(3, 64, 1)
    z = torch.cat([a, b]).cuda().requires_grad_(True)
    g, t = gathered.cuda(), torch.tensor(0.1).cuda()
    loss, _, _ = heads.NTXentFn.apply(z, g, t, 1)
    loss.backward()
    assert z.grad is not None and g.grad is None and t.grad is None
    with torch.no_grad():
        l2, _, _ = heads.NTXentFn.apply(z, g, t, 1)
    assert torch.equal(l2, loss.detach())          # (the forward without the gradient pass computes the same bits)


# ------------------------------------------------------------------------------------------------------------------------------------------
# through the LOSS module
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P", [(17, 128), (49, 128)])
def test_loss_module_is_symmetric_in_its_views(ops, B, P):
    import os

    import simseg.models  # noqa: F401
    from conftest import REPO
    from simseg.core.config import update_cfg
    from simseg.models.criteria.losses.builder import LOSS
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), [], update_clip_config)
    m = LOSS.get("NTXent")(cfg, 0, temperature=0.1, learnable=False).cuda()
    a, b, _ = N.head_embeddings(B, P, 1)
    a, b = a.cuda(), b.cuda()
    lab, acc_ab = m(a, b)
    lba, acc_ba = m(b, a)
    z32 = torch.cat([a, b]).cpu()
    ref = _head_eval(z32, None, 0.1, 0, torch.float64, "cpu")
    yard = _head_eval(z32, None, 0.1, 0, torch.float32, "cuda")
    case = f"LOSS.NTXent B={B} P={P}"
    _check(case, "(a,b)", lab, ref["loss"], yard["loss"])
    _check(case, "(b,a)", lba, ref["loss"], yard["loss"])
    _check(case, "swap", lba, lab.double(), yard["loss"] - ref["loss"].cuda() + lab.double())          # the two calls against each other, same yardstick
    acc = _accs(ref["s"], 0.1, 0)
    assert (acc_ab.item(), acc_ba.item()) == acc
