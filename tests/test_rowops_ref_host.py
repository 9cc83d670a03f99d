"""CPU tests of tests/_rowops_ref.py: the float64 references against autograd, the condition under which the per-cell rule is a fair one
(an honest fp32 evaluation in the kernels' order stays within HALF of every bound, for every toleranced case of test_gpu_rowops.py), and
the judges' ability to fail: restatements with one defect each are rejected, on a case that the whole-tensor gate of
test_gpu_kernels.py (_close, at the tolerance that file uses) lets through."""
import pytest
import torch
import torch.nn.functional as F

import _rowops_ref as R

H = torch.bfloat16


def _fwd_ratios(x, g, b, eps, defect=None):
    """Worst ratio of the restated forward per output, the yardstick being fp32 torch on the CPU."""
    want = R.ln_fwd(x, g, b, eps)
    yard = R.ln_fwd(x, g, b, eps, dtype=torch.float32)
    got = R.ln_fwd_restated(x, g, b, eps, defect)
    return {"y": R.judge(got[0], want[0], yard[0], -1)[0], "mean": R.judge(got[1], want[1], yard[1], None)[0],
            "rstd": R.judge(got[2], want[2], yard[2], None)[0]}, got, want


def test_ulp_and_judge():
    assert R.ulp(torch.tensor([0.0, 1.0, 1.5, 0.75, 2.0 ** -140])).tolist() == [0.0, 2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -149]
    assert R.ulp(torch.tensor([1.0, 3.0]), torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -6]
    assert R.ulp(torch.tensor([1.0]), torch.float16).item() == 2.0 ** -10
    want = torch.tensor([[1.0, 0.5], [0.0, 0.0]], dtype=torch.float64)
    exact = want.float()
    assert R.judge(exact, want, exact, -1) == (0.0, 2)
    off = exact.clone()
    off[0, 1] += 2.0 ** -21                                  # 4 ulps at the row's largest magnitude: on the bound
    assert R.judge(off, want, exact, -1)[0] == 1.0
    off[1, 0] = 1e-30                                        # a zero row has a zero bound
    assert R.judge(off, want, exact, -1)[0] == float("inf")
    assert R.judge(torch.tensor([float("nan")]), want[0, :1], exact[0, :1], None)[0] == float("inf")
    # a column sum's floor is stated in the sum of |terms|, and half an ulp of H is granted element by element
    assert R.judge(torch.tensor([1e-6]), torch.zeros(1, dtype=torch.float64), torch.zeros(1), None, mag=torch.tensor([4.0]))[0] < 1.0
    assert R.judge(torch.tensor([[1.0 + 2.0 ** -8]]), torch.ones(1, 1, dtype=torch.float64), torch.ones(1, 1), -1, half=H)[0] < 1.0
    assert R.judge(torch.tensor([[1.0 + 2.0 ** -7]]), torch.ones(1, 1, dtype=torch.float64), torch.ones(1, 1), -1, half=H)[0] > 1.0


@pytest.mark.parametrize("rows,D", [(5, 100), (33, 260)])
def test_float64_backward_equals_autograd(rows, D):
    x = R.ln_rows("plain", rows, D, 3).double().requires_grad_(True)
    g, b = (t.double().requires_grad_(True) for t in R.ln_gains(D, 4, mixed=True))
    dy = torch.randn(rows, D, generator=R.gen(5), dtype=torch.float64)
    F.layer_norm(x, (D,), g, b, 1e-6).backward(dy)
    _, mean, rstd = R.ln_fwd(x.detach(), g.detach(), b.detach(), 1e-6)
    xh = (x.detach() - mean[:, None]) * rstd[:, None]
    got = R.ln_bwd([dy], xh, rstd, g.detach())
    for k, w in (("dx", x.grad), ("dgamma", g.grad), ("dbeta", b.grad)):
        assert (got[k] - w).abs().max().item() <= 1e-12 * w.abs().max().item(), k
    assert torch.equal(got["dxsum"], got["dx"].sum(0))
    # ... and the law of the y16 path is the same function wherever y16 is the unrounded output
    y = R.ln_fwd(x.detach(), g.detach(), b.detach(), 1e-6)[0]
    xy = R.ln_xhat(x.detach(), mean, rstd, g.detach(), b.detach(), y16=y)
    ok = R.y16_chunks(g.detach(), b.detach())
    assert ok.any() and not ok.all() and torch.equal(xy[:, ~ok], xh[:, ~ok])
    assert (xy - xh).abs().max().item() <= 1e-9


@pytest.mark.parametrize("normalize", [0, 1])
def test_float64_pooling_equals_autograd(normalize):
    B, N, P, k, eps = 3, 33, 64, 3, 1e-8
    tok = R.pool_tokens(B, N, P, torch.float32, 6).double().requires_grad_(True)
    top = tok.topk(k, dim=1)[0].mean(1)
    emb = top / (top.norm(dim=-1, keepdim=True) + eps) if normalize else top
    demb = torch.randn(B, P, generator=R.gen(7), dtype=torch.float64)
    emb.backward(demb)
    vals, idx = R.pool_select(tok.detach(), None, k)
    assert torch.equal(vals, tok.detach().gather(1, idx).float())
    e, n = R.pool_fwd(tok.detach().gather(1, idx), eps, normalize)
    assert (e - emb.detach()).abs().max().item() <= 1e-12 * emb.detach().abs().max().item()
    dense = R.pool_scatter(R.pool_bwd(demb, e, n, k, eps, normalize), idx, N)
    assert (dense - tok.grad).abs().max().item() <= 1e-12 * tok.grad.abs().max().item()


@pytest.mark.parametrize("rows,D", R.LN_FWD_CASES)
def test_forward_restatement_stays_within_half_of_every_bound(rows, D):
    g, b = R.ln_gains(D, 2)
    worst = {}
    for family in R.families_for(D):
        x = R.ln_rows(family, rows, D, 1)
        sd = x.double().std(-1, unbiased=False) if D > 1 else None
        assert bool((x.double().mean(-1).abs() <= 2 * sd).all()), "a toleranced row's mean is more than 2 sigma from 0"
        for eps in R.LN_EPS:
            ratios, _, _ = _fwd_ratios(x, g, b, eps)
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    assert max(worst.values()) <= 0.5, worst
    for first in (0.0, 3.0):                                   # the exact rows: y = beta bit for bit, mean exact
        for eps in R.LN_EPS:
            y, mean, _ = R.ln_fwd_restated(R.ln_exact_rows(rows, D, first), g, b, eps)
            assert torch.equal(y, b.expand(rows, D)) and set(mean.tolist()) <= {0.0, 3.0}


def _bwd_ratios(op, half=None, defect=None):
    want = R.ln_bwd_eval(op)
    yard = R.ln_bwd_eval(op, dtype=torch.float32)
    xh32 = R.ln_xhat(op["x"], op["mean"], op["rstd"], op["g"], op["b"], op["y16"], torch.float32)
    got = R.ln_bwd_restated([t for t in (op["dy16"], op["dy32"]) if t is not None], xh32, op["rstd"], op["g"],
                            [t for t in (op["dres"], op["dres16"]) if t is not None], op["init"], defect)
    out = {"dx": R.judge(got["dx"], want["dx"], yard["dx"], -1)[0]}
    for i, k in enumerate(("dgamma", "dbeta")):
        out[k] = R.judge(got[k], want[k], yard[k], None, mag=want["mag"][i])[0]
    if half is None:                                           # the generic kernel's cases: the fp32 dx is written too
        out["dxsum"] = R.judge_sum_of(got["dx"], op["init"][2], got["dxsum"])[0]
    else:                                                      # the step form: the rounding, and dxsum against float64 (R.ln_step_dxsum_extra)
        out["dx16"] = R.judge(got["dx"].to(half), want["dx"], yard["dx"], -1, half=half)[0]
        out["dxsum"] = R.judge(got["dxsum"], want["dxsum"], yard["dxsum"], None, mag=want["mag"][2], extra=R.ln_step_dxsum_extra(want, yard))[0]
    return out, got, want


@pytest.mark.parametrize("rows,D", R.ln_bwd_shapes(R.LN_BWD_WIDTHS))
def test_backward_restatement_stays_within_half_of_every_bound(rows, D):
    for form in R.LN_BWD_FORMS:
        for mixed in ((False, True) if form.endswith("y16") else (False,)):
            op = R.ln_bwd_case(rows, D, R.ln_bwd_family(rows, D), form, mixed, H, R.ln_bwd_seed(rows, D))
            ratios, _, _ = _bwd_ratios(op)
            assert max(ratios.values()) <= 0.5, (form, mixed, ratios)


@pytest.mark.parametrize("rows,D", R.ln_bwd_shapes(R.LN_BWD16_FULL + R.LN_BWD16_RAGGED))
def test_step_form_restatement_stays_within_half_of_every_bound(rows, D):
    for mixed in (False, True):
        op = R.ln_bwd_case(rows, D, R.ln_bwd_family(rows, D), "dy16+dres16+y16", mixed, H, R.ln_bwd_seed(rows, D))
        assert bool(R.y16_chunks(op["g"], op["b"]).all()) != mixed
        ratios, _, _ = _bwd_ratios(op, half=H)
        dx16 = ratios.pop("dx16")                            # the fp32 values within half of the fp32 bounds, and their rounding within
        assert max(ratios.values()) <= 0.5 and dx16 <= 1.0, (mixed, ratios, dx16)      # the half ulp of H granted for exactly that


# ------------------------------------------------------------------------------------------------------------------------------------------
# the judges must be able to fail
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_rejects_variance_over_d_minus_1():
    """(4, 2048): a relative 1.2e-4 in rstd.  The old gate of the 16-bit forward output (1e-2 of the tensor's scale) lets it through; here
    that output must equal the rounded fp32 one, and the fp32 one fails in every row."""
    g, b = R.ln_gains(2048, 2)
    x = R.ln_rows("plain", 4, 2048, 1)
    ratios, got, want = _fwd_ratios(x, g, b, 1e-6, "bessel")
    assert ratios["y"] > 1.0 and ratios["rstd"] > 1.0 and ratios["mean"] <= 0.5, ratios
    assert R.old_close(got[0].to(H), want[0], 1e-2)
    assert max(_fwd_ratios(x, g, b, 1e-6)[0].values()) <= 0.5


def test_rejects_a_missing_eps_on_a_small_row():
    """eps = 1e-12 left out of a sigma = 1e-3 row: 5e-7 of rstd.  The whole-tensor gate at 1e-5 passes y; the row's rstd fails."""
    g, b = R.ln_gains(64, 2)
    x = (torch.randn(2, 64, generator=R.gen(1)) + 0.5) * 1e-3
    ratios, got, want = _fwd_ratios(x, g, b, 1e-12, "no_eps")
    assert ratios["rstd"] > 1.0, ratios
    assert R.old_close(got[0], want[0], 1e-5) and R.old_close(got[2], want[2], 1e-5)
    assert max(_fwd_ratios(x, g, b, 1e-12)[0].values()) <= 0.5


def test_rejects_the_odd_tail_row_with_its_neighbours_mean():
    """(9, 384) with row scales that fall from 1e3 to 1e-3: the tail row's saved mean is wrong by its neighbour's, 1e-6 of the tensor's
    largest mean - invisible to a pooled maximum, and caught in its own row (mean and y)."""
    g, b = R.ln_gains(384, 2)
    x = R.ln_rows("scales", 9, 384, 1).flip(0).contiguous()
    ratios, got, want = _fwd_ratios(x, g, b, 1e-12, "tail_mean")
    assert ratios["mean"] > 1.0 and ratios["y"] > 1.0, ratios
    assert R.old_close(got[1], want[1], 1e-5)
    assert max(_fwd_ratios(x, g, b, 1e-12)[0].values()) <= 0.5


def test_rejects_a_row_missing_from_dgamma():
    """33 rows, row 1's gradient 1e-4 of the others': its contribution is below the whole-tensor 1e-4 gate and above its columns' bounds."""
    op = dict(R.ln_bwd_case(33, 260, "plain", "dy32", False, H, 1))
    dy = op["dy32"].clone()
    dy[1] *= 1e-4
    op["dy32"] = dy
    ratios, got, want = _bwd_ratios(op, defect="drop_row")
    assert ratios["dgamma"] > 1.0 and max(ratios["dx"], ratios["dbeta"], ratios["dxsum"]) <= 0.5, ratios
    assert R.old_close(got["dgamma"], want["dgamma"], 1e-4)
    assert max(_bwd_ratios(op)[0].values()) <= 0.5


def test_rejects_xhat_rounded_to_bf16_on_the_x_path():
    """The old gates of the 16-bit dx (1e-2) and of dgamma on the y16 path (5e-3) pass; the fp32 dx fails its rows, dgamma its columns."""
    op = R.ln_bwd_case(33, 768, "plain", "dy16+dres16", False, H, 1)
    ratios, got, want = _bwd_ratios(op, defect="xhat_bf16")
    assert ratios["dx"] > 1.0 and ratios["dgamma"] > 1.0, ratios
    assert R.old_close(got["dx"].to(H), want["dx"], 1e-2) and R.old_close(got["dgamma"], want["dgamma"], 5e-3)


def _pool_outputs(tok, mask, k, **defect):
    vals, idx = R.pool_select(tok, mask, k, **defect)
    return idx, R.pool_fwd(vals, 1e-8, 0, dtype=torch.float32)[0]


def test_rejects_a_tie_broken_towards_the_larger_index():
    B, N, P, k = 2, 33, 192, 3
    tok = R.pool_tokens(B, N, P, H, 2)
    idx, emb = _pool_outputs(tok, None, k)
    bad_idx, bad_emb = _pool_outputs(tok, None, k, tie="last")
    assert not torch.equal(bad_idx, idx)                      # the exact comparison of the indices is the judge here
    assert torch.equal(bad_emb, emb)                          # ... the tie-invariant quantities of the old test cannot tell
    assert torch.equal(tok.float().gather(1, bad_idx).sum(1), tok.float().topk(k, dim=1)[0].sum(1))
    v = tok.float()                                           # and the reference order is (value descending, index ascending)
    sel = v.gather(1, idx)
    assert bool(((sel[:, :-1] > sel[:, 1:]) | ((sel[:, :-1] == sel[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))).all())


def test_rejects_a_masked_token_treated_as_unmasked():
    """Batch row 1 holds values 1e-6 of row 0's: one leaked token there moves emb by 1e-6 of the tensor's scale and by many bounds of
    its own row."""
    B, N, P, k = 2, 33, 192, 3
    tok = R.pool_tokens(B, N, P, torch.float32, 2) * torch.tensor([1.0, 1e-4])[:, None, None]      # (row 1 is 1e-2 already)
    mask = R.pool_mask("prefix", B, N, k, 3)
    leak = (1, int(mask[1].sum()))                            # the first masked token of batch row 1
    assert mask[leak] == 0
    idx, emb = _pool_outputs(tok, mask, k)
    bad_idx, bad_emb = _pool_outputs(tok, mask, k, leak=leak)
    want = R.pool_fwd(R.pool_select(tok, mask, k)[0], 1e-8, 0)[0]
    assert not torch.equal(bad_idx, idx)
    assert R.judge(bad_emb, want, emb, -1)[0] > 1.0 and R.judge(emb, want, emb, -1)[0] <= 0.5
    assert torch.equal(bad_emb[0], emb[0]) and R.old_close(bad_emb, want, 1e-5)
