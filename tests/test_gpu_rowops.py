"""The kernels of csrc/rowops.hip on MI355X, judged per cell against float64: LayerNorm forward (ln_fwd2_kernel / ln_fwd_kernel), LayerNorm
backward (ln_bwd_kernel in every MAXC instantiation and operand form, ln_bwd16_kernel FULL and ragged, ln_bwd_reduce_kernel and the
atomic path without partials), top-k pooling (single pass, sliced + merged, backward), column sums, row_rnorm, and bit for bit the
kernels that only move data (im2col, [cls] rows, BERT embedding gather / scatter).

The rule, the references, the inputs and the case tables are tests/_rowops_ref.py's (read its docstring first); tests/
test_rowops_ref_host.py shows on the CPU that the rule is fair to an honest fp32 evaluation and that it rejects seven planted defects.
Every toleranced check prints one `rowops |` line (worst ratio error / bound over its cells, cells judged) before it asserts;
profiles/rowops_tests.txt is that table."""
import pytest
import torch

import _rowops_ref as R

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
SENT32, SENT16 = 0x7FC0BEEF, 0x7FC1          # NaN bit patterns in fp32 and in both 16-bit types


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _name(dtype):
    return {torch.float32: "fp32", BF16: "bf16", FP16: "fp16"}[dtype]


def _rule(case, what, got, want, yard, dim, **kw):
    ratio, cells = R.judge(got, want, yard, dim, **kw)
    print(R.line(case, what, ratio, cells))
    assert ratio <= 1.0, f"{case} {what}: worst cell at {ratio:.3f} of its bound ({cells} cells)"


def _bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                       b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32)), what


def _carve(rows, D, dtype):
    """A [rows, D] output inside a sentinel-filled buffer with one spare row on each side -> (buffer as integers, the view)."""
    it, sent = (torch.int32, SENT32) if dtype == torch.float32 else (torch.int16, SENT16)
    buf = torch.full((rows + 2, D), sent, dtype=it, device="cuda")
    return buf, buf.view(dtype)[1:rows + 1]


def _spare_untouched(buf, what):
    sent = SENT32 if buf.dtype == torch.int32 else SENT16
    assert bool((buf[0] == sent).all()) and bool((buf[-1] == sent).all()), f"{what}: a spare row was written"


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. LayerNorm forward
# ------------------------------------------------------------------------------------------------------------------------------------------
def _ln_fwd_c(ops, x, g, b, eps, half, sixteen_only, what):
    """simseg_layernorm_fwd into carved buffers.  sixteen_only: y in `half`, no copy, no statistics; otherwise fp32 y, a `half` copy, mean
    and rstd.  -> (y, y16, mean, rstd) on the device, the spare rows checked."""
    from simseg_amd.lib import call, ptr, stream
    rows, D = x.shape
    by, y = _carve(rows, D, half if sixteen_only else torch.float32)
    bufs = [by]
    y16 = mean = rstd = None
    if not sixteen_only:
        b16, y16 = _carve(rows, D, half)
        bm, mean = _carve(rows, 1, torch.float32)
        br, rstd = _carve(rows, 1, torch.float32)
        bufs += [b16, bm, br]
    call("simseg_layernorm_fwd", ptr(x), ptr(g), ptr(b), ptr(y), ops.dt(y), ptr(y16), ptr(mean), ptr(rstd), rows, D, float(eps), stream())
    torch.cuda.synchronize()
    for bf in bufs:
        _spare_untouched(bf, what)
    return y, y16, None if mean is None else mean[:, 0], None if rstd is None else rstd[:, 0]


def _ln_fwd_case(ops, rows, D, half):
    g, b = R.ln_gains(D, 2)
    gd, bd = g.cuda(), b.cuda()
    for family in R.families_for(D):
        x = R.ln_rows(family, rows, D, 1)
        xd = x.cuda()
        for eps in R.LN_EPS:
            case = f"ln_fwd {rows}x{D} {family} eps={eps:g} {_name(half)}"
            want = R.ln_fwd(x, g, b, eps)
            yard = R.ln_fwd(x, g, b, eps, dtype=torch.float32, device="cuda")
            y, y16, mean, rstd = _ln_fwd_c(ops, xd, gd, bd, eps, half, False, case)
            _rule(case, "y", y, want[0], yard[0], -1)
            _rule(case, "mean", mean, want[1], yard[1], None)
            _rule(case, "rstd", rstd, want[2], yard[2], None)
            _bits(y16, y.to(half), f"{case}: the 16-bit copy is the rounded fp32 output")
            yo, _, _, _ = _ln_fwd_c(ops, xd, gd, bd, eps, half, True, case)
            _bits(yo, y.to(half), f"{case}: the 16-bit-only output is the rounded fp32 output")
        w = ops.layernorm_fwd(xd, gd, bd, 1e-12, want_bf16_copy=half, save_stats=True)          # (eps = the loop's last)
        for a, c, n in zip(w, (y, y16, mean, rstd), ("y", "y16", "mean", "rstd")):
            _bits(a, c.contiguous(), f"ln_fwd {rows}x{D} {family}: ops.layernorm_fwd's {n}")
    for first in (0.0, 3.0):                     # all-zero and constant-3.0 rows: mean exact, y = beta bit for bit, whatever eps is
        x = R.ln_exact_rows(rows, D, first)
        for eps in R.LN_EPS:
            case = f"ln_fwd {rows}x{D} exact rows from {first} eps={eps:g} {_name(half)}"
            y, y16, mean, rstd = _ln_fwd_c(ops, x.cuda(), gd, bd, eps, half, False, case)
            assert torch.equal(mean.cpu(), x[:, 0]), f"{case}: mean"
            assert bool(torch.isfinite(rstd).all()), f"{case}: rstd"
            assert torch.equal(y.cpu(), b.expand(rows, D)), f"{case}: y is not beta"
            assert torch.equal(y16.cpu(), b.to(half).expand(rows, D)), f"{case}: the 16-bit copy is not beta"
            yo, _, _, _ = _ln_fwd_c(ops, x.cuda(), gd, bd, eps, half, True, case)
            assert torch.equal(yo.cpu(), b.to(half).expand(rows, D)), f"{case}: the 16-bit-only output is not beta"


@pytest.mark.parametrize("rows,D", R.LN_FWD_CASES)
def test_layernorm_fwd(ops, rows, D):
    """Rows 1, 2, 7, 8, 9: one wave, one block, a block and the odd tail of the two-rows-per-wave kernel (whose idle half-wave must store
    nothing: the spare row behind the last one stays untouched); widths with idle lanes, 512 | 516 across the kernel switch, 2044, 2048."""
    _ln_fwd_case(ops, rows, D, BF16)


@pytest.mark.parametrize("rows,D", R.LN_FWD_FP16_CASES)
def test_layernorm_fwd_fp16(ops, rows, D):
    _ln_fwd_case(ops, rows, D, FP16)


@pytest.mark.parametrize("D", [0, 6, 2052])
def test_layernorm_fwd_refuses_unsupported_widths(ops, D):
    from simseg_amd.lib import call, ptr, stream
    rows, W = 3, max(D, 4)
    x, g, b = (torch.ones(rows, W).cuda(), torch.ones(W).cuda(), torch.zeros(W).cuda())
    by, y = _carve(rows, W, torch.float32)
    b16, y16 = _carve(rows, W, BF16)
    bm, mean = _carve(rows, 1, torch.float32)
    with pytest.raises(RuntimeError, match="layernorm_fwd"):
        call("simseg_layernorm_fwd", ptr(x), ptr(g), ptr(b), ptr(y), 0, ptr(y16), ptr(mean), ptr(mean), rows, D, 1e-6, stream())
    torch.cuda.synchronize()
    for bf, sent in ((by, SENT32), (b16, SENT16), (bm, SENT32)):
        assert bool((bf == sent).all()), f"D={D}: a refused call wrote something"


def test_layernorm_fwd_no_rows_is_a_no_op(ops):
    from simseg_amd.lib import call, ptr, stream
    x, g, b = (torch.ones(3, 64).cuda(), torch.ones(64).cuda(), torch.zeros(64).cuda())
    by, y = _carve(3, 64, torch.float32)
    call("simseg_layernorm_fwd", ptr(x), ptr(g), ptr(b), ptr(y), 0, None, None, None, 0, 64, 1e-6, stream())
    torch.cuda.synchronize()
    assert bool((by == SENT32).all())


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm backward
# ------------------------------------------------------------------------------------------------------------------------------------------
def _ln_bwd_run(ops, op, half, want_f32, with_dxsum, drop=(0, 0.0), partials=True):
    """-> dict of device tensors dx32, dx16, dgamma, dbeta, dxsum.  partials=False: the C entry without a workspace (one atomic per column
    and block instead of ln_bwd_reduce_kernel)."""
    from simseg_amd.lib import call, ptr, stream
    d = {k: (None if v is None else v.cuda()) for k, v in op.items()}
    acc = d["init"].clone()
    dxsum = acc[2] if with_dxsum else None
    if partials:
        dx32, dx16 = ops.layernorm_bwd(d["x"], d["mean"], d["rstd"], d["g"], acc[0], acc[1], dy16=d["dy16"], dy32=d["dy32"], dres=d["dres"],
                                       want_f32=want_f32, want_bf16=half, dxsum=dxsum, drop_seed=drop[0], drop_p=drop[1], dres16=d["dres16"],
                                       y16=d["y16"], beta=d["b"])
    else:
        rows, D = d["x"].shape
        dx32 = torch.empty(rows, D, device="cuda") if want_f32 else None
        dx16 = torch.empty(rows, D, device="cuda", dtype=half)
        call("simseg_layernorm_bwd", ptr(d["dy16"]), ptr(d["dy32"]), ptr(d["dres"]), ptr(d["dres16"]), ptr(d["x"]), ptr(d["y16"]),
             ptr(d["b"]) if d["y16"] is not None else None, ptr(d["mean"]), ptr(d["rstd"]), ptr(d["g"]), ptr(dx32), ptr(dx16), ptr(acc[0]), ptr(acc[1]),
             ptr(dxsum), None, rows, D, int(drop[0]), float(drop[1]), stream())
    return {"dx32": dx32, "dx16": dx16, "dgamma": acc[0], "dbeta": acc[1], "dxsum": dxsum}


def _ln_bwd_generic_case(ops, rows, D, form, mixed, half, with_dxsum=True, drop=(0, 0.0), partials=True):
    op = R.ln_bwd_case(rows, D, R.ln_bwd_family(rows, D), form, mixed, half, R.ln_bwd_seed(rows, D))
    case = (f"ln_bwd {rows}x{D} {form}{' mixed' if mixed else ''} {_name(half)}" + ("" if with_dxsum else " -dxsum") +
            (f" p={drop[1]}" if drop[1] else "") + ("" if partials else " atomics"))
    want = R.ln_bwd_eval(op)
    yard = R.ln_bwd_eval(op, dtype=torch.float32, device="cuda")
    got = _ln_bwd_run(ops, op, half, True, with_dxsum, drop, partials)          # (an fp32 dx wanted: never the 16-bit step kernel)
    _rule(case, "dx", got["dx32"], want["dx"], yard["dx"], -1)
    _rule(case, "dgamma", got["dgamma"], want["dgamma"], yard["dgamma"], None, mag=want["mag"][0])
    _rule(case, "dbeta", got["dbeta"], want["dbeta"], yard["dbeta"], None, mag=want["mag"][1])
    written = got["dx32"]
    if drop[1]:                                  # the 16-bit copy and the column sums carry the dense layer's mask, the fp32 stream never
        keep = torch.ones(rows, D, device="cuda")
        ops.dropout_apply_(keep, drop[0], drop[1])
        assert 0 < int((keep == 0).sum()) < keep.numel() // 4 and len(keep.unique()) == 2
        written = torch.where(keep == 0, torch.zeros_like(keep), got["dx32"] * keep)        # (a dropped value is +0, not dx * 0)
    _bits(got["dx16"], written.to(half), f"{case}: the 16-bit dx is the rounded (masked) fp32 dx")
    if with_dxsum:
        ratio, cells = R.judge_sum_of(written, op["init"][2], got["dxsum"], device="cuda")
        print(R.line(case, "dxsum", ratio, cells))
        assert ratio <= 1.0, f"{case} dxsum: worst column at {ratio:.3f} of its bound"


@pytest.mark.parametrize("form", R.LN_BWD_FORMS)
@pytest.mark.parametrize("rows,D", R.ln_bwd_shapes(R.LN_BWD_WIDTHS))
def test_layernorm_bwd_generic(ops, rows, D, form):
    """ln_bwd_kernel<1, 2, 3, 4, 8> (an fp32 dx is always wanted, which keeps the y16 form off the step kernel), 1 / 5 / 33 rows and the
    8200 x 64 case whose row loop wraps, with and without dxsum; the y16 form also with mixed gains (a tiny |gamma| and a large beta, whose
    chunks read x, and a negative eligible gamma)."""
    for mixed in ((False, True) if form.endswith("y16") else (False,)):
        for with_dxsum in (True, False):
            _ln_bwd_generic_case(ops, rows, D, form, mixed, BF16, with_dxsum)


@pytest.mark.parametrize("rows,D,form", [(33, 260, "dy16+dy32+dres"), (5, 768, "dy16+dres16+y16")])
def test_layernorm_bwd_generic_dropout_atomics_fp16(ops, rows, D, form):
    """Dropout 0.1 re-applied to the 16-bit copy (mask regenerated with dropout_apply_ on ones; dxsum sums the masked values before their
    rounding), the column reductions through atomics instead of the partials workspace, and the fp16 flavour."""
    _ln_bwd_generic_case(ops, rows, D, form, False, BF16, drop=(77, 0.1))
    _ln_bwd_generic_case(ops, rows, D, form, True if form.endswith("y16") else False, BF16, partials=False)
    _ln_bwd_generic_case(ops, rows, D, form, False, FP16)
    _ln_bwd_generic_case(ops, rows, D, form, False, FP16, drop=(78, 0.1), partials=False)


def _ln_bwd_step_case(ops, rows, D, mixed, half):
    op = R.ln_bwd_case(rows, D, R.ln_bwd_family(rows, D), "dy16+dres16+y16", mixed, half, R.ln_bwd_seed(rows, D))
    assert bool(R.y16_chunks(op["g"], op["b"]).all()) != mixed
    case = f"ln_bwd16 {rows}x{D}{' mixed' if mixed else ''} {_name(half)}"
    want = R.ln_bwd_eval(op)
    yard = R.ln_bwd_eval(op, dtype=torch.float32, device="cuda")
    got = _ln_bwd_run(ops, op, half, False, True)
    assert got["dx32"] is None
    _rule(case, "dx16", got["dx16"], want["dx"], yard["dx"], -1, half=half)
    _rule(case, "dgamma", got["dgamma"], want["dgamma"], yard["dgamma"], None, mag=want["mag"][0])
    _rule(case, "dbeta", got["dbeta"], want["dbeta"], yard["dbeta"], None, mag=want["mag"][1])
    _rule(case, "dxsum", got["dxsum"], want["dxsum"], yard["dxsum"], None, mag=want["mag"][2], extra=R.ln_step_dxsum_extra(want, yard))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("rows,D", R.ln_bwd_shapes(R.LN_BWD16_FULL + R.LN_BWD16_RAGGED))
def test_layernorm_bwd_16bit_step_form(ops, rows, D, mixed):
    """ln_bwd16_kernel: dy16 + y16 + dres16 -> dx16 and nothing in fp32.  FULL widths (no lane predicate) and ragged ones (clamped
    addresses, masked values), one wave to a wrapped row loop, every gain eligible (no x read at all) and mixed (needx)."""
    _ln_bwd_step_case(ops, rows, D, mixed, BF16)


@pytest.mark.parametrize("rows,D", [(5, 768), (33, 260)])
def test_layernorm_bwd_16bit_step_form_fp16(ops, rows, D):
    for mixed in (False, True):
        _ln_bwd_step_case(ops, rows, D, mixed, FP16)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. top-k pooling
# ------------------------------------------------------------------------------------------------------------------------------------------
def _pool_fwd_c(tok, mask, k, eps, normalize, sliced):
    from simseg_amd.lib import call, ptr, raw, stream
    B, N, P = tok.shape
    emb = torch.full((B, P), float("nan"), device="cuda")
    idx = torch.full((B, k, P), -7, device="cuda", dtype=torch.int32)
    norm = torch.full((B,), float("nan"), device="cuda")
    scratch = torch.empty(raw("simseg_topk_pool_workspace_bytes", B, P, k) // 4, device="cuda") if sliced else None
    call("simseg_topk_pool_l2norm_fwd", ptr(tok), 0 if tok.dtype == torch.float32 else 1, ptr(mask), ptr(emb), ptr(idx), ptr(norm), ptr(scratch),
         B, N, P, k, float(eps), int(normalize), stream())
    return emb, idx, norm


@pytest.mark.parametrize("dtype", [torch.float32, BF16, FP16], ids=_name)
@pytest.mark.parametrize("B,N,P,k", R.POOL_CASES)
def test_topk_pool(ops, B, N, P, k, dtype):
    """Single pass and sliced + merged form on every case (N < 32 leaves slices empty; k = N; k = POOL_MAXK; P = 1024), the selected
    indices exactly the stable descending sort's (value descending, index ascending - 16-bit tokens lie on a grid of halves, ties
    everywhere), the two forms bit-identical, emb / norm and the backward per batch row."""
    eps = 1e-8
    tok = R.pool_tokens(B, N, P, dtype, 7)
    tokd = tok.cuda()
    demb = torch.randn(B, P, generator=R.gen(8))
    for kind in R.POOL_MASKS:
        mask = R.pool_mask(kind, B, N, k, 9)
        maskd = None if mask is None else mask.cuda()
        vals, idx = R.pool_select(tok, mask, k)
        for normalize in (0, 1):
            case = f"topk_pool B{B} N{N} P{P} k{k} {_name(dtype)} mask={kind} norm={normalize}"
            one = _pool_fwd_c(tokd, maskd, k, eps, normalize, False)
            two = _pool_fwd_c(tokd, maskd, k, eps, normalize, True)
            assert torch.equal(one[1].cpu().long(), idx), f"{case}: selected indices (single pass)"
            assert torch.equal(two[1].cpu().long(), idx), f"{case}: selected indices (sliced)"
            _bits(one[0], two[0], f"{case}: emb of the two forms")
            _bits(one[2], two[2], f"{case}: norm of the two forms")
            want = R.pool_fwd(vals, eps, normalize)
            yard = R.pool_fwd(vals, eps, normalize, dtype=torch.float32, device="cuda")
            _rule(case, "emb", one[0], want[0], yard[0], -1)
            _rule(case, "norm", one[2], want[1], yard[1], None)
            if kind == "holes":
                w = ops.topk_pool_l2norm_fwd(tokd, k, maskd, eps, bool(normalize))
                assert all(torch.equal(a, c) for a, c in zip(w, one)), f"{case}: ops.topk_pool_l2norm_fwd"
            # backward: emb and norm are its inputs (the forward's own fp32 results, handed to kernel and reference alike)
            emb32, norm32 = one[0], one[2]
            dtok = ops.topk_pool_l2norm_bwd(demb.cuda(), emb32, norm32, one[1], N, torch.float32, eps, bool(normalize))
            sel = R.pool_scatter(torch.ones(B, P), idx, N) != 0
            assert bool((dtok.cpu()[~sel] == 0).all()), f"{case}: gradient off the selected tokens"
            wantd = R.pool_scatter(R.pool_bwd(demb, emb32.cpu(), norm32.cpu(), k, eps, normalize), idx, N)
            yardd = R.pool_scatter(R.pool_bwd(demb, emb32, norm32, k, eps, normalize, dtype=torch.float32, device="cuda").cpu(), idx, N)
            _rule(case, "dtok", dtok, wantd, yardd, (1, 2))
            for h in ((BF16, FP16) if dtype == torch.float32 else (dtype,)):
                d16 = ops.topk_pool_l2norm_bwd(demb.cuda(), emb32, norm32, one[1], N, h, eps, bool(normalize))
                _bits(d16, dtok.to(h), f"{case}: the {_name(h)} dtok is the rounded fp32 one")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. column sums and row norms
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.COLSUM_N)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_exact(ops, rows, N):
    """Multiples of 1/2: every fp32 sum is exact in any order, so the accumulation onto a prefilled `out` is compared bit for bit.  ld = N
    and ld = N + 8 (the padding columns hold 1024 and must not be read), guard columns behind out[N] untouched."""
    from simseg_amd.lib import call, ptr, stream
    x = R.half_grid((rows, N), rows * 1000 + N)
    pre = R.half_grid((N,), 5, span=64)
    want = pre + x.sum(0)
    assert torch.equal(want.double(), pre.double() + x.double().sum(0))
    for dtype in (torch.float32, BF16, FP16):
        for ld in (N, N + 8):
            buf = torch.full((rows, ld), 1024.0).to(dtype)
            buf[:, :N] = x.to(dtype)
            out = torch.full((N + 8,), 777.25)
            out[:N] = pre
            bufd, outd = buf.cuda(), out.cuda()
            call("simseg_colsum_accum", ptr(bufd), 0 if dtype == torch.float32 else 1, ptr(outd), rows, N, ld, stream())
            got = outd.cpu()
            assert torch.equal(got[:N], want), f"colsum {rows}x{N} ld={ld} {_name(dtype)}"
            assert bool((got[N:] == 777.25).all()), f"colsum {rows}x{N} ld={ld} {_name(dtype)}: guard columns"
        outd = pre.cuda()
        assert torch.equal(ops.colsum_accum(x.to(dtype).cuda(), outd).cpu(), want), f"ops.colsum_accum {rows}x{N} {_name(dtype)}"


@pytest.mark.parametrize("dtype", [torch.float32, BF16, FP16], ids=_name)
@pytest.mark.parametrize("D", R.RNORM_D)
@pytest.mark.parametrize("rows", R.RNORM_ROWS)
def test_row_rnorm(ops, rows, D, dtype):
    x = (4.0 * torch.randn(rows, D, generator=R.gen(rows + D))).to(dtype)
    _rule(f"row_rnorm {rows}x{D} {_name(dtype)}", "rnorm", ops.row_rnorm(x.cuda()), R.rnorm(x, 1e-12), R.rnorm(x, 1e-12, torch.float32, "cuda"), None)
    for eps in (1e-12, 1e-6):                    # a zero row: exactly the fp32 quotient 1 / eps
        x0 = x.clone()
        x0[rows // 2] = 0
        got = ops.row_rnorm(x0.cuda(), eps)[rows // 2].item()
        assert got == (torch.tensor(1.0) / torch.tensor(eps, dtype=torch.float32)).item(), (got, eps)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 5. the kernels that only move data, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hh,W", [(2, 32, 48), (1, 16, 16)])
def test_vit_im2col_bit_exact(ops, B, Hh, W):
    img = torch.randn(B, 3, Hh, W, generator=R.gen(1))
    gh, gw = Hh // 16, W // 16
    want = img.view(B, 3, gh, 16, gw, 16).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, 768)          # columns (c, kh, kw)
    assert torch.equal(ops.vit_im2col(img.cuda(), torch.float32).cpu(), want)
    for h in (BF16, FP16):
        assert torch.equal(ops.vit_im2col(img.cuda(), h).cpu(), want.to(h))


@pytest.mark.parametrize("B,T,D", [(1, 2, 64), (3, 5, 100), (2, 37, 384)])
def test_vit_cls_rows_bit_exact(ops, B, T, D):
    cls, pos = torch.randn(D, generator=R.gen(2)), torch.randn(T, D, generator=R.gen(3))
    x = torch.randn(B, T, D, generator=R.gen(4))
    xd = x.cuda()
    ops.vit_cls_rows(cls.cuda(), pos.cuda(), xd)
    got = xd.cpu()
    assert torch.equal(got[:, 0], (cls + pos[0]).expand(B, D)) and torch.equal(got[:, 1:], x[:, 1:])


@pytest.mark.parametrize("D", [4, 100, 128])
def test_bert_embed_fwd_bit_exact(ops, D):
    B, L, V = 3, 7, 50
    ids = torch.randint(0, V, (B, L), generator=R.gen(5))
    ids[0, 1], ids[1, 0], ids[2, 6], ids[2, 5] = -3, V, V + 5, V - 1               # below 0 and at or above the vocabulary size: clamped
    word, pos, typ = (torch.randn(n, D, generator=R.gen(6 + i)) for i, n in enumerate((V, 16, 2)))
    want = (word[ids.clamp(0, V - 1)] + typ[0]) + pos[:L][None]                  # (word + type0) + pos, in this fp32 order
    got = ops.bert_embed_fwd(ids.cuda(), word.cuda(), pos.cuda(), typ[0].contiguous().cuda())
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("D", [4, 100, 128])
def test_bert_embed_bwd_exact_grid(ops, D):
    """Repeated ids, a mask and out-of-range ids; gradients on the grid of quarters, so the order of the atomics cannot matter."""
    B, L, V = 4, 9, 6
    ids = torch.randint(0, V, (B, L), generator=R.gen(9))
    ids[0, 0], ids[3, 8] = -1, V + 2
    mask = (torch.rand(B, L, generator=R.gen(10)) < 0.7).long()
    mask[0, 0] = mask[3, 8] = 1
    dsum = torch.randint(-16, 16, (B, L, D), generator=R.gen(11)).float() / 4
    pre = torch.randint(-16, 16, (V, D), generator=R.gen(12)).float() / 4
    want = pre.clone().index_add_(0, ids.clamp(0, V - 1).view(-1), (dsum * mask[..., None]).view(-1, D))
    assert len(ids.unique()) < B * L and 0 < int(mask.sum()) < B * L
    for m, w in ((mask, want), (None, pre.clone().index_add_(0, ids.clamp(0, V - 1).view(-1), dsum.view(-1, D)))):
        dword = pre.cuda()
        ops.bert_embed_bwd(ids.cuda(), None if m is None else m.cuda(), dsum.cuda(), dword)
        assert torch.equal(dword.cpu(), w)
