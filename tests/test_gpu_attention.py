"""Attention on MI355X per sequence, head and q / k / v against float64: every kernel path of csrc/attn.hip against the plain torch
float64 reference of tests/_attn_ref.py on exactly the values the kernel receives, judged block by block - one (sequence, head,
component, 32-row tile) cell at a time, lse per (sequence, head), the bias gradient per (component, head) - by the rule written out in
tests/_attn_ref.py: the 16-bit kernels against the larger error of two fp32 emulations that round where the kernels round, the fp32
kernels against the same formula in fp32 torch (8 x + 4 ulps).  Nothing is pooled across sequences, so a one-key sequence's large dV
no longer sets the scale for the full-length sequence next to it; scale is 0.125 and 0.2; masks and dropout reach the ring forward and
the streaming backward (T > 256) too.

Every check prints one line, `attention | case | block kind | worst E_rms / Y_rms | worst E_max / Y_max | blocks | zero-reference
blocks`, before it asserts; profiles/attention_tests.txt is that table.  (batch x head) is 3, 6, 9 or 12, never a multiple of the 8 XCDs
(a case with two or four mask lengths needs B = 2 or 4)."""
import functools

import pytest
import torch

import _attn_ref as A

pytestmark = pytest.mark.gpu

DROP_SEED = 9
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
GRADS = ("out", "lse", "dq", "dk", "dv")
FWD = ("out", "lse")
_OPS = []


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    _OPS[:] = [o]
    return o


@functools.lru_cache(maxsize=None)
def _inputs(B, T, H, dt):
    """(qkv, dout) on the CPU in the type the kernel receives.  Read-only."""
    return A.randn16((B, T, 3 * H * 64), T + 11, 1.2, DT[dt]), A.randn16((B, T, H * 64), T + 12, 1.0, DT[dt])


@functools.lru_cache(maxsize=8)
def _keep(B, H, T, p):
    """The kernels' dropout keep mask [B, H, T, T] (0 or 1 / (1 - p), fp32 on the CPU), regenerated with dropout_apply_ on ones: linear
    index (bh * T + q) * T + key.  None for p = 0."""
    if p == 0.0:
        return None
    keep = _OPS[0].dropout_apply_(torch.ones(B * H * T * T, device="cuda"), DROP_SEED, p).view(B, H, T, T).cpu()
    assert abs(keep.max().item() - 1.0 / (1.0 - p)) < 1e-6 and bool(((keep == 0) | (keep == keep.max())).all())
    assert keep.numel() < 1000 or 0.5 * p < (keep == 0).float().mean().item() < 1.5 * p
    return keep


@functools.lru_cache(maxsize=8)
def _truth(B, T, H, dt, lens, p, scale, grads):
    """(float64 reference, yardsticks) of a dense case, computed once and shared by every kernel selection that runs it.  Read-only."""
    qkv, dout = _inputs(B, T, H, dt)
    dout = dout if grads else None
    keep = _keep(B, H, T, p)
    ref = A.reference(qkv, dout, H, scale, lens, keep)
    if dt == "f32":
        yards = [A.reference(qkv, dout, H, scale, lens, keep, dtype=torch.float32, device="cuda")]
    else:
        yards = [A.emulate(qkv, dout, H, scale, lens, keep, v, rnd=DT[dt], device="cuda") for v in "AB"]
    return ref, [{k: t.cpu() for k, t in y.items()} for y in yards]


def _report(case, got, ref, yards, valid, dt, kinds, lens, H, colsum=None):
    """Prints the table lines of one case, then asserts: every block within its bound, and exactly the expected blocks on the
    zero-reference path."""
    f32 = dt == "f32"
    res = A.judge_all(got, ref, yards, valid, A.PREC[DT[dt]], kinds, f32_rule=f32)
    if colsum is not None:
        res["colsum"] = A.judge_colsum(colsum, ref, yards, valid, H, f32_rule=f32)
    print()                                      # (under -s the first line would otherwise follow pytest's progress dot)
    for kind, r in res.items():
        print(f"attention | {case:<58s} | {kind:<6s} | rms {r['rms']:6.2f} | max {r['max']:6.2f} | blocks {r['blocks']:4d} | zero-ref {r['zero']:3d}")
    zero = sum(r["zero"] for r in res.values())
    want_zero = A.expected_zero_ref_blocks(lens, valid, H, colsum=colsum is not None) if "dq" in kinds else 0
    assert zero == want_zero, f"{case}: {zero} blocks took the zero-reference path, {want_zero} one-key-sequence blocks exist"
    bad = {kind: A.describe(r) for kind, r in res.items() if r["bad"]}
    assert not bad, f"{case}: " + " | ".join(f"{k}: {v}" for k, v in bad.items())


def _dense(ops, path, B, T, H, lens=None, p=0.0, scale=0.125, dt="bf16", variant=0, grads=True, colsum=False):
    """One dense case through ops.attention_fwd / attention_bwd under kernel selection `variant`."""
    qkv, dout = _inputs(B, T, H, dt)
    ref, yards = _truth(B, T, H, dt, lens, p, scale, grads)
    mask = None if lens is None else A.key_mask(lens, T).long().cuda()
    cs = torch.zeros(3 * H * 64, device="cuda") if colsum else None
    ops.set_attention_variant(variant)
    try:
        out, lse = ops.attention_fwd(qkv.cuda(), H, mask, scale=scale, save_lse=True, drop_seed=DROP_SEED, drop_p=p)
        got = {"out": A.split(out, H)[0], "lse": lse}
        if grads:
            dqkv = ops.attention_bwd(qkv.cuda(), out, dout.cuda(), lse, H, mask, scale=scale, drop_seed=DROP_SEED, drop_p=p, colsum=cs)
            got["dq"], got["dk"], got["dv"] = A.split(dqkv, H)
    finally:
        ops.set_attention_variant(0)
    if grads and lens is not None:          # a masked key's gradient is exactly zero, row by row (the block rule says so only for whole tiles)
        dead = ~A.key_mask(lens, T).cuda()[:, None, :, None]
        assert not (got["dk"] * dead).any() and not (got["dv"] * dead).any(), f"{path}: a masked key has a gradient"
    case = f"{path} {dt} B{B} H{H} T{T} {'x'.join(map(str, lens)) if lens else 'unmasked'} p={p} scale={scale}"
    _report(case, got, ref, yards, torch.ones(B, T, dtype=torch.bool), dt, GRADS if grads else FWD, lens or (T,) * B, H, cs)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. resident forward + one-kernel backward (16-bit, T <= 256)
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 31, 32, 33])
def test_resident_tile_edges(ops, T):
    """One token; one row short of, exactly, and one row over a 32-row tile, with a full, a nine-key and a one-key sequence."""
    _dense(ops, "resident+one", 3, T, 3, None if T == 1 else (T, 9, 1))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("scale", [0.125, 0.2])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_resident_text_length(ops, p, scale, dt):
    _dense(ops, "resident+one", 4, 77, 3, (77, 40, 9, 1), p, scale, dt, colsum=True)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("scale", [0.125, 0.2])
def test_resident_vit_length(ops, scale, dt):
    _dense(ops, "resident+one", 3, 197, 3, None, 0.0, scale, dt, colsum=True)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_resident_longest(ops, p):
    """T = 256 with lengths (256, 85, 1): the one-key sequence's dV (a column sum of dout over 256 rows, ~40) sits next to a full-length
    sequence whose gradients have an RMS of 0.2 - each is judged on its own scale."""
    _dense(ops, "resident+one", 3, 256, 3, (256, 85, 1), p, colsum=True)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. ring forward + streaming backward (delta, dkv, dq kernels)
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,lens,p,dt", [(257, 3, None, 0.0, "bf16"), (257, 3, None, 0.1, "bf16"), (300, 4, (300, 257, 33, 1), 0.0, "bf16"),
                                           (300, 4, (300, 257, 33, 1), 0.1, "bf16"), (300, 4, (300, 257, 33, 1), 0.1, "f16")],
                         ids=["257-3-None-0.0", "257-3-None-0.1", "300-4-lens1-0.0", "300-4-lens1-0.1", "300-4-lens1-0.1-f16"])
def test_ring_and_streaming_backward(ops, T, B, lens, p, dt):
    """The first length past the resident kernels, unmasked and masked, with and without dropout: attn_fwd_bf16_kernel<H, DROP, MASK>,
    attn_delta_kernel<H>, attn_bwd_dkv_kernel<H, DROP>, attn_bwd_dq_kernel<H, DROP> and the column-sum pass over dqkv.  The masked case
    with dropout also in fp16: the one case that reaches <DROP, MASK> of all four kernels."""
    _dense(ops, "ring+streaming", B, T, 3, lens, p, dt=dt, colsum=True)


@pytest.mark.parametrize("T,B,H,lens", [(600, 3, 1, (600, 513, 1)), (1088, 2, 3, (1088, 5))])
def test_ring_forward_at_the_mask_limit(ops, T, B, H, lens):
    _dense(ops, "ring fwd masked", B, T, H, lens, grads=False)


@pytest.mark.parametrize("T,B,lens", [(77, 2, (77, 9)), (197, 3, None)])
def test_ring_kernels_forced_on_short_sequences(ops, T, B, lens):
    _dense(ops, "ring forced (variant 1)", B, T, 3, lens, variant=1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. the 64-queries-per-wave forward
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 6, 7])
@pytest.mark.parametrize("T,dt", [(512, "bf16"), (512, "f16"), (513, "bf16"), (513, "f16"), (577, "bf16"), (1025, "bf16")])
def test_w64_forward(ops, T, dt, variant):
    _dense(ops, f"w64 fwd (variant {variant})", 1, T, 3, dt=dt, variant=variant, grads=False)


def test_w64_forward_feeds_the_streaming_backward(ops):
    """Gradients through the lse the w64 kernel saved (its own offset-and-scale form of m + log2 l)."""
    _dense(ops, "w64 fwd + streaming bwd", 1, 513, 3, colsum=True)


@pytest.mark.parametrize("variant", [6, 7])
@pytest.mark.parametrize("scale", [0.125, 0.2])
@pytest.mark.parametrize("T,dt", [(513, "bf16"), (577, "bf16"), (513, "f16")], ids=["513", "577", "513-f16"])
def test_w64_forward_qscaled(ops, T, dt, scale, variant):
    """q columns carry scale * log2(e) before their rounding; the reference divides the factor out of the ROUNDED q."""
    B, H = 1, 3
    c = ops.attention_qscale(scale)
    x = torch.randn(B, T, 3, H, 64, generator=torch.Generator().manual_seed(T + 7)) * 1.2
    x[:, :, 0] *= c
    qkv = x.view(B, T, 3 * H * 64).to(DT[dt])
    ref = A.reference(qkv, None, H, scale, q_div=c)
    yards = [A.emulate(qkv, None, H, scale, variant=v, rnd=DT[dt], device="cuda", qscaled=True) for v in "AB"]
    ops.set_attention_variant(variant)
    try:
        out, lse = ops.attention_fwd_qscaled(qkv.cuda(), H, save_lse=True)
    finally:
        ops.set_attention_variant(0)
    _report(f"w64 qscaled (variant {variant}) {dt} B{B} H{H} T{T} scale={scale}", {"out": A.split(out, H)[0], "lse": lse}, ref, yards,
            torch.ones(B, T, dtype=torch.bool), dt, FWD, (T,) * B, H)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. packed rows
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,dt", [(0.0, "bf16"), (0.1, "bf16"), (0.1, "f16")], ids=["0.0", "0.1", "0.1-f16"])
def test_packed_rows(ops, p, dt):
    """simseg_attention_fwd_rows / _bwd_rows per sequence against float64: the reference is the dense, prefix-masked attention of the
    same tokens (queries past a length carry no dout and are not compared).  The C entry points are called as ops.attention_*_rows call
    them, on buffers pre-filled with a sentinel: rows behind the last sequence and the lse of the EMPTY sequence are not written."""
    from simseg_amd.lib import call, ptr, raw, stream
    lens, T, H, scale, pad, sentinel = (77, 1, 9, 32, 33, 0), 77, 2, 0.125, 5, -1024.0
    B = len(lens)
    qkv, dout = (t.clone() for t in _inputs(B, T, H, dt))
    valid = A.key_mask(lens, T)
    dout[~valid] = 0
    keep = _keep(B, H, T, p)
    ref_lens = tuple(n or T for n in lens)                      # (the empty sequence is not compared: any mask will do for it)
    ref = A.reference(qkv, dout, H, scale, ref_lens, keep)
    yards = [{k: t.cpu() for k, t in A.emulate(qkv, dout, H, scale, ref_lens, keep, v, rnd=DT[dt], device="cuda").items()} for v in "AB"]
    idx = valid.view(-1).nonzero().flatten()
    n = idx.numel()
    qp = torch.cat([qkv.view(B * T, -1)[idx], torch.full((pad, 3 * H * 64), float("nan"), dtype=DT[dt])]).cuda()
    dp = torch.cat([dout.view(B * T, -1)[idx], torch.zeros(pad, H * 64, dtype=DT[dt])]).cuda()
    rs = torch.zeros(B + 1, dtype=torch.int32)
    rs[1:] = torch.tensor(lens).cumsum(0)
    rs = rs.cuda()
    out = torch.full((n + pad, H * 64), sentinel, dtype=DT[dt], device="cuda")
    lse = torch.full((B, H, T), sentinel, device="cuda")
    dqkv = torch.full((n + pad, 3 * H * 64), sentinel, dtype=DT[dt], device="cuda")
    cs = torch.zeros(3 * H * 64, device="cuda")
    ws = torch.empty(raw("simseg_attention_bwd_workspace_bytes", B, T, H) // 4, device="cuda")
    ops.set_attention_variant(0)
    call("simseg_attention_fwd_rows", ptr(qp), ptr(rs), ptr(out), ptr(lse), B, T, H, scale, DROP_SEED, p, stream())
    call("simseg_attention_bwd_rows", ptr(qp), ptr(rs), ptr(out), ptr(dp), ptr(lse), ptr(ws), ptr(dqkv), ptr(cs), B, T, H, scale, DROP_SEED, p, stream())
    assert bool((out[n:] == sentinel).all()) and bool((dqkv[n:] == sentinel).all()), "rows behind the last sequence were written"
    assert bool((lse[5] == sentinel).all()), "the empty sequence's lse was written"

    def dense(packed, width):
        full = torch.zeros(B * T, width, dtype=packed.dtype)
        full[idx] = packed[:n].cpu()
        return full.view(B, T, width)
    got = {"out": A.split(dense(out, H * 64), H)[0], "lse": lse.cpu()}
    got["dq"], got["dk"], got["dv"] = A.split(dense(dqkv, 3 * H * 64), H)
    _report(f"packed rows {dt} B{B} H{H} T{T} {'x'.join(map(str, lens))} p={p} scale={scale}", got, ref, yards, valid, dt, GRADS, lens, H, cs)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 5. the fp32 kernels
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.125, 0.2])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T,H,lens", [(1, 3, None), (33, 3, None), (77, 3, (77, 9, 1)), (300, 1, None)])
def test_fp32_forward_and_backward(ops, T, H, lens, p, scale):
    _dense(ops, "fp32 fwd+bwd", 3, T, H, lens, p, scale, "f32", colsum=True)


@pytest.mark.parametrize("T,H", [(33, 3), (325, 1)])
def test_fp32_forward_on_bf16_pieces(ops, T, H):
    """attention_fwd_x3: fp32 operands as three bf16 pieces on the bf16 matrix pipe, under the fp32 rule."""
    B = 3
    qkv, _ = _inputs(B, T, H, "f32")
    ref, yards = _truth(B, T, H, "f32", None, 0.0, 0.125, False)
    out = ops.attention_fwd_x3(qkv.cuda(), H, 0.125)
    _report(f"fwd_x3 f32 B{B} H{H} T{T} unmasked scale=0.125", {"out": A.split(out, H)[0]}, ref, yards, torch.ones(B, T, dtype=torch.bool),
            "f32", ("out",), (T,) * B, H)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 6. a sequence with no unmasked key
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_fully_masked_sequence_is_finite_and_leaks_nothing(ops, dt):
    """B = 2, T = 40, lengths (40, 0).  Sequence 0 against float64 as everywhere; sequence 1 (unspecified but finite: include/simseg_hip.h)
    has finite out, lse and dqkv; and sequence 0's results are the bits of a B = 1 call on sequence 0 alone."""
    B, T, H = 2, 40, 3
    qkv, dout = _inputs(B, T, H, dt)
    mask = A.key_mask((T, 0), T).long().cuda()
    cs = torch.zeros(3 * H * 64, device="cuda")
    out, lse = ops.attention_fwd(qkv.cuda(), H, mask, save_lse=True)
    dqkv = ops.attention_bwd(qkv.cuda(), out, dout.cuda(), lse, H, mask)
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert bool(torch.isfinite(t[1].float()).all()), f"{name} of the fully masked sequence is not finite"
    q1, d1 = qkv[:1].contiguous().cuda(), dout[:1].contiguous().cuda()
    out1, lse1 = ops.attention_fwd(q1, H, mask[:1].contiguous(), save_lse=True)
    dqkv1 = ops.attention_bwd(q1, out1, d1, lse1, H, mask[:1].contiguous(), colsum=cs)
    assert torch.equal(out[:1], out1) and torch.equal(lse[:1], lse1) and torch.equal(dqkv[:1], dqkv1), "sequence 1 leaked into sequence 0"
    ref = A.reference(qkv[:1], dout[:1], H, 0.125, (T,))
    if dt == "f32":
        yards = [A.reference(qkv[:1], dout[:1], H, 0.125, (T,), dtype=torch.float32, device="cuda")]
    else:
        yards = [A.emulate(qkv[:1], dout[:1], H, 0.125, (T,), None, v, device="cuda") for v in "AB"]
    got = {"out": A.split(out[:1], H)[0], "lse": lse[:1]}
    got["dq"], got["dk"], got["dv"] = A.split(dqkv[:1], H)
    _report(f"fully masked neighbour {dt} B{B} H{H} T{T} 40x0, sequence 0", got, ref, [{k: t.cpu() for k, t in y.items()} for y in yards],
            torch.ones(1, T, dtype=torch.bool), dt, GRADS, (T,), H, cs)
