"""The loss head and the small row kernels on MI355X against float64 references written here in plain torch on the CPU, from the formulas
of include/simseg_hip.h and the kernels' header comments: nce_rows / nce_pair, transpose_multi, the fused heads.ClipLossFn, scale_rows,
scale_by_scalar, vit_cls_grad, segment_mean_l2norm, retrieval_rank / retrieval_rank_cols / recall_counts.

Toleranced checks carry no hand-picked tolerance: the same formula is also evaluated in fp32 torch on the device, its error against the
float64 reference is the yardstick, and the kernel's error against float64 may be at most 8 x the yardstick + 4 fp32 ulps of the compared
tensor's largest magnitude (8: the fast exp / log intrinsics are a couple of ulps where libm's are one, and the sums run in another
order).  Every such check prints one `loss-head |` line (kernel error, yardstick, ratio, floor); profiles/loss_head_tests.txt is that table.
Everything else is compared bit for bit."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTOR = 8.0          # kernel error <= FACTOR * (fp32 torch error) + FLOOR_ULPS ulps of max |reference|
FLOOR_ULPS = 4.0


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _unit_rows(n, d, seed):
    return F.normalize(_randn(n, d, seed=seed), dim=-1)


def _ulp32(m):
    """Spacing of fp32 numbers at magnitude m (0 at 0: an exactly-zero reference is compared exactly)."""
    return 0.0 if m == 0.0 else math.ldexp(1.0, max(math.frexp(m)[1], -125) - 24)


def _check(case, what, got, want64, yard32):
    """The yardstick rule of the module docstring; prints the figures before it asserts."""
    want = want64.detach().double().cpu()
    err = (got.detach().double().cpu() - want).abs().max().item()
    yard = (yard32.detach().double().cpu() - want).abs().max().item()
    floor = FLOOR_ULPS * _ulp32(want.abs().max().item())
    ratio = f"{err / yard:7.2f}" if yard > 0 else "      -"
    print(f"loss-head | {case:<44s} | {what:<6s} | kernel {err:.3e} | fp32 torch {yard:.3e} | ratio {ratio} | floor {floor:.3e}")
    assert math.isfinite(err) and err <= FACTOR * yard + floor, \
        f"{case} {what}: kernel error {err:.3e} > {FACTOR:g} x {yard:.3e} (fp32 torch) + {floor:.3e} ({FLOOR_ULPS:g} ulps)"


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. nce_rows / nce_pair
# ------------------------------------------------------------------------------------------------------------------------------------------
# (N1, N2, target0): a row shorter than one wave; shorter than one block (threads whose running maximum stays at -inf); 256 + 1 elements;
# several elements per thread; targets in the last columns; a rank other than 0 of a gathered batch.
NCE_SHAPES = [(1, 1, 0), (5, 5, 0), (3, 64, 61), (33, 257, 100), (97, 388, 194), (64, 1000, 936), (300, 300, 0)]
# Seeds (found on the CPU, see _margin_ok) for which EVERY row of both blocks keeps its best logit more than 1e-4 of the row's largest |z|
# above its second best in float64: only then is the top-1 accuracy of real-valued inputs a well-posed exact comparison.
NCE_SEED = {(1, 1): 1, (5, 5): 1, (3, 64): 1, (33, 257): 1, (97, 388): 1, (64, 1000): 1, (300, 300): 1}
HEAD_SEED = {(5, 64): 1, (33, 72): 1, (97, 128): 1, (257, 64): 1}


@functools.lru_cache(maxsize=None)
def _sim_blocks(N1, N2, seed):
    """[2, N1, N2] fp32 on the CPU: two blocks of products of unit-norm rows (block 0 serves nce_rows, both serve nce_pair).  Read-only."""
    return torch.stack([_unit_rows(N1, 64, seed + 10 * k) @ _unit_rows(N2, 64, seed + 10 * k + 5).T for k in range(2)])


def _ignore_mask(N1):
    """Drops two rows (as many as leave one row standing) and down-weights a third: weights are 1 - ignore, kept rows are ignore < 1."""
    ign = torch.zeros(N1)
    for i in (N1 // 2, N1 - 1):
        if i > 0:
            ign[i] = 1.0
    if N1 >= 5:
        ign[1] = 0.25
    return ign


def _nce_loss(s, t, target0, smoothing, ign=None):
    """InfoNCE rows of one [N1, N2] block in s's dtype on s's device: z = s / clamp(T, 1e-3, 0.5); per row (1 - eps) * nll +
    eps * mean_j(-logp); row weights 1 - ignore; mean over N1.  -> (loss, z)"""
    z = s / torch.clamp(t, 1e-3, 0.5)
    logp = torch.log_softmax(z, -1)
    tgt = torch.arange(target0, target0 + s.shape[0], device=s.device)
    rows = (1 - smoothing) * -logp.gather(1, tgt[:, None])[:, 0] + smoothing * -logp.mean(-1)
    if ign is not None:
        rows = rows * (1 - ign)
    return rows.mean(), z


def _nce_eval(blocks, t32, target0, smoothing, ign=None, weight=1.0, dtype=torch.float64, device="cpu"):
    """loss = weight * sum_k NCE(blocks[k]) with its autograd gradient w.r.t. the temperature, and per block d NCE(blocks[k]) / d blocks[k],
    in `dtype` on `device`.  The block gradients carry no `weight`: simseg_nce_pair scores each block "as simseg_nce_rows" and writes
    that gradient; the pair's 0.5 is in out4's loss and dLoss/dT only, and heads.ClipLossFn applies it to the blocks in
    transpose_multi (alpha = 0.5) - test_fused_head_vs_float64 checks the product.  (weight is 1 or 0.5: the division is exact.)"""
    s = blocks.to(device=device, dtype=dtype).requires_grad_(True)
    t = t32.to(device=device, dtype=dtype).requires_grad_(True)
    ign = None if ign is None else ign.to(device=device, dtype=dtype)
    parts = [_nce_loss(s[k], t, target0, smoothing, ign) for k in range(s.shape[0])]
    loss = weight * sum(p[0] for p in parts)
    loss.backward()
    dt = t.grad if t.grad is not None else torch.zeros_like(t)
    return {"loss": loss.detach(), "ds": s.grad / weight, "dt": dt.reshape(()), "z": [p[1].detach() for p in parts]}


def _margin_ok(z):
    """Every row's best logit exceeds its second best by more than 1e-4 of the row's largest |z| (a one-column row has no second best)."""
    if z.shape[1] < 2:
        return True
    top = z.topk(2, dim=1).values
    return bool(((top[:, 0] - top[:, 1]) > 1e-4 * z.abs().max(1).values).all())


def _first_max(z):
    """The kernel's top-1 rule: the first index attaining the row maximum."""
    idx = torch.arange(z.shape[1]).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, z.shape[1])).min(1).values


def _acc32(z64, target0, keep=None):
    """hits / kept rows as the one fp32 division the finalize kernels make."""
    hit = _first_max(z64) == torch.arange(target0, target0 + z64.shape[0])
    keep = torch.ones_like(hit) if keep is None else keep
    return (torch.tensor(float((hit & keep).sum()), dtype=torch.float32) / torch.tensor(float(keep.sum()), dtype=torch.float32)).item()


def _run_nce_rows(ops, case, s, T, target0, smoothing, ign, t_ref=None, check_acc=True):
    """One nce_rows case against float64 (reference evaluated at t_ref when given: the clamped temperature) -> out3 on the CPU."""
    t32 = torch.tensor([T], dtype=torch.float32)
    tr = t32 if t_ref is None else torch.tensor([t_ref], dtype=torch.float32)
    ref = _nce_eval(s[None], tr, target0, smoothing, ign)
    yard = _nce_eval(s[None], tr, target0, smoothing, ign, dtype=torch.float32, device="cuda")
    ign_d = None if ign is None else ign.cuda()
    sims = s.cuda().clone()
    out3 = ops.nce_rows(sims, t32.cuda(), target0, ign_d, smoothing)
    _check(case, "loss", out3[0], ref["loss"], yard["loss"])
    _check(case, "dsims", sims, ref["ds"][0], yard["ds"][0])
    if t_ref is None:
        _check(case, "dT", out3[2], ref["dt"], yard["dt"])
    else:
        assert out3[2].item() == 0.0, f"{case}: a clamped temperature passes no gradient, got {out3[2].item()}"
    if check_acc:
        assert _margin_ok(ref["z"][0]), f"{case}: a row's top two logits are too close for an exact accuracy check - pick another seed"
        keep = None if ign is None else ign < 1
        assert out3[1].item() == _acc32(ref["z"][0], target0, keep), f"{case}: top-1 accuracy {out3[1].item()}"
    # write_grad = False: the similarities survive bit for bit, loss and accuracy are the same numbers
    kept = s.cuda().clone()
    o2 = ops.nce_rows(kept, t32.cuda(), target0, ign_d, smoothing, write_grad=False)
    assert torch.equal(kept.cpu(), s), f"{case}: write_grad=False modified sims"
    assert torch.equal(o2[:2], out3[:2]), f"{case}: write_grad=False changed loss / accuracy: {o2.tolist()} vs {out3.tolist()}"
    return out3.cpu()


def _run_nce_pair(ops, case, s2, T, target0, smoothing, t_ref=None, check_acc=True):
    t32 = torch.tensor([T], dtype=torch.float32)
    tr = t32 if t_ref is None else torch.tensor([t_ref], dtype=torch.float32)
    ref = _nce_eval(s2, tr, target0, smoothing, weight=0.5)
    yard = _nce_eval(s2, tr, target0, smoothing, weight=0.5, dtype=torch.float32, device="cuda")
    sims = s2.cuda().clone()
    out4 = ops.nce_pair(sims, t32.cuda(), target0, smoothing)
    _check(case, "loss", out4[0], ref["loss"], yard["loss"])
    _check(case, "dsims", sims, ref["ds"], yard["ds"])
    if t_ref is None:
        _check(case, "dT", out4[3], ref["dt"], yard["dt"])
    else:
        assert out4[3].item() == 0.0, f"{case}: a clamped temperature passes no gradient, got {out4[3].item()}"
    if check_acc:
        for k in range(2):
            assert _margin_ok(ref["z"][k]), f"{case}: block {k}: top two logits too close for an exact accuracy check - pick another seed"
            assert out4[1 + k].item() == _acc32(ref["z"][k], target0), f"{case}: block {k} top-1 accuracy {out4[1 + k].item()}"
    kept = s2.cuda().clone()
    o2 = ops.nce_pair(kept, t32.cuda(), target0, smoothing, write_grad=False)
    assert torch.equal(kept.cpu(), s2), f"{case}: write_grad=False modified sims"
    assert torch.equal(o2[:3], out4[:3]), f"{case}: write_grad=False changed loss / accuracies: {o2.tolist()} vs {out4.tolist()}"
    return out4.cpu()


@pytest.mark.parametrize("T", [0.05, 0.01])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("N1,N2,target0", NCE_SHAPES)
def test_nce_rows_vs_float64(ops, N1, N2, target0, smoothing, masked, T):
    s = _sim_blocks(N1, N2, NCE_SEED[N1, N2])[0]
    case = f"nce_rows {N1}x{N2}+{target0} eps={smoothing} T={T}" + (" ignore" if masked else "")
    _run_nce_rows(ops, case, s, T, target0, smoothing, _ignore_mask(N1) if masked else None)


@pytest.mark.parametrize("T", [0.05, 0.01])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("N1,N2,target0", NCE_SHAPES)
def test_nce_pair_vs_float64(ops, N1, N2, target0, smoothing, T):
    s2 = _sim_blocks(N1, N2, NCE_SEED[N1, N2])
    _run_nce_pair(ops, f"nce_pair {N1}x{N2}+{target0} eps={smoothing} T={T}", s2, T, target0, smoothing)


@pytest.mark.parametrize("T,clamped", [(0.001, None), (0.5, None), (0.0005, 0.001), (0.7, 0.5)])
def test_nce_temperature_clamp(ops, T, clamped):
    """On the clamp's edges (exactly fp32 0.001 and 0.5) the temperature gradient passes and equals the reference's; outside them it is
    exactly 0 and the loss is the reference's at the clamped value."""
    N1, N2, target0 = 33, 257, 100
    s2 = _sim_blocks(N1, N2, NCE_SEED[N1, N2])
    _run_nce_rows(ops, f"nce_rows {N1}x{N2}+{target0} eps=0.1 T={T}", s2[0], T, target0, 0.1, None, t_ref=clamped)
    _run_nce_pair(ops, f"nce_pair {N1}x{N2}+{target0} eps=0.1 T={T}", s2, T, target0, 0.1, t_ref=clamped)


def _tie_block(N1, N2, target0, seed, first_kind):
    """Similarities on the 2^-10 grid (z = s / 2^-5 is exact in fp32) in [-0.25, 0.25) with 0.75 planted per row, cycling through: target
    the unique maximum (hit); tied with an EARLIER column (miss: the first index attaining the maximum wins); tied with a LATER column
    (hit); not the maximum (miss).  The planted columns sit in other threads and waves than the target.  -> (s, expected hits)"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-256, 256, (N1, N2), generator=g).float() / 1024
    hits = torch.zeros(N1, dtype=torch.bool)
    for i in range(N1):
        t, kind = target0 + i, (i + first_kind) % 4
        if kind == 0:
            s[i, t] = 0.75
        elif kind == 1:
            s[i, t] = 0.75
            s[i, t - 37 - i] = 0.75
        elif kind == 2:
            s[i, t] = 0.75
            s[i, t + 70 + i] = 0.75
        else:
            s[i, t] = 0.25
            s[i, (t + 129) % N2] = 0.75
        hits[i] = kind in (0, 2)
    return s, hits


def test_nce_top1_first_maximum_wins(ops):
    """The documented top-1 rule (include/simseg_hip.h, simseg_nce_rows) asserted exactly on inputs whose logits are exact in fp32."""
    N1, N2, target0, T = 33, 257, 100, 2.0 ** -5
    blocks, hits = zip(_tie_block(N1, N2, target0, 3, 0), _tie_block(N1, N2, target0, 4, 2))
    s2 = torch.stack(blocks)
    for k in range(2):                                     # the planted rows are what they claim to be
        z = s2[k].double() / T
        assert torch.equal(_first_max(z) == torch.arange(target0, target0 + N1), hits[k])
        assert (z == z.max(1, keepdim=True).values).sum(1).max() == 2
    t = torch.tensor([T]).cuda()
    ign = torch.zeros(N1)
    ign[[4, 6]] = 1.0                                      # drops one hit (kind 0) and one tied-later hit (kind 2)
    for mask in (None, ign):
        keep = torch.ones(N1, dtype=torch.bool) if mask is None else mask < 1
        want = (torch.tensor(float((hits[0] & keep).sum())) / torch.tensor(float(keep.sum()))).item()
        out3 = ops.nce_rows(s2[0].cuda().clone(), t, target0, None if mask is None else mask.cuda(), 0.0)
        assert out3[1].item() == want, (out3[1].item(), want)
        assert ops.nce_rows(s2[0].cuda().clone(), t, target0, None if mask is None else mask.cuda(), 0.0, write_grad=False)[1].item() == want
    out4 = ops.nce_pair(s2.cuda().clone(), t, target0, 0.1)
    for k in range(2):
        want = (torch.tensor(float(hits[k].sum())) / torch.tensor(float(N1))).item()
        assert out4[1 + k].item() == want, (k, out4[1 + k].item(), want)


@pytest.mark.parametrize("N1,N2,target0", [(33, 257, 225), (0, 257, 0)])
def test_nce_argument_refusals(ops, N1, N2, target0):
    """target0 + N1 > N2 and N1 = 0 are refused by the host check: an exception, and no kernel touched the similarities."""
    t = torch.tensor([0.05]).cuda()
    rows = max(N1, 1)
    s = _randn(2, rows, N2, seed=5).cuda()
    before = s.clone()
    with pytest.raises(RuntimeError, match="nce_rows"):
        ops.nce_rows(s[0, :N1], t, target0)
    with pytest.raises(RuntimeError, match="nce_pair"):
        ops.nce_pair(s[:, :N1], t, target0)
    torch.cuda.synchronize()
    assert torch.equal(s, before)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. transpose_multi, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------------
TR_ORDERS = [
    # (shapes, scale flags): six jobs; 1x70 starts right after the one-tile 1x1, 70x1 and 31x33 after multi-tile jobs
    ([(1, 1), (1, 70), (70, 1), (31, 33), (32, 32), (65, 97)], [1, 0, 1, 1, 0, 1]),
    # the many-tile job first, 65x97 right after the one-tile 1x1, another order of the flags
    ([(257, 40), (32, 32), (1, 1), (65, 97), (70, 1)], [0, 1, 0, 0, 1]),
    ([(65, 97), (257, 40), (31, 33), (1, 70)], [1, 1, 0, 0]),
    ([(65, 97)], [1]),
    ([(257, 40)], [0]),
]


def _tr_expected(mats, flags, f):
    """(transposed copies, inputs afterwards): flagged jobs times the ONE fp32 factor f - in the copy and in place."""
    outs = [((m * f) if fl else m).T.contiguous() for m, fl in zip(mats, flags)]
    ins = [(m * f) if fl else m for m, fl in zip(mats, flags)]
    return outs, ins


@pytest.mark.parametrize("order", range(len(TR_ORDERS)))
def test_transpose_multi_bit_exact(ops, order):
    shapes, flags = TR_ORDERS[order]
    mats = [_randn(r, c, seed=20 + k) for k, (r, c) in enumerate(shapes)]
    scalar, x0, alpha = torch.tensor([1.7]), torch.tensor([-0.3, 9.0]), 0.5
    f = torch.tensor(alpha, dtype=torch.float32) * scalar[0]            # J.alpha * J.scalar[0]: one fp32 product
    want_out, want_in = _tr_expected(mats, flags, f)
    dev = [m.cuda() for m in mats]
    outs, y0 = ops.transpose_multi(dev, flags, scalar=scalar.cuda(), alpha=alpha, x0=x0.cuda())
    for k in range(len(mats)):
        assert outs[k].shape == (shapes[k][1], shapes[k][0])
        assert torch.equal(outs[k].cpu(), want_out[k]), f"order {order} job {k} {shapes[k]} flag {flags[k]}: transposed copy"
        assert torch.equal(dev[k].cpu(), want_in[k]), f"order {order} job {k} {shapes[k]} flag {flags[k]}: input afterwards"
    assert torch.equal(y0.cpu(), scalar[:1] * x0[:1])


def test_transpose_multi_c_entry_writes_only_its_outputs(ops):
    """The C entry point called as ops.transpose_multi calls it, with the outputs carved out of one buffer pre-filled with a sentinel bit
    pattern and gaps before and after each: a ragged-edge tile writes nothing outside its matrix."""
    from simseg_amd.lib import call, ptr, stream
    shapes, flags = TR_ORDERS[0]
    n, gap, sentinel = len(shapes), 67, 0x7FC0BEEF
    mats = [_randn(r, c, seed=40 + k) for k, (r, c) in enumerate(shapes)]
    scalar, alpha = torch.tensor([-2.25]), 0.5
    want_out, want_in = _tr_expected(mats, flags, torch.tensor(alpha, dtype=torch.float32) * scalar[0])
    offs, total = [], gap
    for r, c in shapes:
        offs.append(total)
        total += r * c + gap
    buf = torch.full((total,), sentinel, dtype=torch.int32).cuda()
    fbuf = buf.view(torch.float32)
    dev, sc = [m.cuda() for m in mats], scalar.cuda()
    outs = [fbuf[o:o + r * c] for o, (r, c) in zip(offs, shapes)]
    PT, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int32 * n
    call("simseg_transpose_multi", PT(*[m.data_ptr() for m in dev]), PT(*[o.data_ptr() for o in outs]), I64(*[r for r, _ in shapes]),
         I64(*[c for _, c in shapes]), I32(*flags), n, ptr(sc), alpha, None, None, stream())
    got = buf.cpu()
    untouched = torch.ones(total, dtype=torch.bool)
    for k, (o, (r, c)) in enumerate(zip(offs, shapes)):
        untouched[o:o + r * c] = False
        assert torch.equal(got[o:o + r * c].view(torch.float32).view(c, r), want_out[k]), f"job {k} {shapes[k]}: transposed copy"
        assert torch.equal(dev[k].cpu(), want_in[k]), f"job {k} {shapes[k]}: input afterwards"
    assert untouched.sum() == gap * (n + 1)
    assert bool((got[untouched] == sentinel).all()), "a tile wrote outside its output matrix"


def test_transpose_multi_refusals(ops):
    m = [_randn(3, 4, seed=k).cuda() for k in range(7)]
    sc = torch.tensor([2.0]).cuda()
    with pytest.raises(RuntimeError, match="1..6 jobs"):
        ops.transpose_multi(m, [0] * 7)
    with pytest.raises(RuntimeError, match="empty"):
        ops.transpose_multi([m[0], torch.empty(0, 4).cuda()], [0, 0])
    keep = m[1].clone()
    with pytest.raises(RuntimeError, match="needs the scalar"):
        ops.transpose_multi([m[0], m[1]], [0, 1])
    torch.cuda.synchronize()
    assert torch.equal(m[1], keep)
    outs, y0 = ops.transpose_multi([m[0], m[1]], [0, 1], scalar=sc)                # the same call with the scalar is fine
    assert y0 is None and torch.equal(outs[0], m[0].T) and torch.equal(outs[1], (keep * 2.0).T) and torch.equal(m[1], keep * 2.0)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. the fused head end to end
# ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_embeddings(Bl, P, seed):
    """Unit-norm fp32 image rows and text rows correlated with them (the matching caption is the best one, as in a trained model)."""
    img = _unit_rows(Bl, P, seed)
    return img, F.normalize(img + 0.7 * _unit_rows(Bl, P, seed + 1), dim=-1)


def _head_eval(img32, txt32, t32, smoothing, upstream, dtype, device):
    """upstream * 0.5 * (NCE(img, txt) + NCE(txt, img)) from the embeddings, plain torch autograd in `dtype` on `device`."""
    img = img32.to(device=device, dtype=dtype).requires_grad_(True)
    txt = txt32.to(device=device, dtype=dtype).requires_grad_(True)
    t = t32.to(device=device, dtype=dtype).requires_grad_(True)
    li, zi = _nce_loss(img @ txt.T, t, 0, smoothing)
    lt, zt = _nce_loss(txt @ img.T, t, 0, smoothing)
    loss = 0.5 * (li + lt)
    (upstream * loss).backward()
    return {"loss": loss.detach(), "dimg": img.grad, "dtxt": txt.grad, "dt": t.grad, "z": [zi.detach(), zt.detach()]}


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("Bl,P", [(5, 64), (33, 72), (97, 128), (257, 64)])
def test_fused_head_vs_float64(ops, Bl, P, smoothing):
    """heads.ClipLossFn forward + backward (two GEMMs, nce_pair; transpose_multi, four GEMMs) with an upstream gradient of 3 against
    float64 autograd of 0.5 * (NCE(img, txt) + NCE(txt, img)): a gradient block scaled twice or a transposed operand taken from the
    wrong job shows here."""
    from simseg_amd import heads
    img32, txt32 = _pair_embeddings(Bl, P, HEAD_SEED[Bl, P])
    t32 = torch.tensor(0.05)
    ref = _head_eval(img32, txt32, t32, smoothing, 3.0, torch.float64, "cpu")
    yard = _head_eval(img32, txt32, t32, smoothing, 3.0, torch.float32, "cuda")
    img, txt, t = (x.cuda().requires_grad_(True) for x in (img32, txt32, t32))
    loss, a1, a2 = heads.ClipLossFn.apply(img, txt, t, None, 0, smoothing, True)
    (loss * 3.0).backward()
    case = f"fused head Bl={Bl} P={P} eps={smoothing} T=0.05"
    _check(case, "loss", loss, ref["loss"], yard["loss"])
    _check(case, "dimg", img.grad, ref["dimg"], yard["dimg"])
    _check(case, "dtxt", txt.grad, ref["dtxt"], yard["dtxt"])
    _check(case, "dT", t.grad, ref["dt"], yard["dt"])
    for k, acc in enumerate((a1, a2)):
        assert _margin_ok(ref["z"][k]), f"{case}: direction {k}: top two logits too close for an exact accuracy check - pick another seed"
        assert acc.item() == _acc32(ref["z"][k], 0), f"{case}: direction {k} top-1 accuracy {acc.item()}"


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. the small row kernels
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("mode", ["s", "one_minus_s", "none"])
@pytest.mark.parametrize("rows,D", [(1, 1), (7, 13), (300, 64), (8200, 257)])          # 8200 x 257 > 8192 x 256: the grid-stride loop wraps
def test_scale_rows_exact(ops, rows, D, mode, alpha):
    x, s = _randn(rows, D, seed=1), torch.rand(rows, generator=torch.Generator().manual_seed(2))
    f = {"s": s, "one_minus_s": 1.0 - s, "none": torch.ones(rows)}[mode]
    want = x * f[:, None] * alpha                                                        # x * f * alpha, in this order, in fp32
    got = ops.scale_rows(x.cuda(), None if mode == "none" else s.cuda(), one_minus=(mode == "one_minus_s"), alpha=alpha)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 8192 * 256 + 3])
def test_scale_by_scalar_exact(ops, n, alpha):
    x, scalar = _randn(n, seed=3), torch.tensor([-1.37])
    want = x * (scalar * torch.tensor(alpha, dtype=torch.float32))                       # x * (scalar * alpha): one fp32 factor
    xd = x.cuda()
    assert torch.equal(ops.scale_by_scalar(xd, scalar.cuda(), alpha).cpu(), want)
    assert torch.equal(xd.cpu(), x)
    ret = ops.scale_by_scalar(xd, scalar.cuda(), alpha, out=xd)                          # in place, as optim.py's clipping fallback calls it
    assert ret is xd and torch.equal(xd.cpu(), want)


@pytest.mark.parametrize("B,T,D", [(1, 2, 64), (16, 5, 384), (17, 197, 384), (33, 3, 100), (40, 2, 768)])
def test_vit_cls_grad(ops, B, T, D):
    """dcls += sum_b dx[b, 0, :] within 4 fp32 ulps of sum_b |dx[b, 0, d]| per column (the only freedom is the order of the 16-image
    slices' atomics); token rows t > 0 carry a huge constant and must not be read.  dcls starts from random values sized like the
    column sums, so that the value accumulated onto does not outweigh the magnitude the tolerance is stated in."""
    dx = torch.full((B, T, D), 1e30)
    dx[:, 0] = _randn(B, D, seed=4)
    mag = dx[:, 0].double().abs().sum(0)
    dcls0 = ((torch.rand(D, generator=torch.Generator().manual_seed(5)) * 2 - 1) * mag.float())
    want = dcls0.double() + dx[:, 0].double().sum(0)
    dcls = dcls0.cuda()
    ops.vit_cls_grad(dx.cuda(), dcls)
    err = (dcls.double().cpu() - want).abs()
    tol = torch.tensor([FLOOR_ULPS * _ulp32(m) for m in mag.tolist()], dtype=torch.float64)
    assert bool((err <= tol).all()), f"worst column: err {err.max().item():.3e}, err / ulp {(err / (tol / FLOOR_ULPS)).max().item():.2f}"


@pytest.mark.parametrize("B,D", [(0, 64), (4, 0), (0, 0)])
def test_vit_cls_grad_empty_batch_is_a_no_op(ops, B, D):
    from simseg_amd.lib import call, ptr, stream
    dx, dcls = _randn(4, 3, 64, seed=6).cuda(), _randn(64, seed=7).cuda()
    keep = dcls.clone()
    call("simseg_vit_cls_grad", ptr(dx), ptr(dcls), B, 3, D, stream())
    torch.cuda.synchronize()
    assert torch.equal(dcls, keep)


@pytest.mark.parametrize("S,P,D", [(1, 1, 64), (3, 16, 128), (21, 7, 512), (2, 80, 1024)])
def test_segment_mean_l2norm_vs_float64(ops, S, P, D):
    x = _randn(S, P, D, seed=8)
    m = x.double().mean(1)
    want = m / m.norm(dim=-1, keepdim=True)
    xd = x.cuda()
    md = xd.mean(1)
    _check(f"segment_mean_l2norm S={S} P={P} D={D}", "out", ops.segment_mean_l2norm(xd), want, md / md.norm(dim=-1, keepdim=True))


@pytest.mark.parametrize("D", [96, 2048])
def test_segment_mean_l2norm_refuses_unsupported_widths(ops, D):
    with pytest.raises(RuntimeError, match="segment_mean_l2norm"):
        ops.segment_mean_l2norm(_randn(2, 3, D, seed=9).cuda())


def _retrieval_case(M, N):
    """Scores on the 2^-10 grid from 64 levels only (ties between a best match and non-matches are everywhere, in both directions), in a
    [M, N + 5] buffer whose padding columns are +inf; group ids that leave some rows and some columns without a match."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    q = torch.randint(-32, 32, (M, N), generator=g)
    groups = max(1, min(M, N) // 3)
    lgid = torch.randint(0, groups, (M,), generator=g)
    rgid = torch.randint(0, groups, (N,), generator=g)
    lgid[3::5] = 100000 + torch.arange(M)[3::5]          # rows no column matches
    rgid[2::7] = 200000 + torch.arange(N)[2::7]          # columns no row matches
    if M == 1 and N == 1:
        lgid[:], rgid[:] = 7, 7
    buf = torch.full((M, N + 5), float("inf"))
    buf[:, :N] = q.float() / 1024
    return q, lgid, rgid, buf


def _rank_ref(q, lgid, rgid):
    """Exact integer arithmetic: has = any match; rank = #{scores strictly greater than the best match}."""
    match = lgid[:, None] == rgid[None, :]
    has = match.any(1)
    best = torch.where(match, q, torch.full_like(q, -1 << 40)).max(1).values
    rank = (q > best[:, None]).sum(1)
    ties = ((q == best[:, None]) & ~match & has[:, None]).sum().item()
    return has, rank, ties


def _counts_ref(has, rank, bounds):
    return [int(has.sum())] + [int((has & (rank < b)).sum()) for b in bounds]


@pytest.mark.parametrize("M,N", [(1, 1), (127, 300), (128, 256), (129, 257), (300, 70)])
def test_retrieval_ranks_strided_with_ties(ops, M, N):
    """Both directions from one similarity matrix that is a view (ld = N + 5) of a wider buffer, M on either side of the column pass's
    128-row band: strictly greater counts, equal does not; the +inf padding behind N is never read."""
    from simseg_amd.lib import call, ptr, stream
    q, lgid, rgid, buf = _retrieval_case(M, N)
    has_r, rank_r, ties_r = _rank_ref(q, lgid, rgid)
    has_c, rank_c, ties_c = _rank_ref(q.T.contiguous(), rgid, lgid)
    if M * N > 1:
        assert ties_r > 0 and ties_c > 0 and not has_r.all() and not has_c.all() and has_r.any() and has_c.any()
    d_buf, d_l, d_r = buf.cuda(), lgid.cuda(), rgid.cuda()
    sim = d_buf[:, :N]
    ld = d_buf.stride(0)
    assert ld == N + 5 and sim.data_ptr() == d_buf.data_ptr()
    has, rank = torch.full((M,), -7, dtype=torch.int32).cuda(), torch.full((M,), -7, dtype=torch.int32).cuda()
    call("simseg_retrieval_rank", ptr(sim), ptr(d_l), ptr(d_r), ptr(has), ptr(rank), M, N, ld, stream())
    hasc, rankc = torch.full((N,), -7, dtype=torch.int32).cuda(), torch.full((N,), -7, dtype=torch.int32).cuda()
    scratch = torch.empty(N, dtype=torch.int32).cuda()
    call("simseg_retrieval_rank_cols", ptr(sim), ptr(d_l), ptr(d_r), ptr(hasc), ptr(rankc), ptr(scratch), M, N, ld, stream())
    for what, h, r, hr, rr in (("rows", has, rank, has_r, rank_r), ("columns", hasc, rankc, has_c, rank_c)):
        assert torch.equal(h.cpu().long(), hr.long()), f"{what}: has_match"
        assert torch.equal(r.cpu().long()[hr], rr[hr]), f"{what}: rank where a match exists"
        for bounds in ((1, 5, 10), (2, 3, 4)):
            assert ops.recall_counts(h, r, bounds).cpu().tolist() == _counts_ref(hr, rr, bounds), f"{what}: recall counts for {bounds}"
