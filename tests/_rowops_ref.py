"""What tests/test_gpu_rowops.py and tests/test_rowops_ref_host.py share for the kernels of csrc/rowops.hip: float64 references, fp32
restatements in the kernels' order of operations, the judge and the case tables.  Plain torch; everything runs on the CPU, the formulas
that serve as yardsticks also on the device.

The rule (tests/test_gpu_loss_head.py, FACTOR = 8 and FLOOR_ULPS = 4) applied per CELL instead of per tensor.  A cell is one row of a
row output (one batch row of the pooling outputs) and one column of a column output.  In every cell
    |kernel - float64| <= 8 x yardstick + 4 fp32 ulps at the cell's floor magnitude,
    yardstick = the error, in the same cell, of the same formula evaluated in fp32 torch,
    floor magnitude = the row's largest |reference|; for a column sum (dgamma, dbeta, dxsum) the column's sum of |terms| in float64.
A result that exists only in a 16-bit type H (ln_bwd16_kernel's dx) gets, element by element, half a unit in the last place of H at
|reference| on top.  Every other 16-bit output is compared bit for bit with the rounded fp32 value, as is everything that only moves
data or adds exactly representable values.

dxsum - "the column sums of what was written, before its 16-bit rounding" - is judged as exactly that wherever the kernel also writes the
fp32 dx: as the sum of those values (judge_sum_of).  Only ln_bwd16_kernel's, which has no fp32 dx, is judged against float64, with the
rows' own allowances added (ln_step_dxsum_extra).  The column sums are accumulated onto values sized like the sums (ln_bwd_case).

The LayerNorm backward references take mean and rstd as INPUTS (float64 values rounded to fp32), so that forward and backward fail
independently, and follow the kernels' documented law for the normalised value: a 4-column chunk with every |gamma| >= 0.05 and
|beta| <= 4 |gamma| takes xhat = (y16 - beta) / gamma from the saved 16-bit output when it is given, every other chunk
xhat = (x - mean) * rstd.

Input families of the toleranced LayerNorm rows ("plain": 3 N(0,1) + 0.5; "scales": row sigma from 1e-3 to 1e3 inside one tensor;
"outlier": one column at 1e4) keep |row mean| <= 2 x row sigma: a mean many sigma away costs fp32 arithmetic the digits the rule asks
for (8 sigma: 0.77 of the bound, 1e4 sigma: over it).  D = 4 rows use the "plain" family only: a 4-wide "scales" row reaches 0.94 of the
backward row bound in a plain sequential fp32 evaluation.  test_rowops_ref_host.py asserts, for every toleranced case, that the fp32
restatement alone stays within half of every bound."""
import functools

import torch

FACTOR = 8.0
FLOOR_ULPS = 4.0
PREC = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}       # significand bits, the implicit one included
Y16_MIN_GAIN, Y16_MAX_OFFSET = 0.05, 4.0                              # the y16 eligibility test of ln_bwd_kernel / ln_bwd16_kernel
MASKED_VALUE = -10000.0                                                # pooling.py:60


# ------------------------------------------------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------------------------------------------------
def ulp(m, dtype=torch.float32):
    """Spacing of `dtype` numbers at magnitudes m (float64 tensor); 0 at 0, so that an exactly-zero reference is compared exactly."""
    m = torch.as_tensor(m, dtype=torch.float64).abs()
    e = torch.frexp(m)[1].clamp_min(-125 if dtype != torch.float16 else -13)
    return torch.where(m == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), e - PREC[dtype]))


def old_close(got, want, tol):
    """tests/test_gpu_kernels.py::_close as a predicate: ONE maximum error over the tensor, relative to the tensor's largest value."""
    got, want = got.float().cpu(), want.float().cpu()
    return (got - want).abs().max().item() <= tol * (want.abs().max().item() + 1e-12)


def cell_bounds(want64, yard32, dim):
    """8 x the cell's largest yardstick error + 4 fp32 ulps at the cell's largest |want|, one value per cell (`dim` reduced away)."""
    want = want64.detach().double().cpu()
    yerr = (yard32.detach().double().cpu() - want).abs()
    return FACTOR * yerr.amax(dim) + FLOOR_ULPS * ulp(want.abs().amax(dim))


def judge_sum_of(terms32, init32, got, device="cpu"):
    """A column sum whose terms the kernel also wrote (dxsum next to an fp32 dx: "the column sums of what was written, taken before the
    16-bit rounding") is judged as the sum of THOSE terms, the way test_vit_cls_grad judges dcls: reference = init + sum of the fp32
    terms in float64, yardstick = the same sum in fp32 torch, floor magnitude = the column's sum of |terms|.  The terms themselves are
    judged against float64 row by row elsewhere, so a wrong term and a wrong sum fail independently.  (Judged against the float64 dx
    instead, a one-row column would inherit its single term's error - which the row rule allows at the ROW's magnitude - under a floor
    stated at the term's own: a sequential fp32 evaluation breaks that bound in most cases of few rows.)"""
    t = terms32.detach().float().cpu()
    want = init32.double().cpu() + t.double().sum(0)
    yard = init32.to(device) + t.to(device).sum(0)
    return judge(got, want, yard, None, mag=t.double().abs().sum(0))


def judge(got, want64, yard32, dim, mag=None, half=None, extra=None):
    """-> (worst ratio, cells).  Cells lie along every dimension but `dim` (dim = None: every element is a cell of its own, as for a column
    sum or a per-row statistic).  ratio = |got - want| / bound, element by element, with the bound of the element's cell:
    8 x (the cell's largest yardstick error) + 4 fp32 ulps at `mag` (default: the cell's largest |want|) [+ half an ulp of `half` at
    |want| of the element].  0 / 0 counts as 0: where the bound is zero the value must be exact.  Non-finite results give inf."""
    want = want64.detach().double().cpu()
    err = (got.detach().double().cpu() - want).abs()
    yerr = (yard32.detach().double().cpu() - want).abs()
    if dim is None:
        ycell, m = yerr, want.abs()
    else:
        ycell, m = yerr.amax(dim, keepdim=True), want.abs().amax(dim, keepdim=True)
    if mag is not None:
        m = torch.as_tensor(mag, dtype=torch.float64).reshape(m.shape)
    bound = FACTOR * ycell + FLOOR_ULPS * ulp(m)
    if half is not None:
        bound = bound + 0.5 * ulp(want, half)
    if extra is not None:
        bound = bound + extra
    bound = bound.expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)          # x / 0 = inf
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    cells = ycell.numel()
    return (ratio.max().item() if ratio.numel() else 0.0), cells


def line(case, what, ratio, cells):
    """One row of profiles/rowops_tests.txt."""
    return f"rowops | {case:<58s} | {what:<7s} | {ratio:7.3f} | {cells:6d}"


# ------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def ln_rows(family, rows, D, seed):
    """fp32 [rows, D] on the CPU.  Read-only (cached).  The seed moves on (by 1000) until every row keeps |mean| <= 2 sigma."""
    while True:
        x = _ln_rows(family, rows, D, seed)
        if bool((x.double().mean(-1).abs() <= 2 * x.double().std(-1, unbiased=False)).all()):
            return x
        seed += 1000


def _ln_rows(family, rows, D, seed):
    z = torch.randn(rows, D, generator=gen(seed))
    if family == "plain":
        return 3.0 * z + 0.5
    if family == "scales":                       # sigma 1e-3 .. 1e3 across the rows (a single row: 1e-3), mean half a sigma
        sig = 10.0 ** torch.linspace(-3.0, 3.0, rows) if rows > 1 else torch.tensor([1e-3])
        return (z + 0.5) * sig[:, None].float()
    if family == "outlier":
        x = 3.0 * z + 0.5
        x[:, (7 * D) // 11] = 1e4
        return x
    raise ValueError(family)


def ln_exact_rows(rows, D, first):
    """Rows that alternate between all-zero and constant 3.0, starting with `first`: every partial sum is exact, mean = first exactly, every
    centred value is 0 and y = beta bit for bit whatever eps is."""
    x = torch.zeros(rows, D)
    x[(0 if first == 3.0 else 1)::2] = 3.0
    return x


@functools.lru_cache(maxsize=None)
def ln_gains(D, seed, mixed=False):
    """gamma = exp(0.3 N), beta = 0.1 N: every chunk eligible for the y16 read.  mixed: one tiny |gamma| whose beta passes the offset test
    and one large beta under an ordinary gamma (each of the two tests alone sends its chunk to x), one negative eligible gamma, and in
    the last column both tests met with equality (|gamma| = 0.05, |beta| = 4 |gamma| in fp32: still eligible)."""
    g = torch.exp(0.3 * torch.randn(D, generator=gen(seed)))
    b = 0.1 * torch.randn(D, generator=gen(seed + 1))
    if mixed:
        g[1 % D], b[1 % D] = 0.01, 0.02
        g[D - 2] = -0.8
        b[D // 2] = 30.0
        g[D - 1] = Y16_MIN_GAIN
        b[D - 1] = -Y16_MAX_OFFSET * g[D - 1]
    return g, b


def y16_chunks(g, b):
    """[D] bool: the column's 4-wide chunk takes xhat from y16 (decided in fp32, like the kernels)."""
    g, b = g.float().cpu(), b.float().cpu()
    ok = (g.abs() >= Y16_MIN_GAIN) & (b.abs() <= Y16_MAX_OFFSET * g.abs())
    return ok.view(-1, 4).all(1).repeat_interleave(4)


def families_for(D):
    return ("plain",) if D == 4 else ("plain", "scales", "outlier")


# ------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------------------
def ln_fwd(x, g, b, eps, dtype=torch.float64, device="cpu"):
    """-> y, mean, rstd in `dtype` on `device`: the plain formula (biased variance of the centred values)."""
    x, g, b = (t.to(device=device, dtype=dtype) for t in (x, g, b))
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * g + b, mean[:, 0], rstd[:, 0]


def ln_stats32(x, eps):
    """The backward's inputs: float64 mean and rstd rounded to fp32."""
    _, mean, rstd = ln_fwd(x, torch.ones(x.shape[-1]), torch.zeros(x.shape[-1]), eps)
    return mean.float(), rstd.float()


def _tree(v):
    """Sum over the last (power-of-two) axis as a balanced tree of fp32 additions, neighbours first."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def ln_fwd_restated(x, g, b, eps, defect=None):
    """fp32 on the CPU in the kernels' order: a lane owns the 4-wide chunks lane + L i (L = 32 lanes for D <= 512, else 64) and adds
    (v0 + v1) + (v2 + v3) chunk by chunk, then a tree across the lanes; the centred squares the same way, element by element.
    defect: None | "bessel" (variance / (D - 1)) | "no_eps" | "tail_mean" (the odd last row takes its neighbour's mean)."""
    x, g, b = x.float(), g.float(), b.float()
    rows, D = x.shape
    L = 32 if D <= 512 else 64
    nch = D // 4
    per = (nch + L - 1) // L
    pad = torch.zeros(rows, per * L * 4)
    pad[:, :D] = x
    v = pad.view(rows, per, L, 4)
    live = (torch.arange(per * L * 4) < D).view(per, L, 4)
    s = torch.zeros(rows, L)
    for i in range(per):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    mean = _tree(s) / D
    if defect == "tail_mean" and rows % 2 == 1 and rows > 1:
        mean = mean.clone()
        mean[-1] = mean[-2]
    q = torch.zeros(rows, L)
    for i in range(per):
        for j in range(4):
            d = torch.where(live[i, :, j], v[:, i, :, j] - mean[:, None], torch.zeros(()))
            q = q + d * d
    var = _tree(q) / (D - 1 if defect == "bessel" else D)
    rstd = torch.rsqrt(var + (0.0 if defect == "no_eps" else torch.tensor(eps, dtype=torch.float32)))
    y = (x - mean[:, None]) * rstd[:, None] * g + b
    return y, mean, rstd


def ln_xhat(x, mean, rstd, g, b, y16=None, dtype=torch.float64, device="cpu"):
    """The normalised value the backward works with (module docstring)."""
    c = lambda t: t.to(device=device, dtype=dtype)       # noqa: E731
    xh = (c(x) - c(mean)[:, None]) * c(rstd)[:, None]
    if y16 is None:
        return xh
    return torch.where(y16_chunks(g, b).to(device), (c(y16) - c(b)) / c(g), xh)


def ln_bwd(dy, xhat, rstd, g, dres=None, keep=None, init=None, dtype=torch.float64, device="cpu"):
    """dx = rstd (dy g - mean(dy g) - xhat mean(dy g xhat)) + dres;  dx16's value = dx * keep (keep = 0 or 1 / (1 - p));
    dgamma = init[0] + sum_r dy xhat, dbeta = init[1] + sum_r dy, dxsum = init[2] + sum_r dx keep.  dy and dres are lists of tensors that
    are added up in `dtype` first.  -> dict with dx, dxk, dgamma, dbeta, dxsum and mag (the columns' sums of |terms|, [3, D])."""
    c = lambda t: t.to(device=device, dtype=dtype)       # noqa: E731
    dy = sum(c(t) for t in dy)
    xhat, g = c(xhat), c(g)
    gy = dy * g
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xhat).mean(-1, keepdim=True)
    dx = c(rstd)[:, None] * (gy - s1 - xhat * s2)
    for t in dres or ():
        dx = dx + c(t)
    dxk = dx if keep is None else dx * c(keep)
    terms = (dy * xhat, dy, dxk)
    init = torch.zeros(3, dy.shape[-1]) if init is None else init
    sums = [c(init[k]) + terms[k].sum(0) for k in range(3)]
    return {"dx": dx, "dxk": dxk, "dgamma": sums[0], "dbeta": sums[1], "dxsum": sums[2],
            "mag": torch.stack([t.double().abs().sum(0) for t in terms]).cpu()}


def ln_step_dxsum_extra(want, yard):
    """ln_bwd16_kernel writes no fp32 dx, so its dxsum cannot be judged as the sum of what was written (judge_sum_of); against float64 each
    of its terms may be off by what the row rule allows that row of dx, and the sum by the sum of those allowances - added to the
    column bound.  (A row left out, counted twice or masked wrongly is off by a whole term: orders of magnitude more.)"""
    return cell_bounds(want["dx"], yard["dx"], -1).sum()


def ln_bwd_restated(dy, xhat32, rstd, g, dres=None, init=None, defect=None):
    """fp32 on the CPU: the two row sums sequential, columns left to right (a worse order than the kernels' lane tree); the column sums
    in the kernels' order (column_fold).  xhat32: ln_xhat(..., dtype=float32).
    defect: None | "drop_row" (row 1 missing from dgamma) | "xhat_bf16" (xhat rounded to bf16)."""
    dy = sum(t.float() for t in dy)
    xh = xhat32.float()
    if defect == "xhat_bf16":
        xh = xh.bfloat16().float()
    g, rs = g.float(), rstd.float()
    rows, D = dy.shape
    gy = dy * g
    s1, s2 = torch.zeros(rows), torch.zeros(rows)
    for d in range(D):
        s1 = s1 + gy[:, d]
        s2 = s2 + gy[:, d] * xh[:, d]
    s1, s2 = s1 / D, s2 / D
    dx = rs[:, None] * (gy - s1[:, None] - xh * s2[:, None])
    for t in dres or ():
        dx = dx + t.float()
    tg = dy * xh
    if defect == "drop_row":
        tg[1] = 0.0
    init = torch.zeros(3, D) if init is None else init.float()
    return {"dx": dx, "dgamma": column_fold(tg, init[0]), "dbeta": column_fold(dy, init[1]), "dxsum": column_fold(dx, init[2])}


def column_fold(terms, init):
    """fp32 column sums in the order of ln_bwd_kernel + ln_bwd_reduce_kernel: wave w of block b adds rows 4 b + w, + 4 G, ... (G = min(rows /
    4, 2048) blocks), a block adds its four waves, 32 slices of blocks are summed in four interleaved chains each, and the slice totals
    are added onto the initial value one by one (here in ascending order; on the device in the order the atomics arrive)."""
    rows, D = terms.shape
    G = min((rows + 3) // 4, 2048)
    K = (rows + 4 * G - 1) // (4 * G)
    pad = torch.zeros(K * G * 4, D)
    pad[:rows] = terms
    v = pad.view(K, G, 4, D)
    w = torch.zeros(G, 4, D)
    for k in range(K):
        w = w + v[k]
    blk = torch.zeros(G, D)
    for i in range(4):
        blk = blk + w[:, i]
    per = (G + 31) // 32
    out = init.clone()
    for y in range(32):
        b0, b1 = y * per, min(G, (y + 1) * per)
        if b1 <= b0:
            continue
        s = [torch.zeros(D) for _ in range(4)]
        b = b0
        while b + 4 <= b1:
            for c in range(4):
                s[c] = s[c] + blk[b + c]
            b += 4
        while b < b1:
            s[0] = s[0] + blk[b]
            b += 1
        out = out + ((s[0] + s[1]) + (s[2] + s[3]))
    return out


@functools.lru_cache(maxsize=None)
def ln_bwd_case(rows, D, family, form, mixed, half, seed):
    """The operands of one backward case, on the CPU (read-only, cached).  form: "dy32" | "dy16+dy32+dres" | "dy16+dres16" |
    "dy16+dres16+y16".  mean / rstd and y16 come from the float64 forward, not from the forward kernel."""
    eps = 1e-6
    x = ln_rows(family, rows, D, seed)
    g, b = ln_gains(D, seed + 2, mixed)
    mean, rstd = ln_stats32(x, eps)
    r = lambda s, dt=torch.float32: torch.randn(rows, D, generator=gen(seed + s)).to(dt)       # noqa: E731
    op = {"x": x, "g": g, "b": b, "mean": mean, "rstd": rstd, "dy16": None, "dy32": None, "dres": None, "dres16": None, "y16": None}
    if form == "dy32":
        op["dy32"] = r(10)
    elif form == "dy16+dy32+dres":
        op.update(dy16=r(11, half), dy32=r(12), dres=r(13))
    else:
        op.update(dy16=r(11, half), dres16=r(14, half))
        if form == "dy16+dres16+y16":
            op["y16"] = ln_fwd(x, g, b, eps)[0].to(half)
    # dgamma / dbeta / dxsum are accumulated onto random values sized, column by column, like the SUMS (u |sum of terms|, u in (-1, 1)),
    # not like the sums of |terms| the floor is stated in: the kernels fold up to 32 block partials onto the value with one atomic each,
    # every one rounding at the running total's magnitude.  Starting as high as the sum of |terms| the total runs at up to twice the
    # floor's magnitude and 9 to 32 honest roundings land between 0.9 and 1.001 of the bound, in whichever order the atomics arrive
    # (measured: dgamma of ln_bwd16 33 x 260, dbeta of ln_bwd 8200 x 64); one constant for all columns outweighs the small ones.
    op["init"] = None
    ref = ln_bwd_eval(op)
    sums = torch.stack([ref["dgamma"], ref["dbeta"], ref["dxsum"]]).abs()
    op["init"] = ((torch.rand(3, D, generator=gen(seed + 20), dtype=torch.float64) * 2 - 1) * sums).float()
    return op


def ln_bwd_eval(op, keep=None, dtype=torch.float64, device="cpu"):
    """ln_bwd on a case's operands in `dtype` on `device` (xhat formed in `dtype` too: the yardstick evaluates the whole formula)."""
    xh = ln_xhat(op["x"], op["mean"], op["rstd"], op["g"], op["b"], op["y16"], dtype, device)
    return ln_bwd([t for t in (op["dy16"], op["dy32"]) if t is not None], xh, op["rstd"], op["g"],
                  [t for t in (op["dres"], op["dres16"]) if t is not None], keep, op["init"], dtype, device)


LN_FWD_CASES = [(1, 4), (2, 64), (7, 100), (8, 132), (9, 384), (33, 512), (1, 516), (5, 768), (9, 1028), (3, 2044), (4, 2048)]
LN_FWD_FP16_CASES = [(9, 384), (9, 1028)]
LN_EPS = (1e-6, 1e-12)
LN_BWD_WIDTHS = [4, 100, 256, 260, 768, 1024, 1028, 2048]             # MAXC = 1, 1, 1, 2, 3, 4, 8, 8
LN_BWD_ROWS = [1, 5, 33]
LN_BWD_WRAP = (8200, 64)                                              # more rows than 2048 blocks x 4 waves: the row loop wraps
LN_BWD_FORMS = ["dy32", "dy16+dy32+dres", "dy16+dres16", "dy16+dres16+y16"]
LN_BWD16_FULL = [256, 512, 768, 1024, 2048]
LN_BWD16_RAGGED = [4, 100, 260, 1028, 1280]


LN_BWD_SEED = {}       # (rows, D) -> seed, for a shape whose restatement leaves half a bound at seed 1: none does (the worst sit at 0.50)


def ln_bwd_seed(rows, D):
    return LN_BWD_SEED.get((rows, D), 1)


def ln_bwd_shapes(widths):
    return [(r, D) for D in widths for r in LN_BWD_ROWS] + [LN_BWD_WRAP]


def ln_bwd_family(rows, D):
    """One family per shape (all three at every shape would triple the float64 work for nothing new): they cycle with the row count."""
    return "plain" if D == 4 else {1: "plain", 5: "scales", 33: "outlier"}.get(rows, "plain")


# ------------------------------------------------------------------------------------------------------------------------------------------
# top-k pooling
# ------------------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 1, 64, 1), (2, 5, 64, 5), (3, 8, 128, 8), (2, 33, 192, 3), (3, 257, 64, 2), (1, 300, 1024, 5)]
POOL_MASKS = ["none", "prefix", "holes", "few", "all"]


@functools.lru_cache(maxsize=None)
def pool_tokens(B, N, P, dtype, seed):
    """fp32: N(0, 1) scaled per batch row (1, 1e-2, 1e2, ...); 16-bit: the grid of multiples of 1/2, ties everywhere."""
    t = torch.randn(B, N, P, generator=gen(seed))
    if dtype == torch.float32:
        return t * torch.tensor([1.0, 1e-2, 1e2])[torch.arange(B) % 3][:, None, None]
    return ((t * 2).round() / 2).to(dtype)


def pool_mask(kind, B, N, k, seed):
    """int64 [B, N] (1 = keep) or None."""
    if kind == "none":
        return None
    m = torch.zeros(B, N, dtype=torch.int64)
    if kind == "prefix":
        for b in range(B):
            m[b, :max(1, (N * (b + 1)) // (B + 1))] = 1
    elif kind == "holes":
        m = (torch.rand(B, N, generator=gen(seed)) < 0.6).long()
        m[:, N // 2] = 1
    elif kind == "few":                          # fewer unmasked tokens than k: masked ones are selected, smallest index first
        for b in range(B):
            m[b, torch.randperm(N, generator=gen(seed + b))[:max(0, k - 1 - b)]] = 1
    return m                                     # "all": nothing kept


def pool_select(tok, mask, k, tie="first", leak=None):
    """-> (values [B, k, P] fp32, idx [B, k, P]): the k largest per channel in (value descending, index ascending) order, from a stable
    descending sort.  Masked tokens count as -10000.  tie = "last": the defect of breaking ties towards the larger index.
    leak = (b, n): the defect of treating that masked token as unmasked."""
    v = tok.float().cpu().clone()
    if mask is not None:
        m = mask.clone()
        if leak is not None:
            m[leak] = 1
        v = torch.where(m[..., None] == 0, torch.full_like(v, MASKED_VALUE), v)
    if tie == "last":
        N = v.shape[1]
        vals, idx = torch.sort(v.flip(1), dim=1, descending=True, stable=True)
        return vals[:, :k].contiguous(), (N - 1 - idx[:, :k]).contiguous()
    vals, idx = torch.sort(v, dim=1, descending=True, stable=True)
    return vals[:, :k].contiguous(), idx[:, :k].contiguous()


def pool_fwd(vals, eps, normalize, dtype=torch.float64, device="cpu"):
    """emb [B, P], norm [B] from the selected values: mean over k, then x / (|x| + eps); norm = 1 without normalisation."""
    pooled = vals.to(device=device, dtype=dtype).sum(1) / vals.shape[1]
    if not normalize:
        return pooled, torch.ones(pooled.shape[0], device=device, dtype=dtype)
    n = pooled.pow(2).sum(-1).sqrt()
    return pooled / (n[:, None] + eps), n


def pool_bwd(demb, emb, norm, k, eps, normalize, dtype=torch.float64, device="cpu"):
    """The gradient every selected token of a channel receives, [B, P]; emb and norm are inputs (the forward's fp32 results)."""
    g, y, n = (t.to(device=device, dtype=dtype) for t in (demb, emb, norm))
    if not normalize:
        return g / k
    dot = (g * y).sum(-1, keepdim=True)
    n = n[:, None]
    return (g - y * dot * (n + eps) / n.clamp_min(1e-30)) / (n + eps) / k


def pool_scatter(dx, idx, N):
    """[B, P] values onto the selected tokens -> dense [B, N, P], zero elsewhere."""
    B, k, P = idx.shape
    out = torch.zeros(B, N, P, dtype=dx.dtype)
    return out.scatter_(1, idx.long(), dx[:, None, :].expand(B, k, P).contiguous())


# ------------------------------------------------------------------------------------------------------------------------------------------
# column sums, row norms
# ------------------------------------------------------------------------------------------------------------------------------------------
COLSUM_ROWS = [1, 7, 8, 9, 300, 4100]
COLSUM_N = [8, 264, 776]
RNORM_ROWS = [1, 3, 5, 130]
RNORM_D = [4, 260, 512, 1000]


def half_grid(shape, seed, span=8):
    """Multiples of 1/2 in [-span / 2, span / 2): exact in bf16 and fp16, and every fp32 sum of up to 2^20 of them is exact in any order."""
    return torch.randint(-span, span, shape, generator=gen(seed)).float() / 2


def rnorm(x, eps, dtype=torch.float64, device="cpu"):
    x = x.to(device=device, dtype=dtype)
    return 1.0 / x.pow(2).sum(-1).sqrt().clamp_min(eps)
