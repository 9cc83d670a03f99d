"""What tests/test_gpu_attention.py and tests/test_attention_ref_host.py share: the float64 reference of fused softmax attention, the
emulation that rounds to the 16-bit type where the kernels round (the yardstick), and the per-block error rule.  Plain torch; runs on
the CPU or on the device.  Every tensor here is in the [B, H, T, 64] layout (split()), the log-sum-exp in [B, H, T].

Blocks.  Errors are never pooled across sequences, heads or q / k / v: a block is one (sequence, head, component, 32-row tile) cell -
query rows for out and dq, key rows for dk and dv, the unit one wave owns in every kernel; lse is one block per (sequence, head); the
bias gradient (column sums of dqkv) one block per (component, head).

Rule for the 16-bit kernels.  With E the block's error against float64 and Y the LARGER of the two emulation variants' errors:
    E_rms <= 2 * Y_rms + floor / sqrt(n)   and   E_max <= 4 * Y_max + floor,
    floor = 2 ulps of the output type at the block's largest |reference|, n = the block's element count.
Absolute figures, no normalisation.  The floor allows ONE element to land 2 ulps off at the block's largest magnitude whatever the
yardstick says; in an RMS over n elements that event weighs 1 / sqrt(n).  (Taken whole, the floor would set the RMS bound of a
2048-element block ~20 x above the yardstick - a correct rounding leaves an RMS of ~0.3 ulp at the TYPICAL magnitude - and a 1 % scale
error would pass.  lse, the bias gradient and the fp32 rule keep the whole floor: their yardsticks can be a few fp32 ulps or zero.)
One variant judged by the other alone reaches 2.3 / 3.3, so a single variant is no safe yardstick; 2 and 4 are for what neither models:
the hardware exp2, the MFMA's accumulation order, the online-softmax rescales.  A 1 % error in the softmax scale gives 5-9 x the
yardstick's RMS and fails (test_attention_ref_host.py).
Rule for the fp32 kernels: the same formula in fp32 torch is the one yardstick, 8 x yardstick + 4 fp32 ulps, on both measures.

Blocks whose float64 reference is identically zero by CANCELLATION - the dq and dk of a sequence with one unmasked key: P = 1, so dS =
P (dP - delta) is an fp32 residue - are held to |got| <= 2^-12 x the largest |dv| of the same sequence and head (a mask leak gives
values of order scale * dv, at least 2^-4 of it; the residue of 64 cancelled fp32 products is about 2^-17 of it).  They are found from
the reference - dq or dk of a (sequence, head) whose whole component is zero - and counted; the tests assert the count.  A block that is
zero because its keys are masked (P = 0) has a zero yardstick and a zero floor too: it must be exactly zero.
With dropout that residue is NOT an fp32 one: delta = rowsum(dO * O) is formed from the ROUNDED forward output, O = rnd(v / (1 - p)),
while keep * dP carries the unrounded factor, so dS is a 16-bit rounding residue of dO . v (2^-9 of it in bf16), about 2^-9 of dv per
query row and its sum over the rows in dk - above 2^-12 of dv in both emulation variants (test_attention_ref_host.py shows it).  There
the yardstick is not zero and is the right scale, so a counted zero-reference block passes if it meets the ordinary two bounds OR the
2^-12 bound; without dropout the ordinary bounds are an fp32 residue against a zero floor and the 2^-12 bound is the one that decides.
A mask leak (>= 2^-4 of dv) is far outside both."""
import math

import torch

LOG2E = 1.4426950408889634
PREC = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}       # significand bits, the implicit one included
RMS_FACTOR, MAX_FACTOR, FLOOR_ULPS = 2.0, 4.0, 2.0                     # 16-bit kernels against the larger of the two emulation variants
F32_FACTOR, F32_FLOOR_ULPS = 8.0, 4.0                                  # fp32 kernels against fp32 torch (the loss-head rule)
ZERO_REF_BOUND = 2.0 ** -12
COMPONENTS = ("dq", "dk", "dv")


def split(x, H):
    """[B, T, n * H * 64] -> [n, B, H, T, 64] (a view)."""
    B, T, W = x.shape
    return x.view(B, T, W // (H * 64), H, 64).permute(2, 0, 3, 1, 4)


def key_mask(lens, T):
    """[B, T] bool, True = attend: prefix masks of the given lengths."""
    return torch.arange(T)[None, :] < torch.tensor(lens)[:, None]


def randn16(shape, seed, scale, dtype):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def reference(qkv, dout, H, scale, lens=None, keep=None, dtype=torch.float64, device="cpu", q_div=1.0):
    """softmax(q k^T scale, masked keys at -inf) * keep @ v on exactly the values given, gradients from autograd, lse = logsumexp / ln 2.
    keep: [B, H, T, T] holding 0 or 1 / (1 - p).  q_div: a factor folded into q that is divided out again (attention_fwd_qscaled)."""
    x = qkv.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(dout is not None)
    q, k, v = split(x, H)
    s = (q / q_div if q_div != 1.0 else q) @ k.transpose(-1, -2) * scale
    if lens is not None:
        s = s.masked_fill(~key_mask(lens, s.shape[-1]).to(device)[:, None, None, :], float("-inf"))
    p = s.softmax(-1)
    if keep is not None:
        p = p * keep.to(device=device, dtype=dtype)
    o = p @ v
    res = {"out": o.detach(), "lse": (torch.logsumexp(s, -1) / math.log(2)).detach()}
    if dout is not None:
        o.backward(split(dout.to(device=device, dtype=dtype), H)[0])
        res["dq"], res["dk"], res["dv"] = split(x.grad, H)
    return res


def emulate(qkv, dout, H, scale, lens=None, keep=None, variant="A", rnd=torch.bfloat16, cdt=torch.float32, device="cpu", qscaled=False):
    """The kernels' arithmetic in `cdt` torch with the roundings to `rnd` (None: none) where they round.
    Forward A: O = rnd(P) V with P normalised;  B: O = (rnd(exp2(s - m)) V) / l, l summed from the unrounded exponentials;  O rounded,
    lse = m + log2 l kept in cdt.  Backward after either: P = exp2(s c - lse); delta = rowsum(dO * O_rounded); dS = rnd(P (keep dP -
    delta)); dV = rnd(P keep)^T dO; dQ = scale dS K; dK = scale dS^T Q; outputs rounded.  (With dropout dS is P (keep dP - delta), not
    P keep (dP - delta): a dropped probability still moves the row's normaliser.  test_attention_ref_host.py holds this against autograd.)"""
    R = (lambda t: t) if rnd is None else (lambda t: t.to(rnd).to(cdt))
    q, k, v = split(qkv.to(device=device, dtype=cdt), H)
    s = (q @ k.transpose(-1, -2)) * (1.0 if qscaled else scale * LOG2E)
    if lens is not None:
        s = s.masked_fill(~key_mask(lens, s.shape[-1]).to(device)[:, None, None, :], float("-inf"))
    kp = 1.0 if keep is None else keep.to(device=device, dtype=cdt)
    m = s.amax(-1, keepdim=True)
    pu = torch.exp2(s - m)
    l = pu.sum(-1, keepdim=True)
    o = R(pu / l * kp) @ v if variant == "A" else (R(pu * kp) @ v) / l
    o16 = R(o)
    lse = m + torch.log2(l)
    res = {"out": o16, "lse": lse.squeeze(-1)}
    if dout is not None:
        do = split(dout.to(device=device, dtype=cdt), H)[0]
        P = torch.exp2(s - lse)
        delta = (do * o16).sum(-1, keepdim=True)
        dS = R(P * (kp * (do @ v.transpose(-1, -2)) - delta))
        res["dv"] = R(R(P * kp).transpose(-1, -2) @ do)
        res["dq"] = R(scale * (dS @ k))
        res["dk"] = R(scale * (dS.transpose(-1, -2) @ q))
    return res


def ulp(mag, prec):
    """Spacing of the numbers with `prec` significand bits at magnitude mag (tensor; 0 at 0: an exactly-zero reference is compared exactly)."""
    e = torch.frexp(mag.double())[1].clamp_min(-125)
    return torch.where(mag > 0, torch.ldexp(torch.ones_like(mag, dtype=torch.float64), e - prec), torch.zeros_like(mag, dtype=torch.float64))


def block_stats(x, valid, rows=32):
    """x [B, H, T, d] float64, valid [B, T] bool (rows that exist / that the caller reads) -> per block of `rows` rows (None: all T):
    (rms [B, H, nb], largest magnitude [B, H, nb], valid elements [B, 1, nb])."""
    B, H, T, d = x.shape
    rows = T if rows is None else rows
    nb = (T + rows - 1) // rows
    pad = nb * rows - T
    x = torch.where(valid[:, None, :, None], x.double(), torch.zeros((), dtype=torch.float64))
    x = torch.nn.functional.pad(x, (0, 0, 0, pad)).reshape(B, H, nb, rows * d)
    cnt = torch.nn.functional.pad(valid, (0, pad)).reshape(B, 1, nb, rows).sum(-1) * d
    return (x.pow(2).sum(-1) / cnt.clamp_min(1)).sqrt(), x.abs().amax(-1), cnt


def judge(got, ref, yards, valid, prec, rows=32, f32_rule=False):
    """The rule of the module docstring for one component.  -> dict(rms, max: worst E / Y ratios over the live blocks (0 where E = Y = 0),
    blocks: live blocks, ok [B, H, nb] bool, E_rms, E_max, Y_rms, Y_max, floor)."""
    ref = ref.double().cpu()
    e_rms, e_max, cnt = block_stats(got.double().cpu() - ref, valid, rows)
    live = cnt > 0
    ys = [block_stats(y.double().cpu() - ref, valid, rows) for y in yards]
    y_rms = torch.stack([y[0] for y in ys]).amax(0)
    y_max = torch.stack([y[1] for y in ys]).amax(0)
    fr, fm, fu = (F32_FACTOR, F32_FACTOR, F32_FLOOR_ULPS) if f32_rule else (RMS_FACTOR, MAX_FACTOR, FLOOR_ULPS)
    floor = fu * ulp(block_stats(ref, valid, rows)[1], prec)
    # the floor is the allowance for ONE element landing 2 ulps off at the block's largest magnitude; in the RMS over n elements that event
    # weighs 1 / sqrt(n).  (16-bit tensors only: with the whole floor the RMS bound of a 2048-element block is ~20 x the yardstick and a
    # 1 % scale error passes it; lse and the fp32 rule keep the whole floor - their yardsticks can be a few fp32 ulps or zero)
    floor_rms = floor / cnt.clamp_min(1).double().sqrt() if (rows is not None and not f32_rule) else floor
    ok = (e_rms <= fr * y_rms + floor_rms) & (e_max <= fm * y_max + floor) | ~live        # (a NaN error compares false)

    def worst(e, y):
        r = torch.where(e == 0, torch.zeros_like(e), e / y)        # E > 0 over Y = 0: inf
        return r[live.expand_as(r)].max().item() if live.any() else 0.0
    return {"rms": worst(e_rms, y_rms), "max": worst(e_max, y_max), "blocks": int(live.expand_as(ok).sum()), "ok": ok, "live": live,
            "E_rms": e_rms, "E_max": e_max, "Y_rms": y_rms, "Y_max": y_max, "floor": floor, "floor_rms": floor_rms.expand_as(floor)}


def zero_ref_cells(ref, comp, valid):
    """[B, H] bool: the whole `comp` (dq or dk) of this (sequence, head) is identically zero in the float64 reference on its valid rows
    while the sequence has a valid row - zero by cancellation (one unmasked key)."""
    z = torch.where(valid[:, None, :, None], ref[comp].double().cpu(), torch.zeros((), dtype=torch.float64)).abs().amax((2, 3)) == 0
    return z & valid.any(1)[:, None]


def expected_zero_ref_blocks(lens, valid, H, rows=32, colsum=False):
    """2 * H * (tiles holding a valid row) per sequence with exactly one unmasked key; with the bias gradient 2 * H more (its dq and
    dk block of every head) when EVERY sequence has one key - else the column sums are not zero."""
    T = valid.shape[1]
    nb = (T + rows - 1) // rows
    tiles = torch.nn.functional.pad(valid, (0, nb * rows - T)).reshape(-1, nb, rows).any(-1).sum(-1)
    n = sum(2 * H * int(tiles[b]) for b, n in enumerate(lens) if n == 1)
    return n + (2 * H if colsum and all(n == 1 for n in lens) else 0)


def judge_all(got, ref, yards, valid, prec, kinds, f32_rule=False):
    """Every kind in `kinds` (out, lse, dq, dk, dv) -> {kind: judge() result + 'zero': blocks that took the zero-reference path + 'bad':
    failing (b, h, block) triples}.  dq / dk blocks of zero_ref_cells may meet the |got| <= 2^-12 max |dv| bound instead of the rule
    (module docstring); they are left out of the printed worst ratios."""
    res = {}
    for kind in kinds:
        if kind == "lse":
            r = judge(got[kind][..., None], ref[kind][..., None], [y[kind][..., None] for y in yards], valid, 24, rows=None, f32_rule=f32_rule)
        else:
            r = judge(got[kind], ref[kind], [y[kind] for y in yards], valid, prec, f32_rule=f32_rule)
        r["zero"] = 0
        if kind in ("dq", "dk"):
            cells = zero_ref_cells(ref, kind, valid)                                   # [B, H]
            if cells.any():
                g_max = block_stats(got[kind].double().cpu(), valid)[1]
                dv_max = torch.where(valid[:, None, :, None], ref["dv"].double().cpu(), torch.zeros((), dtype=torch.float64)).abs().amax((2, 3))
                path = cells[:, :, None] & r["live"]
                r["ok"] = torch.where(path, r["ok"] | (g_max <= ZERO_REF_BOUND * dv_max[:, :, None]), r["ok"])
                r["zero"] = int(path.sum())
                rest = r["live"].expand_as(path) & ~path
                for key, e, y in (("rms", r["E_rms"], r["Y_rms"]), ("max", r["E_max"], r["Y_max"])):
                    q = torch.where(e == 0, torch.zeros_like(e), e / y)
                    r[key] = q[rest].max().item() if rest.any() else 0.0
        r["bad"] = [tuple(i) for i in (~r["ok"]).nonzero().tolist()]
        res[kind] = r
    return res


def judge_colsum(got, ref, yards, valid, H, f32_rule=False):
    """The bias gradient: got fp32 [3 * H * 64] against the column sums of the float64 dqkv over the valid rows; yardstick: the fp32 column
    sums of each emulation's ROUNDED dqkv (what a column-sum pass over the written gradient gives).  One block per (component, head).
    A dq / dk block whose reference sum is identically zero (every sequence has one key) may meet 2^-12 of the head's largest dv sum
    instead, and is counted, as in judge_all."""
    w = valid[:, None, :, None]
    zero = torch.zeros((), dtype=torch.float64)

    def sums(d, dt):
        return torch.stack([torch.where(w, d[c].cpu().to(dt), zero.to(dt)).sum((0, 2)) for c in COMPONENTS]).double()      # [3, H, 64]
    want = sums(ref, torch.float64)
    e = got.double().cpu().view(3, H, 64) - want
    ys = [sums(y, torch.float32) - want for y in yards]
    e_rms, e_max = e.pow(2).mean(-1).sqrt(), e.abs().amax(-1)
    y_rms = torch.stack([y.pow(2).mean(-1).sqrt() for y in ys]).amax(0)
    y_max = torch.stack([y.abs().amax(-1) for y in ys]).amax(0)
    fr, fm, fu = (F32_FACTOR, F32_FACTOR, F32_FLOOR_ULPS) if f32_rule else (RMS_FACTOR, MAX_FACTOR, FLOOR_ULPS)
    floor = fu * ulp(want.abs().amax(-1), 24)
    floor_rms = floor
    ok = (e_rms <= fr * y_rms + floor) & (e_max <= fm * y_max + floor)
    path = want.abs().amax(-1) == 0
    path[2] = False
    ok = ok | (path & (got.double().cpu().view(3, H, 64).abs().amax(-1) <= ZERO_REF_BOUND * want[2].abs().amax(-1)[None, :]))

    def q(a, b):
        r = torch.where(a == 0, torch.zeros_like(a), a / b)[~path]
        return r.max().item() if r.numel() else 0.0
    return {"rms": q(e_rms, y_rms), "max": q(e_max, y_max), "blocks": 3 * H, "zero": int(path.sum()), "bad": [tuple(i) for i in (~ok).nonzero().tolist()],
            "E_rms": e_rms, "E_max": e_max, "Y_rms": y_rms, "Y_max": y_max, "floor": floor, "floor_rms": floor_rms}


def describe(r, limit=4):
    """The figures of the first failing blocks of a judge() / judge_colsum() result."""
    out = []
    for i in r["bad"][:limit]:
        out.append(f"block {i}: E_rms {r['E_rms'][i].item():.3e} Y_rms {r['Y_rms'][i].item():.3e} E_max {r['E_max'][i].item():.3e} "
                   f"Y_max {r['Y_max'][i].item():.3e} floor {r['floor'][i].item():.3e} (rms: {r['floor_rms'][i].item():.3e})")
    return f"{len(r['bad'])} of {r['blocks']} blocks over the bound; " + "; ".join(out)
