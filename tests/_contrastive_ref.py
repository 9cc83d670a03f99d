"""Float64 statements of the Triplet and MixUpNCE row kernels, written from the formulas of include/simseg_hip.h (simseg_triplet_rows,
simseg_mix_nce_rows) in closed form - no autograd -, and the input tables the host and the GPU tests share.  The *_eval forms take a
dtype and a device: in float64 on the CPU they are the reference, in fp32 on the device the yardstick of tests/test_gpu_loss_head.py."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 0.2
# (N1, N2, target0): a row shorter than a wave; shorter than a block; 256 + 1 elements; several elements per thread; the target in the last
# columns; rank != 0 of a gathered batch; fully masked rows (N2 == N1 with the block mask)
SHAPES = [(2, 2, 0), (5, 5, 0), (3, 64, 61), (33, 257, 100), (97, 388, 194), (64, 1000, 936), (300, 300, 0)]
FAMILIES = ("random", "aligned")
# Seeds (block 0, block 1) chosen on the CPU so that case_ok holds for every listed block (tests/test_contrastive_losses_host.py asserts
# it; the GPU tests assert it again before they compare).  A seed that fails is replaced here, never skipped there.
SEEDS = {("random", 2, 2): (1, 2), ("random", 5, 5): (1, 2), ("random", 3, 64): (2, 3), ("random", 33, 257): (2, 3),
         ("random", 97, 388): (2, 8), ("random", 64, 1000): (2, 3), ("random", 300, 300): (4, 8),
         ("aligned", 2, 2): (1, 2), ("aligned", 5, 5): (1, 2), ("aligned", 3, 64): (1, 2), ("aligned", 33, 257): (1, 2),
         ("aligned", 97, 388): (1, 2), ("aligned", 64, 1000): (1, 2), ("aligned", 300, 300): (1, 2)}
HEAD_SHAPES = [(5, 64), (33, 72), (97, 128)]          # (N1, P) of the autograd-node tests
HEAD_SEEDS = {(5, 64): 1, (33, 72): 1, (97, 128): 10}


def _unit_rows(n, d, seed):
    return F.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=-1)


@functools.lru_cache(maxsize=None)
def sim_block(family, N1, N2, target0, seed):
    """[N1, N2] fp32 on the CPU, read-only: products of unit-norm rows at D = 64.  "random": independent rows, many violations.
    "aligned": the target rows are the left rows plus noise of 1.5 times their norm (s_ii ~ 0.55), so that a share of rows has no
    violation at margin 0.2."""
    f1 = _unit_rows(N1, 64, seed)
    f2 = _unit_rows(N2, 64, seed + 100000)
    if family == "aligned":
        f2 = f2.clone()
        f2[target0:target0 + N1] = F.normalize(f1 + 1.5 * _unit_rows(N1, 64, seed + 200000), dim=-1)
    return f1 @ f2.T


def sim_blocks(family, N1, N2, target0):
    """[2, N1, N2]: the two blocks of the table's seeds (block 0 serves the single-block calls, both the stacked ones)."""
    return torch.stack([sim_block(family, N1, N2, target0, seed) for seed in SEEDS[family, N1, N2]])


@functools.lru_cache(maxsize=None)
def head_embeddings(N1, P, seed):
    """(img [N1, P], txt [N1, P], gathered [3 N1, P]) fp32 unit rows on the CPU, read-only: the captions are their images plus noise of
    three times the norm (s_ii ~ 0.3: rows with and rows without a violation at margin 0.2); `gathered` is what rank 1 of 3 would hold
    after the exchange - txt in rows [N1, 2 N1), other ranks' rows around it."""
    img = _unit_rows(N1, P, seed)
    txt = F.normalize(img + 3.0 * _unit_rows(N1, P, seed + 1), dim=-1)
    others = _unit_rows(2 * N1, P, seed + 2)
    return img, txt, torch.cat([others[:N1], txt, others[N1:]])


def head_cases(N1, P):
    """(name, similarity block, target0) of every block the autograd-node tests score."""
    img, txt, gathered = head_embeddings(N1, P, HEAD_SEEDS[N1, P])
    return [("global", img @ gathered.T, N1), ("local", img @ txt.T, 0), ("local^T", (img @ txt.T).T.contiguous(), 0)]


def margin32(margin):
    """The C ABI takes the margin as a float: the value the kernel adds."""
    return float(np.float32(margin))


def first_max(z):
    """The kernels' top-1 rule: the first index attaining the row maximum."""
    idx = torch.arange(z.shape[1], device=z.device).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, z.shape[1])).min(1).values


def acc32(z, target0, keep=None):
    """hits / kept rows as the one fp32 division the finalize kernels make."""
    hit = (first_max(z) == torch.arange(target0, target0 + z.shape[0], device=z.device)).cpu()
    keep = torch.ones_like(hit) if keep is None else keep.cpu()
    return (torch.tensor(float((hit & keep).sum()), dtype=torch.float32) / torch.tensor(float(keep.sum()), dtype=torch.float32)).item()


def triplet_eval(s, target0, margin, reduce, mask_block, dtype=torch.float64, device="cpu"):
    """One [N1, N2] block.  reduce: 0 mean, 1 max.  -> dict(rows, total, ds, acc, pre, unmasked, cost)"""
    s = s.to(device=device, dtype=dtype)
    N1, N2 = s.shape
    idx = torch.arange(N1, device=device)
    tgt = target0 + idx
    cols = torch.arange(N2, device=device)[None, :]
    pre = (margin32(margin) + s) - s[idx, tgt][:, None]
    masked = ((cols >= target0) & (cols < target0 + N1)).expand(N1, N2) if mask_block else cols == tgt[:, None]
    passes = ~masked & (pre > 0)                                  # gradient flows through the clamp iff pre > 0
    cost = torch.where(passes, pre, torch.zeros_like(pre))
    ds = torch.zeros_like(s)
    if reduce == 0:
        rows = cost.sum(1) / (N1 - 1)
        ds = passes.to(dtype) / (N1 - 1)
        ds[idx, tgt] = -passes.sum(1).to(dtype) / (N1 - 1)
    else:
        rows = cost.max(1).values
        arg = first_max(torch.where(masked, torch.full_like(cost, -1.0), cost))      # the FIRST unmasked column attaining the maximum
        hot = rows > 0
        ds[idx[hot], arg[hot]] = 1.0
        ds[idx[hot], tgt[hot]] = -1.0
    return {"rows": rows, "total": rows.sum(), "ds": ds, "acc": acc32(s, target0), "pre": pre, "unmasked": ~masked, "cost": cost}


def triplet_ref(s, target0, margin, reduce, mask_block):
    r = triplet_eval(s, target0, margin, reduce, mask_block)
    return r["rows"], r["total"], r["ds"], r["acc"]


def mix_nce_eval(s, T, target0, alpha, smoothing, ign=None, dtype=torch.float64, device="cpu"):
    """One [N1, N2] block.  T: the temperature before the clamp; alpha: a float or an [N1] tensor; ign: [N1] ignore weights or None.
    -> dict(rows, total, ds, dt, acc, z)"""
    s = s.to(device=device, dtype=dtype)
    N1, N2 = s.shape
    idx = torch.arange(N1, device=device)
    a, b = target0 + idx, target0 + (N1 - 1 - idx)
    al = torch.as_tensor(alpha, dtype=torch.float32).to(device=device, dtype=dtype).reshape(-1).expand(N1)
    T = torch.as_tensor(T, dtype=torch.float32).to(device=device, dtype=dtype).reshape(())
    temp = torch.clamp(T, 1e-3, 0.5)
    z = s / temp
    logp = torch.log_softmax(z, -1)
    w = torch.ones(N1, device=device, dtype=dtype) if ign is None else 1 - ign.to(device=device, dtype=dtype)
    rows = ((1 - smoothing) * (al * -logp[idx, a] + (1 - al) * -logp[idx, b]) + smoothing * -logp.mean(-1)) * w
    dz = logp.exp() - smoothing / N2
    dz[idx, a] -= (1 - smoothing) * al
    dz[idx, b] -= (1 - smoothing) * (1 - al)                      # (a == b: both terms land on the same column)
    dz = dz * (w / N1)[:, None]
    inside = float(np.float32(0.001)) <= float(T) <= 0.5          # the kernel's test on the fp32 temperature
    dt = -(dz * s).sum() / (temp * temp) if inside else torch.zeros((), device=device, dtype=dtype)
    keep = None if ign is None else ign < 1
    return {"rows": rows, "total": rows.sum() / N1, "ds": dz / temp, "dt": dt, "acc": acc32(z, target0, keep), "z": z}


def mix_nce_ref(s, T, target0, alpha, smoothing, ign=None):
    r = mix_nce_eval(s, T, target0, alpha, smoothing, ign)
    return r["rows"], r["total"], r["ds"], r["acc"]


def margin_ok(z):
    """_margin_ok of tests/test_gpu_loss_head.py: every row's best value exceeds its second best by more than 1e-4 of the row's largest
    magnitude (a one-column row has no second best)."""
    from test_gpu_loss_head import _margin_ok
    return _margin_ok(z)


def case_ok(s, target0, margin=MARGIN):
    """The three conditions under which the exact comparisons of one [N1, N2] block are well posed, in float64, for both mask modes:
    no unmasked |pre_ij| < 1e-5 (the clamp's side is not a matter of rounding); in max mode every row with a violation has its best cost
    more than 1e-5 above its second best (a row without one has a zero gradient whatever the order of its zeros); the top-1 margin.
    -> list of the conditions that fail (empty: fine)."""
    bad = []
    for mask_block in (0, 1):
        r = triplet_eval(s, target0, margin, 1, mask_block)
        if bool((r["pre"].abs()[r["unmasked"]] < 1e-5).any()):
            bad.append(f"mask_block={mask_block}: an unmasked |pre| below 1e-5")
        if r["cost"].shape[1] >= 2:
            top = r["cost"].topk(2, dim=1).values
            if bool(((top[:, 0] > 0) & (top[:, 0] - top[:, 1] <= 1e-5)).any()):
                bad.append(f"mask_block={mask_block}: best and second best cost within 1e-5")
    if not margin_ok(s.double()):
        bad.append("top-1 margin")
    return bad
