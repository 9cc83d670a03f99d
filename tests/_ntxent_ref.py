"""Float64 statement of the NT-Xent row kernel, written from the formulas of include/simseg_hip.h (simseg_ntxent_rows) in closed form - no
autograd, no code shared with the device path -, the torch statements of the loss the tests differentiate (SLIP's SIMCLRLoss: four logit
blocks, a -1e9 self mask, two cross-entropies and their mean; and the masked cross-entropy of one stacked block), and the input tables the
host and the GPU tests share.  ntxent_eval takes a dtype and a device: in float64 on the CPU it is the reference, in fp32 on the device
the yardstick of tests/test_gpu_loss_head.py.

Every similarity block is s = G[target0 : target0 + N1] @ G.T of unit rows G [N2, 64] in fp32 on the CPU: each row really holds its
self-similarity 1.0, its largest entry, in its own column."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

T_LO, T_HI = float(np.float32(0.001)), 0.5          # the kernel's clamp constants are fp32 numbers: 0.001f is not 1e-3
SETTINGS = [0.1, 0.05, 0.5, 0.7]                    # T; the clamp makes 0.7 act as 0.5, with dLoss/dT = 0
# (N1, N2, target0): one non-self column (loss and every gradient exactly 0, accuracy 1); the smallest block with negatives; one wave, the
# own block in the last columns; 256 + 1 columns; rank 2 of 4; several columns per thread; more rows than threads
SHAPES = [(2, 2, 0), (4, 4, 0), (6, 64, 58), (34, 257, 102), (98, 392, 196), (64, 1000, 936), (300, 300, 0)]
FAMILIES = ("random", "aligned")
# Seeds (block 0, block 1) for which margin_ok holds on every listed block (tests/test_ntxent_host.py asserts it; the GPU tests assert it
# again before they compare).  A seed that fails is replaced here, never skipped there.
SEEDS = {(f, N1, N2): (1, 2) for f in FAMILIES for N1, N2, _ in SHAPES}
SEEDS["random", 64, 1000] = (2, 3)
HEAD_SHAPES = [(1, 64), (3, 64), (17, 72), (49, 128)]          # (B, P) of the autograd-node tests
HEAD_SEEDS = {bp: 1 for bp in HEAD_SHAPES}


def unit_rows(n, d, seed):
    return F.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=-1)


@functools.lru_cache(maxsize=None)
def sim_block(family, N1, N2, target0, seed):
    """[N1, N2] fp32 on the CPU, read-only.  "random": independent rows, the positive is one column among many (accuracy near 0).
    "aligned": view b's rows are view a's plus noise of 1.5 times their norm, so that most rows find their positive."""
    B = N1 // 2
    G = unit_rows(N2, 64, seed)
    if family == "aligned":
        G = G.clone()
        G[target0 + B:target0 + N1] = F.normalize(G[target0:target0 + B] + 1.5 * unit_rows(B, 64, seed + 100000), dim=-1)
    return G[target0:target0 + N1] @ G.T


def blocks(family, N1, N2, target0):
    """[2, N1, N2]: the two blocks of the table's seeds."""
    return torch.stack([sim_block(family, N1, N2, target0, seed) for seed in SEEDS[family, N1, N2]])


@functools.lru_cache(maxsize=None)
def head_embeddings(B, P, seed):
    """(a [B, P], b [B, P], gathered [6 B, P]) fp32 unit rows on the CPU, read-only: view b is view a plus noise of three times its norm;
    `gathered` is what rank 1 of 3 holds after the exchange of the stacked [2B, P] tensors - cat([a, b]) in rows [2B, 4B)."""
    a = unit_rows(B, P, seed)
    b = F.normalize(a + 3.0 * unit_rows(B, P, seed + 1), dim=-1)
    o = unit_rows(4 * B, P, seed + 2)
    return a, b, torch.cat([o[:2 * B], a, b, o[2 * B:]])


def _layout(N1, N2, target0, device):
    idx = torch.arange(N1, device=device)
    own, pos = target0 + idx, target0 + (idx + N1 // 2) % N1
    is_self = torch.arange(N2, device=device)[None, :] == own[:, None]
    return idx, pos, is_self


def first_max(z):
    """The kernels' top-1 rule: the first index attaining the row maximum."""
    idx = torch.arange(z.shape[1], device=z.device).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, z.shape[1])).min(1).values


def _acc32(hit):
    """hits / rows as the one fp32 division the finalize kernel makes."""
    return (torch.tensor(float(hit.sum()), dtype=torch.float32) / torch.tensor(float(hit.numel()), dtype=torch.float32)).item()


def ntxent_eval(s, T, target0, dtype=torch.float64, device="cpu"):
    """One [N1, N2] block, N1 = 2B.  T: the temperature before the clamp.  -> dict(rows, total, ds, dt, acc_a, acc_b, z); z holds -inf in
    every row's own column."""
    s = s.to(device=device, dtype=dtype)
    N1, N2 = s.shape
    B = N1 // 2
    idx, pos, is_self = _layout(N1, N2, target0, device)
    T = torch.as_tensor(T, dtype=torch.float32).to(device=device, dtype=dtype).reshape(())          # an fp32 value: what the kernel reads
    temp = torch.clamp(T, T_LO, T_HI)
    inv_t = 1 / temp
    z = (s * inv_t).masked_fill(is_self, float("-inf"))
    m = z.max(1).values
    lg = torch.log(torch.exp(z - m[:, None]).sum(1))
    rows = (m - z[idx, pos]) + lg
    dz = torch.exp((z - m[:, None]) - lg[:, None])                # exp(-inf) = 0: exactly 0 in the own column
    dz[idx, pos] -= 1
    dz = dz / N1
    inside = T_LO <= float(T) <= T_HI                             # the kernel's test on the fp32 temperature
    dt = -(dz * s).sum() / (temp * temp) if inside else torch.zeros((), device=device, dtype=dtype)
    hit = (first_max(z) == pos).cpu()
    return {"rows": rows, "total": rows.sum() / N1, "ds": dz * inv_t, "dt": dt, "acc_a": _acc32(hit[:B]), "acc_b": _acc32(hit[B:]), "z": z}


def ntxent_torch(s, T, target0):
    """The loss of one stacked block as one writes it in torch, in s's dtype on s's device (autograd flows to whatever requires it): the
    own column pushed out of the softmax by -1e9, a cross-entropy against the positive's column, the mean over the 2B rows."""
    N1, N2 = s.shape
    _, pos, is_self = _layout(N1, N2, target0, s.device)
    logits = s / torch.clamp(T, T_LO, T_HI) - is_self.to(s.dtype) * 1e9
    return F.cross_entropy(logits, pos)


def slip_torch(s, T, target0):
    """SLIP's SimCLR loss statement (Mu et al., ECCV'22) read off the stacked block of rank target0 / N1 of N2 / N1: the four logit blocks
    a.a, a.b, b.a, b.b against the gathered views, -1e9 on the a.a and b.b diagonals of the own rank, two cross-entropies over
    cat([cross, same]) with labels rank * B + i, and their mean."""
    N1, N2 = s.shape
    B = N1 // 2
    assert N2 % N1 == 0 and target0 % N1 == 0
    W, rank = N2 // N1, target0 // N1
    ka = (torch.arange(W, device=s.device)[:, None] * N1 + torch.arange(B, device=s.device)[None, :]).reshape(-1)      # gathered view a
    kb = ka + B
    tau = torch.clamp(T, T_LO, T_HI)
    labels = rank * B + torch.arange(B, device=s.device)
    masks = F.one_hot(labels, W * B).to(s.dtype) * 1e9
    aa, ab = s[:B][:, ka] / tau - masks, s[:B][:, kb] / tau
    ba, bb = s[B:][:, ka] / tau, s[B:][:, kb] / tau - masks
    loss_a = F.cross_entropy(torch.cat([ab, aa], 1), labels)
    loss_b = F.cross_entropy(torch.cat([ba, bb], 1), labels)
    return (loss_a + loss_b) / 2


def margin_ok(z):
    """Every row's best non-self logit exceeds its second best by more than 1e-4 of the row's largest non-self magnitude (z: ntxent_eval's,
    -inf in the own column; a row with one other column has no second best).  The ratio does not depend on T."""
    N1, N2 = z.shape
    if N2 < 3:
        return True
    rest = z[torch.isfinite(z)].view(N1, N2 - 1)
    top = rest.topk(2, dim=1).values
    return bool(((top[:, 0] - top[:, 1]) > 1e-4 * rest.abs().max(1).values).all())
