#!/usr/bin/env python
"""The contrastive task's loss heads, forward + backward from the embeddings, against the reference's torch statements on the SAME
features: NCE (heads.NCEFn), MixUpNCE (heads.MixNCEFn, per-row alpha), Triplet-max and Triplet-mean (heads.TripletFn - the global
direction with the own-rank block masked), at P = 512 on similarity blocks of [512, 512] and [512, 4096] (rank 1 of 8 for the wide
one; [512, 512] is the one-rank case, where the Triplet's block mask covers every column and loss and gradients are 0 on both routes).
The local symmetric Triplet (heads.TripletLocalFn) is timed at [512, 512] as well.  SigLip (heads.SigLipFn, the pairwise sigmoid loss
at T = 0.1, b = -10, gradients w.r.t. the temperature and the bias too) has no statement in the reference: its torch route is
-F.logsigmoid(y * (s / T + b)).sum() / N1.  NTXent (heads.NTXentFn, SimCLR's loss over two stacked views at T = 0.1: the 512 rows are 256
images' view a on their view b, the own block of the gathered matrix holds the same rows) is timed against SLIP's torch statement: four
logit blocks, a -1e9 self mask, two cross-entropies and their mean.

All in one process on one GPU, routes interleaved round by round; every window is `--iters` back-to-back iterations between two device
events.  Median [min .. max] over `--rounds` windows, and the loss both routes computed.

    python tools/contrastive_loss_bench.py [--quick] [--legs NCE,SigLip] [--out profiles/contrastive_losses.txt]
(profiles/siglip_loss.txt is `--legs NCE,SigLip`, profiles/ntxent_loss.txt `--legs NCE,NTXent`.)"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(routes, rounds, iters):
    """routes: [(name, fn)] -> {name: (median, min, max)} over interleaved windows."""
    for _, fn in routes:
        for _ in range(3):
            fn()
    res = {n: [] for n, _ in routes}
    for _ in range(rounds):
        for n, fn in routes:
            res[n].append(window(fn, iters))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}


def fmt(t):
    return f"{t[0]:7.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"


# ---- the reference's statements (mml_loss.py) on embeddings ------------------------------------------------------------------------------
def torch_nce(f1, f2g, temperature, rank, alpha=None):
    N1 = f1.shape[0]
    logits = (f1 @ f2g.T) / torch.clamp(temperature, 0.001, 0.5)
    targets = torch.arange(N1 * rank, N1 * (rank + 1), device=f1.device)
    if alpha is None:
        return F.cross_entropy(logits, targets, reduction="none").mean()
    return (alpha * F.cross_entropy(logits, targets, reduction="none")
            + (1 - alpha) * F.cross_entropy(logits, targets.flip(0), reduction="none")).mean()


def torch_siglip(f1, f2g, temperature, bias, rank):
    N1, N2 = f1.shape[0], f2g.shape[0]
    s = f1 @ f2g.T
    y = torch.full_like(s, -1.0)
    y[torch.arange(N1, device=s.device), N1 * rank + torch.arange(N1, device=s.device)] = 1.0
    return -F.logsigmoid(y * (s / torch.clamp(temperature, 0.001, 0.5) + bias)).sum() / N1


def torch_ntxent(z, zg, temperature, rank):
    """SLIP's SIMCLRLoss on the stacked layout: z = cat([view a, view b]) of the local batch, zg the rank-major gathered stacks."""
    N1 = z.shape[0]
    B, W = N1 // 2, zg.shape[0] // N1
    tau = torch.clamp(temperature, 0.001, 0.5)
    qa, qb = z[:B], z[B:]
    g = zg.view(W, 2, B, -1)
    ka, kb = g[:, 0].reshape(W * B, -1), g[:, 1].reshape(W * B, -1)
    labels = rank * B + torch.arange(B, device=z.device)
    masks = F.one_hot(labels, W * B) * 1e9
    logits_aa, logits_bb = qa @ ka.T / tau - masks, qb @ kb.T / tau - masks
    logits_ab, logits_ba = qa @ kb.T / tau, qb @ ka.T / tau
    loss_a = F.cross_entropy(torch.cat([logits_ab, logits_aa], dim=1), labels)
    loss_b = F.cross_entropy(torch.cat([logits_ba, logits_bb], dim=1), labels)
    return (loss_a + loss_b) / 2


def torch_triplet(f1, f2g, rank, margin, reduce):
    N1 = f1.shape[0]
    scores = f1.mm(f2g.t())
    diagonal = scores[:, N1 * rank: N1 * (rank + 1)].diag().view(N1, 1)
    loss = (margin + scores - diagonal.expand_as(scores)).clamp(min=0)
    mask = torch.zeros_like(loss)
    mask[:, N1 * rank: N1 * (rank + 1)] += 1
    loss = loss.masked_fill_(mask.bool(), 0)
    loss = loss.sum(1) / (N1 - 1) if reduce == "mean" else loss.max(1)[0]
    return loss.sum()


def torch_triplet_local(f1, f2, margin, reduce):
    N1 = f1.shape[0]
    scores = f1.mm(f2.t())
    diagonal = scores.diag().view(N1, 1)
    mask = torch.eye(N1, device=scores.device) > 0.5
    l12 = (margin + scores - diagonal.expand_as(scores)).clamp(min=0).masked_fill_(mask, 0)
    l21 = (margin + scores - diagonal.t().expand_as(scores)).clamp(min=0).masked_fill_(mask, 0)
    l12, l21 = (l12.sum(1) / (N1 - 1), l21.sum(0) / (N1 - 1)) if reduce == "mean" else (l12.max(1)[0], l21.max(0)[0])
    return (l12 + l21).sum()


def section(a, N1, N2, P):
    from simseg_amd import heads
    g = torch.Generator(device="cuda").manual_seed(N2)
    rank = 1 if N2 > N1 else 0
    f1 = F.normalize(torch.randn(N1, P, device="cuda", generator=g), dim=-1).requires_grad_(True)
    f2g = F.normalize(torch.randn(N2, P, device="cuda", generator=g), dim=-1)
    with torch.no_grad():       # captions correlated with their images, as in a model under training
        f2g[rank * N1:(rank + 1) * N1] = F.normalize(f1 + 2.0 * f2g[rank * N1:(rank + 1) * N1], dim=-1)
    f2g.requires_grad_(True)
    temperature = torch.tensor(0.05, device="cuda", requires_grad=True)
    alpha = torch.rand(N1, device="cuda", generator=g)
    sig_t = torch.tensor(0.1, device="cuda", requires_grad=True)          # the SigLIP paper's init: t = 1 / T = 10, b = -10
    sig_b = torch.tensor(-10.0, device="cuda", requires_grad=True)
    margin, got = 0.2, {}
    # NTXent: the N1 rows are view a stacked on view b (b = a plus noise of twice its norm); one rank: the same tensor in both roles
    with torch.no_grad():
        va = F.normalize(torch.randn(N1 // 2, P, device="cuda", generator=g), dim=-1)
        vb = F.normalize(va + 2.0 * F.normalize(torch.randn(N1 // 2, P, device="cuda", generator=g), dim=-1), dim=-1)
    zs = torch.cat([va, vb]).requires_grad_(True)
    if N2 > N1:
        with torch.no_grad():
            zg = F.normalize(torch.randn(N2, P, device="cuda", generator=g), dim=-1)
            zg[rank * N1:(rank + 1) * N1] = zs
        zg.requires_grad_(True)
    else:
        zg = zs
    ntx_t = torch.tensor(0.1, device="cuda", requires_grad=True)

    def run(name, loss_fn):
        def fn():
            f1.grad = f2g.grad = temperature.grad = sig_t.grad = sig_b.grad = zs.grad = zg.grad = ntx_t.grad = None
            loss = loss_fn()
            loss.backward()
            got[name] = loss.detach()
        return fn

    legs = [
        ("NCE", lambda: heads.NCEFn.apply(f1, f2g, temperature, None, None, rank, 0.0)[0], lambda: torch_nce(f1, f2g, temperature, rank)),
        ("MixUpNCE", lambda: heads.MixNCEFn.apply(f1, f2g, temperature, alpha, None, None, rank, 0.0)[0],
         lambda: torch_nce(f1, f2g, temperature, rank, alpha)),
        ("Triplet-max", lambda: heads.TripletFn.apply(f1, f2g, rank, margin, 1)[0], lambda: torch_triplet(f1, f2g, rank, margin, "max")),
        ("Triplet-mean", lambda: heads.TripletFn.apply(f1, f2g, rank, margin, 0)[0], lambda: torch_triplet(f1, f2g, rank, margin, "mean")),
        ("SigLip", lambda: heads.SigLipFn.apply(f1, f2g, sig_t, sig_b, rank)[0], lambda: torch_siglip(f1, f2g, sig_t, sig_b, rank)),
        ("NTXent", lambda: heads.NTXentFn.apply(zs, zg, ntx_t, rank)[0], lambda: torch_ntxent(zs, zg, ntx_t, rank)),
    ]
    if N2 == N1:
        legs += [
            ("Triplet-max local", lambda: heads.TripletLocalFn.apply(f1, f2g, margin, 1)[0], lambda: torch_triplet_local(f1, f2g, margin, "max")),
            ("Triplet-mean local", lambda: heads.TripletLocalFn.apply(f1, f2g, margin, 0)[0], lambda: torch_triplet_local(f1, f2g, margin, "mean")),
        ]
    if a.legs:
        legs = [leg for leg in legs if leg[0].split()[0] in a.legs.split(",")]
    routes = []
    for name, hip, ref in legs:
        routes += [(name + "/hip", run(name + "/hip", hip)), (name + "/torch", run(name + "/torch", ref))]
    r = measure(routes, a.rounds, a.iters)
    torch.cuda.synchronize()
    say(f" sims [{N1}, {N2}], P = {P}, rank {rank} of {N2 // N1}")
    for name, _, _ in legs:
        h, t = r[name + "/hip"], r[name + "/torch"]
        say(f"  {name:19s} HIP {fmt(h)}   torch {fmt(t)}   torch / HIP = {t[0] / h[0]:5.2f}   "
            f"loss HIP {got[name + '/hip'].item():.6f}  torch {got[name + '/torch'].item():.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small blocks, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--legs", default=None, help="comma-separated subset of NCE,MixUpNCE,Triplet-max,Triplet-mean,SigLip,NTXent (default: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrastive_loss_bench.py measures on an MI355X; no GPU here")
    shapes, P = ([(512, 512), (512, 4096)], 512) if not a.quick else ([(8, 8), (8, 32)], 64)
    if a.quick:
        a.rounds, a.iters = 1, 2
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/contrastive_loss_bench.py{' --quick' if a.quick else ''}{' --legs ' + a.legs if a.legs else ''}   device: {pr.name}, torch {torch.__version__}")
    say(f"# loss head forward + backward from the embeddings (gradients w.r.t. both embedding matrices, the temperature for the NCE "
        f"legs and NTXent, temperature and bias for SigLip), fp32; ms per iteration: median [min .. max] over {a.rounds} windows of {a.iters} back-to-back iterations between two "
        "device events, routes interleaved round by round")
    say("# HIP = simseg_amd.heads (NCEFn / MixNCEFn / TripletFn / TripletLocalFn / SigLipFn / NTXentFn); torch = the reference's statements "
        "(mml_loss.py) in torch ops with autograd; SigLip, which the reference lacks: -F.logsigmoid(y * (s / T + b)).sum() / N1; NTXent, "
        "which it lacks too: SLIP's four logit blocks, -1e9 self mask, two cross-entropies, their mean")
    say()
    for N1, N2 in shapes:
        section(a, N1, N2, P)
        say()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
