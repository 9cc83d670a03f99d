#!/usr/bin/env python
"""Weighted k-NN evaluation: the fused route (retrieval.search at K = max(ks) + ops.knn_vote, simseg_amd/knn.py) against the torch
route a user would write for the same answer, on the same tensors, the routes taking turns leg by leg in one process on one GPU:
    torch route : query chunks sized so that the chunk x N fp32 score matrix stays within --budget-gib, and per chunk
                  matmul -> torch.topk(K) -> label gather -> per k: exp((s - s_0) / T), scatter_add_ into [chunk, C], topk(5)
Synthetic unit rows: a bank of N x 768 (--bank, default 1,281,167 and 100,000) held in fp32 and in bf16, C = 1000 classes, a batch of
4,096 queries, ks = (10, 20, 100), T = 0.07.  Every route is warmed up, then timed over `--rounds` windows of back-to-back calls ending in
a device synchronise; median and range of the time per 4,096 queries are printed.  Peak memory is torch.cuda.max_memory_allocated
across ONE call minus the allocation before it: what the route needs above the resident bank, labels and queries.  The share of rows on
which the two routes name the same top-1 class at every k is printed as a cross-check (near-ties and, for bf16, different product
rounding may differ).  No threshold is set: the report states what came out.

    python tools/knn_bench.py [--quick] [--bank N [N ...]] [--out profiles/knn.txt]"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from topk_search_bench import LINES, peak_delta, say, timed, unit_rows      # noqa: E402  (the same timing helpers)

KS, T, C, D, BATCH = (10, 20, 100), 0.07, 1000, 768, 4096


def torch_route(q, bank, labels, chunk):
    """-> top-1 class per k [len(KS), M] (int64).  q in the bank's dtype; the score matrix is formed per query chunk."""
    out = []
    for lo in range(0, q.shape[0], chunk):
        sim = (q[lo:lo + chunk] @ bank.T).float()
        s, i = torch.topk(sim, KS[-1], dim=1, sorted=True)
        del sim
        lab = labels[i]
        w = torch.exp((s - s[:, :1]) / T)
        tops = []
        for k in KS:
            votes = torch.zeros(s.shape[0], C, device=q.device, dtype=torch.float32)
            votes.scatter_add_(1, lab[:, :k], w[:, :k])
            tops.append(votes.topk(5, dim=1).indices[:, 0])
        out.append(torch.stack(tops))
    return torch.cat(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small bank, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--bank", type=int, nargs="+", default=[1281167, 100000])
    ap.add_argument("--budget-gib", type=float, default=4.0, help="largest fp32 score matrix the torch route may form")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench.py measures on an MI355X; no GPU here")
    from simseg_amd import ops, retrieval

    batch = BATCH
    if a.quick:
        a.bank, a.rounds, a.window, batch = [20000], 1, 0.02, 512
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/knn_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    say(f"# {batch} unit queries x bank N x {D}, C = {C}, ks = {KS}, T = {T}; ms per batch: median [min .. max] over {a.rounds} windows of "
        f"back-to-back calls (>= {a.window} s each, synchronised at the end); 3 warm-up calls per route")
    say(f"# torch route: query chunks whose chunk x N fp32 score matrix stays within {a.budget_gib} GiB")
    say("# peak: torch.cuda.max_memory_allocated across one call minus the allocation before it (bank, labels and queries resident)")
    say("# bf16: torch's matmul returns the scores rounded to bf16 and the top-k ranks those; the fused search ranks its fp32 accumulators, so the "
        "two routes rank different numbers (random unit rows in 768 dimensions score within a few bf16 ulps of each other) and the top-1 "
        "agreement is below 100 %")
    say()
    for N in a.bank:
        bank32, q32 = unit_rows(N, D, 2), unit_rows(batch, D, 1)
        labels = torch.randint(0, C, (N,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        labels32 = labels.int()
        chunk = max(1, min(batch, int(a.budget_gib * 2 ** 30 / (4 * N))))
        say(f"## bank {N} x {D}   (full score matrix of the batch: {batch * N * 4 / 1e9:.2f} GB in fp32; torch route: chunks of {chunk} queries)")
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            bank, q = (bank32, q32) if dtype == torch.float32 else (ops.cast(bank32, dtype), ops.cast(q32, dtype))

            def fused():
                score, index = retrieval.search(q, bank, KS[-1], compute_dtype=dtype)
                return ops.knn_vote(score, index, labels32, KS, T)[0]

            def search_only():
                return ops.topk_search(q, bank, KS[-1])

            def vote_only(lists=search_only()):
                return ops.knn_vote(lists[0], lists[1], labels32, KS, T)[0]

            def plain():
                return torch_route(q, bank, labels, chunk)

            f_ms, t_ms = timed(fused, a.rounds, a.window), timed(plain, a.rounds, a.window)
            s_ms, v_ms = timed(search_only, a.rounds, a.window), timed(vote_only, a.rounds, a.window)
            f_pk, t_pk = peak_delta(fused), peak_delta(plain)
            same = (fused()[:, :, 0].long() == plain()).all(dim=0).float().mean().item()
            say(f"{name}  fused search + vote {f_ms[0]:9.3f} ms [{f_ms[1]:.3f} .. {f_ms[2]:.3f}] x{f_ms[3]:<5d} peak {f_pk / 1e6:9.2f} MB   "
                f"(search alone {s_ms[0]:.3f} ms, vote alone {v_ms[0]:.3f} ms)")
            say(f"{name}  torch route         {t_ms[0]:9.3f} ms [{t_ms[1]:.3f} .. {t_ms[2]:.3f}] x{t_ms[3]:<5d} peak {t_pk / 1e6:9.2f} MB   "
                f"fused / this = {f_ms[0] / t_ms[0]:.2f}x time, {f_pk / max(t_pk, 1):.4f}x peak;  rows with the same top-1 at every k {same * 100:.2f} %")
            del bank, q
        del bank32, q32, labels, labels32
        torch.cuda.empty_cache()
        say()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
