#!/usr/bin/env python
"""Fused top-K search (ops.topk_search, csrc/search.hip) against the routes the tree offered for the same answer, one process, one GPU:
    materialise + topk : the score matrix in fp32 (heads._similarity_matrix for fp32 operands, the bf16 MFMA GEMM with fp32 output for
                         bf16 operands) followed by torch.topk(k, sorted=True)
    full argsort       : EmbANN._ann - fp32 GEMM, stable argsort of every row, int64 id gather (fp32 operands, K = 10 legs only)
Legs: 5000 x 25000 x 512 in both directions at K = 10, the same at K = 128, one query against 1 M rows, 512 images against 1000 classes;
fp32 and bf16 operands.  Every route is warmed up, then timed over `--rounds` windows of back-to-back calls ending in a device synchronise
(each window at least `--window` seconds of work); median and range of the per-call time over the windows are printed, with the shader
clock and package power sampled during the fused route's windows (bench.ClockSampler).  Peak-memory deltas are
torch.cuda.max_memory_allocated across ONE call minus the allocation before it (operands excluded, outputs included).

    python tools/topk_search_bench.py [--quick] [--resources FILE] [--out profiles/topk_search.txt]
--resources: text of `python tools/kernel_resources.py simseg_amd/build/search.o topk`, quoted at the end of the report (the objects
are not where the benchmark runs)."""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def unit_rows(rows, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, D, device="cuda", generator=g)
    return x / x.norm(dim=1, keepdim=True)


def timed(fn, rounds, window):
    """-> (median ms per call, min, max, calls per window)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-5)
    reps = max(3, min(2000, int(window / one) + 1))
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / reps * 1e3)
    return statistics.median(per), min(per), max(per), reps


def peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    del out
    return delta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_search_bench.py measures on an MI355X; no GPU here")
    import bench
    from simseg.tasks.clip.hooks.utils import EmbANN, IndexedEmbInfo
    from simseg_amd import heads, ops

    F32, BF16 = torch.float32, torch.bfloat16
    legs = [("image -> text", 5000, 25000, 512, 10, True), ("text -> image", 25000, 5000, 512, 10, True),
            ("image -> text, wide K", 5000, 25000, 512, 128, False), ("one query, 1 M rows", 1, 1000000, 512, 10, False),
            ("512 images x 1000 classes", 512, 1000, 512, 5, False)]
    if a.quick:
        legs = [(n, max(1, M // 50), max(200, N // 50), D, K, ann) for n, M, N, D, K, ann in legs]
        a.rounds, a.window = 1, 0.02
    pr = torch.cuda.get_device_properties(0)
    bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
    say(f"# tools/topk_search_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    say(f"# ms per call: median [min .. max] over {a.rounds} windows of back-to-back calls (>= {a.window} s each, synchronised at the end); 3 warm-up calls per route")
    say("# peak: torch.cuda.max_memory_allocated across one call minus the allocation before it")
    say()
    for name, M, N, D, K, with_ann in legs:
        q32, g32 = unit_rows(M, D, 1), unit_rows(N, D, 2)
        say(f"## {name}: {M} x {N} x {D}, K = {K}   (score matrix: {M * N * 4 / 1e6:.1f} MB in fp32)")
        for dtype, label in ((F32, "fp32"), (BF16, "bf16")):
            q, g = (q32, g32) if dtype == F32 else (ops.cast(q32, BF16), ops.cast(g32, BF16))
            fused = lambda: ops.topk_search(q, g, K)                                   # noqa: E731
            if dtype == F32:
                mat = lambda: torch.topk(heads._similarity_matrix(q, g), min(K, N), dim=1, sorted=True)      # noqa: E731
            else:
                mat = lambda: torch.topk(ops.gemm(q, g, out_dtype=F32), min(K, N), dim=1, sorted=True)       # noqa: E731
            clocks = bench.ClockSampler(period=0.05, bdf=bdf)
            for _ in range(3):
                fused()
            torch.cuda.synchronize()
            clocks.mark()
            f_ms = timed(fused, a.rounds, a.window)
            c = clocks.stop() or {}
            m_ms = timed(mat, a.rounds, a.window)
            f_pk, m_pk = peak_delta(fused), peak_delta(mat)
            fs, fi = fused()
            ms_, mi = mat()
            same = (fi[:, :mi.shape[1]].long() == mi).all(dim=1).float().mean().item()
            worst = (fs[:, :mi.shape[1]] - ms_).abs().max().item()
            say(f"{label}  fused search        {f_ms[0]:9.3f} ms [{f_ms[1]:.3f} .. {f_ms[2]:.3f}] x{f_ms[3]:<5d} peak {f_pk / 1e6:9.2f} MB   "
                f"sclk {c.get('sclk_mhz_avg')} MHz, {c.get('power_w_avg')} W ({c.get('source')})")
            say(f"{label}  materialise + topk  {m_ms[0]:9.3f} ms [{m_ms[1]:.3f} .. {m_ms[2]:.3f}] x{m_ms[3]:<5d} peak {m_pk / 1e6:9.2f} MB   "
                f"fused / this = {f_ms[0] / m_ms[0]:.2f}x time;  rows with identical index lists {same * 100:.2f} %, max |score diff| {worst:.2e}")
            if with_ann and dtype == F32:
                left = IndexedEmbInfo("l", torch.arange(M, device="cuda"), q)
                right = IndexedEmbInfo("r", torch.arange(N, device="cuda"), g)
                ann = lambda: EmbANN()._ann(left, right)                               # noqa: E731
                a_ms = timed(ann, max(1, min(a.rounds, 3)), a.window)
                a_pk = peak_delta(ann)
                say(f"{label}  full argsort (_ann) {a_ms[0]:9.3f} ms [{a_ms[1]:.3f} .. {a_ms[2]:.3f}] x{a_ms[3]:<5d} peak {a_pk / 1e6:9.2f} MB   "
                    f"fused / this = {f_ms[0] / a_ms[0]:.3f}x time")
            del q, g
        del q32, g32
        torch.cuda.empty_cache()
        say()
    if a.resources and os.path.exists(a.resources):
        say("## kernel resources (tools/kernel_resources.py simseg_amd/build/search.o topk)")
        for ln in open(a.resources).read().rstrip().splitlines():
            say(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
