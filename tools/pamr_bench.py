#!/usr/bin/env python
"""PAMR against the DenseCRF as the refinement stage of the zero-shot segmentation route (profiles/pamr.txt).  One process, one GPU.

  stage   segpost.pamr_masks against segpost.crf_masks on one 63-window batch of 512^2 images: low-resolution maps [63, 5, 32, 32]
          (scale 16), the candidate table of a synthetic ops.seg_select (171 classes, top 10: the visited slots per image are printed),
          de-normalised images = smooth colour fields plus noise.  The two take turns round by round; a round is `--reps` back-to-back
          calls between two device events; ms per batch: median [min .. max] over `--rounds` rounds, after 3 warm-up calls each.
          Peak memory: torch.cuda.max_memory_allocated across ONE call, the cached workspaces dropped first, minus the allocation before
          it - what the stage needs above the resident maps and images.
  route   segpost.evaluate_sharded over `--batches` batches of 63 windows (ViT-B/16 towers, random weights, 171 classes) with
          refiner = none (crf=False) / crf / pamr, in bf16 and fp32, pipelined and not: windows/s, median [min .. max] over `--rounds`
          runs after one warm-up run; the configurations of a mode take turns run by run.

No threshold is set: the report states what came out, a loss included.

    python tools/pamr_bench.py [--quick] [--skip-route] [--out profiles/pamr.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from topk_search_bench import LINES, say      # noqa: E402  (the same report helpers)

C, TOP, K = 171, 10, 5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def colour_fields(B, S, g):
    """[B, S, S, 3] uint8: smooth colour fields plus noise (8 distinct images, repeated), as bench.py makes them for the DenseCRF."""
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    base = torch.stack([(xx * 255 // S), (yy * 255 // S), ((xx + yy) * 127 // S)], -1).float()
    u8 = (base[None] + 20 * torch.randn(min(B, 8), S, S, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    return u8.repeat((B + 7) // 8, 1, 1, 1)[:B].contiguous()


def rounds_ms(fns, rounds, reps):
    """The callables take turns round by round -> per callable (median, min, max) ms per call."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            per[i].append(a.elapsed_time(b) / reps)
    return [(statistics.median(p), min(p), max(p)) for p in per]


def peak_delta(fn, drop):
    drop()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    del out
    return delta


def stage(a, B, S):
    from simseg_amd import ops, segpost
    g = torch.Generator().manual_seed(3)
    scores = torch.randn(B, C, generator=g).cuda()
    cand, _, _ = ops.seg_select(scores, TOP, K)
    lo = torch.rand(B, K, S // 16, S // 16, generator=g).cuda()
    u8 = colour_fields(B, S, g).cuda()
    visited = (cand >= 0).sum(1)
    say(f"## stage: one batch of {B} images of {S} x {S}, maps [{B}, {K}, {S // 16}, {S // 16}] at scale 16; visited slots per image: mean "
        f"{visited.float().mean().item():.2f}, min {int(visited.min())}, max {int(visited.max())} ({int(visited.sum())} maps in all)")

    def pamr():
        return segpost.pamr_masks(lo, cand, u8, scale=16)

    def crf():
        return segpost.crf_masks(lo, cand, u8, scale=16)

    def drop():
        ops._PAMR_WS.clear(); ops._CRF_WS.clear(); ops._CRF_SPATIAL.clear()

    for p in range(a.passes):
        (pm, pl, ph), (cm, cl, ch) = rounds_ms([pamr, crf], a.rounds, a.reps)
        say(f"pass {p + 1}:  pamr_masks {pm:8.3f} ms [{pl:.3f} .. {ph:.3f}]   crf_masks {cm:8.3f} ms [{cl:.3f} .. {ch:.3f}]   crf / pamr = {cm / pm:.2f}   "
            f"({a.rounds} rounds of {a.reps} calls each, alternating)")
    dil, iters = segpost.PAMR_PARAMS["dilations"], segpost.PAMR_PARAMS["iters"]
    px = B * S * S
    wbytes = 4 * 8 * len(dil) * px
    say(f"bytes the PAMR kernels must move per batch, from shapes: weights {wbytes / 1e9:.2f} GB written once and read {iters} times "
        f"= {wbytes * (iters + 1) / 1e9:.2f} GB (every image has a visited slot here)")
    pp, cp = peak_delta(pamr, drop), peak_delta(crf, drop)
    say(f"peak memory above the resident tensors, one call, workspace included:  pamr_masks {pp / 1e9:.3f} GB ({pp / px:.0f} B per pixel)   "
        f"crf_masks {cp / 1e9:.3f} GB ({cp / px:.0f} B per pixel)")
    drop()
    torch.cuda.empty_cache()
    say()


def route(a, B, S):
    from simseg_amd import segpost
    from slide_ragged_bench import build_model
    model = build_model()
    g = torch.Generator().manual_seed(5)
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=g), dim=-1).cuda()
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    x = ((colour_fields(B, S, g).permute(0, 3, 1, 2).float() / 255.0 - mean) / std).contiguous().cuda()
    lab = torch.randint(0, C, (B, S, S), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    mean, std = mean.cuda(), std.cuda()
    say(f"## route: segpost.evaluate_sharded, {a.batches} batches of {B} windows of {S} x {S} per run (ViT-B/16, {C} classes); windows/s: median "
        f"[min .. max] over {a.rounds} runs, one warm-up run, configurations alternating run by run")
    for mode in ("bf16", "fp32"):
        os.environ["SIMSEG_AMD_COMPUTE"] = mode
        sim_dt = torch.bfloat16 if mode == "bf16" else None
        confs = [(name, kw, pipe) for name, kw in (("none", dict(crf=False)), ("crf", dict(crf=True)), ("pamr", dict(crf=True, refiner="pamr")))
                 for pipe in (True, False)]

        def run(kw, pipe, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                segpost.evaluate_sharded(model, [(x, lab)] * n, text, TOP, mean=mean, std=std, sim_dtype=sim_dt, device="cuda", pipelined=pipe, **kw)
            torch.cuda.synchronize()
            return n * B / (time.perf_counter() - t0)

        for _, kw, pipe in confs:
            run(kw, pipe, 2)
        got = [[] for _ in confs]
        for _ in range(a.rounds):
            for i, (_, kw, pipe) in enumerate(confs):
                got[i].append(run(kw, pipe, a.batches))
        for (name, _, pipe), v in zip(confs, got):
            say(f"{mode}  refiner {name:<5} pipelined={str(pipe):<5}  {statistics.median(v):9.1f} windows/s [{min(v):.1f} .. {max(v):.1f}]")
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--skip-route", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pamr_bench.py measures on an MI355X; no GPU here")
    B, S = 63, 512
    if a.quick:
        B, a.rounds, a.reps, a.passes, a.batches = 4, 1, 1, 1, 2
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/pamr_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    say("# PAMR (simseg_pamr: dilations 1,2,4,8,12,24, 10 iterations) against the DenseCRF (simseg_dense_crf) in the same process")
    say()
    stage(a, B, S)
    if not a.skip_route:
        route(a, B, S)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
