#!/usr/bin/env python
"""Mixup / CutMix on the device and the two-label soft-target head, against the same recipe in torch ops:

    (a) ops.mix_batch (one launch, in place) against the torch statement - `x * lam + x.flip(0) * (1 - lam)` for mixup, the box assignment
        from a flipped copy `x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]` for cutmix, and for an elem-mode table (half the rows
        mixup, half cutmix, every row its own lam / box) per-row lam and box-mask tensors through torch.where - on fp32 and bf16 batches of
        B x 3 x 224 x 224, B = 256 and 2048
    (b) the soft-target head, simseg_amd.probe.SoftProbeHeadFn forward + loss + backward (labels, partner labels, lam, smoothing; no dense
        target), against F.linear + the dense [B, C] timm target + log_softmax + product + row sum + top-5 accuracy + backward on the SAME
        features, C = 1000, feature dim 768, B = 256 and 2048, with torch.cuda.max_memory_allocated above the resident tensors for both

All in one process on one GPU, routes interleaved round by round; every window is `--iters` back-to-back iterations between two device
events.  Median [min .. max] over `--rounds` windows.  `--test-log` appends the error / gate lines that `pytest -s tests/test_gpu_mixup.py`
printed (the test table of profiles/mixup.txt).

    python tools/mixup_bench.py [--quick] [--test-log pytest_output.txt] [--out profiles/mixup.txt]"""
import argparse
import os
import re
import statistics
import sys

import numpy as np
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
        for _ in range(2):
            fn()
    res = {n: [] for n, _ in routes}
    for _ in range(rounds):
        for n, fn in routes:
            res[n].append(window(fn, iters))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}


def fmt(t):
    return f"{t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"


def mix_section(a, B, S, dtype):
    from simseg_amd import ops
    from simseg_amd.mixup import explicit_params
    rng = np.random.default_rng(B)
    x = torch.randn(B, 3, S, S, device="cuda").to(dtype)
    n_bytes = x.numel() * x.element_size()
    q = S // 4
    box = (q, 3 * q, q // 2, q // 2 + 2 * q)                              # a quarter of the image: lam = 0.75
    tables = {"mixup, one lam": explicit_params([1] * B, [0.3] * B), "cutmix, one box (1/4 of the image)": explicit_params([2] * B, [0.75] * B, [box] * B)}
    kinds = [1 if i % 2 == 0 else 2 for i in range(B)]                    # (B even: a mixup row's partner is a cutmix row)
    lams = rng.beta(0.8, 0.8, B)
    boxes = []
    for _ in range(B):
        h, w = int(rng.integers(S // 8, S // 2 + 1)), int(rng.integers(S // 8, S // 2 + 1))
        y, xx = int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1))
        boxes.append((y, y + h, xx, xx + w))
    tables["elem, half mixup / half cutmix"] = explicit_params(kinds, lams, boxes)
    for name, p in tables.items():
        tab = torch.from_numpy(p["table"]).cuda()
        kind = torch.from_numpy(p["table"][:, 0].astype(np.int64)).cuda()
        lam_t = torch.from_numpy(p["lam"]).cuda().to(dtype).view(B, 1, 1, 1)
        yy, xc = torch.arange(S, device="cuda").view(1, 1, S, 1), torch.arange(S, device="cuda").view(1, 1, 1, S)
        t = torch.from_numpy(p["table"].astype(np.int64)).cuda()
        mask = (yy >= t[:, 1].view(B, 1, 1, 1)) & (yy < t[:, 2].view(B, 1, 1, 1)) & (xc >= t[:, 3].view(B, 1, 1, 1)) & (xc < t[:, 4].view(B, 1, 1, 1))
        is_cut = (kind == 2).view(B, 1, 1, 1)
        yl, yh, xl, xh = (int(v) for v in p["table"][0, 1:5])
        lam0 = float(p["lam"][0])
        keep = {}

        def hip():
            ops.mix_batch(x, tab, p["table"])

        def torch_mixup():
            keep["y"] = x * lam0 + x.flip(0) * (1 - lam0)

        def torch_cutmix():
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]

        def torch_elem():
            xf = x.flip(0)
            keep["y"] = torch.where(is_cut, torch.where(mask, xf, x), x * lam_t + xf * (1 - lam_t))

        ref = torch_mixup if name.startswith("mixup") else torch_cutmix if name.startswith("cutmix") else torch_elem
        r = measure([("hip", hip), ("torch", ref)], a.rounds, a.iters)
        moved = 2 * n_bytes if not name.startswith("cutmix") else 2 * n_bytes * (yh - yl) * (xh - xl) // (S * S)
        say(f"  {name:36s} HIP {fmt(r['hip'])} ({moved / r['hip'][0] / 1e6:7.0f} GB/s of the bytes that must move)   torch {fmt(r['torch'])}   "
            f"torch / HIP = {r['torch'][0] / r['hip'][0]:.2f}")
        x.copy_(torch.randn(B, 3, S, S, device="cuda").to(dtype))        # (repeated blends drift towards the mean: fresh values per table)
    del x
    torch.cuda.empty_cache()


def head_section(a, B, C, D):
    from simseg_amd.probe import SoftProbeHeadFn
    g = torch.Generator(device="cuda").manual_seed(B)
    feats = torch.randn(B, D, device="cuda", generator=g)
    w = torch.nn.Parameter(torch.randn(C, D, device="cuda", generator=g) * 0.02)
    b = torch.nn.Parameter(torch.zeros(C, device="cuda"))
    ya = torch.randint(0, C, (B,), device="cuda", generator=g)
    yb = ya.flip(0)
    lam = torch.rand(B, device="cuda", generator=g)
    eps = 0.1
    acc = {}

    def hip():
        w.grad = b.grad = None
        loss, out3, _ = SoftProbeHeadFn.apply(feats, w, b, ya, yb, lam, eps)
        loss.backward()
        acc["hip"] = out3

    def dense():
        w.grad = b.grad = None
        off = eps / C
        y1 = torch.full((B, C), off, device="cuda").scatter_(1, ya[:, None], 1.0 - eps + off)
        y2 = torch.full((B, C), off, device="cuda").scatter_(1, yb[:, None], 1.0 - eps + off)
        t = y1 * lam[:, None] + y2 * (1.0 - lam[:, None])
        logits = F.linear(feats, w, b)
        loss = torch.sum(-t * F.log_softmax(logits, dim=-1), dim=-1).mean()
        top = logits.detach().topk(5, dim=1).indices == ya[:, None]
        acc["torch"] = torch.stack([loss.detach(), top[:, :1].sum().float(), top.sum().float()])
        loss.backward()

    peak = {}
    for name, fn in (("hip", hip), ("torch", dense)):
        fn()
        w.grad = b.grad = None
        acc.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    hip()
    dense()
    torch.cuda.synchronize()
    h, t = acc["hip"].tolist(), acc["torch"].tolist()
    r = measure([("hip", hip), ("torch", dense)], a.rounds, a.iters)
    say(f"  B={B:5d}  soft head, HIP {fmt(r['hip'])}  peak +{peak['hip']:7.1f} MiB   dense-target torch head {fmt(r['torch'])}  peak +{peak['torch']:7.1f} MiB   "
        f"torch / HIP = {r['torch'][0] / r['hip'][0]:.2f}")
    say(f"           check: HIP loss {h[0]:.6f}, top-1 {int(h[1])}, top-5 {int(h[2])};  torch loss {t[0]:.6f}, top-1 {int(t[1])}, top-5 {int(t[2])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small batches, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--test-log", default=None, help="output of `pytest -s tests/test_gpu_mixup.py`: its error / gate lines are appended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixup_bench.py measures on an MI355X; no GPU here")
    batches, S = ([256, 2048], 224) if not a.quick else ([8], 64)
    if a.quick:
        a.rounds, a.iters = 1, 2
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/mixup_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    say(f"# ms per iteration: median [min .. max] over {a.rounds} windows of {a.iters} back-to-back iterations between two device events, "
        "routes interleaved round by round")
    say()
    say(f"(a) mix_batch, in place, one launch, against the torch statement; batches of B x 3 x {S} x {S}")
    for dtype in (torch.float32, torch.bfloat16):
        for B in batches:
            say(f" {str(dtype).replace('torch.', '')}, B = {B}")
            mix_section(a, B, S, dtype)
    say()
    say("(b) soft-target head forward + loss + backward (fp32, 1000 classes, feature dim 768), peak memory above the resident tensors")
    for B in batches:
        head_section(a, B, 1000, 768)
    if a.test_log:
        say()
        say("(c) tests/test_gpu_mixup.py: error against float64 beside torch's own fp32 deviation and the 4 x gate (pooled over the cases)")
        pat = re.compile(r"^(torch fp32 dense-target|B=\d+ C=\d+ |C=\d+ (loss|dx|dW|db):|mixed batch vs)")
        for line in open(a.test_log):
            line = line.strip()
            m = pat.search(line.lstrip(".FEsx"))
            if m:
                say("  " + line.lstrip(".FEsx"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
