#!/usr/bin/env python
"""Global-norm gradient clipping in front of the one-launch AdamW step, at the parameter shapes of ViT-B/16 + BERT-base (about 195 M fp32
gradients in ~400 tensors, one param group per tensor as the reference's ClipOptimizerHook builds them; synthetic gradients, no towers):

    (a) step()                                  optimizer.step() alone
    (b) fused clip + step()                     AdamW.clip_grad_norm_ (one read-only norm pass, one finish) + the clipped update kernel
    (c) torch clip_grad_norm_ + step()          torch.nn.utils.clip_grad_norm_ over the gradient tensors, then the plain update kernel

All three in one process on one GPU, interleaved round by round; every window is `--iters` back-to-back iterations between two device events
(the host runs ahead, so a window measures device time unless the host is the bottleneck - the host-side time per iteration is printed
next to it).  Median [min .. max] over `--rounds` windows.  The byte model says (b) - (a) is one read of every gradient; the numbers
say what it is.

    python tools/grad_clip_bench.py [--quick] [--out profiles/grad_clip.txt]"""
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


def shapes(quick=False):
    D, L, F = (768, 12, 3072) if not quick else (64, 2, 256)
    vocab, T = (30522, 197) if not quick else (1000, 17)
    out = [(D, 3, 16, 16), (D,), (1, 1, D), (1, T, D)]                                       # ViT: patch embedding, cls token, positions
    for _ in range(L):
        out += [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (F, D), (F,), (D, F), (D,)]
    out += [(D,), (D,)]
    out += [(vocab, D), (512, D), (2, D), (D,), (D,)]                                        # BERT embeddings + LayerNorm
    for _ in range(L):
        out += [(D, D), (D,)] * 4 + [(D,), (D,), (F, D), (F,), (D, F), (D,), (D,), (D,)]
    out += [(D, D), (D,)]                                                                    # pooler
    out += [(512, D), (512,), (512, D), (512,), ()]                                          # the two projections, the temperature
    return out


def window(fn, iters):
    """-> (device ms per iteration between two events, host ms per iteration to enqueue them)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / iters * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench.py measures on an MI355X; no GPU here")
    from simseg_amd.optim import AdamW
    if a.quick:
        a.rounds, a.iters = 1, 3
    gen = torch.Generator(device="cuda").manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.02) for s in shapes(a.quick)]
    grads = [torch.randn(p.shape, device="cuda", generator=gen) * 1e-3 for p in params]
    for p, g in zip(params, grads):
        p.grad = g
    n = sum(p.numel() for p in params)
    opt = AdamW([{"params": [p]} for p in params], lr=1e-6, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)
    true = float(torch.linalg.vector_norm(torch.cat([g.double().view(-1) for g in grads])))
    max_norm = 0.5 * true

    def plain():
        opt.step()

    def fused():
        opt.clip_grad_norm_(max_norm)
        opt.step()

    def via_torch():                                # (scales the gradients in place: from its second call on the coefficient is ~1, the work the same)
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()

    routes = [("(a) step() alone", plain), ("(b) fused clip + step()", fused), ("(c) torch clip_grad_norm_ + step()", via_torch)]
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/grad_clip_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    say(f"# {len(params)} tensors, {n / 1e6:.1f} M fp32 gradients ({4 * n / 1e6:.0f} MB), one param group per tensor; max_norm = 0.5 x the norm "
        f"({true:.4f})")
    say(f"# ms per iteration: median [min .. max] over {a.rounds} windows of {a.iters} back-to-back iterations between two device events, "
        "routes interleaved round by round; 'host' = time to enqueue one iteration")
    say()
    got = float(opt.grad_norm())
    say(f"norm check: fused pass {got:.6f} vs float64 {true:.6f} (relative error {abs(got - true) / true:.2e})")
    for _, fn in routes:                            # warm-up: launch plans, code objects, torch's foreach paths
        for _ in range(3):
            fn()
    res = {name: [] for name, _ in routes}
    for _ in range(a.rounds):
        for name, fn in routes:
            res[name].append(window(fn, a.iters))
    med = {}
    for name, _ in routes:
        dev = [d for d, _ in res[name]]
        host = [h for _, h in res[name]]
        med[name] = statistics.median(dev)
        say(f"{name:38s} {med[name]:8.3f} ms [{min(dev):.3f} .. {max(dev):.3f}]   host {statistics.median(host):.3f} ms [{min(host):.3f} .. {max(host):.3f}]")
    (na, _), (nb, _), (nc, _) = routes
    say()
    say(f"(b) - (a) = {med[nb] - med[na]:.3f} ms: the norm pass and the finish ({4 * n / 1e6:.0f} MB read once: "
        f"{4 * n / max(med[nb] - med[na], 1e-9) / 1e9:.2f} TB/s if that is all it is)")
    say(f"(c) - (a) = {med[nc] - med[na]:.3f} ms: torch's norms and in-place scaling of {len(params)} tensors; (b) / (c) = {med[nb] / med[nc]:.2f}x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
