#!/usr/bin/env python
"""One training step of the linear-probe task (configs/linear_prob/imagenet.yaml) at ViT-B/16, 224 x 224, 1000 classes, in its parts:

    (a) encoder forward          the frozen ViT under torch.no_grad() on the 16-bit path, to the [cls] feature
    (b) head, HIP                simseg_amd.probe.ProbeHeadFn forward + backward on those features: fp32 logits GEMM with the bias epilogue,
                                 the fused cross-entropy / top-1 / top-5 / logit-gradient rows, dW and db
    (c) LARS step, HIP           simseg_amd.optim.LARS.step() on classifier.weight / bias: three launches, no host read
    (d) head, torch ops          F.linear + F.cross_entropy + topk(5) accuracy + backward on the SAME features (fp32)
    (e) LARS step, torch ops     a per-tensor loop with the two norms read on the host, as the reference's optimizer does

All in one process on one GPU, interleaved round by round; every window is `--iters` back-to-back iterations between two device events
(host time to enqueue one iteration printed beside it: (e) waits for the device twice per tensor, so its host time IS its time).  Median
[min .. max] over `--rounds` windows.

    python tools/linear_probe_bench.py [--batch 256] [--quick] [--out profiles/linear_probe.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


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


@torch.no_grad()
def torch_lars_step(params, bufs, lr, momentum=0.9, weight_decay=0.0, eta=0.001, eps=1e-8):
    for i, p in enumerate(params):
        wn, gn = torch.norm(p).item(), torch.norm(p.grad).item()
        local = eta * wn / (gn + weight_decay * wn + eps) if wn != 0 and gn != 0 else 1.0
        d = p.grad.add(p, alpha=weight_decay).mul(local * lr)
        if bufs[i] is None:
            bufs[i] = d.clone()
        else:
            bufs[i].mul_(momentum).add_(d)
        p.sub_(bufs[i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--quick", action="store_true", help="the tiny test ViT at 96 x 96, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_probe_bench.py measures on an MI355X; no GPU here")
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.linear_prob.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    from simseg_amd.optim import LARS
    from simseg_amd.probe import ProbeHeadFn
    argv = []
    if a.quick:
        a.rounds, a.iters, a.batch = 1, 3, min(a.batch, 16)
        argv = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128"]
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/linear_prob/imagenet.yaml"), argv, update_clip_config)
    torch.manual_seed(0)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE).cuda().train()
    S, C, B = cfg.transforms.input_size, cfg.model.classifier.num_classes, a.batch
    gen = torch.Generator(device="cuda").manual_seed(0)
    image = torch.randn(B, 3, S, S, device="cuda", generator=gen)
    label = torch.randint(0, C, (B,), device="cuda", generator=gen)
    feats = model.forward_image_feature(image)
    x32 = feats.float().contiguous()
    w, b = model.classifier.weight, model.classifier.bias
    wt = [torch.nn.Parameter(w.detach().clone()), torch.nn.Parameter(b.detach().clone())]        # the torch routes' own copies
    opt = LARS([{"params": [w]}, {"params": [b]}], lr=cfg.optim.lr.init, momentum=0.9, weight_decay=0.0)
    bufs = [None, None]
    acc = {}

    def encoder():
        model.forward_image_feature(image)

    def head_hip():
        w.grad = b.grad = None
        loss, out3, _ = ProbeHeadFn.apply(feats, w, b, label)
        loss.backward()
        acc["hip"] = out3

    def lars_hip():
        opt.step()

    def head_torch():
        wt[0].grad = wt[1].grad = None
        logits = F.linear(x32, wt[0], wt[1])
        loss = F.cross_entropy(logits, label)
        top = logits.detach().topk(5, dim=1).indices == label[:, None]
        acc["torch"] = torch.stack([loss.detach(), top[:, :1].sum().float(), top.sum().float()])
        loss.backward()

    def lars_torch():
        torch_lars_step(wt, bufs, cfg.optim.lr.init)

    routes = [("(a) encoder forward", encoder), ("(b) head, HIP: fwd + loss + bwd", head_hip), ("(c) LARS step, HIP", lars_hip),
              ("(d) head, torch ops: fwd + loss + bwd", head_torch), ("(e) LARS step, torch per-tensor loop", lars_torch)]
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/linear_probe_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    enc = str(model.amp_dtype if cfg.dist.fp16 else torch.float32).replace("torch.", "")
    say(f"# {cfg.model.image_encoder.tag} at {S} x {S}, batch {B}, {C} classes, feature dim {x32.shape[1]}; encoder compute type {enc} "
        f"(features delivered as {str(feats.dtype).replace('torch.', '')}), head fp32")
    say(f"# ms per iteration: median [min .. max] over {a.rounds} windows of {a.iters} back-to-back iterations between two device events, "
        "routes interleaved round by round; 'host' = time to enqueue one iteration")
    say()
    for _, fn in routes:                            # warm-up: launch plans, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    h, t = acc["hip"].tolist(), acc["torch"].tolist()
    say(f"check: HIP head loss {h[0]:.6f}, top-1 {int(h[1])}, top-5 {int(h[2])};  torch head loss {t[0]:.6f}, top-1 {int(t[1])}, top-5 {int(t[2])}")
    res = {name: [] for name, _ in routes}
    for _ in range(a.rounds):
        for name, fn in routes:
            res[name].append(window(fn, a.iters))
    med = {}
    for name, _ in routes:
        dev = [d for d, _ in res[name]]
        host = [hh for _, hh in res[name]]
        med[name] = statistics.median(dev)
        say(f"{name:40s} {med[name]:8.3f} ms [{min(dev):.3f} .. {max(dev):.3f}]   host {statistics.median(host):.3f} ms [{min(host):.3f} .. {max(host):.3f}]")
    names = [n for n, _ in routes]
    say()
    say(f"head: HIP {med[names[1]]:.3f} ms vs torch ops {med[names[3]]:.3f} ms;  LARS: HIP {med[names[2]]:.3f} ms vs torch loop {med[names[4]]:.3f} ms;  "
        f"head + LARS = {100 * (med[names[1]] + med[names[2]]) / (med[names[0]] + med[names[1]] + med[names[2]]):.1f} % of the HIP step")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
