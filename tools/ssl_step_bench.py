#!/usr/bin/env python
"""What the image self-supervision branch (CLIPModel.enable_ssl: SLIP's NT-Xent on two views through the same image tower) costs on the
training step, measured: ViT-B/16 + BERT-base, 256 pairs at 224^2 and L = 77 in bf16, built with bench.py's own model and batch builders,
branch off (the batch has no "image_ssl") and on (the tower runs on 3 x 256 images) in ONE process, the two interleaved round by round:

    (a) the training step (forward, losses, backward, AdamW; two tower streams) and torch.cuda.max_memory_allocated over one step
    (b) the image tower alone, forward + backward, on 256 and on 768 images
    (c) the branch's own pieces, forward + backward: the projection-head node with its L2 norm on the 512 [cls] rows, and the loss
        (heads.NTXentFn through LOSS.NTXent) on the 512 embeddings
    (d) the slice and cat plumbing: cat([image, view 1, view 2]) forward, and the backward of feats[:B] and feats[B:, 0] - autograd's
        zero-filled scatters and their sum - on the tower's [3B, 197, 768] output

Each leg has its own AdamW (the off leg's over the model's parameters without the head's), so neither re-plans its tensor tables when the
legs alternate.  Every window is `--iters` back-to-back iterations between two device events on the main stream (which waits for the side
stream first); median [min .. max] over `--rounds` windows after warm-up.

    python tools/ssl_step_bench.py [--quick] [--out profiles/ssl_branch.txt]"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def window(fn, iters, side=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(routes, rounds, iters, side=None, warm=2):
    """routes: [(name, fn)] -> {name: (median, min, max)} over interleaved windows."""
    for _, fn in routes:
        for _ in range(warm):
            fn()
    res = {n: [] for n, _ in routes}
    for _ in range(rounds):
        for n, fn in routes:
            res[n].append(window(fn, iters, side))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the tiny test ViT at 96^2, 8 pairs, one round (a rehearsal of the script, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssl_step_bench.py measures on an MI355X; no GPU here")
    import bench
    from simseg.models import PIPELINE
    from simseg.models.components import L2norm
    from simseg.models.pipelines.clip import _side_stream
    from simseg.utils import logger
    from simseg_amd.nn import VIT_ARCH, ViT
    from simseg_amd.optim import AdamW
    logger.STREAM = sys.stderr
    os.environ["SIMSEG_AMD_COMPUTE"] = "bf16"
    adt = torch.bfloat16
    dev = torch.device("cuda", 0)
    tag, img, B, L, hidden, out_dim = ("vit_base_patch16_224_in21k", 224, 256, 77, 4096, 256) if not a.quick else ("vit_test_patch16", 96, 8, 25, 192, 64)
    if a.quick:
        a.rounds, a.iters = 1, 2
    dim = VIT_ARCH[tag]["dim"]
    cfg, build = bench.build_model(tag, dim, img)
    torch.manual_seed(1234)
    model = build(cfg.model.name, cfg, PIPELINE).to(dev).train()
    base_params = list(model.parameters())
    model.enable_ssl(scale=1.0, hidden_dim=hidden, out_dim=out_dim, temperature=0.1)
    (vit,) = [m for m in model.modules() if isinstance(m, ViT)]
    side = _side_stream(dev)
    text = list(model.text_encoder.parameters()) + list(model.text_projection.parameters())
    opts = {}
    for leg, params in (("off", base_params), ("on", list(model.parameters()))):
        opts[leg] = AdamW(params, lr=1e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=1e-3, half_dtype=adt)
        opts[leg].set_param_streams({p: side for p in text})
    batch = bench.synthetic_batch(B, img, L, 30522, 1000, dev)
    g = torch.Generator(device="cuda").manual_seed(5)
    views = torch.stack([batch["image"].flip(-1), batch["image"] + 0.1 * torch.randn(batch["image"].shape, device=dev, generator=g)])
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/ssl_step_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    say(f"# {tag} + {cfg.model.text_encoder.tag}, {B} pairs at {img}^2, L = {L}, bf16 compute, AdamW; branch: Linear({dim}, {hidden}) -> GELU -> "
        f"Linear({hidden}, {out_dim}), NT-Xent at T = 0.1, scale 1; one process, legs interleaved")
    say(f"# ms per iteration: median [min .. max] over {a.rounds} windows of {a.iters} back-to-back iterations between two device events")
    say()

    # ---- (a) the training step -----------------------------------------------------------------------------------------------------------
    def step_of(leg):
        opt = opts[leg]

        def step():
            model.zero_grad(set_to_none=True)
            b = {"image": batch["image"], "input_ids": batch["input_ids"].clone(), "attention_mask": batch["attention_mask"].clone(),
                 "caption_lengths": batch["caption_lengths"]}
            if leg == "on":
                b["image_ssl"] = views
            loss = sum(model(b)[0].values())
            loss.backward()
            opt.step(param_streams=bool(getattr(model, "two_streams_used", False)))
        return step

    steps = [(leg, step_of(leg)) for leg in ("off", "on")]
    t_step = measure(steps, a.rounds, a.iters, side=side)
    peak = {}
    for leg, fn in steps:                                 # peak memory of ONE step, the allocator's high-water mark
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[leg] = (torch.cuda.max_memory_allocated() / 2 ** 30, base / 2 ** 30)
    say("(a) training step: forward, losses, backward, AdamW (two tower streams); peak = torch.cuda.max_memory_allocated over one step")
    for leg in ("off", "on"):
        say(f"  branch {leg:3s}  step {fmt(t_step[leg])}  = {t_step[leg][0] / t_step['off'][0]:.3f} x off   {B / t_step[leg][0] * 1e3:8.1f} pairs/s   "
            f"peak {peak[leg][0]:6.2f} GiB = {peak[leg][0] / peak['off'][0]:.3f} x off  (resident before the step {peak[leg][1]:.2f} GiB)")
    model.zero_grad(set_to_none=True)
    say()

    # ---- (b) the image tower alone -------------------------------------------------------------------------------------------------------
    params = list(vit.parameters())
    T = 1 + vit.patch_embed.num_patches
    images = {B: batch["image"], 3 * B: torch.cat([batch["image"], views[0], views[1]])}
    gys = {n: torch.randn(n, T, dim, device=dev) * 1e-3 for n in images}

    def tower_on(n):
        def run():
            for p in params:
                p.grad = None
            vit(images[n]).backward(gys[n])
        return run

    t_tow = measure([(n, tower_on(n)) for n in images], a.rounds, a.iters)
    say("(b) image tower alone, forward + backward")
    for n in images:
        say(f"  {n:4d} images  {fmt(t_tow[n])}  = {t_tow[n][0] / t_tow[B][0]:.3f} x {B} images")
    for p in params:
        p.grad = None
    del gys
    say()

    # ---- (c) the branch's own pieces ------------------------------------------------------------------------------------------------------
    cls = torch.randn(2 * B, dim, device=dev, requires_grad=True)
    gz = torch.randn(2 * B, out_dim, device=dev) * 1e-3
    z = torch.nn.functional.normalize(torch.randn(2 * B, out_dim, device=dev), dim=-1).requires_grad_(True)
    hp = list(model.ssl_projection.parameters())

    def head():
        cls.grad = None
        for p in hp:
            p.grad = None
        with torch.autocast("cuda", dtype=adt):
            L2norm(model.ssl_projection(cls), dim=-1).backward(gz)

    def loss():
        z.grad = None
        model.ssl_loss(z[:B], z[B:])[0].backward()

    t_p = measure([("head", head), ("loss", loss)], a.rounds, a.iters * 10)
    say("(c) the branch's own pieces, forward + backward")
    say(f"  projection head + L2 norm, [{2 * B}, {dim}] -> {hidden} -> {out_dim}   {fmt(t_p['head'])}")
    say(f"  NT-Xent (cat, GEMM, rows, two gradient GEMMs), [{2 * B}, {out_dim}]      {fmt(t_p['loss'])}")
    say()

    # ---- (d) the plumbing ----------------------------------------------------------------------------------------------------------------
    feats = torch.randn(3 * B, T, dim, device=dev, requires_grad=True)
    g_head, g_cls = torch.randn(B, T, dim, device=dev), torch.randn(2 * B, dim, device=dev)

    def cat():
        torch.cat([batch["image"], views[0], views[1]])

    def slices():
        torch.autograd.grad([feats[:B], feats[B:, 0]], [feats], [g_head, g_cls])

    t_d = measure([("cat", cat), ("slices", slices)], a.rounds, a.iters * 10)
    say("(d) the slice and cat plumbing")
    say(f"  cat of the 3 x {B} images, forward                                   {fmt(t_d['cat'])}")
    say(f"  feats[:B] and feats[B:, 0] on [{3 * B}, {T}, {dim}] fp32, backward       {fmt(t_d['slices'])}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
