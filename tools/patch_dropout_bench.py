#!/usr/bin/env python
"""What patch dropout (simseg_amd/patchdrop.py) saves on the training step, measured: ViT-B/16 + BERT-base, 512 pairs at 224^2 and L = 77 in
bf16 - the shape of bench.py's step, built with bench.py's own model and batch builders - at drop rates 0, 0.25, 0.5 and 0.75 in ONE
process, rates interleaved round by round:

    (a) the training step (forward, loss, backward, AdamW; two tower streams) and torch.cuda.max_memory_allocated over one step
    (b) the image tower alone, forward + backward
    (c) the embedding node alone, forward and backward: ViTEmbedKeepFn at each rate against ViTEmbedFn (rate 0), the backward fed as in the
        step (the gradient arrives as its 16-bit shadow only)
    (d) the sampler, and the three other new kernels alone

Every window is `--iters` back-to-back iterations between two device events on the main stream (which waits for the side stream first);
median [min .. max] over `--rounds` windows after warm-up of every shape.

    python tools/patch_dropout_bench.py [--quick] [--out profiles/patch_dropout.txt]"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LINES = []
RATES = (0.0, 0.25, 0.5, 0.75)


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
        raise SystemExit("patch_dropout_bench.py measures on an MI355X; no GPU here")
    import bench
    from simseg.models import PIPELINE
    from simseg.models.pipelines.clip import _side_stream
    from simseg.utils import logger
    from simseg_amd import ops, patchdrop, towers
    from simseg_amd.nn import VIT_ARCH, ViT
    from simseg_amd.optim import AdamW
    logger.STREAM = sys.stderr
    os.environ["SIMSEG_AMD_COMPUTE"] = "bf16"
    adt = torch.bfloat16
    dev = torch.device("cuda", 0)
    tag, img, B, L = ("vit_base_patch16_224_in21k", 224, 512, 77) if not a.quick else ("vit_test_patch16", 96, 8, 25)
    if a.quick:
        a.rounds, a.iters = 1, 2
    dim = VIT_ARCH[tag]["dim"]
    cfg, build = bench.build_model(tag, dim, img)
    torch.manual_seed(1234)
    model = build(cfg.model.name, cfg, PIPELINE).to(dev).train()
    (vit,) = [m for m in model.modules() if isinstance(m, ViT)]
    N = vit.patch_embed.num_patches
    opt = AdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=1e-3, half_dtype=adt)
    side = _side_stream(dev)
    opt.set_param_streams({p: side for p in list(model.text_encoder.parameters()) + list(model.text_projection.parameters())})
    batch = bench.synthetic_batch(B, img, L, 30522, 1000, dev)
    pr = torch.cuda.get_device_properties(0)
    say(f"# tools/patch_dropout_bench.py{' --quick' if a.quick else ''}   device: {pr.name}, torch {torch.__version__}")
    say(f"# {tag} + {cfg.model.text_encoder.tag}, {B} pairs at {img}^2 (N = {N} patches), L = {L}, bf16 compute, AdamW; one process, rates interleaved")
    say(f"# ms per iteration: median [min .. max] over {a.rounds} windows of {a.iters} back-to-back iterations between two device events")
    say()

    # ---- (a) the training step -----------------------------------------------------------------------------------------------------------
    def step_at(rate):
        def step():
            vit.set_patch_drop(rate)
            opt.zero_grad(set_to_none=True)
            b = {"image": batch["image"], "input_ids": batch["input_ids"].clone(), "attention_mask": batch["attention_mask"].clone(),
                 "caption_lengths": batch["caption_lengths"]}
            loss = model(b)[0]["nce_loss"]
            loss.backward()
            opt.step(param_streams=bool(getattr(model, "two_streams_used", False)))
        return step

    steps = [(r, step_at(r)) for r in RATES]
    t_step = measure(steps, a.rounds, a.iters, side=side)
    peak = {}
    for r, fn in steps:                                   # peak memory of ONE step at each rate, above nothing: the allocator's high-water mark
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[r] = (torch.cuda.max_memory_allocated() / 2 ** 30, base / 2 ** 30)
    say("(a) training step: forward, loss, backward, AdamW (two tower streams); peak = torch.cuda.max_memory_allocated over one step")
    for r in RATES:
        K = patchdrop.num_keep(N, r)
        say(f"  rate {r:4.2f}  T = {1 + K:3d} tokens  step {fmt(t_step[r])}  = {t_step[r][0] / t_step[0.0][0]:.3f} x rate 0   {B / t_step[r][0] * 1e3:8.1f} pairs/s   "
            f"peak {peak[r][0]:6.2f} GiB = {peak[r][0] / peak[0.0][0]:.3f} x rate 0  (resident before the step {peak[r][1]:.2f} GiB)")
    vit.set_patch_drop(0.0)
    opt.zero_grad(set_to_none=True)
    say()

    # ---- (b) the image tower alone -------------------------------------------------------------------------------------------------------
    params = [p for p in vit.parameters()]
    gys = {r: torch.randn(B, 1 + patchdrop.num_keep(N, r), dim, device=dev) * 1e-3 for r in RATES}

    def tower_at(rate):
        def run():
            vit.set_patch_drop(rate)
            for p in params:
                p.grad = None
            vit(batch["image"]).backward(gys[rate])
        return run

    t_tow = measure([(r, tower_at(r)) for r in RATES], a.rounds, a.iters)
    say("(b) image tower alone, forward + backward (the draw included)")
    for r in RATES:
        say(f"  rate {r:4.2f}  {fmt(t_tow[r])}  = {t_tow[r][0] / t_tow[0.0][0]:.3f} x rate 0")
    vit.set_patch_drop(0.0)
    for p in params:
        p.grad = None
    say()

    # ---- (c) the embedding node alone ----------------------------------------------------------------------------------------------------
    ep = [vit.patch_embed.proj.weight, vit.patch_embed.proj.bias, vit.cls_token, vit.pos_embed]
    image = batch["image"]
    fwd, bwd, shadowed = [], [], {}

    def node(rate):
        K = patchdrop.num_keep(N, rate)
        keep, inv = patchdrop.sample_keep(B, N, K, 7, dev) if rate > 0 else (None, None)
        name = f"ViTEmbedKeepFn rate {rate:4.2f}" if rate > 0 else "ViTEmbedFn (all patches) "

        def f():
            if rate > 0:
                return towers.ViTEmbedKeepFn.apply(image, *ep, keep, inv, adt)
            return towers.ViTEmbedFn.apply(image, *ep, adt)

        y = f()
        gy = torch.randn(B, 1 + K, dim, device=dev) * 1e-3
        gy16 = gy.to(adt)
        dsum = gy16.view(-1, dim).float().sum(0)

        def b():
            # as in the step: the first block's backward hands over an unwritten fp32 tensor whose values live in its 16-bit shadow
            gy._simseg_lazy32 = True
            towers._put_shadow(gy, gy16, dsum)
            torch.autograd.grad(y, ep, gy, retain_graph=True)

        hits = towers.SHADOW_HITS[0]
        try:
            b()
            shadowed[name] = towers.SHADOW_HITS[0] > hits
        except RuntimeError:                              # (autograd handed the node another tensor object: time the cast path instead)
            shadowed[name] = False
            del gy._simseg_lazy32

            def b():                                      # noqa: F811
                torch.autograd.grad(y, ep, gy, retain_graph=True)
        fwd.append((name, f))
        bwd.append((name, b))

    for r in RATES:
        node(r)
    t_f, t_b = measure(fwd, a.rounds, a.iters * 4), measure(bwd, a.rounds, a.iters * 4)
    say("(c) the embedding node alone: forward (gather + GEMM + position rows) and backward (dW, db, dcls, dpos)")
    base_f, base_b = t_f[fwd[0][0]][0], t_b[bwd[0][0]][0]
    for (name, _) in fwd:
        say(f"  {name}  forward {fmt(t_f[name])} = {t_f[name][0] / base_f:.3f} x   backward {fmt(t_b[name])} = {t_b[name][0] / base_b:.3f} x"
            f"   ({'16-bit shadow consumed' if shadowed[name] else 'fp32 gradient, cast path'})")
    say()

    # ---- (d) the new kernels alone -------------------------------------------------------------------------------------------------------
    say("(d) the kernels alone")
    kern = []
    pos2 = vit.pos_embed.detach().reshape(N + 1, dim)
    cls1 = vit.cls_token.detach().reshape(-1)
    keepers = []
    for r in RATES[1:]:
        K = patchdrop.num_keep(N, r)
        keep, inv = patchdrop.sample_keep(B, N, K, 7, dev)
        x = torch.zeros(B, 1 + K, dim, device=dev)
        dx16 = torch.randn(B, 1 + K, dim, device=dev).to(adt)
        keepers.append((keep, inv, x, dx16))
        kern += [(f"patch_keep_sample    rate {r:4.2f}", lambda K=K: patchdrop.sample_keep(B, N, K, 7, dev)),
                 (f"vit_im2col_keep      rate {r:4.2f}", lambda keep=keep: ops.vit_im2col_keep(image, keep, adt)),
                 (f"vit_keep_rows        rate {r:4.2f}", lambda keep=keep, x=x: ops.vit_keep_rows(cls1, pos2, keep, x)),
                 (f"vit_keep_pos_grad    rate {r:4.2f}", lambda inv=inv, dx16=dx16: ops.vit_keep_pos_grad(dx16, inv))]
    dxf = torch.randn(B, 1 + N, dim, device=dev).to(adt)
    dpos = torch.zeros((N + 1) * dim, device=dev)
    kern += [("vit_im2col (all patches)      ", lambda: ops.vit_im2col(image, adt)),
             ("colsum_accum -> dpos (all)    ", lambda: ops.colsum_accum(dxf.view(B, (N + 1) * dim), dpos))]
    t_k = measure(kern, a.rounds, a.iters * 10)
    for name, _ in kern:
        say(f"  {name}  {fmt(t_k[name])}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
