#!/usr/bin/env python
"""Multi-scale / flip test-time augmentation against the single-scale sliding-window evaluation (profiles/seg_tta.txt).

ViT-B/16 towers (random weights), 512-pixel windows at stride 256, 171 classes, seeded synthetic RAW uint8 images of Pascal / COCO
shapes resized on the device (short side 512, bicubic), one process:
  routes : segpost.evaluate_sharded over the same raw batches, single scale against scales (0.75, 1.0, 1.25) with flip (6 passes);
           source images/s, the two routes alternating, `--repeats` times each (median and the spread of the repeats);
  kernel : ops.slide_stitch_multi on one batch's six passes against six ops.slide_stitch calls on the same per-pass maps (the fused
           kernel against what the single-pass kernel needs for the same maps), device events, alternating, median and spread.

    python tools/seg_tta_bench.py [--mode bf16] [--crf 0] [--batches 4] [--batch 8] [--repeats 3] [--kernel-reps 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WIN, STRIDE, C, TOP = 512, 256, 171, 10
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALES = (0.75, 1.0, 1.25)
RAW_SIZES = [(375, 500), (500, 375), (333, 500), (480, 640), (427, 640)]


def build_model():
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    argv = [f"transforms.input_size={WIN}", "model.image_encoder.pretrained=False", "model.text_encoder.pretrained=False"]
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"), argv, update_clip_config)
    torch.manual_seed(5)
    return build_from_cfg(cfg.model.name, cfg, PIPELINE).cuda().eval()


def raw_image(H, W, k):
    """Smooth colour fields plus noise: something for the resampling filters to do."""
    rng = np.random.default_rng(1000 + k)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(yy / (7.0 + c) + k) * np.cos(xx / (11.0 - c)) for c in range(3)], -1)
    return torch.from_numpy(np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8))


def make_batches(nb, bs):
    g = torch.Generator().manual_seed(0)
    out, k = [], 0
    for _ in range(nb):
        imgs, labs = [], []
        for _ in range(bs):
            H, W = RAW_SIZES[k % len(RAW_SIZES)]
            imgs.append(raw_image(H, W, k % 16))
            labs.append(torch.randint(0, C, (H, W), generator=g, dtype=torch.int64).to(torch.uint8))
            k += 1
        out.append((imgs, labs))
    return out


def make_preprocess(spec, tta):
    from simseg_amd import preproc, segpost

    def single(raws):
        return preproc.preprocess(raws, spec, device="cuda")

    def multi(raws):
        res = single(raws)
        passes, src = [], None
        for s, target in zip(SCALES, segpost.tta_sizes(res["sizes"], SCALES)):
            if s == 1.0:
                packed, sizes = res["packed"], res["sizes"]
                res["base"] = len(passes)
            else:
                scaled = preproc.preprocess_extents(raws, target, spec, device="cuda", src=src)
                packed, sizes, src = scaled["packed"], scaled["sizes"], scaled["src"]
            passes += [(packed, sizes, False), (packed, sizes, True)]
        res["passes"] = passes
        return res
    return multi if tta else single


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--crf", type=int, default=0)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seg_tta_bench needs an MI355X"
    from simseg_amd import heads, ops, preproc, segpost
    os.environ["SIMSEG_AMD_COMPUTE"] = args.mode
    sim_dt = torch.bfloat16 if args.mode == "bf16" else None
    model = build_model()
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=torch.Generator().manual_seed(0)), dim=-1).cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    spec = preproc.make_spec("short", WIN, "bicubic", mean=MEAN, std=STD)
    batches = make_batches(args.batches, args.batch)
    nimg = args.batches * args.batch
    crf = bool(args.crf)

    def route(tta):
        t0 = time.perf_counter()
        res = segpost.evaluate_sharded(model, batches, text, TOP, slide=(WIN, STRIDE), crf=crf, mean=mean, std=std, sim_dtype=sim_dt, device="cuda",
                                       preprocess=make_preprocess(spec, tta))
        torch.cuda.synchronize()
        return nimg / (time.perf_counter() - t0), float(res["miou"])

    with torch.no_grad():
        for tta in (False, True):                     # warm-up: every shape of both routes
            route(tta)
        rates = {False: [], True: []}
        for _ in range(args.repeats):
            for tta in (False, True):
                rates[tta].append(route(tta)[0])
        for tta in (False, True):
            print(json.dumps({"route": "scales 0.75,1.0,1.25 + flip (6 passes)" if tta else "single scale", "mode": args.mode, "crf": crf, "images": nimg,
                              "images_s": spread(rates[tta])}), flush=True)

        # the fusion kernel alone: one batch's six passes, their maps captured as the towers return them
        seen = []
        pts = heads.patch_text_similarity

        def rec(p, t, compute_dtype=None):
            seen.append(pts(p, t, compute_dtype=compute_dtype))
            return seen[-1]
        heads.patch_text_similarity = rec
        try:
            pre = make_preprocess(spec, True)(batches[0][0])
            st = segpost.encode_images_multiscale(model, pre["passes"], text, TOP, win=WIN, stride=STRIDE, crf=False, sim_dtype=sim_dt, base=pre["base"])
        finally:
            heads.patch_text_similarity = pts
        sims = [s.float().contiguous() for s in seen]
        plans = [ops.slide_plan(sizes, WIN, STRIDE, "cuda") for _, sizes, _ in pre["passes"]]
        flips = [f for _, _, f in pre["passes"]]
        base, cand = st["plan"], st["cand_idx"]

        def fused():
            return ops.slide_stitch_multi(sims, plans, flips, base, cand)

        def six():
            return [ops.slide_stitch(s, pl, cand) for s, pl in zip(sims, plans)]

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3
        for _ in range(3):
            fused(); six()
        torch.cuda.synchronize()
        t_f, t_s = [], []
        for _ in range(args.kernel_reps):
            t_f.append(timed(fused)); t_s.append(timed(six))
        print(json.dumps({"kernel": "slide_stitch_multi, P = 6 (with its output zero fills and table upload)", "images": args.batch,
                          "visited_slots": int((cand >= 0).sum()), "us": spread(t_f)}), flush=True)
        print(json.dumps({"kernel": "6 x slide_stitch on the same per-pass maps (with their output zero fills)", "images": args.batch,
                          "visited_slots": int((cand >= 0).sum()), "us": spread(t_s)}), flush=True)


if __name__ == "__main__":
    main()
