#!/usr/bin/env python
"""Sliding-window evaluation throughput on uniform and on COCO-Stuff-shaped ragged images (profiles/slide_ragged.txt).

ViT-B/16 towers (random weights), 512-pixel windows at stride 256, 171 classes, fp32 and bf16, with and without the DenseCRF:
  (a) uniform 512 x 1024 images (3 windows each) through the exact-tiling path (tensor batches: encode_batch_sliding + finish_batch);
  (b) the same images as lists through the any-size path (encode_images_sliding + finish_sliding);
  (c) COCO-Stuff-shaped ragged images: short side 512, long side cycling over {512, 640, 683, 768, 910}, both orientations (1 to 3
      windows per image), as lists through the any-size path.
Every leg runs segpost.evaluate_sharded (the pipelined product loop) over the same batches; `enc` is the encoder side alone (the towers
and everything up to the stitched maps, each batch synchronised), `e2e` the whole evaluation.  Windows/s and source images/s.

    python tools/slide_ragged_bench.py [--legs a,b,c] [--modes fp32,bf16] [--crf 0,1] [--batches 6] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WIN, STRIDE, C, TOP = 512, 256, 171, 10
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def build_model():
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    argv = [f"transforms.input_size={WIN}", "model.image_encoder.pretrained=False", "model.text_encoder.pretrained=False"]
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"), argv, update_clip_config)
    torch.manual_seed(5)
    return build_from_cfg(cfg.model.name, cfg, PIPELINE).cuda().eval()


def make_sets(nb, g):
    """-> {leg: [(images, labels), ...]}: 8 uniform images per batch for (a) / (b), 12 ragged images per batch for (c)."""
    uni, rag = [], []
    longs = (512, 640, 683, 768, 910)
    k = 0
    for _ in range(nb):
        x = torch.randn(8, 3, 512, 1024, generator=g)
        lab = torch.randint(0, C, (8, 512, 1024), generator=g, dtype=torch.int64).to(torch.uint8)
        uni.append((x, lab))
        imgs, labs = [], []
        for _ in range(12):
            L = longs[k % 5]
            hw = (512, L) if (k // 5) % 2 == 0 else (L, 512)
            k += 1
            imgs.append(torch.randn(3, *hw, generator=g))
            labs.append(torch.randint(0, C, hw, generator=g, dtype=torch.int64).to(torch.uint8))
        rag.append((imgs, labs))
    return {"a": uni, "b": [([x[i] for i in range(8)], [l[i] for i in range(8)]) for x, l in uni], "c": rag}


def windows_of(batch):
    from simseg_amd import segpost
    imgs = batch[0]
    shapes = [tuple(imgs.shape[-2:])] * imgs.shape[0] if torch.is_tensor(imgs) else [tuple(i.shape[-2:]) for i in imgs]
    return sum(len(segpost.slide_windows(h, w, WIN, STRIDE)) for h, w in shapes), len(shapes)


def run_leg(model, text, batches, crf, sim_dt, warmup):
    from simseg_amd import segpost
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    dev = [(([i.cuda() for i in x] if isinstance(x, list) else x.cuda()), ([l.cuda() for l in y] if isinstance(y, list) else y.cuda()))
           for x, y in batches]
    nwin = sum(windows_of(b)[0] for b in dev[warmup:])
    nimg = sum(windows_of(b)[1] for b in dev[warmup:])

    def encode(x):
        if isinstance(x, list):
            return segpost.encode_images_sliding(model, x, text, TOP, win=WIN, stride=STRIDE, crf=crf, mean=mean, std=std, sim_dtype=sim_dt)
        return segpost.encode_batch_sliding(model, x, text, TOP, win=WIN, stride=STRIDE, crf=crf, mean=mean, std=std, sim_dtype=sim_dt)

    with torch.no_grad():
        for x, _ in dev[:warmup]:
            encode(x)
        segpost.evaluate_sharded(model, dev[:warmup], text, TOP, slide=(WIN, STRIDE), crf=crf, mean=mean, std=std, sim_dtype=sim_dt, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for x, _ in dev[warmup:]:
            encode(x)
            torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        res = segpost.evaluate_sharded(model, dev[warmup:], text, TOP, slide=(WIN, STRIDE), crf=crf, mean=mean, std=std, sim_dtype=sim_dt, device="cuda")
        torch.cuda.synchronize()
        t_e2e = time.perf_counter() - t0
    return {"windows": nwin, "images": nimg, "enc_windows_s": nwin / t_enc, "e2e_windows_s": nwin / t_e2e, "e2e_images_s": nimg / t_e2e,
            "miou": float(res["miou"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--crf", default="0,1")
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "slide_ragged_bench needs an MI355X"
    model = build_model()
    g = torch.Generator().manual_seed(0)
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=g), dim=-1).cuda()
    sets = make_sets(args.batches + args.warmup, g)
    for mode in args.modes.split(","):
        os.environ["SIMSEG_AMD_COMPUTE"] = mode
        sim_dt = torch.bfloat16 if mode == "bf16" else None
        for crf in (bool(int(v)) for v in args.crf.split(",")):
            for leg in args.legs.split(","):
                r = run_leg(model, text, sets[leg], crf, sim_dt, args.warmup)
                r.update(leg=leg, mode=mode, crf=crf)
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
