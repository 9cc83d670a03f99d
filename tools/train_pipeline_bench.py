#!/usr/bin/env python
"""Training transforms, the general route (simseg_train_transforms) against the special one (simseg_train_augment)
(profiles/train_pipeline.txt).  512 raw images of 375 x 500 already on the device, S = 224, device events around `--iters` calls.

  shipped  [random_resize_crop, autoaug] with the same sampled parameters through BOTH routes, interleaved in one process (old, new,
           old, new, ...): per route the median, min and max of `--reps` repetitions after `--warmup` untimed ones; the outputs are
           compared once (torch.equal).  The yardstick of the new route is the old one's median here, its allowance the old route's own
           spread (max - min).
  clip     [resize_bicubic, random_crop, random_flip, color_jitter] with random erasing reprob 0.25, mode pixel, through the new route.

  views    (profiles/train_views.txt) the SimCLR list [random_resize_crop, random_flip, color_distortion, gaussian_blur] through
           simseg_train_chain beside the shipped list through simseg_train_transforms, interleaved in one process; the blur alone:
           [random_resize_crop, gaussian_blur] with the blur applied to every image at radius 0.1 and at 2.0, beside [random_resize_crop];
           and Pillow on the host (apply_pipeline_pil, one process, `--host-images` images of the same batch and parameters).

    python tools/train_pipeline_bench.py [--parts shipped,clip] [--reps 24] [--iters 5] [--warmup 3]
    python tools/train_pipeline_bench.py --parts views [--host-images 64]
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python tools/train_pipeline_bench.py --parts clip --reps 1 --iters 4 --warmup 0
      (launches per batch = kernel calls / 4)
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from train_augment_bench import B, H, MEAN, S, STD, W, _raw  # noqa: E402


def _cfg(names, extra=()):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    argv = [f"transforms.train_transforms=[{','.join(names)}]", f"transforms.normalize.mean={MEAN}".replace(" ", ""),
            f"transforms.normalize.std={STD}".replace(" ", "")] + list(extra)
    return update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"), argv, update_clip_config)


def _timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def _batch():
    import torch
    dev = [torch.from_numpy(_raw(i)).cuda() for i in range(16)]
    return [dev[i % len(dev)] for i in range(B)]


def part_shipped(reps, iters, warmup):
    import numpy as np
    import torch
    from simseg_amd import augment as A, ops, pipeline as P, preproc
    cfg = _cfg(["random_resize_crop", "autoaug"])
    chain = P.parse_chain(cfg.transforms.train_transforms, cfg)
    batch, sizes = _batch(), [(H, W)] * B
    old_p = A.sample_params(sizes, np.random.default_rng(0))
    new_p = P.sample_pipeline_params(sizes, np.random.default_rng(0), chain)
    lut = preproc._lut_on(chain["lut"], "cuda")
    old_pl = A.plan(sizes, old_p, S, "cuda")
    new_pl = P.plan_pipeline(sizes, new_p, chain, "cuda")
    src = preproc._pack(batch, old_pl, "cuda")
    old = lambda: ops.train_augment(src, old_pl, lut)            # noqa: E731
    new = lambda: ops.train_transforms(src, new_pl, lut)         # noqa: E731
    same = torch.equal(old()[0], new()[0])
    for _ in range(warmup):
        _timed(old, iters)
        _timed(new, iters)
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(_timed(old, iters))
        t_new.append(_timed(new, iters))
    so, sn = _stats(t_old), _stats(t_new)
    return {"shipped_outputs_equal": bool(same), "shipped_old_route": so, "shipped_new_route": sn,
            "shipped_new_minus_old_ms": sn["median_ms"] - so["median_ms"],
            "shipped_within_old_spread": bool(sn["median_ms"] - so["median_ms"] <= so["spread_ms"])}


def part_clip(reps, iters, warmup):
    import numpy as np
    from simseg_amd import ops, pipeline as P, preproc
    cfg = _cfg(["resize_bicubic", "random_crop", "random_flip", "color_jitter"],
               [f"transforms.resize_bicubic.size={S}", f"transforms.random_crop.size={S}", "transforms.random_erasing.reprob=0.25",
                "transforms.random_erasing.remode=pixel"])
    chain = P.parse_chain(cfg.transforms.train_transforms, cfg)
    batch, sizes = _batch(), [(H, W)] * B
    p = P.sample_pipeline_params(sizes, np.random.default_rng(0), chain)
    lut = preproc._lut_on(chain["lut"], "cuda")
    pl = P.plan_pipeline(sizes, p, chain, "cuda")
    src = preproc._pack(batch, pl, "cuda")
    run = lambda: ops.train_transforms(src, pl, lut)             # noqa: E731
    for _ in range(warmup):
        _timed(run, iters)
    ms = [_timed(run, iters) for _ in range(reps)]
    return {"clip_list": chain["names"], "clip_erase": chain["erase"], "clip_images_erased": int((p["erase_n"] > 0).sum()),
            "clip_images_flipped": int(p["flip"].sum()), "clip_new_route": _stats(ms)}


def part_views(reps, iters, warmup, host_images):
    import time

    import numpy as np
    import torch
    from PIL import Image
    from simseg_amd import ops, pipeline as P, preproc
    batch, sizes = _batch(), [(H, W)] * B
    simclr = ["random_resize_crop", "random_flip", "color_distortion", "gaussian_blur"]
    lists = {"shipped": (["random_resize_crop", "autoaug"], False, None), "simclr": (simclr, True, None),
             "crop_only": (["random_resize_crop"], True, None), "blur_r0.1": (["random_resize_crop", "gaussian_blur"], True, 0.1),
             "blur_r2.0": (["random_resize_crop", "gaussian_blur"], True, 2.0)}
    runs, info, src = {}, {}, None
    for key, (names, full, radius) in lists.items():
        cfg = _cfg(names)
        chain = P.parse_chain(cfg.transforms.train_transforms, cfg, full=full)
        p = P.sample_pipeline_params(sizes, np.random.default_rng(0), chain)
        if radius is not None:                                   # the blur on every image, at one radius
            p["blur_apply"][:] = 1
            p["blur_radius"][:] = radius
        pl = P.plan_pipeline(sizes, p, chain, "cuda")
        lut = preproc._lut_on(chain["lut"], "cuda")
        if src is None:
            src = preproc._pack(batch, pl, "cuda")
        fn = ops.train_chain if full else ops.train_transforms
        runs[key] = (lambda fn=fn, pl=pl, lut=lut: fn(src, pl, lut))
        info[key] = (chain, p)
    for _ in range(warmup):
        for fn in runs.values():
            _timed(fn, iters)
    ms = {k: [] for k in runs}
    for _ in range(reps):                                        # interleaved: every list once per repetition
        for k, fn in runs.items():
            ms[k].append(_timed(fn, iters))
    res = {f"views_{k}": _stats(v) for k, v in ms.items()}
    chain, p = info["simclr"]
    nops = [len(P.op_chain(chain, p, i)) for i in range(B)]
    res.update(views_simclr_list=simclr, views_simclr_mean_ops=sum(nops) / B, views_simclr_blurred=int(p["blur_apply"].sum()),
               views_simclr_jittered=int(p["d_apply"].sum()), views_simclr_gray=int(p["d_gray"].sum()),
               views_simclr_images_per_s=B / (res["views_simclr"]["median_ms"] * 1e-3),
               views_shipped_images_per_s=B / (res["views_shipped"]["median_ms"] * 1e-3))
    # the same list, the same parameters, Pillow on the host (one process, decoded images in memory), checked against the device
    n = min(host_images, B)
    got = runs["simclr"]()[0][:n].cpu()
    pil = [Image.fromarray(batch[i].cpu().numpy()) for i in range(n)]
    t0 = time.perf_counter()
    want = [P.apply_pipeline_pil(pil[i], p, i, chain)[0] for i in range(n)]
    dt = time.perf_counter() - t0
    res.update(views_host_images=n, views_host_ms_per_image=dt / n * 1e3, views_host_images_per_s=n / dt,
               views_simclr_equals_host=bool(all(torch.equal(got[i], want[i]) for i in range(n))))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="shipped,clip")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-images", type=int, default=64)
    a = ap.parse_args()
    res = {"batch": B, "raw": [H, W], "size": S, "iters_per_rep": a.iters}
    parts = a.parts.split(",")
    if "shipped" in parts:
        res.update(part_shipped(a.reps, a.iters, a.warmup))
    if "clip" in parts:
        res.update(part_clip(a.reps, a.iters, a.warmup))
    if "views" in parts:
        res.update(part_views(a.reps, a.iters, a.warmup, a.host_images))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
