#!/usr/bin/env python
"""Training augmentation, device route vs host route (profiles/train_augment.txt).

  kernel   simseg_train_augment alone (its two launches) on a 512-image batch of 375 x 500 raw images already on the device, S = 224,
           parameters sampled from the policy: device events around `--iters` calls after a warm-up, median of `--repeats` windows;
           plus augment() end to end from device-resident images (sampling, plan, pack, kernels) in wall time
  copy     the host-to-device copy of the batch's raw bytes (about 288 MB) from pinned memory, device events, median of `--repeats`
  host     apply_pil + the host tail (_to_tensor, normalize) with 16 worker processes: images/s over `--host-images` images

    python tools/train_augment_bench.py [--parts kernel,copy,host] [--iters 20] [--repeats 5] [--host-images 2048]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MEAN, STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]
B, H, W, S = 512, 375, 500, 224


def _raw(seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 127 // (H + W - 2)], -1) + rng.integers(-30, 31, (H, W, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def _events(fn, iters, repeats):
    import torch
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def part_kernel(iters, repeats):
    import numpy as np
    import torch
    from simseg_amd import augment as A, ops, preproc
    raws = [torch.from_numpy(_raw(i)) for i in range(16)]
    dev = [r.cuda() for r in raws]
    batch = [dev[i % len(dev)] for i in range(B)]
    params = A.sample_params([(H, W)] * B, np.random.default_rng(0))
    lut = preproc._lut_on(preproc.make_lut(MEAN, STD), "cuda")
    pl = A.plan([(H, W)] * B, params, S, "cuda")
    src = preproc._pack(batch, pl, "cuda")
    for _ in range(3):
        ops.train_augment(src, pl, lut)
    torch.cuda.synchronize()
    ms = _events(lambda: ops.train_augment(src, pl, lut), iters, repeats)
    out = {"kernel_ms_per_batch": statistics.median(ms), "kernel_ms_windows": ms, "ops_applied": {
        A.OPS[o]: int(((params["op1"] == o) & (params["apply1"] == 1)).sum() + ((params["op2"] == o) & (params["apply2"] == 1)).sum())
        for o in range(1, len(A.OPS))}}
    # end to end from device-resident images: sample + plan + pack + kernels, wall time per batch
    rng = np.random.default_rng(1)
    aug = A.TrainAugment(S, (0.6, 1.0), True, preproc.make_lut(MEAN, STD))
    aug(batch, rng)
    torch.cuda.synchronize()
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        aug(batch, rng)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    out["augment_e2e_ms_per_batch"] = statistics.median(walls)
    t0 = time.perf_counter()
    for _ in range(repeats):
        aug.sample([(H, W)] * B, rng)
    out["sample_ms_per_batch"] = (time.perf_counter() - t0) * 1e3 / repeats
    return out


def part_copy(repeats):
    import torch
    n = B * H * W * 3
    host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    host.fill_(7)
    dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    ms = _events(lambda: dev.copy_(host, non_blocking=True), 1, repeats)
    return {"h2d_bytes": n, "h2d_ms": statistics.median(ms), "h2d_ms_windows": ms, "h2d_GBps": n / statistics.median(ms) / 1e6}


def _host_worker(job):
    import numpy as np
    import torch
    from PIL import Image
    from simseg_amd import augment as A
    torch.set_num_threads(1)
    seed, n = job
    rng = np.random.default_rng(seed)
    img = Image.fromarray(_raw(seed))
    params = A.sample_params([(H, W)] * n, rng)
    t0 = time.perf_counter()
    for i in range(n):
        A.apply_pil(img, params, i, S, MEAN, STD)
    return n, time.perf_counter() - t0


def part_host(n, workers=16):
    import multiprocessing as mp
    per = n // workers
    with mp.get_context("spawn").Pool(workers) as pool:
        pool.map(_host_worker, [(100 + i, 4) for i in range(workers)])          # imports + warm-up
        t0 = time.perf_counter()
        res = pool.map(_host_worker, [(i, per) for i in range(workers)])
        wall = time.perf_counter() - t0
    one = sum(t for _, t in res) / sum(k for k, _ in res)
    return {"host_workers": workers, "host_images": per * workers, "host_images_per_s": per * workers / wall,
            "host_ms_per_image_one_core": one * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,copy,host")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=2048)
    a = ap.parse_args()
    res = {"batch": B, "raw": [H, W], "size": S}
    parts = a.parts.split(",")
    if "kernel" in parts:
        res.update(part_kernel(a.iters, a.repeats))
    if "copy" in parts:
        res.update(part_copy(a.repeats))
    if "host" in parts:
        res.update(part_host(a.host_images))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
