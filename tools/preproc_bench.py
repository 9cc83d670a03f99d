#!/usr/bin/env python
"""Image preprocessing, host route vs device route (profiles/preproc_device.txt).

  host     PIL resize -> _to_tensor -> normalize (build_transforms) of a 500 x 375 image, per image: on one core, and with 16 worker
           processes (the CPUs one GPU command has), for `resize` 512 (bilinear, -> 512 x 512) and `resize_bicubic` 512 (-> 512 x 683)
  kernel   simseg_image_preprocess alone on 256 such images already on the device (device events around `--iters` launches, every shape
           warmed, about half a second of launches per timed window): time, output pixels/s, and the bytes of the model - source bytes once + 12 output bytes per output pixel - per
           second against the HBM rates; plus preprocess() from host tensors (pack into pinned memory + one copy + the kernel)
  e2e      tools/seg_eval_device.py --synthetic N --synthetic-raw 375x500,500x375,333x500, ViT-B @512 in bf16, without and with the
           DenseCRF and with --slide 512,256: images/s of both routes, alternating, `--repeats` times each, in subprocesses

    python tools/preproc_bench.py [--parts host,kernel,e2e] [--images 2048] [--repeats 2] [--legs nocrf,crf,slide]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # spec; measured float4 copy
SPECS = {"resize 512 bilinear": ["transforms.resize.size=512"],
         "resize_bicubic 512": ["transforms.valid_transforms=[resize_bicubic]", "transforms.resize_bicubic.size=512"]}


def _cfg(argv):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"), list(argv) + ["transforms.input_size=512"], update_clip_config)


def _raw(seed, H=375, W=500):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _host_worker(job):
    argv, n, seed = job
    import torch
    from PIL import Image
    from simseg.transforms import build_transforms
    torch.set_num_threads(1)
    tf = build_transforms(_cfg(argv), "valid")
    img = Image.fromarray(_raw(seed))
    tf(img)
    t0 = time.perf_counter()
    for _ in range(n):
        tf(img)
    return time.perf_counter() - t0


def part_host(n):
    import multiprocessing as mp
    print("host transform (PIL resize + _to_tensor + normalize) of a 500 x 375 image; ms per image")
    print(f"{'transform':24s} {'1 core ms':>10s} {'16 workers: images/s':>22s} {'ms/image/worker':>16s}")
    out = {}
    for name, argv in SPECS.items():
        one = _host_worker((argv, n, 0)) / n * 1e3
        with mp.get_context("fork").Pool(16) as pool:
            t0 = time.perf_counter()
            ts = pool.map(_host_worker, [(argv, n, i) for i in range(16)])
            wall = time.perf_counter() - t0
        rate = 16 * n / max(ts)              # the workers' own timed loops (their start-up is outside)
        print(f"{name:24s} {one:10.2f} {rate:22.0f} {max(ts) / n * 1e3:16.2f}      (wall incl. worker start-up {wall:.1f} s)")
        out[name] = {"one_core_ms": one, "workers16_images_per_s": rate}
    return out


def part_kernel(iters, nimg=256):
    import torch
    from simseg.transforms import build_device_transforms
    from simseg_amd import ops, preproc
    print(f"\nkernel alone: {nimg} images of 375 x 500 (last row: 512 x 512) on the device, {iters} timed launches after warm-up (device events)")
    print(f"{'transform':26s} {'ms':>8s} {'images/s':>10s} {'Gpix/s':>8s} {'model GB':>9s} {'TB/s':>6s} {'of 8.0':>7s} {'of 6.29':>8s}   {'preprocess() from host ms':>26s}")
    out = {}
    planned = {}
    shapes = [(name, argv, (375, 500)) for name, argv in SPECS.items()]
    # the same output bytes as the first shape with ONE tap per axis (both passes are the identity): time against taps at equal traffic
    shapes.append(("512x512 -> 512 (identity)", SPECS["resize 512 bilinear"], (512, 512)))
    for name, argv, (H, W) in shapes:
        _, spec = build_device_transforms(_cfg(argv), "valid")
        raws = [torch.from_numpy(_raw(100 + i % 16, H, W)) for i in range(nimg)]
        pl = preproc.plan([(H, W)] * nimg, spec, "cuda")
        src = torch.cat([r.reshape(-1) for r in raws]).cuda()
        lut = spec["lut"].cuda()
        planned[name] = (spec, raws, pl, src, lut)
        for _ in range(3):
            ops.image_preprocess(src, pl, lut)
            preproc.preprocess(raws, spec)
    torch.cuda.synchronize()
    for rep in range(2):                      # the two shapes alternate; the second round is reported
        for name, (spec, raws, pl, src, lut) in planned.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                ops.image_preprocess(src, pl, lut)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / iters
            t0 = time.perf_counter()
            for _ in range(5):
                preproc.preprocess(raws, spec)
            torch.cuda.synchronize()
            whole = (time.perf_counter() - t0) / 5 * 1e3
            pix = pl["out_numel"] // 3
            model = pl["src_bytes"] + 12 * pix
            bw = model / (ms * 1e-3)
            if rep == 1:
                print(f"{name:26s} {ms:8.3f} {nimg / ms * 1e3:10.0f} {pix / ms / 1e6:8.2f} {model / 1e9:9.3f} {bw / 1e12:6.2f} {bw / HBM_PEAK:7.1%} {bw / HBM_COPY:8.1%}   {whole:26.2f}")
                out[name] = {"ms": ms, "model_bytes": model, "bytes_per_s": bw, "preprocess_from_host_ms": whole}
    from tools.kernel_resources import kernel_resources
    obj = os.path.join(REPO, "simseg_amd", "build", "preproc.o")
    if os.path.exists(obj):
        for kname, vg, sp, sc, lds in kernel_resources(obj):
            print(f"resources: {kname.split('(')[0]}: {vg} VGPRs, {sp} spilled, {sc} B scratch, {lds} B LDS per workgroup")
    else:
        print("resources: simseg_amd/build/preproc.o is not here (objects are not shipped); run tools/kernel_resources.py where the library was built")
    return out


LEGS = {"nocrf": ["--no-crf"], "crf": [], "slide": ["--no-crf", "--slide", "512,256", "transforms.valid_transforms=[resize_bicubic]", "transforms.resize_bicubic.size=512"]}


def part_e2e(images, repeats, legs, batch):
    print(f"\nend to end: tools/seg_eval_device.py --synthetic {images} --batch {batch} --synthetic-raw 375x500,500x375,333x500, ViT-B/16 @512, bf16, "
          f"one process per run, routes alternating; images/s as the tool prints it (its whole loop, loader included)")
    out = {}
    env = dict(os.environ, PYTHONPATH=REPO, SIMSEG_AMD_COMPUTE="bf16")
    port = 29560
    for leg in legs:
        rates, digests = {"host": [], "device": []}, set()
        for rep in range(repeats):
            for route in ("host", "device"):
                port += 1
                env["MASTER_PORT"] = str(port)
                cmd = [sys.executable, os.path.join(REPO, "tools", "seg_eval_device.py"), "--cfg", os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"),
                       "--synthetic", str(images), "--batch", str(batch), "--synthetic-raw", "375x500,500x375,333x500", "transforms.input_size=512",
                       "transforms.resize.size=512"] + LEGS[leg] + (["--device-preproc"] if route == "device" else [])
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
                if r.returncode != 0:
                    raise SystemExit(f"{leg} / {route} failed (exit {r.returncode}): {r.stderr[-1500:]}")
                rates[route].append(float(re.search(r"([0-9.]+) images/s", r.stdout).group(1)))
                digests.add(re.search(r"histogram sha256 ([0-9a-f]{64})", r.stdout).group(1)[:16])
                print(f"  {leg:6s} {route:6s} run {rep}: {rates[route][-1]:8.1f} images/s", flush=True)
        h, d = rates["host"], rates["device"]
        spread = (max(h) - min(h)) / (sum(h) / len(h))
        print(f"{leg:6s} host {sum(h) / len(h):8.1f} images/s (spread {spread:.1%} over {len(h)} runs)   device {sum(d) / len(d):8.1f} images/s "
              f"(min {min(d):.1f})   device / host {sum(d) / len(d) / (sum(h) / len(h)):.2f}x   histogram digests: {sorted(digests)}", flush=True)
        out[leg] = {"host": h, "device": d, "digests": sorted(digests)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="host,kernel,e2e")
    ap.add_argument("--host-images", type=int, default=100)
    ap.add_argument("--iters", type=int, default=1000, help="timed launches per shape (0.4-0.8 ms each: about half a second per window)")
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--legs", default="nocrf,crf,slide")
    args = ap.parse_args()
    parts = args.parts.split(",")
    res = {}
    if "host" in parts:                       # before anything touches the GPU: the workers are forked
        res["host"] = part_host(args.host_images)
    if "kernel" in parts or "e2e" in parts:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("preproc_bench: the kernel and end-to-end parts need an MI355X (no CPU fallback, no CPU timing)")
    if "kernel" in parts:
        res["kernel"] = part_kernel(args.iters)
    if "e2e" in parts:
        res["e2e"] = part_e2e(args.images, args.repeats, args.legs.split(","), args.batch)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
