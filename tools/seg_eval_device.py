#!/usr/bin/env python
"""Zero-shot segmentation evaluation with the whole per-image body on the GPU.

Same command line, config, checkpoint and data layout as the reference's tools/seg_evaluation.py; the differences are in
how the work is laid out, not in what is computed:
  * the prompt-ensemble class embeddings are one batched text-tower call (reference: one batch per class, :57-75);
  * images are processed `--batch` at a time and the similarity map is one fused kernel for all classes (reference: one
    image, up to five GEMVs with host syncs, :99-143);
  * candidate selection, min-max normalisation, binarisation, 7x7 dilate/erode, nearest resize, score-weighted argmax and
    the IoU histograms run on the device (simseg_amd.segpost, :112-170), and so does the DenseCRF between normalisation and
    morphology (:31-54 / :153: mean-field inference on two permutohedral lattices, simseg_dense_crf).  `--refine pamr` runs PAMR
    (pixel-adaptive mask refinement, simseg_pamr; `--pamr-iters`, `--pamr-dilations`) in its place.  `--no-crf` stops at the
    CRF's unary decision; with pydensecrf installed `--host-crf` routes the maps through the library on the host instead
    (cross-check of the device CRF against the package the reference uses).

    python tools/seg_eval_device.py --cfg configs/clip/simseg.vit-b.yaml --ckpt_path ckpts/simseg.vit-b.pth
    python tools/seg_eval_device.py --cfg configs/clip/simseg.vit-s.yaml --synthetic 64        # no data / checkpoint needed

Sliding windows (`--slide WIN,STRIDE`) take images of ANY size: windows are placed as mmseg's slide_inference does (the last one flush
with the border; an image smaller than a window gets one zero-padded window) and `--batch` consecutive images of different sizes go
through the towers together as lists (segpost.encode_images_sliding); a batch of equal-sized images that the windows tile exactly keeps
the exact-tiling route (segpost.encode_batch_sliding).  Images of different sizes cannot be collated, so the loader must yield one image
per batch (data.batch_size_val=1, as the shipped configs set).  The recommended COCO-Stuff run resizes the short side to 512 (bicubic)
and slides 512-pixel windows at stride 256:

    python tools/seg_eval_device.py --cfg configs/clip/simseg.vit-b.yaml --ckpt_path ckpts/simseg.vit-b.pth --slide 512,256 \
        transforms.input_size=512 transforms.valid_transforms=[resize_bicubic] data.valid_name=[coco_stuff]
    python tools/seg_eval_device.py --cfg configs/clip/simseg.vit-s.yaml --synthetic 8 --synthetic-sizes 96x150,80x80,131x257 --slide 96,48 \
        transforms.input_size=96 model.image_encoder.tag=vit_test_patch16 model.image_encoder.embedding_dim=128 \
        model.text_encoder.tag=bert-test model.text_encoder.embedding_dim=128      # ragged images, no data / checkpoint needed

`--device-preproc` leaves only the decode on the host: the loader yields raw uint8 images, and resize, crop and normalisation run on the
device in one launch per batch (simseg_amd.preproc; bit-identical to the host transforms, so the histogram digest printed next to the
mIoU is the same on both routes).  `--synthetic-raw H1xW1,...` makes seeded raw uint8 images and raw-size labels for runs without a
dataset; without `--device-preproc` they go through PIL + build_transforms on the host:

    python tools/seg_eval_device.py --cfg configs/clip/simseg.vit-b.yaml --synthetic 2048 --synthetic-raw 375x500,500x375,333x500 \
        --device-preproc transforms.input_size=512 transforms.resize.size=512

`--scales S1,S2,...` and `--flip` add multi-scale / horizontal-flip test-time augmentation to `--slide` with `--device-preproc`: per batch one
device resize per scale (1.0 = the config's own valid transform, which defines the base size (H, W); the others resize the raw image to
max(1, floor(s H + 0.5)) x max(1, floor(s W + 0.5)), bilinear), every pass cut into the same windows, mirrored passes cut from the mirrored
image, and the passes' pixel-resolution maps fused on the device before candidate selection (segpost.encode_images_multiscale; DESIGN.md
"Multi-scale and flip test-time augmentation").  1.0 must be among the scales:

    python tools/seg_eval_device.py --cfg configs/clip/simseg.vit-b.yaml --ckpt_path ckpts/simseg.vit-b.pth --slide 512,256 --device-preproc \
        --scales 0.75,1.0,1.25 --flip transforms.input_size=512 transforms.valid_transforms=[resize_bicubic] data.valid_name=[coco_stuff]
"""
import argparse
import hashlib
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args():
    ap = argparse.ArgumentParser(description="SimSeg zero-shot segmentation evaluation (device post-processing)")
    ap.add_argument("--cfg", required=True)
    ap.add_argument("--local_rank", "--local-rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)))      # (torch.distributed.run sets LOCAL_RANK; torch.distributed.launch passes the flag)
    ap.add_argument("--ckpt_path", default="")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate N synthetic images with random weights")
    ap.add_argument("--no-crf", action="store_true", help="skip the DenseCRF (binary map = its unary decision)")
    ap.add_argument("--host-crf", action="store_true", help="DenseCRF with pydensecrf on the host instead of the device kernels")
    ap.add_argument("--slide", default="", help="WIN,STRIDE: sliding-window evaluation (BASELINE configs[3]): images are fed at their loader size, cut into "
                                                "WIN-pixel windows at STRIDE, per-window similarity maps overlap-averaged (segpost.encode_batch_sliding); "
                                                "transforms.input_size must be WIN; images of any size (see the module docstring)")
    ap.add_argument("--synthetic-sizes", default="", help="H1xW1,H2xW2,...: sizes of the synthetic images, cycled over them (with --slide)")
    ap.add_argument("--device-preproc", action="store_true", help="resize / crop / normalise on the device from raw uint8 images (simseg_amd.preproc) "
                                                                  "instead of PIL + torch on the host; same results bit for bit")
    ap.add_argument("--synthetic-raw", default="", help="H1xW1,H2xW2,...: sizes of seeded synthetic RAW uint8 images (and their labels), cycled over "
                                                        "them and sent through the config's valid transforms on the host or, with --device-preproc, on the device")
    ap.add_argument("--scales", default="", help="S1,S2,...: multi-scale test-time augmentation (needs --slide and --device-preproc; 1.0 must be among them)")
    ap.add_argument("--flip", action="store_true", help="add a horizontally mirrored pass per scale (needs --slide and --device-preproc)")
    ap.add_argument("--refine", choices=("crf", "pamr"), default="crf", help="the refinement between the normalised maps and the morphology: the reference's "
                                                                             "DenseCRF, or PAMR (pixel-adaptive mask refinement, segpost.pamr_masks)")
    ap.add_argument("--pamr-iters", type=int, default=None, help="PAMR propagation steps (default 10)")
    ap.add_argument("--pamr-dilations", default="", help="d1,d2,...: PAMR dilations (default 1,2,4,8,12,24)")
    args, rest = ap.parse_known_args()
    try:
        args.refiner = refiner_option(args)
    except ValueError as e:
        ap.error(str(e))
    return args, rest


def refiner_option(args):
    """--refine / --pamr-iters / --pamr-dilations -> the `refiner` keyword of segpost (None = the DenseCRF); ValueError with the reason when
    they do not fit the other options."""
    given = args.pamr_iters is not None or bool(args.pamr_dilations)
    if args.refine != "pamr":
        if given:
            raise ValueError("--pamr-iters / --pamr-dilations need --refine pamr")
        return None
    if args.no_crf or args.host_crf:
        raise ValueError("--refine pamr replaces the DenseCRF: it cannot be combined with --no-crf or --host-crf")
    params = {}
    if args.pamr_iters is not None:
        params["iters"] = args.pamr_iters
    if args.pamr_dilations:
        try:
            params["dilations"] = tuple(int(v) for v in args.pamr_dilations.split(","))
        except ValueError:
            raise ValueError(f"--pamr-dilations takes comma-separated integers, got {args.pamr_dilations!r}")
    from simseg_amd import ops
    ops.pamr_check(params.get("dilations", ops.PAMR_DILATIONS), params.get("iters", 10))
    return ("pamr", params)


def tta_options(args):
    """--scales / --flip -> (scales or None, flip); SystemExit with the reason when they do not fit the other options."""
    if not args.scales and not args.flip:
        return None, False
    if not args.slide or not args.device_preproc:
        raise SystemExit("--scales / --flip need --slide WIN,STRIDE and --device-preproc (the passes are resized on the device and fused over sliding windows)")
    try:
        scales = [float(v) for v in args.scales.split(",")] if args.scales else [1.0]
    except ValueError:
        raise SystemExit(f"--scales takes comma-separated numbers, got {args.scales!r}")
    if any(not (v > 0 and v < float("inf")) for v in scales) or len(set(scales)) != len(scales):
        raise SystemExit(f"--scales takes distinct positive numbers, got {args.scales!r}")
    if 1.0 not in scales:
        raise SystemExit(f"--scales must contain 1.0 (the base pass defines the output size), got {args.scales!r}")
    if len(scales) * (2 if args.flip else 1) > 16:
        raise SystemExit(f"--scales / --flip: {len(scales) * (2 if args.flip else 1)} passes, at most 16 are fused in one call")
    return scales, bool(args.flip)


def host_crf_refine(images_uint8):
    import numpy as np
    import pydensecrf.densecrf as dcrf

    def refine(prob, cand_idx, cand_score):
        B, K, H, W = prob.shape
        out = torch.zeros(B, K, H, W, dtype=torch.uint8)
        p = prob.cpu().numpy()
        for b in range(B):
            for k in range(K):
                if int(cand_idx[b, k]) < 0:
                    continue
                probs = np.stack([1 - p[b, k], p[b, k]])
                d = dcrf.DenseCRF2D(W, H, 2)
                d.setUnaryEnergy(np.ascontiguousarray(-np.log(probs + 1e-8).reshape(2, -1).astype(np.float32)))
                d.addPairwiseGaussian(sxy=3, compat=3)
                d.addPairwiseBilateral(sxy=40, srgb=13, rgbim=np.ascontiguousarray(images_uint8[b]), compat=10)
                q = np.argmax(np.array(d.inference(3)), axis=0).reshape(H, W)
                out[b, k] = torch.from_numpy((q * 255).astype(np.uint8))
        return out.to(prob.device)
    return refine


def main():
    args, overrides = parse_args()
    tta_scales, tta_flip = tta_options(args)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29511")
    os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
    from simseg.core import cfg, init_device, update_cfg
    from simseg.core.hooks.checkpoint import get_dist_state_dict
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import ENV, build_from_cfg, interpolate_pos_embed, logger
    from simseg.utils.prompt import openai_imagenet_template
    from simseg_amd import ops, segpost
    from simseg_amd.heads import class_text_embeddings, patch_text_similarity

    if args.synthetic:
        overrides = list(overrides) + ["model.image_encoder.pretrained=False", "model.text_encoder.pretrained=False"]
    update_cfg(task_cfg_init_fn, args.cfg, overrides, preprocess_fn=update_clip_config)
    ENV.cfg, ENV.local_rank = cfg, args.local_rank
    init_device(cfg)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE).to(ENV.device).eval()
    if args.ckpt_path:
        sd = torch.load(args.ckpt_path, map_location="cpu")["state_dict"]
        key = "image_encoder.model.model.pos_embed"
        if key in sd:
            sd[key] = interpolate_pos_embed(sd[key], model.image_encoder.model.model)
        model.load_state_dict(get_dist_state_dict(sd), strict=False)
        logger.emph(f"Loaded ckpt path: {args.ckpt_path}")
    size = cfg.transforms.input_size
    n = size // 16

    def text_matrix(categories):
        if args.synthetic:
            g = torch.Generator().manual_seed(3)
            return torch.nn.functional.normalize(torch.randn(len(categories), 512, generator=g), dim=-1).to(ENV.device)
        from transformers import AutoTokenizer
        tok = AutoTokenizer.from_pretrained(os.environ.get("SIMSEG_TOKENIZER_DIR", cfg.model.text_encoder.tag))
        prompts = [openai_imagenet_template(c) for c in categories]
        enc = tok([t for ts in prompts for t in ts], padding="max_length", truncation=True, max_length=25, return_tensors="pt")
        C, P = len(categories), len(prompts[0])
        with torch.no_grad():
            return class_text_embeddings(model, enc["input_ids"].view(C, P, -1).to(ENV.device), enc["attention_mask"].view(C, P, -1).to(ENV.device))

    def _emit_group(group):
        if all(l.shape == group[0][1].shape and i.shape == group[0][0].shape for i, l in group):
            yield torch.cat([i for i, _ in group]), torch.cat([l for _, l in group])
        else:
            for i, l in group:
                yield i, l

    slide = tuple(int(v) for v in args.slide.split(",")) if args.slide else None
    syn_sizes = [tuple(int(v) for v in s.split("x")) for s in args.synthetic_sizes.split(",")] if args.synthetic_sizes else None
    if syn_sizes and not slide:
        raise SystemExit("--synthetic-sizes needs --slide WIN,STRIDE (images of other sizes go through sliding windows)")

    def _tiles(hw):
        try:
            segpost.window_grid(int(hw[0]), int(hw[1]), *slide)
            return True
        except ValueError:
            return False

    def _emit_slide(group):
        """--slide: `--batch` one-image items -> one batch; tensors when they share one size that the windows tile exactly (the existing
        route), else lists of [3,H,W] images and [Hl,Wl] labels (segpost.encode_images_sliding)."""
        if len({(tuple(i.shape), tuple(l.shape)) for i, l in group}) == 1 and _tiles(group[0][0].shape[-2:]):
            yield torch.cat([i for i, _ in group]), torch.cat([l for _, l in group])
        else:
            yield [i[0] for i, _ in group], [l[0] for _, l in group]

    raw_sizes = [tuple(int(v) for v in s.split("x")) for s in args.synthetic_raw.split(",")] if args.synthetic_raw else None
    if raw_sizes and not args.synthetic:
        raise SystemExit("--synthetic-raw needs --synthetic N")
    if args.device_preproc and args.synthetic and not raw_sizes:
        raise SystemExit("--device-preproc with --synthetic needs --synthetic-raw H1xW1,... (raw images to preprocess)")
    if args.device_preproc and args.host_crf and not args.no_crf:
        raise SystemExit("--device-preproc is not wired to --host-crf")
    preprocess = None
    if args.device_preproc:
        from simseg.transforms import build_device_transforms
        from simseg_amd import preproc
        _, spec = build_device_transforms(cfg, "valid")

        def preprocess(raws):
            return preproc.preprocess(raws, spec, device=ENV.device)

        if tta_scales:
            if spec["crop"] is not None:
                raise SystemExit("--scales / --flip: the valid transform ends in a centre crop; test-time augmentation takes the whole resized image")
            one_pass = preprocess

            def preprocess(raws):
                """One device resize per scale: the base pass through the config's transform, the others to tta_sizes of its extents."""
                res = one_pass(raws)
                passes, src = [], None
                for s, target in zip(tta_scales, segpost.tta_sizes(res["sizes"], tta_scales)):
                    if s == 1.0:
                        packed, sizes = res["packed"], res["sizes"]
                        res["base"] = len(passes)
                    else:
                        scaled = preproc.preprocess_extents(raws, target, spec, device=ENV.device, src=src)
                        packed, sizes, src = scaled["packed"], scaled["sizes"], scaled["src"]
                    passes.append((packed, sizes, False))
                    if tta_flip:
                        passes.append((packed, sizes, True))
                res["passes"] = passes
                return res

    def raw_batches(shard):
        """--synthetic-raw: seeded raw uint8 [H, W, 3] images with raw-size labels, `--batch` per batch.  Device route: the raw lists as they
        are.  Host route: Image.fromarray + build_transforms(cfg, "valid") per image, stacked when the plain route takes them."""
        import numpy as np
        from PIL import Image
        from simseg.transforms import build_transforms
        tf = None if args.device_preproc else build_transforms(cfg, "valid")
        pool = {}

        def raw_item(j):
            # (a pool of 8 distinct images per size, made once: generating pixels is not part of either route)
            k = j % (8 * len(raw_sizes))
            if k not in pool:
                H, W = raw_sizes[k % len(raw_sizes)]
                rng = np.random.default_rng(1000 + k)
                # smooth colour fields plus noise: something for the resampling filters to do
                yy, xx = np.mgrid[0:H, 0:W]
                base = np.stack([128 + 100 * np.sin(yy / (7.0 + c) + k) * np.cos(xx / (11.0 - c)) for c in range(3)], -1)
                pool[k] = (np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8), torch.from_numpy(rng.integers(0, 21, (H, W), dtype=np.uint8)))
            return pool[k]
        for i, s in enumerate(range(0, args.synthetic, args.batch)):
            if shard is not None and i % shard[1] != shard[0]:
                continue
            imgs, labs = [], []
            for j in range(s, min(s + args.batch, args.synthetic)):
                raw, lab = raw_item(j)
                labs.append(lab)
                imgs.append(torch.from_numpy(raw) if tf is None else tf(Image.fromarray(raw)))
            if tf is None or slide:
                yield imgs, labs
            else:
                yield torch.stack(imgs), labs

    def device_loader_batches(name, shard):
        """--device-preproc on a dataset: the loader only decodes; `--batch` consecutive raw images and labels per batch, as lists."""
        from simseg.datasets.seg.seg_dataset import build_torch_valid_loader
        loader = build_torch_valid_loader(cfg, name, mode="valid", device_preproc=True)
        if shard is not None and shard[1] > 1:
            ds = loader.dataset
            idx = [i for i in range(len(ds)) if (i // args.batch) % shard[1] == shard[0]]
            loader = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, idx), batch_size=1, shuffle=False, num_workers=getattr(loader, "num_workers", 0),
                                                 collate_fn=loader.collate_fn)
        imgs, labs = [], []
        for image, label in loader:
            imgs += list(image); labs += [l.to(torch.uint8) for l in label]
            while len(imgs) >= args.batch:
                yield imgs[:args.batch], labs[:args.batch]
                imgs, labs = imgs[args.batch:], labs[args.batch:]
        if imgs:
            yield imgs, labs

    def batches(name, shard=None):
        """shard = (rank, world): only THIS rank's batches are produced (batch i goes to rank i % world - evaluate_sharded's rule), i.e. a
        rank decodes and transforms 1 / world of the images instead of all of them (the reference's loader gives every rank every image,
        simseg/datasets/seg/seg_dataset.py:67-81).  Batches are formed from `--batch` consecutive dataset items; an item whose label shape
        differs from its batch's ends the batch early in the unsharded form only - the sharded form cuts fixed groups of `--batch` items and
        splits a group with mixed shapes into single-image batches."""
        if args.synthetic and raw_sizes:
            yield from raw_batches(shard)
            return
        if args.device_preproc:
            yield from device_loader_batches(name, shard)
            return
        if args.synthetic and syn_sizes:
            g = torch.Generator().manual_seed(1)
            for i, s in enumerate(range(0, args.synthetic, args.batch)):
                group = []
                for j in range(s, min(s + args.batch, args.synthetic)):
                    hw = syn_sizes[j % len(syn_sizes)]
                    group.append((torch.randn(1, 3, *hw, generator=g), torch.randint(0, 21, (1, *hw), generator=g, dtype=torch.int64).to(torch.uint8)))
                if shard is None or i % shard[1] == shard[0]:
                    yield from _emit_slide(group)
            return
        if args.synthetic:
            g = torch.Generator().manual_seed(1)
            for i, s in enumerate(range(0, args.synthetic, args.batch)):
                b = min(args.batch, args.synthetic - s)
                hw = (size, 2 * size) if args.slide else (size, size)        # sliding window: 1 x 3 windows at half-window stride
                lab = torch.randint(0, 21, (b, *hw), generator=g, dtype=torch.int64).to(torch.uint8)
                img = torch.randn(b, 3, *hw, generator=g)
                if shard is None or i % shard[1] == shard[0]:
                    yield img, lab
            return
        from simseg.datasets.seg.seg_dataset import build_torch_valid_loader
        loader = build_torch_valid_loader(cfg, name, mode="valid")
        if slide and cfg.data.batch_size_val != 1:
            raise SystemExit(f"--slide needs one image per loader batch (images of different sizes cannot be collated): "
                             f"set data.batch_size_val=1 (got {cfg.data.batch_size_val})")
        if shard is not None and shard[1] > 1:
            # the same loader over a Subset holding this rank's groups of `--batch` consecutive items
            ds = loader.dataset
            idx = [i for i in range(len(ds)) if (i // args.batch) % shard[1] == shard[0]]
            loader = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, idx), batch_size=1, shuffle=False, num_workers=getattr(loader, "num_workers", 0),
                                                 collate_fn=loader.collate_fn)
            group = []
            for image, label in loader:
                group.append((image, label.to(torch.uint8)))
                if len(group) == args.batch:
                    yield from (_emit_slide(group) if slide else _emit_group(group))
                    group = []
            if group:
                yield from (_emit_slide(group) if slide else _emit_group(group))
            return
        if slide:
            group = []
            for image, label in loader:
                group.append((image, label.to(torch.uint8)))
                if len(group) == args.batch:
                    yield from _emit_slide(group)
                    group = []
            if group:
                yield from _emit_slide(group)
            return
        imgs, labs = [], []
        for image, label in loader:                       # reference loader: batch size 1, labels at raw resolution
            imgs.append(image); labs.append(label.to(torch.uint8))
            same = all(l.shape == labs[0].shape for l in labs)
            if len(imgs) == args.batch or not same:
                keep = len(imgs) if same else len(imgs) - 1
                yield torch.cat(imgs[:keep]), torch.cat(labs[:keep])
                imgs, labs = imgs[keep:], labs[keep:]
        if imgs:
            yield torch.cat(imgs), torch.cat(labs)

    names = ["synthetic"] if args.synthetic else list(cfg.data.valid_name)
    for name in names:
        if args.synthetic:
            cats = [f"class{i}" for i in range(21)]
        else:
            with open(f"data/label_category/{name}.txt") as f:
                cats = [ln.strip() for ln in f]
        top_cls_num = 30 if name == "pascal_context" else 10
        text = text_matrix(cats)
        hist = torch.zeros(3, len(cats), device=ENV.device, dtype=torch.int64)
        mean = torch.tensor(cfg.transforms.normalize.mean, device=ENV.device).view(1, 3, 1, 1)
        std = torch.tensor(cfg.transforms.normalize.std, device=ENV.device).view(1, 3, 1, 1)
        count, t0 = 0, time.perf_counter()
        # two batches in flight on two HIP streams, the next batch's encoder enqueued before the previous batch is finished
        # (segpost.EvalPipeline: the CRF stage's host read and its Python launch loop run under queued MFMA work); the histograms
        # accumulate atomically, so no ordering between batches is needed
        def encode(image, label):
            refine = None
            if args.host_crf and not args.no_crf:
                refine = host_crf_refine((((image * std) + mean) * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy())
            # (the de-normalised input is what the tool hands to dense_crf, tools/seg_evaluation.py:104)
            st = segpost.encode_batch(model, image, text, top_cls_num, crf=not args.no_crf, mean=mean, std=std, refine=refine)
            st["refine"] = refine
            return st

        def finish(st, image, label):
            return segpost.finish_batch(st, label, hist=hist, refine=st["refine"])

        if args.host_crf and not args.no_crf:
            pipe = segpost.EvalPipeline(ENV.device, encode, finish, pipelined=True)
            with torch.no_grad():
                for image, label in batches(name):
                    image, label = image.to(ENV.device), label.to(ENV.device)
                    pipe.submit(image, label)
                    count += image.shape[0]
                pipe.flush()
            torch.cuda.synchronize()
            iou, miou = segpost.iou_from_hist(hist)
        else:
            # the product loop: batches dealt round-robin to the ranks of the process group (one rank when launched plainly; N under
            # `python -m torch.distributed.run --nproc-per-node N tools/seg_eval_device.py ...`), ONE all-reduce of the [3, C] area histograms
            # (each rank's loader produces only its own batches; evaluate_sharded then sees a one-rank deal of them and still ends with the
            #  all-reduce of the histograms over the world)
            on = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
            shard = (dist.get_rank(), dist.get_world_size()) if on else None
            res = segpost.evaluate_sharded(model, batches(name, shard), text, top_cls_num, slide=slide, crf=not args.no_crf, mean=mean, std=std,
                                           device=ENV.device, presharded=on, preprocess=preprocess, refiner=args.refiner)
            torch.cuda.synchronize()
            iou, miou, count, hist = res["iou"], res["miou"], res["images"], res["hist"]
        dt = time.perf_counter() - t0
        print(f"---------------- {count} samples evaluated ({name}, {count / dt:.1f} images/s). ----------------")
        logger.emph("multi class iou:", iou)
        logger.emph("final mean iou:", miou)
        print(f"histogram sha256 {hashlib.sha256(hist.cpu().numpy().tobytes()).hexdigest()} mean iou {float(miou)!r} "
              f"({'device' if args.device_preproc else 'host'} preprocessing)")


if __name__ == "__main__":
    main()
