"""Per-image body of the reference's `evaluate_benchmark` (tools/seg_evaluation.py:99-170) as batched device work.

    feats  = model.forward_image_feature(image)              # [B, n*n, D]
    pooled = model.forward_image_project(feats)              # [B, 512]
    sim    = patch_text_similarity(model.image_projection(feats), text)      # [B, n*n, C]   (K14)
    out    = segment(sim, pooled @ text.T, labels, n, top_cls_num)

Between the normalised map and the morphology the reference runs a fully connected CRF on the CPU for every visited candidate
(pydensecrf, :31-54 / :153).  Here it is `ops.dense_crf` - mean-field inference on two permutohedral lattices built on the device -
when the caller hands over the de-normalised network inputs (`images_u8`, what the tool builds at :104); without them the binary
map is the CRF's unary decision (prob > 0.5), and a caller-supplied `refine` hook can replace either.  `refiner="pamr"` runs PAMR
(`ops.pamr`, pixel-adaptive mask refinement: no lattice, no host read) in the CRF's place; the reference has none.  Everything after it (7x7
dilate + erode, nearest resize, score-weighted argmax, IoU histograms) is the reference's arithmetic again.
"""
import os

import torch

from . import ops


CRF_PARAMS = dict(sxy_g=3.0, compat_g=3.0, sxy_b=40.0, srgb=13.0, compat_b=10.0, iters=3)        # tools/seg_evaluation.py:48-51


def crf_masks(prob, cand_idx, images_u8, chunk=None, scale=1, static=None, **params):
    """prob [B,K,h,w] fp32 normalised candidate maps (at 1/scale of the image resolution: the x16 nearest upsampling of the tool,
    tools/seg_evaluation.py:141-143, is applied here per chunk and only to visited slots), cand_idx [B,K] (-1 = slot not visited),
    images_u8 [B,H,W,3] -> uint8 masks [B,K,H,W] (0/255; unvisited slots zero).  One host read of the candidate table per batch (the
    reference loops on the host per image and candidate); images with a visited candidate go through the device CRF `chunk` at a time
    (an image's candidates share its lattices; images are grouped by their number of visited candidates, so chunks carry few idle maps).
    Per chunk: one gather of the visited low-resolution maps, one upsampling, one CRF call, one scatter of the masks."""
    B, K, h, w = prob.shape
    H, W = h * scale, w * scale
    dev = prob.device
    if static is None:
        static = os.environ.get("SIMSEG_CRF_STATIC", "0") != "0"
    if static:
        # Sync-free form (opt-in): no host read and no data-dependent shapes - every image goes through the CRF in ONE call with all K
        # candidate slots as channels; slots the reference never visits carry the all-zero map seg_masks leaves there and their result is
        # dropped.  K = 5 channels instead of the ~2 visited maps per image: measured 55.6 vs 28.4 ms per 63-window batch of 512^2
        # (round 3), so the chunked form below stays the default.  (Replaying the CRF inside a hipGraph is NOT supported: a first
        # attempt hung in replay - the hash build's probe loops never terminate if a table memset is not replayed - and was not pursued.)
        up = prob if scale == 1 else prob.repeat_interleave(scale, 2).repeat_interleave(scale, 3)
        m, _ = ops.dense_crf(images_u8.contiguous(), up.contiguous(), **dict(CRF_PARAMS, **params))
        return m * (cand_idx >= 0).to(torch.uint8)[:, :, None, None]
    if chunk is None:
        # images per call: ~16.7 M pixels (64 windows of 512^2, 32 images of 512 x 1024; 17.7 GB of workspace).  Round 5, after the lattice
        # build became cheaper per image: 16 / 32 / 64 windows of 512^2 per call = 20.7 / 19.9 / 19.1 ms per 63-window batch
        chunk = int(os.environ.get("SIMSEG_CRF_CHUNK", "0"))
        if not chunk:
            # ... bounded by what the device has FREE: the workspace is ~1.06 KB per pixel and call (17.7 GB at 16.7 M pixels), the encoder
            # pipeline keeps two batches in flight beside it, and a 2048^2 source image alone is 4.2 M pixels - so no floor above one image
            budget = 1 << 24
            if dev.type == "cuda":
                try:
                    free, _ = torch.cuda.mem_get_info(dev)
                    budget = min(budget, int(0.5 * free / 1100))
                except Exception:       # noqa: BLE001
                    pass
            chunk = max(1, min(128, budget // (H * W)))
    masks = torch.zeros(B, K, H, W, device=dev, dtype=torch.uint8)
    visited = (cand_idx >= 0).cpu()
    kw = dict(CRF_PARAMS, **params)
    todo = [(b, visited[b].nonzero().flatten().tolist()) for b in range(B)]
    todo = sorted(((b, ks) for b, ks in todo if ks), key=lambda t: len(t[1]))      # chunks of equal width: no idle zero maps
    for s in range(0, len(todo), chunk):
        part = todo[s:s + chunk]
        cmax = max(len(ks) for _, ks in part)
        slot = torch.full((len(part), cmax), -1, dtype=torch.int64)
        for j, (_, ks) in enumerate(part):
            slot[j, :len(ks)] = torch.tensor(ks)
        valid = (slot >= 0).to(dev)
        bsel = torch.tensor([b for b, _ in part], device=dev)
        ksel = slot.clamp(min=0).to(dev)                           # idle slots repeat a visited map (their result is dropped)
        lo = prob[bsel[:, None], ksel]                             # [n, cmax, h, w]
        up = lo if scale == 1 else lo.repeat_interleave(scale, 2).repeat_interleave(scale, 3)
        m, _ = ops.dense_crf(images_u8[bsel].contiguous(), up.contiguous(), **kw)
        masks[bsel[:, None].expand(-1, cmax)[valid], ksel[valid]] = m[valid]
    return masks


PAMR_PARAMS = dict(dilations=(1, 2, 4, 8, 12, 24), iters=10)


def pamr_masks(prob, cand_idx, images_u8, scale=1, chunk=None, **params):
    """crf_masks() with PAMR (ops.pamr) in the DenseCRF's place: prob [B,K,h,w] fp32 normalised candidate maps at 1/scale of the image
    resolution (read through (y / scale, x / scale) by the first iteration: the upsampled maps never exist), cand_idx [B,K] (-1 = slot not
    visited), images_u8 [B,H,W,3] -> uint8 masks [B,K,H,W] (0/255; unvisited slots zero).  No host read and no per-image loop: unvisited
    slots are skipped inside the kernels, `chunk` images per call.  chunk = None: from the shapes and the device's free memory only -
    the workspace is 4 * 8 D + 8 K bytes per pixel (232 at the defaults), and memory the caching allocator holds but has not handed out
    counts as free.  A pixel's result does not depend on the chunking."""
    B, K, h, w = prob.shape
    H, W = h * scale, w * scale
    kw = dict(PAMR_PARAMS, **params)
    dil = ops.pamr_check(kw["dilations"], kw["iters"], K, scale)
    if chunk is None:
        chunk = B
        if prob.device.type == "cuda":
            per_pixel = 4 * 8 * len(dil) + 8 * K + K                                  # workspace + the masks
            held = ops._PAMR_WS.get((prob.device, torch.cuda.current_stream().cuda_stream))
            free, _ = torch.cuda.mem_get_info(prob.device)
            free += torch.cuda.memory_reserved(prob.device) - torch.cuda.memory_allocated(prob.device) + (held.numel() if held is not None else 0)
            chunk = int(0.5 * free / per_pixel) // (H * W)
    chunk = max(1, min(B, int(chunk)))
    cand_idx, images_u8, prob = cand_idx.contiguous(), images_u8.contiguous(), prob.contiguous()
    if chunk >= B:
        return ops.pamr(images_u8, prob, cand_idx, scale=scale, **kw)[0]
    masks = torch.empty(B, K, H, W, device=prob.device, dtype=torch.uint8)
    for s in range(0, B, chunk):
        masks[s:s + chunk] = ops.pamr(images_u8[s:s + chunk], prob[s:s + chunk], cand_idx[s:s + chunk], scale=scale, **kw)[0]
    return masks


def parse_refiner(refiner, crf=True):
    """The `refiner` keyword of the encode_* / eval functions: None or "crf" -> None (the DenseCRF under crf=True: the default);
    "pamr" or ("pamr", {parameters of pamr_masks}) -> ("pamr", {checked parameters}).  PAMR needs the images, so crf=False with it is an
    error."""
    if refiner is None or refiner == "crf":
        return None
    pair = (refiner, {}) if isinstance(refiner, str) else tuple(refiner) if isinstance(refiner, (tuple, list)) else ()
    if len(pair) != 2 or pair[0] != "pamr" or not isinstance(pair[1], dict):
        raise ValueError(f'refiner: None, "crf", "pamr" or ("pamr", {{parameters}}) expected, got {refiner!r}')
    params = dict(pair[1])
    unknown = set(params) - {"dilations", "iters", "chunk"}
    if unknown:
        raise ValueError(f"refiner: unknown PAMR parameters {sorted(unknown)}")
    kw = dict(PAMR_PARAMS, **params)
    ops.pamr_check(kw["dilations"], kw["iters"])
    if not crf:
        raise ValueError('refiner="pamr" refines the maps with the images: it cannot be combined with crf=False')
    return ("pamr", params)


def refine_masks(prob, cand_idx, images_u8, scale, refiner=None):
    """The refinement stage of a state: the DenseCRF, or what parse_refiner() stored."""
    if refiner is None:
        return crf_masks(prob, cand_idx, images_u8, scale=scale)
    return pamr_masks(prob, cand_idx, images_u8, scale=scale, **refiner[1])


def segment_begin(sim, scores, num_patch, top_cls_num, ncand=5, need_prob=False):
    """First half of segment(): candidate selection and the per-candidate min-max maps - device work only, nothing is read back."""
    cand_idx, cand_score, thr = ops.seg_select(scores, top_cls_num, ncand)
    masks, prob = ops.seg_masks(sim, cand_idx, num_patch, want_prob=need_prob)
    return {"cand_idx": cand_idx, "cand_score": cand_score, "threshold": thr, "masks": masks, "prob": prob, "num_patch": num_patch,
            "num_classes": sim.shape[2]}


def segment_finish(st, labels, num_classes=None, ignore_index=255, refine=None, hist=None, want_pred=True, closing=True, images_u8=None):
    """Second half of segment(): DenseCRF (ONE host read of the candidate table) - or PAMR where the state says so (st["refiner"],
    parse_refiner) - closing, resize + argmax + IoU histograms."""
    cand_idx, cand_score, masks, prob, num_patch = st["cand_idx"], st["cand_score"], st["masks"], st["prob"], st["num_patch"]
    num_classes = num_classes or st["num_classes"]
    if refine is not None or images_u8 is not None:
        B, K, N = prob.shape
        nh, nw = (num_patch, num_patch) if isinstance(num_patch, int) else num_patch
        lo = prob.view(B, K, nh, nw)
        if refine is not None:
            up = lo.repeat_interleave(16, 2).repeat_interleave(16, 3)
            masks = refine(up, cand_idx, cand_score).to(torch.uint8).contiguous()
        else:
            masks = refine_masks(lo, cand_idx, images_u8, 16, st.get("refiner"))
    if closing:
        masks = ops.close7(masks, cand_idx.reshape(-1))                       # cv2.dilate then cv2.erode (:156-157), visited slots only
    pred, hist = ops.seg_predict(masks, cand_idx, cand_score, labels, num_classes, ignore_index, hist=hist, want_pred=want_pred)
    return {"pred": pred, "hist": hist, "cand_idx": cand_idx, "cand_score": cand_score, "threshold": st["threshold"], "masks": masks}


def segment(sim, scores, labels, num_patch, top_cls_num, num_classes=None, ncand=5, ignore_index=255, refine=None, hist=None,
            want_pred=True, closing=True, images_u8=None):
    """sim [B,n*n,C] fp32, scores [B,C], labels [B,H,W] uint8 -> dict(pred, hist, cand_idx, cand_score, threshold).
    images_u8 [B,16n,16n,3] uint8 (RGB): run the reference's DenseCRF on every visited candidate map."""
    st = segment_begin(sim, scores, num_patch, top_cls_num, ncand, need_prob=refine is not None or images_u8 is not None)
    return segment_finish(st, labels, num_classes or sim.shape[2], ignore_index, refine, hist, want_pred, closing, images_u8)


def encode_batch(model, image, text, top_cls_num, crf=True, mean=None, std=None, sim_dtype=None, refine=None, refiner=None):
    """Everything of eval_batch() up to the candidate maps: towers -> pooled embedding + projected patch tokens -> similarity map for all
    classes -> candidate selection + min-max maps.  Device work only (no host read): the caller may enqueue the NEXT batch's encoder
    before it finishes this one (EvalPipeline)."""
    from .heads import patch_text_similarity
    refiner = parse_refiner(refiner, crf)
    if refiner is not None and refine is not None:
        raise ValueError("encode_batch: a refine hook and refiner= are two answers to one question")
    feats = model.forward_image_feature(image)                    # [B, n*n, D]
    pooled = model.forward_image_project(feats)                   # [B, 512]
    n = int(round(feats.shape[1] ** 0.5))
    sim = patch_text_similarity(model.image_projection(feats), text, compute_dtype=sim_dtype)
    raw = None
    if crf and refine is None:
        raw = (((image * std) + mean) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    st = segment_begin(sim, ops.gemm(pooled.float(), text), n, top_cls_num, need_prob=refine is not None or raw is not None)
    st["images_u8"] = raw
    st["refiner"] = refiner
    return st


# ---- sliding-window evaluation (BASELINE configs[3]: "ViT-B zero-shot seg eval, COCO-Stuff-shaped 171 classes, slide-window 512x512") ----
# The reference tool resizes every image to ONE network input (tools/seg_evaluation.py:84-85,109); SURVEY.md 8d cfg 4 defines the
# sliding-window form this package adds: windows of `win` pixels at stride `stride` over the (larger) source image, each window through the
# towers as an image of its own, the per-window patch x class similarity maps overlap-AVERAGED on the source image's patch grid, and then the
# reference's per-image body (candidate classes, min-max, DenseCRF, 7x7 closing, resize, score-weighted argmax, IoU areas) ONCE per source
# image on the stitched map.  Image-level class scores (:112-123 works on the pooled embedding of the one resized image) are the mean of
# the windows' scores.  oracle/segpost_ref.py sliding_window_image() is the per-image loop this is tested against.

def window_grid(H, W, win=512, stride=256):
    """-> (wy, wx): windows per column / row.  The image must be tiled exactly: (H - win) and (W - win) multiples of the stride (the
    caller pads or resizes otherwise), win and stride multiples of the 16-pixel patch."""
    if win % 16 or stride % 16 or stride <= 0 or stride > win:
        raise ValueError(f"window_grid: win {win} and stride {stride} must be multiples of the 16-pixel patch with 0 < stride <= win")
    if H < win or W < win or (H - win) % stride or (W - win) % stride:
        raise ValueError(f"window_grid: a {H}x{W} image is not tiled exactly by {win}-pixel windows at stride {stride}")
    return (H - win) // stride + 1, (W - win) // stride + 1


def extract_windows(image, win=512, stride=256):
    """image [B,3,H,W] -> [B*wy*wx, 3, win, win]: an image's windows consecutive, row-major over its window grid (a strided copy)."""
    B, C, H, W = image.shape
    wy, wx = window_grid(H, W, win, stride)
    v = image.unfold(2, win, stride).unfold(3, win, stride)            # [B, C, wy, wx, win, win] view
    return v.permute(0, 2, 3, 1, 4, 5).reshape(B * wy * wx, C, win, win)


def encode_batch_sliding(model, image, text, top_cls_num, win=512, stride=256, crf=True, mean=None, std=None, sim_dtype=None, window_batch=None,
                         refiner=None):
    """encode_batch() for source images larger than the network input: image [B,3,H,W] -> B*wy*wx windows through the towers (at most
    `window_batch` windows per call), similarity maps stitched on the [H/16, W/16] patch grid (ops.stitch_windows), image-level scores =
    the mean of the windows' pooled scores -> candidate selection and min-max maps on the stitched grid.  Device work only."""
    from .heads import patch_text_similarity
    refiner = parse_refiner(refiner, crf)
    B, _, H, W = image.shape
    wy, wx = window_grid(H, W, win, stride)
    wins = extract_windows(image, win, stride)
    n = win // 16
    sims, scores = [], []
    wb = window_batch or wins.shape[0]
    for s in range(0, wins.shape[0], wb):
        feats = model.forward_image_feature(wins[s:s + wb])          # [b, n*n, D]
        pooled = model.forward_image_project(feats)                   # [b, 512]
        sims.append(patch_text_similarity(model.image_projection(feats), text, compute_dtype=sim_dtype))
        scores.append(ops.gemm(pooled.float(), text))
    sim_w = sims[0] if len(sims) == 1 else torch.cat(sims)
    sc_w = scores[0] if len(scores) == 1 else torch.cat(scores)
    sim = ops.stitch_windows(sim_w.float(), wy, wx, n, stride // 16)                       # [B, nh*nw, C]
    sc = ops.stitch_windows(sc_w.float().view(B * wy * wx, 1, -1), wy, wx, 1, 0).view(B, -1)      # mean over an image's windows
    raw = None
    if crf:
        raw = (((image * std) + mean) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    st = segment_begin(sim, sc, (H // 16, W // 16), top_cls_num, need_prob=raw is not None)
    st["images_u8"] = raw
    st["refiner"] = refiner
    st["windows"] = (wy, wx)
    return st


# ---- sliding windows on images of ANY size (DESIGN.md "Sliding windows on any image size") ----------------------------------------------
# Real evaluation images (COCO-Stuff ~640x480 resized to a short side of 512 -> 683x512) are not tiled exactly by 512-pixel windows at
# stride 256.  Windows are then placed as mmseg's slide_inference does (the last one flush with the border, one window at (0, 0) padded with
# zeros past the border of an image smaller than the window), the per-window maps are stitched at PIXEL resolution (the windows' offsets
# need not share a patch grid) and any number of images of different sizes go through the towers together.  Where window_grid() accepts
# an image the result is bit-identical to encode_batch_sliding + finish_batch.

def slide_windows(H, W, win=512, stride=256):
    """-> [(y0, x0), ...] row-major: ny = max(H - win + stride - 1, 0) // stride + 1 rows at y0(i) = min(i * stride, max(H - win, 0)), the
    same for x.  H, W any positive sizes; win and stride multiples of the 16-pixel patch with 0 < stride <= win."""
    if win % 16 or stride % 16 or stride <= 0 or stride > win or win <= 0:
        raise ValueError(f"slide_windows: win {win} and stride {stride} must be multiples of the 16-pixel patch with 0 < stride <= win")
    if H <= 0 or W <= 0:
        raise ValueError(f"slide_windows: a {H}x{W} image")

    def axis(L):
        return [min(i * stride, max(L - win, 0)) for i in range(max(L - win + stride - 1, 0) // stride + 1)]
    return [(y, x) for y in axis(H) for x in axis(W)]


def encode_images_sliding(model, images, text, top_cls_num, win=512, stride=256, crf=True, mean=None, std=None, sim_dtype=None, window_batch=None,
                          sizes=None, refiner=None):
    """encode_batch_sliding() for images of any sizes: images = a list of [3, H_i, W_i] normalised fp32 tensors (or one [B,3,H,W] tensor),
    or - with sizes = [(H_i, W_i), ...] - the flat fp32 buffer that already holds them back to back (what preproc.preprocess writes: taken
    as it is, nothing is concatenated).
    All windows of all images (slide_windows offsets, ops.slide_extract) go through the towers together, at most `window_batch` per call;
    image scores = the mean of an image's window scores (ops.slide_scores) -> candidate selection -> per visited slot the pixel-resolution
    stitched map, min-max normalised, and its binary map (ops.slide_stitch).  Device work only (no host read).  finish_sliding() ends it."""
    from .heads import patch_text_similarity
    refiner = parse_refiner(refiner, crf)
    if sizes is not None:
        sizes = [(int(h), int(w)) for h, w in sizes]
        flat = images.contiguous().reshape(-1)
        if flat.dtype != torch.float32 or flat.numel() != sum(3 * h * w for h, w in sizes):
            raise ValueError(f"encode_images_sliding: a packed fp32 buffer of {sum(3 * h * w for h, w in sizes)} elements expected for sizes {sizes}, "
                             f"got {flat.numel()} {flat.dtype}")
        groups, at = {}, 0
        for b, (h, w) in enumerate(sizes):
            bs, views = groups.setdefault((h, w), ([], []))
            bs.append(b)
            views.append(flat[at:at + 3 * h * w].view(3, h, w))
            at += 3 * h * w
        if crf:
            groups = {hw: (bs, v[0][None] if len(v) == 1 else torch.stack(v)) for hw, (bs, v) in groups.items()}
    elif torch.is_tensor(images):
        B, _, H, W = images.shape
        sizes, flat, groups = [(H, W)] * B, images.contiguous().reshape(-1), {(H, W): (list(range(B)), images)}
    else:
        images = [im.contiguous() for im in images]
        sizes = [(im.shape[1], im.shape[2]) for im in images]
        flat = images[0].reshape(-1) if len(images) == 1 else torch.cat([im.reshape(-1) for im in images])
        groups = {}
        for b, hw in enumerate(sizes):
            groups.setdefault(hw, ([], None))[0].append(b)
        groups = {hw: (bs, images[bs[0]][None] if len(bs) == 1 else torch.stack([images[b] for b in bs])) for hw, (bs, _) in groups.items()}
    plan = ops.slide_plan(sizes, win, stride, flat.device)
    Nw = len(plan["windows"])
    wb = window_batch or Nw
    sims, scores = [], []
    for s in range(0, Nw, wb):
        wins = ops.slide_extract(flat, plan, s, min(wb, Nw - s))
        feats = model.forward_image_feature(wins)                     # [b, n*n, D]
        pooled = model.forward_image_project(feats)                   # [b, 512]
        sims.append(patch_text_similarity(model.image_projection(feats), text, compute_dtype=sim_dtype))
        scores.append(ops.gemm(pooled.float(), text))
    sim_w = sims[0] if len(sims) == 1 else torch.cat(sims)
    sc_w = scores[0] if len(scores) == 1 else torch.cat(scores)
    sc = ops.slide_scores(sc_w.float().contiguous(), plan)
    cand_idx, cand_score, thr = ops.seg_select(sc, top_cls_num, plan["ncand"])
    prob, masks, minmax = ops.slide_stitch(sim_w.float().contiguous(), plan, cand_idx)
    raw = None
    if crf:
        # the de-normalised source images (tools/seg_evaluation.py:104), one [g, H, W, 3] tensor per image size
        raw = {hw: (bs, (((x * std) + mean) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()) for hw, (bs, x) in groups.items()}
    return {"cand_idx": cand_idx, "cand_score": cand_score, "threshold": thr, "scores": sc, "prob": prob, "masks": masks, "minmax": minmax,
            "plan": plan, "images_u8": raw, "num_classes": sim_w.shape[2], "refiner": refiner}


# ---- multi-scale and flip test-time augmentation (DESIGN.md "Multi-scale and flip test-time augmentation") ------------------------------
# The evaluation protocol that goes with sliding windows: the same image at several scales and mirrored, every pass cut into windows
# with the same win / stride, the passes' pixel-resolution maps fused on the device (ops.slide_stitch_multi) before candidate selection
# and post-processing.  The reference has no such protocol (as it has no sliding window); tests/_tta_ref.py restates it in numpy.

def tta_sizes(sizes, scales):
    """-> per scale s the list [(H_p, W_p)] with H_p = max(1, floor(s * H + 0.5)), W_p likewise, for base sizes [(H, W), ...]."""
    import math
    out = []
    for s in scales:
        s = float(s)
        if not s > 0 or not math.isfinite(s):
            raise ValueError(f"tta_sizes: scales are positive numbers, got {s!r}")
        out.append([(max(1, int(math.floor(s * int(H) + 0.5))), max(1, int(math.floor(s * int(W) + 0.5)))) for H, W in sizes])
    return out


def tta_nearest_index(i, L, Lp):
    """Row (column) of a pass of extent Lp that base row (column) i of extent L samples: nearest with pixel centres, integers only."""
    return min(((2 * i + 1) * Lp) // (2 * L), Lp - 1)


def encode_images_multiscale(model, passes, text, top_cls_num, win=512, stride=256, crf=True, mean=None, std=None, sim_dtype=None,
                             window_batch=None, base=0, refiner=None):
    """encode_images_sliding() with test-time augmentation.  passes = [(flat, sizes, flip), ...]: per pass the flat fp32 buffer that holds
    the batch's normalised [3, H_p, W_p] images back to back (what preproc.preprocess writes for that scale; NOT mirrored), their sizes,
    and whether the pass runs on the mirrored images (the mirror is taken while the windows are cut: ops.slide_extract_flip).
    passes[base] is the unflipped scale-1 pass: its sizes define the plan of the outputs and its pixels feed the CRF.  Every pass is cut
    into windows with the same win / stride and goes through the towers at most `window_batch` windows per call (passes are not mixed in
    a call).  Image scores: per pass the ops.slide_scores mean, summed over the passes in pass order in fp32 and divided once by their
    number; candidates from the fused scores; prob / masks / minmax from ops.slide_stitch_multi.  -> the dict of encode_images_sliding
    (plan = the base plan, scores = the fused scores): finish_sliding() ends it.  One pass (the base alone) gives encode_images_sliding's
    result bit for bit."""
    from .heads import patch_text_similarity
    refiner = parse_refiner(refiner, crf)
    P = len(passes)
    if P == 0 or not 0 <= base < P:
        raise ValueError(f"encode_images_multiscale: {P} passes, base index {base}")
    if passes[base][2]:
        raise ValueError("encode_images_multiscale: the base pass is the unflipped scale-1 pass")
    flats, plans, flips = [], [], []
    B = len(passes[base][1])
    for p, (buf, sizes, flip) in enumerate(passes):
        sizes = [(int(h), int(w)) for h, w in sizes]
        flat = buf.contiguous().reshape(-1)
        if len(sizes) != B:
            raise ValueError(f"encode_images_multiscale: pass {p} holds {len(sizes)} images, the base pass {B}")
        if flat.dtype != torch.float32 or flat.numel() != sum(3 * h * w for h, w in sizes):
            raise ValueError(f"encode_images_multiscale: pass {p}: a packed fp32 buffer of {sum(3 * h * w for h, w in sizes)} elements expected for "
                             f"sizes {sizes}, got {flat.numel()} {flat.dtype}")
        flats.append(flat); flips.append(bool(flip))
        plans.append(ops.slide_plan(sizes, win, stride, flat.device))
    plan = plans[base]
    sims, sc = [], None
    for flat, pl, flip in zip(flats, plans, flips):
        Nw = len(pl["windows"])
        wb = window_batch or Nw
        sim_p, sc_p = [], []
        for s in range(0, Nw, wb):
            wins = ops.slide_extract_flip(flat, pl, s, min(wb, Nw - s), flip=flip)
            feats = model.forward_image_feature(wins)                     # [b, n*n, D]
            pooled = model.forward_image_project(feats)                   # [b, 512]
            sim_p.append(patch_text_similarity(model.image_projection(feats), text, compute_dtype=sim_dtype))
            sc_p.append(ops.gemm(pooled.float(), text))
        sim_w = sim_p[0] if len(sim_p) == 1 else torch.cat(sim_p)
        sc_w = sc_p[0] if len(sc_p) == 1 else torch.cat(sc_p)
        sims.append(sim_w.float().contiguous())
        one = ops.slide_scores(sc_w.float().contiguous(), pl)
        sc = one if sc is None else sc + one
    if P > 1:
        sc = sc / float(P)
    cand_idx, cand_score, thr = ops.seg_select(sc, top_cls_num, plan["ncand"])
    prob, masks, minmax = ops.slide_stitch_multi(sims, plans, flips, plan, cand_idx)
    raw = None
    if crf:
        # the de-normalised base images (tools/seg_evaluation.py:104), one [g, H, W, 3] tensor per image size
        groups, at = {}, 0
        for b, (h, w) in enumerate(plan["sizes"]):
            bs, views = groups.setdefault((h, w), ([], []))
            bs.append(b)
            views.append(flats[base][at:at + 3 * h * w].view(3, h, w))
            at += 3 * h * w
        raw = {hw: (bs, (((x * std) + mean) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
               for hw, (bs, x) in ((hw, (bs, v[0][None] if len(v) == 1 else torch.stack(v))) for hw, (bs, v) in groups.items())}
    return {"cand_idx": cand_idx, "cand_score": cand_score, "threshold": thr, "scores": sc, "prob": prob, "masks": masks, "minmax": minmax,
            "plan": plan, "images_u8": raw, "num_classes": sims[0].shape[2], "refiner": refiner}


def _crf_cached_size(device):
    """(H, W) of the spatial lattice ops.dense_crf holds for the current stream, or None."""
    sig = ops._CRF_SPATIAL.get((device, torch.cuda.current_stream().cuda_stream))
    return None if sig is None else (sig[1], sig[2])


def finish_sliding(st, labels, hist=None, num_classes=None, ignore_index=255, want_pred=False, closing=True):
    """Second half of the any-size sliding-window evaluation: labels = a list of [Hl_i, Wl_i] uint8 tensors (or one [B,Hl,Wl] tensor).
    Images are grouped by (H, W, label shape); per group: DenseCRF on the full-resolution prob maps (crf_masks(..., scale=1)) when
    encode_images_sliding was given crf=True (PAMR, pamr_masks(..., scale=1), under refiner="pamr"), else the binary maps; 7x7 closing;
    nearest resize to the labels + score-weighted argmax + IoU histograms (ops.seg_predict, accumulated into `hist`).  Groups that share an image size run back to back, starting with the size
    whose spatial lattice the CRF holds, so that lattice is rebuilt once per size.
    -> dict(hist, cand_idx, cand_score, masks [per image: ncand x H x W uint8, after closing], pred [per image, or None])."""
    plan = st["plan"]
    sizes = plan["sizes"]
    C = num_classes or st["num_classes"]
    dev = st["cand_idx"].device
    if hist is None:
        hist = torch.zeros(3, C, device=dev, dtype=torch.int64)
    labels = list(labels) if torch.is_tensor(labels) else labels
    if len(labels) != len(sizes):
        raise ValueError(f"finish_sliding: {len(labels)} label maps for {len(sizes)} images")
    keys = {}
    for b, (hw, lab) in enumerate(zip(sizes, labels)):
        keys.setdefault(hw + tuple(lab.shape[-2:]), []).append(b)
    order = sorted(keys)
    raw = st.get("images_u8")
    refiner = st.get("refiner")
    if raw is not None and refiner is None:
        first = _crf_cached_size(dev)
        order.sort(key=lambda k: (k[:2] != first, k))
    out_masks, out_pred = [None] * len(sizes), [None] * len(sizes)

    def take(t, rows):            # rows of a device tensor: a view for a contiguous run, else a gather (index copied without a host wait)
        if rows == list(range(rows[0], rows[0] + len(rows))):
            return t[rows[0]:rows[0] + len(rows)]
        return t[ops.to_device_async(rows, dev)]

    for key in order:
        bs = keys[key]
        cand, score = take(st["cand_idx"], bs), take(st["cand_score"], bs)
        src = st["prob"] if raw is not None else st["masks"]
        planes = [ops.slide_planes(src, plan, b) for b in bs]
        maps = planes[0][None] if len(bs) == 1 else torch.stack(planes)
        if raw is not None:
            gb, u8 = raw[key[:2]]
            img = take(u8, [gb.index(b) for b in bs])
            maps = refine_masks(maps, cand, img, 1, refiner)
        if closing:
            maps = ops.close7(maps, cand.reshape(-1))
        lab = labels[bs[0]][None] if len(bs) == 1 else torch.stack([labels[b] for b in bs])
        pred, hist = ops.seg_predict(maps, cand, score, lab.contiguous(), C, ignore_index, hist=hist, want_pred=want_pred)
        for j, b in enumerate(bs):
            out_masks[b] = maps[j]
            if want_pred:
                out_pred[b] = pred[j]
    return {"hist": hist, "cand_idx": st["cand_idx"], "cand_score": st["cand_score"], "threshold": st["threshold"], "masks": out_masks,
            "pred": out_pred if want_pred else None}


def shard_batches(batches, rank, world):
    """Round-robin shard of an iterable of batches: rank r takes batches r, r + world, ... (independent units, no data-path collective)."""
    for i, b in enumerate(batches):
        if i % world == rank:
            yield b


def evaluate_sharded(model, batches, text, top_cls_num, num_classes=None, group=None, slide=None, crf=True, mean=None, std=None, sim_dtype=None,
                     device=None, pipelined=None, window_batch=None, presharded=False, preprocess=None, refiner=None):
    """The zero-shot segmentation evaluation over `batches` = an iterable of (image [b,3,H,W], label [b,Hl,Wl] uint8) - the SAME iterable on
    every rank - data-parallel over the ranks of `group` (default: the world, or a single process when torch.distributed is not
    initialised): batches are dealt round-robin (shard_batches; the reference's loader gives every rank every image,
    simseg/datasets/seg/seg_dataset.py:67-81), each rank accumulates its [3, C] area histograms on its device and ONE all-reduce(SUM) of that
    tensor ends the evaluation (simseg/utils/metrics.py:85-97 sums the same three vectors over the images).  Every rank still ITERATES the
    whole iterable (a batch it skips is produced and dropped): when producing a batch is expensive, hand in this rank's share only - a loader
    over a dataset sharded with the same i % world == rank rule - and say presharded=True (tools/seg_eval_device.py does).  slide = (win, stride): the
    sliding-window form (encode_batch_sliding); None: one network input per image (encode_batch).  A batch whose image and label elements are
    LISTS (images [3,H_i,W_i] of any sizes, labels [Hl_i,Wl_i]) takes the any-size sliding-window path (encode_images_sliding + finish_sliding).
    preprocess: a callable for batches whose image element is a list of RAW uint8 [H, W, 3] images (host or device): it turns the list into
    the network input - a [b,3,S,S] tensor, or the dict of simseg_amd.preproc.preprocess, whose packed buffer the any-size path takes as it
    is - and is called inside the encoder stage, on the encoder stream of EvalPipeline: the preprocessing kernel is queued with the batch it
    feeds and the raw bytes stay referenced as long as the batch does.  Labels of such a batch are a list ([Hl_i, Wl_i], any sizes).
    A preprocess that returns dict(passes=[(packed, sizes, flip), ...], base=index) with slide set takes the multi-scale / flip path
    (encode_images_multiscale).
    -> dict(iou [C] float64, miou, hist [3,C] int64 (global), images (global count), images_local)."""
    import torch.distributed as dist
    refiner = parse_refiner(refiner, crf)
    on = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if on else 0
    world = dist.get_world_size(group) if on else 1
    C = num_classes or text.shape[0]
    dev = torch.device(device) if device is not None else text.device
    hist = torch.zeros(3, C, device=dev, dtype=torch.int64)

    def encode(image, label):
        if preprocess is not None:
            res = preprocess(image)
            # (the state keeps what preprocess returned - packed buffer, plan, tables - referenced for as long as EvalPipeline keeps the batch)
            if isinstance(res, dict) and slide is not None and "passes" in res:
                # test-time augmentation: preprocess returned dict(passes=[(packed, sizes, flip), ...], base=index) (encode_images_multiscale)
                st = encode_images_multiscale(model, res["passes"], text, top_cls_num, win=slide[0], stride=slide[1], crf=crf, mean=mean, std=std,
                                              sim_dtype=sim_dtype, window_batch=window_batch, base=res["base"], refiner=refiner)
                st["preprocessed"] = res
                return st
            if isinstance(res, dict) and slide is not None:
                st = encode_images_sliding(model, res["packed"], text, top_cls_num, win=slide[0], stride=slide[1], crf=crf, mean=mean, std=std,
                                           sim_dtype=sim_dtype, window_batch=window_batch, sizes=res["sizes"], refiner=refiner)
                st["preprocessed"] = res
                return st
            image = res["images"] if isinstance(res, dict) else res
            if not torch.is_tensor(image):
                raise ValueError("evaluate_sharded: without slide=(win, stride) the preprocessed images of a batch must share one size")
            if slide is None:
                st = encode_batch(model, image, text, top_cls_num, crf=crf, mean=mean, std=std, sim_dtype=sim_dtype, refiner=refiner)
                st["preprocessed"] = res
                return st
        if isinstance(image, (list, tuple)):        # images of any sizes: the any-size sliding-window path
            return encode_images_sliding(model, image, text, top_cls_num, win=slide[0], stride=slide[1], crf=crf, mean=mean, std=std,
                                         sim_dtype=sim_dtype, window_batch=window_batch, refiner=refiner)
        if slide is not None:
            return encode_batch_sliding(model, image, text, top_cls_num, win=slide[0], stride=slide[1], crf=crf, mean=mean, std=std,
                                        sim_dtype=sim_dtype, window_batch=window_batch, refiner=refiner)
        return encode_batch(model, image, text, top_cls_num, crf=crf, mean=mean, std=std, sim_dtype=sim_dtype, refiner=refiner)

    def finish(st, image, label):
        if "plan" in st:                            # the any-size path's state (encode_images_sliding)
            return finish_sliding(st, label, hist=hist, num_classes=C)
        if isinstance(label, (list, tuple)):        # raw-size labels of a preprocessed batch: one seg_predict per label size
            return _finish_by_label_size(st, label, hist)
        return finish_batch(st, label, hist=hist)

    count = 0
    # (PAMR has no host read for the pipeline to hide: whole batches back to back, as under crf=False - DESIGN.md "PAMR refinement")
    pipe = EvalPipeline(dev, encode, finish, pipelined=(crf and refiner is None) if pipelined is None else pipelined)
    with torch.no_grad():
        for image, label in (batches if presharded else shard_batches(batches, rank, world)):      # presharded: `batches` is already this rank's share
            if preprocess is not None:
                # raw images stay where they are: preprocess packs host ones into one pinned buffer and copies that once
                pipe.submit(list(image), [y.to(dev, non_blocking=True) for y in label] if isinstance(label, (list, tuple)) else label.to(dev, non_blocking=True))
                count += len(image)
                continue
            if isinstance(image, (list, tuple)):
                if slide is None:
                    raise ValueError("evaluate_sharded: batches of image lists need slide=(win, stride)")
                pipe.submit([x.to(dev, non_blocking=True) for x in image], [y.to(dev, non_blocking=True) for y in label])
                count += len(image)
                continue
            pipe.submit(image.to(dev, non_blocking=True),
                        [y.to(dev, non_blocking=True) for y in label] if isinstance(label, (list, tuple)) else label.to(dev, non_blocking=True))
            count += image.shape[0]
        pipe.flush()
    n_img = torch.tensor([count], device=dev, dtype=torch.int64)
    if world > 1:
        dist.all_reduce(hist, op=dist.ReduceOp.SUM, group=group)          # the evaluation's only collective: 3*C int64 areas
        dist.all_reduce(n_img, op=dist.ReduceOp.SUM, group=group)
    iou, miou = iou_from_hist(hist)
    return {"iou": iou, "miou": miou, "hist": hist, "images": int(n_img), "images_local": count, "rank": rank, "world": world}


PER_IMAGE_KEYS = ("cand_idx", "cand_score", "threshold", "masks", "prob", "images_u8")      # the entries of encode_batch's state with one row per image


def _finish_by_label_size(st, labels, hist):
    """finish_batch() for a batch whose labels are a list of [Hl_i, Wl_i] maps: images that share a label size finish together (the
    histogram sums are independent of the grouping).  The rows of the PER_IMAGE_KEYS entries are taken per group; everything else in the
    state is passed on as it is."""
    keys = {}
    for b, lab in enumerate(labels):
        keys.setdefault(tuple(lab.shape[-2:]), []).append(b)
    if len(keys) == 1:
        return finish_batch(st, labels[0][None].contiguous() if len(labels) == 1 else torch.stack(list(labels)), hist=hist)
    dev = st["cand_idx"].device
    for k in PER_IMAGE_KEYS:
        if st.get(k) is not None and st[k].shape[0] != len(labels):
            raise ValueError(f"_finish_by_label_size: state entry {k!r} has {st[k].shape[0]} rows for {len(labels)} labels")
    out = None
    for bs in keys.values():
        idx = ops.to_device_async(bs, dev)
        sub = {k: (v[idx] if k in PER_IMAGE_KEYS and v is not None else v) for k, v in st.items()}
        out = finish_batch(sub, torch.stack([labels[b] for b in bs]), hist=hist)
    return out


def finish_batch(st, label, hist=None, refine=None, want_pred=False):
    return segment_finish(st, label, hist=hist, want_pred=want_pred, refine=refine, images_u8=st.get("images_u8"))


def eval_batch(model, image, label, text, top_cls_num, hist=None, crf=True, mean=None, std=None, sim_dtype=None, refine=None,
               want_pred=False, refiner=None):
    """One batch of the zero-shot segmentation evaluation, everything on the device (tools/seg_evaluation.py:99-170 for every image of
    the batch at once): towers -> pooled embedding + projected patch tokens -> similarity map for all classes -> segment().
    image [B,3,S,S] normalised network input, label [B,H,W] uint8, text [C,512] unit-norm class embeddings.  crf: run the DenseCRF on
    the de-normalised input (image * std + mean, :104) as the reference does; refiner="pamr" (or ("pamr", {parameters})): PAMR in its
    place (pamr_masks); hist [3,C] int64 accumulates."""
    st = encode_batch(model, image, text, top_cls_num, crf=crf, mean=mean, std=std, sim_dtype=sim_dtype, refine=refine, refiner=refiner)
    return finish_batch(st, label, hist=hist, refine=refine, want_pred=want_pred)


_PIPE_STREAMS = {}


def _pipeline_streams(device):
    """Two normal-priority encoder streams + one high-priority finishing stream per device, created ONCE per process: the runtime maps
    streams onto a few hardware queues when they are created, and two streams that land on one queue serialise - a fresh set per
    evaluation made the finishing stage's luck (its own queue, or behind an encoder's) vary from call to call."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    st = _PIPE_STREAMS.get(key)
    if st is None:
        lo, hi = 0, -1
        try:
            lo, hi = torch.cuda.Stream.priority_range()
        except Exception:       # noqa: BLE001  (older torch: the documented default range)
            pass
        st = _PIPE_STREAMS[key] = ([torch.cuda.Stream(device=device, priority=lo) for _ in range(2)], torch.cuda.Stream(device=device, priority=hi))
    return st


class EvalPipeline:
    """Software-pipelined evaluation: batch i's ENCODER is enqueued before batch i-1 is finished, and the finishing stage runs on its
    own HIGH-PRIORITY stream.  The DenseCRF stage needs one host read (the candidate table) and then issues ~100 small dependent
    launches per chunk from a Python loop; run back to back with its own encoder, the GPU idles through that loop (6 of the 23 ms the
    stage took per 63-window batch of 512^2).  Here the encoders alternate between two normal-priority streams (two batches in flight:
    one's attention / LayerNorm phases fill the tile-grid tails of the other's GEMMs), so MFMA work is always queued, and the stage's
    small kernels take the CUs they need as soon as a GEMM tile retires (without the priority a chain of small dependent kernels
    queues behind whole GEMM launches of the other stream: measured 3x slower end to end in fp32).  Same work per batch, same results
    (the histograms accumulate atomically: no ordering between batches is needed).
    Memory: a batch's intermediate tensors are produced under an encoder stream and read by the finishing stream.  They are kept
    referenced here until an event behind the finishing stage has completed (no record_stream: that defers the allocator's reuse of
    every marked block and sent each batch back to hipMalloc), at most `depth` batches deep."""

    def __init__(self, device, encode, finish, depth=3, pipelined=True):
        # pipelined = False: whole batches on the two alternating streams, each finished right behind its encoder - the better order when
        # the finishing stage has no host read and no long chain of small launches (no DenseCRF: 3071 vs 2927 windows/s, ViT-B bf16 512^2)
        self.pipelined = pipelined
        self.enc_streams, self.post_stream = _pipeline_streams(torch.device(device))
        self.encode, self.finish, self.depth = encode, finish, depth
        self.i, self.pending, self.last, self.retire = 0, None, None, []

    def _reap(self, keep):
        while self.retire and (len(self.retire) > keep or self.retire[0][0].query()):
            self.retire[0][0].synchronize()
            self.retire.pop(0)

    def submit(self, *batch):
        self._reap(self.depth)
        cur = torch.cuda.current_stream()
        st = self.enc_streams[self.i % 2]
        self.i += 1
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            enc = self.encode(*batch)
            ev = torch.cuda.Event()
            ev.record()
            if not self.pipelined:
                self.last = self.finish(enc, *batch)
                # the batch was allocated under the caller's stream and is read by kernels queued on this one: keep it (and the encoder's
                # outputs) referenced until an event behind them has completed, as the pipelined path does - otherwise the caching
                # allocator may hand those blocks to the caller's next host->device copy while they are still being read
                done = torch.cuda.Event()
                done.record()
                self.retire.append((done, enc, batch))
                return
        prev, self.pending = self.pending, (ev, enc, batch)
        if prev is not None:
            self._finish(prev)

    def _finish(self, item):
        ev, enc, batch = item
        self.post_stream.wait_event(ev)
        with torch.cuda.stream(self.post_stream):
            self.last = self.finish(enc, *batch)
            done = torch.cuda.Event()
            done.record()
        self.retire.append((done, enc, batch))

    def flush(self):
        if self.pending is not None:
            self._finish(self.pending)
            self.pending = None
        self._reap(0)
        cur = torch.cuda.current_stream()
        for st in self.enc_streams + [self.post_stream]:
            cur.wait_stream(st)
        return self.last


def iou_from_hist(hist):
    """hist [3,C] int64 -> (per-class IoU float64 with NaN where the class never occurs, mean over non-NaN) as :172-173."""
    inter, pred, label = hist[0].double(), hist[1].double(), hist[2].double()
    union = pred + label - inter
    iou = inter / union
    return iou, iou[~torch.isnan(iou)].mean()
