"""Device-side image preprocessing: decoded uint8 [H, W, 3] images -> the towers' normalised fp32 input in ONE launch per batch,
bit-identical to the host route PIL.Image.resize -> _to_tensor -> normalize (simseg/transforms).  DESIGN.md "Device-side image
preprocessing" states the arithmetic; resample_ref() below is the same statement in numpy.

Pillow's uint8 resample is integer arithmetic: per axis a float64 filter table rounded to 22 fractional bits, an int32 accumulator
that starts at 2^21, a shift and a clamp; horizontal pass first, its uint8 result feeds the vertical pass.  The host computes the
tables (axis_coefficients), the device applies them (csrc/preproc.hip), and the normalisation is a [3, 256] fp32 look-up table the
host fills with its own arithmetic, so no result depends on how the device divides."""
import math
import threading

import numpy as np
import torch

PRECISION_BITS = 22
FILTERS = {"bilinear": 1.0, "bicubic": 2.0}        # filter -> support
IMG_COLS = 16                                      # int64 columns of the image table (include/simseg_hip.h simseg_image_preprocess)
TILE_W, TILE_H = 64, 32                            # output tile of one workgroup (csrc/resample.h PP_TW, PP_TH)


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x, a=-0.5):                           # Keys, a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


_FILTER_FN = {"bilinear": _bilinear, "bicubic": _bicubic}
_AXIS = {}


def axis_coefficients(n_in, n_out, filt):
    """-> (bounds int32 [out, 2] = (xmin, n), coeffs int32 [out, ksize]) of one axis, float64 on the host, cached per key.  Unused
    tail coefficients of a row are zero.  in == out gives the identity (xmin = x, n = 1, k = 2^22): the pass Pillow skips."""
    key = (int(n_in), int(n_out), filt)
    hit = _AXIS.get(key)
    if hit is not None:
        return hit
    n_in, n_out = key[0], key[1]
    if n_in < 1 or n_out < 1:
        raise ValueError(f"axis_coefficients: lengths must be positive, got {n_in} -> {n_out}")
    if filt not in FILTERS:
        raise ValueError(f"axis_coefficients: filter is one of {sorted(FILTERS)}, got {filt!r}")
    if n_in == n_out:
        bounds = np.stack([np.arange(n_out, dtype=np.int32), np.ones(n_out, dtype=np.int32)], 1)
        coeffs = np.full((n_out, 1), 1 << PRECISION_BITS, dtype=np.int32)
    else:
        f = _FILTER_FN[filt]
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = FILTERS[filt] * fs
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / fs                              # (the argument is scaled by this reciprocal, as Pillow's precompute_coeffs does)
        bounds = np.zeros((n_out, 2), dtype=np.int32)
        coeffs = np.zeros((n_out, ksize), dtype=np.int32)
        for x in range(n_out):
            center = (x + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), n_in)
            n = xmax - xmin
            w = f((np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss)
            ww = 0.0
            for v in w:                            # summed left to right
                ww += float(v)
            if ww != 0.0:
                w = w / ww
            k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS))
            bounds[x] = (xmin, n)
            coeffs[x, :n] = np.trunc(k).astype(np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    _AXIS[key] = (bounds, coeffs)
    return bounds, coeffs


def _pass_ref(a, n_out, filt):
    """One pass along axis 1 of a uint8 [R, in, C] array."""
    bounds, coeffs = axis_coefficients(a.shape[1], n_out, filt)
    out = np.empty((a.shape[0], n_out, a.shape[2]), dtype=np.uint8)
    src = a.astype(np.int64)
    for x in range(n_out):
        xmin, n = int(bounds[x, 0]), int(bounds[x, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.einsum("rnc,n->rc", src[:, xmin:xmin + n], coeffs[x, :n].astype(np.int64))
        assert np.abs(acc).max(initial=0) < (1 << 31)
        out[:, x] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample_ref(u8, out_hw, filt):
    """numpy statement of Pillow's uint8 resize: u8 [H, W, C] -> [OH, OW, C]; horizontal pass first (skipped when the width does not
    change), its uint8 result is the input of the vertical pass (skipped when the height does not change)."""
    a = np.asarray(u8)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("resample_ref: a uint8 [H, W, C] array is expected")
    OH, OW = int(out_hw[0]), int(out_hw[1])
    if a.shape[1] != OW:
        a = _pass_ref(a, OW, filt)
    if a.shape[0] != OH:
        a = _pass_ref(a.transpose(1, 0, 2), OH, filt).transpose(1, 0, 2)
    return np.ascontiguousarray(a)


# ---- the spec: which resize, which crop, which normalisation ----------------------------------------------------------------------------
def make_spec(kind, size, filt, crop=None, mean=None, std=None, lut=None):
    """kind 'square' (-> size x size) or 'short' (shorter side -> size, the longer one max(1, round(...))); crop: centre-crop size or None;
    lut: fp32 [3, 256], byte value -> normalised value per channel."""
    if kind not in ("square", "short") or filt not in FILTERS:
        raise ValueError(f"make_spec: kind 'square' | 'short' and filter {sorted(FILTERS)} expected, got {kind!r}, {filt!r}")
    return {"kind": kind, "size": int(size), "filter": filt, "crop": None if crop is None else int(crop),
            "mean": None if mean is None else [float(m) for m in mean], "std": None if std is None else [float(s) for s in std], "lut": lut}


def make_lut(mean, std):
    """[3, 256] fp32: the 256 byte values through the host route's own arithmetic (uint8 -> float / 255, then (t - mean) / std)."""
    t = torch.arange(256, dtype=torch.uint8).view(1, 1, 256).expand(3, 1, 256).float().div_(255.0)
    mean = torch.tensor(mean).view(-1, 1, 1)
    std = torch.tensor(std).view(-1, 1, 1)
    return ((t - mean) / std).view(3, 256).contiguous()


def resized_size(spec, H, W):
    """(RH, RW) of the resize alone, as resize_op / resize_bicubic_op compute it."""
    s = spec["size"]
    if spec["kind"] == "square":
        return s, s
    if W <= H:
        return max(1, round(H * s / W)), s
    return s, max(1, round(W * s / H))


def geometry(spec, H, W):
    """-> (RH, RW, top, left, OH, OW): the resized extent and the output rectangle inside it."""
    RH, RW = resized_size(spec, H, W)
    c = spec["crop"]
    if c is None:
        return RH, RW, 0, 0, RH, RW
    left, top = int(round((RW - c) / 2.0)), int(round((RH - c) / 2.0))
    if left < 0 or top < 0 or left + c > RW or top + c > RH:
        raise NotImplementedError(f"device preprocessing: a {c} x {c} centre crop does not lie inside the resized {RH} x {RW} image "
                                  "(PIL pads such a crop with black; use the host route)")
    return RH, RW, top, left, c, c


# ---- plan: host geometry + device tables ------------------------------------------------------------------------------------------------
# Axis tables and look-up tables are uploaded ONCE and then read by launches on whatever stream is current (EvalPipeline alternates between
# two encoder streams).  Two rules keep that safe:
#   * visibility: every upload records an event on the stream that queued the copy, and every use makes the current stream wait for the
#     events that have not completed yet (_Uploads) - a launch on stream 1 never runs ahead of a copy queued on stream 0;
#   * lifetime: cached device memory is never handed back while work may still read it.  The axis tables live in a fixed-size arena per
#     device that only grows inside itself; when it is full (ARENA_INTS, ~800 axes of a 512-pixel evaluation) the DEVICE IS SYNCHRONISED
#     before the arena is replaced, and the look-up table cache does the same before it is cleared.
ARENA_INTS = 1 << 22
_LOCK = threading.Lock()


class _Uploads:
    """The events of uploads that other streams may not have seen yet, one (the latest) per uploading stream."""

    def __init__(self):
        self.events = {}

    def uploaded(self):
        ev = torch.cuda.Event()
        ev.record()
        self.events[torch.cuda.current_stream().cuda_stream] = ev

    def wait(self):
        cur = torch.cuda.current_stream()
        for sid, ev in list(self.events.items()):
            if ev.query():
                del self.events[sid]
            elif sid != cur.cuda_stream:
                cur.wait_event(ev)


class _Arena:
    """One int32 device buffer per device that holds, per axis (in, out, filter), bounds [out, 2] then coeffs [out, ksize] at a fixed
    offset, with a host mirror of the same layout (what the C entry point checks).  An axis is uploaded once, when it is first seen."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.dev = torch.zeros(ARENA_INTS, dtype=torch.int32, device=self.device)
        self.host = np.zeros(ARENA_INTS, dtype=np.int32)
        self.where, self.used, self.uploads = {}, 0, _Uploads()
        if self.device.type == "cuda":
            self.uploads.uploaded()                     # the zero fill above is queued work like any upload

    def fits(self, axes):
        need = sum(sum(t.size for t in axis_coefficients(*ax)) for ax in axes if ax not in self.where)
        return self.used + need <= ARENA_INTS

    def add(self, axes):
        new = [ax for ax in sorted(axes) if ax not in self.where]
        if self.device.type == "cuda":
            self.uploads.wait()                         # before writing too: the fill queued on another stream must not land on a later upload
        if new:
            start = self.used
            for ax in new:
                b, c = axis_coefficients(*ax)
                self.where[ax] = (self.used, c.shape[1])
                self.host[self.used:self.used + b.size] = b.reshape(-1)
                self.host[self.used + b.size:self.used + b.size + c.size] = c.reshape(-1)
                self.used += b.size + c.size
            piece = torch.from_numpy(self.host[start:self.used])
            if self.device.type == "cuda":
                self.dev[start:self.used].copy_(piece.pin_memory(), non_blocking=True)
                self.uploads.uploaded()
            else:
                self.dev[start:self.used].copy_(piece)


_ARENAS = {}


def _arena(axes, device):
    """The device's arena with `axes` in it and visible to the current stream."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    with _LOCK:
        ar = _ARENAS.get(device)
        if ar is not None and not ar.fits(axes):
            if device.type == "cuda":
                torch.cuda.synchronize(device)          # launches that read the full arena have finished before it is let go
            ar = None
        if ar is None:
            ar = _ARENAS[device] = _Arena(device)
            if not ar.fits(axes):
                raise ValueError(f"preproc.plan: the axis tables of one batch need more than {ARENA_INTS} int32 entries")
        ar.add(axes)
        return ar


def plan(sizes, spec, device):
    """sizes [(H, W), ...] of the raw images -> dict: img_tab (device int64 [B, 16]) + its host copy, the axis tables (the device's arena
    and its host mirror: an axis is uploaded once per process, and the current stream is made to wait for uploads other streams queued),
    out_sizes [(OH, OW)], src_off (bytes), out_off (fp32 elements; the images' [3, OH, OW] planes lie back to back: the packed layout
    of ops.slide_plan's src_off), src_bytes, out_numel, tiles."""
    from . import ops
    filt = spec["filter"]
    geo = [geometry(spec, int(H), int(W)) for H, W in sizes]
    axes = set()
    for (H, W), (RH, RW, *_r) in zip(sizes, geo):
        axes.add((int(W), RW, filt))
        axes.add((int(H), RH, filt))
    ar = _arena(axes, device)
    tab, tab_host, where = ar.dev, ar.host, ar.where
    rows, src_off, out_off, out_sizes = [], [], [], []
    s = o = tiles = 0
    for (H, W), (RH, RW, top, left, OH, OW) in zip(sizes, geo):
        H, W = int(H), int(W)
        hoff, hks = where[(W, RW, filt)]
        voff, vks = where[(H, RH, filt)]
        rows.append([s, H, W, o, OH, OW, top, left, hoff, hks, voff, vks, RH, RW, o, tiles])
        src_off.append(s); out_off.append(o); out_sizes.append((OH, OW))
        s += H * W * 3
        o += 3 * OH * OW
        tiles += -(-OW // TILE_W) * -(-OH // TILE_H)
    host = np.asarray(rows, dtype=np.int64).reshape(-1, IMG_COLS)
    return {"img_tab": ops.to_device_async(rows, device), "img_tab_host": host, "tab": tab, "tab_host": tab_host, "sizes": [(int(H), int(W)) for H, W in sizes],
            "out_sizes": out_sizes, "src_off": src_off, "out_off": out_off, "src_bytes": s, "out_numel": o, "tiles": tiles}


def plan_extents(sizes, targets, filt, device):
    """plan() for explicit per-image target extents: raw image i of sizes[i] = (H, W) is resized to targets[i] = (OH, OW) with `filt`, no
    crop (the scaled passes of segpost.encode_images_multiscale).  Same dict, same tables, same kernel."""
    from . import ops
    if filt not in FILTERS:
        raise ValueError(f"plan_extents: filter is one of {sorted(FILTERS)}, got {filt!r}")
    if len(sizes) != len(targets):
        raise ValueError(f"plan_extents: {len(sizes)} images and {len(targets)} target extents")
    sizes = [(int(H), int(W)) for H, W in sizes]
    targets = [(int(OH), int(OW)) for OH, OW in targets]
    if any(min(hw) < 1 for hw in sizes + targets):
        raise ValueError(f"plan_extents: extents must be positive, got {sizes} -> {targets}")
    axes = set()
    for (H, W), (OH, OW) in zip(sizes, targets):
        axes.add((W, OW, filt))
        axes.add((H, OH, filt))
    ar = _arena(axes, device)
    rows, src_off, out_off = [], [], []
    s = o = tiles = 0
    for (H, W), (OH, OW) in zip(sizes, targets):
        hoff, hks = ar.where[(W, OW, filt)]
        voff, vks = ar.where[(H, OH, filt)]
        rows.append([s, H, W, o, OH, OW, 0, 0, hoff, hks, voff, vks, OH, OW, o, tiles])
        src_off.append(s); out_off.append(o)
        s += H * W * 3
        o += 3 * OH * OW
        tiles += -(-OW // TILE_W) * -(-OH // TILE_H)
    host = np.asarray(rows, dtype=np.int64).reshape(-1, IMG_COLS)
    return {"img_tab": ops.to_device_async(rows, device), "img_tab_host": host, "tab": ar.dev, "tab_host": ar.host, "sizes": sizes,
            "out_sizes": targets, "src_off": src_off, "out_off": out_off, "src_bytes": s, "out_numel": o, "tiles": tiles}


def preprocess_extents(images_u8, targets, spec, filt="bilinear", mean=None, std=None, device=None, src=None):
    """preprocess() to explicit per-image extents targets = [(OH, OW), ...] with `filt`: the spec supplies the normalisation only.
    src: the packed raw bytes of an earlier call on the same images (its 'src'), reused instead of being packed and copied again.
    -> dict('packed', 'sizes', 'plan', 'src')."""
    from . import ops
    if not images_u8:
        raise ValueError("preprocess_extents: an empty batch")
    if device is None:
        device = images_u8[0].device if images_u8[0].is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("simseg_amd.preproc.preprocess_extents runs on MI355X only; there is no CPU fallback (resample_ref is the host statement)")
    lut = spec.get("lut")
    if mean is not None or std is not None or lut is None:
        m = spec["mean"] if mean is None else mean
        s = spec["std"] if std is None else std
        if m is None or s is None:
            raise ValueError("preprocess_extents: the spec names no normalisation and none was given")
        lut = make_lut(m, s)
    lut_dev = _lut_on(lut, device)
    pl = plan_extents([tuple(t.shape[:2]) for t in images_u8], targets, filt, device)
    if src is None:
        src = _pack(images_u8, pl, device)
    packed, _ = ops.image_preprocess(src, pl, lut_dev)
    return {"packed": packed, "sizes": pl["out_sizes"], "plan": pl, "src": src}


def _pack(images_u8, pl, device):
    """The batch's [H, W, 3] uint8 images in one device buffer at pl['src_off']: host images go through ONE pinned buffer and ONE
    non-blocking copy, device images are packed on the device."""
    for t, (H, W) in zip(images_u8, pl["sizes"]):
        if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape) != (H, W, 3):
            raise ValueError(f"preprocess: uint8 [H, W, 3] images expected, got {tuple(t.shape)} {t.dtype}")
    if all(t.is_cuda for t in images_u8):
        return images_u8[0].reshape(-1) if len(images_u8) == 1 and images_u8[0].is_contiguous() else torch.cat([t.reshape(-1) for t in images_u8])
    if any(t.is_cuda for t in images_u8):
        raise ValueError("preprocess: the images of a batch are all on the host or all on the device")
    pinned = torch.empty(pl["src_bytes"], dtype=torch.uint8, pin_memory=True)
    for t, o in zip(images_u8, pl["src_off"]):
        pinned[o:o + t.numel()].view(t.shape).copy_(t)
    return pinned.to(device, non_blocking=True)


def preprocess(images_u8, spec, mean=None, std=None, want_u8=False, device=None):
    """images_u8: list of uint8 [H, W, 3] tensors (all host or all device) -> dict: 'images' = one [B, 3, S, S] fp32 tensor when every
    output has the same size, else a list of [3, H_i, W_i] views; 'packed' = the flat fp32 buffer behind them (the images back to back:
    what segpost.encode_images_sliding takes with 'sizes'); 'sizes' = [(OH, OW)]; 'u8' (want_u8) = the resized uint8 [OH, OW, 3] images.
    mean / std override the spec's normalisation."""
    from . import ops
    if not images_u8:
        raise ValueError("preprocess: an empty batch")
    if device is None:
        device = images_u8[0].device if images_u8[0].is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("simseg_amd.preproc.preprocess runs on MI355X only; there is no CPU fallback (resample_ref is the host statement)")
    lut = spec.get("lut")
    if mean is not None or std is not None or lut is None:
        m = spec["mean"] if mean is None else mean
        s = spec["std"] if std is None else std
        if m is None or s is None:
            raise ValueError("preprocess: the spec names no normalisation and none was given")
        lut = make_lut(m, s)
    lut_dev = _lut_on(lut, device)
    pl = plan([tuple(t.shape[:2]) for t in images_u8], spec, device)
    src = _pack(images_u8, pl, device)
    packed, u8 = ops.image_preprocess(src, pl, lut_dev, want_u8=want_u8)
    out_sizes = pl["out_sizes"]
    if all(sz == out_sizes[0] for sz in out_sizes):
        images = packed.view(len(out_sizes), 3, *out_sizes[0])
    else:
        images = [packed[o:o + 3 * h * w].view(3, h, w) for o, (h, w) in zip(pl["out_off"], out_sizes)]
    res = {"images": images, "packed": packed, "sizes": out_sizes, "plan": pl}
    if want_u8:
        res["u8"] = [u8[o:o + 3 * h * w].view(h, w, 3) for o, (h, w) in zip(pl["out_off"], out_sizes)]
    return res


_LUTS = {}
_LUT_UPLOADS = _Uploads()


def _lut_on(lut, device):
    """The look-up table on the device, uploaded once per (content, device) and visible to the current stream (see _Uploads)."""
    if tuple(lut.shape) != (3, 256) or lut.dtype != torch.float32:
        raise ValueError(f"preprocess: the look-up table is fp32 [3, 256], got {tuple(lut.shape)} {lut.dtype}")
    key = (lut.numpy().tobytes(), str(device))
    with _LOCK:
        hit = _LUTS.get(key)
        if hit is None:
            if len(_LUTS) >= 16:
                torch.cuda.synchronize()                # nothing still reads the tables that are let go
                _LUTS.clear()
            hit = _LUTS[key] = lut.contiguous().pin_memory().to(device, non_blocking=True)
            _LUT_UPLOADS.uploaded()
        _LUT_UPLOADS.wait()
    return hit
