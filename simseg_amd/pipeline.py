"""Device-side training transforms: every transforms.train_transforms list of the grammar below, on decoded uint8 [H, W, 3] images, in
TWO launches per batch (csrc/augment.hip, simseg_train_transforms), bit-identical to Pillow's own calls in list order
(apply_pipeline_pil).  augment.py is the special case [random_resize_crop, autoaug]; this module is the general chain on the same kernels.

    list      := geometry+ colour*
    geometry  := resize | resize_bicubic | random_resize_crop | center_crop | random_crop | random_flip
    colour    := autoaug | color_jitter          (each at most once, either order)

At most one resample (resize | resize_bicubic | random_resize_crop), random_flip at most once, crops anywhere; the final extent is the
same square S (32 .. 384) for every image.  After normalisation, random erasing iff transforms.random_erasing.reprob > 0.

The host samples every random choice (sample_pipeline_params) from a numpy Generator, in list order; plan_pipeline folds the geometry
into one integer source box, one resample and one output window with a flip flag, the colour ops into a chain of at most five ops, and
the erase boxes into the image's row.  DESIGN.md "Device-side training transforms" states the sampling law, the arithmetic, the table and
the noise index.

parse_chain(..., full=True) widens the grammar to the whole registry (DESIGN.md "SimCLR colour distortion and Gaussian blur"):

    list      := geometry+ pixel*
    pixel     := autoaug | color_jitter | color_distortion | gaussian_blur          (each at most once, any order)

Such a chain has up to twelve ops and runs through simseg_train_chain (the 144-column table) on the same two kernels; the hue shift, the
grayscale and the Gaussian blur are restated here in numpy (rgb_to_hsv_ref, hsv_to_rgb_ref, gaussian_blur_ref) as Pillow computes them."""
import math

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageFilter

from . import augment as A
from . import preproc

GEOMETRY = ("resize", "resize_bicubic", "random_resize_crop", "center_crop", "random_crop", "random_flip")
RESAMPLES = ("resize", "resize_bicubic", "random_resize_crop")
COLOUR = ("autoaug", "color_jitter")
ERASE_MODES = ("const", "rand", "pixel")
MAX_OPS, MAX_ERASE = 5, 4
OP_BRIGHTNESS = len(A.OPS)                                     # 11: the one op code the AutoAugment set lacks
JITTER_OPS = (OP_BRIGHTNESS, A.OP_CODE["contrast"], A.OP_CODE["color"], None)     # order index -> op (hue: the registry passes none)
# the full grammar (parse_chain(full=True), simseg_train_chain): the SimCLR pair and the three op codes it adds
PIXEL = COLOUR + ("color_distortion", "gaussian_blur")
OP_GRAY, OP_HUE, OP_BLUR = 12, 13, 14
DISTORT_OPS = JITTER_OPS[:3] + (OP_HUE,)                       # the distortion's ColorJitter passes a hue
FULL_MAX_OPS = 12                                              # 2 autoaug + 3 jitter + 4 distortion + gray + blur = 11
BLUR_MAX_R = 7                                                 # the kernel keeps the R + 1 bytes behind x in one 64-bit register
DISTORTION_DEFAULT = {"strength": 1.0}                         # transforms.color_distortion / gaussian_blur when the config has no such key
BLUR_DEFAULT = {"p": 0.5, "radius_min": 0.1, "radius_max": 2.0}

# the image table of simseg_train_transforms (include/simseg_hip.h); columns 0 .. 10 are augment.plan's
TT_COLS = 81
(T_SRC, T_H, T_W, T_TOP, T_LEFT, T_CH, T_CW, T_HOFF, T_HKS, T_VOFF, T_VKS, T_RH, T_RW, T_WTOP, T_WLEFT, T_FLIP, T_NOPS, T_NERASE, T_MODE,
 T_SEED) = range(20)
T_BOX, T_OP, T_P = 20, 36, 41

FIELDS = A.FIELDS + ("rcrop", "flip", "order", "jb", "jc", "js", "erase_n", "erase_box")          # per image; "seed" is per batch
FULL_FIELDS = ("d_apply", "d_order", "db", "dc", "ds", "dh", "d_gray", "blur_apply", "blur_radius")   # more, in every parameter set
# the image table of simseg_train_chain: columns 0 .. 35 as above, then 12 op codes and 12 x 8 slots
TC_COLS, TC_OP, TC_P = 144, 36, 48


# ---- the grammar ----------------------------------------------------------------------------------------------------------------------------
def _refuse(rule, names):
    raise NotImplementedError(f"train transforms {list(names)}: {rule}")


def _keys_of(tr, name, default):
    """transforms.<name> as a dict of floats: the config's keys where it has them, the registry's defaults where it has not."""
    got = tr.get(name) if hasattr(tr, "get") else getattr(tr, name, None)
    return {k: float(got[k]) if got is not None and k in got else v for k, v in default.items()}


def parse_chain(names, cfg, lut=None, full=False):
    """names (transforms.train_transforms) + the config -> the chain: dict of names, geom [(name, size)], colour [name], size S, scale,
    jitter v, erase {reprob, mode, recount} or None, mean, std, lut, full.  A list outside the grammar raises NotImplementedError naming
    the rule; recount outside 1 .. 4 raises ValueError.  full: the grammar list := geometry+ pixel* (color_distortion and gaussian_blur
    too); the chain then also holds distort {strength} and blur {p, radius_min, radius_max} (None when the list lacks the op) and runs
    through simseg_train_chain."""
    names = [str(n) for n in names]
    tr = cfg.transforms
    pixel, word = (PIXEL, "pixel") if full else (COLOUR, "colour")
    for n in names:
        if n not in GEOMETRY + pixel:
            _refuse(f"rule 'geometry | {word}': {n!r} is none of {list(GEOMETRY + pixel)}", names)
    ng = 0
    while ng < len(names) and names[ng] in GEOMETRY:
        ng += 1
    if ng == 0:
        _refuse(f"rule 'list := geometry+ {word}*': the list starts with at least one geometry op", names)
    for n in names[ng:]:
        if n in GEOMETRY:
            _refuse(f"rule 'list := geometry+ {word}*': geometry op {n!r} stands after a {word} op", names)
    if sum(n in RESAMPLES for n in names) > 1:
        _refuse(f"rule 'at most one resample': more than one of {list(RESAMPLES)}", names)
    for n in ("random_flip",) + pixel:
        if names.count(n) > 1:
            _refuse(f"rule '{n} at most once': it stands {names.count(n)} times", names)
    distort = blur = None
    if "color_distortion" in names:
        distort = _keys_of(tr, "color_distortion", DISTORTION_DEFAULT)
        if not 0.0 < distort["strength"] <= 2.5:
            _refuse(f"rule 'color_distortion.strength in (0, 2.5]' (the hue range 0.2 * strength is at most 0.5): got {distort['strength']}",
                    names)
    if "gaussian_blur" in names:
        blur = _keys_of(tr, "gaussian_blur", BLUR_DEFAULT)
        if not 0.0 <= blur["p"] <= 1.0:
            _refuse(f"rule 'gaussian_blur.p in [0, 1]': got {blur['p']}", names)
        if not 0.0 < blur["radius_min"] <= blur["radius_max"]:
            _refuse(f"rule 'gaussian_blur: 0 < radius_min <= radius_max': got {blur['radius_min']}, {blur['radius_max']}", names)
        if blur_weights(blur["radius_max"])[0] > BLUR_MAX_R:
            _refuse(f"rule 'gaussian_blur: the box radius of radius_max is at most {BLUR_MAX_R}' (Pillow radii up to 8.4): got "
                    f"radius_max {blur['radius_max']}", names)
    size_of = {"resize": lambda: tr.resize.size, "resize_bicubic": lambda: tr.resize_bicubic.size,
               "random_resize_crop": lambda: tr.random_resize_crop.size, "center_crop": lambda: tr.center_crop.size,
               "random_crop": lambda: tr.random_crop.size, "random_flip": lambda: 0}
    geom = [(n, int(size_of[n]())) for n in names[:ng]]
    # the final extent, symbolically: None = the raw image's, ("short", s) after resize_bicubic, ("square", s)
    ext = None
    for n, s in geom:
        if n == "resize_bicubic":
            ext = ("short", s)
        elif n != "random_flip":
            ext = ("square", s)
    if ext is None or ext[0] != "square" or not 32 <= ext[1] <= 384:
        _refuse("rule 'the final extent is the same square S for every image, 32 <= S <= 384': the geometry ends with resize, "
                f"random_resize_crop or a crop of such a size (it ends with the extent {ext})", names)
    erase = None
    er = tr.random_erasing
    if float(er.reprob) > 0:
        if er.remode not in ERASE_MODES:
            _refuse(f"rule 'remode in const | rand | pixel': got {er.remode!r}", names)
        if not 1 <= int(er.recount) <= MAX_ERASE:
            raise ValueError(f"train transforms: random_erasing.recount is 1 .. {MAX_ERASE}, got {er.recount}")
        erase = {"reprob": float(er.reprob), "mode": str(er.remode), "recount": int(er.recount)}
    mean, std = [float(m) for m in tr.normalize.mean], [float(s) for s in tr.normalize.std]
    return {"names": names, "geom": geom, "colour": names[ng:], "size": ext[1], "scale": tuple(float(v) for v in tr.random_resize_crop.scale),
            "jitter": float(tr.color_jitter), "erase": erase, "mean": mean, "std": std,
            "lut": preproc.make_lut(mean, std) if lut is None else lut, "full": bool(full), "distort": distort, "blur": blur}


# ---- Pillow's arithmetic of the three new ops, in numpy (tests/test_train_views_host.py: zero differing bytes) ------------------------------
def blur_weights(radius):
    """ImageFilter.GaussianBlur(radius) -> (R, ww, fw) of its box passes: the fractional box radius fr in float32 (the square root's
    argument alone in double), R = int(fr), ww = int(2^24 / (2 fr + 1)) with a FLOAT32 division, fw = (2^24 - (2R + 1) ww) // 2."""
    f = np.float32
    r = f(radius)
    s2 = f(f(r * r) / f(3.0))
    L = f(math.sqrt(12.0 * float(s2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = f(f(f(2.0) * l + f(1.0)) * f(f(l * f(l + f(1.0))) - f(f(3.0) * s2)))
    a = f(a / f(f(6.0) * f(s2 - f(f(l + f(1.0)) * f(l + f(1.0))))))
    fr = f(l + a)
    R = int(fr)
    ww = int(f(16777216.0) / f(f(fr * f(2.0)) + f(1.0)))
    return R, ww, ((1 << 24) - (2 * R + 1) * ww) // 2


def _box_pass(a, R, ww, fw):
    """One box pass along the last axis of a uint8 array, indices clamped to the line, rounded to bytes."""
    n = a.shape[-1]
    v = a.astype(np.int64)
    at = lambda d: v[..., np.clip(np.arange(n) + d, 0, n - 1)]          # noqa: E731
    acc = sum(at(d) for d in range(-R, R + 1)) * ww + (at(-R - 1) + at(R + 1)) * fw + (1 << 23)
    return (acc >> 24).astype(np.uint8)


def gaussian_blur_ref(a, radius):
    """uint8 [H, W, C] -> ImageFilter.GaussianBlur(radius) of it: three box passes along the rows, then three along the columns, every
    pass on the bytes the pass before it left."""
    R, ww, fw = blur_weights(radius)
    out = np.ascontiguousarray(np.moveaxis(np.asarray(a, np.uint8), 2, 0))          # [C, H, W]
    for _ in range(3):
        out = _box_pass(out, R, ww, fw)
    out = np.swapaxes(out, 1, 2)
    for _ in range(3):
        out = _box_pass(out, R, ww, fw)
    return np.ascontiguousarray(np.moveaxis(np.swapaxes(out, 1, 2), 0, 2))


def rgb_to_hsv_ref(rgb):
    """uint8 [..., 3] -> Pillow's convert("HSV") of it: float32 divisions, h formed in float32 (r the maximum) or in double, then
    fmod(h / 6 + 1, 1) in double, H and S truncated."""
    rgb = np.asarray(rgb, np.uint8)
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(f)
        s = cr / mx.astype(f)
        rc, gc, bc = ((mx - c).astype(f) / cr for c in (r, g, b))
        h_r = (bc - gc).astype(f)
        h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(f)
        h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(f)
        h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
        hh = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f)
        H = np.clip((hh.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        Sv = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H, Sv = np.where(grey, 0, H), np.where(grey, 0, Sv)
    return np.stack([H, Sv, mx], axis=-1).astype(np.uint8)


def hsv_to_rgb_ref(hsv):
    """uint8 [..., 3] HSV -> Pillow's convert("RGB") of it, all in double: p, q, t = floor(x + 0.5) clipped."""
    hsv = np.asarray(hsv, np.uint8)
    H, Sv, V = (hsv[..., i].astype(np.float64) for i in range(3))
    fs = Sv / 255.0
    h6 = H * 6.0 / 255.0
    i = np.floor(h6)
    fr = h6 - i
    rnd = lambda x: np.clip(np.floor(x + 0.5), 0, 255)                  # noqa: E731
    p, q, t = rnd(V * (1.0 - fs)), rnd(V * (1.0 - fs * fr)), rnd(V * (1.0 - fs * (1.0 - fr)))
    k = i.astype(np.int64) % 6
    sel = lambda *c: np.choose(k, c)                                    # noqa: E731
    out = np.stack([sel(V, q, p, p, t, V), sel(t, V, V, q, p, p), sel(p, p, t, V, V, q)], axis=-1)
    grey = hsv[..., 1] == 0
    return np.where(grey[..., None], hsv[..., 2:3], out).astype(np.uint8)


def hue_shift(hue_factor):
    """torchvision's adjust_hue on PIL: the byte added to H = int(hue_factor * 255), truncated toward zero, modulo 256."""
    return int(hue_factor * 255) & 255


def hue_ref(rgb, shift):
    """uint8 [..., 3] -> RGB -> HSV, H + shift modulo 256, -> RGB (shift 0 still makes the lossy round trip)."""
    hsv = rgb_to_hsv_ref(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + int(shift)) & 255
    return hsv_to_rgb_ref(hsv)


# ---- geometry: one walk for the sampler and the plan ------------------------------------------------------------------------------------------
def center_box(h, w, size):
    """center_crop_op's corner on an h x w image."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def short_side(h, w, size):
    """resize_bicubic_op's (RH, RW): the shorter side -> size."""
    if w <= h:
        return max(1, round(h * size / w)), size
    return size, max(1, round(w * size / h))


class _Drawn:
    """The random choices of one image's geometry, drawn from rng in list order and written into its row."""

    def __init__(self, rng, row, scale):
        self.rng, self.row, self.scale = rng, row, scale

    def rrc(self, h, w):
        box = A.crop_box(self.rng, h, w, self.scale)
        self.row.update(zip(("top", "left", "h", "w", "fallback"), box))
        return box[:4]

    def rcrop(self, k, h, w, size):
        if size > h or size > w:
            raise ValueError(f"train transforms: a {size} x {size} random_crop does not lie inside the current {h} x {w} extent (no padding)")
        tl = (int(self.rng.integers(0, h - size + 1)), int(self.rng.integers(0, w - size + 1)))
        self.row["rcrop"].append(tl)
        return tl

    def flip(self):
        self.row["flip"] = int(self.rng.random() < 0.5)
        return self.row["flip"]


class _Recorded:
    """The same choices read back from the parameters of image i."""

    def __init__(self, params, i):
        self.p, self.i = params, i

    def rrc(self, h, w):
        return tuple(int(self.p[f][self.i]) for f in ("top", "left", "h", "w"))

    def rcrop(self, k, h, w, size):
        return int(self.p["rcrop"][self.i][k][0]), int(self.p["rcrop"][self.i][k][1])

    def flip(self):
        return int(self.p["flip"][self.i])


def fold_geometry(chain, H, W, choices, who="image"):
    """The geometry ops of the chain on an H x W image, folded: -> dict box (top, left, h, w: the integer source box, in the raw image's
    unmirrored coordinates), RH, RW, filter (the one resample of the box; RH, RW = the box's extent when the list has none), wtop, wleft
    (the S x S output window inside the resized box, unmirrored coordinates) and flip (the window's columns are mirrored).

    A crop before the resample moves the source box, one after it moves the window; resize and FLIP_LEFT_RIGHT commute byte for byte
    (tests/test_train_pipeline_host.py repeats the check), so a flip is carried as a flag: while it is set, a crop's columns
    [l, l + cw) of the mirrored w-wide image are columns [w - l - cw, w - l) of the unmirrored one."""
    S = chain["size"]
    h, w = int(H), int(W)
    box, win, flipped, filt, k = [0, 0, h, w], None, 0, "bilinear", 0

    def crop(t, l, ch, cw, what):
        nonlocal h, w, box, win
        if not (0 <= t and 0 <= l and 0 < ch and 0 < cw and t + ch <= h and l + cw <= w):
            raise ValueError(f"train transforms: {who}: {what} {(t, l, ch, cw)} does not lie inside the current {h} x {w} extent "
                             "(no padding is provided)")
        cur = box if win is None else win
        cur[0] += t
        cur[1] += (w - l - cw) if flipped else l
        cur[2], cur[3] = ch, cw
        h, w = ch, cw

    def resample(rh, rw, f):
        nonlocal h, w, win, filt, RH, RW
        RH, RW, filt = int(rh), int(rw), f
        win = [0, 0, RH, RW]
        h, w = RH, RW

    RH = RW = None
    for name, size in chain["geom"]:
        if name == "random_flip":
            flipped ^= choices.flip()
        elif name == "random_crop":
            t, l = choices.rcrop(k, h, w, size)
            k += 1
            crop(t, l, size, size, "random_crop")
        elif name == "center_crop":
            t, l = center_box(h, w, size)
            crop(t, l, size, size, "center_crop")
        elif name == "random_resize_crop":
            crop(*choices.rrc(h, w), "random_resize_crop's box")
            resample(size, size, "bilinear")
        elif name == "resize":
            resample(size, size, "bilinear")
        else:
            resample(*short_side(h, w, size), "bicubic")
    if win is None:                                             # no resample: launch 1 copies the box
        RH, RW = box[2], box[3]
        win = [0, 0, RH, RW]
    if (win[2], win[3]) != (S, S):
        raise ValueError(f"train transforms: {who}: the final extent is {win[2]} x {win[3]}, not {S} x {S}")
    return {"box": tuple(box), "RH": RH, "RW": RW, "filter": filt, "wtop": win[0], "wleft": win[1], "flip": flipped}


# ---- parameters ---------------------------------------------------------------------------------------------------------------------------------
def _blank(chain):
    return {"top": 0, "left": 0, "h": 0, "w": 0, "fallback": 0, "policy": -1, "op1": 0, "mag1": 0.0, "apply1": 0, "sign1": 1, "op2": 0,
            "mag2": 0.0, "apply2": 0, "sign2": 1, "rcrop": [], "flip": 0, "order": [0, 1, 2, 3], "jb": 1.0, "jc": 1.0, "js": 1.0,
            "erase_n": 0, "erase_box": [], "d_apply": 0, "d_order": [0, 1, 2, 3], "db": 1.0, "dc": 1.0, "ds": 1.0, "dh": 0.0, "d_gray": 0,
            "blur_apply": 0, "blur_radius": 1.0}


def _columns(rows, chain, seed):
    B = len(rows)
    nrc = max(1, sum(n == "random_crop" for n, _ in chain["geom"]))
    reals = ("mag1", "mag2", "jb", "jc", "js", "db", "dc", "ds", "dh", "blur_radius")
    p = {f: np.array([r[f] for r in rows], dtype=np.float64 if f in reals else np.int64)
         for f in FIELDS + FULL_FIELDS if f not in ("rcrop", "erase_box")}
    p["rcrop"] = np.zeros((B, nrc, 2), np.int64)
    p["erase_box"] = np.zeros((B, MAX_ERASE, 4), np.int64)
    for i, r in enumerate(rows):
        for k, tl in enumerate(r["rcrop"]):
            p["rcrop"][i, k] = tl
        for k, bx in enumerate(r["erase_box"]):
            p["erase_box"][i, k] = bx
    p["order"] = p["order"].reshape(B, 4)
    p["d_order"] = p["d_order"].reshape(B, 4)
    p["seed"] = np.uint64(seed)
    return p


def erase_boxes(rng, S, reprob, recount):
    """One image's random-erasing draws -> [(top, left, h, w)] (DESIGN.md states the law; a box whose ten tries all fail is left out)."""
    if rng.random() > reprob:
        return []
    count = 1 if recount == 1 else int(rng.integers(1, recount + 1))
    out = []
    for _ in range(count):
        for _try in range(10):
            target = rng.uniform(0.02, 1 / 3) * S * S / count
            ar = math.exp(rng.uniform(math.log(0.3), math.log(1 / 0.3)))
            h = int(round(math.sqrt(target * ar)))
            w = int(round(math.sqrt(target / ar)))
            if w < S and h < S:
                out.append((int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w))
                break
    return out


def sample_pipeline_params(sizes, rng, chain):
    """sizes [(H, W)] of the raw images + a numpy Generator -> the batch's parameters.  Per image, in list order: the geometry draws
    (random_resize_crop: augment.crop_box on the current extent; random_crop: top then left, uniform; random_flip: U[0, 1) < 0.5), the
    colour draws (autoaug: augment.draw_autoaug; color_jitter: a permutation of 4, then b, c, s ~ U(max(0, 1 - v), 1 + v)), the erase
    boxes; after the last image one 64-bit noise seed when erasing is on.  For [random_resize_crop, autoaug] without erasing these are
    augment.sample_params' draws.  The same generator state gives the same parameters.  The full grammar's two ops draw everything
    whether or not they apply, so streams stay aligned: color_distortion: U[0, 1) <= 0.8 applies the jitter, a permutation of 4, then
    b, c, s ~ U(max(0, 1 - 0.8 st), 1 + 0.8 st) and hue ~ U(-0.2 st, 0.2 st), then U[0, 1) < 0.2 for the grayscale; gaussian_blur:
    U[0, 1) <= p, then radius ~ U(radius_min, radius_max)."""
    rows = []
    v, er, S = chain["jitter"], chain["erase"], chain["size"]
    for i, (H, W) in enumerate(sizes):
        r = _blank(chain)
        fold_geometry(chain, int(H), int(W), _Drawn(rng, r, chain["scale"]), who=f"image {i}")
        for name in chain["colour"]:
            if name == "autoaug":
                A.draw_autoaug(rng, r)
            elif name == "color_jitter":
                r["order"] = [int(j) for j in rng.permutation(4)]
                r["jb"], r["jc"], r["js"] = (float(rng.uniform(max(0.0, 1.0 - v), 1.0 + v)) for _ in range(3))
            elif name == "color_distortion":
                st = chain["distort"]["strength"]
                r["d_apply"] = int(rng.random() <= 0.8)
                r["d_order"] = [int(j) for j in rng.permutation(4)]
                r["db"], r["dc"], r["ds"] = (float(rng.uniform(max(0.0, 1.0 - 0.8 * st), 1.0 + 0.8 * st)) for _ in range(3))
                r["dh"] = float(rng.uniform(-0.2 * st, 0.2 * st))
                r["d_gray"] = int(rng.random() < 0.2)
            else:
                bl = chain["blur"]
                r["blur_apply"] = int(rng.random() <= bl["p"])
                r["blur_radius"] = float(rng.uniform(bl["radius_min"], bl["radius_max"]))
        if er:
            r["erase_box"] = erase_boxes(rng, S, er["reprob"], er["recount"])
            r["erase_n"] = len(r["erase_box"])
        rows.append(r)
    seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64)) if er else 0
    return _columns(rows, chain, seed)


def _per_image(v, i, B):
    return v[i] if isinstance(v, list) and len(v) == B else v


def _list_per_image(v, i):
    """v: one list of tuples for every image, or a list of such lists (one per image)."""
    return v[i] if v and isinstance(v[0], list) else v


def explicit_pipeline_params(chain, B, rrc=None, rcrop=None, flip=0, aa=None, jitter=None, erase=None, seed=0, distort=None, blur=None):
    """Parameters with every choice given, for tests and tools.  Each argument is one value for all B images or a list of B values:
    rrc (top, left, h, w); flip 0 | 1; aa (op1, mag1, sign1, op2, mag2, sign2) with op names, both applied; jitter (order, b, c, s).
    rcrop [(top, left)], one tuple per random_crop of the list, and erase [(top, left, h, w)] (at most four) are lists of tuples for
    every image, or lists of B such lists.  distort (apply, order, b, c, s, hue, gray) and blur (apply, radius): one for all or B."""
    rows = []
    for i in range(B):
        r = _blank(chain)
        if rrc is not None:
            r.update(zip(("top", "left", "h", "w"), _per_image(rrc, i, B)))
        if rcrop is not None:
            r["rcrop"] = [tuple(tl) for tl in _list_per_image(rcrop, i)]
        r["flip"] = int(_per_image(flip, i, B))
        if aa is not None:
            o1, m1, s1, o2, m2, s2 = _per_image(aa, i, B)
            r.update(op1=A.OP_CODE[o1], mag1=float(m1), apply1=int(o1 != "none"), sign1=int(s1), op2=A.OP_CODE[o2], mag2=float(m2),
                     apply2=int(o2 != "none"), sign2=int(s2))
        if jitter is not None:
            order, b, c, s = _per_image(jitter, i, B)
            r.update(order=[int(j) for j in order], jb=float(b), jc=float(c), js=float(s))
        if erase is not None:
            r["erase_box"] = [tuple(bx) for bx in _list_per_image(erase, i)]
            r["erase_n"] = len(r["erase_box"])
        if distort is not None:
            ap, order, b, c, s, hue, gray = _per_image(distort, i, B)
            r.update(d_apply=int(ap), d_order=[int(j) for j in order], db=float(b), dc=float(c), ds=float(s), dh=float(hue), d_gray=int(gray))
        if blur is not None:
            ap, radius = _per_image(blur, i, B)
            r.update(blur_apply=int(ap), blur_radius=float(radius))
        rows.append(r)
    return _columns(rows, chain, seed)


def op_chain(chain, params, i):
    """Image i's colour ops in list order -> [(op code, augment.OP_SLOTS parameter slots)]: the applied AutoAugment ops, the jitter's three
    blends in its drawn order (the hue slot does nothing); the applied distortion's four ops in its drawn order (hue: slot 0 = the byte
    added to H) and its grayscale; the applied blur (slots R, ww, fw of blur_weights).  At most MAX_OPS, FULL_MAX_OPS in the full grammar."""
    S, out = chain["size"], []
    for name in chain["colour"]:
        if name == "autoaug":
            for j in (1, 2):
                op = int(params[f"op{j}"][i])
                if params[f"apply{j}"][i] and op:
                    if not 0 < op < len(A.OPS):
                        raise ValueError(f"train transforms: image {i}: op code {op}")
                    out.append((op, A.op_slots(op, float(params[f"mag{j}"][i]), int(params[f"sign{j}"][i]), S)))
        elif name == "color_jitter":
            f = {0: params["jb"][i], 1: params["jc"][i], 2: params["js"][i]}
            for j in params["order"][i]:
                if JITTER_OPS[int(j)] is not None:
                    out.append((JITTER_OPS[int(j)], [A._f32_bits(np.float32(f[int(j)]))] + [0] * (A.OP_SLOTS - 1)))
        elif name == "color_distortion":
            f = {0: params["db"][i], 1: params["dc"][i], 2: params["ds"][i]}
            for j in (params["d_order"][i] if params["d_apply"][i] else ()):
                first = hue_shift(float(params["dh"][i])) if int(j) == 3 else A._f32_bits(np.float32(f[int(j)]))
                out.append((DISTORT_OPS[int(j)], [first] + [0] * (A.OP_SLOTS - 1)))
            if params["d_gray"][i]:
                out.append((OP_GRAY, [0] * A.OP_SLOTS))
        elif params["blur_apply"][i]:
            R, ww, fw = blur_weights(float(params["blur_radius"][i]))
            if not (0 <= R <= BLUR_MAX_R and ww > 0 and fw >= 0):
                raise ValueError(f"train transforms: image {i}: blur radius {params['blur_radius'][i]} gives R, ww, fw = {(R, ww, fw)}; "
                                 f"0 <= R <= {BLUR_MAX_R}, ww > 0 and fw >= 0 are needed")
            out.append((OP_BLUR, [R, ww, fw] + [0] * (A.OP_SLOTS - 3)))
    return out


# ---- the host reference ---------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def hash_u32_ref(seed, idx):
    """csrc/common.h hash_u32 in numpy: seed (one uint64) and idx (uint64 array) -> uint32 values (held in uint64)."""
    seed = np.uint64(seed)
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = ((idx & _M32) * np.uint64(0x9E3779B1) + (idx >> np.uint64(32)) * np.uint64(0x85EBCA77) + (seed & _M32)
             + (seed >> np.uint64(32)) * np.uint64(0xC2B2AE3D)) & _M32
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x21F0AAAD)) & _M32
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x735A2D97)) & _M32
        x ^= x >> np.uint64(15)
    return x


def erase_noise_ref(seed, b, k, box, mode):
    """The fill of erase box k = (top, left, h, w) of image b in float64: [3, h, w].  const: zeros; rand: one normal per channel;
    pixel: one per (channel, y, x).  normal(i) = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((h1 >> 8) + 1) 2^-24, u2 = (h2 >> 8) 2^-24,
    h1 = hash_u32(seed, 2 i), h2 = hash_u32(seed, 2 i + 1), i = ((b * 4 + k) * 3 + c) * 2^18 + y * 512 + x (y = x = 0 for rand)."""
    t, l, h, w = (int(v) for v in box)
    if mode == "const":
        return np.zeros((3, h, w))
    c = np.arange(3, dtype=np.uint64).reshape(3, 1, 1)
    i = (np.uint64((b * MAX_ERASE + k) * 3) + c) << np.uint64(18)
    if mode == "pixel":
        y = np.arange(t, t + h, dtype=np.uint64).reshape(1, h, 1)
        x = np.arange(l, l + w, dtype=np.uint64).reshape(1, 1, w)
        i = i + y * np.uint64(512) + x
    u1 = ((hash_u32_ref(seed, i * np.uint64(2)) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (hash_u32_ref(seed, i * np.uint64(2) + np.uint64(1)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return np.broadcast_to(z, (3, h, w)).copy()


def erase_ref(planes, params, i, chain):
    """fp32 [3, S, S] -> the same with image i's erase boxes filled, in order (erase_noise_ref rounded to fp32)."""
    out = planes.clone()
    mode = chain["erase"]["mode"] if chain["erase"] else "const"
    for k in range(int(params["erase_n"][i])):
        t, l, h, w = (int(v) for v in params["erase_box"][i][k])
        out[:, t:t + h, l:l + w] = torch.from_numpy(erase_noise_ref(params["seed"], i, k, (t, l, h, w), mode).astype(np.float32))
    return out


def apply_pipeline_pil_u8(img, params, i, chain):
    """Image i's parameters applied with Pillow's own calls, in list order -> the PIL image (before normalisation and erasing)."""
    img = img.convert("RGB")
    sizes = dict(chain["geom"])
    k = 0
    for name in chain["names"]:
        if name == "random_resize_crop":
            t, l, h, w = (int(params[f][i]) for f in ("top", "left", "h", "w"))
            img = img.crop((l, t, l + w, t + h)).resize((sizes[name], sizes[name]), Image.BILINEAR)
        elif name == "resize":
            img = img.resize((sizes[name], sizes[name]), Image.BILINEAR)
        elif name == "resize_bicubic":
            rh, rw = short_side(img.size[1], img.size[0], sizes[name])
            img = img.resize((rw, rh), Image.BICUBIC)
        elif name == "center_crop":
            t, l = center_box(img.size[1], img.size[0], sizes[name])
            img = img.crop((l, t, l + sizes[name], t + sizes[name]))
        elif name == "random_crop":
            t, l = (int(v) for v in params["rcrop"][i][k])
            k += 1
            img = img.crop((l, t, l + sizes[name], t + sizes[name]))
        elif name == "random_flip":
            if params["flip"][i]:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
        elif name == "autoaug":
            for j in (1, 2):
                if params[f"apply{j}"][i] and params[f"op{j}"][i]:
                    img = A._PIL[A.OPS[int(params[f"op{j}"][i])]](img, float(params[f"mag{j}"][i]), int(params[f"sign{j}"][i]))
        elif name == "color_jitter":
            for j in params["order"][i]:
                if j == 0:
                    img = ImageEnhance.Brightness(img).enhance(float(params["jb"][i]))
                elif j == 1:
                    img = ImageEnhance.Contrast(img).enhance(float(params["jc"][i]))
                elif j == 2:
                    img = ImageEnhance.Color(img).enhance(float(params["js"][i]))
        elif name == "color_distortion":
            for j in (params["d_order"][i] if params["d_apply"][i] else ()):
                if j == 0:
                    img = ImageEnhance.Brightness(img).enhance(float(params["db"][i]))
                elif j == 1:
                    img = ImageEnhance.Contrast(img).enhance(float(params["dc"][i]))
                elif j == 2:
                    img = ImageEnhance.Color(img).enhance(float(params["ds"][i]))
                else:                                            # torchvision's adjust_hue on PIL
                    h, s, v = img.convert("HSV").split()
                    h = Image.fromarray(((np.asarray(h, dtype=np.int64) + hue_shift(float(params["dh"][i]))) & 255).astype(np.uint8), "L")
                    img = Image.merge("HSV", (h, s, v)).convert("RGB")
            if params["d_gray"][i]:
                g = img.convert("L")
                img = Image.merge("RGB", (g, g, g))
        elif name == "gaussian_blur":
            if params["blur_apply"][i]:
                img = img.filter(ImageFilter.GaussianBlur(float(params["blur_radius"][i])))
    return img


def apply_pipeline_pil(img, params, i, chain):
    """The host route (the oracle of every device test): apply_pipeline_pil_u8, the host tail _to_tensor + normalize, then erase_ref
    -> (fp32 [3, S, S], uint8 [S, S, 3] before normalisation and erasing)."""
    from simseg.transforms import _to_tensor
    out = apply_pipeline_pil_u8(img, params, i, chain)
    m = torch.tensor(chain["mean"]).view(-1, 1, 1)
    s = torch.tensor(chain["std"]).view(-1, 1, 1)
    return erase_ref((_to_tensor(out) - m) / s, params, i, chain), np.asarray(out, dtype=np.uint8)


# ---- plan + run -----------------------------------------------------------------------------------------------------------------------------------
def plan_pipeline(sizes, params, chain, device):
    """sizes [(H, W)] of the raw images + their parameters -> dict: img_tab (device int64 [B, TT_COLS], [B, TC_COLS] for a chain of the
    full grammar) + its host copy, the axis tables
    (preproc's per-device arena and its host mirror), src_off / src_bytes of the packed raw images, sizes, size, geometry (fold_geometry
    per image).  A crop outside the current extent raises ValueError."""
    from . import ops
    S, B = chain["size"], len(sizes)
    full = chain.get("full", False)
    cols, max_ops, t_p = (TC_COLS, FULL_MAX_OPS, TC_P) if full else (TT_COLS, MAX_OPS, T_P)
    if B < 1 or any(len(params[f]) != B for f in FIELDS):
        raise ValueError(f"train transforms: {B} images and parameters for {[len(params[f]) for f in FIELDS]}")
    geo = [fold_geometry(chain, int(H), int(W), _Recorded(params, i), who=f"image {i}") for i, (H, W) in enumerate(sizes)]
    axes = set()
    for g in geo:
        axes.add((g["box"][3], g["RW"], g["filter"]))
        axes.add((g["box"][2], g["RH"], g["filter"]))
    ar = preproc._arena(axes, device)
    mode = ERASE_MODES.index(chain["erase"]["mode"]) if chain["erase"] else 0
    seed = int(np.uint64(params["seed"]).astype(np.int64))
    rows, src_off, s = [], [], 0
    for i, ((H, W), g) in enumerate(zip(sizes, geo)):
        H, W = int(H), int(W)
        t, l, h, w = g["box"]
        hoff, hks = ar.where[(w, g["RW"], g["filter"])]
        voff, vks = ar.where[(h, g["RH"], g["filter"])]
        chain_ops = op_chain(chain, params, i)
        ne = int(params["erase_n"][i])
        if len(chain_ops) > max_ops or not 0 <= ne <= MAX_ERASE:
            raise ValueError(f"train transforms: image {i}: {len(chain_ops)} ops (at most {max_ops}), {ne} erase boxes (at most {MAX_ERASE})")
        row = [0] * cols
        row[:T_SEED + 1] = [s, H, W, t, l, h, w, hoff, hks, voff, vks, g["RH"], g["RW"], g["wtop"], g["wleft"], g["flip"], len(chain_ops), ne,
                            mode, seed]
        for k in range(ne):
            bt, bl, bh, bw = (int(v) for v in params["erase_box"][i][k])
            if not (0 <= bt and 0 <= bl and 0 < bh and 0 < bw and bt + bh <= S and bl + bw <= S):
                raise ValueError(f"train transforms: image {i}: erase box {(bt, bl, bh, bw)} does not lie inside the {S} x {S} output")
            row[T_BOX + 4 * k:T_BOX + 4 * k + 4] = [bt, bl, bh, bw]
        for k, (op, slots) in enumerate(chain_ops):
            row[T_OP + k] = op
            row[t_p + k * A.OP_SLOTS:t_p + (k + 1) * A.OP_SLOTS] = slots
        rows.append(row)
        src_off.append(s)
        s += H * W * 3
    host = np.asarray(rows, dtype=np.int64).reshape(-1, cols)
    return {"img_tab": ops.to_device_async(rows, device), "img_tab_host": host, "tab": ar.dev, "tab_host": ar.host, "size": S, "full": full,
            "sizes": [(int(H), int(W)) for H, W in sizes], "src_off": src_off, "src_bytes": s, "geometry": geo}


def run_pipeline(images_u8, params, chain, want_u8=False, device=None):
    """images_u8: list of uint8 [H, W, 3] tensors (all host or all device) + their parameters -> dict: 'images' fp32 [B, 3, S, S], 'u8'
    (want_u8) uint8 [B, S, S, 3] = the bytes before normalisation and erasing, 'plan'."""
    from . import ops
    if not images_u8:
        raise ValueError("train transforms: an empty batch")
    if device is None:
        device = images_u8[0].device if images_u8[0].is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("simseg_amd.pipeline.run_pipeline runs on MI355X only; there is no CPU fallback (apply_pipeline_pil is the "
                           "host statement)")
    lut_dev = preproc._lut_on(chain["lut"], device)
    pl = plan_pipeline([tuple(t.shape[:2]) for t in images_u8], params, chain, device)
    src = preproc._pack(images_u8, pl, device)
    out, u8 = (ops.train_chain if pl["full"] else ops.train_transforms)(src, pl, lut_dev, want_u8=want_u8)
    res = {"images": out, "plan": pl}
    if want_u8:
        res["u8"] = u8
    return res


class TrainPipeline:
    """A batch of raw uint8 [H, W, 3] images + a numpy Generator -> sample_pipeline_params -> run_pipeline -> fp32 [B, 3, S, S] on the
    device."""

    def __init__(self, chain):
        self.chain, self.size = chain, chain["size"]

    def sample(self, sizes, rng):
        return sample_pipeline_params(sizes, rng, self.chain)

    def __call__(self, images_u8, rng, want_u8=False, device=None):
        params = self.sample([tuple(t.shape[:2]) for t in images_u8], rng)
        res = run_pipeline(images_u8, params, self.chain, want_u8=want_u8, device=device)
        res["params"] = params
        return res

    def __repr__(self):
        return f"TrainPipeline({self.chain['names']}, size={self.size}, erase={self.chain['erase']})"
