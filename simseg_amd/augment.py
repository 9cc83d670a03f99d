"""Device-side training augmentation: RandomResizedCrop(size, scale) + the ImageNet AutoAugment policy on decoded uint8 [H, W, 3]
images, bit-identical to the same parameters applied with Pillow (apply_pil), in TWO launches per batch (csrc/augment.hip).

The host samples every random choice (sample_params: crop box, sub-policy, apply flags, signs) from a numpy Generator; the device only
applies them.  DESIGN.md "Device-side training augmentation" states the sampling and each op's arithmetic; apply_pil is the oracle.

Launch 1 crops and resizes (Pillow's bilinear uint8 resample: the axis tables of simseg_amd.preproc, read through a source row pitch)
into a uint8 [S, S, 3] scratch per image.  Launch 2 runs one workgroup per image: the image sits in LDS when it fits (S <= 230, so the
shipped S = 224), else it is worked on in global memory; it applies op1 and op2 and writes the normalised fp32 [3, S, S] planes through
the same [3, 256] look-up table as preproc.make_lut."""
import math
import struct

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageOps

from . import preproc

# ---- the policy, restated as data ---------------------------------------------------------------------------------------------------------
OPS = ("none", "posterize", "solarize", "invert", "autocontrast", "equalize", "color", "contrast", "sharpness", "rotate", "shearX")
OP_CODE = {name: i for i, name in enumerate(OPS)}
SIGNED = ("color", "contrast", "sharpness", "shearX")        # a sign +-1 is drawn when one of these is applied
# magnitude index 0..9 -> magnitude, per op (the policy's ranges; posterize is the number of bits kept, rounded to int)
MAGNITUDES = {
    "shearX": np.linspace(0, 0.3, 10),
    "rotate": np.linspace(0, 30, 10),
    "color": np.linspace(0.0, 0.9, 10),
    "posterize": [int(v) for v in np.round(np.linspace(8, 4, 10), 0)],
    "solarize": np.linspace(256, 0, 10),
    "contrast": np.linspace(0.0, 0.9, 10),
    "sharpness": np.linspace(0.0, 0.9, 10),
    "autocontrast": [0] * 10,
    "equalize": [0] * 10,
    "invert": [0] * 10,
}
# the 25 sub-policies: (p1, op1, magnitude index 1, p2, op2, magnitude index 2)
POLICY = (
    (0.4, "posterize", 8, 0.6, "rotate", 9),
    (0.6, "solarize", 5, 0.6, "autocontrast", 5),
    (0.8, "equalize", 8, 0.6, "equalize", 3),
    (0.6, "posterize", 7, 0.6, "posterize", 6),
    (0.4, "equalize", 7, 0.2, "solarize", 4),
    (0.4, "equalize", 4, 0.8, "rotate", 8),
    (0.6, "solarize", 3, 0.6, "equalize", 7),
    (0.8, "posterize", 5, 1.0, "equalize", 2),
    (0.2, "rotate", 3, 0.6, "solarize", 8),
    (0.6, "equalize", 8, 0.4, "posterize", 6),
    (0.8, "rotate", 8, 0.4, "color", 0),
    (0.4, "rotate", 9, 0.6, "equalize", 2),
    (0.0, "equalize", 7, 0.8, "equalize", 8),
    (0.6, "invert", 4, 1.0, "equalize", 8),
    (0.6, "color", 4, 1.0, "contrast", 8),
    (0.8, "rotate", 8, 1.0, "color", 2),
    (0.8, "color", 8, 0.8, "solarize", 7),
    (0.4, "sharpness", 7, 0.6, "invert", 8),
    (0.6, "shearX", 5, 1.0, "equalize", 9),
    (0.4, "color", 0, 0.6, "equalize", 3),
    (0.4, "equalize", 7, 0.2, "solarize", 4),
    (0.6, "solarize", 5, 0.6, "autocontrast", 5),
    (0.6, "invert", 4, 1.0, "equalize", 8),
    (0.6, "color", 4, 1.0, "contrast", 8),
    (0.8, "equalize", 8, 0.6, "equalize", 3),
)
FILL = 128                                                    # rotate and shearX fill (grey)

# ---- parameters ---------------------------------------------------------------------------------------------------------------------------
FIELDS = ("top", "left", "h", "w", "fallback", "policy", "op1", "mag1", "apply1", "sign1", "op2", "mag2", "apply2", "sign2")
_FLOAT_FIELDS = ("mag1", "mag2")


def _params(rows):
    """list of per-image dicts -> dict of column arrays (FIELDS)."""
    return {f: np.array([r[f] for r in rows], dtype=np.float64 if f in _FLOAT_FIELDS else np.int64) for f in FIELDS}


def take(params, idx):
    """The parameters of images idx (a list of indices), in that order."""
    idx = np.asarray(idx, dtype=np.int64)
    return {f: params[f][idx] for f in FIELDS}


def crop_box(rng, H, W, scale, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop.get_params: -> (top, left, h, w, fallback).  Ten tries of (area fraction ~ U(scale), log-aspect ~ U(log ratio),
    w = round(sqrt(A r)), h = round(sqrt(A / r)), corner uniform); then the centre crop with the aspect ratio clamped into `ratio`."""
    area = H * W
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        r = math.exp(rng.uniform(lr0, lr1))
        w = int(round(math.sqrt(target * r)))
        h = int(round(math.sqrt(target / r)))
        if 0 < w <= W and 0 < h <= H:
            top = int(rng.integers(0, H - h + 1))
            left = int(rng.integers(0, W - w + 1))
            return top, left, h, w, 0
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w, 1


def sample_params(sizes, rng, scale=(0.6, 1.0), autoaug=True):
    """sizes [(H, W)] of the raw images + a numpy Generator -> the batch's parameters (dict of FIELDS columns).  Per image: the crop box,
    then (autoaug) the sub-policy index ~ U{0..24}, then for op1 and op2 in turn: applied iff U[0, 1) < p, and for a signed op that is
    applied a sign ~ U{-1, +1}.  The same generator state gives the same parameters."""
    rows = []
    for H, W in sizes:
        top, left, h, w, fb = crop_box(rng, int(H), int(W), scale)
        r = {"top": top, "left": left, "h": h, "w": w, "fallback": fb, "policy": -1, "op1": 0, "mag1": 0.0, "apply1": 0, "sign1": 1,
             "op2": 0, "mag2": 0.0, "apply2": 0, "sign2": 1}
        if autoaug:
            draw_autoaug(rng, r)
        rows.append(r)
    return _params(rows)


def draw_autoaug(rng, r):
    """One image's AutoAugment draws into its row r: the sub-policy, then per op the apply flag and (applied, signed) the sign."""
    k = int(rng.integers(0, len(POLICY)))
    p1, o1, m1, p2, o2, m2 = POLICY[k]
    r["policy"] = k
    for j, (p, op, mi) in enumerate(((p1, o1, m1), (p2, o2, m2)), 1):
        applied = rng.random() < p
        r[f"op{j}"] = OP_CODE[op]
        r[f"mag{j}"] = float(MAGNITUDES[op][mi])
        r[f"apply{j}"] = int(applied)
        if applied and op in SIGNED:
            r[f"sign{j}"] = 1 if rng.integers(0, 2) else -1


def explicit_params(boxes, op1="none", mag1=0.0, sign1=1, op2="none", mag2=0.0, sign2=1):
    """Parameters that apply the given ops (always) to every image, for tests and tools: boxes [(top, left, h, w)]."""
    rows = [{"top": t, "left": l, "h": h, "w": w, "fallback": 0, "policy": -1, "op1": OP_CODE[op1], "mag1": float(mag1),
             "apply1": int(op1 != "none"), "sign1": int(sign1), "op2": OP_CODE[op2], "mag2": float(mag2), "apply2": int(op2 != "none"),
             "sign2": int(sign2)} for t, l, h, w in boxes]
    return _params(rows)


# ---- the host reference -------------------------------------------------------------------------------------------------------------------
def _rotate(img, deg):
    rot = img.convert("RGBA").rotate(deg)
    return Image.composite(rot, Image.new("RGBA", rot.size, (FILL,) * 4), rot).convert(img.mode)


_PIL = {
    "posterize": lambda img, m, s: ImageOps.posterize(img, int(m)),
    "solarize": lambda img, m, s: ImageOps.solarize(img, m),
    "invert": lambda img, m, s: ImageOps.invert(img),
    "autocontrast": lambda img, m, s: ImageOps.autocontrast(img),
    "equalize": lambda img, m, s: ImageOps.equalize(img),
    "color": lambda img, m, s: ImageEnhance.Color(img).enhance(1 + m * s),
    "contrast": lambda img, m, s: ImageEnhance.Contrast(img).enhance(1 + m * s),
    "sharpness": lambda img, m, s: ImageEnhance.Sharpness(img).enhance(1 + m * s),
    "rotate": lambda img, m, s: _rotate(img, m),
    "shearX": lambda img, m, s: img.transform(img.size, Image.AFFINE, (1, m * s, 0, 0, 1, 0), Image.BICUBIC, fillcolor=(FILL,) * 3),
}


def apply_pil_u8(img, params, i, size):
    """Image i's parameters applied with Pillow's own calls: crop, bilinear resize to size x size, op1, op2 -> the PIL image."""
    t, l, h, w = (int(params[f][i]) for f in ("top", "left", "h", "w"))
    img = img.convert("RGB").crop((l, t, l + w, t + h)).resize((size, size), Image.BILINEAR)
    for j in (1, 2):
        if params[f"apply{j}"][i] and params[f"op{j}"][i]:
            img = _PIL[OPS[int(params[f"op{j}"][i])]](img, float(params[f"mag{j}"][i]), int(params[f"sign{j}"][i]))
    return img


def apply_pil(img, params, i, size, mean, std):
    """The host route (the oracle of every device test): apply_pil_u8, then the host tail _to_tensor + normalize -> (fp32 [3, S, S],
    uint8 [S, S, 3])."""
    from simseg.transforms import _to_tensor
    out = apply_pil_u8(img, params, i, size)
    m = torch.tensor(mean).view(-1, 1, 1)
    s = torch.tensor(std).view(-1, 1, 1)
    return (_to_tensor(out) - m) / s, np.asarray(out, dtype=np.uint8)


# ---- plan: per-image rows + axis tables -------------------------------------------------------------------------------------------------
AUG_COLS = 30                     # int64 columns of the image table (include/simseg_hip.h simseg_train_augment)
OP_SLOTS = 8                      # int64 parameter slots per op
(C_SRC, C_H, C_W, C_TOP, C_LEFT, C_CH, C_CW, C_HOFF, C_HKS, C_VOFF, C_VKS, C_RSV, C_OP1, C_OP2) = range(14)
C_P1, C_P2 = 14, 14 + OP_SLOTS


def _f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def _f64_bits(v):
    return struct.unpack("<q", struct.pack("<d", float(v)))[0]


def _fix16(v):
    """Pillow's 16.16 fixed point of an affine coefficient: floor(v * 65536 + 0.5) (ties round up, not to even)."""
    return int(math.floor(v * 65536.0 + 0.5))


def rotate_matrix(deg, S):
    """Image.rotate's inverse matrix for an S x S image about its centre, as Pillow builds it."""
    ang = -math.radians(deg % 360.0)
    m = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
    cx = cy = S / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def op_slots(op, mag, sign, S):
    """-> OP_SLOTS int64 parameters of one op as the kernel reads them (DESIGN.md lists each)."""
    p = [0] * OP_SLOTS
    name = OPS[op]
    if name == "posterize":
        p[0] = ~(2 ** (8 - int(mag)) - 1) & 255                     # the mask Pillow ANDs each byte with
    elif name == "solarize":
        p[0] = sum(1 for i in range(256) if i < mag)                # bytes below this are kept, the others inverted
    elif name in ("color", "contrast", "sharpness"):
        p[0] = _f32_bits(np.float32(1 + mag * sign))                # Image.blend's factor, a C float
    elif name == "rotate":
        a = rotate_matrix(mag, S)
        p[:6] = [_fix16(a[0]), _fix16(a[1]), _fix16(a[3]), _fix16(a[4]), _fix16(a[2] + a[1] * 0.5 + a[0] * 0.5),
                 _fix16(a[5] + a[4] * 0.5 + a[3] * 0.5)]
        if (mag % 360.0) in (90.0, 180.0, 270.0):
            raise NotImplementedError(f"rotate by {mag} degrees: Pillow transposes there instead of resampling (no policy uses it)")
    elif name == "shearX":
        p[:6] = [_f64_bits(v) for v in (1.0, mag * sign, 0.0, 0.0, 1.0, 0.0)]
    return p


def plan(sizes, params, size, device):
    """sizes [(H, W)] of the raw images + their parameters -> dict: img_tab (device int64 [B, AUG_COLS]) + its host copy, the axis tables
    (preproc's per-device arena and its host mirror), src_off / src_bytes of the packed raw images, sizes."""
    from . import ops
    S = int(size)
    if not 32 <= S <= 384:
        raise ValueError(f"augment: the output size is 32 .. 384, got {S}")
    B = len(sizes)
    if B < 1 or any(len(params[f]) != B for f in FIELDS):
        raise ValueError(f"augment: {B} images and parameters for {[len(params[f]) for f in FIELDS]}")
    axes = set()
    for i in range(B):
        axes.add((int(params["w"][i]), S, "bilinear"))
        axes.add((int(params["h"][i]), S, "bilinear"))
    ar = preproc._arena(axes, device)
    rows, src_off, s = [], [], 0
    for i, (H, W) in enumerate(sizes):
        H, W = int(H), int(W)
        t, l, h, w = (int(params[f][i]) for f in ("top", "left", "h", "w"))
        if not (0 <= t and 0 <= l and 0 < h and 0 < w and t + h <= H and l + w <= W):
            raise ValueError(f"augment: image {i}: crop box {(t, l, h, w)} does not lie inside its {H} x {W} image")
        hoff, hks = ar.where[(w, S, "bilinear")]
        voff, vks = ar.where[(h, S, "bilinear")]
        row = [s, H, W, t, l, h, w, hoff, hks, voff, vks, 0]
        slots = []
        for j in (1, 2):
            op = int(params[f"op{j}"][i]) if params[f"apply{j}"][i] else 0
            if not 0 <= op < len(OPS):
                raise ValueError(f"augment: image {i}: op code {op}")
            row.append(op)
            slots += op_slots(op, float(params[f"mag{j}"][i]), int(params[f"sign{j}"][i]), S)
        rows.append(row + slots)
        src_off.append(s)
        s += H * W * 3
    host = np.asarray(rows, dtype=np.int64).reshape(-1, AUG_COLS)
    return {"img_tab": ops.to_device_async(rows, device), "img_tab_host": host, "tab": ar.dev, "tab_host": ar.host, "size": S,
            "sizes": [(int(H), int(W)) for H, W in sizes], "src_off": src_off, "src_bytes": s}


def augment(images_u8, params, lut, size, want_u8=False, device=None):
    """images_u8: list of uint8 [H, W, 3] tensors (all host or all device) + their parameters -> dict: 'images' fp32 [B, 3, S, S]
    (lut [3, 256]: byte -> normalised value per channel, preproc.make_lut), 'u8' (want_u8) uint8 [B, S, S, 3], 'plan'."""
    from . import ops
    if not images_u8:
        raise ValueError("augment: an empty batch")
    if device is None:
        device = images_u8[0].device if images_u8[0].is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("simseg_amd.augment.augment runs on MI355X only; there is no CPU fallback (apply_pil is the host statement)")
    lut_dev = preproc._lut_on(lut, device)
    pl = plan([tuple(t.shape[:2]) for t in images_u8], params, size, device)
    src = preproc._pack(images_u8, pl, device)
    out, u8 = ops.train_augment(src, pl, lut_dev, want_u8=want_u8)
    res = {"images": out, "plan": pl}
    if want_u8:
        res["u8"] = u8
    return res


class TrainAugment:
    """A batch of raw uint8 [H, W, 3] images + a numpy Generator -> sample_params -> augment -> fp32 [B, 3, S, S] on the device."""

    def __init__(self, size, scale, autoaug, lut):
        self.size, self.scale, self.autoaug, self.lut = int(size), (float(scale[0]), float(scale[1])), bool(autoaug), lut

    def sample(self, sizes, rng):
        return sample_params(sizes, rng, scale=self.scale, autoaug=self.autoaug)

    def __call__(self, images_u8, rng, want_u8=False, device=None):
        params = self.sample([tuple(t.shape[:2]) for t in images_u8], rng)
        res = augment(images_u8, params, self.lut, self.size, want_u8=want_u8, device=device)
        res["params"] = params
        return res

    def __repr__(self):
        return f"TrainAugment(size={self.size}, scale={self.scale}, autoaug={self.autoaug})"
