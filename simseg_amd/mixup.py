"""Mixup / CutMix on the device (timm 0.6.13's `Mixup`, the batch-level transform of ViT fine-tuning recipes) and its two-label target.

  Mixup.sample(B, H, W, rng)      every random choice of one batch, drawn on the host from a numpy Generator -> params
  Mixup.apply(images, labels, p)  one async copy of the table, one launch (ops.mix_batch, in place) -> (images, target dict)
  explicit_params(...)            a table by hand (tests)
  mix_ref / soft_target_ref       the host statements of both laws (the counterpart of pipeline.apply_pipeline_pil)

Sample i is mixed with its partner j = B - 1 - i (x.flip(0)), so B is even.  params = {"table": int32 [B, 8], "lam": fp32 [B],
"smoothing": eps}; table[i] = {kind, yl, yh, xl, xh, lam bits, om bits, 0} with kind 0 = untouched, 1 = mixup, 2 = cutmix, the box as
rows [yl, yh) x columns [xl, xh), lam as fp32 and om = float32(1.0 - float64(lam)) formed HERE, so that the kernel has no freedom
(include/simseg_hip.h: simseg_mix_batch).  "lam" is the same column as fp32: the weight of the sample's own label.

The target never becomes a dense [B, C] tensor: apply() returns {"label", "label_b" = label.flip(0), "lam", "smoothing"}, which
LinearProbModel.forward hands to the fused soft-target head (ops.soft_ce_rows).

Draw order (per draw unit: the batch in mode "batch", pair (i, B-1-i) for i = 0 .. B/2-1 in mode "pair", sample 0 .. B-1 in mode
"elem"; it does not follow numpy's legacy global stream, which timm draws from):
  1. u = rng.random(): the unit is mixed when u < prob; otherwise kind 0, lam 1, and nothing more is drawn for it;
  2. only when both alphas are positive: v = rng.random(): cutmix when v < switch_prob (with one positive alpha its kind is taken);
  3. lam = rng.beta(alpha, alpha) with the chosen kind's alpha; a lam that is 1 as fp32 makes the unit kind 0 and ends its draws;
  4. cutmix without cutmix_minmax: cy = rng.integers(0, H), cx = rng.integers(0, W); cut_h = int(H * sqrt(1 - lam)), cut_w likewise;
     the edges are clip(c - cut // 2, 0, dim) and clip(c + cut // 2, 0, dim);
     cutmix with cutmix_minmax = (lo, hi): cut_h from [int(H * lo), int(H * hi)), cut_w from [int(W * lo), int(W * hi)), then yl from
     [0, H - cut_h) and xl from [0, W - cut_w), in this order, each by rng.integers - an EMPTY range [a, a) gives a without a draw
     (numpy's randint raises there; a 1 x 1 image must still be samplable);
  5. with correct_lam, or with cutmix_minmax, lam = 1 - box area / (H * W), in double, rounded to fp32."""
import math

import numpy as np
import torch

from . import ops

KIND_NONE, KIND_MIXUP, KIND_CUTMIX = 0, 1, 2
MODES = ("batch", "pair", "elem")


def _om(lam32):
    return np.float32(1.0 - float(lam32))


def _row(kind, lam, box=(0, 0, 0, 0)):
    lam32 = np.float32(lam)
    r = np.zeros(8, dtype=np.int32)
    r[0] = kind
    r[1:5] = box
    r[5:7] = np.array([lam32, _om(lam32)], dtype=np.float32).view(np.int32)
    return r


def _params(table, smoothing):
    table = np.ascontiguousarray(table, dtype=np.int32)
    return {"table": table, "lam": table[:, 5].copy().view(np.float32), "smoothing": float(smoothing)}


def explicit_params(kinds, lams, boxes=None, smoothing=0.0):
    """A table by hand: kinds[i] in {0, 1, 2}, lams[i] (rounded to fp32), boxes[i] = (yl, yh, xl, xh) (default: empty).  Nothing is
    checked here - the entry point checks every field on the host copy - so a test can also build a table that must be refused."""
    B = len(kinds)
    boxes = [(0, 0, 0, 0)] * B if boxes is None else boxes
    return _params(np.stack([_row(k, l, b) for k, l, b in zip(kinds, lams, boxes)]), smoothing)


def _randint(rng, lo, hi):
    return int(rng.integers(lo, hi)) if hi > lo else int(lo)


class Mixup:
    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch", correct_lam=True,
                 label_smoothing=0.0, num_classes=1000):
        if mode not in MODES:
            raise ValueError(f"Mixup: mode must be one of {MODES}, got {mode!r}")
        if mixup_alpha < 0 or cutmix_alpha < 0 or not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0 or not 0.0 <= label_smoothing < 1.0:
            raise ValueError("Mixup: alphas >= 0, prob and switch_prob in [0, 1], label_smoothing in [0, 1)")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.cutmix_minmax = None
        if cutmix_minmax is not None:
            lo, hi = cutmix_minmax
            if not 0.0 <= lo <= hi <= 1.0:
                raise ValueError(f"Mixup: cutmix_minmax = (lo, hi) with 0 <= lo <= hi <= 1, got {cutmix_minmax}")
            self.cutmix_minmax = (float(lo), float(hi))
            if self.cutmix_alpha == 0.0:
                self.cutmix_alpha = 1.0                   # (timm: minmax forces cutmix on)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.correct_lam, self.label_smoothing, self.num_classes = bool(correct_lam), float(label_smoothing), int(num_classes)

    def __repr__(self):
        return (f"Mixup(mixup_alpha={self.mixup_alpha}, cutmix_alpha={self.cutmix_alpha}, cutmix_minmax={self.cutmix_minmax}, prob={self.prob}, "
                f"switch_prob={self.switch_prob}, mode={self.mode!r}, correct_lam={self.correct_lam}, label_smoothing={self.label_smoothing}, "
                f"num_classes={self.num_classes})")

    def _draw(self, H, W, rng):
        """One draw unit -> a table row (the module docstring's order)."""
        if not rng.random() < self.prob or (self.mixup_alpha == 0.0 and self.cutmix_alpha == 0.0):
            return _row(KIND_NONE, 1.0)
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = bool(rng.random() < self.switch_prob)
        else:
            cut = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(rng.beta(alpha, alpha))
        if np.float32(lam) == np.float32(1.0):
            return _row(KIND_NONE, 1.0)
        if not cut:
            return _row(KIND_MIXUP, lam)
        if self.cutmix_minmax is None:
            cy, cx = _randint(rng, 0, H), _randint(rng, 0, W)
            ratio = math.sqrt(1.0 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
            xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
        else:
            lo, hi = self.cutmix_minmax
            cut_h, cut_w = _randint(rng, int(H * lo), int(H * hi)), _randint(rng, int(W * lo), int(W * hi))
            yl, xl = _randint(rng, 0, H - cut_h), _randint(rng, 0, W - cut_w)
            yh, xh = yl + cut_h, xl + cut_w
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1.0 - ((yh - yl) * (xh - xl)) / float(H * W)
        return _row(KIND_CUTMIX, lam, (yl, yh, xl, xh))

    def sample(self, B, H, W, rng):
        if B < 2 or B % 2:
            raise ValueError(f"Mixup: a batch is mixed with its flipped self in pairs (i, B-1-i), so its size must be even (got {B})")
        if self.mode == "batch":
            table = np.tile(self._draw(H, W, rng), (B, 1))
        elif self.mode == "pair":
            half = np.stack([self._draw(H, W, rng) for _ in range(B // 2)])
            table = np.concatenate([half, half[::-1]])
        else:
            table = np.stack([self._draw(H, W, rng) for _ in range(B)])
        return _params(table, self.label_smoothing)

    def apply(self, images, labels, params):
        """images [B, C, H, W] on the device, mixed IN PLACE; labels int64 [B] on the device.  One pinned host-to-device copy carries the
        table and, behind it, the lam column as its own contiguous vector; one launch mixes.  -> (images, {"label": labels, "label_b":
        labels.flip(0), "lam": fp32 [B] on the device, "smoothing": eps})."""
        table = params["table"]
        B = table.shape[0]
        buf = ops.to_device_async(np.concatenate([table.reshape(-1), table[:, 5]]), images.device, dtype=torch.int32)
        ops.mix_batch(images, buf[:8 * B].view(B, 8), table)
        return images, {"label": labels, "label_b": labels.flip(0), "lam": buf[8 * B:].view(torch.float32), "smoothing": params["smoothing"]}

    def __call__(self, images, labels, rng):
        return self.apply(images, labels, self.sample(images.shape[0], images.shape[2], images.shape[3], rng))


# ---- host statements ------------------------------------------------------------------------------------------------------------------
def mix_ref(images_cpu, params):
    """The law of simseg_mix_batch in torch ops on the host, from a COPY of the original batch (so that a partner's original values are
    read whatever has been written): kind 1 as two fp32 products and an fp32 sum rounded once to the storage type, kind 2 as a box
    assignment, kind 0 untouched.  -> a new tensor of the input's dtype."""
    x0 = images_cpu.detach().clone()
    out = x0.clone()
    table = params["table"]
    B = x0.shape[0]
    fl = table[:, 5:7].copy().view(np.float32)
    for i in range(B):
        j = B - 1 - i
        kind, yl, yh, xl, xh = (int(v) for v in table[i, :5])
        if kind == KIND_MIXUP:
            lam, om = torch.tensor(fl[i, 0]), torch.tensor(fl[i, 1])               # (fp32 0-dim tensors: fp32 products, no promotion)
            out[i] = (x0[i].float() * lam + x0[j].float() * om).to(x0.dtype)
        elif kind == KIND_CUTMIX:
            out[i, :, yl:yh, xl:xh] = x0[j, :, yl:yh, xl:xh]
    return out


def soft_target_ref(labels, params, C, smoothing=None):
    """The dense target the two-label form stands for, in float64 [B, C]: timm's mixup_target, y1 * lam + y2 * (1 - lam) with y1 / y2 the
    one-hot rows of labels / labels.flip(0) at on = 1 - eps + eps / C, off = eps / C."""
    eps = params["smoothing"] if smoothing is None else smoothing
    labels = labels.detach().cpu().long()
    off = eps / C
    on = 1.0 - eps + off
    y1 = torch.full((labels.shape[0], C), off, dtype=torch.float64).scatter_(1, labels[:, None], on)
    y2 = torch.full((labels.shape[0], C), off, dtype=torch.float64).scatter_(1, labels.flip(0)[:, None], on)
    lam = torch.from_numpy(params["lam"].astype(np.float64))[:, None]
    return y1 * lam + y2 * (1.0 - lam)
