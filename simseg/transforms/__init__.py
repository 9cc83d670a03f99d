"""Eval-time image transforms with the reference's builder API (simseg/transforms/mml/transforms.py:74-93) but without
torchvision (absent here): PIL resampling + torch tensors.  build_transforms / build_device_transforms do not provide the training-time
augmentations (autoaug, random_resize_crop, random erasing) and raise for them; build_train_augmentation is their route: the host decodes,
the parameters are sampled on the host, and crop, resize, AutoAugment and normalisation run on the device (simseg_amd/augment.py).
build_device_transforms is the eval-time route that leaves only the decode on the host: resize, crop and normalisation run on the device
(simseg_amd/preproc.py).  build_train_pipeline is the general training route: every train_transforms list of the grammar
list := geometry+ colour* (geometry: resize | resize_bicubic | random_resize_crop | center_crop | random_crop | random_flip; colour:
autoaug | color_jitter), plus random erasing when transforms.random_erasing.reprob > 0, sampled on the host and applied on the device
in two launches (simseg_amd/pipeline.py); the three other builders keep their behaviour.  build_train_views is build_train_pipeline for
the whole registry: color_distortion and gaussian_blur (the SimCLR pair) join the colour ops, any order, each at most once."""
import numpy as np
import torch
from PIL import Image

from simseg.utils import logger
from simseg.utils.registry import Registry

__all__ = ["TRANSFORMS", "build_transforms", "build_device_transforms", "build_train_augmentation", "build_train_pipeline",
           "build_train_views"]

TRANSFORMS = Registry("TRANSFORMS")


class Compose:
    def __init__(self, ops):
        self.ops = ops

    def __call__(self, x):
        for op in self.ops:
            x = op(x)
        return x

    def __repr__(self):
        return "Compose(" + ", ".join(getattr(o, "__name__", o.__class__.__name__) for o in self.ops) + ")"


@TRANSFORMS.register_obj
def resize(cfg, **kwargs):
    size = cfg.transforms.resize.size

    def resize_op(img):                       # torchvision Resize((s, s)) on PIL: bilinear
        return img.resize((size, size), Image.BILINEAR)
    return resize_op


@TRANSFORMS.register_obj
def resize_bicubic(cfg, **kwargs):
    size = cfg.transforms.resize_bicubic.size

    def resize_bicubic_op(img):               # Resize(size, interpolation=BICUBIC): shorter side -> size
        w, h = img.size
        if w <= h:
            return img.resize((size, max(1, round(h * size / w))), Image.BICUBIC)
        return img.resize((max(1, round(w * size / h)), size), Image.BICUBIC)
    return resize_bicubic_op


@TRANSFORMS.register_obj
def center_crop(cfg, **kwargs):
    size = cfg.transforms.center_crop.size

    def center_crop_op(img):
        w, h = img.size
        left, top = int(round((w - size) / 2.0)), int(round((h - size) / 2.0))
        return img.crop((left, top, left + size, top + size))
    return center_crop_op


def _to_tensor(img):
    a = np.asarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div_(255.0)


@TRANSFORMS.register_obj
def normalize(cfg, **kwargs):
    mean = torch.tensor(cfg.transforms.normalize.mean).view(-1, 1, 1)
    std = torch.tensor(cfg.transforms.normalize.std).view(-1, 1, 1)

    def normalize_op(t):
        return (t - mean) / std
    return normalize_op


def build_transforms(cfg, mode="train"):
    names = cfg.transforms.train_transforms if mode == "train" else cfg.transforms.valid_transforms
    ops = []
    for name in names:
        factory = TRANSFORMS.get(name)
        if factory is None:
            raise NotImplementedError(f"transform {name!r} is a training-time augmentation outside the accelerated path; "
                                      f"available: {sorted(TRANSFORMS.obj_dict)}")
        ops.append(factory(cfg))
    ops.extend([_to_tensor, TRANSFORMS.get("normalize")(cfg)])
    t = Compose(ops)
    logger.emph(f"{mode} image transform is composed of:", t)
    return t


def _to_u8(img):
    a = np.asarray(img.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(a.copy())


def build_device_transforms(cfg, mode="valid"):
    """-> (host_op, spec) of the device route: host_op maps a PIL image to its uint8 [H, W, 3] tensor and nothing else; spec
    (simseg_amd.preproc.make_spec) names the resize, the optional centre crop and the normalisation that simseg_amd.preproc.preprocess
    applies on the device, with results bit-identical to build_transforms(cfg, mode)."""
    from simseg_amd.preproc import make_spec
    names = list(cfg.transforms.train_transforms if mode == "train" else cfg.transforms.valid_transforms)
    for name in names:
        if TRANSFORMS.get(name) is None:
            raise NotImplementedError(f"transform {name!r} is a training-time augmentation outside the accelerated path; "
                                      f"available: {sorted(TRANSFORMS.obj_dict)}")
    crop = None
    if names and names[-1] == "center_crop":
        crop = cfg.transforms.center_crop.size
        names = names[:-1]
    if names == ["resize"]:
        kind, size, filt = "square", cfg.transforms.resize.size, "bilinear"
    elif names == ["resize_bicubic"]:
        kind, size, filt = "short", cfg.transforms.resize_bicubic.size, "bicubic"
    else:
        raise NotImplementedError(f"the device route takes one resize (resize | resize_bicubic) and an optional center_crop after it, "
                                  f"got {list(cfg.transforms.train_transforms if mode == 'train' else cfg.transforms.valid_transforms)}")
    # the 256 byte values through the host route's own tensor arithmetic: the table IS that route's result per byte
    lut = TRANSFORMS.get("normalize")(cfg)(_to_tensor(np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)))
    spec = make_spec(kind, size, filt, crop=crop, mean=list(cfg.transforms.normalize.mean), std=list(cfg.transforms.normalize.std),
                     lut=lut.reshape(3, 256).contiguous())
    logger.emph(f"{mode} image transform on the device:", {k: v for k, v in spec.items() if k != "lut"})
    return _to_u8, spec


def _normalize_lut(cfg):
    """The 256 byte values through the host route's own tensor arithmetic: the table IS that route's result per byte."""
    lut = TRANSFORMS.get("normalize")(cfg)(_to_tensor(np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)))
    return lut.reshape(3, 256).contiguous()


def build_train_augmentation(cfg):
    """-> (host_op, augment) of the training route: host_op maps a PIL image to its uint8 [H, W, 3] tensor and nothing else; augment
    (simseg_amd.augment.TrainAugment), given a batch of those tensors and a numpy Generator, samples RandomResizedCrop and AutoAugment
    parameters on the host and returns the augmented, normalised fp32 [B, 3, S, S] batch from the device.  Accepts train_transforms
    [random_resize_crop, autoaug] or [random_resize_crop]."""
    from simseg_amd.augment import TrainAugment
    names = list(cfg.transforms.train_transforms)
    if names not in (["random_resize_crop", "autoaug"], ["random_resize_crop"]):
        raise NotImplementedError(f"the training augmentation route takes train_transforms [random_resize_crop, autoaug] or "
                                  f"[random_resize_crop], got {names}")
    rrc = cfg.transforms.random_resize_crop
    aug = TrainAugment(rrc.size, tuple(rrc.scale), autoaug=len(names) == 2, lut=_normalize_lut(cfg))
    logger.emph("train image augmentation on the device:", aug)
    return _to_u8, aug


def build_train_pipeline(cfg):
    """-> (host_op, pipeline) of the general training route: host_op maps a PIL image to its uint8 [H, W, 3] tensor and nothing else;
    pipeline (simseg_amd.pipeline.TrainPipeline), given a batch of those tensors and a numpy Generator, samples every random choice of
    cfg.transforms.train_transforms (and of random erasing, when its reprob > 0) on the host and returns the transformed, normalised fp32
    [B, 3, S, S] batch from the device.  A list outside the grammar raises NotImplementedError naming the rule it breaks."""
    from simseg_amd.pipeline import TrainPipeline, parse_chain
    pipe = TrainPipeline(parse_chain(list(cfg.transforms.train_transforms), cfg, lut=_normalize_lut(cfg)))
    logger.emph("train image transforms on the device:", pipe)
    return _to_u8, pipe


def build_train_views(cfg):
    """build_train_pipeline for the whole registry: the grammar list := geometry+ pixel* with pixel := autoaug | color_jitter |
    color_distortion | gaussian_blur (the SimCLR pair under transforms.color_distortion.strength and transforms.gaussian_blur.{p,
    radius_min, radius_max}; strength 1.0 and p 0.5, radii 0.1 .. 2.0 where the config has no such keys).  -> (host_op, pipeline) as
    build_train_pipeline; a list of the old grammar gives the same parameters and the same bytes as build_train_pipeline's."""
    from simseg_amd.pipeline import TrainPipeline, parse_chain
    pipe = TrainPipeline(parse_chain(list(cfg.transforms.train_transforms), cfg, lut=_normalize_lut(cfg), full=True))
    logger.emph("train image views on the device:", pipe)
    return _to_u8, pipe


def build_mixup(cfg):
    """-> simseg_amd.mixup.Mixup from cfg.transforms.{mixup, cutmix, cutmix_minmax, mixup_prob, mixup_switch_prob, mixup_mode},
    cfg.loss.smoothing and cfg.model.classifier.num_classes (timm's Mixup arguments under the reference's key names), or None when both
    alphas are 0.  Called explicitly by a data loop that wants mixing, as build_train_pipeline is: the task defaults carry mixup = 0.8 and
    cutmix = 1.0, and nothing enables mixing from the config on its own."""
    t = cfg.transforms
    if not (t.mixup > 0 or t.cutmix > 0 or t.cutmix_minmax is not None):
        return None
    from simseg_amd.mixup import Mixup
    minmax = None if t.cutmix_minmax is None else tuple(t.cutmix_minmax)
    mix = Mixup(mixup_alpha=t.mixup, cutmix_alpha=t.cutmix, cutmix_minmax=minmax, prob=t.mixup_prob, switch_prob=t.mixup_switch_prob,
                mode=t.mixup_mode, label_smoothing=cfg.loss.smoothing, num_classes=cfg.model.classifier.num_classes)
    logger.emph("mixup / cutmix on the device:", mix)
    return mix
