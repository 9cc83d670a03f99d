"""`timm_modelzoo` backbone (mirror of simseg/models/backbones/mml/timm_builder.py:7-21): timm.create_model(tag, num_classes=0) called as
a whole model.  For the ViT tags this package knows that is the token-pooled feature: the [cls] row [B, D] of the tokens after the final
LayerNorm - the same MI355X-native tower and parameter names (model.model.*) as `vit_modelzoo`, so the image tower of a SimSeg
checkpoint loads into it.  The linear-probe recipe (configs/linear_prob/imagenet.yaml) names this backbone."""
import torch.nn as nn

from simseg_amd.nn import ViT

from ..builder import BACKBONE
from ._weights import maybe_load_pretrained

__all__ = ["TimmModel", "timm_modelzoo"]


class TimmModel(nn.Module):
    def __init__(self, cfg, img_size=224, **kwargs):
        super().__init__()
        tag = cfg.model.image_encoder.tag
        if "vit" not in tag:
            raise NotImplementedError(f"timm_modelzoo: {tag!r} is not a ViT; only the ViT tower is on the MI355X path")
        self.model = ViT(tag, img_size=img_size)
        if cfg.model.image_encoder.pretrained:
            maybe_load_pretrained(self.model, tag)

    def forward(self, x):
        return self.model(x)[:, 0]


@BACKBONE.register_obj
def timm_modelzoo(cfg, **kwargs):
    return TimmModel(cfg, **kwargs)
