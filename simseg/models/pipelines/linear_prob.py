"""`LinearProbModel` with the reference's attribute / method / state-dict surface (simseg/models/pipelines/linear_prob.py:12-104): a ViT
image encoder - frozen by the shipped recipe - and one nn.Linear on its [cls] token, trained with cross-entropy; the standard score of
the encoder a contrastive run produced.

state-dict keys: image_encoder.model.model.* (timm names; the same ImageEncoder and key layout as pipelines/clip.py, so
`ckpt.only_load_image_encoder` loads the image tower of a SimSeg checkpoint), classifier.weight, classifier.bias.

On the device the head is one autograd node, simseg_amd.probe.ProbeHeadFn: fp32 logits from the fp32 master weights, the fused
cross-entropy / top-k / logit-gradient rows, fp32 weight and bias gradients.  Logits and gradients of the head are fp32 whatever 16-bit
type the encoder computes in, so this task uses no loss scaling.  A Mixup / CutMix batch (simseg_amd.mixup.Mixup.apply: `label_b`, `lam`
and `smoothing` beside `label`) takes the same head against its two-label soft target, SoftProbeHeadFn; the accuracies stay those against
`label`, the samples' own labels."""
import os

import torch
import torch.nn as nn

from simseg.models.pipelines.builder import PIPELINE
from simseg.utils import ENV

from .clip import ImageEncoder


class LinearProbModel(nn.Module):
    def __init__(self, cfg, rank):
        super().__init__()
        self.cfg = cfg
        self.image_encoder = ImageEncoder(cfg)
        if not cfg.model.classifier.num_classes > 0:
            raise AssertionError("model.classifier.num_classes must be positive")
        self.image_pool = nn.Identity()
        self.classifier = nn.Linear(cfg.model.image_encoder.embedding_dim, cfg.model.classifier.num_classes)
        if cfg.loss.extra_losses:
            raise NotImplementedError(f"linear_prob: extra losses {cfg.loss.extra_losses} are not on the path")
        amp = os.environ.get("SIMSEG_AMD_AMP_DTYPE", "bf16").lower().replace("torch.", "")
        self.amp_dtype = torch.float16 if amp in ("fp16", "float16", "half") else torch.bfloat16

    def train(self, mode=True):
        """A frozen encoder stays in eval() mode whatever the model's mode (and runs under torch.no_grad(): forward_image_feature)."""
        nn.Module.train(self, mode)
        if not self.image_encoder.trainable:
            self.image_encoder.eval()
        return self

    def forward_image_feature(self, image):
        """[B, 3, H, W] -> the [cls] row [B, D] when model.image_encoder.vit.only_cls_token is set, else every token [B, 1 + N, D].
        The encoder computes in the 16-bit type when cfg.dist.fp16 is set (bf16, or SIMSEG_AMD_AMP_DTYPE); a frozen one (`trainable:
        False`) runs under torch.no_grad(), so its parameters never get a .grad and nothing is saved for a backward."""
        frozen = not self.image_encoder.trainable
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=bool(self.cfg.dist.fp16) and image.is_cuda):
            if frozen:
                with torch.no_grad():
                    feats = self.image_pool(self.image_encoder(image))
            else:
                feats = self.image_pool(self.image_encoder(image))
        if self.cfg.model.image_encoder.vit.only_cls_token and feats.dim() == 3:
            feats = feats[:, 0]
        return feats

    def _head(self, batch):
        """A batch that carries `label_b` and `lam` (simseg_amd.mixup.Mixup.apply) takes the soft-target head with `smoothing` from the
        batch (default 0); any other batch takes ProbeHeadFn, and the soft path is not even imported."""
        feats = self.forward_image_feature(batch["image"])
        if "label_b" in batch and "lam" in batch:
            from simseg_amd.probe import SoftProbeHeadFn
            return SoftProbeHeadFn.apply(feats, self.classifier.weight, self.classifier.bias, batch["label"], batch["label_b"], batch["lam"],
                                         float(batch.get("smoothing", 0.0)))
        from simseg_amd.probe import ProbeHeadFn
        return ProbeHeadFn.apply(feats, self.classifier.weight, self.classifier.bias, batch["label"])

    def forward(self, batch, valid=False, **kwargs):
        """-> ({'<loss.name>_loss'.lower(): loss}, acc1, acc5) with the accuracies in percent as tensors of shape [1] (the reference's
        `accuracy`); valid=True -> (loss_dict, prediction [B, C], label)."""
        loss, out3, logits = self._head(batch)
        loss_dict = {f"{self.cfg.loss.name}_loss".lower(): loss}
        if valid:
            return loss_dict, logits, batch["label"]
        scale = 100.0 / batch["label"].shape[0]
        return loss_dict, out3[1:2] * scale, out3[2:3] * scale

    @torch.no_grad()
    def eval_counts(self, batch):
        """float64 [3] on the device: {sum of the batch's loss rows, top-1 hits, top-5 hits} - what an evaluation pass accumulates
        (simseg_amd.probe.LinearProbeTrainer.evaluate) without reading anything back per batch."""
        _, out3, _ = self._head(batch)
        tot = out3.double()
        tot[0] *= batch["label"].shape[0]
        return tot


@PIPELINE.register_obj
def linear_prob(cfg):
    return LinearProbModel(cfg, ENV.rank)
