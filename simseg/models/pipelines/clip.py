"""The drop-in boundary: `CLIPModel` with the reference's attribute / method / state-dict surface
(simseg/models/pipelines/clip.py:13-229), computing on the MI355X-native towers and heads.

state-dict keys: image_encoder.model.model.* (timm names), text_encoder.model.model.* (HF names),
image_projection.linear.weight, text_projection.linear.weight, loss.temperature."""
import numpy as np
import os

import torch
import torch.nn as nn

from simseg.models.backbones.builder import BACKBONE
from simseg.models.criteria.losses.builder import LOSS
from simseg.models.pipelines.builder import PIPELINE
from simseg.utils import ENV, logger
from simseg_amd.heads import discard_prefetched, prefetch_gather
from simseg_amd.nn import compute_dtype
from simseg_amd.towers import ProjectPoolFn, packed_text

from ..components import AvgPooling, ComplexProjection, L2norm, MlpProjection, SimpleProjection, TopKPooling
from ..components.pooling import clip_k_to_shortest


class CLIPModel(nn.Module):
    def __init__(self, cfg, rank):
        super().__init__()
        self.cfg = cfg
        self.image_encoder = ImageEncoder(cfg)
        self.text_encoder = TextEncoder(cfg)
        self.random_seed = np.random.RandomState(seed=2021)
        heads = {"simple": SimpleProjection, "complex": ComplexProjection}
        if cfg.model.projection.name not in heads:
            raise NotImplementedError(cfg.model.projection.name)
        Head = heads[cfg.model.projection.name]
        self.image_projection = Head(cfg, embedding_dim=cfg.model.image_encoder.embedding_dim, projection_dim=cfg.model.projection.dim,
                                     trainable=cfg.model.projection.image_projector_trainable)
        self.text_projection = Head(cfg, embedding_dim=cfg.model.text_encoder.embedding_dim, projection_dim=cfg.model.projection.dim,
                                    trainable=cfg.model.projection.text_projector_trainable)
        if cfg.model.pool.name == "loda":
            self.text_pool = TopKPooling(cfg.model.pool.loda.text_k, dim=1)
            self.image_pool = TopKPooling(cfg.model.pool.loda.image_k, dim=1)
        elif cfg.model.pool.name == "avg":
            self.text_pool, self.image_pool = AvgPooling(), AvgPooling()
        else:
            self.text_pool, self.image_pool = nn.Identity(), nn.Identity()
        if cfg.loss.name == "NTXent":
            raise NotImplementedError("loss.name=NTXent cannot be a CLIPModel's main loss: the image and the text embeddings are not two views of one "
                                      "input (and the prefetched embedding gathers would never be taken).  Keep the image-text loss and call "
                                      "CLIPModel.enable_ssl() - or Trainer(ssl={...}) - for the two-view image branch")
        self.rank = rank
        self.loss = LOSS.get(cfg.loss.name)(cfg, rank)
        self.global_reduce = cfg.loss.global_reduce
        self.text_target_token_idx = cfg.model.text_encoder.target_token_idx
        self._fused_heads = cfg.model.pool.name == "loda" and cfg.model.projection.name == "simple"

    # ---- image side ---------------------------------------------------------------------------------------------
    def forward_image_feature(self, image):
        """[B,3,H,W] -> patch tokens [B,N,D] (pool != identity) or the [cls] token [B,D] (clip.py:65-84)."""
        feats = self.image_encoder(image)
        if self.cfg.model.pool.name == "identity":
            return feats[:, 0] if feats.dim() == 3 else feats
        return feats[:, 1:] if feats.dim() == 3 else feats

    def _image_embeddings(self, image):
        """forward_image_project(forward_image_feature(image)) for the training / embedding path.  With the fused heads the tower's whole
        output goes to ProjectPoolFn, which leaves the [cls] token out of the pooling itself (skip=1) - no slice copy of the features, no
        zero-filled scatter of their gradient, no cast (simseg_amd/towers.py ProjectPoolFn).  Same values as the two calls."""
        if self._fused_heads and self.cfg.model.pool.name != "identity" and os.environ.get("SIMSEG_AMD_FUSED_IMAGE_HEAD", "1") != "0":
            feats = self.image_encoder(image)
            if feats.dim() == 3 and feats.is_cuda:
                return ProjectPoolFn.apply(feats, self.image_projection.linear.weight, self.image_pool.k, None, compute_dtype(), 1)
            return self.forward_image_project(feats[:, 1:] if feats.dim() == 3 else feats)
        return self.forward_image_project(self.forward_image_feature(image))

    def forward_image_project(self, image_features):
        """projection -> LoDA pool -> L2norm: [B,N,D] -> [B,P] (clip.py:87-93), one fused node."""
        if self._fused_heads and image_features.dim() == 3:
            return ProjectPoolFn.apply(image_features, self.image_projection.linear.weight, self.image_pool.k, None, compute_dtype())
        emb = self.image_pool(self.image_projection(image_features))
        return L2norm(emb, dim=-1) if self.cfg.model.projection.name == "simple" else emb

    # ---- image self-supervision (SLIP: the image-text loss plus SimCLR's NT-Xent on two augmented views through the same image tower) ----
    def enable_ssl(self, scale=1.0, hidden_dim=4096, out_dim=256, temperature=0.1):
        """Switch the two-view image branch on - before the optimizer is built, so that its parameters are trained.  Adds
        `ssl_projection` (Linear(D, hidden_dim, bias) -> erf-GELU -> Linear(hidden_dim, out_dim, bias=False) on the [cls] token, one
        autograd node; its output goes through L2norm) and `ssl_loss` = NTXent at a constant `temperature`.  From then on forward(batch)
        with batch["image_ssl"] - a [2, B, 3, S, S] tensor or a pair of [B, 3, S, S] tensors: two outputs of
        simseg.transforms.build_train_views on the same raw batch - runs the image tower ONCE on cat([image, view 1, view 2]) (one backward
        per tower and step, which the gradient exchange and the lazy 16-bit residual gradients rely on), feeds rows [0, B) to the CLIP head
        as before and the [cls] tokens of rows [B, 3B) to the branch, and adds "ssl_loss" = scale * NT-Xent to the loss dict (its top-1
        accuracy of view 1's rows: self.ssl_acc).  Without the key, or for embeddings != False, forward is the one without the branch.
        The switch is per instance: forward and _image_embeddings of a model that never calls this are the class's own, untouched."""
        if getattr(self, "ssl_projection", None) is not None:
            raise RuntimeError("enable_ssl: the branch is already on")
        w = self.image_projection.linear.weight
        self.ssl_projection = MlpProjection(self.cfg.model.image_encoder.embedding_dim, int(hidden_dim), int(out_dim)).to(w.device)
        self.ssl_loss = LOSS.get("NTXent")(self.cfg, self.rank, temperature=temperature, learnable=False).to(w.device)
        self.ssl_scale, self.ssl_acc, self._ssl_views, self._ssl_z = float(scale), None, None, None
        self.forward = self._forward_ssl
        self._image_embeddings = self._image_embeddings_ssl
        return self

    def forward_image_ssl(self, image, views):
        """(CLIP image embeddings [B, P], view 1's and view 2's branch embeddings [B, out_dim] each) from ONE image-tower call on the 3B
        images cat([image, views[0], views[1]]).  Patch dropout, when on, applies to all 3B images; [cls] is never dropped."""
        B = image.shape[0]
        feats = self.image_encoder(torch.cat([image, views[0], views[1]]))
        if feats.dim() != 3:
            raise NotImplementedError("the image self-supervision branch reads the [cls] token: the image tower must return tokens [B, N, D]")
        head = feats[:B]
        if self.cfg.model.pool.name == "identity":
            img = self.forward_image_project(head[:, 0])
        elif self._fused_heads and feats.is_cuda and os.environ.get("SIMSEG_AMD_FUSED_IMAGE_HEAD", "1") != "0":
            sh16 = getattr(feats, "_simseg_fwd16", None)       # (the 16-bit copy the tower's last LayerNorm wrote: the head's rows of it)
            if sh16 is not None and sh16[1] == feats._version:
                head._simseg_fwd16 = (sh16[0][:B], head._version)
            img = ProjectPoolFn.apply(head, self.image_projection.linear.weight, self.image_pool.k, None, compute_dtype(), 1)
        else:
            img = self.forward_image_project(head[:, 1:])
        z = L2norm(self.ssl_projection(feats[B:, 0]), dim=-1)
        return img, z[:B], z[B:]

    def _image_embeddings_ssl(self, image):
        if self._ssl_views is None:
            return CLIPModel._image_embeddings(self, image)
        img, za, zb = self.forward_image_ssl(image, self._ssl_views)
        self._ssl_z = (za, zb)
        return img

    def _forward_ssl(self, batch, embeddings=False):
        views = batch.get("image_ssl") if embeddings is False and isinstance(batch, dict) else None
        if views is None:
            return CLIPModel.forward(self, batch, embeddings)
        if len(views) != 2 or tuple(views[0].shape) != tuple(batch["image"].shape) or tuple(views[1].shape) != tuple(batch["image"].shape):
            raise ValueError(f"image_ssl: two views of the batch's images, [2, B, 3, S, S] or a pair of [B, 3, S, S], for images {tuple(batch['image'].shape)}")
        self._ssl_views = views
        try:
            loss_dict, i2t_acc, t2i_acc = CLIPModel.forward(self, batch, embeddings)
            za, zb = self._ssl_z
        finally:
            self._ssl_views = self._ssl_z = None
        ssl, self.ssl_acc = self.ssl_loss(za, zb)
        loss_dict["ssl_loss"] = self.ssl_scale * ssl
        return loss_dict, i2t_acc, t2i_acc

    # ---- text side ----------------------------------------------------------------------------------------------
    def forward_text_feature(self, input_ids, attention_mask):
        feats = self.text_encoder(input_ids=input_ids, attention_mask=attention_mask)
        if self.cfg.model.pool.name == "identity":
            return feats[:, self.text_target_token_idx, :]
        return feats[:, self.text_target_token_idx:, :]

    def forward_text_project(self, text_features, attention_mask):
        if self.cfg.model.pool.name == "identity":
            emb = self.text_pool(self.text_projection(text_features))
            return L2norm(emb, dim=-1) if self.cfg.model.projection.name == "simple" else emb
        mask = attention_mask[:, self.text_target_token_idx:] if self.text_target_token_idx else attention_mask
        if self._fused_heads:
            k = clip_k_to_shortest(self.text_pool.k, mask)
            return ProjectPoolFn.apply(text_features, self.text_projection.linear.weight, k, mask.contiguous().long(), compute_dtype())
        emb = self.text_pool(self.text_projection(text_features), mask)
        return L2norm(emb, dim=-1) if self.cfg.model.projection.name == "simple" else emb

    # ---- loss / dispatch ----------------------------------------------------------------------------------------
    def _prefetch(self, emb, embeddings):
        """Start the global-batch all-gather of one tower's embeddings (the exchange step of mml_loss.py:60-64) as soon as they
        exist, so that it runs under the other tower instead of in front of the loss."""
        if embeddings is False and self.global_reduce and getattr(self.loss, "group", None) is not None:
            prefetch_gather(emb, self.loss.group)

    def forward_loss(self, image_embeddings, text_embeddings, ignore_mask=None, **loss_kwargs):
        """loss_kwargs go to both loss calls as they are (MixUpNCE's image_alpha / text_alpha: the reference's formula applies the same
        alpha_i and flipped target in both directions); a loss that takes keywords is not driven through `both`."""
        if (self.global_reduce and ignore_mask is None and not loss_kwargs and hasattr(self.loss, "both") and image_embeddings.is_cuda
                and os.environ.get("SIMSEG_AMD_FUSED_LOSS", "1") != "0"):
            # both directions as one node (same arithmetic and kernels as the two calls below: tests/test_gpu_model.py)
            loss, i2t_acc, t2i_acc = self.loss.both(image_embeddings, text_embeddings)
        elif self.global_reduce:
            i2t_loss, i2t_acc = self.loss(image_embeddings, text_embeddings, ignore_mask=ignore_mask, **loss_kwargs)
            t2i_loss, t2i_acc = self.loss(text_embeddings, image_embeddings, ignore_mask=ignore_mask, **loss_kwargs)
            loss = 0.5 * (i2t_loss + t2i_loss)
        else:
            loss, i2t_acc, t2i_acc = self.loss(image_embeddings, text_embeddings, ignore_mask=ignore_mask, **loss_kwargs)
        return {f"{self.cfg.loss.name}_loss".lower(): loss}, i2t_acc, t2i_acc

    def forward(self, batch, embeddings=False):
        if embeddings == "image":
            return self.forward_image_feature(batch["image"])
        if embeddings == "text":
            return self.forward_text_feature(batch["input_ids"], batch["attention_mask"])
        image, ids, mask = batch["image"], batch["input_ids"], batch["attention_mask"]
        # optional, beyond the reference's batch keys: the captions' token counts as HOST numbers (what the tokenizer returned before the
        # host->device copy).  With them the text tower sizes its packed rows without reading anything back from the GPU.
        lengths = batch.get("caption_lengths") if isinstance(batch, dict) else None
        discard_prefetched(logger.warning)           # gathers of an earlier step that never reached the loss
        self.two_streams_used = bool(image.is_cuda and _two_streams_ok())      # (read by callers that launch per-tower work on the tower's stream)
        if self.two_streams_used:
            # The two towers are independent until the loss: the text tower runs on a second HIP stream so that its kernels
            # fill the CUs the image tower's kernels leave idle (partial last rounds of the 256-CU tile grids, memory-bound
            # LayerNorm / attention phases).  autograd replays each tower's backward on the stream its forward used.
            main = torch.cuda.current_stream()
            side = _side_stream(image.device)
            side.wait_stream(main)
            # (which tower is enqueued first makes no measurable difference: 126.2 vs 126.4 ms/step)
            img = self._image_embeddings(image)
            self._prefetch(img, embeddings)          # the image embeddings travel while the text tower is still computing
            with torch.cuda.stream(side), packed_text(lengths):
                txt = self.forward_text_project(self.forward_text_feature(ids, mask), mask)
                self._prefetch(txt, embeddings)
            main.wait_stream(side)
            txt.record_stream(main)
            # The caption tensors were allocated under the main stream but are read by side-stream kernels in the forward AND, through
            # the saved tensors of the text tower, in its backward.  Without this mark the caching allocator hands their memory back to
            # the main stream the moment the last Python / autograd reference drops, while those kernels may still be queued (a batch
            # that goes out of scope after the step: wrong word-embedding and first-layer gradients, found by the full-size parity test).
            for t in (ids, mask):
                if t.is_cuda:
                    t.record_stream(side)
        else:
            img = self._image_embeddings(image)
            self._prefetch(img, embeddings)
            with packed_text(lengths):      # only the masked pooling reads the text tower's output here: padded token rows are not computed
                txt = self.forward_text_project(self.forward_text_feature(ids, mask), mask)
        if embeddings == "all":
            return [img, txt]
        # MixUpNCE alone reads the mixing weight of the batch (simseg_amd.mixup.Mixup.apply's `lam` for the mixed modality); under any
        # other loss such a key is ignored
        loss_kwargs = {}
        if self.cfg.loss.name == "MixUpNCE":
            loss_kwargs = {k: batch[k] for k in ("image_alpha", "text_alpha") if k in batch}
        return self.forward_loss(img, txt, ignore_mask=None, **loss_kwargs)


_SIDE = {}


def _two_streams_ok():
    """SIMSEG_AMD_TWO_STREAMS: 0 = never, 1 = always; default = unless gradients flow through torch DDP (its bucket hooks
    synchronise the all-reduce with ONE stream - the one that produced the last gradient of a bucket - which is not a
    guarantee this repo can test on a single-GPU box when gradients come from two streams)."""
    env = os.environ.get("SIMSEG_AMD_TWO_STREAMS")
    if env is not None:
        return env != "0"
    multi = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
    return not (multi and torch.is_grad_enabled())


def _side_stream(device):
    st = _SIDE.get(device)
    if st is None:
        st = _SIDE[device] = torch.cuda.Stream(device=device)
        # text-tower gradients are produced on the side stream and accumulated on the parameters' stream: intended
        # (autograd inserts the synchronisation), so its advisory warning is switched off
        f = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
        if f is not None:
            f(False)
    return st


class ImageEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.model_tag = cfg.model.image_encoder.tag
        self.pretrained = cfg.model.image_encoder.pretrained
        self.trainable = cfg.model.image_encoder.trainable
        kwargs = {}
        if "vit" in self.model_tag:
            kwargs["img_size"] = cfg.transforms.input_size      # clip.py:193-194
        else:
            kwargs["global_pool"] = ""
        self.model = BACKBONE.get(cfg.model.image_encoder.name)(cfg, **kwargs)
        for p in self.model.parameters():
            p.requires_grad = self.trainable

    def forward(self, x):
        return self.model(x)


class TextEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.model_tag = cfg.model.text_encoder.tag
        self.pretrained = cfg.model.text_encoder.pretrained
        self.trainable = cfg.model.text_encoder.trainable
        self.model = BACKBONE.get(cfg.model.text_encoder.name)(cfg)
        for p in self.model.parameters():
            p.requires_grad = self.trainable

    def forward(self, input_ids, attention_mask):
        return self.model(input_ids=input_ids, attention_mask=attention_mask).last_hidden_state


@PIPELINE.register_obj
def clip(cfg):
    return CLIPModel(cfg, ENV.rank)
