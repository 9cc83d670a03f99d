"""InfoNCE of the SimSeg contrastive objective (mirror of simseg/models/criteria/losses/mml_loss.py:12-103) on the
fused HIP loss path: fp32 MFMA similarity block -> in-place cross-entropy rows -> gradient GEMMs, with the embedding
exchange as an RCCL all-gather forward / reduce-scatter backward.  MixUpNCE (:105-197) and Triplet (:256-347) score the same
similarity block with their own row kernels, and so do two losses the reference does not have: SigLip, the pairwise sigmoid loss of SigLIP, and NTXent, SimCLR's
image-to-image loss over two views (the self-supervised half of SLIP)."""
import torch
import torch.distributed as dist
import torch.nn as nn

from simseg.utils import ENV, GatherLayer, logger
from simseg.utils.dist import generate_local_groups
from simseg_amd.heads import ClipLossFn, MixNCEFn, NCEFn, NTXentFn, SigLipFn, TripletFn, TripletLocalFn, all_gather_rows

from .builder import LOSS

__all__ = ["NCE", "MixUpNCE", "Triplet", "SigLip", "NTXent", "LabelSmoothingCrossEntropy", "SoftTargetCrossEntropy"]


class _GlobalLoss(nn.Module):
    """What the global_reduce losses share: the loss group, the temperature, and the exchange of the other side's embeddings."""

    group, rank, gather_backward = None, 0, False

    def _loss_group(self, cfg, who):
        """self.group, self.rank: generate_local_groups(loss.group_size) under a process group, (None, 0) without one."""
        if dist.is_available() and dist.is_initialized():
            group_size = cfg.loss.group_size if cfg.loss.group_size >= 0 else ENV.size
            self.group, self.rank = generate_local_groups(group_size)
            logger.info(f"{who} Loss Group size, Group Rank, Env Rank:", group_size, self.rank, ENV.rank, root_only=False)
        else:   # single process: the gather is the identity (the reference insists on a process group)
            self.group, self.rank = None, 0
            logger.info(f"{who}: no process group, global_reduce degenerates to the local batch")

    def _init_temperature(self, cfg, value=None, learnable=None):
        """self.temperature = loss.temperature.value (or `value`): an nn.Parameter under loss.temperature.name=parameter, a non-persistent
        buffer under `constant`; `learnable` (True / False) overrides the name's choice."""
        name = cfg.loss.temperature.name
        if name not in ("parameter", "constant"):
            raise NotImplementedError(name)
        t = torch.ones([]) * float(cfg.loss.temperature.value if value is None else value)
        if name == "parameter" if learnable is None else learnable:
            self.temperature = nn.Parameter(t)
        else:
            self.register_buffer("temperature", t, persistent=False)

    def _gather(self, t):
        if self.group is None:
            return t
        if self.gather_backward and t.requires_grad:
            return GatherLayer.apply(t, self.group, self.rank)
        return all_gather_rows(t, self.group)

    def _gather_global(self, feat1, feat2, what="batch size"):
        """feat2's rows of every rank of the group: a whole number of blocks of feat1's size."""
        feat2_global = self._gather(feat2)
        if feat2_global.shape[0] % feat1.shape[0] != 0:
            raise AssertionError(f"global size: {feat2_global.shape[0]}, {what}: {feat1.shape[0]}")
        return feat2_global

    def _gather_ignore(self, ignore_mask):
        return None if ignore_mask is None else all_gather_rows(ignore_mask.float(), self.group) if self.group else ignore_mask.float()


@LOSS.register_obj
class NCE(_GlobalLoss):
    def __init__(self, cfg, rank):
        super().__init__()
        self.cfg = cfg
        self.global_reduce = cfg.loss.global_reduce
        if self.global_reduce:
            self.gather_backward = cfg.loss.nce_loss.gather_backward
            self._loss_group(cfg, "NCE")
        self._init_temperature(cfg)
        self.smoothing = float(cfg.loss.smoothing)

    def both(self, image_embeddings, text_embeddings):
        """0.5 * (self(image, text)[0] + self(text, image)[0]) and the two top-1 accuracies - what CLIPModel.forward_loss computes with
        two calls of this module (pipelines/clip.py:129-140) - as ONE autograd node with the embedding exchange inside
        (simseg_amd.heads.ClipLossFn: same kernels, a third of the launches).  global_reduce losses without an ignore mask only."""
        if not self.global_reduce:
            raise NotImplementedError("NCE.both: the fused head is the global_reduce form")
        return ClipLossFn.apply(image_embeddings, text_embeddings, self.temperature, self.group, self.rank, self.smoothing, self.gather_backward)

    def forward(self, feat1, feat2, label=None, ignore_mask=None):
        if self.global_reduce:
            feat2_global = self._gather_global(feat1, feat2)
            return NCEFn.apply(feat1, feat2_global, self.temperature, ignore_mask, self._gather_ignore(ignore_mask), self.rank, self.smoothing)
        if ignore_mask is not None:
            raise NotImplementedError("ignore_mask with loss.global_reduce=False is outside the accelerated path")
        # local branch (:79-86): symmetric loss over the local batch, three return values
        l1, a1 = NCEFn.apply(feat1, feat2, self.temperature, None, None, 0, self.smoothing)
        l2, a2 = NCEFn.apply(feat2, feat1, self.temperature, None, None, 0, self.smoothing)
        return 0.5 * (l1 + l2), a1, a2


@LOSS.register_obj
class MixUpNCE(_GlobalLoss):
    """InfoNCE against mixed targets (mml_loss.py:105-197 of the reference): one modality of the batch was mixed with its flipped self
    (x_i <- alpha_i x_i + (1 - alpha_i) x_{B-1-i}), and row i is scored against its own column with weight alpha_i and against column
    B - 1 - i (`targets.flip(0)`) with 1 - alpha_i, on the fused row path (simseg_amd.heads.MixNCEFn).  Constructed like NCE;
    loss.global_reduce=False raises NotImplementedError, as in the reference.

    forward(feat1, feat2, ignore_mask=None, image_alpha=... | text_alpha=...) needs exactly ONE of the two keywords: a float, a 0-dim
    tensor or an [N1] tensor.  simseg_amd.mixup.Mixup.apply on the image batch yields exactly this weight as `lam`, and its partner order
    B - 1 - i is this loss's flip.  The reference's formula applies the SAME alpha_i and flipped target in both directions (image -> text
    and text -> image), whichever modality was mixed; so does this class.  Returns (loss, top-1 acc against the row's own column); there
    is no `both` method."""

    def __init__(self, cfg, rank):
        super().__init__()
        self.cfg = cfg
        self.global_reduce = cfg.loss.global_reduce
        if not self.global_reduce:
            raise NotImplementedError("MixUpNCE: loss.global_reduce=False")
        self.gather_backward = cfg.loss.nce_loss.gather_backward
        self._loss_group(cfg, "MixUpNCE")
        self._init_temperature(cfg)
        self.smoothing = float(cfg.loss.smoothing)

    def forward(self, feat1, feat2, label=None, ignore_mask=None, **kwargs):
        if ("image_alpha" in kwargs) == ("text_alpha" in kwargs):
            raise NotImplementedError("MixUpNCE loss only supports mixing up one modal, please consider M3ixupNCE")
        alpha = kwargs["image_alpha"] if "image_alpha" in kwargs else kwargs["text_alpha"]
        N1 = feat1.shape[0]
        alpha = torch.as_tensor(alpha, dtype=torch.float32).to(feat1.device).detach().reshape(-1).contiguous()
        if alpha.numel() not in (1, N1):
            raise ValueError(f"MixUpNCE: alpha holds {alpha.numel()} values for a batch of {N1}")
        feat2_global = self._gather_global(feat1, feat2)
        return MixNCEFn.apply(feat1, feat2_global, self.temperature, alpha, ignore_mask, self._gather_ignore(ignore_mask), self.rank, self.smoothing)


@LOSS.register_obj
class Triplet(_GlobalLoss):
    """The max-violation hinge of VSE++ (mml_loss.py:256-347 of the reference) on the fused row path: cost_ij = max(margin + s_ij - s_ii, 0)
    over the negatives of row i, reduced per row by loss.triplet_loss.reduce_mode = "max" (the hardest negative) or "mean"
    (sum / (N1 - 1)), and SUMMED over rows.  Gradient passes the clamp where margin + s_ij - s_ii > 0 (include/simseg_hip.h).

    loss.global_reduce=True: feat1 against the gathered feat2; returns (loss, acc).  The reference masks the WHOLE own-rank block of
    columns, not only the diagonal, and so does this class: with ONE rank every column is masked, and the loss and all gradients are
    exactly 0.  loss.global_reduce=False: the symmetric local form over one matrix (rows: 1 -> 2, columns: 2 -> 1), only the diagonal
    masked; returns (loss, i2t acc, t2i acc).

    Gathering follows _GlobalLoss._gather without gather_backward: with no process group the local tensor is used and gradient flows through
    both roles; with a group the gather is detached, as the reference's all_gather / all_gather_group are.  The diagonal block is taken at
    the GROUP rank: the reference overwrites it with the global rank (mml_loss.py:272), which is only correct where the two coincide.
    ignore_mask is accepted and not applied, as in the reference.  There is no `both` method."""

    def __init__(self, cfg, rank):
        super().__init__()
        self.cfg = cfg
        self.margin = float(cfg.loss.triplet_loss.margin)
        self.reduce = cfg.loss.triplet_loss.reduce_mode
        if self.reduce not in ("mean", "max"):
            raise NotImplementedError("Reduce method {} is not implemented yet".format(self.reduce))
        self.global_reduce = cfg.loss.global_reduce
        if self.global_reduce:
            self._loss_group(cfg, "Triplet")

    def forward(self, feat1, feat2, label=None, ignore_mask=None):
        reduce = 0 if self.reduce == "mean" else 1
        if not self.global_reduce:
            return TripletLocalFn.apply(feat1, feat2, self.margin, reduce)
        return TripletFn.apply(feat1, self._gather_global(feat1, feat2), self.rank, self.margin, reduce)       # (no gather_backward: detached)


@LOSS.register_obj
class SigLip(_GlobalLoss):
    """The pairwise sigmoid loss of SigLIP (Zhai et al., "Sigmoid Loss for Language Image Pre-Training", ICCV'23; open_clip's SigLipLoss)
    on the fused row path (simseg_amd.heads.SigLipFn; formulas in include/simseg_hip.h, simseg_siglip_rows): every (row, column) pair of
    the [N1, N2] similarity block is a binary problem, loss = (1 / N1) sum_ij -log sigmoid(y_ij (s_ij / T + b)) with y = +1 on the row's
    own column and -1 elsewhere.  No row-wise softmax, and a learnable bias b beside the temperature.  Not in the reference: selected by
    loss.name=SigLip and driven by keys that exist - loss.temperature.{name, value}, loss.global_reduce, loss.nce_loss.gather_backward,
    loss.group_size, loss.smoothing (which must be 0).

    T is the quantity the other losses here call the temperature, clamped to [1e-3, 0.5] like NCE's - the logit scale is t = 1 / T, and
    what is learned is T itself, not log t as in the paper.  The bias has no config key: INIT_BIAS = -10.0, or the constructor's
    init_bias.  With loss.temperature.value=0.1 that is the paper's initialisation, t = 10 and b = -10.  Under
    loss.temperature.name=parameter both temperature and bias are nn.Parameters (trained, and in the state dict); under `constant` the
    temperature is a non-persistent buffer as in NCE and the bias a PERSISTENT one: it is not derivable from the config, so a checkpoint
    carries it.  As parameters both fall under the optimizer's base weight_decay like any other (trainer.param_groups): decay pulls the
    bias from -10 towards 0 and shrinks T.  open_clip exempts its logit scale and bias; to do the same add an optim.param_group_rules
    entry such as {regex: "^loss\\.(bias|temperature)$", param: {weight_decay: 0.0}}.

    The group and the exchange are _GlobalLoss's (_loss_group, _gather).  With a process group and gather_backward=False the gathered
    embeddings are detached: each rank's loss then differentiates only through its own rows' role as feat1, and the gradient a rank's
    embeddings receive as OTHER ranks' negatives - for this loss every off-diagonal pair is a term of its own, so that is most of the
    negatives' signal - is dropped; gather_backward=True (or no process group) keeps it.  The loss is normalised by the local batch N1
    on every rank, as in the paper.

    forward(feat1, feat2, label=None, ignore_mask=None) -> (loss, top-1 acc).  There is no `both` method: CLIPModel.forward_loss calls
    the module once per direction and returns {"siglip_loss": 0.5 * (i2t + t2i)}.  loss.global_reduce=False, a non-zero loss.smoothing and
    an ignore mask are refused."""

    INIT_BIAS = -10.0

    def __init__(self, cfg, rank, init_bias=None):
        super().__init__()
        self.cfg = cfg
        self.global_reduce = cfg.loss.global_reduce
        if not self.global_reduce:
            raise NotImplementedError("SigLip: loss.global_reduce=False (the local form) is not built; the loss scores feat1 against the gathered feat2")
        if float(cfg.loss.smoothing) != 0.0:
            raise ValueError(f"SigLip: loss.smoothing={cfg.loss.smoothing} - the pairwise sigmoid loss has no label smoothing, set it to 0")
        self.gather_backward = cfg.loss.nce_loss.gather_backward
        self._loss_group(cfg, "SigLip")
        self._init_temperature(cfg)
        b = torch.ones([]) * float(self.INIT_BIAS if init_bias is None else init_bias)
        if isinstance(self.temperature, nn.Parameter):
            self.bias = nn.Parameter(b)
        else:
            self.register_buffer("bias", b, persistent=True)

    def forward(self, feat1, feat2, label=None, ignore_mask=None):
        if ignore_mask is not None:
            raise NotImplementedError("SigLip: an ignore_mask is not supported (every pair is a term of the loss; no row weights are built)")
        return SigLipFn.apply(feat1, self._gather_global(feat1, feat2), self.temperature, self.bias, self.rank)


@LOSS.register_obj
class NTXent(_GlobalLoss):
    """NT-Xent, the loss of SimCLR (Chen et al., ICML'20), in the global form of SLIP's SIMCLRLoss (Mu et al., ECCV'22) on the fused row
    path (simseg_amd.heads.NTXentFn; formulas in include/simseg_hip.h, simseg_ntxent_rows): the two views' embeddings are stacked to
    [2B, P], the stacked tensor is gathered ONCE (rank-major: this rank's rows are block `rank` of the gathered matrix, and every other
    rank's a and b rows are negatives), and each of the 2B rows is a cross-entropy over all gathered rows but itself, its positive the
    other view of the same image.  Not in the reference: an image-to-image loss, the consumer of simseg.transforms.build_train_views.

    The temperature is read from loss.temperature.{name, value} - clamped to [1e-3, 0.5] like NCE's - unless the constructor's
    `temperature` (a value) and `learnable` (True: an nn.Parameter, False: a non-persistent buffer) override it; the group and the
    exchange are _GlobalLoss's (_loss_group, _gather, loss.nce_loss.gather_backward, loss.group_size).

    forward(view_a, view_b, label=None, ignore_mask=None) -> (loss, top-1 acc of view_a's rows): the (loss, acc) shape of the other
    global_reduce losses; forward(view_b, view_a) gives the same loss and view_b's accuracy.  loss.global_reduce=False, a non-zero
    loss.smoothing and an ignore mask are refused.  It is not a CLIPModel main loss (image and text embeddings are not two views):
    CLIPModel.enable_ssl builds one for the image self-supervision branch."""

    def __init__(self, cfg, rank, temperature=None, learnable=None):
        super().__init__()
        self.cfg = cfg
        self.global_reduce = cfg.loss.global_reduce
        if not self.global_reduce:
            raise NotImplementedError("NTXent: loss.global_reduce=False (a local form) is not built; the stacked views are scored against their gathered selves")
        if float(cfg.loss.smoothing) != 0.0:
            raise ValueError(f"NTXent: loss.smoothing={cfg.loss.smoothing} - the row kernel has no label smoothing, set it to 0")
        self.gather_backward = cfg.loss.nce_loss.gather_backward
        self._loss_group(cfg, "NTXent")
        self._init_temperature(cfg, temperature, learnable)

    def forward(self, view_a, view_b, label=None, ignore_mask=None):
        if ignore_mask is not None:
            raise NotImplementedError("NTXent: an ignore_mask is not supported (the row kernel builds no row weights)")
        if view_a.shape != view_b.shape:
            raise ValueError(f"NTXent: the two views differ in shape, {tuple(view_a.shape)} against {tuple(view_b.shape)}")
        z = torch.cat([view_a, view_b])
        loss, acc_a, _ = NTXentFn.apply(z, self._gather_global(z, z, "stacked batch size"), self.temperature, self.rank)
        return loss, acc_a


def _reduce(rows, reduction):
    if reduction == "mean":
        return rows.mean()
    return rows


@LOSS.register_obj
class LabelSmoothingCrossEntropy(nn.Module):
    """NLL loss with label smoothing (mml_loss.py:350-376 of the reference): confidence * nll + smoothing * mean_c(-log softmax_c), which
    is the cross-entropy against (1 - smoothing) * onehot(target) + smoothing / C - the two-label kernel with a = b = target and lam = 1
    (simseg_amd.probe.SoftCEFn over ops.soft_ce_rows), one autograd node, no log-softmax tensor.  reduction="mean" returns the mean,
    anything else the rows, as the reference does."""

    def __init__(self, cfg, rank, smoothing=0.1, reduction="mean", **kwargs):
        super().__init__()
        if not smoothing < 1.0:
            raise AssertionError("smoothing must be below 1")
        self.smoothing, self.confidence, self.reduction = smoothing, 1.0 - smoothing, reduction

    def forward(self, x, target):
        from simseg_amd.probe import SoftCEFn
        lam = torch.ones(target.shape[0], device=x.device, dtype=torch.float32)
        return SoftCEFn.apply(x, target, target, lam, self.smoothing, self.reduction == "mean")


@LOSS.register_obj
class SoftTargetCrossEntropy(nn.Module):
    """Cross-entropy against soft targets (mml_loss.py:379-391 of the reference).

    forward(x, target) with a dense [B, C] target is the reference's three lines in torch ops - the UNFUSED form: it materialises the
    log-softmax and the product beside the target, and also runs on the CPU.  A Mixup / CutMix target never has more than two
    non-uniform entries per row, so forward(x, {"label", "label_b", "lam", "smoothing"}) - the dict simseg_amd.mixup.Mixup.apply returns
    - takes the fused kernel instead (one autograd node, no dense tensor beside the logits)."""

    def __init__(self, cfg, rank, reduction="mean", **kwargs):
        super().__init__()
        self.reduction = reduction

    def forward(self, x, target):
        if isinstance(target, dict):
            from simseg_amd.probe import SoftCEFn
            return SoftCEFn.apply(x, target["label"], target["label_b"], target["lam"], float(target.get("smoothing", 0.0)),
                                  self.reduction == "mean")
        loss = torch.sum(-target * torch.log_softmax(x, dim=-1), dim=-1)
        return _reduce(loss, self.reduction)
