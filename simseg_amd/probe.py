"""The linear-probe task on the HIP path (the reference's simseg/tasks/linear_prob + simseg/models/pipelines/linear_prob.py):

  ProbeHeadFn          classifier + nn.CrossEntropyLoss + accuracy(topk=(1, 5)) as ONE autograd node
  SoftProbeHeadFn      the same head against the two-label soft target of a Mixup / CutMix batch (simseg_amd.mixup), same backward
  SoftCEFn             the soft-target rows alone as one node (LabelSmoothingCrossEntropy / SoftTargetCrossEntropy of the LOSS registry)
  LinearProbeTrainer   one training iteration / an evaluation pass / checkpoints, with the reference's semantics
                       (LinearProbRunner + ClipOptimizerHook + LinearEvalHook), as simseg_amd.trainer.Trainer is for the clip task

The head's logits and gradients are fp32 (fp32 GEMMs on the fp32 master weights, fp32 loss rows and logit gradient), so this task uses no
loss scaling: there is no GradScaler anywhere on its path, whatever 16-bit type the frozen encoder computes in."""
import time

import torch

from . import ops
from .towers import _GradAwareFn, _saving
from .trainer import lr_multiplier, param_groups

F32 = torch.float32


class ProbeHeadFn(_GradAwareFn):
    """(x [B, D], weight [C, D], bias [C], labels int64 [B]) -> (loss, out3, logits).

    forward:  logits = x . weight^T + bias   (ops.gemm, bias epilogue, fp32 from the fp32 masters)
              out3 = {mean cross-entropy, top-1 count, top-5 count}, dlogits = (softmax - onehot) / B   (ops.ce_rows, one pass)
              loss = out3[0]
    backward: dW = dlogits^T . x  (the same GEMM on transposed copies), db = column sums of dlogits (ops.colsum_accum; a class count that
              is no multiple of 8 takes the transposed copy times a row of ones through the GEMM),
              dx = dlogits . W only if x asks for it (a trainable encoder); all times the upstream gradient, read on the device.
    out3 and logits are not differentiable outputs (accuracy counts, and the prediction the evaluation hook gathers)."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels):
        x32 = x.detach().to(F32).contiguous()
        w = weight.detach().contiguous()
        logits = ops.gemm(x32, w, bias=bias.detach().contiguous(), out_dtype=F32)
        need = _saving(ctx)                     # (False under torch.no_grad(): an evaluation pass writes no gradient)
        out3, _, _, dlogits = ops.ce_rows(logits, labels.contiguous(), write_grad=need)
        if need:
            ctx.save_for_backward(x32, w, dlogits)
        ctx.x_dtype = x.dtype
        ctx.mark_non_differentiable(out3, logits)
        return out3[0].clone(), out3, logits

    @staticmethod
    def backward(ctx, gloss, _g3, _glogits):
        x32, w, dlogits = ctx.saved_tensors
        dl = ops.scale_by_scalar(dlogits, gloss.to(F32).reshape(1).contiguous())       # (the upstream gradient stays on the device)
        dx = dw = db = None
        dlt = ops.transpose_f32(dl) if ctx.needs_input_grad[1] or (ctx.needs_input_grad[2] and dl.shape[1] % 8) else None
        if ctx.needs_input_grad[1]:
            dw = ops.gemm(dlt, ops.transpose_f32(x32), out_dtype=F32)                             # [C, B] . [D, B]^T
        if ctx.needs_input_grad[2]:
            if dl.shape[1] % 8 == 0:
                db = ops.colsum_accum(dl, torch.zeros(dl.shape[1], device=dl.device, dtype=F32))
            else:       # simseg_colsum_accum takes widths that are multiples of 8: the row sums of the transposed copy, as a GEMM with ones
                db = ops.gemm(dlt, torch.ones(1, dl.shape[0], device=dl.device, dtype=F32), out_dtype=F32).reshape(-1)
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(dl, ops.transpose_f32(w), out_dtype=F32).to(ctx.x_dtype)                 # [B, C] . [D, C]^T
        return dx, dw, db, None


class SoftProbeHeadFn(ProbeHeadFn):
    """(x [B, D], weight [C, D], bias [C], labels_a int64 [B], labels_b int64 [B], lam fp32 [B], smoothing) -> (loss, out3, logits).

    ProbeHeadFn against the two-label soft target of a Mixup / CutMix batch, t = lam * s(a) + (1 - lam) * s(b) with s(y) = (1 - smoothing)
    * onehot(y) + smoothing / C (ops.soft_ce_rows: the same single pass, no dense target): loss = mean of -sum_c t_c log softmax_c,
    dlogits = (softmax - t) / B, and out3's counts are top-1 / top-5 hits against labels_a, the samples' own labels.  The backward is
    ProbeHeadFn's: it only needs dlogits."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels_a, labels_b, lam, smoothing):
        x32 = x.detach().to(F32).contiguous()
        w = weight.detach().contiguous()
        logits = ops.gemm(x32, w, bias=bias.detach().contiguous(), out_dtype=F32)
        need = _saving(ctx)
        out3, _, _, dlogits = ops.soft_ce_rows(logits, labels_a.contiguous(), labels_b.contiguous(), lam.detach().to(F32).contiguous(),
                                               smoothing=float(smoothing), write_grad=need)
        if need:
            ctx.save_for_backward(x32, w, dlogits)
        ctx.x_dtype = x.dtype
        ctx.mark_non_differentiable(out3, logits)
        return out3[0].clone(), out3, logits

    @staticmethod
    def backward(ctx, gloss, _g3, _glogits):
        return ProbeHeadFn.backward(ctx, gloss, _g3, _glogits) + (None, None, None)


class SoftCEFn(_GradAwareFn):
    """(logits [B, C] fp32 / bf16 / fp16, labels_a, labels_b int64 [B], lam fp32 [B], smoothing, mean) -> the mean of the two-label
    soft-target cross-entropy rows (mean=True) or the rows themselves, as ONE autograd node over ops.soft_ce_rows: the forward pass already
    wrote (softmax - t) / B, the backward scales it by the upstream gradient on the device (per row, times B, for the rows)."""

    @staticmethod
    def forward(ctx, logits, labels_a, labels_b, lam, smoothing, mean):
        need = _saving(ctx)
        out3, rows, _, dlogits = ops.soft_ce_rows(logits.detach().contiguous(), labels_a.contiguous(), labels_b.contiguous(),
                                                  lam.detach().to(F32).contiguous(), smoothing=float(smoothing), write_grad=need)
        if need:
            ctx.save_for_backward(dlogits)
        ctx.mean, ctx.dtype = bool(mean), logits.dtype
        return out3[0].clone() if mean else rows

    @staticmethod
    def backward(ctx, g):
        dlogits, = ctx.saved_tensors
        if ctx.mean:
            dl = ops.scale_by_scalar(dlogits, g.to(F32).reshape(1).contiguous())
        else:
            dl = ops.scale_rows(dlogits, g.to(F32).contiguous(), alpha=float(dlogits.shape[0]))
        return dl.to(ctx.dtype), None, None, None, None, None


def optimizer_class(name):
    """cfg.optim.name -> class: `LARS` (the reference's simseg.core.optimizer.LARS) is this package's; dotted or bare torch names as the
    reference's OptimizerHook.build_optimizer resolves them (core/hooks/optimizer.py:103-115)."""
    import importlib
    if name.rpartition(".")[2] == "LARS":
        from simseg.core.optimizer import LARS
        return LARS
    mod, _, cls = name.rpartition(".")
    return getattr(importlib.import_module(mod or "torch.optim"), cls)


class LinearProbeTrainer:
    def __init__(self, model, cfg, steps_per_epoch):
        """model: a LinearProbModel on the device.  The optimizer is built as the reference's hook builds it: one param group per trainable
        parameter (trainer.param_groups), cfg.optim.param with lr = cfg.optim.lr.init; the lr schedule is a stateless function of the
        global step (trainer.lr_multiplier over cfg.optim.lr.*)."""
        self.model, self.cfg = model, cfg
        p = dict(cfg.optim.param)
        p["lr"] = cfg.optim.lr.init
        self.optimizer = optimizer_class(cfg.optim.name)(param_groups(model, cfg), **p)
        self.base_lrs = [g["lr"] for g in self.optimizer.param_groups]
        total = steps_per_epoch * cfg.epoch
        warm = 0
        if cfg.optim.lr.warmup_proportion is not None:
            warm = int(total * cfg.optim.lr.warmup_proportion)
        if cfg.optim.lr.warmup_epoch is not None:
            warm = int(steps_per_epoch * cfg.optim.lr.warmup_epoch)
        self.sched = dict(name=cfg.optim.lr.name, num_warmup_steps=warm, num_training_steps=total, **dict(cfg.optim.lr.param))
        self.step, self.epoch, self.inner_step = 0, 0, 0

    def set_lrs(self, step):
        m = lr_multiplier(step=step, **self.sched)
        lrs = [b * m for b in self.base_lrs]
        for g, lr in zip(self.optimizer.param_groups, lrs):
            g["lr"] = lr
        return lrs

    def train_step(self, batch):
        """-> {loss, acc1, acc5 (device tensors, no host read), lr}."""
        lrs = self.set_lrs(self.step)
        self.optimizer.zero_grad(set_to_none=True)
        loss_dict, acc1, acc5 = self.model(batch)
        loss = sum(loss_dict.values())
        loss.backward()
        self.optimizer.step()
        self.step += 1
        self.inner_step += 1
        return {"loss": loss.detach(), "acc1": acc1, "acc5": acc5, "lr": lrs[0]}

    @torch.no_grad()
    def evaluate(self, batches):
        """Top-1 / top-5 accuracy (percent) and the mean loss over an iterable of batches.  The counts and the summed loss accumulate on the
        device across batches; they are read back once, at the end."""
        was_training = self.model.training
        self.model.eval()
        acc = None
        n = 0
        for batch in batches:
            tot = self.model.eval_counts(batch)              # fp64 [3] on the device: {sum of the loss rows, top-1 hits, top-5 hits}
            acc = tot if acc is None else acc + tot
            n += int(batch["label"].shape[0])
        self.model.train(was_training)
        if acc is None:
            return {"loss": float("nan"), "acc1": float("nan"), "acc5": float("nan"), "count": 0}
        s, h1, h5 = acc.tolist()                             # the one host read
        return {"loss": s / n, "acc1": 100.0 * h1 / n, "acc5": 100.0 * h5 / n, "count": n}

    # ---- checkpoints in the reference's layout (core/hooks/checkpoint.py:14-45) --------------------------------------------------
    def checkpoint(self, end_of_epoch=False):
        meta = dict(time=time.asctime(), simseg_version="0.1.0+mi355x", torch_version=torch.__version__,
                    epoch=self.epoch + 1 if end_of_epoch else self.epoch, step=self.step, inner_step=0 if end_of_epoch else self.inner_step)
        return dict(state_dict=self.model.state_dict(), optimizer=self.optimizer.state_dict(), meta=meta)

    def load_checkpoint(self, state, load_optimizer=True):
        sd = state.get("state_dict") or state.get("model_state_dict") or state.get("model")
        sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
        if self.cfg.ckpt.only_load_image_encoder:             # a SimSeg (clip task) checkpoint: its image tower only
            sd = {k: v for k, v in sd.items() if k.startswith("image_encoder.")}
            load_optimizer = False
        missing, unexpected = self.model.load_state_dict(sd, strict=False)
        if load_optimizer and "optimizer" in state:
            self.optimizer.load_state_dict(state["optimizer"])
        if not self.cfg.ckpt.only_load_image_encoder:
            meta = state.get("meta", {})
            self.step, self.epoch, self.inner_step = meta.get("step", 0), meta.get("epoch", 0), meta.get("inner_step", 0)
        return missing, unexpected
