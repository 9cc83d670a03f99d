"""The table-driven optimizers: AdamW (torch.optim.AdamW's update rule and hyper-parameters, configs/clip/simseg.vit-b.yaml:31-36; fp32
state m, v) and LARS, each ONE update launch for every parameter tensor of every param group (the reference's ClipOptimizerHook builds
one group per parameter, tasks/clip/hooks/optimizer.py:18-36, so "one launch per group" would be ~400 launches).

Both stand on one TensorTable (device contract: csrc/tensor_table.h): six 8-byte words per tensor - the fp32 master, its gradient, then
the optimizer's own (state pointers, the 16-bit copy, the (lr, weight_decay) pair, flags) - plus the sizes and the list of CHUNK-element
chunks, one block each.  The rows are completed in pinned host memory each step (gradient tensors are re-allocated by autograd, learning
rates follow the schedule) and uploaded without a host-device synchronisation; the pinned buffers form a ring, each guarded by an event
recorded after its upload, so the host never rewrites a buffer whose asynchronous copy has not executed yet.  The optimizers keep their
bucketing key, their row layout, their flat state buffers and their launches.  p16 is the 16-bit compute copy of the parameter, written
by the update kernel and handed to the towers (towers.weights_rewritten), so a training step launches no weight-cast kernels.

AdamW checkpoints use torch.optim.AdamW's state layout ({step, exp_avg, exp_avg_sq} per parameter), so the reference's optimizer
checkpoints (core/hooks/checkpoint.py:14-45) load here and ours load there; the bias-correction step counter travels with them."""
import contextlib
import math

import numpy as np
import torch
from torch.amp.grad_scaler import OptState
from torch.optim.optimizer import required

from .lib import call, note_half, ptr, stream
from .towers import weights_rewritten

CHUNK = 1 << 16
RING = 4


def chunk_lists(sizes, chunk):
    """-> (tid int32, coff int64, first int32 [len(sizes) + 1]): chunk c covers [coff[c], coff[c] + chunk) of tensor tid[c]; tensor t owns
    the chunks first[t] .. first[t + 1] - 1 (none when it has no elements)."""
    tid, coff, first = [], [], [0]
    for t, n in enumerate(sizes):
        for c in range(0, n, chunk):
            tid.append(t); coff.append(c)
        first.append(len(tid))
    return np.array(tid, dtype=np.int32), np.array(coff, dtype=np.int64), np.array(first, dtype=np.int32)


def pack_lr_wd(lr, wd):
    """Per-tensor learning rates and weight decays -> the int64 table words that hold them as two float32 (lr in the low half)."""
    hyper = np.empty((len(lr), 2), dtype=np.float32)
    hyper[:, 0], hyper[:, 1] = lr, wd
    return hyper.view(np.int64)[:, 0]


class TensorTable:
    """One bucket's launch plan: what does not change from step to step, and the ring through which each step's rows reach the device.
    static: int64 [n, 6], the masters' addresses in column 0 and whatever else is fixed; the optimizers add their buffers as attributes."""

    def __init__(self, params, static, chunk=CHUNK):
        dev = params[0].device
        self.params, self.ids, self.static = params, tuple(id(p) for p in params), static
        self.sizes_host = np.array([p.numel() for p in params], dtype=np.int64)
        self.tid_host, self.coff_host, self.first_host = chunk_lists(self.sizes_host.tolist(), chunk)
        host = (self.sizes_host, self.tid_host, self.coff_host, self.first_host)
        self.sizes, self.tid, self.coff, self.first = (torch.from_numpy(a).to(dev) for a in host)
        self.n_tensors, self.n_chunks, self.chunk = len(params), len(self.tid_host), chunk
        self.ring = [torch.empty(len(params), 6, dtype=torch.int64).pin_memory() for _ in range(RING)]
        self.events, self.slot = [None] * RING, 0
        self.table = torch.empty(len(params), 6, dtype=torch.int64, device=dev)

    def __getitem__(self, name):
        """plan["n_chunks"]: a field by name, as when the plans were dicts."""
        return getattr(self, name)

    def matches(self, params):
        """The same parameter objects, and their storage where it was (.to() and a load with assign swap it)."""
        return self.ids == tuple(id(p) for p in params) and all(p.data_ptr() == a for p, a in zip(params, self.static[:, 0]))

    def upload(self, grads, columns, stream=None):
        """This step's rows = static + the gradients' addresses (column 1) + columns {index: values}, copied on `stream` (default: the
        current one) without a synchronisation.  grads are kept alive: the kernels read them asynchronously."""
        slot = self.slot
        self.slot = (slot + 1) % RING
        if self.events[slot] is not None:
            self.events[slot].synchronize()          # the upload that last used this pinned buffer has executed (RING steps ago)
        host = self.ring[slot].numpy()
        host[:] = self.static
        host[:, 1] = [g.data_ptr() for g in grads]
        for col, values in columns.items():
            host[:, col] = values
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            self.table.copy_(self.ring[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.events[slot] = ev
        self.keepalive = grads

    def launch_args(self, host=False):
        """The leading arguments of every entry point over the table (host=True: of those that check the host copies first)."""
        mid = (self.sizes_host.ctypes.data, self.tid_host.ctypes.data, self.coff_host.ctypes.data, self.n_tensors) if host else ()
        return (ptr(self.table), ptr(self.sizes), ptr(self.tid), ptr(self.coff)) + mid + (self.n_chunks, self.chunk)


def norm_type_code(norm_type):
    """norm_type of torch.nn.utils.clip_grad_norm_ -> the kernels' code: 2 (Euclidean) or 0 (infinity).  Checked on the host, before any
    device work."""
    nt = float(norm_type)
    if nt == 2.0:
        return 2
    if nt == math.inf:
        return 0
    raise NotImplementedError(f"norm_type {norm_type!r}: the fused gradient norm knows 2 and infinity (torch.nn.utils.clip_grad_norm_ has the others)")


def live_scale(scaler):
    """The loss scale of an enabled torch.amp.GradScaler as its float32 device tensor (what AdamW.clip_grad_norm_ takes as loss_scale);
    None for a disabled scaler, for None, and before the scaler's first scale() call (the gradients are then unscaled anyway)."""
    if scaler is None or not scaler.is_enabled():
        return None
    return scaler._scale


class AdamW(torch.optim.Optimizer):
    # torch.amp.GradScaler's contract for optimizers that handle the loss scale themselves (grad_scaler.py: `_step_supports_amp_scaling`):
    # scaler.step(optimizer) then sets optimizer.grad_scale / optimizer.found_inf (device tensors) and calls step() WITHOUT reading the
    # overflow flag on the host; the kernel unscales the gradients and skips the update on the device (simseg_adamw_multi_step_amp).
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=1e-3, half_dtype=torch.bfloat16):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if half_dtype not in (torch.bfloat16, torch.float16):
            raise TypeError("half_dtype: torch.bfloat16 (the default) or torch.float16 (the reference's AMP type, the benchmark headline since round 5)")
        self.half_dtype = half_dtype      # type of the 16-bit compute copies the kernel writes (what the towers' GEMMs read next step)
        self._step = 0                    # step() calls without a GradScaler (every one of them updates)
        self._step_dev = None             # AMP: float32 [2] on the device, the count of steps actually TAKEN (skipped ones do not count)
        self._amp_calls = 0               #      which slot is current
        self._plans = {}
        self._prepared = None
        self._streams = {}                # id(parameter) -> stream its update is launched on (set_param_streams); default: the current stream
        self._clip_coef = None            # armed by clip_grad_norm_: float32 [1] on the device, the coefficient the next step() multiplies in
        self._norm_partials = None        # float32 [sum of the buckets' n_chunks]: one partial per chunk of the gradient-norm pass
        self._norm_out = None             # float32 [2, 2]: {norm, coefficient} of clip_grad_norm_ (row 0) and of grad_norm (row 1)

    def set_param_streams(self, mapping):
        """mapping: {parameter: torch.cuda.Stream or None}.  The update of those parameters is launched on that stream instead of the current
        one - for a tower whose forward AND backward run on a stream of their own (the text tower of CLIPModel's two-stream schedule) it
        then starts when that tower's backward ends instead of waiting behind the other tower's: ~0.5 ms of a 512-pair step.  The caller owns
        the ordering: every later reader of these parameters (and of their 16-bit copies) must run on that stream or wait for it, and
        their gradients must be complete on it (single-process training; with a gradient exchange leave them on the current stream)."""
        for p_, st in mapping.items():
            if st is None:
                self._streams.pop(id(p_), None)
            else:
                self._streams[id(p_)] = st
        self._plans.clear()
        self._prepared = None

    # ---- launch plan: row = {p, g, m, v, p16, (lr, weight_decay)} ------------------------------------------------------------
    def _plan(self, key, params):
        plan = self._plans.get(key)
        if plan is not None and plan.matches(params):
            return plan
        dev = params[0].device
        total = sum(p.numel() for p in params)
        m = torch.zeros(total, device=dev, dtype=torch.float32)
        v = torch.zeros(total, device=dev, dtype=torch.float32)
        p16 = torch.empty(total, device=dev, dtype=self.half_dtype)
        o = 0
        for p in params:
            st = self.state[p]
            n = p.numel()
            if "m" in st:                     # keep moments across a re-plan / a loaded checkpoint
                m[o:o + n].copy_(st["m"].reshape(-1)); v[o:o + n].copy_(st["v"].reshape(-1))
            st["m"], st["v"] = m[o:o + n].view_as(p), v[o:o + n].view_as(p)
            o += n
        # bf16 copies: matrices first, in parameter order - the weights of modules that share an input (BERT's query / key / value)
        # then sit back to back and the towers use them as one [3D, D] operand without a concatenation (towers._wt_stacked)
        o = 0
        for p in sorted(params, key=lambda q: q.dim() < 2):
            n = p.numel()
            self.state[p]["p16"] = p16[o:o + n].view_as(p)
            o += n
        static = np.zeros((len(params), 6), dtype=np.int64)
        for t, p in enumerate(params):
            st = self.state[p]
            static[t, 0], static[t, 2], static[t, 3], static[t, 4] = p.data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), st["p16"].data_ptr()
        plan = self._plans[key] = TensorTable(params, static)
        plan.m, plan.v, plan.p16, plan.p16_filled, plan.stream = m, v, p16, False, None
        return plan

    def _prepare(self, on_own=True):
        """Per-step tables of every bucket (gradient pointers, learning rates) uploaded; reused by the call that follows immediately
        (found_inf_check() then step() inside one scaler.step)."""
        grads_now = tuple(id(p.grad) for g in self.param_groups for p in g["params"])
        if self._prepared is not None and self._prepared[0] == grads_now:
            return self._prepared[1]
        buckets = {}
        for group in self.param_groups:
            key0 = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
            for p in group["params"]:
                if p.grad is not None:
                    st = self._streams.get(id(p))
                    key = key0 + ((st.cuda_stream,) if st is not None else ())
                    buckets.setdefault(key, []).append((p, float(group["lr"]), float(group["weight_decay"])))
        ready = []
        for key, items in buckets.items():
            params = [it[0] for it in items]
            if any(not p.is_contiguous() or p.dtype != torch.float32 for p in params):
                raise TypeError("simseg_amd AdamW expects contiguous fp32 master parameters")
            plan = self._plan(key, params)
            grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params]
            plan.stream = self._streams.get(id(params[0])) if (len(key) > 3 and on_own) else None      # where this step's upload + launch go
            if not plan.p16_filled:
                # a new plan's 16-bit copies start as the masters' values: a skipped AMP step (overflow) writes nothing, yet step()
                # hands the copies to the towers.  Once per plan, on the stream the kernel is launched on (ordered before its writes).
                with (torch.cuda.stream(plan.stream) if plan.stream is not None else contextlib.nullcontext()):
                    for p in params:
                        self.state[p]["p16"].copy_(p.detach())
                plan.p16_filled = True
            plan.upload(grads, {5: pack_lr_wd([it[1] for it in items], [it[2] for it in items])}, plan.stream)
            ready.append((key, plan, params))
        self._prepared = (grads_now, ready)
        return ready

    @torch.no_grad()
    def found_inf_check(self, found_inf):
        """found_inf (float32 scalar tensor on the device) = 1 if any gradient holds an inf / nan: GradScaler's overflow check as one
        read-only launch per bucket over this optimizer's tensor table (simseg_amd.optim.GradScaler calls it instead of torch's
        read-modify-write pass over every gradient tensor)."""
        for key, plan, params in self._prepare(on_own=False):
            call("simseg_grads_nonfinite", *plan.launch_args(), ptr(found_inf), stream())
        return found_inf

    # ---- global gradient norm / clipping over the same tables ---------------------------------------------------------------
    def _norm_pass(self, code, max_norm, loss_scale, row):
        """One read-only launch per bucket into one partials buffer, one finish: _norm_out[row] = {norm, min(1, max_norm / (norm + 1e-6))}."""
        ready = self._prepare(on_own=False)       # every bucket on the current stream: the norm needs them all
        total = sum(plan.n_chunks for _, plan, _ in ready)
        if self._norm_out is None or self._norm_partials.numel() < total:     # (with the plans: the first call, or a re-plan that grew)
            dev = ready[0][1].table.device if ready else self.param_groups[0]["params"][0].device
            self._norm_partials = torch.empty(max(total, 1), device=dev, dtype=torch.float32)
            if self._norm_out is None:
                self._norm_out = torch.zeros(2, 2, device=dev, dtype=torch.float32)
        if loss_scale is not None and (loss_scale.dtype != torch.float32 or not loss_scale.is_cuda):
            raise TypeError("loss_scale: a float32 tensor on the device (torch.amp.GradScaler's scale: optim.live_scale)")
        first = 0
        for key, plan, params in ready:
            call("simseg_grads_norm_partials", *plan.launch_args(), code, ptr(self._norm_partials[first:]), stream())
            first += plan.n_chunks
        call("simseg_grads_norm_finish", ptr(self._norm_partials), first, code, float(max_norm), ptr(loss_scale), ptr(self._norm_out[row]), stream())
        return ready

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, norm_type=2.0, error_if_nonfinite=False, loss_scale=None, materialize=False):
        """torch.nn.utils.clip_grad_norm_ over this optimizer's parameters, fused into the next step(): one read-only pass over the
        gradients (one launch per bucket over the step's own tensor tables, which the step() - and a GradScaler's overflow check - that
        follows reuses: one upload), one finish, and the update kernel multiplies every gradient element by
        min(1, max_norm / (total_norm + 1e-6)) as it reads it.  Returns the total norm, a 0-dim float32 device tensor (a view of a buffer
        the next call overwrites: clone it to keep it).  No allocation after the first call and no host read: it adds to the step nothing
        that a graph capture (simseg_amd/graph.py) or a sync-debug run would trip over.

        * p.grad is left UNCLIPPED; only the update sees the clipped values.  materialize=True also scales p.grad in place (one small
          launch per tensor) for callers that look at the gradients afterwards; step() then applies no coefficient.
        * It arms the NEXT step() only - call it immediately before step() / scaler.step() - and step() disarms it; zero_grad() does too.
          An armed step launches every bucket on the current stream (set_param_streams is ignored, as under a GradScaler).
        * The gradients must be final: call it after any gradient exchange (parallel.GradSync.finish()).  Parameters whose grad is None
          do not count, as in torch.
        * loss_scale (a float32 device scalar: live_scale(scaler)) says the gradients still carry a GradScaler's loss scale: norm and
          coefficient then refer to the UNSCALED gradients - the reference unscales before it clips (core/hooks/optimizer.py:45-47) -
          while the gradients stay scaled until the update kernel divides the scale out.  GradScaler.clip_grad_norm_ passes it.
        * norm_type: 2 or infinity.  error_if_nonfinite=True reads the norm on the host (the only path here that does)."""
        code = norm_type_code(norm_type)
        ready = self._norm_pass(code, max_norm, loss_scale, 0)
        norm, coef = self._norm_out[0, 0], self._norm_out[0, 1:2]
        if error_if_nonfinite and not bool(torch.isfinite(norm)):
            self._prepared = None
            raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be clipped.")
        if materialize:
            for key, plan, params in ready:
                for p, g in zip(params, plan.keepalive):
                    call("simseg_scale_by_scalar", ptr(g), ptr(coef), ptr(g), g.numel(), 1.0, stream())
                    if g is not p.grad:               # (a non-contiguous gradient: the table addresses a contiguous copy)
                        p.grad.copy_(g)
            self._clip_coef = None
        else:
            self._clip_coef = coef
        return norm

    @torch.no_grad()
    def grad_norm(self, norm_type=2.0):
        """The total gradient norm (2 or infinity) as a 0-dim float32 device tensor, by the same read-only pass; arms nothing and leaves an
        armed clip alone.  For logging: no host read; the value is overwritten by the next grad_norm() call.  The gradients must be
        final (after any gradient exchange) and count as they are - under a GradScaler that is the SCALED norm.  It uploads tables of
        its own (the step that follows prepares again)."""
        code = norm_type_code(norm_type)
        self._norm_pass(code, math.inf, None, 1)
        self._prepared = None
        return self._norm_out[1, 0]

    def clip_coef(self):
        """The coefficient min(1, max_norm / (total_norm + 1e-6)) of the last clip_grad_norm_ call: a 0-dim float32 device tensor (1 = the
        clip did not bite), overwritten by the next call."""
        if self._norm_out is None:
            raise RuntimeError("clip_coef(): no clip_grad_norm_ call yet")
        return self._norm_out[0, 1]

    def zero_grad(self, set_to_none=True):
        self._prepared, self._clip_coef = None, None      # tables and a coefficient of gradients that are going away
        super().zero_grad(set_to_none=set_to_none)

    def steps_taken(self):
        """Updates actually applied (a host read of the device counter when a GradScaler drives this optimizer: skipped steps do not count)."""
        if self._step_dev is not None:
            return int(round(float(self._step_dev[self._amp_calls & 1])))
        return self._step

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, param_streams=True):
        # torch.amp.GradScaler.step() sets these two attributes around the call (and deletes them afterwards)
        loss_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        amp = loss_scale is not None or found_inf is not None
        coef, self._clip_coef = self._clip_coef, None      # clip_grad_norm_ armed this step only
        # param_streams=False (or a GradScaler-driven step, whose overflow flag is produced on the current stream; or a clipped one, whose
        # coefficient is): every launch on the current stream, whatever set_param_streams said - the caller's backward did not run on those
        # streams this time
        on_own = param_streams and not amp and coef is None
        ready = self._prepare(on_own)
        self._prepared = None
        if amp:
            if self._step_dev is None:       # the device counter takes over from the host one
                dev = ready[0][1].table.device if ready else torch.device("cuda")
                self._step_dev = torch.full((2,), float(self._step), device=dev, dtype=torch.float32)
                self._amp_calls = 0
            for t in (loss_scale, found_inf):
                if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
                    raise TypeError("grad_scale / found_inf: float32 tensors on the device (torch.amp.GradScaler's)")
        else:
            if self._step_dev is not None:   # back from a GradScaler-driven phase: one host read of how many of its steps were taken
                self._step = self.steps_taken()
                self._step_dev = None
            self._step += 1
        name = "simseg_adamw_multi_step" + ("_amp" if amp else "") + ("_clip" if coef is not None else "")
        for key, plan, params in ready:
            with (torch.cuda.stream(plan.stream) if plan.stream is not None else contextlib.nullcontext()):
                note_half(self.half_dtype)        # (the 16-bit copies are addressed through the table: tell the binding which flavour they are)
                if amp:
                    cur = self._amp_calls & 1
                    own = (float(grad_scale), ptr(loss_scale), ptr(found_inf), ptr(self._step_dev[cur:cur + 1]), ptr(self._step_dev[1 - cur:2 - cur]))
                else:
                    own = (self._step, float(grad_scale))
                call(name, *plan.launch_args(), *key[:3], *own, *((ptr(coef),) if coef is not None else ()), stream())
                for p in params:                 # same stream as the next forward: the copies are current when it runs
                    weights_rewritten(p, self.state[p]["p16"])
        if amp and ready:
            self._amp_calls += 1             # (several buckets: every launch of this call read the same slot and wrote the other; a call
                                             #  with no gradient at all launched nothing - the other slot was not written, so do not flip)

    # ---- checkpoints in torch.optim.AdamW's layout ---------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        steps = self.steps_taken()
        out = {}
        for idx, st in sd["state"].items():
            if "m" in st:
                out[idx] = {"step": torch.tensor(float(steps)), "exp_avg": st["m"].clone(), "exp_avg_sq": st["v"].clone()}
        sd["state"] = out
        for g in sd["param_groups"]:            # keys torch.optim.AdamW.load_state_dict expects to find
            g.setdefault("amsgrad", False)
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        steps, conv = [], {}
        for idx, st in sd["state"].items():
            if "exp_avg" in st:
                conv[idx] = {"m": st["exp_avg"], "v": st["exp_avg_sq"]}
                steps.append(int(float(st["step"])))
            elif "m" in st:                     # round-1 checkpoints of this package
                conv[idx] = {"m": st["m"], "v": st["v"]}
        sd["state"] = conv
        if "_step" in state_dict:
            steps.append(int(state_dict["_step"]))
        super().load_state_dict(sd)
        self._plans.clear()                     # moments are re-packed (and the bf16 copies rewritten) by the next step
        for st in self.state.values():
            st["m"], st["v"] = st["m"].float().contiguous(), st["v"].float().contiguous()
            st.pop("p16", None)
        self._step = max(steps) if steps else 0
        self._step_dev, self._amp_calls, self._prepared, self._clip_coef = None, 0, None, None


class GradScaler(torch.amp.GradScaler):
    """torch.amp.GradScaler (same state, same state_dict, same scale / step / update calls as the reference makes: clip_runner.py:226-230,
    core/hooks/optimizer.py:73-82) whose overflow check of a simseg_amd AdamW is that optimizer's one read-only kernel instead of torch's
    read-modify-write pass over ~400 gradient tensors.  With either scaler the step has no host read: the skip decision stays on the device
    (AdamW._step_supports_amp_scaling)."""

    def __init__(self, device="cuda", **kw):
        super().__init__(device, **kw)

    def _check_inf_per_device(self, optimizer):
        if not isinstance(optimizer, AdamW):
            return super()._check_inf_per_device(optimizer)
        _scale, _ = self._check_scale_growth_tracker("_check_inf_per_device")
        found_inf = torch.zeros((), dtype=torch.float32, device=_scale.device)
        optimizer.found_inf_check(found_inf)
        self._per_optimizer_states[id(optimizer)]["found_inf_per_device"] = {_scale.device: found_inf}
        return self._per_optimizer_states[id(optimizer)]["found_inf_per_device"]

    def clip_grad_norm_(self, optimizer, max_norm, norm_type=2.0, error_if_nonfinite=False, materialize=False):
        """Between backward() and step(optimizer): clips a simseg_amd AdamW's gradients by their global norm, in the reference's order -
        unscale, then clip (core/hooks/optimizer.py:45-47) - without unscaling them: AdamW.clip_grad_norm_ gets the live scale tensor, so
        the norm it returns and the coefficient it arms for step() refer to the unscaled gradients, while the gradients stay scaled until
        the update kernel divides the scale out.  Returns the (unscaled) total norm as a 0-dim device tensor."""
        if not isinstance(optimizer, AdamW):
            raise TypeError("GradScaler.clip_grad_norm_ drives a simseg_amd AdamW; for another optimizer: scaler.unscale_(optimizer), then "
                            "torch.nn.utils.clip_grad_norm_")
        # (after an explicit scaler.unscale_(optimizer) the gradients carry no scale any more, and step() gets none either)
        unscaled = self.is_enabled() and self._per_optimizer_states[id(optimizer)]["stage"] is OptState.UNSCALED
        return optimizer.clip_grad_norm_(max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite,
                                         loss_scale=None if unscaled else live_scale(self), materialize=materialize)


class LARS(torch.optim.Optimizer):
    """Layer-wise adaptive rate scaling for SGD: the reference's simseg.core.optimizer.LARS (lars.py:36-127; same constructor arguments,
    defaults and ValueErrors, the group key `lars_exclude`, the state key `momentum_buffer`) as THREE launches over a tensor table,
    whatever the number of tensors: per-chunk sums of p^2 and g^2, one block per tensor that turns them into the local learning rate
    eta * |p| / (|g| + weight_decay * |p| + eps) ON THE DEVICE (the reference reads both norms on the host: two .item() calls per tensor),
    and the update itself, which also refreshes the 16-bit compute copies the towers read (as AdamW's kernel does).  Parameters are
    bucketed by (momentum, dampening, nesterov, eta); lr, weight_decay and lars_exclude travel per tensor in the table.

    Each step refreshes the table's gradient pointers, learning rates and first-step flags.  Optimizer checkpoints use torch's layout
    with `momentum_buffer`, so they load into the reference's LARS and the reference's load here."""

    def __init__(self, params, lr=required, momentum=0, weight_decay=0, dampening=0, eta=0.001, nesterov=False, eps=1e-8,
                 half_dtype=torch.bfloat16):
        if lr is not required and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if eta < 0.0:
            raise ValueError(f"Invalid LARS coefficient value: {eta}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if half_dtype not in (torch.bfloat16, torch.float16):
            raise TypeError("half_dtype: torch.bfloat16 (the default) or torch.float16")
        self.eps = eps
        self.half_dtype = half_dtype
        self._plans = {}
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, eta=eta))

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)

    # ---- launch plan: row = {p, g, momentum buffer, p16, (lr, weight_decay), flags} --------------------------------------------
    def _plan(self, key, params):
        plan = self._plans.get(key)
        if plan is not None and plan.matches(params):
            return plan
        dev = params[0].device
        starts, o = [], 0
        for p in params:                      # every tensor starts on a 16-byte boundary of the flat buffers (the kernels' 16-byte path)
            starts.append(o)
            o += (p.numel() + 3) // 4 * 4
        total = max(o, 4)
        use_buf = key[0] != 0.0
        buf = torch.zeros(total, device=dev, dtype=torch.float32) if use_buf else None
        p16 = torch.empty(total, device=dev, dtype=self.half_dtype)
        views = []
        static = np.zeros((len(params), 6), dtype=np.int64)
        for t, (p, o) in enumerate(zip(params, starts)):
            st, n = self.state[p], p.numel()
            if use_buf:
                view = buf[o:o + n].view_as(p)
                if "momentum_buffer" in st:       # keep the momentum across a re-plan / a loaded checkpoint
                    view.copy_(st["momentum_buffer"])
                    st["momentum_buffer"] = view
                views.append(view)                # (handed to the state after the tensor's first step: the reference has no buffer before)
            st["p16"] = p16[o:o + n].view_as(p)
            st["p16"].copy_(p.detach())
            static[t, 0], static[t, 2], static[t, 3] = p.data_ptr(), (view.data_ptr() if use_buf else 0), st["p16"].data_ptr()
        plan = self._plans[key] = TensorTable(params, static)
        plan.buf, plan.p16, plan.views = buf, p16, views
        plan.partials = torch.empty(max(plan.n_chunks, 1), 2, device=dev, dtype=torch.float64)
        plan.local_lr = torch.empty(len(params), device=dev, dtype=torch.float32)
        return plan

    def local_lrs(self):
        """{parameter: its local learning rate of the last step} as 0-dim fp32 device tensors (views; the next step overwrites them)."""
        return {p: plan.local_lr[t] for plan in self._plans.values() for t, p in enumerate(plan.params)}

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        buckets = {}
        for group in self.param_groups:
            key = (float(group["momentum"]), float(group["dampening"]), bool(group["nesterov"]), float(group["eta"]))
            exclude = bool(group.get("lars_exclude", False))
            for p in group["params"]:
                if p.grad is not None:
                    buckets.setdefault(key, []).append((p, float(group["lr"]), float(group["weight_decay"]), exclude))
        for key, items in buckets.items():
            params = [it[0] for it in items]
            if any(not p.is_contiguous() or p.dtype != torch.float32 or not p.is_cuda for p in params):
                raise TypeError("simseg_amd LARS expects contiguous fp32 master parameters on the device")
            plan = self._plan(key, params)
            grads = [p.grad if (p.grad.is_contiguous() and p.grad.dtype == torch.float32) else p.grad.float().contiguous() for p in params]
            use_buf = key[0] != 0.0
            flags = [int(it[3]) | (2 if (use_buf and "momentum_buffer" not in self.state[it[0]]) else 0) for it in items]
            plan.upload(grads, {4: pack_lr_wd([it[1] for it in items], [it[2] for it in items]), 5: flags})
            ops.lars_norm_partials(plan, plan.partials)
            ops.lars_finish(plan, plan.partials, key[3], self.eps, plan.local_lr)
            note_half(self.half_dtype)           # (the 16-bit copies are addressed through the table: tell the binding which flavour they are)
            ops.lars_multi_step(plan, plan.local_lr, key[0], key[1], key[2])
            for t, p in enumerate(params):
                if use_buf and "momentum_buffer" not in self.state[p]:
                    self.state[p]["momentum_buffer"] = plan.views[t]
                weights_rewritten(p, self.state[p]["p16"])
        return loss

    # ---- checkpoints in the reference's layout ---------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {idx: {"momentum_buffer": st["momentum_buffer"].clone()} for idx, st in sd["state"].items() if "momentum_buffer" in st}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans.clear()                     # the buffers are re-packed (and the 16-bit copies rewritten) by the next step
        for st in self.state.values():
            st.pop("p16", None)
            if "momentum_buffer" in st:
                st["momentum_buffer"] = st["momentum_buffer"].float().contiguous()
