"""The pinned ring of the optimizers' tensor table (simseg_amd.optim.TensorTable) past its wrap-around: 2 * RING + 1 steps of AdamW and of
LARS over tensors of 1, 3, 8 and CHUNK + 1 elements (a scalar tail only, two 16-byte lanes, a chunk plus a one-element chunk), every step
with a fresh gradient tensor (an address the table has not seen) and its own learning rate, so a row left over from the step that used
the staging buffer RING steps earlier would show.  Every gradient stays alive to the end: a stale address would read old values, not
freed memory.

Expectations and tolerances are the ones of the existing tests of the same comparisons: AdamW against torch.optim.AdamW in fp32 on the same
inputs, within 1e-5 of the largest expected magnitude (tests/test_gpu_kernels.py:1124, test_adamw_multi_tensor_optimizer, and its _close,
:27-31); LARS against the float64 restatement within _lars_ref.LARS_TOL by _lars_ref.rel_dev (tests/test_gpu_linear_probe.py:206-217)."""
import numpy as np
import pytest
import torch

from _lars_ref import LARS_TOL, lars_step64, rel_dev

pytestmark = pytest.mark.gpu


def _problem(seed):
    """-> (sizes, initial values, gradients per step, learning rate per step); CPU generator, float32."""
    from simseg_amd.optim import CHUNK, RING
    g = np.random.default_rng(seed)
    sizes = [1, 3, 8, CHUNK + 1]
    steps = 2 * RING + 1
    p0 = [(g.standard_normal(n) * 0.3).astype(np.float32) for n in sizes]
    grads = [[(g.standard_normal(n) * 0.05).astype(np.float32) for n in sizes] for _ in range(steps + 1)]      # (+ 1: the re-plan step)
    lrs = [1e-3 * (1.0 + 0.37 * s) for s in range(steps + 1)]
    return sizes, p0, grads, lrs


def _fresh_grads(params, gs, seen, alive):
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g).cuda()
        assert p.grad.data_ptr() not in seen
        seen.add(p.grad.data_ptr())
        alive.append(p.grad)


def test_adamw_past_the_ring():
    from simseg_amd.optim import RING, AdamW
    sizes, p0, grads, lrs = _problem(3)
    ours = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in p0]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    kw = dict(lr=lrs[0], betas=(0.9, 0.98), eps=1e-6, weight_decay=1e-2)
    o1, o2 = AdamW(ours, **kw), torch.optim.AdamW(ref, **kw)
    seen, alive = set(), []
    for s in range(2 * RING + 1):
        _fresh_grads(ours, grads[s], seen, alive)
        for q, g in zip(ref, grads[s]):
            q.grad = torch.from_numpy(g).cuda()
        for opt in (o1, o2):
            for group in opt.param_groups:
                group["lr"] = lrs[s]
        o1.step(); o2.step()
    plan, = o1._plans.values()
    assert plan.slot == (2 * RING + 1) % RING and all(e is not None for e in plan.events)            # every buffer used, the first ones twice
    for n, a, b in zip(sizes, ours, ref):
        got, want = a.detach().float().cpu(), b.detach().float().cpu()
        scale = want.abs().max().item() + 1e-12
        err = (got - want).abs().max().item()
        print(f"adamw, {n} elements after {2 * RING + 1} steps: max err {err:.3e} vs scale {scale:.3e}")
        assert err <= 1e-5 * scale
        assert torch.equal(o1.state[a]["p16"], a.detach().bfloat16())


def test_lars_past_the_ring_and_across_a_storage_swap():
    from simseg_amd.optim import LARS, RING
    sizes, p0, grads, lrs = _problem(5)
    hyper = dict(momentum=0.9, weight_decay=1e-4)
    params = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in p0]
    opt = LARS(params, lr=lrs[0], **hyper)
    assert opt.local_lrs() == {}
    p64, buf64 = [a.astype(np.float64) for a in p0], [None] * len(sizes)
    seen, alive = set(), []

    def step(s):
        _fresh_grads(params, grads[s], seen, alive)
        for group in opt.param_groups:
            group["lr"] = lrs[s]
        opt.step()
        for i in range(len(params)):
            p64[i], buf64[i], _ = lars_step64(p64[i], grads[s][i], buf64[i], lr=lrs[s], **hyper)

    def check(tag):
        worst = 0.0
        for i, p in enumerate(params):
            worst = max(worst, rel_dev(p.detach().cpu().numpy(), p64[i]), rel_dev(opt.state[p]["momentum_buffer"].cpu().numpy(), buf64[i]))
            assert torch.equal(opt.state[p]["p16"], p.detach().bfloat16())
        print(f"lars {tag}: largest relative deviation {worst:.3e} (gate {LARS_TOL:.3e})")
        assert worst <= LARS_TOL

    for s in range(2 * RING + 1):              # (no device read in between: the uploads run behind the host)
        step(s)
    check(f"after {2 * RING + 1} steps")
    plan, = opt._plans.values()
    assert plan.slot == (2 * RING + 1) % RING and set(opt.local_lrs()) == set(params)
    # a master's storage is swapped: the next step builds a new table (and keeps the momentum)
    params[2].data = params[2].data.clone()
    step(2 * RING + 1)
    check("after the storage swap")
    new, = opt._plans.values()
    assert new is not plan and new.matches(params) and not plan.matches(params)
