"""The linear-probe task on the MI355X: the fused cross-entropy / top-k / logit-gradient rows, the table-driven LARS and the
LinearProbModel / LinearProbeTrainer around them.

Tolerances are never taken from the code under test.  Cross-entropy: ranks and counts exact; loss rows and gradients within 4 x the
deviation of torch's own fp32 cross_entropy (on the device, same rounded inputs) from the float64 result, pooled over every case of this
file and printed.  LARS: _lars_ref.LARS_TOL, 4 x the deviation of the reference's fp32 trajectories from the float64 restatement (fixed by
tests/test_linear_probe_host.py).  Model: the same rule with torch's fp32 F.linear + cross_entropy head on the same features."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _lars_ref import LARS_TOL, golden_cases, lars_step64, rel_dev, trajectory64
from conftest import GOLD, REPO, tt

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (4, 3), (16, 1000), (7, 1001), (5, 4099), (2, 65536)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
INT_MAX = 2 ** 31 - 1


def _ce_inputs(B, C, seed):
    """Logits (fp32) and labels with the edge rows of the issue; -> (x, labels, {kind: row})."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * 3.0
    y = torch.randint(0, C, (B,), generator=g)
    rows = {}
    if C >= 2 and B >= 3:
        x[0] = -80.0
        x[0, C - 1] = 80.0
        y[0] = C - 1                                  # the maximum at +80, the rest at -80
        rows["plus80"] = 0
        x[1] = 1.5
        y[1] = min(2, C - 1)                          # all equal: the rank is the number of smaller class ids
        rows["equal"] = 1
        r = 2
    else:
        r = 0
    if C >= 2:
        a, b = (0, C - 1) if C < 8 else (5, C - 1)
        x[r, a] = x[r, b] = x[r].max() + 1.0          # a duplicated maximum, the label on the later copy: rank 1, a top-1 miss
        y[r] = b
        rows["dup"] = r
    if B >= 4 and C >= 5:
        y[3] = C                                      # a label outside [0, C)
        rows["bad"] = 3
    if B > 4:
        y[4] = 0
    elif B == 4:
        y[3] = 0
    elif C >= 2 and B == 2:
        y[1] = 0
    return x, y, rows


@pytest.fixture(scope="module")
def ce_cases():
    """Every (shape, dtype) case once: the rounded inputs, the float64 reference and torch's fp32 result on the device, plus the two
    pooled tolerances."""
    cases, dev_loss, dev_grad = {}, 0.0, 0.0
    for si, (B, C) in enumerate(SHAPES):
        x32, y, rows = _ce_inputs(B, C, 100 + si)
        bad = rows.get("bad")
        ok = torch.ones(B, dtype=torch.bool)
        if bad is not None:
            ok[bad] = False
        y_ref = torch.where(ok, y, torch.zeros_like(y))
        for dt in DTYPES:
            xr = x32.to(dt)                                            # the values the kernel sees
            x64 = xr.double()
            loss64 = F.cross_entropy(x64, y_ref, reduction="none")
            xy = x64.gather(1, y_ref[:, None])
            cols = torch.arange(C)[None, :]
            rank = ((x64 > xy) | ((x64 == xy) & (cols < y_ref[:, None]))).sum(1)
            grad64 = (torch.softmax(x64, dim=1) - F.one_hot(y_ref, C).double()) / B
            grad64[~ok] = 0.0
            rank = torch.where(ok, rank, torch.full_like(rank, INT_MAX))
            # torch's own fp32 arithmetic on the device, on the same rounded values
            xd = xr.float().cuda().requires_grad_(True)
            rows32 = F.cross_entropy(xd, y_ref.cuda(), reduction="none")
            (rows32 * ok.cuda()).sum().div(B).backward()
            l32, g32 = rows32.detach().cpu().double(), xd.grad.cpu().double()
            dev_loss = max(dev_loss, float(((l32 - loss64).abs() / loss64.abs().clamp(min=1.0))[ok].max()))
            dev_grad = max(dev_grad, float((g32 - grad64).abs().max()))
            cases[(B, C, dt)] = dict(x=xr.cuda(), y=y.cuda(), ok=ok, rows=rows, loss64=loss64, rank=rank, grad64=grad64)
    tol = dict(loss=4 * dev_loss, grad=4 * dev_grad)
    print(f"\ntorch fp32 cross_entropy vs float64 over {len(cases)} cases: loss rows {dev_loss:.3e} (relative, floor 1), "
          f"gradient {dev_grad:.3e} (absolute) -> gates {tol['loss']:.3e} / {tol['grad']:.3e}")
    return cases, tol


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,C", SHAPES)
def test_ce_rows(ce_cases, B, C, dt):
    from simseg_amd import ops
    cases, tol = ce_cases
    c = cases[(B, C, dt)]
    ok = c["ok"]
    out3, loss_rows, ranks, dlogits = ops.ce_rows(c["x"], c["y"])
    torch.cuda.synchronize()
    loss_rows, ranks, dlogits, out3 = loss_rows.cpu(), ranks.cpu(), dlogits.cpu(), out3.cpu()
    # ranks and counts: exact
    assert torch.equal(ranks.long(), c["rank"])
    assert out3[1].item() == int((c["rank"] < 1).sum()) and out3[2].item() == int((c["rank"] < 5).sum())
    rows = c["rows"]
    if "dup" in rows:
        assert ranks[rows["dup"]] == 1                                  # the label sits on the LATER copy of the maximum: a top-1 miss
    if "equal" in rows:
        assert ranks[rows["equal"]] == min(2, C - 1)                    # equal logits rank by ascending class id
    if C < 5:
        assert out3[2].item() == B                                      # fewer than five classes: every row is a top-5 hit
    # loss rows and gradient against float64, at 4 x torch's own fp32 deviation
    el = ((loss_rows.double() - c["loss64"]).abs() / c["loss64"].abs().clamp(min=1.0))[ok].max().item()
    eg = (dlogits.double() - c["grad64"]).abs().max().item()
    print(f"B={B} C={C} {dt}: loss rows {el:.3e} (gate {tol['loss']:.3e}), gradient {eg:.3e} (gate {tol['grad']:.3e})")
    assert el <= tol["loss"] and eg <= tol["grad"]
    if "bad" in rows:                                                   # NaN loss, zero gradient row, a miss - and nothing else disturbed
        b = rows["bad"]
        assert torch.isnan(loss_rows[b]) and ranks[b] == INT_MAX and not dlogits[b].any()
        assert torch.isfinite(loss_rows[ok]).all()
    else:
        assert torch.isfinite(loss_rows).all()
    # the mean: the index-order double-precision sum of the rows, divided by B, rounded to fp32 - exactly
    acc = 0.0
    for v in loss_rows.double().tolist():
        acc += v
    want = np.float32(acc / B)
    assert np.array_equal(np.float32(out3[0].item()), want, equal_nan=True)
    # a second call gives the same bits
    again = ops.ce_rows(c["x"], c["y"])
    assert torch.equal(again[0].cpu().view(torch.int32), out3.view(torch.int32)) and torch.equal(again[3].cpu(), dlogits)


def test_ce_rows_without_gradient_and_refusals(ce_cases):
    from simseg_amd import ops
    cases, _ = ce_cases
    c = cases[(16, 1000, torch.float32)]
    out3, loss_rows, ranks, dlogits = ops.ce_rows(c["x"], c["y"], write_grad=False)
    full = ops.ce_rows(c["x"], c["y"])
    assert dlogits is None
    assert torch.equal(out3.view(torch.int32), full[0].view(torch.int32)) and torch.equal(ranks, full[2])
    with pytest.raises(RuntimeError, match="ce_rows.*C"):
        ops.ce_rows(torch.zeros(1, 65537, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError, match="int64"):
        ops.ce_rows(c["x"], c["y"].int())


@pytest.mark.parametrize("C", [10, 16])
def test_probe_head_gradients(C):
    """The head node alone, with an input that asks for its gradient (a trainable encoder): dW, db and dx against float64 autograd, at
    4 x the deviation of torch's fp32 head on the device.  C = 16 takes the column-sum kernel for db, C = 10 the GEMM route."""
    from simseg_amd.probe import ProbeHeadFn
    g = torch.Generator().manual_seed(40 + C)
    B, D = 8, 128
    x = torch.randn(B, D, generator=g)
    w = torch.randn(C, D, generator=g) * 0.1
    b = torch.randn(C, generator=g) * 0.1
    y = torch.randint(0, C, (B,), generator=g)
    up = 0.37                                                            # an upstream gradient other than 1
    def grads(dtype, dev):
        t = [v.to(device=dev, dtype=dtype).requires_grad_(True) for v in (x, w, b)]
        (F.cross_entropy(F.linear(*t), y.to(dev)) * up).backward()
        return [v.grad.double().cpu().numpy() for v in t]
    want, ref32 = grads(torch.float64, "cpu"), grads(torch.float32, "cuda")
    t = [v.cuda().requires_grad_(True) for v in (x, w, b)]
    loss, out3, logits = ProbeHeadFn.apply(t[0], t[1], t[2], y.cuda())
    assert not out3.requires_grad and not logits.requires_grad
    (loss * up).backward()
    for name, v, w64, r32 in zip(("dx", "dW", "db"), t, want, ref32):
        got, gate = rel_dev(v.grad.cpu().numpy(), w64), 4 * rel_dev(r32, w64)
        print(f"C={C} {name}: {got:.3e} (gate {gate:.3e})")
        assert got <= gate, name


# ---- LARS ---------------------------------------------------------------------------------------------------------------------------
def _run_lars(kws, p0, grads, half=torch.bfloat16, groups=None):
    """Three steps of simseg_amd.optim.LARS on the device; -> (optimizer, params, [p per step], [buf per step], [local lr per step])
    and checks the 16-bit copy after every step."""
    from simseg_amd.optim import LARS
    params = [torch.nn.Parameter(tt(np.asarray(a, dtype=np.float32)).cuda()) for a in p0]
    if groups is None:
        groups = [dict(params=[p], lr=kw["lr"], momentum=kw.get("momentum", 0.0), weight_decay=kw.get("weight_decay", 0.0),
                       dampening=kw.get("dampening", 0.0), eta=kw.get("eta", 0.001), nesterov=kw.get("nesterov", False),
                       lars_exclude=kw.get("exclude", False)) for p, kw in zip(params, kws)]
    else:
        groups = groups(params)
    opt = LARS(groups, lr=kws[0]["lr"], eps=kws[0].get("eps", 1e-8), half_dtype=half)
    ps, bufs, lls = [], [], []
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = tt(np.asarray(g, dtype=np.float32)).cuda()
        opt.step()
        torch.cuda.synchronize()
        for p in params:
            assert torch.equal(opt.state[p]["p16"], p.detach().to(half))           # the 16-bit copy is the rounded master
        ps.append([p.detach().cpu().numpy().copy() for p in params])
        bufs.append([opt.state[p]["momentum_buffer"].cpu().numpy().copy() if "momentum_buffer" in opt.state[p] else None for p in params])
        ll = opt.local_lrs()
        lls.append([float(ll[p]) for p in params])
    return opt, params, ps, bufs, lls


def _check_trajectory(tag, got_p, got_buf, want_p, want_buf, tol=LARS_TOL):
    worst = 0.0
    for s in range(len(want_p)):
        for i in range(len(want_p[s])):
            worst = max(worst, rel_dev(got_p[s][i], want_p[s][i]))
            if want_buf[s][i] is not None:
                assert got_buf[s][i] is not None
                worst = max(worst, rel_dev(got_buf[s][i], want_buf[s][i]))
            else:
                assert got_buf[s][i] is None
    print(f"{tag}: largest relative deviation {worst:.3e} (gate {tol:.3e})")
    assert worst <= tol
    return worst


@pytest.mark.parametrize("case", ["m9", "m9_wd_nesterov", "m9_wd_damp_exclude"])
def test_lars_against_the_golden_and_the_restatement(case):
    c = golden_cases(np.load(os.path.join(GOLD, "linear_prob_head.npz")))[case]
    _, _, ps, bufs, lls = _run_lars(c["kws"], c["p0"], c["g"])
    _check_trajectory(case + " vs the reference's fp32 result", ps, bufs, c["p"], c["buf"])
    p64, b64, l64 = trajectory64(c["kws"], c["p0"], c["g"])
    _check_trajectory(case + " vs the float64 restatement", ps, bufs, p64, b64)
    for s in range(3):
        assert np.allclose(lls[s], l64[s], rtol=1e-6, atol=0)
        assert all(l == 1.0 for l, kw in zip(lls[s], c["kws"]) if kw["exclude"])


HYPER = {
    "momentum0": dict(lr=0.5, momentum=0.0, weight_decay=0.0),
    "m9_wd": dict(lr=0.5, momentum=0.9, weight_decay=1e-4),
    "m9_damp": dict(lr=0.5, momentum=0.9, dampening=0.1, weight_decay=0.0),
    "m9_nesterov_wd": dict(lr=0.5, momentum=0.9, nesterov=True, weight_decay=1e-4),
}


def _sized_problem(seed=7):
    from simseg_amd.optim import CHUNK
    g = np.random.default_rng(seed)
    sizes = [1, 63, 65, 7680, CHUNK + 1, 65, 63, 12]          # the sixth has a zero gradient, the seventh zero weights, the last is excluded
    p0 = [(g.standard_normal(n) * 0.3).astype(np.float32) for n in sizes]
    p0[6][:] = 0.0
    grads = []
    for _ in range(3):
        gs = [(g.standard_normal(n) * 0.05).astype(np.float32) for n in sizes]
        gs[5][:] = 0.0
        grads.append(gs)
    return sizes, p0, grads


@pytest.mark.parametrize("half", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hyper", list(HYPER))
def test_lars_sizes_and_hyperparameters(hyper, half):
    """Tensors of 1, 63, 65 and 7 680 elements, one of chunk + 1 (two chunks), a zero gradient, zero weights (local lr 1 for both) and a
    lars_exclude tensor; three steps against the float64 restatement."""
    sizes, p0, grads = _sized_problem()
    kws = [dict(HYPER[hyper], exclude=(i == len(sizes) - 1)) for i in range(len(sizes))]
    opt, params, ps, bufs, lls = _run_lars(kws, p0, grads, half=half)
    p64, b64, l64 = trajectory64(kws, p0, grads)
    _check_trajectory(f"{hyper} {half}", ps, bufs, p64, b64)
    for s in range(3):
        assert lls[s][5] == 1.0 and lls[s][7] == 1.0 and (s > 0 or lls[s][6] == 1.0)
        assert np.allclose(lls[s], l64[s], rtol=1e-6, atol=0)
    assert len(opt._plans) == 1 and next(iter(opt._plans.values()))["n_chunks"] == len(sizes) + 1      # one table, the big tensor in two chunks


def test_lars_continues_identically_from_a_state_dict():
    from simseg_amd.optim import LARS
    sizes, p0, grads = _sized_problem(seed=11)
    kw = HYPER["m9_wd"]
    kws = [dict(kw) for _ in sizes]
    opt, params, ps, _, _ = _run_lars(kws, p0, grads[:2])
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = LARS([dict(params=[p]) for p in clones], lr=123.0, momentum=0.0)        # (everything that matters comes from the state dict)
    opt2.load_state_dict(opt.state_dict())
    assert opt2.param_groups[0]["lr"] == kw["lr"] and opt2.param_groups[0]["momentum"] == 0.9
    for p, q, g in zip(params, clones, grads[2]):
        p.grad = tt(g).cuda()
        q.grad = tt(g).cuda()
    opt.step()
    opt2.step()
    for p, q in zip(params, clones):
        assert torch.equal(p, q) and torch.equal(opt.state[p]["momentum_buffer"], opt2.state[q]["momentum_buffer"])
        assert torch.equal(opt.state[p]["p16"], opt2.state[q]["p16"])


def test_corrupted_tables_are_refused():
    """A tensor id out of range, a negative size and a chunk offset past the end are refused on the host, under the entry point's name,
    before anything is launched; so is a broken chunk range of the finish."""
    from simseg_amd import ops
    sizes, p0, grads = _sized_problem(seed=13)
    kws = [dict(HYPER["m9_wd"]) for _ in sizes]
    opt, params, _, _, _ = _run_lars(kws, p0, grads[:1])
    plan = next(iter(opt._plans.values()))
    before = [p.detach().clone() for p in params]
    T, n = plan["n_tensors"], plan["n_chunks"]

    def broken(key, idx, val):
        bad = copy.copy(plan)
        setattr(bad, key, getattr(plan, key).copy())
        getattr(bad, key)[idx] = val
        return bad

    for key, idx, val, what in [("tid_host", 0, T, "tensor id"), ("tid_host", n - 1, -1, "tensor id"), ("sizes_host", 2, -5, "negative size"),
                                ("coff_host", n - 1, sizes[-1], "past the end"), ("coff_host", 0, -1, "past the end")]:
        with pytest.raises(RuntimeError, match=f"lars_norm_partials.*{what}"):
            ops.lars_norm_partials(broken(key, idx, val), plan["partials"])
        with pytest.raises(RuntimeError, match=f"lars_multi_step.*{what}"):
            ops.lars_multi_step(broken(key, idx, val), plan["local_lr"], 0.9, 0.0, False)
    with pytest.raises(RuntimeError, match="lars_finish.*chunk range"):
        ops.lars_finish(broken("first_host", T, n + 1), plan["partials"], 0.001, 1e-8, plan["local_lr"])
    with pytest.raises(RuntimeError, match="lars_finish.*chunk range"):
        ops.lars_finish(broken("first_host", 1, n), plan["partials"], 0.001, 1e-8, plan["local_lr"])
    with pytest.raises(RuntimeError, match="lars_multi_step.*Nesterov"):
        ops.lars_multi_step(plan, plan["local_lr"], 0.9, 0.1, True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, p) for a, p in zip(before, params))                   # nothing was launched


# ---- model ----------------------------------------------------------------------------------------------------------------------------
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.classifier.num_classes=10", "optim.lr.warmup_proportion=0.0", "epoch=2", "ckpt.only_load_image_encoder=False"]


def _build(seed=0):
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.linear_prob.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/linear_prob/imagenet.yaml"), TINY, update_clip_config)
    torch.manual_seed(seed)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    g = np.load(os.path.join(GOLD, "clip_glue.npz"))
    sd = {k[3:]: tt(g[k]) for k in g.files if k.startswith("sd.image_encoder.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and sorted(missing) == ["classifier.bias", "classifier.weight"]
    return model.cuda().train(), cfg


def _batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.randn(B, 3, 96, 96, generator=g).cuda(), "label": torch.randint(0, 10, (B,), generator=g).cuda()}


def _head64(x, w, b, y):
    """float64 head on the CPU: (logits, loss, dW, db)."""
    w = w.detach().double().cpu().requires_grad_(True)
    b = b.detach().double().cpu().requires_grad_(True)
    logits = F.linear(x.double().cpu(), w, b)
    loss = F.cross_entropy(logits, y.cpu())
    loss.backward()
    return logits.detach(), loss.detach(), w.grad, b.grad


def _lars_update(p, g, lr):
    return lars_step64(p.detach().cpu().double().numpy(), g.detach().cpu().double().numpy(), None, lr=lr, momentum=0.9, weight_decay=0.0)[0]


def test_train_step_against_a_torch_head_on_the_same_features():
    from simseg_amd.probe import LinearProbeTrainer
    model, cfg = _build()
    trainer = LinearProbeTrainer(model, cfg, steps_per_epoch=10)
    batch = _batch(8, 1)
    enc0 = {k: v.detach().clone() for k, v in model.image_encoder.named_parameters()}
    w0, b0 = model.classifier.weight.detach().clone(), model.classifier.bias.detach().clone()
    feats = model.forward_image_feature(batch["image"])
    assert feats.shape == (8, 128) and not feats.requires_grad
    x = feats.float()
    # references: float64, and torch's own fp32 head on the device (its deviation from float64 sets the gates)
    lg64, loss64, dw64, db64 = _head64(x, w0, b0, batch["label"])
    w32, b32 = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    lg32 = F.linear(x, w32, b32)
    loss32 = F.cross_entropy(lg32, batch["label"])
    loss32.backward()
    lr = cfg.optim.lr.init
    assert lr == 6.4 and trainer.set_lrs(0) == [6.4, 6.4]
    w1_64, b1_64 = _lars_update(w0, dw64, lr), _lars_update(b0, db64, lr)
    w1_32 = _lars_update(w0, w32.grad, lr).astype(np.float32)
    b1_32 = _lars_update(b0, b32.grad, lr).astype(np.float32)
    # the loss is 2-Lipschitz in the logits (maximum norm), so the scale of its fp32 error is the logits' own: the gate is 4 x (torch's
    # deviation on the loss + its largest deviation on a logit) - one number alone could land on the float64 value's rounding by chance
    dev_logit = float((lg32.detach().cpu().double() - lg64).abs().max())
    gates = dict(loss=4 * (abs(loss32.item() - loss64.item()) + dev_logit), w=4 * rel_dev(w1_32, w1_64), b=4 * rel_dev(b1_32, b1_64))
    out = trainer.train_step(batch)
    torch.cuda.synchronize()
    got = dict(loss=abs(out["loss"].item() - loss64.item()),
               w=rel_dev(model.classifier.weight.detach().cpu().numpy(), w1_64), b=rel_dev(model.classifier.bias.detach().cpu().numpy(), b1_64))
    print("train step vs the float64 head + LARS:", {k: f"{v:.3e}" for k, v in got.items()}, "gates", {k: f"{v:.3e}" for k, v in gates.items()})
    assert got["loss"] <= gates["loss"] and got["w"] <= gates["w"] and got["b"] <= gates["b"]
    top = lg64.topk(5, dim=1).indices
    hit = top == batch["label"].cpu()[:, None]
    assert out["acc1"].shape == (1,) and out["acc1"].item() == 100.0 * hit[:, :1].sum().item() / 8
    assert out["acc5"].item() == 100.0 * hit.sum().item() / 8
    assert trainer.step == 1 and out["lr"] == 6.4
    # the frozen encoder: bit-identical, and no gradient anywhere
    for k, v in model.image_encoder.named_parameters():
        assert torch.equal(v, enc0[k]) and v.grad is None, k
    assert not model.image_encoder.training and model.training
    # forward(valid=True): the prediction is the linear layer on those features
    w1, b1 = model.classifier.weight.detach(), model.classifier.bias.detach()
    loss_dict, pred, label = model(batch, valid=True)
    assert list(loss_dict) == ["crossentropy_loss"] and label is batch["label"]
    want = F.linear(x.double().cpu(), w1.double().cpu(), b1.double().cpu())
    dev32 = rel_dev(F.linear(x, w1, b1).cpu().numpy(), want.numpy())
    got_lg = rel_dev(pred.cpu().numpy(), want.numpy())
    print(f"valid logits vs float64 F.linear: {got_lg:.3e} (torch fp32: {dev32:.3e}, gate {4 * dev32:.3e})")
    assert got_lg <= 4 * dev32


def test_evaluate_accumulates_over_batches(ce_cases):
    from simseg_amd.probe import LinearProbeTrainer
    _, tol = ce_cases
    model, cfg = _build(seed=1)
    trainer = LinearProbeTrainer(model, cfg, steps_per_epoch=10)
    batches = [_batch(8, 21), _batch(5, 22), _batch(3, 23)]
    res = trainer.evaluate(batches)
    assert model.training                                                # evaluate() restores the mode
    with torch.no_grad():
        logits = torch.cat([model(b, valid=True)[1] for b in batches]).double().cpu()
    labels = torch.cat([b["label"] for b in batches]).cpu()
    top = logits.topk(5, dim=1).indices
    hit = top == labels[:, None]
    assert res["count"] == 16
    assert res["acc1"] == 100.0 * hit[:, :1].sum().item() / 16 and res["acc5"] == 100.0 * hit.sum().item() / 16
    want = F.cross_entropy(logits, labels).item()
    print(f"evaluate loss {res['loss']:.9f} vs float64 on the concatenated logits {want:.9f}")
    assert abs(res["loss"] - want) <= (tol["loss"] + 2.0 ** -23) * max(1.0, abs(want))      # (+ the fp32 rounding of each batch's mean)


def test_checkpoint_round_trip_continues_identically():
    from simseg_amd.probe import LinearProbeTrainer
    model, cfg = _build(seed=2)
    trainer = LinearProbeTrainer(model, cfg, steps_per_epoch=10)
    trainer.train_step(_batch(8, 31))
    trainer.train_step(_batch(8, 32))
    ckpt = trainer.checkpoint()
    assert set(ckpt) == {"state_dict", "optimizer", "meta"} and ckpt["meta"]["step"] == 2
    assert all(set(st) == {"momentum_buffer"} for st in ckpt["optimizer"]["state"].values()) and len(ckpt["optimizer"]["state"]) == 2
    ckpt = {k: (v if k == "meta" else _clone(v)) for k, v in ckpt.items()}
    other, _ = _build(seed=5)                                            # a different classifier initialisation
    t2 = LinearProbeTrainer(other, cfg, steps_per_epoch=10)
    missing, unexpected = t2.load_checkpoint(ckpt)
    assert not missing and not unexpected and t2.step == 2
    a, b = trainer.train_step(_batch(8, 33)), t2.train_step(_batch(8, 33))
    torch.cuda.synchronize()
    assert torch.equal(a["loss"], b["loss"]) and a["lr"] == b["lr"]
    assert torch.equal(model.classifier.weight, other.classifier.weight) and torch.equal(model.classifier.bias, other.classifier.bias)


def _clone(obj):
    if torch.is_tensor(obj):
        return obj.detach().clone()
    if isinstance(obj, dict):
        return {k: _clone(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_clone(v) for v in obj)
    return obj
