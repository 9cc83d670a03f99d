"""Mixup / CutMix on the MI355X: the in-place mix kernel bit for bit against its host statement, the two-label soft-target cross-entropy rows
against float64, the soft head's gradients, and the model / trainer / Mixup.apply around them.

Tolerances are never taken from the code under test.  The mix is exact (bits).  Soft cross-entropy: ranks and counts exact; loss rows and
gradients within 4 x the deviation of torch's own fp32 dense-target computation (on the device, same rounded inputs) from the float64
result, pooled over every case of this file and printed - the rule of tests/test_gpu_linear_probe.py::test_ce_rows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _lars_ref import rel_dev
from _mix_ref import INT_MAX, dense_target64, ranks64, soft_ce64
from test_gpu_linear_probe import _batch, _build, _ce_inputs

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- mix_batch ------------------------------------------------------------------------------------------------------------------------
LAMS = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 0.3, 0.8125]


def _boxes(H, W):
    """empty, one pixel (the last one), the full image, touching the right edge, the top-left corner, an interior box, a one-row strip."""
    return [(0, 0, 0, 0), (H - 1, H, W - 1, W), (0, H, 0, W), (0, H, W // 2, W), (0, max(1, H // 2), 0, max(1, W // 2)),
            (min(1, H - 1), max(H - 1, 1), min(1, W - 1), max(W - 1, 1)), (H // 2, H // 2 + 1, 0, W), (2 % H, H, 0, 0)]


def _tables(B, H, W):
    from simseg_amd.mixup import explicit_params
    bx = _boxes(H, W)
    out = {"mixup": explicit_params([1] * B, [LAMS[i % len(LAMS)] for i in range(B)])}
    for s in range(0, len(bx), 2):                # cutmix, a different box per row: every box meets every position of a pair over the shifts
        out[f"cutmix{s}"] = explicit_params([2] * B, [0.5] * B, [bx[(i + s) % len(bx)] for i in range(B)])
    out["cutmix_pair"] = explicit_params([2] * B, [0.5] * B, [bx[min(i, B - 1 - i) + 3] for i in range(B)])        # same box on both rows
    # elem: row 0 is a mixup row whose partner is a cutmix row with a box; further rows alternate, with a kind-0 row when there is room
    kinds = [1, 2, 0, 1, 2][:B - 1] + [2]
    out["elem"] = explicit_params(kinds, [LAMS[(i + 2) % len(LAMS)] for i in range(B)], [bx[(i + 4) % len(bx)] for i in range(B)])
    out["elem_rev"] = explicit_params(kinds[::-1], [LAMS[(i + 1) % len(LAMS)] for i in range(B)], [bx[(i + 5) % len(bx)] for i in range(B)])
    out["none"] = explicit_params([0] * B, [1.0] * B)
    return out


def _images(B, H, W, dtype, seed, offset=0):
    """A batch with a few special values; offset: elements past a 16-byte boundary at which the batch starts."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g) * 2.0
    flat = x.view(-1)
    flat[0] = -0.0
    flat[-1] = 1e-30
    flat[flat.numel() // 2] = 6.0e4
    x = x.to(dtype)
    buf = torch.zeros(x.numel() + 16, dtype=dtype, device="cuda")
    dev = buf[offset:offset + x.numel()].view(B, 3, H, W)
    dev.copy_(x)
    assert dev.is_contiguous() and dev.data_ptr() % 16 == (offset * x.element_size()) % 16
    return x, dev


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (16, 16), (33, 19)])
@pytest.mark.parametrize("B", [2, 4, 6])
def test_mix_batch_bits(B, H, W, dtype):
    from simseg_amd import ops
    from simseg_amd.mixup import mix_ref
    for name, p in _tables(B, H, W).items():
        for offset in ((0, 1) if (H, W) == (16, 16) else (0,)):          # one element off 16 bytes: the vector path has to stand down
            x, dev = _images(B, H, W, dtype, 7 * B + H, offset)
            want = mix_ref(x, p)
            tab = torch.from_numpy(p["table"]).cuda()
            got = ops.mix_batch(dev, tab, p["table"])
            assert got is dev
            torch.cuda.synchronize()
            first = dev.cpu()
            assert torch.equal(_bits(first), _bits(want)), (name, offset)
            for i in np.nonzero(p["table"][:, 0] == 0)[0]:                # a kind-0 row keeps its bits
                assert torch.equal(_bits(first[i]), _bits(x[i]))
            dev.copy_(x)                                                  # the same input again: the same bits
            ops.mix_batch(dev, tab, p["table"])
            assert torch.equal(_bits(dev.cpu()), _bits(first)), (name, offset)


def test_mix_batch_refusals():
    from simseg_amd import ops
    from simseg_amd.mixup import explicit_params

    def refused(x, p, match):
        keep = x.clone()
        tab = torch.from_numpy(p["table"]).cuda()
        with pytest.raises(RuntimeError, match=match):
            ops.mix_batch(x, tab, p["table"])
        torch.cuda.synchronize()
        assert torch.equal(x, keep)                                       # nothing was launched

    x = torch.randn(4, 3, 5, 7, device="cuda")
    refused(torch.randn(3, 3, 5, 7, device="cuda"), explicit_params([1, 1, 1], [0.5] * 3), "mix_batch.*even")
    refused(x, explicit_params([2, 2, 2, 2], [0.5] * 4, [(0, 5, 0, 7), (0, 5, 0, 7), (0, 6, 0, 7), (0, 5, 0, 7)]), "mix_batch.*sample 2")
    refused(x, explicit_params([2, 2, 2, 2], [0.5] * 4, [(0, 5, 0, 7), (3, 2, 0, 7), (0, 5, 0, 7), (0, 5, 0, 7)]), "mix_batch.*sample 1")
    refused(x, explicit_params([1, 1, 1, 3], [0.5] * 4), "mix_batch.*sample 3 has kind 3")
    refused(x, explicit_params([1, 1, 1, 1], [0.5, float("nan"), 0.5, 0.5]), "mix_batch.*sample 1")
    refused(x, explicit_params([1, 1, 1, 1], [1.5, 0.5, 0.5, 0.5]), "mix_batch.*sample 0")
    p = explicit_params([1, 1, 1, 1], [0.5] * 4)
    refused(torch.randn(4, 3, 7, 5, device="cuda").transpose(2, 3), p, "mix_batch.*contiguous")
    with pytest.raises(ValueError, match="mix_batch"):
        ops.mix_batch(x, torch.from_numpy(p["table"][:2]).cuda(), p["table"])
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mix_batch(x.cpu(), torch.from_numpy(p["table"]).cuda(), p["table"])


def test_mixup_apply_end_to_end():
    from simseg_amd.mixup import Mixup, mix_ref
    rng = np.random.default_rng(21)
    for mode, dtype in (("batch", torch.float32), ("pair", torch.bfloat16), ("elem", torch.float32), ("elem", torch.float16)):
        mix = Mixup(0.8, 1.0, mode=mode, label_smoothing=0.1, num_classes=10)
        x = torch.randn(6, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(dtype)
        labels = torch.arange(6).cuda()
        p = mix.sample(6, 32, 32, rng)
        dev = x.cuda()
        out, tgt = mix.apply(dev, labels, p)
        torch.cuda.synchronize()
        assert out is dev and torch.equal(_bits(dev.cpu()), _bits(mix_ref(x, p)))
        assert tgt["label"] is labels and torch.equal(tgt["label_b"], labels.flip(0)) and tgt["smoothing"] == 0.1
        assert tgt["lam"].dtype == torch.float32 and tgt["lam"].is_contiguous() and np.array_equal(tgt["lam"].cpu().numpy(), p["lam"])


# ---- soft_ce_rows ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 5), (4, 3), (16, 1000), (7, 1001), (5, 4099), (2, 65536)]
EPS = [0.0, 0.1]
LAM_ROWS = [1.0, 0.0, 0.5, 0.3]


def _soft_inputs(B, C, seed):
    """test_ce_rows' logits and labels (the +80 / -80 row, the all-equal row, the duplicated maximum, a bad label in a) plus partner labels
    (a == b on some rows, a bad label in b on a row of its own) and lam cycling through {1, 0, 0.5, 0.3}."""
    x, a, rows = _ce_inputs(B, C, seed)
    g = torch.Generator().manual_seed(seed + 50)
    b = torch.randint(0, C, (B,), generator=g)
    b[B - 1] = a[B - 1] if 0 <= a[B - 1] < C else 0                       # a == b
    if "equal" in rows:
        b[rows["equal"]] = a[rows["equal"]]
    rows = dict(rows)
    if B >= 5 and C >= 5:
        rows["bad_b"] = 5 if B >= 7 else 4
        b[rows["bad_b"]] = -1 if B % 2 else C + 7
    lam = torch.tensor([LAM_ROWS[(i + 1) % 4] if i else 0.3 for i in range(B)], dtype=torch.float32)
    return x, a, b, lam, rows


@pytest.fixture(scope="module")
def soft_cases():
    cases, dev_loss, dev_grad = {}, 0.0, 0.0
    for si, (B, C) in enumerate(SHAPES):
        x32, a, b, lam, rows = _soft_inputs(B, C, 101 + si)               # (seeds: test_ce_rows' own, its SHAPES start one shape earlier)
        ok = (a >= 0) & (a < C) & (b >= 0) & (b < C)
        a_ref, b_ref = torch.where(ok, a, torch.zeros_like(a)), torch.where(ok, b, torch.zeros_like(b))
        for dt in DTYPES:
            xr = x32.to(dt)
            x64 = xr.double()
            rank = torch.where(ok, ranks64(x64, a_ref), torch.full_like(a, INT_MAX))
            for eps in EPS:
                t64 = dense_target64(a_ref, b_ref, lam.numpy(), eps, C)
                loss64, grad64 = soft_ce64(x64, t64)
                grad64[~ok] = 0.0
                # torch's own fp32 arithmetic on the device with the DENSE target, on the same rounded values
                xd = xr.float().cuda().requires_grad_(True)
                rows32 = -(t64.float().cuda() * F.log_softmax(xd, dim=1)).sum(1)
                (rows32 * ok.cuda()).sum().div(B).backward()
                l32, g32 = rows32.detach().cpu().double(), xd.grad.cpu().double()
                dl = float(((l32 - loss64).abs() / loss64.abs().clamp(min=1.0))[ok].max())
                dg = float((g32 - grad64).abs().max())
                dev_loss, dev_grad = max(dev_loss, dl), max(dev_grad, dg)
                cases[(B, C, dt, eps)] = dict(x=xr.cuda(), a=a.cuda(), b=b.cuda(), lam=lam.cuda(), ok=ok, rows=rows, loss64=loss64, rank=rank,
                                              grad64=grad64, torch_dev=(dl, dg))
    tol = dict(loss=4 * dev_loss, grad=4 * dev_grad)
    print(f"\ntorch fp32 dense-target cross-entropy vs float64 over {len(cases)} cases: loss rows {dev_loss:.3e} (relative, floor 1), "
          f"gradient {dev_grad:.3e} (absolute) -> gates {tol['loss']:.3e} / {tol['grad']:.3e}")
    return cases, tol


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_soft_ce_rows(soft_cases, B, C, dt, eps):
    from simseg_amd import ops
    cases, tol = soft_cases
    c = cases[(B, C, dt, eps)]
    ok, rows = c["ok"], c["rows"]
    out3, loss_rows, ranks, dlogits = ops.soft_ce_rows(c["x"], c["a"], c["b"], c["lam"], smoothing=eps)
    torch.cuda.synchronize()
    loss_rows, ranks, dlogits, out3 = loss_rows.cpu(), ranks.cpu(), dlogits.cpu(), out3.cpu()
    assert torch.equal(ranks.long(), c["rank"])                           # ranks against the sample's own label, exact
    assert out3[1].item() == int((c["rank"] < 1).sum()) and out3[2].item() == int((c["rank"] < 5).sum())
    if "dup" in rows:
        assert ranks[rows["dup"]] == 1
    if "equal" in rows:
        assert ranks[rows["equal"]] == min(2, C - 1)
    el = ((loss_rows.double() - c["loss64"]).abs() / c["loss64"].abs().clamp(min=1.0))[ok].max().item()
    eg = (dlogits.double() - c["grad64"]).abs().max().item()
    print(f"B={B} C={C} {dt} eps={eps}: loss rows {el:.3e} (torch {c['torch_dev'][0]:.3e}, gate {tol['loss']:.3e}), "
          f"gradient {eg:.3e} (torch {c['torch_dev'][1]:.3e}, gate {tol['grad']:.3e})")
    assert el <= tol["loss"] and eg <= tol["grad"]
    for key in ("bad", "bad_b"):                                          # a bad label in a, and one in b: NaN, a miss, a zero gradient row
        if key in rows:
            r = rows[key]
            assert not ok[r] and torch.isnan(loss_rows[r]) and ranks[r] == INT_MAX and not dlogits[r].any()
    assert torch.isfinite(loss_rows[ok]).all() and int((~ok).sum()) == sum(k in rows for k in ("bad", "bad_b"))
    acc = 0.0
    for v in loss_rows.double().tolist():
        acc += v
    assert np.array_equal(np.float32(out3[0].item()), np.float32(acc / B), equal_nan=True)      # the index-order double sum, exactly
    again = ops.soft_ce_rows(c["x"], c["a"], c["b"], c["lam"], smoothing=eps)
    assert torch.equal(_bits(again[0].cpu()), _bits(out3)) and torch.equal(_bits(again[1].cpu()), _bits(loss_rows))
    assert torch.equal(again[3].cpu(), dlogits)
    nograd = ops.soft_ce_rows(c["x"], c["a"], c["b"], c["lam"], smoothing=eps, write_grad=False)
    assert nograd[3] is None and torch.equal(_bits(nograd[0].cpu()), _bits(out3)) and torch.equal(nograd[2].cpu(), ranks)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_soft_ce_rows_degenerates_to_ce_rows_bit_for_bit(soft_cases, B, C, dt):
    """lam = 1, eps = 0: loss rows, ranks, gradient and out3 are ce_rows' bits, whatever the (valid) partner label is."""
    from simseg_amd import ops
    c = soft_cases[0][(B, C, dt, 0.0)]
    a = c["a"]
    a_ok = (a >= 0) & (a < C)
    ones = torch.ones(B, device="cuda")
    for b in (a, torch.where(a_ok, (a + 1) % C, a)):
        for wg in (True, False):
            soft = ops.soft_ce_rows(c["x"], a, b, ones, smoothing=0.0, write_grad=wg)
            hard = ops.ce_rows(c["x"], a, write_grad=wg)
            for s, h in zip(soft[:3], hard[:3]):
                assert torch.equal(_bits(s), _bits(h))
            assert (soft[3] is None and hard[3] is None) if not wg else torch.equal(_bits(soft[3]), _bits(hard[3]))


def test_soft_ce_rows_refusals(soft_cases):
    from simseg_amd import ops
    c = soft_cases[0][(16, 1000, torch.float32, 0.1)]
    with pytest.raises(RuntimeError, match="soft_ce_rows.*smoothing"):
        ops.soft_ce_rows(c["x"], c["a"], c["b"], c["lam"], smoothing=1.0)
    with pytest.raises(TypeError, match="int64"):
        ops.soft_ce_rows(c["x"], c["a"], c["b"].int(), c["lam"])
    with pytest.raises(TypeError, match="fp32"):
        ops.soft_ce_rows(c["x"], c["a"], c["b"], c["lam"].double())
    with pytest.raises(ValueError, match="soft_ce_rows"):
        ops.soft_ce_rows(c["x"], c["a"], c["b"], c["lam"][:3])
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.soft_ce_rows(c["x"], c["a"], c["b"], c["lam"].cpu())


# ---- heads and losses -----------------------------------------------------------------------------------------------------------------
def _dense_head(x, w, b, t, dtype, dev, up):
    """Gradients of up * mean(-sum_c t_c log softmax(x W^T + b)_c) by torch autograd."""
    v = [u.detach().to(device=dev, dtype=dtype, copy=True).requires_grad_(True) for u in (x, w, b)]
    loss = -(t.to(device=dev, dtype=dtype) * F.log_softmax(F.linear(*v), dim=1)).sum(1).mean()
    (loss * up).backward()
    return loss.item(), [u.grad.double().cpu().numpy() for u in v]


@pytest.mark.parametrize("C", [10, 16])
def test_soft_probe_head_gradients(C):
    from simseg_amd.probe import SoftProbeHeadFn
    g = torch.Generator().manual_seed(60 + C)
    B, D, eps, up = 8, 128, 0.1, 0.37
    x = torch.randn(B, D, generator=g)
    w = torch.randn(C, D, generator=g) * 0.1
    b = torch.randn(C, generator=g) * 0.1
    ya, yb = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    lam = torch.tensor([1.0, 0.0, 0.5, 0.3, 0.8, 0.25, 0.3, 0.9])
    t64 = dense_target64(ya, yb, lam.numpy(), eps, C)
    loss64, want = _dense_head(x, w, b, t64, torch.float64, "cpu", up)
    loss32, ref32 = _dense_head(x, w, b, t64, torch.float32, "cuda", up)
    t = [v.cuda().requires_grad_(True) for v in (x, w, b)]
    loss, out3, logits = SoftProbeHeadFn.apply(t[0], t[1], t[2], ya.cuda(), yb.cuda(), lam.cuda(), eps)
    assert not out3.requires_grad and not logits.requires_grad
    (loss * up).backward()
    lg64 = F.linear(x.double(), w.double(), b.double())
    dev_logit = float((F.linear(x.cuda(), w.cuda(), b.cuda()).cpu().double() - lg64).abs().max())
    gate_loss = 4 * (abs(loss32 - loss64) + dev_logit)                    # (the loss is 2-Lipschitz in the logits: test_gpu_linear_probe.py)
    print(f"C={C} loss: {abs(loss.item() - loss64):.3e} (gate {gate_loss:.3e})")
    assert abs(loss.item() - loss64) <= gate_loss
    assert out3[1].item() == int((ranks64(lg64, ya) < 1).sum())
    for name, v, w64, r32 in zip(("dx", "dW", "db"), t, want, ref32):
        got, gate = rel_dev(v.grad.cpu().numpy(), w64), 4 * rel_dev(r32, w64)
        print(f"C={C} {name}: {got:.3e} (gate {gate:.3e})")
        assert got <= gate, name


def test_registered_losses_on_the_device(soft_cases):
    """LabelSmoothingCrossEntropy and the two-label form of SoftTargetCrossEntropy: one autograd node each over the fused rows, mean and
    reduction='none', against float64 at the pooled gates of test_soft_ce_rows."""
    from simseg.models.criteria.losses import LOSS
    cases, tol = soft_cases
    c = cases[(16, 1000, torch.float32, 0.1)]
    ok = c["ok"]
    B, C = c["x"].shape
    a, b = torch.where(ok.cuda(), c["a"], torch.zeros_like(c["a"])), torch.where(ok.cuda(), c["b"], torch.zeros_like(c["b"]))
    x64 = c["x"].double().cpu()
    up = torch.linspace(0.5, 1.5, B)
    for name, target, t64 in (("LabelSmoothingCrossEntropy", a, dense_target64(a.cpu(), a.cpu(), np.ones(B), 0.1, C)),
                              ("SoftTargetCrossEntropy", {"label": a, "label_b": b, "lam": c["lam"], "smoothing": 0.1},
                               dense_target64(a.cpu(), b.cpu(), c["lam"].cpu().numpy(), 0.1, C))):
        rows64, grad64 = soft_ce64(x64, t64)
        kw = dict(smoothing=0.1) if name.startswith("Label") else {}
        x = c["x"].clone().requires_grad_(True)
        mean = LOSS.get(name)(None, 0, **kw)(x, target)
        assert mean.shape == () and mean.grad_fn is not None and mean.grad_fn.next_functions[0][0].variable is x      # ONE node
        (mean * 0.37).backward()
        assert abs(mean.item() - rows64.mean().item()) <= tol["loss"] * max(1.0, abs(rows64.mean().item()))
        assert (x.grad.cpu().double() - 0.37 * grad64).abs().max().item() <= tol["grad"]
        x = c["x"].clone().requires_grad_(True)
        rows = LOSS.get(name)(None, 0, reduction="none", **kw)(x, target)
        assert rows.shape == (B,)
        assert ((rows.detach().cpu().double() - rows64).abs() / rows64.abs().clamp(min=1.0)).max().item() <= tol["loss"]
        (rows * up.cuda()).sum().backward()
        assert (x.grad.cpu().double() - grad64 * B * up[:, None].double()).abs().max().item() <= tol["grad"] * B * 1.5
    dense = LOSS.get("SoftTargetCrossEntropy")(None, 0)(c["x"], t64.float().cuda())                  # the unfused form, on the device
    assert abs(dense.item() - rows64.mean().item()) <= tol["loss"] * max(1.0, abs(rows64.mean().item()))


# ---- model ----------------------------------------------------------------------------------------------------------------------------
def _mixed_batch(B, seed, eps=0.1):
    from simseg_amd.mixup import Mixup
    batch = _batch(B, seed)
    mix = Mixup(0.8, 1.0, mode="elem", label_smoothing=eps, num_classes=10)
    image, tgt = mix(batch["image"], batch["label"], np.random.default_rng(seed))
    return {"image": image, **tgt}


def test_mixed_batch_through_the_model_against_a_torch_dense_head():
    model, cfg = _build()
    batch = _mixed_batch(8, 4)
    assert set(batch) == {"image", "label", "label_b", "lam", "smoothing"}
    w0, b0 = model.classifier.weight.detach().clone(), model.classifier.bias.detach().clone()
    x = model.forward_image_feature(batch["image"]).float()
    t64 = dense_target64(batch["label"].cpu(), batch["label_b"].cpu(), batch["lam"].cpu().numpy(), 0.1, 10)
    loss64, (_, dw64, db64) = _dense_head(x, w0, b0, t64, torch.float64, "cpu", 1.0)
    loss32, (_, dw32, db32) = _dense_head(x, w0, b0, t64, torch.float32, "cuda", 1.0)
    lg64 = F.linear(x.double().cpu(), w0.double().cpu(), b0.double().cpu())
    dev_logit = float((F.linear(x, w0, b0).cpu().double() - lg64).abs().max())
    loss_dict, acc1, acc5 = model(batch)
    loss = sum(loss_dict.values())
    loss.backward()
    torch.cuda.synchronize()
    got = dict(loss=abs(loss.item() - loss64), w=rel_dev(model.classifier.weight.grad.cpu().numpy(), dw64),
               b=rel_dev(model.classifier.bias.grad.cpu().numpy(), db64))
    gates = dict(loss=4 * (abs(loss32 - loss64) + dev_logit), w=4 * rel_dev(dw32, dw64), b=4 * rel_dev(db32, db64))
    print("mixed batch vs the float64 dense-target head:", {k: f"{v:.3e}" for k, v in got.items()}, "gates", {k: f"{v:.3e}" for k, v in gates.items()})
    assert all(got[k] <= gates[k] for k in got)
    r = ranks64(lg64, batch["label"].cpu())                               # accuracy against the samples' own labels
    assert acc1.shape == (1,) and acc1.item() == 100.0 * int((r < 1).sum()) / 8 and acc5.item() == 100.0 * int((r < 5).sum()) / 8


def test_train_step_with_a_mixed_batch_and_the_hard_path_unchanged():
    from simseg_amd.probe import LinearProbeTrainer, ProbeHeadFn
    model, cfg = _build()
    # a batch WITHOUT the keys: bit-identical to ProbeHeadFn called directly
    plain = _batch(8, 2)
    feats = model.forward_image_feature(plain["image"])
    want = ProbeHeadFn.apply(feats, model.classifier.weight, model.classifier.bias, plain["label"])
    loss_dict, acc1, acc5 = model(plain)
    _, pred, _ = model(plain, valid=True)
    assert torch.equal(_bits(sum(loss_dict.values()).detach()), _bits(want[0].detach())) and torch.equal(pred, want[2])
    assert torch.equal(acc1, want[1][1:2] * (100.0 / 8)) and torch.equal(acc5, want[1][2:3] * (100.0 / 8))
    tot = model.eval_counts(plain)
    assert tot[1].item() == want[1][1].item() and tot[2].item() == want[1][2].item()
    trainer = LinearProbeTrainer(model, cfg, steps_per_epoch=10)
    w0 = model.classifier.weight.detach().clone()
    out = trainer.train_step(_mixed_batch(8, 5))
    torch.cuda.synchronize()
    assert all(torch.isfinite(out[k]).all() for k in ("loss", "acc1", "acc5")) and out["loss"].item() > 0
    assert trainer.step == 1 and not torch.equal(model.classifier.weight, w0)
