"""The SigLIP pairwise sigmoid loss on MI355X: ops.siglip_rows, the autograd node heads.SigLipFn, and LOSS.SigLip driven through CLIPModel
and Trainer.

Toleranced checks follow the yardstick rule of tests/test_gpu_loss_head.py, unchanged (its _check): the kernel's error against the float64
statement of tests/_siglip_ref.py is at most 8 x the error of the same formula in fp32 torch on the device + 4 fp32 ulps of the largest
reference magnitude.  Every such check prints one `loss-head |` line; profiles/siglip_loss_tests.txt is that table.  What the header states
exactly is compared exactly: the accuracy, dLoss/dT = 0 outside the clamp, write_grad = 0, run-to-run bits, exact zeros at saturation.
Every case first ASSERTS the top-1 margin on s in float64 (tests/test_siglip_host.py asserts it on the CPU too); none is skipped."""
import os

import numpy as np
import pytest
import torch

import _contrastive_ref as R
import _siglip_ref as S
from conftest import REPO, tt
from test_gpu_loss_head import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _dev(v):
    return torch.tensor([v], dtype=torch.float32).cuda()


def _blocks(family, N1, N2, target0):
    s2 = S.blocks(family, N1, N2, target0)
    for k in range(2):
        assert R.margin_ok(s2[k].double()), f"{family} {N1}x{N2}+{target0} block {k}: top-1 margin on s - pick another seed"
    return s2


def _rows_case(ops, case, s, T, b, target0):
    N1, N2 = s.shape
    ref = S.siglip_eval(s, T, b, target0)
    yard = S.siglip_eval(s, T, b, target0, dtype=torch.float32, device="cuda")
    sims = s.cuda().clone()
    out4, rows = ops.siglip_rows(sims, _dev(T), _dev(b), target0)
    assert out4.shape == (4,) and rows.shape == (N1,)
    _check(case, "rows", rows, ref["rows"], yard["rows"])
    _check(case, "total", out4[0], ref["total"], yard["total"])
    _check(case, "dsims", sims, ref["ds"], yard["ds"])
    _check(case, "dT", out4[2], ref["dt"], yard["dt"])
    _check(case, "db", out4[3], ref["db"], yard["db"])
    assert out4[1].item() == ref["acc"], f"{case}: top-1 accuracy {out4[1].item()} vs {ref['acc']}"
    if not (S.T_LO <= float(np.float32(T)) <= S.T_HI):
        assert out4[2].item() == 0.0, f"{case}: dLoss/dT outside the clamp must be exactly 0"
    assert out4[3].item() != 0.0, f"{case}: dLoss/db"
    return out4, rows, sims


@pytest.mark.parametrize("T,b", S.SETTINGS)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", S.ROW_SHAPES)
def test_siglip_rows_vs_float64(ops, N1, N2, target0, family, T, b):
    s2 = _blocks(family, N1, N2, target0)
    for k in range(2):
        _rows_case(ops, f"siglip {family} {N1}x{N2}+{target0} T={T:g} b={b:g} b{k}", s2[k], T, b, target0)


@pytest.mark.parametrize("T,b", [(0.1, -10.0), (0.7, -3.0)])
@pytest.mark.parametrize("N1,N2,target0", S.ROW_SHAPES)
def test_siglip_rows_without_the_gradient_and_twice(ops, N1, N2, target0, T, b):
    s = _blocks("aligned", N1, N2, target0)[0]
    sims = s.cuda().clone()
    out4, rows = ops.siglip_rows(sims, _dev(T), _dev(b), target0)
    # write_grad = False: the similarities survive bit for bit, loss, accuracy and row losses are the same bits
    kept = s.cuda().clone()
    o2, r2 = ops.siglip_rows(kept, _dev(T), _dev(b), target0, write_grad=False)
    assert torch.equal(kept.cpu().view(torch.int32), s.view(torch.int32)), "write_grad=False touched the similarities"
    assert torch.equal(o2[:2].view(torch.int32), out4[:2].view(torch.int32)) and torch.equal(r2.view(torch.int32), rows.view(torch.int32))
    # no atomics: a second run on the same input gives the same bits
    again = s.cuda().clone()
    o3, r3 = ops.siglip_rows(again, _dev(T), _dev(b), target0)
    assert torch.equal(o3.view(torch.int32), out4.view(torch.int32)) and torch.equal(r3.view(torch.int32), rows.view(torch.int32))
    assert torch.equal(again.view(torch.int32), sims.view(torch.int32))


def test_siglip_rows_saturation(ops):
    """|z| ~ 1000: exp(-|x|) underflows to 0, the pair loss is max(x, 0) and the sigmoid 0 or 1 - finite everywhere, and the gradient is
    exactly 0 wherever the float64 statement rounds to 0 in fp32."""
    N1, N2, target0, T, b = 3, 64, 10, 1e-3, 0.0
    g = torch.Generator().manual_seed(11)
    s = (torch.randint(0, 2, (N1, N2), generator=g).float() * 2 - 1)
    s[0, target0], s[1, target0 + 1], s[2, target0 + 2] = 1.0, -1.0, 1.0          # a satisfied positive, a violated one, a satisfied one
    s[:2, :target0] = -1.0         # (row 0's first +1 is its target: a hit; row 1's target holds -1: a miss)
    ref = S.siglip_eval(s, T, b, target0)
    yard = S.siglip_eval(s, T, b, target0, dtype=torch.float32, device="cuda")
    sims = s.cuda().clone()
    out4, rows = ops.siglip_rows(sims, _dev(T), _dev(b), target0)
    assert bool(torch.isfinite(out4).all()) and bool(torch.isfinite(rows).all()) and bool(torch.isfinite(sims).all())
    assert 0.0 < ref["acc"] < 1.0 and out4[1].item() == ref["acc"]          # (exact ties on exact inputs: the first index wins on both sides)
    case = "siglip saturation 3x64+10 T=0.001 b=0"
    _check(case, "rows", rows, ref["rows"], yard["rows"])
    _check(case, "total", out4[0], ref["total"], yard["total"])
    _check(case, "dsims", sims, ref["ds"], yard["ds"])
    _check(case, "dT", out4[2], ref["dt"], yard["dt"])
    _check(case, "db", out4[3], ref["db"], yard["db"])
    zero = ref["ds"].float() == 0
    assert bool(zero.any()) and bool((~zero).any())
    assert not sims.cpu()[zero].any(), "dS must be exactly 0 where the float64 gradient rounds to 0 in fp32"
    assert bool((sims.cpu()[~zero] != 0).all())
    assert ref["total"].item() > 1000.0 and out4[2].item() != 0.0          # T = 0.001f is inside the clamp


@pytest.mark.parametrize("what", ["targets_outside", "negative_target0", "bf16_sims", "two_element_bias", "columns_past_int32"])
def test_siglip_rows_refusals_launch_nothing(ops, what):
    s = torch.randn(4, 9, generator=torch.Generator().manual_seed(5)).cuda()
    before = s.clone()
    t, b = _dev(0.1), _dev(-10.0)
    if what == "targets_outside":
        with pytest.raises(RuntimeError, match="siglip_rows: targets"):
            ops.siglip_rows(s, t, b, 6)
    elif what == "negative_target0":
        with pytest.raises(RuntimeError, match="siglip_rows: targets"):
            ops.siglip_rows(s, t, b, -1)
    elif what == "bf16_sims":
        h = s.bfloat16()
        hb = h.clone()
        with pytest.raises(TypeError, match="siglip_rows: sims must be fp32"):
            ops.siglip_rows(h, t, b, 0)
        torch.cuda.synchronize()
        assert torch.equal(h, hb)
    elif what == "two_element_bias":
        with pytest.raises(ValueError, match="siglip_rows: bias holds one element"):
            ops.siglip_rows(s, t, torch.tensor([-10.0, -10.0]).cuda(), 0)
    else:
        # the C entry itself, with a column count the kernel's 32-bit indices cannot hold (refused before any launch: nothing is read)
        from simseg_amd.lib import call, ptr, stream
        scratch, out4 = torch.zeros(4, 4).cuda(), torch.zeros(4).cuda()
        with pytest.raises(RuntimeError, match="siglip_rows: N2 = 2147483648 columns"):
            call("simseg_siglip_rows", ptr(s), ptr(t), ptr(b), ptr(scratch[0]), ptr(scratch[1]), ptr(scratch[2]), ptr(scratch[3]), ptr(out4),
                 4, 2 ** 31, 0, 1, stream())
    torch.cuda.synchronize()
    assert torch.equal(s, before)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the autograd node against float64 autograd of the torch statement
# ------------------------------------------------------------------------------------------------------------------------------------------
UP = 3.0          # the upstream gradient


def _head_eval(a32, g32, T, b, rank, dtype, device):
    a = a32.to(device=device, dtype=dtype).requires_grad_(True)
    g = g32.to(device=device, dtype=dtype).requires_grad_(True)
    t = torch.tensor(T, dtype=torch.float32).to(device=device, dtype=dtype).requires_grad_(True)
    bias = torch.tensor(b, dtype=torch.float32).to(device=device, dtype=dtype).requires_grad_(True)
    s = a @ g.T
    loss = S.siglip_torch(s, t, bias, rank * a.shape[0])
    (UP * loss).backward()
    return {"loss": loss.detach(), "da": a.grad, "dg": g.grad, "dt": t.grad, "db": bias.grad, "s": s.detach()}


@pytest.mark.parametrize("T,b", [(0.1, -10.0), (0.02, -10.0)])
@pytest.mark.parametrize("N1,P", R.HEAD_SHAPES)
def test_siglip_fn_vs_float64(ops, N1, P, T, b):
    """rank 1 of 3 with a hand-built gathered matrix; gradients w.r.t. both embeddings (the gathered rows of other ranks included), the
    temperature and the bias."""
    from simseg_amd import heads
    img, _, gathered = R.head_embeddings(N1, P, R.HEAD_SEEDS[N1, P])
    ref = _head_eval(img, gathered, T, b, 1, torch.float64, "cpu")
    yard = _head_eval(img, gathered, T, b, 1, torch.float32, "cuda")
    assert R.margin_ok(ref["s"]), f"head N1={N1} P={P}: pick another seed"
    a, g = img.cuda().requires_grad_(True), gathered.cuda().requires_grad_(True)
    t = torch.tensor(T).cuda().requires_grad_(True)
    bias = torch.tensor(b).cuda().requires_grad_(True)
    loss, acc = heads.SigLipFn.apply(a, g, t, bias, 1)
    assert not acc.requires_grad
    (loss * UP).backward()
    case = f"SigLipFn N1={N1} P={P} T={T:g} b={b:g} rank 1/3"
    _check(case, "loss", loss, ref["loss"], yard["loss"])
    _check(case, "dfeat1", a.grad, ref["da"], yard["da"])
    _check(case, "dfeat2", g.grad, ref["dg"], yard["dg"])
    _check(case, "dT", t.grad, ref["dt"], yard["dt"])
    _check(case, "db", bias.grad, ref["db"], yard["db"])
    assert acc.item() == R.acc32(ref["s"], N1)
    assert t.grad.shape == () and bias.grad.shape == ()


def test_siglip_fn_returns_none_for_inputs_that_need_no_gradient(ops):
    from simseg_amd import heads
    img, _, gathered = R.head_embeddings(5, 64, R.HEAD_SEEDS[5, 64])
    a = img.cuda().requires_grad_(True)
    g, t, bias = gathered.cuda(), torch.tensor(0.1).cuda(), torch.tensor(-10.0).cuda()
    loss, _ = heads.SigLipFn.apply(a, g, t, bias, 1)
    loss.backward()
    assert a.grad is not None and g.grad is None and t.grad is None and bias.grad is None
    with torch.no_grad():
        l2, _ = heads.SigLipFn.apply(a, g, t, bias, 1)
    assert torch.equal(l2, loss.detach())          # (the forward without the gradient pass computes the same bits)


# ------------------------------------------------------------------------------------------------------------------------------------------
# end to end through CLIPModel and Trainer  (_model / _batch as in tests/test_gpu_contrastive_losses.py)
# ------------------------------------------------------------------------------------------------------------------------------------------
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False", "epoch=1", "optim.lr.init=1e-3",
        "optim.lr.warmup_proportion=0.0"]          # (no warm-up: the schedule's first step would otherwise run at lr = 0)


def _model(golden, extra):
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), TINY + list(extra), update_clip_config)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    g = golden("clip_glue")
    model.load_state_dict({k[3:]: tt(g[k]) for k in g.files if k.startswith("sd.")}, strict=False)
    return model.cuda().eval()                      # (eval: no dropout, so that two runs see the same numbers)


def _batch(golden):
    g = golden("clip_train_ws1")
    return {"image": tt(g["r0.image"]).cuda(), "input_ids": tt(g["r0.input_ids"]).cuda(), "attention_mask": tt(g["r0.attention_mask"]).cuda()}


def _nce_bits(golden, batch):
    n = _model(golden, ["loss.name=NCE"])
    assert "loss.bias" not in n.state_dict()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        d, a1, a2 = n(batch)
    assert list(d) == ["nce_loss"]
    return d["nce_loss"].clone(), a1.clone(), a2.clone()


@pytest.mark.parametrize("tname", ["parameter", "constant"])
def test_model_with_the_siglip_loss(golden, tname):
    from simseg_amd import trainer as T
    batch = _batch(golden)
    nce_before = _nce_bits(golden, batch)
    extra = ["loss.name=SigLip", f"loss.temperature.name={tname}", "loss.temperature.value=0.1"]
    m = _model(golden, extra)
    # (the golden state dict holds NCE's temperature parameter, 0.02: under `parameter` it is loaded over the configured 0.1)
    t0 = m.loss.temperature.item()
    assert m.loss.bias.item() == -10.0 and t0 == pytest.approx(0.02 if tname == "parameter" else 0.1)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_dict, a1, a2 = m(batch)
        assert list(loss_dict) == ["siglip_loss"] and np.isfinite(loss_dict["siglip_loss"].item())
        with torch.no_grad():
            img, txt = m(batch, embeddings="all")
            l1, w1 = m.loss(img, txt)
            l2, w2 = m.loss(txt, img)
    assert loss_dict["siglip_loss"].item() == (0.5 * (l1 + l2)).item() and a1.item() == w1.item() and a2.item() == w2.item()
    assert loss_dict["siglip_loss"].item() > 0
    names = [k for k, _ in m.named_parameters()]
    assert ("loss.bias" in names) == ("loss.temperature" in names) == (tname == "parameter")
    tr = T.Trainer(m, m.cfg, steps_per_epoch=40)
    trained = {id(p) for g in tr.optimizer.param_groups for p in g["params"]}
    assert (id(m.loss.bias) in trained) == (tname == "parameter")
    out = tr.train_step(batch)
    assert np.isfinite(float(out["loss"])) and tr.optimizer.steps_taken() == 1 and out["lr"] > 0
    if tname == "parameter":
        assert m.loss.bias.grad is not None and m.loss.bias.grad.item() != 0.0 and m.loss.temperature.grad.item() != 0.0
        assert m.loss.bias.item() != -10.0 and m.loss.temperature.item() != t0
    else:
        assert m.loss.bias.item() == -10.0 and m.loss.temperature.item() == t0
    # a state-dict round trip restores the bias (a parameter, or the persistent buffer)
    with torch.no_grad():
        m.loss.bias.fill_(-7.25)
    sd = tr.checkpoint()["state_dict"]
    assert "loss.bias" in sd and ("loss.temperature" in sd) == (tname == "parameter")
    fresh = _model(golden, extra)
    assert fresh.loss.bias.item() == -10.0
    fresh.load_state_dict(sd)
    assert fresh.loss.bias.item() == -7.25 and fresh.loss.bias.is_cuda
    # nothing leaked into the default path: a model built with loss.name=NCE gives the bits it gave before
    nce_after = _nce_bits(golden, batch)
    assert all(torch.equal(x, y) for x, y in zip(nce_before, nce_after))
