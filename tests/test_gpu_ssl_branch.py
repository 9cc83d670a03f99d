"""The image self-supervision branch (SLIP: the image-text loss plus NT-Xent on two views through the same image tower) on MI355X: the
projection-head node towers.MlpHeadFn against float64, the default path's bits with the branch in the process, the loss dict of
CLIPModel.enable_ssl recomputed from the same single concatenated tower call, one Trainer(ssl=...) step, and the step under patch dropout.

The tiny model and batch are those of tests/test_gpu_siglip.py (clip_glue weights, the clip_train_ws1 batch); image_ssl is two fixed
perturbations of the batch's images.  Toleranced checks are _check of tests/test_gpu_loss_head.py, unchanged: in fp32 the yardstick is
the same formula in fp32 torch on the device, under bf16 the same torch formula under bf16 autocast on the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_loss_head import _check
from test_gpu_siglip import _batch, _model

pytestmark = pytest.mark.gpu

D, HID, OUT = 128, 192, 64


def _views(image):
    """Two fixed perturbations of the batch's images (what two draws of the view pipeline would hand over): a flip with a gain, and an
    offset with noise."""
    g = torch.Generator().manual_seed(7)
    noise = torch.randn(image.shape, generator=g).to(image.device)
    return torch.stack([image.flip(-1) * 0.9, image + 0.1 + 0.05 * noise])


# ------------------------------------------------------------------------------------------------------------------------------------------
# the head node alone
# ------------------------------------------------------------------------------------------------------------------------------------------
def _head_inputs(rows):
    g = torch.Generator().manual_seed(100 + rows)
    x = torch.randn(rows, D, generator=g)
    w1, b1 = torch.randn(HID, D, generator=g) * 0.1, torch.randn(HID, generator=g) * 0.1
    w2 = torch.randn(OUT, HID, generator=g) * 0.1
    dy = torch.randn(rows, OUT, generator=g)
    return x, w1, b1, w2, dy


def _head_torch(ts, dtype, device, autocast=None):
    x, w1, b1, w2 = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in ts[:4]]
    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
        y = F.linear(F.gelu(F.linear(x, w1, b1)), w2)
    y.backward(ts[4].to(device=device, dtype=y.dtype))
    return {"y": y.detach(), "dx": x.grad, "dw1": w1.grad, "db1": b1.grad, "dw2": w2.grad}


@pytest.mark.parametrize("adt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [6, 70])
def test_mlp_head_node_vs_float64(rows, adt):
    from simseg_amd.towers import MlpHeadFn
    assert torch.cuda.is_available()
    ts = _head_inputs(rows)
    ref = _head_torch(ts, torch.float64, "cpu")
    yard = _head_torch(ts, torch.float32, "cuda", autocast=None if adt == torch.float32 else adt)
    x, w1, b1, w2 = [t.cuda().requires_grad_(True) for t in ts[:4]]
    y = MlpHeadFn.apply(x, w1, b1, w2, adt)
    assert y.dtype == torch.float32 and tuple(y.shape) == (rows, OUT)
    y.backward(ts[4].cuda())
    case = f"MlpHeadFn {rows}x{D}->{HID}->{OUT} {'fp32' if adt == torch.float32 else 'bf16'}"
    _check(case, "y", y, ref["y"], yard["y"])
    _check(case, "dx", x.grad, ref["dx"], yard["dx"])
    _check(case, "dw1", w1.grad, ref["dw1"], yard["dw1"])
    _check(case, "db1", b1.grad, ref["db1"], yard["db1"])
    _check(case, "dw2", w2.grad, ref["dw2"], yard["dw2"])
    with torch.no_grad():          # evaluation saves nothing and computes the same output
        y2 = MlpHeadFn.apply(x, w1, b1, w2, adt)
    _check(case, "y eval", y2, ref["y"], yard["y"])


# ------------------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------------------
def _ssl_model(golden, scale=1.0, extra=()):
    torch.manual_seed(3)          # (the projection head's initialisation)
    m = _model(golden, ["loss.name=NCE"] + list(extra))
    return m.enable_ssl(scale=scale, hidden_dim=HID, out_dim=OUT, temperature=0.1)


def _nce_bits(golden, batch):
    n = _model(golden, ["loss.name=NCE"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        d, a1, a2 = n(batch)
    assert list(d) == ["nce_loss"]
    return d["nce_loss"].clone(), a1.clone(), a2.clone()


def test_default_path_is_unchanged(golden):
    from simseg_amd import trainer as T
    batch = _batch(golden)
    with_key = dict(batch, image_ssl=_views(batch["image"]))
    before = _nce_bits(golden, batch)
    ignored = _nce_bits(golden, with_key)          # the key is ignored when the branch is off
    assert all(torch.equal(x, y) for x, y in zip(before, ignored))
    m = _ssl_model(golden)
    tr = T.Trainer(m, m.cfg, steps_per_epoch=40)
    tr.train_step(with_key)
    after = _nce_bits(golden, batch)               # an SSL model was built and stepped in the process
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_branch_on_loss_dict_and_one_tower_call(golden):
    batch = _batch(golden)
    views = _views(batch["image"])
    with_key = dict(batch, image_ssl=views)
    B = batch["image"].shape[0]
    m = _ssl_model(golden)
    calls = []
    hook = m.image_encoder.register_forward_hook(lambda mod, args, out: calls.append(args[0].shape[0]))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_dict, a1, a2 = m(with_key)
        assert calls == [3 * B], f"the image tower ran {len(calls)} times on {calls} images"
        assert list(loss_dict) == ["nce_loss", "ssl_loss"] and all(np.isfinite(v.item()) for v in loss_dict.values())
        assert loss_dict["ssl_loss"].requires_grad and 0.0 <= m.ssl_acc.item() <= 1.0
        with torch.no_grad():
            # recomputed through the same single concatenated tower call
            img, z1, z2 = m.forward_image_ssl(batch["image"], views)
            assert tuple(img.shape)[0] == B and tuple(z1.shape) == (B, OUT) and tuple(z2.shape) == (B, OUT)
            ssl, acc = m.ssl_loss(z1, z2)
            _, txt = m(batch, embeddings="all")
            nce, w1, w2 = m.forward_loss(img, txt)
            # a pair of tensors is the same key as the stacked tensor
            pair_dict, _, _ = m(dict(batch, image_ssl=(views[0], views[1])))
            # the branch is skipped: without the key, and for embeddings != False
            calls.clear()
            plain, _, _ = m(batch)
            both = m(with_key, embeddings="all")
            assert calls == [B, B] and list(plain) == ["nce_loss"] and len(both) == 2 and tuple(both[0].shape)[0] == B
    hook.remove()
    assert loss_dict["ssl_loss"].item() == ssl.item() and m.ssl_acc.item() == acc.item()
    assert loss_dict["nce_loss"].item() == nce["nce_loss"].item() and a1.item() == w1.item() and a2.item() == w2.item()
    assert pair_dict["ssl_loss"].item() == ssl.item() and pair_dict["nce_loss"].item() == nce["nce_loss"].item()
    assert ssl.item() > 0
    # scale = 0.5 halves ssl_loss exactly (same initialisation: the seed in _ssl_model)
    h = _ssl_model(golden, scale=0.5)
    assert torch.equal(h.ssl_projection.fc1.weight, m.ssl_projection.fc1.weight)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        half, _, _ = h(with_key)
    assert half["ssl_loss"].item() == 0.5 * ssl.item() and half["nce_loss"].item() == nce["nce_loss"].item()
    with pytest.raises(ValueError, match="image_ssl: two views"):
        m(dict(batch, image_ssl=views[:, :2]))


def _grads(m):
    return {k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_one_trainer_step_with_the_branch(golden):
    from simseg_amd import trainer as T
    batch = _batch(golden)
    with_key = dict(batch, image_ssl=_views(batch["image"]))
    off = _model(golden, ["loss.name=NCE"])
    tr_off = T.Trainer(off, off.cfg, steps_per_epoch=40)
    out_off = tr_off.train_step(batch)
    assert "ssl_loss" not in out_off and "ssl_acc" not in out_off
    g_off = _grads(off)
    torch.manual_seed(3)
    m = _model(golden, ["loss.name=NCE"])
    tr = T.Trainer(m, m.cfg, steps_per_epoch=40, ssl=dict(scale=1.0, hidden_dim=HID, out_dim=OUT, temperature=0.1))
    names = ["ssl_projection.fc1.weight", "ssl_projection.fc1.bias", "ssl_projection.fc2.weight"]
    params = dict(m.named_parameters())
    trained = {id(p) for g in tr.optimizer.param_groups for p in g["params"]}
    assert all(id(params[k]) in trained for k in names) and not list(m.ssl_loss.parameters())
    w0 = {k: params[k].detach().clone() for k in names}
    out = tr.train_step(with_key)
    assert tr.optimizer.steps_taken() == 1 and out["lr"] > 0
    assert np.isfinite(float(out["loss"])) and np.isfinite(float(out["ssl_loss"])) and 0.0 <= float(out["ssl_acc"]) <= 1.0
    assert float(out["ssl_loss"]) > 0 and float(out["loss"]) > float(out["ssl_loss"])
    g = _grads(m)
    for k in names:
        assert k in g and bool(torch.isfinite(g[k]).all()) and bool(g[k].any()), k
        assert not torch.equal(params[k].detach(), w0[k]), f"{k} did not move"
    tower = [k for k, p in m.named_parameters() if k.startswith("image_encoder.") and p.requires_grad]
    assert tower and all(k in g and bool(torch.isfinite(g[k]).all()) for k in tower)
    pe = "image_encoder.model.model.patch_embed.proj.weight"
    assert not torch.equal(g[pe], g_off[pe]), "the branch's gradient did not reach the patch embedding"
    # a checkpoint round trip restores the projection head
    sd = tr.checkpoint()["state_dict"]
    assert all(k in sd for k in names)
    fresh = _model(golden, ["loss.name=NCE"]).enable_ssl(hidden_dim=HID, out_dim=OUT)
    assert not torch.equal(fresh.ssl_projection.fc2.weight, m.ssl_projection.fc2.weight)
    fresh.load_state_dict(sd)
    assert all(torch.equal(dict(fresh.named_parameters())[k], params[k]) for k in names) and fresh.ssl_projection.fc1.weight.is_cuda


def test_step_under_patch_dropout_uses_the_cls_rows(golden):
    from simseg_amd import trainer as T
    batch = _batch(golden)
    views = _views(batch["image"])
    B = batch["image"].shape[0]
    m = _model(golden, ["loss.name=NCE"])
    tr = T.Trainer(m, m.cfg, steps_per_epoch=40, patch_drop_rate=0.5, ssl=dict(hidden_dim=HID, out_dim=OUT))
    m.train()
    seen = {}
    h1 = m.image_encoder.register_forward_hook(lambda mod, args, out: seen.update(feats=out.detach().clone(), n=args[0].shape[0]))
    h2 = m.ssl_projection.register_forward_hook(lambda mod, args, out: seen.update(cls=args[0].detach().clone()))
    out = tr.train_step(dict(batch, image_ssl=views))
    h1.remove(); h2.remove()
    N = (batch["image"].shape[-1] // 16) ** 2
    assert seen["n"] == 3 * B and seen["feats"].shape[1] == 1 + N // 2          # every one of the 3B images lost half its patches, none its [cls]
    assert torch.equal(seen["cls"], seen["feats"][B:, 0])
    assert tr.optimizer.steps_taken() == 1 and np.isfinite(float(out["loss"])) and np.isfinite(float(out["ssl_loss"]))
