"""Patch dropout on the MI355X: the device sampler against its numpy statement, the gather against the full im2col, the new embedding node
forward and backward against float64 torch, the whole tower against the project's own composition (full embedding -> gather -> the same
blocks), and the switches on the model and the trainer.

Bounds: fp32 forward 1e-5 * max|ref| (the patch-embed test of tests/test_gpu_kernels.py), fp32 gradients 2e-4 * max|ref| and 16-bit
gradients cosine > 0.99 with a norm ratio in (0.9, 1.1) (tests/test_gpu_model.py); everything that is a selection or an ordered fp32 sum
is compared for equality."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, tt

pytestmark = pytest.mark.gpu

TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False"]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _rand(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _keep(B, N, K, seed):
    from simseg_amd.patchdrop import sample_keep_ref
    keep, inv = sample_keep_ref(B, N, K, seed)
    return tt(keep).cuda(), tt(inv).cuda()


def _rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-300))


def _cos_ratio(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300)), float(a.norm() / (b.norm() + 1e-300))


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, (1 << 40) + 17], ids=["small_seed", "seed_above_2^32"])
@pytest.mark.parametrize("B,N,K", [(1, 1, 1), (3, 36, 9), (5, 196, 98), (2, 196, 196), (4, 1024, 256), (2, 1024, 1), (300, 36, 35), (2, 4096, 2048)])
def test_sampler_equals_its_numpy_statement(B, N, K, seed):
    from simseg_amd.patchdrop import sample_keep, sample_keep_ref
    keep, inv = sample_keep(B, N, K, seed, "cuda")
    want_keep, want_inv = sample_keep_ref(B, N, K, seed)
    assert keep.dtype == torch.int32 and inv.dtype == torch.int32 and keep.is_cuda and inv.is_cuda
    assert torch.equal(keep.cpu(), tt(want_keep)) and torch.equal(inv.cpu(), tt(want_inv))


# ---- the gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,K", [(96, 96, 3, 9), (32, 64, 2, 3)], ids=["96x96", "32x64"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_im2col_keep_selects_rows_of_the_full_im2col(dtype, H, W, B, K):
    """(the non-square image: a swapped patch row / column, or a grid width taken from H, reads other pixels)"""
    from simseg_amd import ops
    N = (H // 16) * (W // 16)
    image = _rand(B, 3, H, W, seed=1)
    keep, _ = _keep(B, N, K, 5)
    full = ops.vit_im2col(image, DTYPES[dtype]).view(B, N, 768)
    want = torch.gather(full, 1, keep.long()[:, :, None].expand(-1, -1, 768)).reshape(B * K, 768)
    got = ops.vit_im2col_keep(image, keep, DTYPES[dtype])
    assert got.dtype == DTYPES[dtype] and got.shape == (B * K, 768)
    assert torch.equal(got, want)
    bad = keep.clone()
    bad[0, 0], bad[-1, -1] = -1, N                       # an entry outside [0, N): a zero row, nothing read
    got = ops.vit_im2col_keep(image, bad, DTYPES[dtype])
    assert (got[0] == 0).all() and (got[-1] == 0).all() and torch.equal(got[1:-1], want[1:-1])


# ---- the embedding node ---------------------------------------------------------------------------------------------------------------
def _embed_params(D, N, seed=0):
    w, bias = _rand(D, 3, 16, 16, seed=seed + 2, scale=0.05), _rand(D, seed=seed + 3)
    cls, pos = _rand(1, 1, D, seed=seed + 4), _rand(1, 1 + N, D, seed=seed + 5)
    return w, bias, cls, pos


def _embed_ref64(image, w, bias, cls, pos, keep):
    """conv patch embed, cat cls, add pos, gather - in float64 on the host."""
    B = image.shape[0]
    x = F.conv2d(image, w, bias, stride=16).flatten(2).transpose(1, 2)
    x = torch.cat([cls.expand(B, -1, -1), x], 1) + pos
    idx = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + keep.long().cpu()], 1)
    return torch.gather(x, 1, idx[:, :, None].expand(-1, -1, x.shape[-1]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_embed_with_every_patch_kept_equals_the_full_embedding(dtype):
    """keep = arange(N): GEMM with bias and row_group, then + pos in vit_keep_rows, gives the bits of the full path's epilogue
    (+ bias, + residual): the same two fp32 additions in the same order."""
    from simseg_amd import towers as T
    B, D, S = 3, 128, 96
    N = (S // 16) ** 2
    image = _rand(B, 3, S, S, seed=1)
    w, bias, cls, pos = _embed_params(D, N)
    keep = torch.arange(N, dtype=torch.int32, device="cuda").expand(B, N).contiguous()
    with torch.no_grad():
        want = T.ViTEmbedFn.apply(image, w, bias, cls, pos, DTYPES[dtype])
        got = T.ViTEmbedKeepFn.apply(image, w, bias, cls, pos, keep, keep.clone(), DTYPES[dtype])
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,S,K", [(3, 96, 9), (1, 96, 35)])
def test_embed_forward_fp32_vs_float64(B, S, K):
    from simseg_amd import towers as T
    D, N = 128, (S // 16) ** 2
    image = _rand(B, 3, S, S, seed=1)
    w, bias, cls, pos = _embed_params(D, N)
    keep, inv = _keep(B, N, K, 11)
    with torch.no_grad():
        got = T.ViTEmbedKeepFn.apply(image, w, bias, cls, pos, keep, inv, torch.float32)
    want = _embed_ref64(*(t.double().cpu() for t in (image, w, bias, cls, pos)), keep)
    assert got.shape == (B, 1 + K, D)
    err = _rel(got, want)
    print(f"embed forward fp32 B={B} K={K}: {err:.2e} of max|ref|")
    assert err <= 1e-5


# (B, image size, K): two images keeping 3 of 36 (most positions kept by nobody), one image, and more images than the position-gradient
# kernel walks in one chunk (256) - on a 2 x 2 grid so that the case stays small
@pytest.mark.parametrize("B,S,K", [(2, 96, 3), (1, 96, 18), (300, 32, 2)], ids=["B2_K3_N36", "B1", "B300_over_one_chunk"])
def test_embed_backward_fp32_vs_float64_autograd(B, S, K):
    from simseg_amd import towers as T
    D, N = 128, (S // 16) ** 2
    image = _rand(B, 3, S, S, seed=1)
    params = [p.requires_grad_(True) for p in _embed_params(D, N)]
    keep, inv = _keep(B, N, K, 13)
    gy = _rand(B, 1 + K, D, seed=9)
    got = torch.autograd.grad(T.ViTEmbedKeepFn.apply(image, *params, keep, inv, torch.float32), params, gy)
    again = torch.autograd.grad(T.ViTEmbedKeepFn.apply(image, *params, keep, inv, torch.float32), params, gy)
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in params]
    want = torch.autograd.grad(_embed_ref64(image.double().cpu(), *p64, keep), p64, gy.double().cpu())
    for name, g, a, w_ in zip(("dW", "db", "dcls", "dpos"), got, again, want):
        err = _rel(g, w_)
        print(f"embed backward fp32 B={B} K={K} {name}: {err:.2e} of max|ref|")
        assert g.shape == w_.shape and err <= 2e-4, (name, err)
    assert torch.equal(got[3], again[3])                               # ordered sums: the same bits every run (rows 1..N, and row 0)
    dropped = (inv < 0).all(0).cpu()                                   # positions no image kept
    if (B, K) == (2, 3):
        assert int(dropped.sum()) >= N - 6
    assert (got[3][0, 1:][dropped] == 0).all() and (want[3][0, 1:][dropped] == 0).all()
    assert torch.equal(got[2].view(-1), got[3][0, 0])                  # the [cls] gradient is row 0 of the position gradient


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,N,K", [(1, 36, 18), (5, 36, 3), (300, 4, 2), (513, 9, 8)])
def test_pos_grad_adds_in_ascending_image_order(dtype, B, N, K):
    """The contract of simseg_vit_keep_pos_grad: one fp32 accumulator per element, terms in ascending b.  fp32 addition is exact to state on
    the host in that order, so the comparison is for equality (a tree or an atomic sum would differ in the last bits)."""
    from simseg_amd import ops
    D = 128
    keep, inv = _keep(B, N, K, 21)
    dx = _rand(B, 1 + K, D, seed=3).to(DTYPES[dtype])
    got = ops.vit_keep_pos_grad(dx, inv)
    x, iv = dx.float().cpu().numpy(), inv.cpu().numpy()
    want = np.zeros((N + 1, D), dtype=np.float32)
    for b in range(B):
        want[0] += x[b, 0]
        n = np.nonzero(iv[b] >= 0)[0]
        want[1 + n] += x[b, 1 + iv[b, n]]
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), tt(want))
    bad = inv.clone()
    bad[0, :] = K                                                      # an entry >= K counts as dropped: nothing outside dx is read
    n0 = np.nonzero(iv[0] >= 0)[0]
    if B == 1:
        assert (ops.vit_keep_pos_grad(dx, bad)[1:] == 0).all()
    else:
        assert not torch.equal(ops.vit_keep_pos_grad(dx, bad)[1 + n0], got[1 + n0])


# ---- the whole tower --------------------------------------------------------------------------------------------------------------------
def _vit(seed=0):
    from simseg_amd.nn import ViT
    m = ViT("vit_test_patch16", img_size=96)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                                # (no parameter at its degenerate initial value: zero biases, unit gains, a 1e-6 [cls])
        for name, p in m.named_parameters():
            if name == "cls_token":
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    return m.cuda()


def _blocks(m, x, adt, lazy_ok):
    from simseg_amd import towers as T
    for blk in m.blocks:
        x = T.ViTBlockFn.apply(x, m.num_heads, adt, blk.norm1.weight, blk.norm1.bias, blk.attn.qkv.weight, blk.attn.qkv.bias,
                               blk.attn.proj.weight, blk.attn.proj.bias, blk.norm2.weight, blk.norm2.bias,
                               blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias, lazy_ok)
    return T.LayerNormFn.apply(x, m.norm.weight, m.norm.bias, 1e-6, adt, lazy_ok)


def _composed(m, image, adt, keep):
    """The project's own pieces: the full embedding, a torch gather of [cls] + the kept rows under autograd, the same blocks."""
    from simseg_amd import towers as T
    x = T.ViTEmbedFn.apply(image, m.patch_embed.proj.weight, m.patch_embed.proj.bias, m.cls_token, m.pos_embed, adt)
    B, _, D = x.shape
    idx = torch.cat([torch.zeros(B, 1, dtype=torch.long, device=x.device), 1 + keep.long()], 1)
    return _blocks(m, torch.gather(x, 1, idx[:, :, None].expand(-1, -1, D)), adt, False)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_tower_equals_full_embedding_then_gather(dtype):
    from simseg_amd import towers as T
    adt = DTYPES[dtype]
    m = _vit()
    B, N, K = 4, 36, 18
    image = _rand(B, 3, 96, 96, seed=1)
    keep, inv = _keep(B, N, K, 17)
    gy = _rand(B, 1 + K, m.embed_dim, seed=2)
    names, params = zip(*m.named_parameters())
    hits = T.SHADOW_HITS[0]
    y = T.vit_forward(m, image, adt, keep, inv)
    got = torch.autograd.grad(y, params, gy)
    hits_keep = T.SHADOW_HITS[0] - hits
    y_ref = _composed(m, image, adt, keep)
    want = torch.autograd.grad(y_ref, params, gy)
    assert y.shape == (B, 1 + K, m.embed_dim)
    pairs = [("output", y.detach(), y_ref.detach())] + list(zip(names, got, want))
    if adt == torch.float32:
        errs = {name: _rel(g, w_) for name, g, w_ in pairs}
        worst = max(errs, key=errs.get)
        print(f"tower fp32: largest error {errs[worst]:.2e} of max|ref| ({worst}); output {errs['output']:.2e}")
        assert errs[worst] <= 2e-4, (worst, errs[worst])
    else:
        cr = {name: _cos_ratio(g, w_) for name, g, w_ in pairs}
        lo = min(cr, key=lambda k: cr[k][0])
        far = max(cr, key=lambda k: abs(cr[k][1] - 1))
        print(f"tower {dtype}: lowest cosine {cr[lo][0]:.6f} ({lo}); norm ratio furthest from 1: {cr[far][1]:.4f} ({far}); output cosine {cr['output'][0]:.6f}")
        for name, (c, ratio) in cr.items():
            assert c > 0.99 and 0.9 < ratio < 1.1, (name, c, ratio)
    if dtype == "bf16":          # the new node consumed the first block's 16-bit shadow, as ViTEmbedFn does in a run without dropout
        hits = T.SHADOW_HITS[0]
        torch.autograd.grad(T.vit_forward(m, image, adt), params, _rand(B, 1 + N, m.embed_dim, seed=2))
        assert hits_keep == T.SHADOW_HITS[0] - hits and hits_keep >= 3


# ---- model and trainer ------------------------------------------------------------------------------------------------------------------
def _build(golden, extra=()):
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), TINY + list(extra), update_clip_config)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    g = golden("clip_glue")
    model.load_state_dict({k[3:]: tt(g[k]) for k in g.files if k.startswith("sd.")}, strict=False)
    return model.cuda()


def _batch(golden):
    g = golden("clip_train_ws1")
    return {"image": tt(g["r0.image"]).cuda(), "input_ids": tt(g["r0.input_ids"]).cuda(), "attention_mask": tt(g["r0.attention_mask"]).cuda()}


def _the_vit(model):
    from simseg_amd.nn import ViT
    (vit,) = [m for m in model.modules() if isinstance(m, ViT)]
    return vit


def test_model_trains_on_half_the_patches_and_evaluates_on_all(golden, monkeypatch):
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "bf16")
    from simseg_amd import nn as snn
    from simseg_amd.patchdrop import sample_keep_ref
    batch = _batch(golden)
    B = batch["image"].shape[0]
    m = _build(golden)
    vit = _the_vit(m)
    vit.set_patch_drop(0.5)
    m.train()
    snn.manual_dropout_seed(4321)
    feats = m.image_encoder(batch["image"])
    assert feats.shape == (B, 1 + 18, 128)
    first = vit.last_keep.clone()
    snn.manual_dropout_seed(4321)
    seed = snn.next_dropout_seed()                       # the seed that forward drew
    want_keep, want_inv = sample_keep_ref(B, 36, 18, seed)
    assert not vit.last_keep.requires_grad and not vit.last_inv.requires_grad
    assert torch.equal(first.cpu(), tt(want_keep)) and torch.equal(vit.last_inv.cpu(), tt(want_inv))
    m.image_encoder(batch["image"])
    assert not torch.equal(vit.last_keep, first)         # the next forward draws another subset
    loss = m(batch)[0]["nce_loss"]
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 20 and all(torch.isfinite(g_).all() for g_ in grads)
    assert vit.pos_embed.grad is not None and vit.patch_embed.proj.weight.grad.abs().max() > 0
    # evaluation never drops: all 36 patches, the bits of a model built without the feature
    m.eval()
    plain = _build(golden).eval()
    with torch.no_grad():
        f_eval, f_plain = m.image_encoder(batch["image"]), plain.image_encoder(batch["image"])
    assert f_eval.shape == (B, 1 + 36, 128) and torch.equal(f_eval, f_plain)


def test_trainer_runs_with_patch_dropout(golden):
    from simseg_amd.trainer import Trainer
    m = _build(golden, ["epoch=1", "optim.lr.init=1e-3"])
    m.train()
    tr = Trainer(m, m.cfg, steps_per_epoch=40, patch_drop_rate=0.5)
    vit = _the_vit(m)
    assert vit.patch_drop_rate == 0.5
    batch = _batch(golden)
    keeps = []
    for _ in range(3):
        out = tr.train_step(batch)
        assert torch.isfinite(out["loss"])
        keeps.append(vit.last_keep.clone())
    assert tr.step == 3 and keeps[0].shape == (batch["image"].shape[0], 18) and not torch.equal(keeps[0], keeps[1])
    assert all(torch.isfinite(p).all() for p in m.parameters())
    with pytest.raises(ValueError, match="image_k"):
        Trainer(m, m.cfg, steps_per_epoch=40, patch_drop_rate=0.9)
    m2 = _build(golden)
    Trainer(m2, m2.cfg, steps_per_epoch=40)               # None touches nothing
    assert _the_vit(m2).patch_drop_rate == 0.0


def test_rate_zero_is_the_model_without_the_feature(golden, monkeypatch):
    """train() with rate 0: the dropout seeds drawn (all of them the text tower's) and the loss are those of a ViT whose forward is the
    one-line call it was before the feature."""
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "bf16")
    from simseg_amd import nn as snn
    from simseg_amd import towers
    batch = _batch(golden)
    m = _build(golden)
    m.train()
    drawn = []
    real = snn.next_dropout_seed

    def spy():
        drawn.append(real())
        return drawn[-1]

    monkeypatch.setattr(snn, "next_dropout_seed", spy)
    snn.manual_dropout_seed(99)
    with_attr = m(batch)[0]["nce_loss"].detach().clone()
    seeds_with, state_with = list(drawn), snn._seed_state[0]
    drawn.clear()
    monkeypatch.setattr(snn.ViT, "forward", lambda self, x: towers.vit_forward(self, x, snn.compute_dtype()))
    snn.manual_dropout_seed(99)
    without = m(batch)[0]["nce_loss"].detach().clone()
    assert seeds_with and seeds_with == drawn and state_with == snn._seed_state[0]
    assert torch.equal(with_attr, without)
    assert _the_vit(m).last_keep is None
