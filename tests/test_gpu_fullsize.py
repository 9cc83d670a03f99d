"""BASELINE.json-sized cases and size-independent properties on MI355X."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _maxerr(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().max().item()


def test_retrieval_full_config5():
    """5000 images x 25000 captions, both directions (config 5): ranks equal a chunked torch evaluation of the same
    definition, recalls are monotone in k, and every caption's own image is retrievable."""
    from simseg_amd import ops
    from simseg_amd.heads import retrieval_recalls
    g = torch.Generator().manual_seed(5)
    img = F.normalize(torch.randn(5000, 512, generator=g), dim=-1).cuda()
    txt = F.normalize(img.repeat_interleave(5, 0) + 0.08 * torch.randn(25000, 512, generator=g).cuda(), dim=-1)
    gi, gt = torch.arange(5000).cuda(), (torch.arange(25000) // 5).cuda()
    i2t = retrieval_recalls(img, gi, txt, gt)
    t2i = retrieval_recalls(txt, gt, img, gi)
    for r in (i2t, t2i):
        assert 0.0 < r["R@1"] <= r["R@5"] <= r["R@10"] <= 1.0
    # ranks vs torch on a row sample (fp32 MFMA GEMM vs torch matmul differ in summation order: compare with a margin)
    sim = ops.gemm(txt, img)
    has, rank = ops.retrieval_rank(sim, gt, gi)
    assert int(has.sum()) == 25000
    rows = torch.arange(0, 25000, 97).cuda()
    s = txt[rows] @ img.T
    best = s.gather(1, gt[rows, None])
    lo = (s > best + 1e-5).sum(1)
    hi = (s > best - 1e-5).sum(1)
    r = rank[rows].long()
    assert bool(((r >= lo) & (r <= hi)).all())
    assert abs(t2i["R@1"] - float((rank == 0).float().mean())) < 1e-6
    # both directions from ONE similarity matrix (columns rank their rows): the same recalls as the two single-direction calls,
    # and column ranks of the [5000, 25000] matrix equal the row ranks of its transpose (same fp32 products, same comparisons)
    from simseg_amd.heads import retrieval_recalls_both
    a, b = retrieval_recalls_both(img, gi, txt, gt)
    for k in ("R@1", "R@5", "R@10"):
        assert abs(a[k] - i2t[k]) < 1e-9 and abs(b[k] - t2i[k]) < 2e-4, (k, a[k], i2t[k], b[k], t2i[k])
    simT = ops.gemm(img, txt)
    hasc, rankc = ops.retrieval_rank_cols(simT, gi, gt)
    assert int(hasc.sum()) == 25000
    rc = rankc[rows].long()
    assert bool(((rc >= lo) & (rc <= hi)).all())


def test_seg_similarity_full_config4():
    """Dense map for 8 windows of 512x512 (N=1024 patches) x 171 classes: fused row-normalise + GEMM vs torch."""
    from simseg_amd.heads import patch_text_similarity
    g = torch.Generator().manual_seed(3)
    proj = (torch.randn(8, 1024, 512, generator=g) * 2.5).cuda()
    text = F.normalize(torch.randn(171, 512, generator=g), dim=-1).cuda()
    sim = patch_text_similarity(proj, text)
    ref = F.normalize(proj, dim=-1) @ text.T
    assert _maxerr(sim, ref) < 1e-5
    assert float(sim.abs().max()) <= 1.0 + 1e-5            # cosine similarities
    # linearity in the text matrix (size-independent property)
    sim2 = patch_text_similarity(proj, 0.5 * text)
    assert _maxerr(sim2, 0.5 * sim) < 1e-6


def test_vit_small_512_window_vs_oracle(monkeypatch):
    """ViT-S on one 512x512 window (T = 1025 tokens, 17 attention key tiles): fp32 kernels vs the CPU oracle."""
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    from oracle import simseg_ref as R
    from simseg_amd.nn import ViT
    ref = R.init_weights_(R.RefViT("vit_small_patch16_224_in21k", 512), seed=4).eval()
    m = ViT("vit_small_patch16_224_in21k", 512)
    m.load_state_dict(ref.state_dict(), strict=False)
    m = m.cuda().eval()
    x = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = ref(x)
        got = m(x.cuda())
    assert got.shape == (1, 1025, 384)
    assert _maxerr(got, want) < 1e-3


def test_ddp_wrapper_single_process_matches_plain(monkeypatch):
    """torch DDP around the drop-in model (the reference wraps every model in DDP): same loss and gradients as the
    bare module -- exercises gradient_as_bucket_view with our hand-written backward nodes."""
    import torch.distributed as dist
    from test_gpu_model import _build
    from conftest import tt
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "bf16")
    created = False
    if not dist.is_initialized():
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29577", RANK="0", WORLD_SIZE="1")
        dist.init_process_group("nccl", rank=0, world_size=1)
        created = True
    try:
        def golden(name):
            return np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
        g = golden("clip_train_ws1")
        batch = {"image": tt(g["r0.image"]).cuda(), "input_ids": tt(g["r0.input_ids"]).cuda(), "attention_mask": tt(g["r0.attention_mask"]).cuda()}
        plain = _build(golden).eval()
        plain(batch)[0]["nce_loss"].backward()
        wrapped = _build(golden).eval()
        ddp = torch.nn.parallel.DistributedDataParallel(wrapped, device_ids=[0], gradient_as_bucket_view=True)
        for _ in range(2):                       # second iteration: grads are bucket views, zeroed in place
            ddp.zero_grad(set_to_none=False)
            loss = ddp(batch)[0]["nce_loss"]
            loss.backward()
        for (n, p), (_, q) in zip(plain.named_parameters(), wrapped.named_parameters()):
            assert p.grad is not None and q.grad is not None, n
            assert _maxerr(p.grad, q.grad) <= 1e-6 * (1 + float(p.grad.abs().max())), n
    finally:
        if created:
            dist.destroy_process_group()


# ---- full-size towers, both directions (ViT-B/16 + BERT-base dimensions: D=768, H=12, T=197 / L=77) ----------------------------------
def _build_vitb(img_size, extra=()):
    from conftest import REPO
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    argv = [f"transforms.input_size={img_size}", "model.image_encoder.pretrained=False", "model.text_encoder.pretrained=False"]
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-b.yaml"), argv + list(extra), update_clip_config)
    return build_from_cfg(cfg.model.name, cfg, PIPELINE)


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))


def test_vitb_bertbase_train_step_gradients_vs_oracle(monkeypatch):
    """BASELINE config 3's towers at full width and depth (ViT-B/16 @224: T=197, BERT-base L=77, ragged masks), B=6: bf16 (and, last, exact-fp32) forward +
    InfoNCE + backward on the HIP path against the fp32 CPU oracle on the same weights, under both tower schedules (one / two HIP
    streams).  Exercises the GEMM dispatch at D=768, the split-K weight gradients, 3- and 4-wave attention blocks, every fused epilogue.

    The bar.  A 12-layer bf16 network does not reproduce fp32 gradients to 0.999: torch's OWN bf16 autocast of the oracle (the
    reference's mixed-precision recipe, run here on the host as the yardstick) reaches cosines of 0.983-0.997 on these tensors.  So:
    loss within 1e-2 relative; every parameter gradient within 3 % in norm, cosine >= 0.985 AND at least as close to the fp32
    gradient as torch's autocast-bf16 gradient of the same tensor is (1 - cos <= 1 - cos_autocast, with a 1e-3 floor).  BERT's key
    bias is in the null space of the loss (softmax shift invariance): its gradient must be rounding noise (<= 1 % of the value-bias
    gradient of the same block; the flash-style delta = rowsum(dO * O) leaves ~5e-4)."""
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "bf16")
    from oracle import simseg_ref as R
    B, L = 6, 77
    ref = R.init_weights_(R.RefCLIP("vit_base_patch16_224_in21k", "bert-base-uncased", img_size=224), seed=12).eval()
    image = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(21))
    ids, mask = R.synthetic_text(B, L, 30522, seed=22, min_len=8)
    torch.set_num_threads(min(32, os.cpu_count() or 8))     # (the GPU box reports 256 logical CPUs; oversubscribing them is 100x slower)
    want, _, _ = ref.forward_loss_local(image, ids, mask)
    want.backward()
    g32 = {n: p.grad.clone() for n, p in ref.named_parameters()}
    ref.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        l16, _, _ = ref.forward_loss_local(image, ids, mask)
    l16.backward()
    yard = {n: _cos(p.grad, g32[n]) for n, p in ref.named_parameters()}
    # (round 3: the same step once more in the fp16 flavour - the reference's own AMP type - under the loss scale its GradScaler starts from)
    for mode, two in (("bf16", "0"), ("bf16", "1"), ("fp16", "1")):
        monkeypatch.setenv("SIMSEG_AMD_COMPUTE", mode)
        scale = 65536.0 if mode == "fp16" else 1.0
        monkeypatch.setenv("SIMSEG_AMD_TWO_STREAMS", two)
        m = _build_vitb(224)
        missing, unexpected = m.load_state_dict(ref.state_dict(), strict=False)
        assert not unexpected and all("position_ids" in k for k in missing)
        m = m.cuda().eval()                                      # eval: no dropout, so gradients are comparable
        # the batch is a temporary: its device tensors die with the forward call unless the model keeps them alive correctly
        loss = m({"image": image.cuda(), "input_ids": ids.cuda(), "attention_mask": mask.cuda()})[0]["nce_loss"]
        (loss * scale).backward()
        torch.cuda.synchronize()
        assert abs(loss.item() - want.item()) < 1e-2 * abs(want.item()), (loss.item(), want.item())
        worst_c, worst_r, bad, null = 1.0, 0.0, [], []
        for n, p in m.named_parameters():
            gr = g32[n]
            assert p.grad is not None, n
            assert torch.isfinite(p.grad).all(), n
            p.grad.div_(scale)
            if float(gr.norm()) < 1e-6:
                assert n.endswith("attention.self.key.bias"), (n, float(gr.norm()))
                rel = float(p.grad.float().norm()) / float(g32[n.replace(".key.", ".value.")].norm())
                null.append(rel)
                if rel > 1e-2:
                    bad.append((n, "null-space gradient / value-bias gradient", round(rel, 4)))
                continue
            c = _cos(p.grad, gr)
            r = float(p.grad.double().norm().cpu() / gr.double().norm())
            worst_c, worst_r = min(worst_c, c), max(worst_r, abs(r - 1))
            if not (c >= 0.985 and abs(r - 1) <= 0.03 and (1 - c) <= max(1 - yard[n], 1e-3)):
                bad.append((n, round(c, 5), round(r, 4), "autocast yardstick", round(yard[n], 5)))
        print(f"two_streams={two}: ViT-B/BERT-base {mode} gradients vs fp32 oracle: worst cosine {worst_c:.5f} (torch autocast-bf16 yardstick: "
              f"worst {min(v for k, v in yard.items() if not k.endswith('key.bias')):.5f}), worst |norm ratio - 1| {worst_r:.4f}; "
              f"key-bias null-space size max {max(null):.2e}")
        for b_ in bad:
            print("BAD", b_)
        assert not bad, f"{len(bad)} tensors outside the bar"
        del m
    # exact mode (a non-AMP run): the same hand-written backward in fp32 arithmetic reproduces the oracle's gradients elementwise -
    # which pins the backward's ALGEBRA at full size independently of bf16 rounding
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    monkeypatch.setenv("SIMSEG_AMD_TWO_STREAMS", "1")
    m = _build_vitb(224)
    m.load_state_dict(ref.state_dict(), strict=False)
    m = m.cuda().eval()
    loss = m({"image": image.cuda(), "input_ids": ids.cuda(), "attention_mask": mask.cuda()})[0]["nce_loss"]
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - want.item()) < 1e-4 * abs(want.item()), (loss.item(), want.item())
    worst, bad = 0.0, []
    for n, p in m.named_parameters():
        gr = g32[n]
        if float(gr.norm()) < 1e-6:
            continue
        err = float((p.grad.float().cpu() - gr).abs().max() / gr.abs().max())
        c = _cos(p.grad, gr)
        worst = max(worst, err)
        if not (err < 2e-3 and c > 0.99999):
            bad.append((n, err, c))
    print(f"fp32 exact mode: worst max-abs gradient error relative to the tensor's max {worst:.2e}")
    assert not bad, bad


def test_vitb_512_window_forward_vs_oracle(monkeypatch):
    """Config 4's tower: ViT-B/16 on a 512x512 window (T = 1025, the 256x256-tile GEMM region for B*T >= 256 rows, 17 key tiles):
    exact-fp32 kernels vs the CPU oracle <= 1e-3, and the bf16 path within bf16 noise of it."""
    from oracle import simseg_ref as R
    from simseg_amd.nn import ViT
    ref = R.init_weights_(R.RefViT("vit_base_patch16_224_in21k", 512), seed=14).eval()
    m = ViT("vit_base_patch16_224_in21k", 512)
    m.load_state_dict(ref.state_dict(), strict=False)
    m = m.cuda().eval()
    x = torch.randn(2, 3, 512, 512, generator=torch.Generator().manual_seed(3))
    torch.set_num_threads(min(32, os.cpu_count() or 8))     # (the GPU box reports 256 logical CPUs; oversubscribing them is 100x slower)
    with torch.no_grad():
        want = ref(x)
        monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
        got = m(x.cuda())
        monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "bf16")
        got16 = m(x.cuda())
    assert got.shape == (2, 1025, 768)
    err = _maxerr(got, want)
    assert err < 1e-3, err
    rel16 = float((got16.float().cpu() - want).norm() / want.norm())
    assert rel16 < 2e-2, rel16
    print(f"ViT-B@512 fp32 max err {err:.2e}; bf16 relative L2 error {rel16:.2e}")


def test_vitb_512_window_qscaled_attention_path(monkeypatch):
    """Round 6: in 16-bit evaluation at T >= 512 the ViT blocks fold scale * log2(e) into the q rows of `attn.qkv` (towers._wt_qscaled) and
    call simseg_attention_fwd_qscaled.  (i) bf16 and fp16 outputs with the folded projection agree with the unfolded path
    (SIMSEG_AMD_QSCALED=0: the generic entry point, q scaled by the kernel) to 16-bit noise and are as close to the fp32 oracle; (ii) the
    folded copy is a cache keyed on the parameters' versions: an in-place update of the weight changes the output exactly as it does without
    the fold."""
    from oracle import simseg_ref as R
    from simseg_amd import towers
    from simseg_amd.nn import ViT
    ref = R.init_weights_(R.RefViT("vit_base_patch16_224_in21k", 512), seed=15).eval()
    m = ViT("vit_base_patch16_224_in21k", 512)
    m.load_state_dict(ref.state_dict(), strict=False)
    m = m.cuda().eval()
    x = torch.randn(2, 3, 512, 512, generator=torch.Generator().manual_seed(4))
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    with torch.no_grad():
        want = ref(x)
        for mode, tol in (("bf16", 2e-2), ("fp16", 4e-3)):
            monkeypatch.setenv("SIMSEG_AMD_COMPUTE", mode)
            monkeypatch.setattr(towers, "_QSCALED", True)
            n0 = towers.COPIES.count("qscaled")
            got = m(x.cuda()).float().cpu()
            assert towers.COPIES.count("qscaled") >= max(n0, 12)         # one folded copy per block
            monkeypatch.setattr(towers, "_QSCALED", False)
            plain = m(x.cuda()).float().cpu()
            rel, rel0 = float((got - want).norm() / want.norm()), float((plain - want).norm() / want.norm())
            diff = float((got - plain).norm() / want.norm())
            print(f"ViT-B@512 {mode}: relative L2 error folded {rel:.2e}, unfolded {rel0:.2e}, between them {diff:.2e}")
            assert rel < tol and rel0 < tol and diff < tol and rel < 1.5 * rel0 + 1e-4
        # cache invalidation: perturb block 0's qkv weight in place
        monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "bf16")
        monkeypatch.setattr(towers, "_QSCALED", True)
        before = m(x.cuda()).float()
        w = dict(m.named_parameters())["blocks.0.attn.qkv.weight"]
        w.mul_(1.5)
        after = m(x.cuda()).float()
        monkeypatch.setattr(towers, "_QSCALED", False)
        after_plain = m(x.cuda()).float()
        assert float((after - before).norm() / before.norm()) > 1e-2                     # the update is seen
        assert float((after - after_plain).norm() / after_plain.norm()) < 2e-2           # and it is the same update


def test_compact_saved_tensors_keep_the_gradient_fidelity(monkeypatch):
    """Round 4 halves three streams of the 16-bit training step: the MLP blocks save GELU' as an 8-bit tile-blocked image (simseg_gemm act 7 / 8)
    instead of a 16-bit one (act 5 / 6), the ViT blocks hand the residual-stream gradient from LayerNorm backward to LayerNorm backward
    as the 16-bit copy those kernels write anyway instead of an fp32 image (simseg_layernorm_bwd dres_bf16; towers._RES16), and those kernels
    take the normalised value from the layer's saved 16-bit output instead of its fp32 input (y_bf16; towers._XHAT_Y).  At a batch whose
    GEMMs take the blocked path (B = 256: 50 432 image rows = 197 full tiles), ViT-B/16 + BERT-base: every parameter gradient of the bf16
    step stays as close to the exact-fp32 gradient (the same hand-written backward in fp32 arithmetic, same weights, same batch) as with
    the round-3 forms - per tensor and on average."""
    from oracle import simseg_ref as R
    from simseg_amd import ops, towers
    B, L = 256, 77
    assert ops.gemm_aux_blocked_ok(B * 197, 3072, 768)
    torch.manual_seed(5)
    m = _build_vitb(224).cuda().eval()
    # LayerNorm parameters of the image tower as a trained model has them (gains spread over a decade, some small; offsets of the gains' order):
    # the third compact form below takes the normalised value from the saved 16-bit LayerNorm output, (y - beta) / gamma
    gg = torch.Generator(device="cuda").manual_seed(9)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "image_encoder" in n and "norm" in n and n.endswith("weight"):
                p.copy_(torch.exp(torch.randn(p.shape, device="cuda", generator=gg) * 0.7).clamp(0.03, 4.0))
            if "image_encoder" in n and "norm" in n and n.endswith("bias"):
                p.copy_(torch.randn(p.shape, device="cuda", generator=gg) * 0.3)
    image = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(31)).cuda()
    ids, mask = R.synthetic_text(B, L, 30522, seed=32, min_len=8)
    batch = {"image": image, "input_ids": ids.cuda(), "attention_mask": mask.cuda()}
    monkeypatch.setenv("SIMSEG_AMD_TWO_STREAMS", "1")
    calls, lnb = [], []
    real_gemm, real_lnb = ops.gemm, ops.layernorm_bwd
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: (calls.append(k.get("act", 0)), real_gemm(*a, **k))[1])
    monkeypatch.setattr(ops, "layernorm_bwd", lambda *a, **k: (lnb.append((k.get("dres16") is not None, k.get("want_f32", True))), real_lnb(*a, **k))[1])
    grads, losses = {}, {}
    for tag, mode, g8, r16, xy in (("fp32", "fp32", False, False, False), ("r3", "bf16", False, False, False), ("g8", "bf16", True, False, False),
                                   ("g8r16", "bf16", True, True, False), ("g8r16y", "bf16", True, True, True)):
        monkeypatch.setenv("SIMSEG_AMD_COMPUTE", mode)
        monkeypatch.setattr(towers, "_GELU8", g8)
        monkeypatch.setattr(towers, "_RES16", r16)
        monkeypatch.setattr(towers, "_XHAT_Y", xy)
        calls.clear(); lnb.clear()
        m.zero_grad(set_to_none=True)
        loss = m(batch)[0]["nce_loss"]
        loss.backward()
        torch.cuda.synchronize()
        losses[tag] = float(loss)
        grads[tag] = {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}
        if tag == "r3":
            assert calls.count(5) == 24 and calls.count(6) == 24 and 7 not in calls, sorted(set(calls))
            assert not any(a for a, _ in lnb)
        if tag == "g8r16y":
            assert sum(1 for a, _ in lnb if a) == 24      # (the same 24 calls; they now carry y16 / beta - checked at the kernel level)
        if tag in ("g8", "g8r16", "g8r16y"):
            assert calls.count(7) == 24 and calls.count(8) == 24 and 5 not in calls, sorted(set(calls))      # every MLP block of both towers
        if tag in ("g8r16", "g8r16y"):       # the 24 LayerNorm backward calls of the ViT blocks take the 16-bit residual gradient; 24 + the final norm write no fp32 image
            assert sum(a for a, _ in lnb) == 24 and sum(not w for _, w in lnb) == 25, lnb
    assert abs(losses["g8r16y"] - losses["r3"]) < 1e-6 * abs(losses["r3"]) + 1e-7      # the forward does not change
    base = {n: 1 - _cos(grads["r3"][n], g) for n, g in grads["fp32"].items() if float(g.norm()) >= 1e-6}
    for tag in ("g8", "g8r16", "g8r16y"):
        d = {n: 1 - _cos(grads[tag][n], grads["fp32"][n]) for n in base}
        worse = [(n, base[n], d[n]) for n in base if d[n] > 1.25 * base[n] + 2e-4]
        print(f"1 - cosine to the exact-fp32 gradient, mean over {len(base)} tensors: round-3 forms {np.mean(list(base.values())):.4e}, {tag} {np.mean(list(d.values())):.4e}; "
              f"max {max(base.values()):.4e} / {max(d.values()):.4e}")
        assert not worse, worse[:5]
        assert np.mean(list(d.values())) <= 1.05 * np.mean(list(base.values())) + 1e-5


def test_sliding_window_full_config4_properties(monkeypatch):
    """BASELINE configs[3] at its full size - ViT-B/16, 512 x 1024 source images, 3 windows of 512^2 at stride 256, 171 classes - through
    size-independent properties of the stitch (the oracle loop is far too slow here; tests/test_gpu_miou_gate.py pins the pipeline
    against it at a small size):  the stitched map equals window 0 / window 2 where only they cover the image (patch columns 0-15 /
    48-63), is the mean of the two covering windows in between, the image scores are the mean of the window scores, and the areas the
    evaluation accumulates are exactly the labelled pixels.  Exact fp32 and bf16."""
    from simseg_amd import ops, segpost
    from simseg_amd.heads import patch_text_similarity
    B, H, W, C, win, stride = 2, 512, 1024, 171, 512, 256
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, 3, H, W, generator=g).cuda()
    text = F.normalize(torch.randn(C, 512, generator=g), dim=-1).cuda()
    labels = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    labels[torch.rand(B, H, W, generator=g) < 0.05] = 255
    labels = labels.cuda()
    torch.manual_seed(5)
    model = _build_vitb(win).cuda().eval()
    for mode, sim_dt, tol in (("fp32", None, 0.0), ("bf16", torch.bfloat16, 0.0)):
        monkeypatch.setenv("SIMSEG_AMD_COMPUTE", mode)
        with torch.no_grad():
            wins = segpost.extract_windows(x, win, stride)
            assert wins.shape == (B * 3, 3, win, win) and torch.equal(wins[4], x[1, :, :, 256:768])
            feats = model.forward_image_feature(wins)
            sim_w = patch_text_similarity(model.image_projection(feats), text, compute_dtype=sim_dt).float()      # [6, 1024, C]
            sc_w = ops.gemm(model.forward_image_project(feats).float(), text)
            st = segpost.encode_batch_sliding(model, x, text, 10, win=win, stride=stride, crf=False, sim_dtype=sim_dt)
            sim = ops.stitch_windows(sim_w, 1, 3, 32, 16).view(B, 32, 64, C)
        w = sim_w.view(B, 3, 32, 32, C)
        assert torch.equal(sim[:, :, :16], w[:, 0, :, :16]) and torch.equal(sim[:, :, 48:], w[:, 2, :, 16:])
        assert torch.equal(sim[:, :, 16:32], (w[:, 0, :, 16:] + w[:, 1, :, :16]) / 2) and torch.equal(sim[:, :, 32:48], (w[:, 1, :, 16:] + w[:, 2, :, :16]) / 2)
        sc = ((sc_w.view(B, 3, C)[:, 0] + sc_w.view(B, 3, C)[:, 1]) + sc_w.view(B, 3, C)[:, 2]) / 3
        ci, cs, _ = ops.seg_select(sc, 10)
        # (the pipeline's own pass over the towers is a second launch sequence: scores agree to rounding, candidates exactly)
        assert torch.equal(ci, st["cand_idx"]) and torch.allclose(cs, st["cand_score"], rtol=1e-5 if mode == "fp32" else 2e-2, atol=1e-6)
        assert st["masks"].shape == (B, 5, H, W)
        hist = torch.zeros(3, C, device="cuda", dtype=torch.int64)
        with torch.no_grad():
            out = segpost.finish_batch(st, labels, hist=hist, want_pred=True)
        assert int(hist[2].sum()) == int((labels != 255).sum()) == int(hist[1].sum())
        assert int(hist[0].sum()) == int(((out["pred"] == labels.int()) & (labels != 255)).sum())
