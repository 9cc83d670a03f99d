"""Sliding-window zero-shot segmentation on images of any size (segpost.encode_images_sliding + finish_sliding; the kernels
simseg_slide_extract / _scores / _stitch): against the numpy pixel-stitch loop (tests/test_slide_geometry.py), against the exact-tiling
path it must reproduce (encode_batch_sliding + finish_batch), against the oracle's per-image loop, and beyond the old 4096-patch cap."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_gpu_miou_gate import MEAN, STD, _build, _labels_from, _miou, _voc_like
from test_slide_geometry import normalise_ref, stitch_pixels_ref

pytestmark = pytest.mark.gpu

RAGGED = [(96, 150), (80, 80), (131, 257), (96, 192)]


def _pad_window(img, y0, x0, win):
    """[3, H, W] -> the window at (y0, x0), zero past the border (numpy)."""
    out = np.zeros((3, win, win), np.float32)
    h, w = min(win, img.shape[1] - y0), min(win, img.shape[2] - x0)
    out[:, :h, :w] = img[:, y0:y0 + h, x0:x0 + w]
    return out


def test_slide_kernels_vs_numpy_loop():
    """extract == slicing the zero-padded image, scores == the window-order mean, stitched prob / mask / min-max == the numpy loop, bit for
    bit; a constant map gives NaN / 0 as seg_masks does."""
    from simseg_amd import ops, segpost
    win, stride, C, K = 96, 48, 21, 5
    rng = np.random.default_rng(11)
    imgs = [rng.standard_normal((3, H, W)).astype(np.float32) for H, W in RAGGED]
    plan = ops.slide_plan(RAGGED, win, stride, "cuda")
    flat = torch.cat([torch.from_numpy(i).reshape(-1) for i in imgs]).cuda()
    Nw = len(plan["windows"])
    got = ops.slide_extract(flat, plan).cpu().numpy()
    want = np.stack([_pad_window(imgs[b], y0, x0, win) for b, y0, x0 in plan["windows"]])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ops.slide_extract(flat, plan, 3, 5).cpu().numpy(), want[3:8])
    sc_w = rng.standard_normal((Nw, C)).astype(np.float32)
    sc = ops.slide_scores(torch.from_numpy(sc_w).cuda(), plan).cpu().numpy()
    sim_w = rng.standard_normal((Nw, 36, C)).astype(np.float32)
    for w, (b, _, _) in enumerate(plan["windows"]):
        if b == 2:
            sim_w[w, :, 4] = 0.25                                          # image 2, class 4: a constant stitched map
    cand = torch.tensor([[3, 7, -1, 12, -1], [5, -1, -1, -1, -1], [4, 9, 1, -1, 20], [-1, -1, -1, -1, -1]], dtype=torch.int32)
    prob, mask, minmax = ops.slide_stitch(torch.from_numpy(sim_w).cuda(), plan, cand.cuda())
    for b, (H, W) in enumerate(RAGGED):
        ws = [w for w, (bb, _, _) in enumerate(plan["windows"]) if bb == b]
        ref = np.zeros(C, np.float32)
        for w in ws:
            ref += sc_w[w]
        np.testing.assert_array_equal(sc[b], ref / np.float32(len(ws)))
        offs = [plan["windows"][w][1:] for w in ws]
        P, M = ops.slide_planes(prob, plan, b).cpu().numpy(), ops.slide_planes(mask, plan, b).cpu().numpy()
        for k in range(K):
            c = int(cand[b, k])
            if c < 0:
                assert not M[k].any() and not P[k].any()
                continue
            S = stitch_pixels_ref(sim_w[ws][:, :, c:c + 1], offs, H, W, win)[:, :, 0]
            p, m = normalise_ref(S)
            np.testing.assert_array_equal(P[k], p)
            np.testing.assert_array_equal(M[k], m)
            assert minmax[b, k].tolist() == [float(S.min()), float(S.max())]
    assert np.isnan(ops.slide_planes(prob, plan, 2)[0].cpu().numpy()).all()


class _Memo:
    """The towers' split-K GEMMs accumulate with atomics, so two passes over the same windows agree to rounding, not to the bit.  This
    wrapper (and _memo_ops) hands the second path the first path's tower outputs for bit-identical inputs, so that what is compared is
    everything downstream of the towers."""

    def __init__(self, m):
        self.m, self.cache = m, {}

    def _get(self, name, x, fn):
        key = (name, tuple(x.shape), str(x.dtype), hashlib.sha1(x.contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest())
        if key not in self.cache:
            self.cache[key] = fn(x)
        return self.cache[key]

    def forward_image_feature(self, x):
        return self._get("feat", x, self.m.forward_image_feature)

    def forward_image_project(self, x):
        return self._get("pool", x, self.m.forward_image_project)

    def image_projection(self, x):
        return self._get("proj", x, self.m.image_projection)


def _memo_ops(monkeypatch, memo, text):
    from simseg_amd import heads, ops
    pts, gemm = heads.patch_text_similarity, ops.gemm
    monkeypatch.setattr(heads, "patch_text_similarity", lambda p, t, compute_dtype=None: memo._get(f"sim{compute_dtype}", p, lambda x: pts(x, t, compute_dtype=compute_dtype)))
    monkeypatch.setattr(ops, "gemm", lambda a, b, **kw: memo._get("score", a, lambda x: gemm(x, b)) if (b is text and not kw) else gemm(a, b, **kw))


def _vitb(win):
    from test_gpu_fullsize import _build_vitb
    torch.manual_seed(5)
    return _build_vitb(win).cuda().eval()


@pytest.mark.parametrize("case", ["tiny_fp32", "tiny_fp32_crf", "vitb_fp32", "vitb_bf16"])
def test_exact_tiling_equals_existing_path(case, monkeypatch):
    """On images that window_grid() accepts, encode_images_sliding + finish_sliding == encode_batch_sliding + finish_batch: candidates,
    masks and histograms.  Without the CRF bit for bit.  With it, the device CRF's hash build numbers lattice points in arrival order, so
    two calls agree to rounding in their marginals (tests/test_segpost.py): there the masks must agree on >= 99.99 % of the pixels."""
    from simseg_amd import segpost
    crf = case.endswith("crf")
    mode, sim_dt = ("bf16", torch.bfloat16) if case.endswith("bf16") else ("fp32", None)
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", mode)
    if case.startswith("vitb"):
        win, stride, H, W, C, B = 512, 256, 512, 1024, 171, 2
        model = _vitb(win)
    else:
        win, stride, H, W, C, B = 96, 48, 96, 192, 21, 3
        model = _build("vit_test_patch16", 128, "bert-test", 128, win, seed=5).eval().cuda()
    _, x = _voc_like(B, W, seed=23)
    x = x[:, :, :H].contiguous().cuda()
    g = torch.Generator().manual_seed(3)
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=g), dim=-1).cuda()
    labels = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    labels[torch.rand(B, H, W, generator=g) < 0.05] = 255
    labels = labels.cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    memo = _Memo(model)
    _memo_ops(monkeypatch, memo, text)
    h_old = torch.zeros(3, C, device="cuda", dtype=torch.int64)
    h_new = torch.zeros(3, C, device="cuda", dtype=torch.int64)
    with torch.no_grad():
        st = segpost.encode_batch_sliding(memo, x, text, 10, win=win, stride=stride, crf=crf, mean=mean, std=std, sim_dtype=sim_dt)
        old = segpost.finish_batch(st, labels, hist=h_old)
        n_cached = len(memo.cache)
        st2 = segpost.encode_images_sliding(memo, [x[b] for b in range(B)], text, 10, win=win, stride=stride, crf=crf, mean=mean, std=std,
                                            sim_dtype=sim_dt)
        new = segpost.finish_sliding(st2, [labels[b] for b in range(B)], hist=h_new)
    assert len(memo.cache) == n_cached                       # the new path cut bit-identical windows: every tower call was a cache hit
    assert torch.equal(st["cand_idx"], st2["cand_idx"]) and torch.equal(st["cand_score"], st2["cand_score"])
    assert (st["cand_idx"] >= 0).sum() >= B
    m_old, m_new = old["masks"], torch.stack(new["masks"])
    if crf:
        agree = float((m_old == m_new).float().mean())
        print(f"{case}: mask agreement {agree:.6f}")
        assert agree >= 0.9999
        assert float((h_old - h_new).abs().sum()) <= 1e-4 * 3 * B * H * W
    else:
        assert torch.equal(m_old, m_new)
        assert torch.equal(h_old, h_new)


def test_end_to_end_vs_oracle_loop(monkeypatch):
    """Ragged images (one smaller than the window, odd sizes), labels at another resolution, the DenseCRF: the device path against the
    oracle's loop - oracle towers per zero-padded window, the numpy pixel stitch, oracle candidates, crf_ref.dense_crf, 7x7 closing, nearest
    resize.  fp32 towers; pixel agreement >= 0.999 and |delta mIoU| <= 0.1."""
    from oracle import crf_ref as CR
    from oracle import segpost_ref as SR
    from oracle import simseg_ref as R
    from simseg_amd import segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    win, stride, C, top = 96, 48, 21, 10
    sizes = [(96, 150), (80, 80), (131, 197), (113, 96)]
    lab_sizes = [(64, 112), (96, 96), (128, 192), (80, 64)]            # (multiples of 16: _labels_from relabels 16-pixel blocks)
    g = torch.Generator().manual_seed(3)
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=g), dim=-1)
    model = _build("vit_test_patch16", 128, "bert-test", 128, win, seed=5).eval()
    ref = R.RefCLIP("vit_test_patch16", "bert-test", img_size=win)
    ref.load_state_dict(model.state_dict(), strict=False)
    ref.eval()
    model = model.cuda()
    u8s, xs, wants = [], [], []
    visited = 0
    with torch.no_grad():
        for b, (H, W) in enumerate(sizes):
            u8, x = _voc_like(1, max(H, W), seed=40 + b)
            u8, x = np.ascontiguousarray(u8[0, :H, :W]), x[0, :, :H, :W].contiguous()
            u8s.append(u8); xs.append(x)
            offs = segpost.slide_windows(H, W, win, stride)
            wm, ws = [], []
            for y0, x0 in offs:
                xw = torch.from_numpy(_pad_window(x.numpy(), y0, x0, win))[None]
                feats = ref.forward_image_feature(xw)
                wm.append(R.seg_similarity(ref.image_projection(feats), text)[0].numpy())
                ws.append(R.seg_image_scores(ref.forward_image_project(feats), text)[0].numpy())
            S = stitch_pixels_ref(np.stack(wm), offs, H, W, win)
            sc = np.zeros(C, np.float32)
            for w_ in ws:
                sc += w_.astype(np.float32)
            sc = sc / np.float32(len(ws))
            idx, scv, _ = SR.select_candidates(torch.from_numpy(sc), top)
            Hl, Wl = lab_sizes[b]
            temp = np.zeros((C, Hl, Wl))
            for k, c in enumerate(idx):
                if c < 0:
                    continue
                visited += 1
                prob, _ = normalise_ref(S[:, :, c])
                m = (CR.dense_crf(u8, prob) * 255).astype(np.uint8)
                m = SR.morph7_fast(SR.morph7_fast(m, False), True)
                temp[c] = SR.resize_nearest(m, Hl, Wl).astype(np.float64) * scv[k]
            wants.append(temp.argmax(0))
    assert visited >= len(sizes)
    labels = [_labels_from(w[None], seed=9 + b, C=C)[0] for b, w in enumerate(wants)]
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    hist = torch.zeros(3, C, device="cuda", dtype=torch.int64)
    with torch.no_grad():
        st = segpost.encode_images_sliding(model, [x.cuda() for x in xs], text.cuda(), top, win=win, stride=stride, crf=True, mean=mean, std=std)
        out = segpost.finish_sliding(st, [torch.from_numpy(l).cuda() for l in labels], hist=hist, want_pred=True)
    hist_ref = np.zeros((3, C))
    agree_n = total = 0
    for b in range(len(sizes)):
        hist_ref += np.stack([h.numpy() for h in SR.intersect_and_union(wants[b], labels[b], C)])
        p = out["pred"][b].cpu().numpy()
        agree_n += int((p == wants[b]).sum()); total += p.size
    agree = agree_n / total
    (_, miou), (_, miou_ref) = _miou(hist.cpu().numpy()), _miou(hist_ref)
    print(f"any-size sliding window: pixel agreement {agree:.5f}, mIoU {miou:.3f} vs oracle loop {miou_ref:.3f}")
    assert agree >= 0.999 and abs(miou - miou_ref) <= 0.1


def test_batching_invariance(monkeypatch):
    """A ragged list in one call (windows through the towers 5 at a time: 5 does not divide the 17 windows) == each image alone."""
    from simseg_amd import segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    win, stride, C = 96, 48, 21
    model = _build("vit_test_patch16", 128, "bert-test", 128, win, seed=5).eval().cuda()
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=torch.Generator().manual_seed(3)), dim=-1).cuda()
    g = torch.Generator().manual_seed(8)
    xs = [torch.randn(3, H, W, generator=g).cuda() for H, W in RAGGED]
    labs = [torch.randint(0, C, (H, W), generator=g, dtype=torch.int64).to(torch.uint8).cuda() for H, W in RAGGED]
    assert sum(len(segpost.slide_windows(H, W, win, stride)) for H, W in RAGGED) == 17
    hist = torch.zeros(3, C, device="cuda", dtype=torch.int64)
    with torch.no_grad():
        st = segpost.encode_images_sliding(model, xs, text, 10, win=win, stride=stride, crf=False, window_batch=5)
        out = segpost.finish_sliding(st, labs, hist=hist)
        hsum = torch.zeros_like(hist)
        for b in range(len(xs)):
            st1 = segpost.encode_images_sliding(model, [xs[b]], text, 10, win=win, stride=stride, crf=False)
            one = segpost.finish_sliding(st1, [labs[b]], hist=hsum)
            assert torch.equal(one["cand_idx"][0], out["cand_idx"][b])
            assert torch.equal(one["masks"][0], out["masks"][b])
    assert torch.equal(hist, hsum)
    assert int(hist[2].sum()) == sum(int((l != 255).sum()) for l in labs)


def test_beyond_the_old_patch_cap(monkeypatch):
    """A 1024 x 1536 image (6144 patches, 15 windows; seg_masks stops at 4096 patches) with ViT-S, random weights, bf16, no CRF: the stitched
    maps equal the numpy loop applied to the same per-window similarity maps."""
    from simseg_amd import heads, segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "bf16")
    win, stride, C, H, W = 512, 256, 21, 1024, 1536
    model = _build("vit_small_patch16_224_in21k", 384, "bert-test", 128, win, seed=6).eval().cuda()
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=torch.Generator().manual_seed(3)), dim=-1).cuda()
    x = torch.randn(3, H, W, generator=torch.Generator().manual_seed(2)).cuda()
    seen = []
    pts = heads.patch_text_similarity

    def rec(p, t, compute_dtype=None):
        seen.append(pts(p, t, compute_dtype=compute_dtype))
        return seen[-1]
    monkeypatch.setattr(heads, "patch_text_similarity", rec)
    with torch.no_grad():
        st = segpost.encode_images_sliding(model, [x], text, 10, win=win, stride=stride, crf=False, sim_dtype=torch.bfloat16, window_batch=8)
    torch.cuda.synchronize()
    assert (H // 16) * (W // 16) > 4096
    sim_w = torch.cat(seen).float().cpu().numpy()
    offs = segpost.slide_windows(H, W, win, stride)
    assert sim_w.shape == (15, 1024, C) and len(offs) == 15
    from simseg_amd import ops
    P, M = ops.slide_planes(st["prob"], st["plan"], 0).cpu().numpy(), ops.slide_planes(st["masks"], st["plan"], 0).cpu().numpy()
    cand = st["cand_idx"][0].tolist()
    assert any(c >= 0 for c in cand)
    for k, c in enumerate(cand):
        if c < 0:
            continue
        p, m = normalise_ref(stitch_pixels_ref(sim_w[:, :, c:c + 1], offs, H, W, win)[:, :, 0])
        np.testing.assert_array_equal(P[k], p)
        np.testing.assert_array_equal(M[k], m)


def test_sharded_evaluation_on_list_batches(monkeypatch):
    """evaluate_sharded(..., slide=) on batches of image / label LISTS in one process (the pipelined path with the DenseCRF) == the sum of
    the per-batch histograms of encode_images_sliding + finish_sliding."""
    from simseg_amd import segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    win, stride, C, top = 96, 48, 21, 10
    model = _build("vit_test_patch16", 128, "bert-test", 128, win, seed=5).eval().cuda()
    text = torch.nn.functional.normalize(torch.randn(C, 512, generator=torch.Generator().manual_seed(3)), dim=-1).cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    g = torch.Generator().manual_seed(4)
    batches = []
    for i in range(4):
        sz = [RAGGED[(i + j) % 4] for j in range(1 + i % 3)]
        imgs = []
        for b, (H, W) in enumerate(sz):
            _, x = _voc_like(1, max(H, W), seed=70 + 5 * i + b)
            imgs.append(x[0, :, :H, :W].contiguous())
        labs = [torch.randint(0, C, (H + 7, W - 5), generator=g, dtype=torch.int64).to(torch.uint8) for H, W in sz]
        batches.append((imgs, labs))
    with torch.no_grad():
        res = segpost.evaluate_sharded(model, batches, text, top, slide=(win, stride), crf=True, mean=mean, std=std, device="cuda")
        want = torch.zeros(3, C, device="cuda", dtype=torch.int64)
        for imgs, labs in batches:
            st = segpost.encode_images_sliding(model, [x.cuda() for x in imgs], text, top, win=win, stride=stride, crf=True, mean=mean, std=std)
            segpost.finish_sliding(st, [l.cuda() for l in labs], hist=want)
    torch.cuda.synchronize()
    assert res["images"] == sum(len(i) for i, _ in batches)
    print(f"sharded list batches: |hist - sum of batches| = {int((res['hist'] - want).abs().sum())} of {int(want[2].sum())} labelled pixels")
    # (the DenseCRF's hash build numbers lattice points in arrival order: two runs agree to rounding in the marginals, tests/test_segpost.py)
    assert float((res["hist"] - want).abs().sum()) <= 1e-4 * float(want[2].sum() * 3)
    assert int(res["hist"][2].sum()) == int(want[2].sum())


def test_tool_ragged_synthetic():
    """tools/seg_eval_device.py --synthetic-sizes: ragged synthetic images through the any-size path, end to end in a subprocess."""
    env = dict(os.environ, MASTER_PORT="29534", PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, "tools", "seg_eval_device.py"), "--cfg", os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"),
           "--synthetic", "8", "--batch", "3", "--synthetic-sizes", "96x150,80x80,131x257", "--slide", "96,48", "transforms.input_size=96",
           "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128", "model.text_encoder.tag=bert-test",
           "model.text_encoder.embedding_dim=128"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "8 samples evaluated" in out.stdout and "final mean iou" in (out.stdout + out.stderr)
