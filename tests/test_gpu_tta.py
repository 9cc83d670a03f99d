"""Multi-scale and flip test-time augmentation over sliding windows (segpost.encode_images_multiscale; the kernels
simseg_slide_extract_flip / simseg_slide_stitch_multi) against the NumPy restatement of the contract (tests/_tta_ref.py, float64) and
against the single-pass path it must reproduce bit for bit (ops.slide_stitch, segpost.encode_images_sliding)."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import _tta_ref as TR
from _tta_ref import C, K, SIZES, STRIDE, WIN

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # configs/clip/*.yaml transforms.normalize
ATOL = 2e-6       # cosines in [-1, 1]; <= 4 covering windows per pass and <= 6 passes: < 32 fp32 roundings at <= 2^-24 relative on magnitudes <= 6


def _plans(per_pass_sizes):
    from simseg_amd import ops
    return [ops.slide_plan(sz, WIN, STRIDE, "cuda") for sz in per_pass_sizes]


def test_extract_flip_equals_extract_of_the_flipped_image():
    """An odd W, an image smaller than the window, windows running past the border: bit-identical to slide_extract(torch.flip(image))."""
    from simseg_amd import ops
    g = torch.Generator().manual_seed(7)
    imgs = [torch.randn(3, H, W, generator=g) for H, W in SIZES]
    plan = ops.slide_plan(SIZES, WIN, STRIDE, "cuda")
    flat = torch.cat([i.reshape(-1) for i in imgs]).cuda()
    flat_m = torch.cat([torch.flip(i, [-1]).contiguous().reshape(-1) for i in imgs]).cuda()
    want = ops.slide_extract(flat_m, plan)
    got = ops.slide_extract_flip(flat, plan)
    assert got.shape == (len(plan["windows"]), 3, WIN, WIN) and len(plan["windows"]) > len(SIZES)
    assert torch.equal(got, want)
    assert torch.equal(ops.slide_extract_flip(flat, plan, 2, 5), want[2:7])
    assert torch.equal(ops.slide_extract_flip(flat, plan, flip=False), ops.slide_extract(flat, plan))
    with pytest.raises(ValueError):
        ops.slide_extract_flip(flat[:-1], plan)
    with pytest.raises(ValueError):
        ops.slide_extract_flip(flat.double(), plan)
    with pytest.raises(ValueError):
        ops.slide_extract_flip(flat, plan, 3, len(plan["windows"]))


def test_fusion_against_numpy_reference():
    """Five passes (scale 1 plain and mirrored, 0.5, 1.5 mirrored, 0.75 mirrored) over four ragged images in one batch."""
    from simseg_amd import ops
    case = TR.fusion_case()
    plans = _plans(case["sizes"])
    sims = [torch.from_numpy(s).cuda() for s in case["sims"]]
    cand = torch.tensor(case["cand"], dtype=torch.int32).cuda()
    prob, mask, minmax = ops.slide_stitch_multi(sims, plans, case["flips"], plans[0], cand)
    torch.cuda.synchronize()
    minmax = minmax.cpu().numpy()
    worst = {"F": 0.0, "minmax": 0.0, "prob": 0.0}
    differ = near = total = 0
    for b in range(len(SIZES)):
        P_, M_ = ops.slide_planes(prob, plans[0], b).cpu().numpy(), ops.slide_planes(mask, plans[0], b).cpu().numpy()
        for k in range(K):
            if case["cand"][b][k] < 0:
                assert not P_[k].any() and not M_[k].any() and not minmax[b, k].any()          # unvisited slots stay all zero
                continue
            p_ref, m_ref, (mn, mx), F = case["ref"][(b, k)]
            worst["minmax"] = max(worst["minmax"], abs(minmax[b, k, 0] - mn), abs(minmax[b, k, 1] - mx))
            worst["prob"] = max(worst["prob"], float(np.abs(P_[k] - p_ref).max()))
            # F as the device holds it: prob de-normalised with the device's own min / max (float64 arithmetic on its fp32 values)
            F_dev = P_[k].astype(np.float64) * (np.float64(minmax[b, k, 1]) - np.float64(minmax[b, k, 0])) + np.float64(minmax[b, k, 0])
            worst["F"] = max(worst["F"], float(np.abs(F_dev - F).max()))
            close = np.abs(p_ref - 0.5) < 1e-5
            differ += int(((M_[k] != m_ref) & ~close).sum())
            near += int(close.sum()); total += close.size
            assert set(np.unique(M_[k])) <= {0, 255}
    print(f"fused stitch vs float64 reference: max |dF| {worst['F']:.3e}, |dminmax| {worst['minmax']:.3e}, |dprob| {worst['prob']:.3e}; "
          f"{near} of {total} mask pixels within 1e-5 of the threshold, {differ} differing elsewhere")
    assert worst["F"] <= ATOL and worst["minmax"] <= ATOL and worst["prob"] <= ATOL
    assert differ == 0 and near <= 1e-3 * total
    # pad bytes between the images' planes stay zero too
    used = torch.zeros(plans[0]["out_numel"], dtype=torch.bool)
    for b, (H, W) in enumerate(SIZES):
        used[plans[0]["out_off"][b]:plans[0]["out_off"][b] + K * H * W] = True
    assert not prob.cpu()[~used].any() and not mask.cpu()[~used].any()


def test_single_pass_is_slide_stitch_bit_for_bit():
    """passes = [(1.0, no flip)] pins the layout: prob, mask and minmax of slide_stitch_multi == ops.slide_stitch on the same inputs."""
    from simseg_amd import ops
    case = TR.fusion_case()
    plan = _plans(case["sizes"][:1])[0]
    sim = torch.from_numpy(case["sims"][0]).cuda()
    cand = torch.tensor(case["cand"], dtype=torch.int32).cuda()
    want = ops.slide_stitch(sim, plan, cand)
    got = ops.slide_stitch_multi([sim], [plan], [False], plan, cand)
    assert int((cand >= 0).sum()) >= 8
    for g, w, name in zip(got, want, ("prob", "mask", "minmax")):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert torch.equal(g.view(torch.uint8) if g.dtype != torch.uint8 else g, w.view(torch.uint8) if w.dtype != torch.uint8 else w), name


def test_flip_symmetry_at_kernel_level():
    """A mirrored pass fed the mirrored arrangement of another pass's cells (window j <-> nx-1-j, cell column cx <-> n-1-cx) on images
    whose window sets are mirror-symmetric (W = win + 2 stride) reproduces the unflipped result.  Image 0 has one row of windows: a pixel's
    two covering windows swap places in the sum, a + b == b + a, so the result is bit-identical.  Image 1 has two rows: the four terms are
    summed in another order there, which agrees to rounding (2e-6)."""
    from simseg_amd import ops
    sizes = [(WIN, WIN + 2 * STRIDE), (WIN + STRIDE, WIN + 2 * STRIDE)]
    plan = ops.slide_plan(sizes, WIN, STRIDE, "cuda")
    n = WIN // 16
    rng = np.random.default_rng(31)
    a = rng.uniform(-1, 1, (len(plan["windows"]), n, n, C)).astype(np.float32)
    b_ = np.empty_like(a)
    w0 = 0
    for (H, W) in sizes:
        from simseg_amd import segpost
        offs = segpost.slide_windows(H, W, WIN, STRIDE)
        nx = len({x for _, x in offs}); ny = len(offs) // nx
        assert [W - WIN - x for _, x in offs[:nx]] == [x for _, x in offs[:nx]][::-1]            # mirror-symmetric window columns
        for i in range(ny):
            for j in range(nx):
                b_[w0 + i * nx + j] = a[w0 + i * nx + (nx - 1 - j)][:, ::-1]
        w0 += len(offs)
    cand = torch.tensor([[0, 3, -1, 6, 2], [5, -1, 1, 4, -1]], dtype=torch.int32).cuda()
    sa, sb = torch.from_numpy(a.reshape(-1, n * n, C)).cuda(), torch.from_numpy(np.ascontiguousarray(b_).reshape(-1, n * n, C)).cuda()
    plain = ops.slide_stitch_multi([sa], [plan], [False], plan, cand)
    flipped = ops.slide_stitch_multi([sb], [plan], [True], plan, cand)
    for t0, t1 in zip(plain, flipped):
        p0, p1 = ops.slide_planes(t0, plan, 0) if t0.dim() == 1 else t0[0], ops.slide_planes(t1, plan, 0) if t1.dim() == 1 else t1[0]
        assert torch.equal(p0, p1)
    assert float((ops.slide_planes(plain[0], plan, 1) - ops.slide_planes(flipped[0], plan, 1)).abs().max()) <= ATOL
    assert float((plain[2][1] - flipped[2][1]).abs().max()) <= ATOL


def test_too_many_passes_and_argument_checks():
    from simseg_amd import ops
    case = TR.fusion_case()
    plan = _plans(case["sizes"][:1])[0]
    sim = torch.from_numpy(case["sims"][0]).cuda()
    cand = torch.tensor(case["cand"], dtype=torch.int32).cuda()
    with pytest.raises(RuntimeError, match=r"slide_stitch_multi: 17 passes, 1 <= P <= 16"):
        ops.slide_stitch_multi([sim] * 17, [plan] * 17, [False] * 17, plan, cand)
    ops.slide_stitch_multi([sim] * 16, [plan] * 16, [False, True] * 8, plan, cand)          # the cap itself is accepted
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.slide_stitch_multi([sim.double()], [plan], [False], plan, cand)
    with pytest.raises(ValueError):
        ops.slide_stitch_multi([sim[:-1]], [plan], [False], plan, cand)                     # windows do not match the plan
    with pytest.raises(ValueError):
        ops.slide_stitch_multi([sim, sim], [plan], [False, False], plan, cand)
    three = ops.slide_plan(SIZES[:3], WIN, STRIDE, "cuda")
    sim3 = sim[:len(three["windows"])].contiguous()
    with pytest.raises(ValueError):
        ops.slide_stitch_multi([sim, sim3], [plan, three], [False, False], plan, cand)      # a pass with another number of images
    with pytest.raises(ValueError):
        ops.slide_stitch_multi([sim], [plan], [False], plan, cand[:, :4].contiguous())


# ---- model level ----------------------------------------------------------------------------------------------------------------------
def _build(vit_tag, vit_dim, bert_tag, bert_dim, size, seed, image_k=2):
    """(the helper of tests/test_gpu_miou_gate.py, plus image_k: a 32-pixel window has 4 patches, fewer than the config's top-5 pooling takes)"""
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    argv = [f"transforms.input_size={size}", f"model.image_encoder.tag={vit_tag}", f"model.image_encoder.embedding_dim={vit_dim}",
            "model.image_encoder.pretrained=False", f"model.text_encoder.tag={bert_tag}", f"model.text_encoder.embedding_dim={bert_dim}",
            "model.text_encoder.pretrained=False", f"model.pool.loda.image_k={image_k}"]
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), argv, update_clip_config)
    torch.manual_seed(seed)
    return build_from_cfg(cfg.model.name, cfg, PIPELINE)


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


RAW_SIZES = [(48, 64), (37, 53)]
LABEL_SIZES = [(48, 64), (40, 50)]
TEXT_SEED = 3


def _structured(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(yy / (7.0 + c) + seed) * np.cos(xx / (11.0 - c)) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)


def _model_inputs():
    """The tiny model, two raw images, labels, and a text matrix with two planted classes.  Random class embeddings against a
    random-weight tower give ten near-equal top scores, of which none need clear seg_select's mean + std threshold: no visited slot, and
    nothing for the map comparisons to compare.  So classes 5 and 9 are planted along the mean pooled embedding m of the base windows
    (unit vectors e_w): a window scores <e_w, m / |m|> on class 5, at least 0.5 on average unless the windows' embeddings are mutually
    anti-correlated, while the other classes score like random unit vectors in 512 dimensions (standard deviation 0.044).  Two scores far
    above eight small ones clear mean + std of the top ten, for every image and every pass."""
    from simseg_amd import ops, preproc
    model = _build("vit_test_patch16", 128, "bert-test", 128, WIN, seed=5).eval().cuda()
    g = torch.Generator().manual_seed(TEXT_SEED)
    text = torch.nn.functional.normalize(torch.randn(21, 512, generator=g), dim=-1)
    noise = torch.nn.functional.normalize(torch.randn(512, generator=g), dim=-1)
    raws = [torch.from_numpy(_structured(H, W, 50 + i)) for i, (H, W) in enumerate(RAW_SIZES)]
    labels = [torch.randint(0, 21, hw, generator=g, dtype=torch.int64).to(torch.uint8).cuda() for hw in LABEL_SIZES]
    spec = preproc.make_spec("square", WIN, "bilinear", mean=MEAN, std=STD)
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    with torch.no_grad():
        res = preproc.preprocess_extents(raws, RAW_SIZES, spec)
        wins = ops.slide_extract(res["packed"], ops.slide_plan(RAW_SIZES, WIN, STRIDE, "cuda"))
        pooled = model.forward_image_project(model.forward_image_feature(wins)).float().cpu()
    m = torch.nn.functional.normalize(pooled.mean(0), dim=-1)
    text[5] = m
    text[9] = torch.nn.functional.normalize(m + 0.3 * noise, dim=-1)
    return model, text.cuda(), raws, labels, spec, mean, std


def _passes(raws, spec, scales, flip):
    """Per scale one device resize of the raw images to tta_sizes of the base extents (scale 1: the raw size itself)."""
    from simseg_amd import preproc, segpost
    passes, base = [], None
    for s, target in zip(scales, segpost.tta_sizes(RAW_SIZES, scales)):
        res = preproc.preprocess_extents(raws, target, spec)
        assert res["sizes"] == target
        if s == 1.0:
            base = len(passes)
        passes.append((res["packed"], res["sizes"], False))
        if flip:
            passes.append((res["packed"], res["sizes"], True))
    return passes, base


def test_model_single_base_pass_equals_encode_images_sliding(monkeypatch):
    from simseg_amd import segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    model, text, raws, labels, spec, mean, std = _model_inputs()
    memo = _Memo(model)
    _memo_ops(monkeypatch, memo, text)
    passes, base = _passes(raws, spec, [1.0], False)
    with torch.no_grad():
        for crf in (True, False):
            old = segpost.encode_images_sliding(memo, passes[0][0], text, 10, win=WIN, stride=STRIDE, crf=crf, mean=mean, std=std, sizes=passes[0][1])
            n_cached = len(memo.cache)
            new = segpost.encode_images_multiscale(memo, passes, text, 10, win=WIN, stride=STRIDE, crf=crf, mean=mean, std=std, base=base)
            assert len(memo.cache) == n_cached                 # bit-identical windows: every tower call was a cache hit
            assert set(new) == set(old)
            for key in ("cand_idx", "cand_score", "threshold", "scores", "prob", "masks", "minmax"):
                assert new[key].dtype == old[key].dtype and torch.equal(new[key].view(torch.uint8) if new[key].dtype != torch.uint8 else new[key],
                                                                        old[key].view(torch.uint8) if old[key].dtype != torch.uint8 else old[key]), key
            assert new["plan"]["sizes"] == old["plan"]["sizes"] and new["plan"]["out_off"] == old["plan"]["out_off"]
            assert new["num_classes"] == old["num_classes"]
            if crf:
                assert set(new["images_u8"]) == set(old["images_u8"])
                for hw, (bs, u8) in old["images_u8"].items():
                    assert new["images_u8"][hw][0] == bs and torch.equal(new["images_u8"][hw][1], u8)
            else:
                assert new["images_u8"] is None and old["images_u8"] is None
                h_old, h_new = (torch.zeros(3, 21, device="cuda", dtype=torch.int64) for _ in range(2))
                segpost.finish_sliding(old, labels, hist=h_old)
                segpost.finish_sliding(new, labels, hist=h_new)
                assert torch.equal(h_old, h_new) and int(h_new[2].sum()) == sum(l.numel() for l in labels)
    assert int((new["cand_idx"] >= 0).sum()) >= 2


def test_model_multiscale_flip_against_numpy_reference(monkeypatch):
    """Scales (0.5, 1.0, 1.5) with flip = 6 passes: each pass's per-window maps and window scores are captured as the existing ops return
    them and pushed through the NumPy reference; fused scores, candidates, prob and min / max are compared; finish_sliding runs on the
    result with and without the CRF."""
    from oracle import segpost_ref as SR
    from simseg_amd import heads, ops, segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    model, text, raws, labels, spec, mean, std = _model_inputs()
    scales, top = [0.5, 1.0, 1.5], 10
    passes, base = _passes(raws, spec, scales, True)
    assert len(passes) == 6 and base == 2
    seen_sim, seen_sc = [], []
    pts, gemm = heads.patch_text_similarity, ops.gemm

    def rec_sim(p, t, compute_dtype=None):
        seen_sim.append(pts(p, t, compute_dtype=compute_dtype))
        return seen_sim[-1]

    def rec_gemm(a, b, **kw):
        out = gemm(a, b, **kw)
        if b is text and not kw:
            seen_sc.append(out)
        return out
    monkeypatch.setattr(heads, "patch_text_similarity", rec_sim)
    monkeypatch.setattr(ops, "gemm", rec_gemm)
    with torch.no_grad():
        st = segpost.encode_images_multiscale(model, passes, text, top, win=WIN, stride=STRIDE, crf=True, mean=mean, std=std, base=base)
    torch.cuda.synchronize()
    monkeypatch.setattr(heads, "patch_text_similarity", pts)
    monkeypatch.setattr(ops, "gemm", gemm)
    assert len(seen_sim) == len(seen_sc) == 6                     # one tower call per pass (window_batch=None)
    sims = [s.float().cpu().numpy() for s in seen_sim]
    scs = [s.float().cpu().numpy() for s in seen_sc]
    flips = [f for _, _, f in passes]
    offs = [[segpost.slide_windows(h, w, WIN, STRIDE) for h, w in sizes] for _, sizes, _ in passes]
    cand = st["cand_idx"].cpu().numpy()
    minmax = st["minmax"].cpu().numpy()
    scores = st["scores"].cpu().numpy()
    worst = {"scores": 0.0, "minmax": 0.0, "prob": 0.0}
    visited = 0
    for b, (H, W) in enumerate(RAW_SIZES):
        w0 = [sum(len(o) for o in offs[p][:b]) for p in range(6)]
        sc_ref = TR.scores_ref([scs[p][w0[p]:w0[p] + len(offs[p][b])] for p in range(6)])
        worst["scores"] = max(worst["scores"], float(np.abs(scores[b] - sc_ref).max()))
        idx_ref, _, _ = SR.select_candidates(torch.from_numpy(sc_ref.astype(np.float32)), top)
        idx_ref = [int(i) for i in idx_ref]
        if [int(c) for c in cand[b]] != idx_ref:
            order = np.sort(sc_ref)[::-1][:top]
            assert float(np.min(order[:-1] - order[1:])) < 1e-5, (cand[b], idx_ref)          # only near-ties may reorder the candidates
            assert {int(c) for c in cand[b]} == set(idx_ref)
        P_ = ops.slide_planes(st["prob"], st["plan"], b).cpu().numpy()
        for k, c in enumerate(cand[b]):
            if c < 0:
                assert not P_[k].any()
                continue
            visited += 1
            maps = [TR.stitch_ref(sims[p][w0[p]:w0[p] + len(offs[p][b]), :, c], offs[p][b], *passes[p][1][b], WIN) for p in range(6)]
            p_ref, _, (mn, mx), _ = TR.normalise_ref(TR.fuse_ref(maps, flips, H, W)) + (None,)
            worst["minmax"] = max(worst["minmax"], abs(minmax[b, k, 0] - mn), abs(minmax[b, k, 1] - mx))
            worst["prob"] = max(worst["prob"], float(np.abs(P_[k] - p_ref).max()))
    print(f"multiscale + flip vs float64 reference: max |dscores| {worst['scores']:.3e}, |dminmax| {worst['minmax']:.3e}, |dprob| {worst['prob']:.3e}, "
          f"{visited} visited slots")
    assert visited >= 2
    assert worst["scores"] <= ATOL and worst["minmax"] <= ATOL and worst["prob"] <= ATOL
    with torch.no_grad():
        out = segpost.finish_sliding(st, labels, want_pred=True)
        st2 = segpost.encode_images_multiscale(model, passes, text, top, win=WIN, stride=STRIDE, crf=False, base=base, window_batch=3)
        out2 = segpost.finish_sliding(st2, labels, want_pred=True)
    for o in (out, out2):
        assert [tuple(p.shape) for p in o["pred"]] == LABEL_SIZES
        assert int(o["hist"][2].sum()) == sum(l.numel() for l in labels)


# ---- the tool -------------------------------------------------------------------------------------------------------------------------
TOOL = ["--synthetic", "4", "--batch", "2", "--synthetic-raw", "40x56,75x50", "--slide", "32,16", "--no-crf", "transforms.input_size=32",
        "transforms.resize_bicubic.size=32", "transforms.valid_transforms=[resize_bicubic]", "model.image_encoder.tag=vit_test_patch16",
        "model.image_encoder.embedding_dim=128", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.pool.loda.image_k=2"]          # (a 32-pixel window has 4 patches, fewer than the config's top-5 pooling takes)
DIGEST = r"histogram sha256 ([0-9a-f]{64}) mean iou (\S+) \((\w+) preprocessing\)"


def _run_tool(extra, port):
    env = dict(os.environ, PYTHONPATH=REPO, MASTER_PORT=str(port))
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "tools", "seg_eval_device.py"), "--cfg",
           os.path.join(REPO, "configs/clip/simseg.vit-s.yaml")] + TOOL + extra
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "4 samples evaluated" in out.stdout and "final mean iou" in (out.stdout + out.stderr)
    m = re.search(DIGEST, out.stdout)
    assert m, out.stdout[-1000:]
    return m


def test_tool_scales_and_flip():
    """--scales 0.5,1.0,1.5 --flip end to end in a child process of its own: exit 0 and an mIoU line."""
    m = _run_tool(["--device-preproc", "--scales", "0.5,1.0,1.5", "--flip"], 29561)
    assert m.group(3) == "device" and np.isfinite(float(m.group(2)))
    print("tta", m.group(0))


def test_tool_without_the_flags_is_unchanged():
    """Without --scales / --flip the device route still prints the histogram digest and mIoU of the host route (PIL + build_transforms,
    which this feature does not touch): what the tool printed for this command before the feature existed."""
    dev = _run_tool(["--device-preproc"], 29562)
    host = _run_tool([], 29563)
    assert dev.group(3) == "device" and host.group(3) == "host"
    assert dev.group(1, 2) == host.group(1, 2)
