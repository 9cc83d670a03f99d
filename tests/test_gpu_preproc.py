"""Device-side image preprocessing (simseg_amd/preproc.py, csrc/preproc.hip) against Pillow and against the host transform route:
every comparison is exact (bit for bit), from the kernel's bytes to the evaluation histogram."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import REPO

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# (H, W) -> (OH, OW)
CASES = [((375, 500), (512, 512)), ((500, 375), (288, 288)), ((480, 640), (512, 683)), ((1024, 2048), (512, 1024)), ((333, 500), (512, 769)),
         ((64, 48), (224, 224)), ((512, 512), (512, 512)), ((427, 640), (512, 512)), ((2000, 3000), (288, 288))]
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def _raw(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _host(pil, mean=MEAN, std=STD):
    """The host route's tail on a resized PIL image: _to_tensor + normalize."""
    from simseg.transforms import _to_tensor
    return (_to_tensor(pil) - torch.tensor(mean).view(-1, 1, 1)) / torch.tensor(std).view(-1, 1, 1)


def _plan_explicit(sizes_out, filt, device="cuda", crops=None):
    """A plan for explicit (H, W) -> (RH, RW) pairs (the spec route derives RH, RW from a config; the kernel takes any)."""
    from simseg_amd import preproc
    sizes = [s for s, _ in sizes_out]
    orig = preproc.geometry
    geo = {}
    for i, ((H, W), (RH, RW)) in enumerate(sizes_out):
        top, left, OH, OW = crops[i] if crops else (0, 0, RH, RW)
        geo[i] = (RH, RW, top, left, OH, OW)
    it = iter(range(len(sizes)))
    preproc.geometry = lambda spec, H, W: geo[next(it)]
    try:
        return preproc.plan(sizes, preproc.make_spec("square", 1, filt), device)
    finally:
        preproc.geometry = orig


def _run(raws, pl, want_u8=True):
    from simseg_amd import ops, preproc
    lut = preproc.make_lut(MEAN, STD).cuda()
    src = torch.cat([torch.from_numpy(r).reshape(-1) for r in raws]).cuda()
    out, u8 = ops.image_preprocess(src, pl, lut, want_u8=want_u8)
    torch.cuda.synchronize()
    f32 = [out[o:o + 3 * h * w].view(3, h, w).cpu() for o, (h, w) in zip(pl["out_off"], pl["out_sizes"])]
    b8 = [u8[o:o + 3 * h * w].view(h, w, 3).cpu().numpy() for o, (h, w) in zip(pl["out_off"], pl["out_sizes"])] if want_u8 else None
    return f32, b8


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_kernel_vs_pillow_one_ragged_batch(filt):
    """The 9 size cases as ONE ragged batch: uint8 output == Image.resize, fp32 output == the host transform; each image alone gives the
    same bytes (batching invariance)."""
    raws = [_raw(H, W, 10 + i) for i, ((H, W), _) in enumerate(CASES)]
    f32, b8 = _run(raws, _plan_explicit(CASES, filt))
    for i, (raw, (_, (OH, OW))) in enumerate(zip(raws, CASES)):
        pil = Image.fromarray(raw).resize((OW, OH), PIL_FILTER[filt])
        diff = int((np.asarray(pil) != b8[i]).sum())
        print(f"{filt} {raw.shape[:2]} -> {(OH, OW)}: {diff} differing bytes")
        assert np.array_equal(np.asarray(pil), b8[i])
        assert torch.equal(f32[i], _host(pil))
    for i in range(len(CASES)):
        one32, one8 = _run([raws[i]], _plan_explicit([CASES[i]], filt))
        assert np.array_equal(one8[0], b8[i]) and torch.equal(one32[0], f32[i])


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_extreme_ratios(filt):
    cases = [((2000, 3000), (288, 288)), ((64, 48), (512, 512))]
    raws = [_raw(H, W, 30 + i) for i, ((H, W), _) in enumerate(cases)]
    f32, b8 = _run(raws, _plan_explicit(cases, filt))
    for raw, (_, (OH, OW)), got8, got32 in zip(raws, cases, b8, f32):
        pil = Image.fromarray(raw).resize((OW, OH), PIL_FILTER[filt])
        assert np.array_equal(np.asarray(pil), got8)
        assert torch.equal(got32, _host(pil))


def test_centre_crop_through_the_spec():
    """resize_bicubic (short side 256) + center_crop 224 through preprocess(): equals PIL resize + crop + the host tail."""
    from simseg_amd import preproc
    spec = preproc.make_spec("short", 256, "bicubic", crop=224, mean=MEAN, std=STD)
    raws = [_raw(375, 500, 40), _raw(500, 333, 41), _raw(256, 256, 42)]
    res = preproc.preprocess([torch.from_numpy(r) for r in raws], spec, want_u8=True)
    assert isinstance(res["images"], torch.Tensor) and tuple(res["images"].shape) == (3, 3, 224, 224)
    for raw, got32, got8 in zip(raws, res["images"], res["u8"]):
        H, W = raw.shape[:2]
        RH, RW = preproc.resized_size(spec, H, W)
        pil = Image.fromarray(raw).resize((RW, RH), Image.BICUBIC)
        left, top = int(round((RW - 224) / 2.0)), int(round((RH - 224) / 2.0))
        pil = pil.crop((left, top, left + 224, top + 224))
        assert np.array_equal(np.asarray(pil), got8.cpu().numpy())
        assert torch.equal(got32.cpu(), _host(pil))
    with pytest.raises(NotImplementedError):
        preproc.plan([(64, 64)], preproc.make_spec("short", 100, "bicubic", crop=224), "cuda")
    # device-resident raw images take the same route
    res2 = preproc.preprocess([torch.from_numpy(r).cuda() for r in raws], spec)
    assert torch.equal(res2["images"], res["images"])


def test_tables_uploaded_on_one_stream_are_seen_on_another():
    """Axis tables and the look-up table are uploaded once and cached.  Here their copies are queued on stream A BEHIND a long run of
    matrix products, and stream B - which nothing orders behind A - preprocesses images of the same (new) sizes straight away: its
    launch must wait for A's copies (the upload events), or it would read tables that are not there yet."""
    from simseg_amd import preproc
    mean, std = [0.40, 0.41, 0.42], [0.21, 0.22, 0.23]                 # a table no other test uses
    spec = preproc.make_spec("short", 130, "bicubic", mean=mean, std=std)
    sizes = [(97, 141), (143, 89)]                                        # axes no other test uses
    raws_a = [_raw(H, W, 70 + i) for i, (H, W) in enumerate(sizes)]
    raws_b = [_raw(H, W, 80 + i) for i, (H, W) in enumerate(sizes)]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.randn(8192, 8192, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        for _ in range(40):
            big = (big @ big).clamp_(-1, 1)                                # tens of milliseconds of queued work in front of the uploads
        res_a = preproc.preprocess([torch.from_numpy(r) for r in raws_a], spec, want_u8=True)
    with torch.cuda.stream(b):
        res_b = preproc.preprocess([torch.from_numpy(r) for r in raws_b], spec, want_u8=True)
        done_b_first = not a.query()                                       # (informational: A still busy when B was queued)
    b.synchronize()
    got = [(u.cpu().numpy(), x.cpu()) for u, x in zip(res_b["u8"], res_b["images"])]
    torch.cuda.synchronize()
    print("stream A still busy when stream B was queued:", done_b_first)
    for raws, res in ((raws_b, None), (raws_a, res_a)):
        for i, raw in enumerate(raws):
            RH, RW = preproc.resized_size(spec, *raw.shape[:2])
            pil = Image.fromarray(raw).resize((RW, RH), Image.BICUBIC)
            u8, x = got[i] if res is None else (res["u8"][i].cpu().numpy(), res["images"][i].cpu())
            assert np.array_equal(np.asarray(pil), u8)
            assert torch.equal(x, _host(pil, mean, std))


def test_finish_by_label_size_vs_one_image_at_a_time(monkeypatch):
    """A batch whose labels have different sizes: the grouped finish == finish_batch on hand-cut one-image states, summed."""
    from simseg_amd import segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    model, text = _towers(96)
    B = 21                                                                 # == the number of classes: nothing may be cut by coincidence of sizes
    x = torch.randn(B, 3, 96, 96, generator=torch.Generator().manual_seed(6)).cuda()
    g = torch.Generator().manual_seed(7)
    shapes = [(80, 110), (96, 96), (80, 110), (50, 70)]
    labs = [torch.randint(0, 21, shapes[i % 4], generator=g, dtype=torch.int64).to(torch.uint8).cuda() for i in range(B)]
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    with torch.no_grad():
        st = segpost.encode_batch(model, x, text, 10, crf=False, mean=mean, std=std)
        got = torch.zeros(3, 21, device="cuda", dtype=torch.int64)
        segpost._finish_by_label_size(st, labs, got)
        want = torch.zeros_like(got)
        for i in range(B):
            one = {k: (v[i:i + 1].contiguous() if k in ("cand_idx", "cand_score", "threshold", "masks") else v) for k, v in st.items()}
            segpost.finish_batch(one, labs[i][None].contiguous(), hist=want)
    assert st["prob"] is None and st["images_u8"] is None
    assert torch.equal(got, want) and int(got[2].sum()) == sum(l.numel() for l in labs)


def test_bad_tables_raise_before_any_launch():
    """Every corrupted table is refused by the host-side check of the C entry point (nothing is launched on out-of-range offsets)."""
    from simseg_amd import ops, preproc
    raws = [_raw(40, 60, 1), _raw(50, 30, 2)]
    lut = preproc.make_lut(MEAN, STD).cuda()
    src = torch.cat([torch.from_numpy(r).reshape(-1) for r in raws]).cuda()

    def fresh():
        pl = dict(_plan_explicit([((40, 60), (64, 64)), ((50, 30), (32, 48))], "bicubic"))
        pl["img_tab_host"] = pl["img_tab_host"].copy()
        pl["tab_host"] = pl["tab_host"].copy()
        return pl
    good = fresh()
    ops.image_preprocess(src, good, lut)
    torch.cuda.synchronize()
    hoff, voff = int(good["img_tab_host"][0, 8]), int(good["img_tab_host"][0, 10])
    edits = {"source offset": lambda p: p["img_tab_host"].__setitem__((1, 0), 10 ** 9),
             "negative source offset": lambda p: p["img_tab_host"].__setitem__((0, 0), -3),
             "output offset": lambda p: p["img_tab_host"].__setitem__((1, 3), p["out_numel"]),
             "zero OH": lambda p: p["img_tab_host"].__setitem__((0, 4), 0),
             "zero OW": lambda p: p["img_tab_host"].__setitem__((0, 5), 0),
             "crop outside": lambda p: p["img_tab_host"].__setitem__((0, 6), 1),
             "table offset": lambda p: p["img_tab_host"].__setitem__((0, 8), p["tab_host"].size),
             "ksize smaller than n": lambda p: p["img_tab_host"].__setitem__((0, 9), 1),
             "tile start": lambda p: p["img_tab_host"].__setitem__((1, 15), 0),
             "source wider than stated": lambda p: p["img_tab_host"].__setitem__((0, 2), 59),
             "xmin + n > in": lambda p: p["tab_host"].__setitem__(hoff + 2 * 63, 60),
             "negative xmin": lambda p: p["tab_host"].__setitem__(voff, -1),
             "n = 0": lambda p: p["tab_host"].__setitem__(voff + 1, 0)}
    for what, edit in edits.items():
        pl = fresh()
        edit(pl)
        with pytest.raises(RuntimeError, match="image_preprocess"):
            ops.image_preprocess(src, pl, lut)
        print("refused:", what)
    with pytest.raises(ValueError):
        ops.image_preprocess(src[:-1], fresh(), lut)
    torch.cuda.synchronize()


# ---- end to end: the evaluation downstream of the two routes ------------------------------------------------------------------------------
def _cfg(argv):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), list(argv), update_clip_config)


def _structured(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(yy / (7.0 + c) + seed) * np.cos(xx / (11.0 - c)) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)


def _towers(win):
    from test_gpu_miou_gate import _build
    model = _build("vit_test_patch16", 128, "bert-test", 128, win, seed=5).eval().cuda()
    text = torch.nn.functional.normalize(torch.randn(21, 512, generator=torch.Generator().manual_seed(3)), dim=-1).cuda()
    return model, text


def test_encode_finish_device_vs_host(monkeypatch):
    """encode_batch + finish_batch on a batch preprocessed on the device vs on the host: same input bits, same candidates, masks, histogram."""
    from simseg.transforms import build_device_transforms, build_transforms
    from simseg_amd import preproc, segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    cfg = _cfg(["transforms.resize.size=96", "transforms.input_size=96"])
    tf = build_transforms(cfg, "valid")
    host_op, spec = build_device_transforms(cfg, "valid")
    model, text = _towers(96)
    raws = [_structured(H, W, 50 + i) for i, (H, W) in enumerate([(75, 100), (100, 75), (64, 64), (120, 90)])]
    lab = torch.randint(0, 21, (4, 80, 110), generator=torch.Generator().manual_seed(2), dtype=torch.int64).to(torch.uint8).cuda()
    x_host = torch.stack([tf(Image.fromarray(r)) for r in raws]).cuda()
    x_dev = preproc.preprocess([host_op(Image.fromarray(r)) for r in raws], spec)["images"]
    assert torch.equal(x_dev, x_host)
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    outs = []
    with torch.no_grad():
        for x in (x_host, x_dev):
            hist = torch.zeros(3, 21, device="cuda", dtype=torch.int64)
            st = segpost.encode_batch(model, x, text, 10, crf=False, mean=mean, std=std)
            outs.append((segpost.finish_batch(st, lab, hist=hist), hist))
    (a, ha), (b, hb) = outs
    assert torch.equal(a["cand_idx"], b["cand_idx"]) and torch.equal(a["masks"], b["masks"]) and torch.equal(ha, hb)
    assert int(ha[2].sum()) == lab.numel()


def test_sliding_device_vs_host(monkeypatch):
    """encode_images_sliding + finish_sliding on ragged raw sizes under resize_bicubic: the packed buffer the kernel wrote (taken as it
    is) vs the host-transformed list."""
    from simseg.transforms import build_device_transforms, build_transforms
    from simseg_amd import preproc, segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    cfg = _cfg(["transforms.valid_transforms=[resize_bicubic]", "transforms.resize_bicubic.size=96", "transforms.input_size=96"])
    tf = build_transforms(cfg, "valid")
    host_op, spec = build_device_transforms(cfg, "valid")
    model, text = _towers(96)
    sizes = [(75, 100), (100, 75), (64, 64), (75, 100), (60, 131)]
    raws = [_structured(H, W, 60 + i) for i, (H, W) in enumerate(sizes)]
    g = torch.Generator().manual_seed(4)
    labs = [torch.randint(0, 21, (H, W), generator=g, dtype=torch.int64).to(torch.uint8).cuda() for H, W in sizes]
    xs = [tf(Image.fromarray(r)).cuda() for r in raws]
    res = preproc.preprocess([host_op(Image.fromarray(r)) for r in raws], spec)
    assert isinstance(res["images"], list) and res["sizes"] == [tuple(x.shape[1:]) for x in xs]
    for got, want in zip(res["images"], xs):
        assert torch.equal(got, want)
    hh, hd = torch.zeros(3, 21, device="cuda", dtype=torch.int64), torch.zeros(3, 21, device="cuda", dtype=torch.int64)
    with torch.no_grad():
        a = segpost.finish_sliding(segpost.encode_images_sliding(model, xs, text, 10, win=96, stride=48, crf=False, window_batch=5), labs, hist=hh)
        b = segpost.finish_sliding(segpost.encode_images_sliding(model, res["packed"], text, 10, win=96, stride=48, crf=False, window_batch=5,
                                                                 sizes=res["sizes"]), labs, hist=hd)
    assert torch.equal(a["cand_idx"], b["cand_idx"]) and torch.equal(hh, hd)
    for ma, mb in zip(a["masks"], b["masks"]):
        assert torch.equal(ma, mb)
    assert int(hh[2].sum()) == sum(l.numel() for l in labs)
    with pytest.raises(ValueError):
        segpost.encode_images_sliding(model, res["packed"][:-1], text, 10, win=96, stride=48, crf=False, sizes=res["sizes"])


@pytest.mark.parametrize("slide", [None, (96, 48)])
def test_evaluate_sharded_preprocess(slide, monkeypatch):
    """evaluate_sharded(preprocess=) on raw uint8 lists vs the same batches transformed on the host: the same histogram."""
    from simseg.transforms import build_device_transforms, build_transforms
    from simseg_amd import preproc, segpost
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    argv = ["transforms.input_size=96", "transforms.resize.size=96", "transforms.resize_bicubic.size=96"]
    cfg = _cfg(argv + (["transforms.valid_transforms=[resize_bicubic]"] if slide else []))
    tf = build_transforms(cfg, "valid")
    host_op, spec = build_device_transforms(cfg, "valid")
    model, text = _towers(96)
    sizes = [(75, 100), (100, 75), (64, 64)]
    g = torch.Generator().manual_seed(9)
    raw_batches, host_batches = [], []
    for i in range(4):
        sz = [sizes[(i + j) % 3] for j in range(1 + i % 3)]
        raws = [_structured(H, W, 80 + 7 * i + j) for j, (H, W) in enumerate(sz)]
        labs = [torch.randint(0, 21, (H, W), generator=g, dtype=torch.int64).to(torch.uint8) for H, W in sz]
        raw_batches.append(([torch.from_numpy(r) for r in raws], labs))
        xs = [tf(Image.fromarray(r)) for r in raws]
        host_batches.append((xs if slide else torch.stack(xs), labs))
    seen = []

    def pre(images):
        seen.append(torch.cuda.current_stream().cuda_stream)
        return preproc.preprocess(images, spec)
    with torch.no_grad():
        want = segpost.evaluate_sharded(model, host_batches, text, 10, slide=slide, crf=False, device="cuda")
        got = segpost.evaluate_sharded(model, raw_batches, text, 10, slide=slide, crf=False, device="cuda", preprocess=pre)
    torch.cuda.synchronize()
    assert got["images"] == want["images"] == sum(len(l) for _, l in raw_batches)
    assert torch.equal(got["hist"], want["hist"]) and int(got["hist"][2].sum()) == sum(l.numel() for _, ls in raw_batches for l in ls)
    assert len(seen) == 4 and torch.cuda.default_stream().cuda_stream not in seen          # called on the pipeline's encoder streams


TOOL = ["--synthetic", "8", "--batch", "3", "--synthetic-raw", "75x100,100x75,64x64", "transforms.input_size=96", "transforms.resize.size=96",
        "transforms.resize_bicubic.size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128"]


@pytest.mark.parametrize("mode", ["plain", "slide"])
def test_tool_both_routes_same_digest(mode):
    """tools/seg_eval_device.py on seeded raw images, host route vs --device-preproc, each in a subprocess of its own: the same histogram
    digest and the same mIoU."""
    env = dict(os.environ, PYTHONPATH=REPO)
    extra = ["--slide", "96,48", "transforms.valid_transforms=[resize_bicubic]"] if mode == "slide" else []
    lines = []
    for k, route in enumerate(([], ["--device-preproc"])):
        env["MASTER_PORT"] = str(29540 + 2 * k + (mode == "slide"))
        cmd = [sys.executable, os.path.join(REPO, "tools", "seg_eval_device.py"), "--cfg", os.path.join(REPO, "configs/clip/simseg.vit-s.yaml")] + TOOL + extra + route
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "8 samples evaluated" in out.stdout
        m = re.search(r"histogram sha256 ([0-9a-f]{64}) mean iou (\S+) \((\w+) preprocessing\)", out.stdout)
        assert m, out.stdout[-1000:]
        assert m.group(3) == ("device" if route else "host")
        print(mode, m.group(0))
        lines.append((m.group(1), m.group(2)))
    assert lines[0] == lines[1]
