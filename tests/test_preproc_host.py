"""Host side of the device preprocessing route (simseg_amd/preproc.py, simseg.transforms.build_device_transforms, the raw-image
loader): the numpy statement of Pillow's integer resample against Pillow itself, the spec's geometry against the PIL ops, the look-up
table route against build_transforms, and the loader.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import REPO

CASES = [((375, 500), (512, 512)), ((500, 375), (288, 288)), ((480, 640), (512, 683)), ((1024, 2048), (512, 1024)), ((333, 500), (512, 769)),
         ((64, 48), (224, 224)), ((512, 512), (512, 512)), ((427, 640), (512, 512)), ((2000, 3000), (288, 288))]
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
RAW_SIZES = [(375, 500), (500, 375), (333, 500), (512, 512), (700, 3)]


def _cfg(argv, yaml="configs/clip/simseg.vit-s.yaml"):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, os.path.join(REPO, yaml), list(argv), update_clip_config)


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_resample_ref_equals_pillow(case, filt):
    """Uniform-random bytes (bicubic overshoots on them: the clamp is exercised) on the 9 size cases x 2 filters."""
    from simseg_amd import preproc
    (H, W), (OH, OW) = CASES[case]
    a = np.random.default_rng(case).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a).resize((OW, OH), PIL_FILTER[filt]))
    got = preproc.resample_ref(a, (OH, OW), filt)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if filt == "bicubic" and OH > H and OW > W:          # upscaled noise overshoots: both ends of the clamp are reached
        assert want.min() == 0 and want.max() == 255


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_resample_ref_on_a_gradient(filt):
    from simseg_amd import preproc
    yy, xx = np.mgrid[0:300, 0:420]
    a = np.stack([(yy * 255 // 299), (xx * 255 // 419), ((yy + xx) * 255 // 718)], -1).astype(np.uint8)
    for OH, OW in ((512, 717), (96, 96), (300, 512)):
        assert np.array_equal(preproc.resample_ref(a, (OH, OW), filt), np.asarray(Image.fromarray(a).resize((OW, OH), PIL_FILTER[filt])))


def test_axis_coefficients_rows():
    from simseg_amd import preproc
    for filt, s in preproc.FILTERS.items():
        for n_in, n_out in ((375, 512), (500, 288), (3000, 288), (48, 512), (640, 683), (3, 2), (1, 7), (512, 512)):
            bounds, coeffs = preproc.axis_coefficients(n_in, n_out, filt)
            ksize = coeffs.shape[1]
            if n_in != n_out:
                assert ksize == int(np.ceil(s * max(n_in / n_out, 1.0))) * 2 + 1
            assert bounds.shape == (n_out, 2) and bounds.dtype == np.int32 and coeffs.dtype == np.int32
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ksize).all()
            assert (bounds[:, 0] + bounds[:, 1] <= n_in).all()
            assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds[:, 0] + bounds[:, 1]) >= 0).all()
            for x in range(n_out):
                n = bounds[x, 1]
                assert (coeffs[x, n:] == 0).all()
                assert abs(int(coeffs[x, :n].astype(np.int64).sum()) - (1 << 22)) <= ksize
                assert 255 * int(np.abs(coeffs[x].astype(np.int64)).sum()) + (1 << 21) < (1 << 31)
    assert preproc.axis_coefficients(375, 512, "bicubic")[1] is preproc.axis_coefficients(375, 512, "bicubic")[1]      # cached per key
    with pytest.raises(ValueError):
        preproc.axis_coefficients(10, 20, "lanczos")


@pytest.mark.parametrize("valid", [["resize"], ["resize_bicubic"], ["resize_bicubic", "center_crop"]])
def test_spec_geometry_equals_the_pil_ops(valid):
    from simseg.transforms import build_device_transforms, build_transforms
    from simseg_amd import preproc
    cfg = _cfg([f"transforms.valid_transforms=[{','.join(valid)}]", "transforms.resize.size=96", "transforms.resize_bicubic.size=64",
                "transforms.center_crop.size=48"])
    tf = build_transforms(cfg, "valid")
    host_op, spec = build_device_transforms(cfg, "valid")
    assert spec["filter"] == ("bilinear" if valid == ["resize"] else "bicubic") and (spec["crop"] == 48) == ("center_crop" in valid)
    for H, W in RAW_SIZES:
        pil = Image.fromarray(np.zeros((H, W, 3), np.uint8))
        want = tuple(tf(pil).shape[1:])
        if "center_crop" in valid and min(preproc.resized_size(spec, H, W)) < 48:
            with pytest.raises(NotImplementedError):
                preproc.geometry(spec, H, W)
            continue
        RH, RW, top, left, OH, OW = preproc.geometry(spec, H, W)
        assert (OH, OW) == want, (H, W, valid)
        assert 0 <= top and top + OH <= RH and 0 <= left and left + OW <= RW
        raw = host_op(pil)
        assert raw.dtype == torch.uint8 and tuple(raw.shape) == (H, W, 3)
    pl = preproc.plan([(375, 500), (500, 375), (375, 500)], spec, "cpu")
    assert pl["img_tab_host"].shape == (3, preproc.IMG_COLS) and pl["src_off"] == [0, 375 * 500 * 3, 2 * 375 * 500 * 3]
    assert pl["out_off"][1] == 3 * pl["out_sizes"][0][0] * pl["out_sizes"][0][1] and pl["out_numel"] == sum(3 * h * w for h, w in pl["out_sizes"])
    # an axis is placed in the device's table arena once: a later plan finds it at the same offset, whatever else its batch holds
    again = preproc.plan([(500, 375), (333, 500), (375, 500)], spec, "cpu")
    assert again["tab"] is pl["tab"] and again["tab_host"] is pl["tab_host"]
    assert again["img_tab_host"][2, 8:12].tolist() == pl["img_tab_host"][0, 8:12].tolist()
    assert again["img_tab_host"][0, 8:12].tolist() == pl["img_tab_host"][1, 8:12].tolist()
    hoff, hks, RW = int(pl["img_tab_host"][0, 8]), int(pl["img_tab_host"][0, 9]), int(pl["img_tab_host"][0, 13])
    b, c = preproc.axis_coefficients(500, RW, spec["filter"])
    assert np.array_equal(pl["tab_host"][hoff:hoff + 2 * RW], b.reshape(-1)) and np.array_equal(pl["tab_host"][hoff + 2 * RW:hoff + (2 + hks) * RW], c.reshape(-1))
    assert np.array_equal(pl["tab"].numpy(), pl["tab_host"])


def test_unknown_transforms_raise():
    from simseg.transforms import build_device_transforms
    with pytest.raises(NotImplementedError):
        build_device_transforms(_cfg(["transforms.valid_transforms=[autoaug]"]), "valid")
    with pytest.raises(NotImplementedError):
        build_device_transforms(_cfg(["transforms.valid_transforms=[center_crop]"]), "valid")
    with pytest.raises(NotImplementedError):
        build_device_transforms(_cfg([]), "train")


@pytest.mark.parametrize("setup", [("configs/clip/simseg.vit-s.yaml", []), ("configs/clip/simseg.vit-b.yaml", []),
                                   ("configs/clip/simseg.vit-s.yaml", ["transforms.valid_transforms=[resize_bicubic,center_crop]",
                                                                       "transforms.resize_bicubic.size=256", "transforms.center_crop.size=224"])])
def test_lut_route_equals_build_transforms(setup):
    """LUT[c][resample_ref(raw)] == build_transforms(cfg, 'valid')(pil) exactly, for both shipped configs and a crop override."""
    from simseg.transforms import build_device_transforms, build_transforms
    from simseg_amd import preproc
    cfg = _cfg(setup[1], setup[0])
    tf = build_transforms(cfg, "valid")
    host_op, spec = build_device_transforms(cfg, "valid")
    lut = spec["lut"]
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256)
    assert torch.equal(lut, preproc.make_lut(cfg.transforms.normalize.mean, cfg.transforms.normalize.std))
    rng = np.random.default_rng(5)
    for H, W in ((375, 500), (500, 333), (300, 300)):
        raw = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pil = Image.fromarray(raw)
        want = tf(pil)
        RH, RW, top, left, OH, OW = preproc.geometry(spec, H, W)
        u8 = preproc.resample_ref(host_op(pil).numpy(), (RH, RW), spec["filter"])[top:top + OH, left:left + OW]
        got = torch.stack([lut[c][torch.from_numpy(u8[:, :, c].astype(np.int64))] for c in range(3)])
        assert got.dtype == torch.float32 and torch.equal(got, want)


def test_loader_with_device_preproc(tmp_path):
    """A fake VOC tree: the raw loader yields the decoded bytes and the default loader's labels; the default loader is unchanged."""
    from simseg.datasets.seg.seg_dataset import build_torch_valid_loader
    from simseg.transforms import build_transforms
    root = tmp_path / "VOCdevkit" / "VOC2012"
    for d in ("JPEGImages", "SegmentationClass", "ImageSets/Segmentation"):
        (root / d).mkdir(parents=True)
    names, sizes = ["a", "b", "c"], [(40, 60), (56, 33), (40, 60)]
    (root / "ImageSets/Segmentation/val.txt").write_text("\n".join(names) + "\n")
    rng = np.random.RandomState(0)
    for n, (H, W) in zip(names, sizes):
        Image.fromarray(rng.randint(0, 255, (H, W, 3), dtype=np.uint8)).save(root / "JPEGImages" / f"{n}.jpg")
        Image.fromarray(rng.randint(0, 21, (H, W), dtype=np.uint8)).save(root / "SegmentationClass" / f"{n}.png")
    cfg = _cfg([f"data.data_path={tmp_path}", "data.num_workers=0", "transforms.resize.size=32"])
    default = list(build_torch_valid_loader(cfg, "pascal_voc"))
    tf = build_transforms(cfg, "valid")
    loader = build_torch_valid_loader(cfg, "pascal_voc", device_preproc=True)
    assert loader.preproc_spec["kind"] == "square" and loader.preproc_spec["size"] == 32
    raw = list(loader)
    assert len(raw) == len(default) == 3
    for n, (H, W), (imgs, labs), (dimg, dlab) in zip(names, sizes, raw, default):
        assert isinstance(imgs, list) and isinstance(labs, list) and len(imgs) == len(labs) == 1
        pil = Image.open(root / "JPEGImages" / f"{n}.jpg").convert("RGB")
        assert imgs[0].dtype == torch.uint8 and np.array_equal(imgs[0].numpy(), np.asarray(pil))
        assert torch.equal(labs[0], dlab[0]) and labs[0].dtype == torch.uint8
        assert tuple(dimg.shape) == (1, 3, 32, 32) and torch.equal(dimg[0], tf(pil))            # the default route is what it was
    two = list(build_torch_valid_loader(_cfg([f"data.data_path={tmp_path}", "data.num_workers=0", "data.batch_size_val=2"]), "pascal_voc",
                                        device_preproc=True))
    assert [len(i) for i, _ in two] == [2, 1] and tuple(two[0][0][1].shape) == (56, 33, 3)
