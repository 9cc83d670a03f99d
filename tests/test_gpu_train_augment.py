"""Device-side training augmentation (simseg_amd/augment.py, csrc/augment.hip) against apply_pil, the same parameters applied with Pillow's
own calls: zero differing bytes in the uint8 output and torch.equal on the fp32 output, for every case."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import REPO, tt

pytestmark = pytest.mark.gpu

MEAN, STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]
RAW_SIZES = [(375, 500), (500, 333), (224, 224), (97, 1203), (8, 600)]
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False"]


def _synth(H, W, seed):
    """Structured image: a diagonal gradient, flat blocks, a noisy band and a few saturated pixels."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y) * 127 // max(H + W - 2, 1))], -1).astype(np.int64)
    a[H // 4:H // 2, W // 5:W // 2] = rng.integers(0, 256, 3)                        # a flat block
    band = slice(H // 2, H // 2 + max(1, H // 6))
    a[band] = (a[band] + rng.integers(-40, 41, a[band].shape)) % 256                  # noise
    pts = rng.integers(0, H * W, max(4, H * W // 500))
    a.reshape(-1, 3)[pts[: len(pts) // 2]] = 255
    a.reshape(-1, 3)[pts[len(pts) // 2:]] = 0
    return np.clip(a, 0, 255).astype(np.uint8)


def _edge_images(S):
    """Square S x S images, used with the whole-image box (the resize is then the identity): constant, two levels, and one where
    equalize's step (sum of the histogram without its last non-empty bin, // 255) is 0 in every channel."""
    const = np.full((S, S, 3), 77, np.uint8)
    two = np.full((S, S, 3), 30, np.uint8)
    two[:, S // 3:] = 200
    step0 = np.full((S, S, 3), 180, np.uint8)
    step0[:5, :20] = 12                                                              # 100 pixels below the top level
    return [const, two, step0]


def _raws():
    return [_synth(H, W, 10 + i) for i, (H, W) in enumerate(RAW_SIZES)]


def _boxes(sizes):
    """A fixed box per raw image: the middle 70 % (at least 1 pixel) of each side."""
    out = []
    for H, W in sizes:
        h, w = max(1, int(H * 0.7)), max(1, int(W * 0.7))
        out.append(((H - h) // 2, (W - w) // 2, h, w))
    return out


def _check(raws, params, S, want_u8=True, label=""):
    """Device result == apply_pil for every image: uint8 bytes and fp32 values."""
    from simseg_amd import augment as A, preproc
    lut = preproc.make_lut(MEAN, STD)
    res = A.augment([torch.from_numpy(r) for r in raws], params, lut, S, want_u8=True)
    torch.cuda.synchronize()
    f32, u8 = res["images"].cpu(), res["u8"].cpu().numpy()
    bad = []
    for i, r in enumerate(raws):
        want_f, want_u = A.apply_pil(Image.fromarray(r), params, i, S, MEAN, STD)
        nd = int((u8[i] != want_u).sum())
        if nd or not torch.equal(f32[i], want_f):
            bad.append((i, A.OPS[int(params["op1"][i])] if params["apply1"][i] else "-", A.OPS[int(params["op2"][i])] if params["apply2"][i] else "-",
                        nd, float((f32[i] - want_f).abs().max())))
    print(f"{label} S={S}: {len(raws)} images, {len(bad)} differ", bad[:8])
    assert not bad, f"{label}: images differ (index, op1, op2, differing bytes, max fp32 error): {bad[:8]}"
    return res


def _policy_magnitudes():
    """op -> the distinct magnitudes the policy uses."""
    from simseg_amd import augment as A
    out = {}
    for p1, o1, m1, p2, o2, m2 in A.POLICY:
        for o, m in ((o1, m1), (o2, m2)):
            v = float(A.MAGNITUDES[o][m])
            out.setdefault(o, [])
            if v not in out[o]:
                out[o].append(v)
    return out


@pytest.mark.parametrize("S", [224, 96, 288])
def test_each_op_alone(S):
    """Every op alone at every magnitude the policy uses, both signs for the signed ones, on ragged raw images and the edge images."""
    from simseg_amd import augment as A
    raws = _raws() + _edge_images(S)
    boxes = _boxes(RAW_SIZES) + [(0, 0, S, S)] * 3
    mags = _policy_magnitudes()
    assert sorted(mags) == sorted(A.OPS[1:])
    for op in A.OPS[1:]:
        for m in mags[op]:
            for sign in ((1, -1) if op in A.SIGNED else (1,)):
                _check(raws, A.explicit_params(boxes, op, m, sign), S, label=f"{op} m={m} sign={sign}")
    _check(raws, A.explicit_params(boxes), S, label="crop + resize alone")


def test_all_subpolicies_all_flags():
    """The 25 sub-policies x the four apply-flag combinations, end to end from raw images (signs alternate)."""
    from simseg_amd import augment as A
    raws, rows = _raws(), []
    boxes = _boxes(RAW_SIZES)
    k = 0
    for pi, (p1, o1, m1, p2, o2, m2) in enumerate(A.POLICY):
        for a1 in (0, 1):
            for a2 in (0, 1):
                j = k % len(raws)
                t, l, h, w = boxes[j]
                rows.append({"top": t, "left": l, "h": h, "w": w, "fallback": 0, "policy": pi, "op1": A.OP_CODE[o1],
                             "mag1": float(A.MAGNITUDES[o1][m1]), "apply1": a1, "sign1": 1 if k % 2 else -1, "op2": A.OP_CODE[o2],
                             "mag2": float(A.MAGNITUDES[o2][m2]), "apply2": a2, "sign2": -1 if k % 3 else 1})
                k += 1
    params = A._params(rows)
    _check([raws[i % len(raws)] for i in range(len(rows))], params, 224, label="policies x flags")


def test_sampled_batch_of_512_and_batch_invariance():
    """512 images with sampled parameters: each matches apply_pil, and each gives the same bytes alone as inside the batch."""
    from simseg_amd import augment as A, preproc
    base = _raws()
    raws = [base[i % len(base)] for i in range(512)]
    params = A.sample_params([r.shape[:2] for r in raws], np.random.default_rng(1234))
    res = _check(raws, params, 224, label="sampled 512")
    lut = preproc.make_lut(MEAN, STD)
    dev = [torch.from_numpy(r).cuda() for r in base]
    diff = []
    for i in range(512):
        one = A.augment([dev[i % len(base)]], A.take(params, [i]), lut, 224, want_u8=True)
        if not (torch.equal(one["u8"][0], res["u8"][i]) and torch.equal(one["images"][0], res["images"][i])):
            diff.append(i)
    assert not diff, f"images that differ alone vs in the batch: {diff[:16]}"


def test_host_and_device_resident_inputs_agree():
    from simseg_amd import augment as A, preproc
    raws = _raws()
    params = A.sample_params([r.shape[:2] for r in raws], np.random.default_rng(7))
    lut = preproc.make_lut(MEAN, STD)
    h = A.augment([torch.from_numpy(r) for r in raws], params, lut, 224, want_u8=True)
    d = A.augment([torch.from_numpy(r).cuda() for r in raws], params, lut, 224, want_u8=True)
    assert torch.equal(h["images"], d["images"]) and torch.equal(h["u8"], d["u8"])


def test_bad_tables_and_parameters_are_refused():
    """Corrupted host tables and parameters are refused before anything is launched."""
    from simseg_amd import augment as A, ops, preproc
    raws = _raws()
    params = A.explicit_params(_boxes(RAW_SIZES), "color", 0.4, 1, "rotate", 30.0)
    lut = preproc.make_lut(MEAN, STD).cuda()
    pl = A.plan([r.shape[:2] for r in raws], params, 224, "cuda")
    src = preproc._pack([torch.from_numpy(r) for r in raws], pl, "cuda")
    out, _ = ops.train_augment(src, pl, lut)                                          # the untouched plan runs
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    nan_bits = int(np.array([np.nan], np.float32).view(np.int32)[0])
    for col, val, what in [(A.C_TOP, 10_000, "crop box"), (A.C_CW, 0, "crop box"), (A.C_SRC, 1 << 40, "source offset"),
                           (A.C_HOFF, -5, "axis table"), (A.C_VKS, 0, "axis table"), (A.C_OP1, 99, "code"),
                           (A.C_P1, nan_bits, "blend factor"), (A.C_P2, 1 << 50, "rotate coefficient"), (A.C_H, 0, "source extent")]:
        bad = dict(pl)
        bad["img_tab_host"] = pl["img_tab_host"].copy()
        bad["img_tab_host"][1, col] = val
        with pytest.raises(RuntimeError, match=what):
            ops.train_augment(src, bad, lut)
    bad = dict(pl, size=17)
    with pytest.raises(RuntimeError, match="output size"):
        ops.train_augment(src, bad, lut)
    with pytest.raises(ValueError):                                                    # a box outside its image never reaches the plan
        A.plan([(8, 600)], A.explicit_params([(0, 0, 9, 10)]), 224, "cuda")


def _build_tiny(golden, extra=()):
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), TINY + ["epoch=1", "optim.lr.init=1e-3"] + list(extra),
                     update_clip_config)
    model = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    g = golden("clip_glue")
    sd = {k[3:]: tt(g[k]) for k in g.files if k.startswith("sd.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing)
    return model.cuda()


def test_trainer_step_on_augmented_batch_matches_host_route(golden):
    """The small model (S = its image size, eval() so the step is deterministic): one Trainer.train_step on the device-augmented batch
    gives the same loss, bit for bit, as on the apply_pil batch."""
    from simseg.transforms import build_train_augmentation
    from simseg_amd import augment as A
    from simseg_amd.trainer import Trainer
    g = golden("clip_train_ws1")
    ids, mask = tt(g["r0.input_ids"]).cuda(), tt(g["r0.attention_mask"]).cuda()
    B = ids.shape[0]
    extra = ["transforms.random_resize_crop.size=96"]                                 # S = the model's image size
    m1 = _build_tiny(golden, extra)
    cfg = m1.cfg
    S = cfg.transforms.input_size
    host_op, aug = build_train_augmentation(cfg)
    assert aug.size == S == 96
    raws = [host_op(Image.fromarray(_synth(H, W, 40 + i))) for i, (H, W) in enumerate(RAW_SIZES[:B])]
    res = aug(raws, np.random.default_rng(99))
    mean, std = list(cfg.transforms.normalize.mean), list(cfg.transforms.normalize.std)
    host = torch.stack([A.apply_pil(Image.fromarray(r.numpy()), res["params"], i, S, mean, std)[0] for i, r in enumerate(raws)])
    assert torch.equal(res["images"].cpu(), host)
    losses = []
    for images in (res["images"], host.cuda()):
        m = _build_tiny(golden, extra) if losses else m1
        m.eval()
        tr = Trainer(m, cfg, steps_per_epoch=40)
        losses.append(tr.train_step({"image": images, "input_ids": ids, "attention_mask": mask})["loss"])
    print("losses", [float(v) for v in losses])
    assert torch.equal(torch.as_tensor(losses[0]).cpu(), torch.as_tensor(losses[1]).cpu()), losses
