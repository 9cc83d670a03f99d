"""Patch dropout, host side: the keep count, the numpy statement of the draw (structure, determinism, uniformity), the C interface and its
argument checks, and the switches on ViT and Trainer.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import REPO

TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False"]
SYMBOLS = {"simseg_patch_keep_sample": ["keep", "inv", "B", "N", "K", "seed", "stream"],
           "simseg_vit_im2col_keep": ["image", "keep", "cols", "out_dtype", "B", "H", "W", "K", "stream"],
           "simseg_vit_keep_rows": ["cls", "pos", "keep", "x", "B", "N", "K", "D", "stream"],
           "simseg_vit_keep_pos_grad": ["dx", "dx_dtype", "inv", "dpos", "B", "N", "K", "D", "stream"]}


def test_num_keep():
    from simseg_amd.patchdrop import num_keep
    assert num_keep(196, 0.5) == 98 and num_keep(196, 0.75) == 49 and num_keep(36, 0.99) == 1 and num_keep(196, 0.001) == 195
    assert num_keep(36, 0.5) == 18
    for N in (1, 36, 196, 1024, 4096):
        assert num_keep(N, 0) == N and num_keep(N, 0.0) == N
    for bad in (-0.1, -1e-9, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="0 <= rate < 1"):
            num_keep(196, bad)


@pytest.mark.parametrize("B,N,K", [(1, 1, 1), (3, 36, 9), (5, 196, 98), (2, 196, 196), (2, 1024, 1), (7, 36, 35)])
def test_sample_keep_ref_structure(B, N, K):
    from simseg_amd.patchdrop import sample_keep_ref
    keep, inv = sample_keep_ref(B, N, K, 77)
    assert keep.dtype == np.int32 and inv.dtype == np.int32 and keep.shape == (B, K) and inv.shape == (B, N)
    assert (keep >= 0).all() and (keep < N).all()
    assert (np.diff(keep, axis=1) > 0).all()                                  # ascending, hence distinct
    for b in range(B):
        want = np.full(N, -1, dtype=np.int32)
        want[keep[b]] = np.arange(K)
        assert np.array_equal(inv[b], want)
    assert ((inv >= 0).sum(1) == K).all()


def test_sample_keep_ref_is_a_function_of_seed_image_n_and_k():
    from simseg_amd.patchdrop import sample_keep_ref
    from simseg_amd.pipeline import hash_u32_ref
    a, ai = sample_keep_ref(8, 196, 98, 1234)
    b, bi = sample_keep_ref(8, 196, 98, 1234)
    assert np.array_equal(a, b) and np.array_equal(ai, bi)
    c, _ = sample_keep_ref(8, 196, 98, 1235)
    assert not np.array_equal(a, c)
    assert not any(np.array_equal(a[0], a[i]) for i in range(1, 8))            # every image its own subset
    first, fi = sample_keep_ref(3, 196, 98, 1234)                              # image b does not depend on the batch size
    assert np.array_equal(first, a[:3]) and np.array_equal(fi, ai[:3])
    hi, _ = sample_keep_ref(8, 196, 98, 1234 + (1 << 32))                      # the seed's upper word counts
    hi2, _ = sample_keep_ref(8, 196, 98, 1234 + (5 << 40))
    assert not np.array_equal(a, hi) and not np.array_equal(hi, hi2)
    # the law, spelled out on one image: the K smallest keys, ties (none here) to the lower position
    keys = hash_u32_ref(1234, np.arange(2 * 196, 3 * 196, dtype=np.uint64))
    assert len(set(keys.tolist())) == 196
    assert np.array_equal(np.sort(np.argsort(keys, kind="stable")[:98]), a[2])
    for bad in ((1, 36, 0), (1, 36, 37), (1, 4097, 5), (1 << 20, 2048, 5), (0, 36, 5)):
        with pytest.raises(ValueError, match="patch dropout"):
            sample_keep_ref(*bad, 1)


@pytest.mark.parametrize("K", [98, 49])
@pytest.mark.parametrize("seed", [1234, 2 ** 61 + 12345])
def test_sample_keep_ref_is_uniform(seed, K):
    """A condition on the law, not a measurement of the code: with independent uniform keys every position is kept with p = K / N and a pair
    of positions with K (K - 1) / (N (N - 1)); over B = 4096 images the frequencies stay within 4.5 / 5 binomial standard deviations."""
    from simseg_amd.patchdrop import sample_keep_ref
    B, N = 4096, 196
    _, inv = sample_keep_ref(B, N, K, seed)
    kept = inv >= 0
    p = K / N
    z = np.abs(kept.mean(0) - p) / np.sqrt(p * (1 - p) / B)
    p2 = K * (K - 1) / (N * (N - 1))
    z2 = np.abs((kept[:, :-1] & kept[:, 1:]).mean(0) - p2) / np.sqrt(p2 * (1 - p2) / B)
    print(f"seed {seed} K {K}: worst position {z.max():.2f} sd, worst adjacent pair {z2.max():.2f} sd")
    assert z.max() < 4.5 and z2.max() < 5.0


def test_header_declares_and_library_exports_the_symbols():
    from simseg_amd import build, lib
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name, args in SYMBOLS.items():
        assert [n for _, n in protos[name][1]] == args
        assert hasattr(so, name)
    import glob
    objs = [os.path.basename(o) for o in glob.glob(os.path.join(REPO, "simseg_amd", "build", "patchdrop*.o"))]
    assert not getattr(build, "TWICE", ()) and objs in ([], ["patchdrop.o"])     # the type is a template argument: ONE object (none here when the library was built elsewhere)
    assert os.path.exists(os.path.join(REPO, "simseg_amd/csrc/patchdrop.hip"))


def test_argument_checks_fire_before_any_device_work():
    """Every refusal is made on the host: callable without a GPU.  (Non-null pointers below are never dereferenced: each call fails a check.)"""
    from simseg_amd import lib
    l = lib.load()
    p = 1 << 20             # a non-null, 16-byte aligned stand-in

    def refused(name, *args, msg):
        assert getattr(l, name)(*args) != 0, (name, args)
        err = l.simseg_last_error().decode()
        assert msg in err and name[len("simseg_"):] in err, err

    # the sampler
    refused("simseg_patch_keep_sample", None, p, 2, 36, 9, 1, None, msg="null pointer")
    refused("simseg_patch_keep_sample", p, None, 2, 36, 9, 1, None, msg="null pointer")
    refused("simseg_patch_keep_sample", p, p, 2, 36, 37, 1, None, msg="1 <= K <= N <= 4096")
    refused("simseg_patch_keep_sample", p, p, 2, 36, 0, 1, None, msg="1 <= K <= N <= 4096")
    refused("simseg_patch_keep_sample", p, p, 2, 4097, 9, 1, None, msg="1 <= K <= N <= 4096")
    refused("simseg_patch_keep_sample", p, p, 1 << 20, 2048, 9, 1, None, msg="B * N < 2^31")
    refused("simseg_patch_keep_sample", p, p, 0, 36, 9, 1, None, msg="B >= 1")
    # the gather
    refused("simseg_vit_im2col_keep", None, p, p, 0, 2, 96, 96, 9, None, msg="null pointer")
    refused("simseg_vit_im2col_keep", p, None, p, 0, 2, 96, 96, 9, None, msg="null pointer")
    refused("simseg_vit_im2col_keep", p, p, None, 0, 2, 96, 96, 9, None, msg="null pointer")
    refused("simseg_vit_im2col_keep", p, p, p, 0, 2, 100, 96, 9, None, msg="multiples of the 16x16 patch")
    refused("simseg_vit_im2col_keep", p, p, p, 0, 2, 96, 40, 9, None, msg="multiples of the 16x16 patch")
    refused("simseg_vit_im2col_keep", p, p, p, 0, 2, 96, 96, 37, None, msg="1 <= K <= N <= 4096")
    refused("simseg_vit_im2col_keep", p, p, p, 0, 2, 1024, 1040, 9, None, msg="1 <= K <= N <= 4096")
    refused("simseg_vit_im2col_keep", p, p, p, 0, 1 << 20, 1024, 512, 9, None, msg="B * N < 2^31")
    refused("simseg_vit_im2col_keep", p, p, p, 2, 2, 96, 96, 9, None, msg="out_dtype")
    # the embedding rows
    for i in range(4):
        ptrs = [p] * 4
        ptrs[i] = None
        refused("simseg_vit_keep_rows", *ptrs, 2, 36, 9, 128, None, msg="null pointer")
    refused("simseg_vit_keep_rows", p, p, p, p, 2, 36, 37, 128, None, msg="1 <= K <= N <= 4096")
    refused("simseg_vit_keep_rows", p, p, p, p, 2, 4097, 9, 128, None, msg="1 <= K <= N <= 4096")
    refused("simseg_vit_keep_rows", p, p, p, p, 1 << 20, 2048, 9, 128, None, msg="B * N < 2^31")
    refused("simseg_vit_keep_rows", p, p, p, p, 2, 36, 9, 130, None, msg="multiple of 4")
    # the position gradient
    refused("simseg_vit_keep_pos_grad", None, 0, p, p, 2, 36, 9, 128, None, msg="null pointer")
    refused("simseg_vit_keep_pos_grad", p, 0, None, p, 2, 36, 9, 128, None, msg="null pointer")
    refused("simseg_vit_keep_pos_grad", p, 0, p, None, 2, 36, 9, 128, None, msg="null pointer")
    refused("simseg_vit_keep_pos_grad", p, 0, p, p, 2, 36, 37, 128, None, msg="1 <= K <= N <= 4096")
    refused("simseg_vit_keep_pos_grad", p, 0, p, p, 2, 4097, 9, 128, None, msg="1 <= K <= N <= 4096")
    refused("simseg_vit_keep_pos_grad", p, 0, p, p, 1 << 20, 2048, 9, 128, None, msg="B * N < 2^31")
    refused("simseg_vit_keep_pos_grad", p, 0, p, p, 2, 36, 9, 126, None, msg="multiple of 4")
    refused("simseg_vit_keep_pos_grad", p, 3, p, p, 2, 36, 9, 128, None, msg="dx_dtype")


def test_python_wrappers_refuse_the_host():
    from simseg_amd import ops, patchdrop
    with pytest.raises(RuntimeError, match="MI355X only"):
        patchdrop.sample_keep(2, 36, 9, 1, "cpu")
    with pytest.raises(ValueError, match="patch dropout"):
        patchdrop.sample_keep(2, 36, 37, 1, "cpu")                                # (the shape is checked first)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.vit_im2col_keep(torch.zeros(2, 3, 96, 96), torch.zeros(2, 9, dtype=torch.int32), torch.float32)


def test_vit_switch():
    from simseg_amd.nn import ViT
    m = ViT("vit_test_patch16", img_size=96)
    assert m.patch_drop_rate == 0.0 and m.last_keep is None and m.last_inv is None
    assert ViT("vit_test_patch16", 96, patch_drop_rate=0.25).patch_drop_rate == 0.25
    m.set_patch_drop(0.5)
    assert m.patch_drop_rate == 0.5
    for bad in (-0.5, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match="0 <= rate < 1"):
            m.set_patch_drop(bad)
        with pytest.raises(ValueError, match="0 <= rate < 1"):
            ViT("vit_test_patch16", 96, patch_drop_rate=bad)
    assert m.patch_drop_rate == 0.5                                               # a refused value changes nothing
    m.set_patch_drop(0)
    assert m.patch_drop_rate == 0.0
    assert not any("patch_drop" in k or "last_" in k for k in m.state_dict())     # the state dict is the one of a model without the feature


def _tiny_model(extra=()):
    from simseg.core.config import update_cfg
    from simseg.models import PIPELINE
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    from simseg.utils import build_from_cfg
    cfg = update_cfg(task_cfg_init_fn, os.path.join(REPO, "configs/clip/simseg.vit-s.yaml"), TINY + list(extra), update_clip_config)
    return build_from_cfg(cfg.model.name, cfg, PIPELINE), cfg


def test_trainer_refuses_fewer_kept_tokens_than_loda_pools():
    from simseg_amd import trainer as T
    from simseg_amd.nn import ViT
    model, cfg = _tiny_model()
    vit = next(m for m in model.modules() if isinstance(m, ViT))
    assert cfg.model.pool.name == "loda" and cfg.model.pool.loda.image_k == 5 and vit.patch_embed.num_patches == 36
    with pytest.raises(ValueError, match="image_k"):
        T.Trainer(model, cfg, steps_per_epoch=10, patch_drop_rate=0.9)           # keeps int(3.6) = 3 < 5
    assert vit.patch_drop_rate == 0.0                                             # refused before anything was set
    with pytest.raises(ValueError, match="0 <= rate < 1"):
        T.Trainer(model, cfg, steps_per_epoch=10, patch_drop_rate=1.0)
    assert T.set_patch_drop(model, cfg, 0.86) is vit and vit.patch_drop_rate == 0.86     # keeps int(5.04) = 5: allowed
    T.set_patch_drop(model, cfg, 0.0)
    assert vit.patch_drop_rate == 0.0
    model2, cfg2 = _tiny_model(["model.pool.loda.image_k=2"])
    assert T.set_patch_drop(model2, cfg2, 0.9).patch_drop_rate == 0.9            # 3 kept tokens are enough for top-2
