"""The NT-Xent loss and the image self-supervision branch, host side: the float64 statement of tests/_ntxent_ref.py against float64 autograd
of SLIP's torch statement, the top-1 margin of every input block the GPU tests use, the C ABI, the registry / constructor / refusals of
LOSS.NTXent, and the state dict with and without CLIPModel.enable_ssl.  No GPU."""
import ctypes
import os

import pytest
import torch

import _ntxent_ref as N
from conftest import REPO

YAML = os.path.join(REPO, "configs/clip/simseg.vit-s.yaml")
TINY = ["transforms.input_size=96", "model.image_encoder.tag=vit_test_patch16", "model.image_encoder.embedding_dim=128",
        "model.image_encoder.pretrained=False", "model.text_encoder.tag=bert-test", "model.text_encoder.embedding_dim=128",
        "model.text_encoder.pretrained=False"]


def _cfg(argv=()):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, YAML, list(argv), update_clip_config)


def _loss(argv=(), **kw):
    import simseg.models  # noqa: F401
    from simseg.models.criteria.losses.builder import LOSS
    return LOSS.get("NTXent")(_cfg(["loss.name=NTXent"] + list(argv)), 0, **kw)


def _autograd(statement, s32, T, target0):
    s = s32.double().requires_grad_(True)
    t = torch.tensor(T, dtype=torch.float32).double().requires_grad_(True)
    loss = statement(s, t, target0)
    loss.backward()
    return loss.detach(), s.grad, t.grad


def _compare(r, loss, ds, dt, T):
    torch.testing.assert_close(r["total"], loss, rtol=1e-12, atol=2e-9)
    torch.testing.assert_close(r["ds"], ds, rtol=0, atol=3e-9)
    assert bool((r["ds"][~torch.isfinite(r["z"])] == 0).all()), "the own column's gradient is exactly 0"
    inside = N.T_LO <= float(torch.tensor(T, dtype=torch.float32)) <= N.T_HI
    assert inside == (T != 0.7)
    if inside:
        torch.testing.assert_close(r["dt"], dt, rtol=0, atol=6e-8)
    else:
        assert r["dt"].item() == 0.0 and (dt is None or dt.item() == 0.0)


@pytest.mark.parametrize("T", N.SETTINGS)
@pytest.mark.parametrize("family", N.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", [sh for sh in N.SHAPES if sh[1] % sh[0] == 0 and sh[2] % sh[0] == 0])
def test_ntxent_eval_is_autograd_of_slips_statement(N1, N2, target0, family, T):
    """One rank - (2, 2, 0), (4, 4, 0), (300, 300, 0) - and rank 2 of 4, (98, 392, 196): SLIP's four blocks are read off the stacked one."""
    s = N.blocks(family, N1, N2, target0)[0]
    _compare(N.ntxent_eval(s, T, target0), *_autograd(N.slip_torch, s, T, target0), T)


@pytest.mark.parametrize("T", N.SETTINGS)
@pytest.mark.parametrize("family", N.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", N.SHAPES)
def test_ntxent_eval_is_autograd_of_the_masked_cross_entropy(N1, N2, target0, family, T):
    for s in N.blocks(family, N1, N2, target0):
        _compare(N.ntxent_eval(s, T, target0), *_autograd(N.ntxent_torch, s, T, target0), T)


def test_one_other_column_is_exactly_zero():
    for family in N.FAMILIES:
        r = N.ntxent_eval(N.blocks(family, 2, 2, 0)[0], 0.1, 0)
        assert r["total"].item() == 0.0 and not r["ds"].any() and r["dt"].item() == 0.0 and r["acc_a"] == r["acc_b"] == 1.0


@pytest.mark.parametrize("family", N.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", N.SHAPES)
def test_row_blocks_keep_the_top1_margin(N1, N2, target0, family):
    for k, s in enumerate(N.blocks(family, N1, N2, target0)):
        r = N.ntxent_eval(s, 0.1, target0)
        assert N.margin_ok(r["z"]), f"{family} {N1}x{N2}+{target0} block {k}: top-1 margin - pick another seed"
        # every row really holds its self-similarity as its largest entry
        own = s[torch.arange(N1), target0 + torch.arange(N1)]
        assert bool((own >= s.max(1).values).all()) and bool((own - 1).abs().max() < 1e-6)
        if N1 >= 34:
            # (the families are what they are named: measured 0.875 .. 1.0 and 0 .. 0.02)
            assert (r["acc_a"] > 0.8 and r["acc_b"] > 0.8) if family == "aligned" else (r["acc_a"] < 0.1 and r["acc_b"] < 0.1)


@pytest.mark.parametrize("B,P", N.HEAD_SHAPES)
def test_head_blocks_keep_the_top1_margin(B, P):
    a, b, gathered = N.head_embeddings(B, P, N.HEAD_SEEDS[B, P])
    z = torch.cat([a, b]).double()
    assert N.margin_ok(N.ntxent_eval(z @ gathered.double().T, 0.1, 2 * B)["z"]), f"head B={B} P={P} gathered: pick another seed"
    assert N.margin_ok(N.ntxent_eval(z @ z.T, 0.1, 0)["z"]), f"head B={B} P={P} single process: pick another seed"


def test_c_abi_declares_and_exports_ntxent_rows():
    from simseg_amd import lib
    protos = lib.parse_header()
    assert [n for _, n in protos["simseg_ntxent_rows"][1]] == ["sims", "temperature", "row_loss", "row_correct", "row_tdot", "out4", "N1", "N2",
                                                               "target0", "write_grad", "stream"]
    assert protos["simseg_ntxent_rows"][0] is ctypes.c_int
    so = ctypes.CDLL(lib.LIB_PATH)          # (the built library: the suite runs after the build)
    src = open(os.path.join(REPO, "simseg_amd/csrc/loss.hip")).read()
    assert 'extern "C" int simseg_ntxent_rows(' in src and "ntxent_rows_kernel" in src and "ntxent_finalize_kernel" in src
    assert hasattr(so, "simseg_ntxent_rows"), "simseg_ntxent_rows is not exported"


def test_registry_and_temperature_override():
    import simseg.models  # noqa: F401
    from simseg.models.criteria.losses import mml_loss
    from simseg.models.criteria.losses.builder import LOSS
    assert LOSS.has("NTXent") and "NTXent" in mml_loss.__all__
    c = _loss(["loss.temperature.name=constant", "loss.temperature.value=0.05"])
    assert c.temperature.item() == pytest.approx(0.05) and not list(c.parameters()) and not c.state_dict()
    assert c.group is None and c.rank == 0 and not hasattr(c, "both")
    p = _loss(["loss.temperature.name=parameter", "loss.temperature.value=0.05"])
    assert isinstance(p.temperature, torch.nn.Parameter) and p.temperature.dim() == 0 and sorted(p.state_dict()) == ["temperature"]
    # the constructor's keywords override the config, each on its own
    o = _loss(["loss.temperature.name=parameter", "loss.temperature.value=0.05"], temperature=0.1, learnable=False)
    assert o.temperature.item() == pytest.approx(0.1) and not list(o.parameters()) and not o.state_dict()
    q = _loss(["loss.temperature.name=constant"], temperature=0.2, learnable=True)
    assert isinstance(q.temperature, torch.nn.Parameter) and q.temperature.item() == pytest.approx(0.2)
    fresh = _loss(["loss.temperature.name=constant"], learnable=True)
    fresh.load_state_dict(q.state_dict())
    assert fresh.temperature.item() == pytest.approx(0.2)
    with pytest.raises(NotImplementedError, match="schedule"):
        _loss(["loss.temperature.name=schedule"])


def test_the_four_refusals_name_their_rule():
    with pytest.raises(NotImplementedError, match="NTXent: loss.global_reduce=False"):
        _loss(["loss.global_reduce=False"])
    with pytest.raises(ValueError, match="NTXent: loss.smoothing=0.1"):
        _loss(["loss.smoothing=0.1"])
    f = torch.zeros(4, 8)
    with pytest.raises(NotImplementedError, match="NTXent: an ignore_mask is not supported"):
        _loss()(f, f, ignore_mask=torch.zeros(4))
    from simseg.models import PIPELINE
    from simseg.utils import build_from_cfg
    cfg = _cfg(TINY + ["loss.name=NTXent"])
    with pytest.raises(NotImplementedError, match="loss.name=NTXent cannot be a CLIPModel's main loss.*enable_ssl"):
        build_from_cfg(cfg.model.name, cfg, PIPELINE)


def test_enable_ssl_adds_exactly_the_projection_keys():
    from simseg.models import PIPELINE
    from simseg.models.pipelines.clip import CLIPModel
    from simseg.utils import build_from_cfg
    cfg = _cfg(TINY)
    plain = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    keys = list(plain.state_dict())
    # a model without enable_ssl has the state dict it has today: the towers, the two projections and nothing of the branch
    assert not [k for k in keys if "ssl" in k] and not [n for n, _ in plain.named_modules() if "ssl" in n]
    assert {k.split(".")[0] for k in keys} == {"image_encoder", "text_encoder", "image_projection", "text_projection", "loss"}
    import numpy as np
    g = np.load(os.path.join(REPO, "tests/golden/clip_glue.npz"))          # (a state dict recorded long before the branch existed)
    assert set(keys) - {"text_encoder.model.model.embeddings.position_ids"} == {k[3:] for k in g.files if k.startswith("sd.")}
    assert "forward" not in vars(plain) and "_image_embeddings" not in vars(plain)          # the class's own methods run
    m = build_from_cfg(cfg.model.name, cfg, PIPELINE)
    assert list(m.state_dict()) == keys
    assert m.enable_ssl(scale=0.5, hidden_dim=192, out_dim=64, temperature=0.2) is m
    added = [k for k in m.state_dict() if k not in keys]
    assert added == ["ssl_projection.fc1.weight", "ssl_projection.fc1.bias", "ssl_projection.fc2.weight"]
    assert [k for k in m.state_dict() if k not in added] == keys
    assert tuple(m.ssl_projection.fc1.weight.shape) == (192, 128) and tuple(m.ssl_projection.fc2.weight.shape) == (64, 192)
    assert m.ssl_projection.fc2.bias is None and m.ssl_scale == 0.5
    assert m.ssl_loss.temperature.item() == pytest.approx(0.2) and not list(m.ssl_loss.parameters())
    assert vars(m)["forward"].__func__ is CLIPModel._forward_ssl
    with pytest.raises(RuntimeError, match="already on"):
        m.enable_ssl()
    # a state-dict round trip restores the projection
    other = build_from_cfg(cfg.model.name, cfg, PIPELINE).enable_ssl(hidden_dim=192, out_dim=64)
    other.load_state_dict(m.state_dict())
    assert torch.equal(other.ssl_projection.fc2.weight, m.ssl_projection.fc2.weight)
