"""The SigLIP pairwise sigmoid loss, host side: the float64 statement of tests/_siglip_ref.py against float64 autograd of the loss as one
writes it in torch, the C ABI, the registry / config / constructor (parameter against buffer, init_bias, the three refusals), and the top-1
margin condition of every input block the GPU tests use.  No GPU."""
import ctypes
import os

import pytest
import torch

import _contrastive_ref as R
import _siglip_ref as S
from conftest import REPO

YAML = os.path.join(REPO, "configs/clip/simseg.vit-s.yaml")


def _cfg(argv=()):
    from simseg.core.config import update_cfg
    from simseg.tasks.clip.config import task_cfg_init_fn, update_clip_config
    return update_cfg(task_cfg_init_fn, YAML, ["loss.name=SigLip"] + list(argv), update_clip_config)


def _loss(argv=(), **kw):
    import simseg.models  # noqa: F401
    from simseg.models.criteria.losses.builder import LOSS
    return LOSS.get("SigLip")(_cfg(argv), 0, **kw)


@pytest.mark.parametrize("T,b", S.SETTINGS)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", [(5, 5, 0), (3, 64, 61), (33, 257, 100)])
def test_siglip_eval_is_autograd_of_the_torch_statement(N1, N2, target0, family, T, b):
    s = S.blocks(family, N1, N2, target0)[0].double().requires_grad_(True)
    t = torch.tensor(T, dtype=torch.float32).double().requires_grad_(True)
    bias = torch.tensor(b, dtype=torch.float32).double().requires_grad_(True)
    loss = S.siglip_torch(s, t, bias, target0)
    loss.backward()
    r = S.siglip_eval(s.detach(), T, b, target0)
    torch.testing.assert_close(r["total"], loss.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r["rows"].sum() / N1, loss.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r["ds"], s.grad, rtol=1e-10, atol=1e-16)
    torch.testing.assert_close(r["db"], bias.grad, rtol=1e-10, atol=1e-16)
    inside = S.T_LO <= t.item() <= S.T_HI
    assert inside == (T in (0.1, 0.02))
    if inside:
        torch.testing.assert_close(r["dt"], t.grad, rtol=1e-10, atol=1e-14)
        assert r["dt"].item() != 0.0
    else:
        assert r["dt"].item() == 0.0 and (t.grad is None or t.grad.item() == 0.0)
    assert r["db"].item() != 0.0


def test_siglip_eval_rows_are_the_pairs_of_one_row():
    """Row i's loss counts row i's pairs only: scoring the rows one by one (each with its own target column) gives the same numbers."""
    N1, N2, target0 = 33, 257, 100
    s = S.blocks("aligned", N1, N2, target0)[0]
    r = S.siglip_eval(s, 0.1, -10.0, target0)
    for i in (0, 7, 32):
        one = S.siglip_torch(s[i:i + 1].double(), torch.tensor(0.1, dtype=torch.float32).double(),
                             torch.tensor(-10.0, dtype=torch.float64), target0 + i)
        torch.testing.assert_close(r["rows"][i], one, rtol=1e-12, atol=0)


def test_c_abi_declares_and_exports_siglip_rows():
    from simseg_amd import build, lib
    protos = lib.parse_header()
    assert [n for _, n in protos["simseg_siglip_rows"][1]] == ["sims", "temperature", "bias", "row_loss", "row_correct", "row_tdot", "row_bdot",
                                                               "out4", "N1", "N2", "target0", "write_grad", "stream"]
    assert protos["simseg_siglip_rows"][0] is ctypes.c_int
    so = ctypes.CDLL(lib.LIB_PATH)          # (the built library: the suite runs after the build)
    import glob
    objs = [os.path.basename(o) for o in glob.glob(os.path.join(REPO, "simseg_amd", "build", "loss*.o"))]
    assert not getattr(build, "TWICE", ()) and objs in ([], ["loss.o"])     # fp32 rows, one entry point: ONE object (none here when the library was built elsewhere)
    assert glob.glob(os.path.join(REPO, "simseg_amd", "csrc", "loss*.hip")) == [os.path.join(REPO, "simseg_amd", "csrc", "loss.hip")]
    src = open(os.path.join(REPO, "simseg_amd/csrc/loss.hip")).read()
    assert 'extern "C" int simseg_siglip_rows(' in src, "simseg_siglip_rows is not defined in loss.hip"
    assert "siglip_rows_kernel" in src and "siglip_finalize_kernel" in src
    assert hasattr(so, "simseg_siglip_rows"), "simseg_siglip_rows is not exported"
    assert not hasattr(so, "simseg_siglip_rows_h16")


def test_registry_and_config():
    import simseg.models  # noqa: F401
    from simseg.models.criteria.losses import mml_loss
    from simseg.models.criteria.losses.builder import LOSS
    assert LOSS.has("SigLip") and "SigLip" in mml_loss.__all__
    cfg = _cfg()
    assert cfg.loss.name == "SigLip" and cfg.loss.global_reduce and float(cfg.loss.smoothing) == 0.0


def test_constructor_parameter_and_constant():
    from simseg.models.criteria.losses.mml_loss import SigLip
    assert SigLip.INIT_BIAS == -10.0
    p = _loss(["loss.temperature.name=parameter", "loss.temperature.value=0.1"])
    assert isinstance(p.temperature, torch.nn.Parameter) and isinstance(p.bias, torch.nn.Parameter)
    assert p.bias.dim() == 0 and p.bias.dtype == torch.float32 and p.bias.item() == -10.0
    assert p.temperature.item() == pytest.approx(0.1) and p.group is None and p.rank == 0 and not hasattr(p, "both")
    assert sorted(dict(p.named_parameters())) == ["bias", "temperature"] and sorted(p.state_dict()) == ["bias", "temperature"]
    c = _loss(["loss.temperature.name=constant"])
    assert not list(c.parameters()) and sorted(dict(c.named_buffers())) == ["bias", "temperature"]
    assert sorted(c.state_dict()) == ["bias"], "under `constant` the bias is a persistent buffer, the temperature a non-persistent one"
    assert c.bias.dim() == 0 and c.bias.item() == -10.0 and not c.bias.requires_grad
    with pytest.raises(NotImplementedError, match="schedule"):
        _loss(["loss.temperature.name=schedule"])


def test_init_bias_is_honoured_and_round_trips():
    for name in ("parameter", "constant"):
        m = _loss([f"loss.temperature.name={name}"], init_bias=-4.5)
        assert m.bias.item() == -4.5
        fresh = _loss([f"loss.temperature.name={name}"])
        assert fresh.bias.item() == -10.0
        fresh.load_state_dict(m.state_dict())
        assert fresh.bias.item() == -4.5


def test_the_three_refusals_name_their_rule():
    with pytest.raises(NotImplementedError, match="SigLip: loss.global_reduce=False"):
        _loss(["loss.global_reduce=False"])
    with pytest.raises(ValueError, match="SigLip: loss.smoothing=0.1"):
        _loss(["loss.smoothing=0.1"])
    m = _loss()
    f = torch.zeros(4, 8)
    with pytest.raises(NotImplementedError, match="SigLip: an ignore_mask is not supported"):
        m(f, f, ignore_mask=torch.zeros(4))


def test_forward_loss_takes_the_two_call_branch():
    """No `both`: CLIPModel.forward_loss calls the module once per direction and names the key after loss.name."""
    from simseg.models.pipelines.clip import CLIPModel
    calls = []

    class Loss:
        def __call__(self, a, b, ignore_mask=None):
            calls.append((a, b))
            return torch.tensor(float(len(calls))), 0

    class M:
        global_reduce, loss = True, Loss()
        cfg = _cfg()

    class Emb:
        is_cuda = True

    img, txt = Emb(), Emb()
    out, _, _ = CLIPModel.forward_loss(M(), img, txt)
    assert calls == [(img, txt), (txt, img)] and list(out) == ["siglip_loss"] and out["siglip_loss"].item() == 1.5


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N1,N2,target0", S.ROW_SHAPES)
def test_row_blocks_keep_the_top1_margin_on_s(N1, N2, target0, family):
    """The kernel's top-1 is taken on s, so the condition is case_ok's margin condition on s - with z = s / T + b the bias would inflate
    max |z| and several of these blocks would fail it."""
    s2 = S.blocks(family, N1, N2, target0)
    for k in range(2):
        assert R.margin_ok(s2[k].double()), f"{family} {N1}x{N2}+{target0} block {k}: top-1 margin on s - pick another seed"
    if (N1, N2) != (1, 1):
        for k in range(2):
            assert "top-1 margin" not in R.case_ok(s2[k], target0)


@pytest.mark.parametrize("N1,P", R.HEAD_SHAPES)
def test_head_blocks_keep_the_top1_margin_on_s(N1, P):
    img, _, gathered = R.head_embeddings(N1, P, R.HEAD_SEEDS[N1, P])
    assert R.margin_ok((img.double() @ gathered.double().T)), f"head N1={N1} P={P}: pick another seed"
