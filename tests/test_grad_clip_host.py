"""Host-side contract of the fused gradient clipping: the C ABI declares the new entry points (one each for both 16-bit types), the
optimizer has the two methods with the documented signatures, and an unsupported norm type is refused before any device work."""
import inspect
import math
import os
import re

import pytest

from conftest import REPO

NEW = ["simseg_grads_norm_partials", "simseg_grads_norm_finish", "simseg_adamw_multi_step_clip", "simseg_adamw_multi_step_amp_clip"]
# the row kernels' entry points (csrc/rowops.hip), which had an fp16 twin each while that source was compiled twice
ROWOPS = ["simseg_layernorm_fwd", "simseg_layernorm_bwd", "simseg_layernorm_bwd_workspace_bytes", "simseg_colsum_accum", "simseg_vit_im2col",
          "simseg_topk_pool_workspace_bytes", "simseg_topk_pool_l2norm_fwd", "simseg_topk_pool_l2norm_bwd", "simseg_row_rnorm", "simseg_cast",
          "simseg_dropout_apply"]


def test_header_declares_the_entry_points_and_no_second_flavour_renames_them():
    from simseg_amd import lib
    decl = lib.parse_header()
    for name in NEW:
        assert name in decl, name
    # the clipped steps: the argument lists of the plain ones plus the device coefficient, in front of the stream
    for plain, clip in (("simseg_adamw_multi_step", "simseg_adamw_multi_step_clip"), ("simseg_adamw_multi_step_amp", "simseg_adamw_multi_step_amp_clip")):
        a, b = decl[plain][1], decl[clip][1]
        assert b[:-2] == a[:-1] and b[-1] == a[-1] and b[-2][1] == "grad_coef", (plain, clip)
    assert [n for _, n in decl["simseg_grads_norm_partials"][1]] == ["table", "sizes", "chunk_tid", "chunk_off", "n_chunks", "chunk", "norm_type",
                                                                     "partials", "stream"]
    assert [n for _, n in decl["simseg_grads_norm_finish"][1]] == ["partials", "n_partials", "norm_type", "max_norm", "loss_scale", "out2", "stream"]
    # one entry point serves both 16-bit types (the kernel takes the type as a template argument): no renamed second flavour
    from simseg_amd import build
    assert not getattr(build, "TWICE", ()) and not os.path.exists(os.path.join(REPO, "simseg_amd", "csrc", "half_names.h"))
    for f, entries in (("optim.hip", NEW), ("rowops.hip", ROWOPS)):
        src = open(os.path.join(REPO, "simseg_amd", "csrc", f)).read()
        for name in entries:
            assert len(re.findall(rf'^extern "C" (?:int|int64_t) {name}\(', src, flags=re.M)) == 1, name
            assert f"{name}_h16" not in src, name


def test_library_exports_one_entry_for_both_flavours():
    import ctypes
    from simseg_amd import lib
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW + ROWOPS:
        assert hasattr(so, name) and not hasattr(so, name + "_h16"), name


def test_optimizer_methods_and_signatures():
    from simseg_amd.optim import AdamW, GradScaler
    sig = inspect.signature(AdamW.clip_grad_norm_)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("max_norm", inspect.Parameter.empty), ("norm_type", 2.0), ("error_if_nonfinite", False), ("loss_scale", None), ("materialize", False)]
    sig = inspect.signature(AdamW.grad_norm)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("norm_type", 2.0)]
    assert "unclipped" in AdamW.clip_grad_norm_.__doc__.lower() and "gradient exchange" in AdamW.clip_grad_norm_.__doc__
    assert callable(GradScaler.clip_grad_norm_)


@pytest.mark.parametrize("bad", [3, 1.0, 0.5, -math.inf])
def test_other_norm_types_are_refused_on_the_host(bad):
    """No GPU (and no library call) is needed to reach the check."""
    import torch
    from simseg_amd.optim import AdamW, norm_type_code
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = AdamW([p])
    with pytest.raises(NotImplementedError):
        opt.clip_grad_norm_(1.0, norm_type=bad)
    with pytest.raises(NotImplementedError):
        opt.grad_norm(norm_type=bad)
    assert norm_type_code(2) == 2 and norm_type_code(2.0) == 2 and norm_type_code(math.inf) == 0 and norm_type_code("inf") == 0


def test_trainer_switch_is_read_at_import_and_documented():
    from simseg_amd import trainer
    assert isinstance(trainer.FUSED_CLIP, bool)
    assert "SIMSEG_AMD_FUSED_CLIP" in open(os.path.join(REPO, "INTEGRATION.md")).read()
