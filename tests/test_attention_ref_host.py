"""Guards the yardstick of tests/test_gpu_attention.py (tests/_attn_ref.py) on the CPU: the emulation's hand-written backward against
autograd of the float64 reference, the larger-of-two-variants rule applied to the variants themselves, and the count of the blocks that
take the zero-reference path."""
import pytest
import torch

import _attn_ref as A

B, T, H, LENS = 3, 33, 2, (33, 9, 1)


def _inputs(dtype=torch.bfloat16):
    return A.randn16((B, T, 3 * H * 64), 5, 1.2, dtype), A.randn16((B, T, H * 64), 6, 1.0, dtype)


def _keep(p):
    """A fixed random keep mask holding 0 or 1 / (1 - p); None for p = 0."""
    if p == 0.0:
        return None
    g = torch.Generator().manual_seed(7)
    return (torch.rand(B, H, T, T, generator=g) >= p).double() / (1.0 - p)


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("scale", [0.125, 0.2])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_manual_backward_equals_autograd_in_float64(p, scale, variant):
    """With the rounding switched off and everything in float64 the emulation IS the reference: output, log-sum-exp and the hand-written
    dQ / dK / dV agree with autograd to 1e-12 of each tensor's largest magnitude - the only independent check of those formulas."""
    qkv, dout = _inputs()
    keep = _keep(p)
    ref = A.reference(qkv, dout, H, scale, LENS, keep)
    emu = A.emulate(qkv, dout, H, scale, LENS, keep, variant, rnd=None, cdt=torch.float64)
    if p > 0:
        assert (keep == 0).any() and (keep[0] > 0).any()
    for kind in ("out", "lse", "dq", "dk", "dv"):
        err = (emu[kind] - ref[kind]).abs().max().item()
        assert err <= 1e-12 * ref[kind].abs().max().item(), f"{kind} p={p} scale={scale} variant {variant}: {err:.3e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_each_variant_is_within_the_larger_of_two(p, dtype):
    """With the rounding on, each variant judged by the larger-of-two yardstick gives ratios <= 1 on every block, and the blocks of the
    one-key sequence's dq and dk - and no others - take the zero-reference path: 2 * H * tiles of them."""
    qkv, dout = _inputs(dtype)
    keep = _keep(p)
    ref = A.reference(qkv, dout, H, 0.125, LENS, keep)
    yards = [A.emulate(qkv, dout, H, 0.125, LENS, keep, v, rnd=dtype) for v in "AB"]
    valid = torch.ones(B, T, dtype=torch.bool)
    want_zero = A.expected_zero_ref_blocks(LENS, valid, H)
    assert want_zero == 2 * H * 2                                                     # T = 33: two 32-row tiles
    for y in yards:
        res = A.judge_all(y, ref, yards, valid, A.PREC[dtype], ("out", "lse", "dq", "dk", "dv"))
        for kind, r in res.items():
            assert not r["bad"], f"{kind}: {A.describe(r)}"
            assert r["rms"] <= 1.0 and r["max"] <= 1.0, (kind, r["rms"], r["max"])
        assert res["dq"]["zero"] + res["dk"]["zero"] == want_zero and res["dv"]["zero"] == 0
        assert res["out"]["blocks"] == B * H * 2 and res["lse"]["blocks"] == B * H


def test_rule_rejects_a_scale_error_and_a_mask_leak():
    """The rule does resolve what it is meant to: the emulation with scale * 1.01 fails gradient blocks of the full-length sequence, and
    a one-key sequence whose dq carries scale * dv fails the zero-reference bound."""
    qkv, dout = _inputs()
    ref = A.reference(qkv, dout, H, 0.125, LENS)
    yards = [A.emulate(qkv, dout, H, 0.125, LENS, None, v) for v in "AB"]
    valid = torch.ones(B, T, dtype=torch.bool)
    off = A.emulate(qkv, dout, H, 0.125 * 1.01, LENS, None, "A")
    res = A.judge_all(off, ref, yards, valid, 8, ("dq", "dk", "dv"))
    assert any(i[0] == 0 for i in res["dq"]["bad"]) and any(i[0] == 0 for i in res["dk"]["bad"])
    leak = {k: v.clone() for k, v in yards[0].items()}
    leak["dq"][2] = 0.125 * leak["dv"][2]
    res = A.judge_all(leak, ref, yards, valid, 8, ("dq", "dk", "dv"))
    assert res["dq"]["bad"] and all(i[0] == 2 for i in res["dq"]["bad"]) and not res["dk"]["bad"]


def test_one_key_sequence_residue_with_and_without_dropout():
    """Why a counted zero-reference block may pass by the ordinary bounds too (tests/_attn_ref.py): without dropout both emulation variants
    leave an fp32 residue far below 2^-12 of the sequence's largest |dv| in the one-key sequence's dq and dk; with dropout the residue
    is a bf16 rounding of the forward output and lies above it in both variants, so the 2^-12 bound alone cannot be met by any
    backward that takes delta from the rounded output."""
    qkv, dout = _inputs()
    for p, above in ((0.0, False), (0.1, True)):
        keep = _keep(p)
        ref = A.reference(qkv, dout, H, 0.125, LENS, keep)
        assert ref["dq"][2].abs().max() == 0 and ref["dk"][2].abs().max() == 0
        for v in "AB":
            emu = A.emulate(qkv, dout, H, 0.125, LENS, keep, v)
            for h in range(H):
                bound = A.ZERO_REF_BOUND * ref["dv"][2, h].abs().max().item()
                worst = max(emu["dq"][2, h].abs().max().item(), emu["dk"][2, h].abs().max().item())
                assert (worst > bound) == above and (above or worst <= bound / 16), (p, v, h, worst, bound)


def test_ulp_and_block_stats():
    m = torch.tensor([0.0, 1.0, 1.5, 2.0, 42.9])
    assert A.ulp(m, 8).tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -2]
    assert A.ulp(m, 24)[1].item() == 2.0 ** -23
    x = torch.zeros(1, 1, 33, 64, dtype=torch.float64)
    x[0, 0, 32] = 3.0                                                                 # the second tile holds ONE row: its RMS is over 64 values
    valid = torch.ones(1, 33, dtype=torch.bool)
    rms, mx, cnt = A.block_stats(x, valid)
    assert rms.tolist() == [[[0.0, 3.0]]] and mx.tolist() == [[[0.0, 3.0]]] and cnt.tolist() == [[[32 * 64, 64]]]
    valid[0, 32] = False
    rms, mx, cnt = A.block_stats(x, valid)
    assert rms.tolist() == [[[0.0, 0.0]]] and cnt.tolist() == [[[32 * 64, 0]]]
