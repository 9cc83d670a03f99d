"""Guards the case table and the yardstick of tests/test_gpu_gemm.py (tests/_gemm_ref.py) on the CPU: the table covers what it claims, the
preconditions of the exact-integer regimes hold for every case, no block of a toleranced case has an all-zero reference, and the block
judge fails the errors that a whole-matrix tolerance forgives."""
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as G

LIN = G.CASES
NL = G.NL_CASES


def test_table_names_every_kernel_layout_and_output_type():
    names = [c.name for c in LIN] + ["nl-" + c.name for c in NL]
    assert len(set(names)) == len(names)
    have = {(c.kernel, c.op, c.layout, c.out) for c in LIN}
    want = {(1, "f32", "NT", "f32")}
    want |= {(1, "h", lay, out) for lay in ("NT", "NN", "TT") for out in ("f32", "h")}
    want |= {(4, "f32", "NT", "f32"), (4, "h", "NT", "f32"), (4, "h", "NT", "h"), (5, "h", "NT", "f32"), (5, "h", "NT", "h")}
    want |= {(k, "h", lay, out) for k in (3, 10) for lay in ("NT", "NN") for out in ("f32", "h")} | {(3, "h", "TT", "f32")}
    assert have == want, (have ^ want)
    # both tilings of kernel 4 in both operand types (dispatch_small: 64x64 from t64 = 192 on)
    for op in ("f32", "h"):
        t64 = {(-(-c.M // 64)) * (-(-c.N // 64)) >= 192 for c in LIN if c.kernel == 4 and c.op == op}
        assert t64 == {True, False}
    # every linear epilogue on every kernel that carries it (kernel 10: pp2_ok's list)
    for k in (1, 4, 5, 3):
        assert {c.epi for c in LIN if c.kernel == k} >= set(G.LIN_ALL), k
    assert {c.epi for c in LIN if c.kernel == 10} == {"plain", "alpha_bias", "drop"}
    assert {c.kernel for c in LIN if c.epi == "splitk"} == {1, 3}
    for k, epis in ((1, {"gelu1", "act34", "act2"}), (4, {"gelu1", "act34", "act2"}), (5, {"gelu1", "act34", "act2"}),
                    (3, {"gelu1", "act34", "act2", "blocked56", "blocked78"}), (10, {"gelu1", "gelu3", "blocked56", "blocked78"})):
        assert {c.epi for c in NL if c.kernel == k} == epis, k
    # K of one slab, NSTAGE - 1, NSTAGE, NSTAGE + 1 slabs on the two ring kernels
    for k, op, slab in ((4, "f32", 32), (4, "h", 64), (5, "h", 64)):
        assert {c.K // slab for c in LIN if c.kernel == k and c.op == op} >= {1, 3, 4, 5}, (k, op)
    # the persistent kernel: more than 256 full tiles, an even and an odd number of K-tiles
    for c in LIN + NL:
        if c.kernel == 10:
            assert c.M % 256 == 0 and c.N % 256 == 0 and (c.M // 256) * (c.N // 256) > 256
    assert {(c.K // 64) % 2 for c in LIN if c.kernel == 10} == {0, 1}


def test_alignment_rules_of_the_c_abi_hold_for_every_case():
    for c in LIN + NL + G.AUTO:
        if c.op == "h":
            assert (c.M if c.layout == "TT" else c.K) % 8 == 0 and (c.N if c.layout != "NT" else c.K) % 8 == 0, c
        else:
            assert c.layout == "NT" and c.out == "f32", c
    for c in LIN + NL:
        if c.kernel == 4:
            assert c.layout == "NT" and c.K * (4 if c.op == "f32" else 2) % 128 == 0, c
        if c.kernel == 5:
            assert c.layout == "NT" and c.K % 64 == 0 and c.M >= 128 and c.N >= 128, c
        if c.kernel in (3, 10):
            assert c.K % 64 == 0 and c.K >= 128 and c.M >= 256 and c.N >= 128, c


def test_no_case_exceeds_the_multiply_add_cap():
    over = [c.name for c in LIN + NL if c.M * c.N * c.K > G.MAC_CAP]
    assert over == ["k10-h-NT-oh-11008x1536x768-blocked56", "k10-h-NT-oh-11008x1536x768-blocked78"], over          # (the one shape: see _nl_table)
    assert all(c.M * c.N * c.K <= G.MAC_CAP for c in G.AUTO)
    assert all(g.rows * sum(o * i for o, i in g.problems) <= G.MAC_CAP for g in G.GROUPED)


@pytest.mark.parametrize("case", LIN, ids=lambda c: c.name)
def test_exact_regime_preconditions(case):
    """Every partial sum and every stored value below 2^24 and a multiple of a power of two that keeps it an fp32 number; in the second
    regime K <= 256 and - on the very values the GPU test uses - everything that is rounded to 16 bits is representable in bf16 and fp16."""
    bound, gran = G.exact_bound(case)
    assert case.K <= 4096 and bound < 2 ** 24 and bound / gran < 2 ** 24, (bound, gran)
    small = G.macs(case) <= 2 ** 28
    if G.regime(case) == 2:
        assert case.K <= 256 and small
    if not small:
        return
    d = G.int_inputs(case)
    keep = (torch.rand(case.M, case.N, generator=torch.Generator().manual_seed(1)) < 0.5).double() * 2 if G.flags(case).get("drop") else None
    ref = G.linear_ref(case, d, keep)
    partial = (d["A"].abs().double() @ d["B"].abs().double().T).max().item()          # bounds every partial sum in every order
    assert partial <= (1 if G.regime(case) == 2 else 16) * case.K and ref["C"].abs().max().item() <= bound
    assert bool((ref["C"] / gran == torch.floor(ref["C"] / gran)).all())
    assert G.representable(ref["C"], torch.float32)
    if "colsum" in ref:
        assert ref["colsum"].abs().max().item() <= bound and G.representable(ref["colsum"], torch.float32)
    if G.regime(case) == 2:
        for half in G.HALVES:
            assert G.representable(ref["pre"], half) and G.representable(ref["C"], half), half


@pytest.mark.parametrize("case", [c for c in NL if c.epi != "blocked56" or c.kernel == 3], ids=lambda c: c.name)
def test_no_block_of_a_toleranced_case_has_a_zero_reference(case):
    halves = [None] if case.op == "f32" else (G.HALVES if G.macs(case) <= 2 ** 28 else G.HALVES[:1])
    for half in halves:
        d = G.nl_inputs(case, half)
        pre = G.nl_pre(d, torch.float64)
        refs = [G.gelu(pre), G.dgelu(pre), pre]
        if case.epi == "act2":
            refs.append(pre * G.dgelu(d["aux"].double()))
        for r in refs:
            assert int((G.block_stats(r, 32, 32)[1] == 0).sum()) == 0
        assert int((G.block_stats(refs[0].sum(0)[None], 1, 32)[1] == 0).sum()) == 0
        # the ramp does what it is for: tiles differ in magnitude by about 2^8
        if case.M >= 160 and case.N >= 160:
            m = G.block_stats(pre, 32, 32)[1]
            assert m.max() / m.min() > 2 ** 6


def _toy(dtype):
    c = G.Case(1, "h", "NT", "h", 160, 192, 64, "gelu1", 1, "")
    d = G.nl_inputs(c, dtype)
    pre64, pre32 = G.nl_pre(d, torch.float64), G.nl_pre(d, torch.float32)
    return pre64, pre32


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_judge_fails_what_a_whole_matrix_tolerance_forgives(dtype):
    """The errors of the issue: a tanh-GELU for the erf-GELU (worst error ~1e-3: inside 1e-2 of the matrix scale), ONE 32x32 tile 0.5 % off,
    a wrong small edge tile - each fails the block rule; the same arithmetic with its sums in another order passes."""
    pre64, pre32 = _toy(dtype)
    ref = G.gelu(pre64)
    R = (lambda t: t.to(dtype).float())
    yard = R(G.gelu(pre32))
    other_order = R(G.gelu((pre32.double() * (1 + 2.0 ** -25)).float()))
    assert G.judge2d(other_order, ref, [yard], dtype)["bad"] == []
    assert G.judge2d(yard, ref, [yard], dtype)["bad"] == []
    tanh = R(F.gelu(pre32, approximate="tanh"))
    assert (tanh - ref).abs().max().item() < 1e-2 * ref.abs().max().item()          # what _close(…, 1e-2) accepts
    assert G.judge2d(tanh, ref, [yard], dtype)["bad"] != []
    tile = yard.clone()
    tile[64:96, 32:64] = R(ref[64:96, 32:64].float() * 1.005)
    assert G.judge2d(tile, ref, [yard], dtype)["bad"] == [[2, 1]]
    edge = yard.clone()
    edge[128:160, 128:160] = 0                                                        # the smallest tile of the ramp: 2^-8 of the matrix scale
    assert (edge - ref).abs().max().item() < 1e-2 * ref.abs().max().item()
    assert G.judge2d(edge, ref, [yard], dtype)["bad"] == [[4, 4]]
    assert G.judge2d(yard, ref, [yard], dtype)["zero"] == 0


def test_quant8_is_the_header_formula():
    g = torch.linspace(-0.129, 1.129, 4001, dtype=torch.float64)
    q = torch.round((g + 0.132) * 255 / 1.264)
    assert q.min() >= 0 and q.max() <= 255
    back = G.quant8(g)
    assert (back - (q / (255 / 1.264) - 0.132)).abs().max().item() < 1e-12
    assert (back - g).abs().max().item() <= 0.5 * 1.264 / 255 + 1e-12


def test_blocked_image_index_is_a_permutation():
    idx = G.blocked_index(512, 768)
    assert idx.shape == (512, 768) and torch.equal(idx.flatten().sort().values, torch.arange(512 * 768))


def test_gelu_poly_has_the_documented_fit_error():
    """csrc/common.h: "Fit error (fp32 Horner): CDF 7e-6, GELU 1.3e-5, GELU' 4.4e-4" on |x| <= 3.5 - the emulation that serves as a yardstick
    of the accumulator-layout epilogues has that error and no more; the tanh form it must not be confused with is 30 x further off."""
    x = torch.linspace(-3.5, 3.5, 70001)
    e = (G.gelu_poly(x).double() - G.gelu(x.double())).abs().max().item()
    de = (G.gelu_poly(x, grad=True).double() - G.dgelu(x.double())).abs().max().item()
    assert 3e-6 < e < 2.6e-5 and 1e-4 < de < 4.6e-4, (e, de)
    assert (F.gelu(x, approximate="tanh").double() - G.gelu(x.double())).abs().max().item() > 10 * e
    far = torch.tensor([-9.0, -4.0, 4.0, 9.0])
    assert (G.gelu_poly(far).double() - G.gelu(far.double())).abs().max().item() < 9 * 2.4e-4
