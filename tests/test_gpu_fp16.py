"""The fp16 flavour of the 16-bit kernels - the type of the reference's AMP mode (torch.cuda.amp.autocast() + GradScaler,
simseg/tasks/clip/clip_runner.py:226-230, simseg/core/hooks/optimizer.py:73-82).  The same kernels as bf16 with _Float16 as their type
argument (v_mfma_f32_32x32x16_f16), selected per call by the tensors' dtype.  Kernels against fp64 / fp32 references; the model's
fp16 gradients against its exact-fp32 gradients; the trainer's live loss scaling (scaled backward, unscale, overflow -> skipped step +
back-off, growth, checkpointed state)."""
import os

import numpy as np
import pytest
import torch

from conftest import tt
from test_gpu_model import _build

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))


@pytest.mark.parametrize("kind,M,N,K", [("nt", 4096, 768, 768), ("nn", 1024, 3072, 768), ("tn", 768, 768, 8192), ("nt", 333, 130, 72), ("nt", 25856, 2304, 768)])
def test_gemm_fp16_flavour(kind, M, N, K):
    from simseg_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    a32 = torch.randn((K, M) if kind == "tn" else (M, K), device="cuda", generator=g)
    b32 = torch.randn((K, N) if kind in ("nn", "tn") else (N, K), device="cuda", generator=g) * 0.1
    err = {}
    for hd in (BF16, F16):
        a, b = a32.to(hd), b32.to(hd)
        A = a.double().T if kind == "tn" else a.double()
        B = b.double() if kind in ("nn", "tn") else b.double().T
        want = A @ B
        if kind == "tn":
            out = torch.zeros(M, N, device="cuda")
            ops.gemm(a, b, trans_a=True, trans_b=True, out=out, accumulate=True, splitk=4)
        else:
            out = ops.gemm(a, b, trans_b=(kind == "nn"), out_dtype=torch.float32)
        e32 = float((out.double() - want).abs().max() / want.abs().max())
        assert e32 < 1e-5, (hd, e32)                             # fp32 accumulation of exact 16-bit products
        if kind != "tn":
            o16 = ops.gemm(a, b, trans_b=(kind == "nn"))         # 16-bit output: one rounding of the result
            assert o16.dtype == hd
            err[hd] = float((o16.double() - want).abs().max() / want.abs().max())
    if err:
        assert err[F16] < 1e-3 and err[BF16] < 8e-3 and err[F16] < err[BF16], err      # 11 vs 8 significant bits


def test_fp16_values_beyond_bf16_precision_survive():
    """The two flavours really are different types: 1 + 2^-10 is an fp16 number and not a bf16 one."""
    from simseg_amd import ops
    x = torch.full((256, 64), 1.0 + 2.0 ** -10, device="cuda")
    eye = torch.eye(64, device="cuda")
    for hd, exact in ((F16, True), (BF16, False)):
        h = ops.cast(x, hd)
        assert h.dtype == hd and torch.equal(h, x.to(hd))
        y = ops.gemm(h, eye.to(hd), out_dtype=torch.float32)
        assert bool((y == 1.0 + 2.0 ** -10).all()) == exact
        assert torch.equal(ops.cast(h, torch.float32), h.float())


@pytest.mark.parametrize("T,drop", [(197, 0.0), (77, 0.1), (300, 0.0)])
def test_attention_fp16_fwd_bwd(T, drop):
    from simseg_amd import ops
    B, H = 3, 4
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv32 = torch.randn(B, T, 3 * H * 64, device="cuda", generator=g)
    do32 = torch.randn(B, T, H * 64, device="cuda", generator=g)
    mask = None
    if T == 77:
        lens = torch.tensor([77, 40, 9], device="cuda")
        mask = (torch.arange(T, device="cuda")[None] < lens[:, None]).long()
    outs = {}
    for hd in (BF16, F16):
        qkv = qkv32.to(hd)
        out, lse = ops.attention_fwd(qkv, H, mask, scale=0.125, save_lse=True, drop_seed=7, drop_p=drop)
        dqkv = ops.attention_bwd(qkv, out, do32.to(hd), lse, H, mask, scale=0.125, drop_seed=7, drop_p=drop)
        assert out.dtype == hd and dqkv.dtype == hd
        outs[hd] = (out.float(), dqkv.float())
    if drop == 0.0:
        q, k, v = [t.view(B, T, H, 64).transpose(1, 2).double() for t in qkv32.to(F16).chunk(3, -1)]
        s = q @ k.transpose(-1, -2) * 0.125
        if mask is not None:
            s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
        want = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, T, H * 64)
        assert float((outs[F16][0].double() - want).abs().max()) < 3e-3
    # both flavours compute the same function of (their rounding of) the same inputs: bf16-level agreement, fp16 the finer one
    valid = slice(None) if mask is None else None
    for i in range(2):
        a, b = outs[F16][i], outs[BF16][i]
        if mask is not None:
            keep = mask.bool()[:, :, None].expand_as(a)
            a, b = a[keep], b[keep]
        assert _cos(a, b) > (0.999 if drop == 0.0 else 0.99), (i, _cos(a, b))
    assert torch.isfinite(outs[F16][1]).all()


def test_layernorm_and_rowops_fp16():
    from simseg_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(1000, 768, device="cuda", generator=g) * 3 + 0.5
    w, b = torch.randn(768, device="cuda", generator=g), torch.randn(768, device="cuda", generator=g)
    want = torch.nn.functional.layer_norm(x, (768,), w, b, 1e-6)
    y, _, mean, rstd = ops.layernorm_fwd(x, w, b, 1e-6, out_dtype=F16, save_stats=True)
    assert y.dtype == F16 and float((y.float() - want).abs().max()) < 2e-2
    y32, y16, _, _ = ops.layernorm_fwd(x, w, b, 1e-6, want_bf16_copy=F16)
    assert y16.dtype == F16 and torch.equal(y16, y32.to(F16))
    dy = torch.randn(1000, 768, device="cuda", generator=g)
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (768,), w, b, 1e-6).backward(dy.to(F16).float())
    dg, db = torch.zeros(768, device="cuda"), torch.zeros(768, device="cuda")
    dx32, dx16 = ops.layernorm_bwd(x, mean, rstd, w, dg, db, dy16=dy.to(F16))
    assert dx16.dtype == F16 and float((dx32 - xr.grad).abs().max()) < 1e-3 * float(xr.grad.abs().max()) + 1e-4
    assert torch.equal(dx16, dx32.to(F16))
    s = torch.zeros(768, device="cuda")
    ops.colsum_accum(dy.to(F16), s)
    assert float((s - dy.to(F16).float().sum(0)).abs().max()) < 1e-2


def _halves(r, shape, lo=-4, hi=4):
    """Multiples of 1/2 in [lo, hi]: exact in bf16 and in fp16, and so is every fp32 sum of a few thousand of them, in any order."""
    return torch.from_numpy(r.integers(2 * lo, 2 * hi + 1, shape) * 0.5).float().cuda()


def _ln_bwd_operands(r, rows, D, zero_rows=()):
    """LayerNorm-backward operands on which the kernel's fp32 arithmetic is EXACT, so that neither the order of the column atomics nor a
    contraction to FMA can move a bit: gains +-1 / +-2, xhat and dy multiples of 1/2, rstd a power of two, and the two row sums the kernel
    divides by D settled at sum(dy gamma) = D / 4 (through dy[:, :16], where gamma = 1 and xhat = 0) and sum(dy gamma xhat) = D / 2
    (through xhat[:, 16:48], where dy gamma = 1/2).  x and the saved output y are consistent with xhat: the kernel may take it from
    either.  One 4-channel chunk has |beta| > 4 |gamma|: the 16-bit step form then reads xhat from x there (its `needx` path).
    zero_rows: rows without a gradient (dy = dres = 0 -> dx = 0)."""
    gamma = r.choice([-2.0, -1.0, 1.0, 2.0], D)
    gamma[:48] = 1.0
    beta = r.integers(-2, 3, D).astype(np.float64)
    gamma[64:68], beta[64:68] = 1.0, 8.0
    xh = r.integers(-4, 5, (rows, D)) * 0.5
    dy = r.integers(-4, 5, (rows, D)) * 0.5
    xh[:, :16], dy[:, 16:48] = 0.0, 0.5
    n = np.rint((D / 4 - (dy * gamma).sum(1)) / 0.5).astype(np.int64)[:, None]
    dy[:, :16] += 0.5 * (n // 16 + (np.arange(16) < n % 16))
    m = np.rint((D / 2 - (dy * gamma * xh).sum(1)) / 0.25).astype(np.int64)[:, None]
    xh[:, 16:48] += 0.5 * (m // 32 + (np.arange(32) < m % 32))
    dres = r.integers(-4, 5, (rows, D)) * 0.5
    rs = r.choice([0.25, 0.5, 1.0], rows)[:, None]
    mu = r.integers(-3, 4, rows).astype(np.float64)[:, None]
    s1, s2 = 0.25, 0.5
    for z in zero_rows:
        dy[z], dres[z] = 0.0, 0.0
    live = np.ones((rows, 1))
    live[list(zero_rows)] = 0.0
    assert np.array_equal((dy * gamma).sum(1, keepdims=True), live * D / 4) and np.array_equal((dy * gamma * xh).sum(1, keepdims=True), live * D / 2)
    dx = rs * (dy * gamma - live * s1 - xh * live * s2) + dres
    assert max(np.abs(dy).max(), np.abs(xh * gamma + beta).max(), np.abs(dres).max()) <= 64         # <= 8 significant bits: exact in bf16
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().cuda()      # noqa: E731
    return dict(gamma=f(gamma), beta=f(beta), x=f(xh / rs + mu), y=f(xh * gamma + beta), dy=f(dy), dres=f(dres), mean=f(mu[:, 0]), rstd=f(rs[:, 0]),
                dx=f(dx), dgamma=f((dy * xh).sum(0)), dbeta=f(dy.sum(0)), dxsum=f(dx.sum(0)))


_ROWOPS_RUNS = {}


def _rowops_run(hd):
    """Every entry point of csrc/rowops.hip that picks the 16-bit type per call, on one fixed set of exactly representable values with
    its 16-bit tensors of type `hd` - or, hd = float32, through dtype code 0.  -> (f32, h16, twin): the fp32 / integer outputs by name, the
    16-bit outputs by name, and for some of those the fp32 tensor the same launch (or the same entry's fp32 launch) wrote."""
    if hd in _ROWOPS_RUNS:
        return _ROWOPS_RUNS[hd]
    from simseg_amd import ops
    r = np.random.default_rng(5)
    is16 = hd != torch.float32
    f32, h16, twin = {}, {}, {}
    put = (lambda k, t: h16.__setitem__(k, t)) if is16 else (lambda k, t: f32.__setitem__(k, t))      # an output of the type under test
    for D, rows in ((384, 13), (768, 5)):                    # two rows per wave with a ragged tail; one row per wave
        x, w, b = _halves(r, (rows, D)), _halves(r, (D,)), _halves(r, (D,))
        y, _, f32[f"ln_fwd{D}.mean"], f32[f"ln_fwd{D}.rstd"] = ops.layernorm_fwd(x, w, b, 1e-6, out_dtype=hd, save_stats=True)
        put(f"ln_fwd{D}.y", y)
        o = _ln_bwd_operands(r, rows, D)
        if is16:
            k = f"ln_fwd{D}.copy"                            # fp32 output and its 16-bit copy from one launch
            twin[k], h16[k], f32[k + ".mean"], f32[k + ".rstd"] = ops.layernorm_fwd(x, w, b, 1e-6, want_bf16_copy=hd, save_stats=True)
            k = f"ln_bwd{D}"                                 # the generic backward: dx in both types from one launch
            f32[k + ".dgamma"], f32[k + ".dbeta"], f32[k + ".dxsum"] = (torch.zeros(D, device="cuda") for _ in range(3))
            twin[k], h16[k] = ops.layernorm_bwd(o["x"], o["mean"], o["rstd"], o["gamma"], f32[k + ".dgamma"], f32[k + ".dbeta"], dy16=o["dy"].to(hd),
                                                dres=o["dres"], dxsum=f32[k + ".dxsum"])
            f32[k + ".dx32"] = twin[k]
            for name in ("dgamma", "dbeta", "dxsum"):
                assert torch.equal(f32[f"{k}.{name}"], o[name]), (k, name)
            assert torch.equal(twin[k], o["dx"]), k
    for D, rows, p in ((768, 13, 0.0), (768, 13, 0.1), (320, 13, 0.0), (320, 13, 0.1)):       # FULL and not; 13 rows: four blocks
        # (with dropout the kept values carry the factor 1 / 0.9 and their column sums are no longer exact: rows 4 .. 11 - the second and third
        #  block - then have no gradient, which leaves two non-zero partial sums per column, and a + b does not depend on the order)
        o = _ln_bwd_operands(r, rows, D, zero_rows=range(4, 12) if p else ())
        if not is16:
            continue
        k = f"ln_bwd16.{D}.{p}"
        f32[k + ".dgamma"], f32[k + ".dbeta"], f32[k + ".dxsum"] = (torch.zeros(D, device="cuda") for _ in range(3))
        a16 = dict(dy16=o["dy"].to(hd), dres16=o["dres"].to(hd), y16=o["y"].to(hd), beta=o["beta"])
        _, h16[k] = ops.layernorm_bwd(o["x"], o["mean"], o["rstd"], o["gamma"], f32[k + ".dgamma"], f32[k + ".dbeta"], want_f32=False, want_bf16=hd,
                                      dxsum=f32[k + ".dxsum"], drop_seed=9, drop_p=p, **a16)
        # its fp32-output run: the same entry asked for dx in fp32 too (written before the mask), times the mask the dropout entry writes in fp32
        dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        dx32, _ = ops.layernorm_bwd(o["x"], o["mean"], o["rstd"], o["gamma"], dg, db, want_f32=True, want_bf16=hd, **a16)
        keep = torch.ones(rows * D, device="cuda")
        ops.dropout_apply_(keep, 9, p)
        twin[k] = torch.where(keep.view(rows, D) != 0, dx32 * keep.view(rows, D), torch.zeros_like(dx32))
        assert torch.equal(dx32, o["dx"]) and torch.equal(f32[k + ".dgamma"], o["dgamma"]) and torch.equal(f32[k + ".dbeta"], o["dbeta"]), k
        if not p:
            assert torch.equal(f32[k + ".dxsum"], o["dxsum"]), k
    x = _halves(r, (300, 64))                                # few rows: the grid of 8-row blocks
    f32["colsum"] = ops.colsum_accum(x.to(hd), torch.zeros(64, device="cuda"))
    assert torch.equal(f32["colsum"], x.sum(0))
    put("im2col", ops.vit_im2col(_halves(r, (2, 3, 32, 48)), hd))
    for k, (B, N) in (("pool", (3, 37)), ("pool_sliced", (2, 256))):
        tok, demb = _halves(r, (B, N, 64)), _halves(r, (B, 64))
        mask = torch.from_numpy(r.integers(0, 4, (B, N)) > 0).long().cuda() if k == "pool" else None
        f32[k + ".emb"], f32[k + ".idx"], f32[k + ".norm"] = ops.topk_pool_l2norm_fwd(tok.to(hd), 5, mask)
        put(k + ".dtok", ops.topk_pool_l2norm_bwd(demb, f32[k + ".emb"], f32[k + ".norm"], f32[k + ".idx"], N, hd))
    f32["rnorm"] = ops.row_rnorm(_halves(r, (5, 64)).to(hd))
    g = _halves(r, (1000,)).to(hd)
    ops.dropout_apply_(g, 11, 0.5)
    put("dropout", g)
    x = torch.from_numpy(r.standard_normal(1028)).float().cuda()
    if is16:
        twin["cast"], h16["cast"] = x, ops.cast(x, hd)       # (values that DO round: the cast is the one entry whose job that is)
        f32["cast.back"] = ops.cast(_halves(r, (1028,)).to(hd), torch.float32)
    torch.cuda.synchronize()
    _ROWOPS_RUNS[hd] = (f32, h16, twin)
    return _ROWOPS_RUNS[hd]


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("hd", [BF16, F16], ids=["bf16", "fp16"])
def test_rowops_pick_the_16bit_type_per_call(hd):
    """csrc/rowops.hip is compiled once and chooses __bf16 or _Float16 at eleven launch sites.  Both types run every site on the same
    values, all exactly representable in both (see _halves, _ln_bwd_operands):
      1. what a launch writes in fp32 or int32 - mean, rstd, dx32, dgamma, dbeta, dxsum, column sums, emb, norm, idx, rnorm, the cast back -
         is bit-equal between the bf16 run and the fp16 run (a launch that reads one type as the other is off by orders of magnitude);
      2. each 16-bit output equals the same entry's fp32 output on the same values - dtype code 0, or the fp32 tensor the launch writes next
         to it - rounded once to that type, bit for bit.
    No tolerance anywhere: profiles/rowops_once.txt."""
    f32, h16, twin = _rowops_run(hd)
    of32, oh16, _ = _rowops_run(F16 if hd == BF16 else BF16)
    plain, _, _ = _rowops_run(torch.float32)
    assert set(f32) == set(of32) and set(h16) == set(oh16) and len(h16) == 15
    for k, v in f32.items():
        assert v.dtype in (torch.float32, torch.int32) and torch.equal(_bits(v), _bits(of32[k])), k
    for k, v in h16.items():
        ref = twin[k] if k in twin else plain[k]
        assert v.dtype == hd and ref.dtype == torch.float32 and torch.equal(_bits(v), _bits(ref.to(hd))), k
    assert not torch.equal(_bits(h16["cast"]), _bits(oh16["cast"]))          # (the two runs did differ in type)


def _gemm_case(kernel, layout, out, M, N, K, epi="plain"):
    import _gemm_ref as G
    (c,) = [c for c in G.CASES if (c.kernel, c.op, c.layout, c.out, c.M, c.N, c.K, c.epi) == (kernel, "h", layout, out, M, N, K, epi)]
    return c


def _launch_gemm(site, hd):
    """-> (output, exact result) of one launch of a GEMM launch site in the type hd: a case of the GEMM suite, judged as there (integers)."""
    import _gemm_ref as G
    import test_gpu_gemm as TG
    from simseg_amd import ops
    if site == "grouped":
        grp = G.GROUPED[0]
        bufs, wants = [], []
        for i, (out, inn) in enumerate(grp.problems):
            g = torch.Generator().manual_seed(G.seed_of(f"wg{grp.rows}-{i}"))
            dy, x = G._randint(-4, 4, (grp.rows, out), g).cuda(), G._randint(-4, 4, (grp.rows, inn), g).cuda()
            w0 = G._randint(-16, 16, (out, inn), g).cuda()
            bufs.append((TG.Buf(grp.rows, out, hd, dy.to(hd), False), TG.Buf(grp.rows, inn, hd, x.to(hd), False), TG.Buf(out, inn, torch.float32, w0, False)))
            wants.append((w0.double() + dy.double().T @ x.double()).float().flatten())
        n, ran = TG._group_call(ops, bufs, grp.rows, grp.slices)          # (lib.call raises on a non-zero status)
        assert n == len(grp.problems) and ran == 3
        return torch.cat([dw.t.flatten() for _, _, dw in bufs]), torch.cat(wants)
    case = {"small": _gemm_case(4, "NT", "h", 31, 63, 64), "ring": _gemm_case(5, "NT", "h", 128, 128, 64),
            "pp": _gemm_case(3, "NT", "h", 256, 256, 128), "pp f32": _gemm_case(3, "NT", "f32", 256, 256, 128),
            "pp split-K": _gemm_case(3, "TT", "f32", 1024, 1536, 4096, "splitk"), "pp2": _gemm_case(10, "NT", "h", 11008, 1536, 128)}[site]
    got = TG.run_linear(ops, case, hd, padded=False)["C"]            # (asserts the kernel that ran; lib.call raises on a non-zero status)
    want = G.linear_ref(case, TG._lin_inputs(case))["C"].float().to(got.dtype)
    return got, want


def _launch_attention(site, hd):
    """-> outputs of one forward (+ backward) of an attention launch site in the type hd, on the attention suite's inputs for that shape."""
    import test_gpu_attention as TA
    from simseg_amd import ops
    B, T, H, lens, grads = {"resident + one-kernel": (3, 33, 3, (33, 9, 1), True), "w64": (1, 512, 3, None, False)}[site]
    qkv, dout = TA._inputs(B, T, H, {BF16: "bf16", F16: "f16"}[hd])
    mask = None if lens is None else TA.A.key_mask(lens, T).long().cuda()      # (the same instantiations as TA._dense on these arguments)
    out, lse = ops.attention_fwd(qkv.cuda(), H, mask, scale=0.125, save_lse=True)
    res = [out, lse]
    if grads:
        res.append(ops.attention_bwd(qkv.cuda(), out, dout.cuda(), lse, H, mask, scale=0.125))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("site", ["small", "ring", "pp", "pp f32", "pp split-K", "pp2", "grouped", "resident + one-kernel", "w64"])
def test_launch_sites_reserve_their_lds_per_16bit_type(site):
    """csrc/gemm.hip and csrc/attn.hip are compiled once; their launchers raise a kernel's dynamic-LDS limit on its first launch, behind a
    function-local flag.  A flag shared by the __bf16 and the _Float16 instantiation of a kernel would leave the second type's kernel at the
    default limit: its first launch fails (invalid value).  So every such launcher runs bf16, fp16, bf16 in this process, at the smallest
    shape of the GEMM / attention suite that reaches it (one instantiation per launcher; the GEMM and attention suites run the others in
    both types): every call returns 0 (lib.call raises otherwise); the GEMM outputs - integer
    operands, the split-K and grouped fp32 atomics included - equal the exact result bit for bit, as in test_gpu_gemm.test_exact; the
    attention kernels are deterministic, so the second bf16 run equals the first bit for bit, and the fp16 run is judged by the attention
    suite's float64 rule (tests/_attn_ref.py)."""
    if site in ("resident + one-kernel", "w64"):
        import test_gpu_attention as TA
        from simseg_amd import ops
        first = _launch_attention(site, BF16)
        if site == "w64":
            TA._dense(ops, "w64 fwd (launch sites)", 1, 512, 3, dt="f16", grads=False)
        else:
            TA._dense(ops, "resident+one (launch sites)", 3, 33, 3, (33, 9, 1), dt="f16")
        again = _launch_attention(site, BF16)
        assert len(first) == len(again) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, again))
        return
    runs = [_launch_gemm(site, hd) for hd in (BF16, F16, BF16)]
    for hd, (got, want) in zip((BF16, F16, BF16), runs):
        assert int((got != want).sum()) == 0, (site, hd)
    assert torch.equal(_bits(runs[0][0]), _bits(runs[2][0]))


def test_model_fp16_gradients_vs_exact_fp32(golden, monkeypatch):
    """The drop-in CLIPModel under torch.autocast(dtype=float16): loss and every parameter gradient against the exact-fp32 run of the
    same step (the reference's own gradients are pinned against that mode), next to the bf16 autocast run of the same step.  Bars: loss
    within 2e-3; every gradient cosine >= 0.99 (the bf16 bar of tests/test_gpu_model.py) and within 3 % in norm; and - fp16 carries three
    more bits than bf16 - closer to the fp32 gradients than the bf16 run on average."""
    g = golden("clip_train_ws1")
    batch = {"image": tt(g["r0.image"]).cuda(), "input_ids": tt(g["r0.input_ids"]).cuda(), "attention_mask": tt(g["r0.attention_mask"]).cuda()}
    m = _build(golden).eval()
    monkeypatch.setenv("SIMSEG_AMD_COMPUTE", "fp32")
    loss32 = m(batch)[0]["nce_loss"]
    loss32.backward()
    ref = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    monkeypatch.delenv("SIMSEG_AMD_COMPUTE")
    cos, SCALE = {}, 65536.0
    for hd in (torch.bfloat16, torch.float16):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=hd):
            loss16 = m(batch)[0]["nce_loss"]
        (loss16 * SCALE).backward()                                # the loss scale the reference's GradScaler starts from (fp16 gradients
                                                                   # below 6e-5 are subnormal: at a scale of 1024 the query-weight gradients of this model lose most of their bits)
        l16, l32 = float(loss16.detach()), float(loss32.detach())
        assert abs(l16 - l32) < (2e-3 if hd == torch.float16 else 2e-2) * abs(l32), (hd, l16, l32)
        cos[hd] = {}
        for n, p in m.named_parameters():
            gr = p.grad / SCALE
            assert torch.isfinite(gr).all(), n
            if "key.bias" in n or float(ref[n].abs().max()) < 1e-7:     # (the null space of the loss: pure rounding noise)
                continue
            cos[hd][n] = _cos(gr, ref[n])
            if hd == torch.float16:
                assert cos[hd][n] > 0.99, (n, cos[hd][n])
                assert abs(float(gr.norm() / ref[n].norm()) - 1) < 3e-2, n
    m16, mb = np.mean([1 - c for c in cos[torch.float16].values()]), np.mean([1 - c for c in cos[torch.bfloat16].values()])
    print(f"mean (1 - cosine) to the exact-fp32 gradients: fp16 autocast {m16:.2e} (worst cosine {min(cos[torch.float16].values()):.4f}), "
          f"bf16 autocast {mb:.2e} (worst {min(cos[torch.bfloat16].values()):.4f})")
    assert m16 < mb


def test_trainer_fp16_amp_with_live_gradscaler(golden, tmp_path):
    """The reference's AMP iteration on this engine: fp16 autocast forward, scaler.scale(loss).backward(), scaler.step (unscale, overflow
    check), scaler.update; an overflowing step is skipped and halves the scale; the scale grows after growth_interval clean steps; the
    scaler's state travels in the checkpoint; the 16-bit weight copies the optimizer kernel writes are fp16."""
    from simseg_amd.trainer import Trainer
    g = golden("clip_train_ws1")
    batch = {"image": tt(g["r0.image"]).cuda(), "input_ids": tt(g["r0.input_ids"]).cuda(), "attention_mask": tt(g["r0.attention_mask"]).cuda()}
    m = _build(golden, ["epoch=1", "optim.lr.init=1e-3", "dist.fp16=True"])
    m.eval()
    tr = Trainer(m, m.cfg, steps_per_epoch=40, amp_dtype="fp16")
    assert tr.scaler.is_enabled() and tr.amp_dtype == torch.float16
    tr.scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 14, growth_interval=4)
    losses = [float(tr.train_step(batch)["loss"]) for _ in range(10)]
    assert losses[-1] < losses[0] - 0.05, losses
    assert tr.scaler.get_scale() >= 2.0 ** 15                         # grew at least once over ten clean steps (interval 4)
    p16 = tr.optimizer.state[next(iter(m.parameters()))]["p16"]
    assert p16.dtype == torch.float16
    w = m.image_projection.linear.weight
    assert torch.equal(tr.optimizer.state[w]["p16"], w.detach().to(torch.float16))      # refreshed by the optimizer kernel
    # an overflow: a scale fp16 gradients cannot carry -> inf in the scaled gradients -> the step is skipped, the scale backs off
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    from simseg_amd.optim import GradScaler
    assert isinstance(tr.scaler, torch.amp.GradScaler) and not isinstance(tr.scaler, GradScaler)      # (the ten steps above: torch's own scaler, as the reference constructs it)
    tr.scaler = GradScaler("cuda", init_scale=2.0 ** 40, growth_interval=1000)      # the same scaler with this package's one-kernel overflow check
    step_no = tr.optimizer.steps_taken()
    assert step_no == 10
    tr.train_step(batch)
    assert tr.scaler.get_scale() == 2.0 ** 39
    assert tr.optimizer.steps_taken() == step_no                      # the kernel skipped the update on the device (no host read in scaler.step)
    assert all(torch.equal(before[n], p.detach()) for n, p in m.named_parameters())
    ck = tr.checkpoint()
    assert ck["scaler"]["scale"] == 2.0 ** 39
    m2 = _build(golden, ["epoch=1", "optim.lr.init=1e-3", "dist.fp16=True"])
    tr2 = Trainer(m2, m2.cfg, steps_per_epoch=40, amp_dtype="fp16")
    tr2.load_checkpoint(ck)
    assert tr2.scaler.get_scale() == 2.0 ** 39
    # the resumed trainer's first step overflows at that scale and is skipped; it is also the first step of the optimizer's new launch plan,
    # whose 16-bit weight copies the skipped kernel never writes: the resumed model must still evaluate bit for bit as the one it came from
    n2 = tr2.optimizer.steps_taken()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                                          # a NaN block of the copy buffer's size, freed: the plan's buffer
    nan = torch.full((sum(p.numel() for p in m2.parameters()),), float("nan"), device="cuda", dtype=torch.float16)    # gets it, so an
    torch.cuda.synchronize()                                          # unwritten copy cannot happen to hold matching bytes
    del nan
    tr2.train_step(batch)
    assert tr2.scaler.get_scale() == 2.0 ** 38
    assert tr2.optimizer.steps_taken() == n2
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(m.parameters(), m2.parameters()))
    m2.eval()
    for p in m2.parameters():
        assert torch.equal(tr2.optimizer.state[p]["p16"], p.detach().to(torch.float16))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        e1, e2 = m(batch, embeddings="all"), m2(batch, embeddings="all")
    assert all(torch.equal(a, b) for a, b in zip(e1, e2))
    # no host synchronisation anywhere in the AMP iteration (forward, scaled backward, overflow check, unscale + update / skip, scale update);
    # the scale has come down to where steps are taken again, so this also covers a TAKEN step with either scaler
    for scaler in (GradScaler("cuda", init_scale=2.0 ** 14), torch.amp.GradScaler("cuda", init_scale=2.0 ** 14)):
        tr.scaler = scaler
        tr.train_step(batch)
        torch.cuda.synchronize()
        n0 = tr.optimizer.steps_taken()
        torch.cuda.set_sync_debug_mode("error")
        try:
            tr.train_step(batch)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert tr.optimizer.steps_taken() == n0 + 1
