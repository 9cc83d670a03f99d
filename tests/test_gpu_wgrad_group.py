"""A block's split-K weight gradients as one grouped launch (ops.wgrad_group -> simseg_gemm_wgrad_group): dW_i += dy_i^T . x_i for
several problems over the same rows.  Reference: the product in fp64 on the same 16-bit operands; bound: the split-K bound of
tests/test_gpu_kernels.py (max abs error <= 2e-5 x max |reference|), in bf16 and in fp16."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-5
HALVES = [torch.bfloat16, torch.float16]
OUTS4 = [(256, 256), (768, 256), (1024, 256), (256, 1024)]          # 1 + 3 + 4 + 4 = 12 tiles of 256x256


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _close(got, want, tol, what=""):
    got, want = got.float().cpu(), want.float().cpu()
    scale = want.abs().max().item() + 1e-12
    err = (got - want).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.2e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


_OPERANDS = {}


def _problems(rows, shapes, dtype, seed=0):
    """[(dy, x, fp64 reference)] - made once per (rows, shapes, dtype) and shared, never written."""
    if not isinstance(rows, (list, tuple)):
        rows = [rows] * len(shapes)
    key = (tuple(rows), tuple(shapes), dtype, seed)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(seed)
        made = []
        for r, (o, i) in zip(rows, shapes):
            dy = torch.randn(r, o, generator=g).to(dtype).cuda()
            x = torch.randn(r, i, generator=g).to(dtype).cuda()
            made.append((dy, x, dy.double().T @ x.double()))
        _OPERANDS[key] = made
    return _OPERANDS[key]


def _run(ops, probs, slices, prefill=None):
    outs = [torch.zeros(dy.shape[1], x.shape[1], device="cuda") if prefill is None else prefill[i].clone() for i, (dy, x, _) in enumerate(probs)]
    ops.wgrad_group([(dy, x, o) for (dy, x, _), o in zip(probs, outs)], slices=slices)
    return outs


@pytest.mark.parametrize("dtype", HALVES)
def test_four_problems_uneven_slices_and_xcd_remainder(ops, dtype):
    """rows = 3200: 50 K-tiles in 3 slices of 17 / 17 / 16; 12 tiles x 3 = 36 blocks, not a multiple of the 8 XCDs."""
    probs = _problems(3200, OUTS4, dtype)
    outs = _run(ops, probs, 3)
    assert ops.wgrad_group_last() == 4 and ops.gemm_last_variant() == 3
    for (dy, x, ref), o in zip(probs, outs):
        _close(o, ref, TOL, f"grouped dW {tuple(o.shape)} {dtype}")


@pytest.mark.parametrize("dtype", HALVES)
def test_accumulates_into_prefilled_outputs(ops, dtype):
    """out = prefill + product: accumulate semantics, and nothing but the problems' own blocks wrote."""
    probs = _problems(3200, OUTS4, dtype)
    g = torch.Generator().manual_seed(7)
    pre = [(torch.randn(o, i, generator=g) * 50).cuda() for o, i in OUTS4]
    outs = _run(ops, probs, 3, prefill=pre)
    assert ops.wgrad_group_last() == 4
    for (dy, x, ref), o, p in zip(probs, outs, pre):
        _close(o, p.double() + ref, TOL, f"prefilled dW {tuple(o.shape)} {dtype}")


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("shapes", [[(512, 256)], [(256, 512), (768, 256)]], ids=["one", "two"])
@pytest.mark.parametrize("rows,slices", [(3072, 3), (3200, 3), (2048, 1)], ids=["even", "uneven", "unsplit"])
def test_small_groups(ops, dtype, shapes, rows, slices):
    """One and two problems; 48 K-tiles = 3 x 16, 50 = 17 + 17 + 16, and one slice (plain accumulate, no atomics)."""
    probs = _problems(rows, shapes, dtype, seed=3)
    outs = _run(ops, probs, slices)
    assert ops.wgrad_group_last() == len(shapes)
    for (dy, x, ref), o in zip(probs, outs):
        _close(o, ref, TOL, f"dW {tuple(o.shape)} rows {rows} {dtype}")


@pytest.mark.parametrize("dtype", HALVES)
def test_planned_slices(ops, dtype, monkeypatch):
    """slices=None: the planner's count (7 for 12 tiles at 112 K-tiles) is what reaches the library."""
    probs = _problems(7168, OUTS4, dtype, seed=4)
    want = ops.wgrad_group_plan([1, 3, 4, 4], 7168 // 64)
    assert want == 7
    seen = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (seen.append((name, a)), real(name, *a))[1])
    outs = _run(ops, probs, None)
    assert [a[3] for n, a in seen if n == "simseg_gemm_wgrad_group"] == [want]
    assert ops.wgrad_group_last() == 4
    for (dy, x, ref), o in zip(probs, outs):
        _close(o, ref, TOL, f"planned dW {tuple(o.shape)} {dtype}")


def _expect_fallback(ops, probs, what):
    ops.wgrad_group([(dy, x, torch.zeros(dy.shape[1], x.shape[1], device="cuda")) for dy, x, _ in _problems(3200, OUTS4, torch.bfloat16)], slices=3)
    assert ops.wgrad_group_last() == 4                                  # (so that the 0 below is this call's)
    outs = _run(ops, probs, 3)
    assert ops.wgrad_group_last() == 0
    for (dy, x, ref), o in zip(probs, outs):
        _close(o, ref, TOL, f"fallback {what} dW {tuple(o.shape)}")


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("case", ["width384", "rows3210", "rows_differ"])
def test_fallbacks(ops, dtype, case):
    """Not eligible: nothing is launched grouped, the per-problem GEMMs give the result."""
    rows, shapes = {"width384": (3200, [(256, 256), (384, 256)]), "rows3210": (3210, [(256, 256), (512, 256)]),
                    "rows_differ": ([3200, 3264], [(256, 256), (512, 256)])}[case]
    _expect_fallback(ops, _problems(rows, shapes, dtype, seed=5), f"{case} {dtype}")


def test_fallback_fp32_operands(ops):
    _expect_fallback(ops, _problems(3200, [(256, 256), (512, 256)], torch.float32, seed=5), "fp32")


# ---- block level -----------------------------------------------------------------------------------------------
D, H = 256, 4


def _params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, generator=g) * (0.05 if len(s) == 2 else 0.1) + (1.0 if len(s) == 1 and k % 4 == 0 else 0.0)).cuda())
            for k, s in enumerate(shapes)]


def _vit_grads(towers, adt):
    B, T = 8, 128                                                           # 1024 rows
    ps = _params([(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,)], seed=11)
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(12)).cuda().requires_grad_()
    y = towers.ViTBlockFn.apply(x, H, adt, *ps)
    dy = torch.randn(B, T, D, generator=torch.Generator().manual_seed(13)).cuda()
    y.backward(dy)
    return [p.grad for p in ps] + [x.grad]


def _bert_grads(towers, adt):
    B, L = 32, 48
    lens = torch.tensor([24 + (7 * b) % 16 for b in range(B)])           # 1008 real tokens -> 1024 packed rows
    mask = (torch.arange(L)[None] < lens[:, None]).long().cuda()
    plan = towers.ragged_plan(mask)
    assert plan.idx.numel() == 1024 and plan.cu is not None
    ps = _params([(D, D), (D,), (D, D), (D,), (D, D), (D,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,), (D,), (D,)], seed=21)
    x = torch.randn(1024, D, generator=torch.Generator().manual_seed(22)).cuda()
    x[plan.nv:] = 0
    x.requires_grad_()
    y = towers.BertLayerFn.apply(x, mask, H, adt, 0.1, 1234, *ps, plan.idx, plan.inv, plan.cu, plan.nv)
    dy = torch.randn(1024, D, generator=torch.Generator().manual_seed(23)).cuda()
    dy[plan.nv:] = 0
    y.backward(dy)
    return [p.grad for p in ps] + [x.grad]


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("block", ["vit", "bert"])
def test_block_gradients_group_on_vs_off(ops, dtype, block, monkeypatch):
    """Every parameter gradient of a ViT block / a packed BERT layer (dropout on, same seed) with the grouped launch against the per-GEMM
    launches; the grouped path runs once per backward."""
    from simseg_amd import towers
    fn = _vit_grads if block == "vit" else _bert_grads
    monkeypatch.setattr(towers, "_WG_GROUP", False)
    n0 = towers.WGRAD_GROUPS[0]
    want = fn(towers, dtype)
    assert towers.WGRAD_GROUPS[0] == n0
    monkeypatch.setattr(towers, "_WG_GROUP", True)
    got = fn(towers, dtype)
    assert towers.WGRAD_GROUPS[0] == n0 + 1
    assert len(got) == len(want) and all(g is not None for g in want)
    for k, (g, w) in enumerate(zip(got, want)):
        _close(g, w, TOL, f"{block} block gradient {k} {tuple(w.shape)} {dtype}")
