"""Every GEMM kernel of csrc/gemm.hip per tile (tests/_gemm_ref.py holds the case table, the references and the judge):
  * exact: integer operands whose every partial sum is an fp32 number - the output must equal the integer result bit for bit (a 16-bit
    output: that result rounded once), whatever the summation order;
  * guards: the same calls with every tensor a view into a larger allocation (leading dimensions wider than the extents where the kernel
    accepts that) - nothing outside the written region changes, NaN around the operands never shows, results bit-equal to the packed call;
  * the nonlinear epilogues per 32x32 block against float64, bounds measured by an fp32 yardstick;
  * the kernel every call ran on (simseg_gemm_last_variant), forced and under the automatic size rules.
Every call goes through lib.call("simseg_gemm", ...) so that leading dimensions are free.  Every check prints one `gemm |` row before it
asserts (profiles/gemm_tests.txt is that table).  Every guard region lies inside the torch allocation of the tensor it surrounds."""
import ctypes
import functools

import pytest
import torch

import _gemm_ref as G

pytestmark = pytest.mark.gpu

PRE, PAD = 8, 8                    # guard rows before and behind a view, guard columns behind its extent (8: keeps every 16-byte alignment class)
SENT = {4: 0x7FC0BEEF, 2: 0x7FDE, 1: 0xA5}          # quiet NaNs in fp32, bf16 and fp16; a byte for the 8-bit image
INT = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
HALF_IDS = {torch.bfloat16: "bf16", torch.float16: "fp16", None: "fp32"}


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


class Buf:
    """A [rows, cols] view (leading dimension ld) inside one sentinel-filled allocation with PRE rows before and behind it."""

    def __init__(self, rows, cols, dtype, value=None, padded=True, pad_cols=True):
        self.rows, self.cols = rows, cols
        self.ld = cols + (PAD if padded and pad_cols else 0)
        self.pre = PRE if padded else 0
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.empty((2 * self.pre + rows) * self.ld, dtype=dtype, device="cuda")
        self.bits().fill_(SENT[self.es])
        self.t = self.raw[self.pre * self.ld:(self.pre + rows) * self.ld].view(rows, self.ld)[:, :cols]
        if value is not None:
            self.t.copy_(value)

    def bits(self):
        return self.raw.view(INT[self.es])

    def rows_bits(self):
        return self.bits()[self.pre * self.ld:(self.pre + self.rows) * self.ld].view(self.rows, self.ld)

    def outside_intact(self, written_rows=None):
        """Every element outside [written rows] x [0, cols) still holds the sentinel: guard rows, pad columns, and the rows of the view that
        the call must not touch (the [cls] rows of a row_group output)."""
        return self.outside_touched(written_rows) == 0

    def outside_touched(self, written_rows=None):
        """How many of those elements no longer hold the sentinel."""
        hit = torch.ones(2 * self.pre + self.rows, self.ld, dtype=torch.bool, device="cuda")
        rows = torch.arange(self.rows, device="cuda") if written_rows is None else written_rows
        hit[self.pre + rows, :self.cols] = False
        return int((self.bits().view(-1, self.ld)[hit] != SENT[self.es]).sum())


def vec(n, dtype, value, padded):
    b = Buf(1, n, dtype, value[None] if value is not None else None, padded)
    return b


def t16(x, dtype):
    return x.to(dtype) if dtype is not None else x


def gemm_call(ops, a, b, c, M, N, K, ta, tb, *, alpha=1.0, bias=None, rowscale=None, residual=None, act=0, aux=None, aux_out=None,
              row_group=0, res_mod=0, accumulate=0, splitk=1, drop_p=0.0, colsum=None):
    """simseg_gemm on Buf views; a HIP error raises (lib.call) and fails the test once."""
    from simseg_amd.lib import call, ptr, stream
    P = lambda x: ptr(x.t) if x is not None else None      # noqa: E731
    call("simseg_gemm", P(a), P(b), P(c), M, N, K, a.ld, b.ld, c.ld, ops.dt(a.t), ops.dt(c.t), int(ta), int(tb), float(alpha), P(bias), P(rowscale),
         P(residual), residual.ld if residual is not None else 0, int(act), P(aux), P(aux_out), int(row_group), int(res_mod), int(accumulate),
         int(splitk), G.DROP_SEED, float(drop_p), P(colsum), stream())
    torch.cuda.synchronize()
    return ops.gemm_last_variant()


def operands(d, case, half, padded):
    """A / B of the logical inputs in the case's layout and operand type."""
    A, B = t16(d["A"], half if case.op == "h" else None), t16(d["B"], half if case.op == "h" else None)
    A, B = (A.T if case.layout == "TT" else A), (B.T if case.layout != "NT" else B)
    return Buf(A.shape[0], A.shape[1], A.dtype, A, padded), Buf(B.shape[0], B.shape[1], B.dtype, B, padded)


@functools.lru_cache(maxsize=4)
def keep_mask(M, N):
    """The kernels' dropout mask at p = 0.5 (0 or exactly 2), regenerated with dropout_apply_ on ones: element index row * N + col."""
    from simseg_amd import ops as o
    k = o.dropout_apply_(torch.ones(M * N, device="cuda"), G.DROP_SEED, G.DROP_P).view(M, N)
    assert bool(((k == 0) | (k == 2)).all()) and 0.4 < (k == 0).float().mean().item() < 0.6
    return k


def forced(ops, kernel):
    ops.set_gemm_variant(kernel)


def out_dtype(case, half):
    return torch.float32 if case.out == "f32" else half


@functools.lru_cache(maxsize=2)
def _lin_inputs(case):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in G.int_inputs(case).items()}


def run_linear(ops, case, half, padded):
    """One launch of a linear case.  -> dict(C: the written rows [M, N], colsum, c: the output Buf, cs: the colsum Buf, wrote: output rows)."""
    f, d = G.flags(case), _lin_inputs(case)
    odt = out_dtype(case, half)
    a, b = operands(d, case, half, padded)
    R = G.out_rows(case)
    c = Buf(R, case.N, odt, d.get("c0"), padded)
    bias = vec(case.N, torch.float32, d["bias"], padded) if "bias" in d else None
    rs = vec(case.M, torch.float32, d["rowscale"], padded) if "rowscale" in d else None
    res = Buf(d["residual"].shape[0], case.N, torch.float32, d["residual"], padded) if "residual" in d else None
    aux = Buf(R, case.N, odt, d["aux"], padded) if "aux" in d else None
    cs = vec(case.N, torch.float32, d["cs0"], padded) if "cs0" in d else None
    forced(ops, case.kernel)
    try:
        ran = gemm_call(ops, a, b, c, case.M, case.N, case.K, case.ta, case.tb, alpha=d["alpha"], bias=bias, rowscale=rs, residual=res,
                        act=f.get("act", 0), aux=aux, row_group=G.ROW_GROUP if f.get("row_group") else 0, res_mod=f.get("res_mod", 0),
                        accumulate=f.get("accumulate", 0), splitk=case.splitk, drop_p=G.DROP_P if f.get("drop") else 0.0, colsum=cs)
    finally:
        ops.set_gemm_variant(0)
    assert ran == case.kernel, f"{case.name}: ran on kernel {ran}"
    wrote = G.orow(case, "cuda")
    return {"C": c.t[wrote], "colsum": cs.t[0] if cs is not None else None, "c": c, "cs": cs, "wrote": wrote, "ins": [a, b, bias, rs, res, aux]}


def _halves(case):
    return list(G.HALVES) if case.op == "h" else [None]


LIN_PARAMS = [pytest.param(c, h, id=f"{c.name}-{HALF_IDS[h]}") for c in G.CASES for h in _halves(c)]
NL_PARAMS = [pytest.param(c, h, id=f"{c.name}-{HALF_IDS[h]}") for c in G.NL_CASES if not c.epi.startswith("blocked") for h in _halves(c)]


@pytest.mark.parametrize("case,half", LIN_PARAMS)
def test_exact(ops, case, half):
    """Integer operands: the output equals the float64 result of the same integers bit for bit (16-bit outputs: rounded once, to nearest
    even), the column sums too; the [cls] rows of a row_group output are untouched row by row.  The comparison is on values: the sign of a
    zero is not distinguished (which zero a cancelling sum ends on depends on the summation order, in the kernels and in the reference)."""
    d = _lin_inputs(case)
    keep = keep_mask(case.M, case.N) if G.flags(case).get("drop") else None
    ref = G.linear_ref(case, d, keep)
    got = run_linear(ops, case, half, padded=False)
    odt = out_dtype(case, half)
    want = ref["C"].float().to(odt)
    wrong = int((got["C"] != want).sum())
    cs_wrong = int((got["colsum"] != ref["colsum"].float()).sum()) if got["colsum"] is not None else 0
    print(G.line(f"{case.name} {HALF_IDS[half]}", case.kernel, "exact", "0 tol", f"{wrong + cs_wrong} off", want.numel()))
    assert wrong == 0, f"{case.name}: {wrong} of {want.numel()} elements differ from the exact result; first at {(got['C'] != want).nonzero()[:4].tolist()}"
    assert cs_wrong == 0, f"{case.name}: {cs_wrong} column sums differ from the exact sums"
    if G.flags(case).get("row_group"):
        cls = got["c"].rows_bits()[::G.ROW_GROUP + 1]
        assert cls.shape[0] == -(-case.M // G.ROW_GROUP)
        for i in range(cls.shape[0]):
            assert bool((cls[i, :case.N] == SENT[got["c"].es]).all()), f"{case.name}: [cls] row {i * (G.ROW_GROUP + 1)} was written"
    assert got["c"].outside_intact(got["wrote"])


@pytest.mark.parametrize("case,half", LIN_PARAMS)
def test_guards_linear(ops, case, half):
    """Output guards: C (ldc = N + 8) and the column sums lie in sentinel-filled allocations; pad columns, the rows before and behind the
    view and the [cls] rows are bit-unchanged.  Operand guards: A, B (lda / ldb wider than the extents), bias, rowscale, residual (ldr = N + 8)
    and aux are surrounded by quiet NaNs; the result is bit-equal to the packed call's."""
    tight = run_linear(ops, case, half, padded=False)
    wide = run_linear(ops, case, half, padded=True)
    assert wide["c"].ld == case.N + PAD and wide["ins"][0].ld > wide["ins"][0].cols
    diff = int((wide["C"].view(INT[wide["c"].es]) != tight["C"].view(INT[tight["c"].es])).sum())
    hit = wide["c"].outside_touched(wide["wrote"])
    if wide["cs"] is not None:
        diff += int((wide["colsum"].view(torch.int32) != tight["colsum"].view(torch.int32)).sum())
        hit += wide["cs"].outside_touched()
    hit_in = sum(x.outside_touched() for x in wide["ins"] if x is not None)          # (operands are read-only: their guards are as they were)
    print(G.line(f"{case.name} {HALF_IDS[half]}", case.kernel, "guards", f"{diff} diff", f"{hit + hit_in} hit", wide["C"].numel()))
    assert diff == 0, f"{case.name}: the padded and the packed call differ in {diff} elements"
    assert hit == 0, f"{case.name}: {hit} elements outside C[M, N] / the column sums were written"
    assert hit_in == 0


# ---- the kernel the size rules choose ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto,half", [pytest.param(a, h, id=f"{a.op}-{a.layout}-o{a.out}-{a.M}x{a.N}x{a.K}-{HALF_IDS[h]}")
                                       for a in G.AUTO for h in (G.HALVES if a.op == "h" else [None])])
def test_auto_dispatch_names_its_kernel(ops, auto, half):
    """Selector 0: simseg_gemm / dispatch_h16 pick the kernel by their size rules; the rule's both sides are in the list, so a changed
    threshold fails here.  The result is checked exactly, as in test_exact."""
    case = G.Case(auto.want, auto.op, auto.layout, auto.out, auto.M, auto.N, auto.K, "splitk" if auto.splitk > 1 else "plain", auto.splitk, auto.note)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in G.int_inputs(case).items()}
    a, b = operands(d, case, half, False)
    c = Buf(case.M, case.N, out_dtype(case, half), d.get("c0"), False)
    ops.set_gemm_variant(0)
    ran = gemm_call(ops, a, b, c, case.M, case.N, case.K, case.ta, case.tb, alpha=d["alpha"], accumulate=int(auto.splitk > 1), splitk=auto.splitk)
    assert ran == auto.want, f"{auto.note}: ran on kernel {ran}, the rule says {auto.want}"
    want = G.linear_ref(case, d)["C"].float().to(c.t.dtype)
    wrong = int((c.t != want).sum())
    print(G.line(f"auto {auto.op}-{auto.layout}-{auto.M}x{auto.N}x{auto.K} {HALF_IDS[half]}", ran, "exact", "0 tol", f"{wrong} off", want.numel()))
    assert wrong == 0


# ---- the grouped weight-gradient launch ----------------------------------------------------------------------------------------------------
def _group_call(ops, bufs, rows, slices):
    from simseg_amd.lib import call, ptr, raw, stream
    desc = []
    for dy, x, dw in bufs:
        desc += [ptr(dy.t), ptr(x.t), ptr(dw.t), dy.cols, x.cols, dy.ld, x.ld, dw.ld]
    ops.set_gemm_variant(0)
    call("simseg_gemm_wgrad_group", (ctypes.c_int64 * len(desc))(*desc), len(bufs), rows, slices, stream())
    torch.cuda.synchronize()
    return raw("simseg_wgrad_group_last"), ops.gemm_last_variant()


@pytest.mark.parametrize("half", G.HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("grp", G.GROUPED, ids=lambda g: f"wg-{g.rows}-s{g.slices}")
def test_grouped_wgrad_exact_and_guarded(ops, grp, half):
    """dW_i += dY_i^T X_i for problems of different out / in in one launch: exact on integers (start value included), and with the records'
    own leading dimensions (ld_dY / ld_X / ld_dW wider than the extents) bit-equal to the packed launch, nothing written outside dW_i."""
    results = {}
    for padded in (False, True):
        bufs, wants = [], []
        for i, (out, inn) in enumerate(grp.problems):
            g = torch.Generator().manual_seed(G.seed_of(f"wg{grp.rows}-{i}"))
            dy, x = G._randint(-4, 4, (grp.rows, out), g).cuda(), G._randint(-4, 4, (grp.rows, inn), g).cuda()
            w0 = G._randint(-16, 16, (out, inn), g).cuda()
            bufs.append((Buf(grp.rows, out, half, dy.to(half), padded), Buf(grp.rows, inn, half, x.to(half), padded), Buf(out, inn, torch.float32, w0, padded)))
            wants.append((w0.double() + dy.double().T @ x.double()).float())
        n, ran = _group_call(ops, bufs, grp.rows, grp.slices)
        assert n == len(grp.problems) and ran == 3, (n, ran)
        for i, ((dy, x, dw), want) in enumerate(zip(bufs, wants)):
            wrong = int((dw.t != want).sum())
            print(G.line(f"wg rows {grp.rows} s{grp.slices} #{i} {dw.rows}x{dw.cols} {HALF_IDS[half]}{' padded' if padded else ''}", "wg", "exact", "0 tol", f"{wrong} off", want.numel()))
            assert wrong == 0
            assert dw.outside_intact() and dy.outside_intact() and x.outside_intact()
        results[padded] = [dw.t.clone() for _, _, dw in bufs]
    assert all(torch.equal(p, q) for p, q in zip(results[False], results[True]))


# ---- nonlinear epilogues against float64, block by block -------------------------------------------------------------------------------------
def _judge(name, kernel, kind, got, ref, yards, odt, **kw):
    r = G.judge2d(got, ref, yards, odt, **kw)
    print(G.line(name, kernel, kind, r["rms"], r["max"], r["blocks"]))
    return r


def _finish(results):
    for name, kind, r in results:
        assert r["zero"] == 0, f"{name} {kind}: {r['zero']} blocks with an all-zero reference"
        assert not r["bad"], f"{name} {kind}: {r['text']}"


def run_nonlinear(ops, case, half, padded):
    """The launches of one nonlinear case.  -> (tensors by kind, Bufs that the calls wrote, Bufs that they read)."""
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in G.nl_inputs(case, half).items()}
    odt = out_dtype(case, half)
    a, b = operands(d, case, half, padded)
    bias = vec(case.N, torch.float32, d["bias"], padded)
    M, N, K = case.M, case.N, case.K
    got, wrote, read = {}, [], [a, b, bias]
    forced(ops, case.kernel)
    try:
        if case.epi == "gelu1":
            c, x = Buf(M, N, odt, None, padded), Buf(M, N, odt, None, padded)
            ran = gemm_call(ops, a, b, c, M, N, K, case.ta, case.tb, bias=bias, act=1, aux_out=x)
            got.update(out=c.t, pre=x.t)
            wrote += [c, x]
        elif case.epi in ("act34", "gelu3"):
            c, x = Buf(M, N, odt, None, padded), Buf(M, N, odt, None, padded)
            ran = gemm_call(ops, a, b, c, M, N, K, case.ta, case.tb, bias=bias, act=3, aux_out=x)
            got.update(out=c.t, dact=x.t)
            wrote += [c, x]
            if case.epi == "act34":
                assert ran == case.kernel
                c4, cs = Buf(M, N, odt, None, padded), vec(N, torch.float32, torch.zeros(N), padded)
                ran = gemm_call(ops, a, b, c4, M, N, K, case.ta, case.tb, bias=bias, act=4, aux=x, colsum=cs)
                got.update(prod=c4.t, colsum=cs.t[0])
                wrote += [c4, cs]
        elif case.epi == "act2":
            c, x = Buf(M, N, odt, None, padded), Buf(M, N, odt, d["aux"], padded)
            ran = gemm_call(ops, a, b, c, M, N, K, case.ta, case.tb, bias=bias, act=2, aux=x)
            got.update(prod2=c.t)
            wrote, read = wrote + [c], read + [x]
    finally:
        ops.set_gemm_variant(0)
    assert ran == case.kernel, f"{case.name}: ran on kernel {ran}"
    return d, got, wrote, read


def nl_expect(case, d, got, odt):
    """{kind: (float64 reference, [yardsticks])}: the same formula in float64 and in fp32 torch on the device, the yardstick rounded to the
    output type where the kernel rounds - the stored tensors, and on the ping-pong kernel's full tiles the product ahead of act 4's
    multiplication (pp_epilogue_bf16, EK = 1: "rounded to the 16-bit type BEFORE the multiplication").  Partial tiles take the staged
    epilogue, which multiplies and sums the unrounded fp32 value; no case mixes full and partial tiles, so each has ONE act 4 yardstick."""
    R = (lambda t: t.to(odt).float())
    p64, p32 = G.nl_pre(d, torch.float64), G.nl_pre(d, torch.float32)
    exp = {}
    # (the accumulator-layout epilogues evaluate the documented polynomial fit of the CDF: _gemm_ref.gelu_poly holds the decision)
    y_gelu = [R(G.gelu(p32))] + ([R(G.gelu_poly(p32))] if G.poly_epilogue(case) else [])
    y_dgelu = [R(G.dgelu(p32))] + ([R(G.gelu_poly(p32, grad=True))] if G.poly_epilogue(case) else [])
    if "pre" in got:
        exp["out"], exp["pre"] = (G.gelu(p64), y_gelu), (p64, [R(p32)])
    if "dact" in got:
        exp["out"], exp["dact"] = (G.gelu(p64), y_gelu), (G.dgelu(p64), y_dgelu)
    if "prod" in got:
        s = got["dact"].float()          # exactly the values the kernel receives
        raw = [(R(p32) if G.poly_epilogue(case) else p32) * s]
        exp["prod"] = (p64 * s.double(), [R(y) for y in raw])
        # the column sums are an fp32 output added up from the fp32 products ahead of their rounding (epilogue_block: cs += v; pp_epilogue_bf16:
        # cs += pv): the yardstick is the fp32 sum of the same unrounded products, the rule the fp32 one
        exp["colsum"] = ((p64 * s.double()).sum(0), [y.sum(0) for y in raw])
    if "prod2" in got:
        exp["prod2"] = (p64 * G.dgelu(d["aux"].double()), [R(p32 * G.dgelu(d["aux"]))])
    return exp


@pytest.mark.parametrize("case,half", NL_PARAMS)
def test_nonlinear_epilogues_per_block(ops, case, half):
    """act 1 / 3 / 3-then-4 / 2 against float64 on exactly the values the kernel receives, one 32x32 accumulator tile at a time (column
    sums: 32 columns), rows and columns of the operands ramped over 2^8 so that a whole-matrix scale would forgive the small tiles."""
    odt = out_dtype(case, half)
    d, got, _, _ = run_nonlinear(ops, case, half, padded=False)
    name = f"{case.name} {HALF_IDS[half]}"
    results = []
    for kind, (ref, yards) in nl_expect(case, d, got, odt).items():
        results.append((name, kind, _judge(name, case.kernel, kind, got[kind], ref, yards, torch.float32 if kind == "colsum" else odt)))
    _finish(results)


@pytest.mark.parametrize("case,half", NL_PARAMS)
def test_guards_nonlinear(ops, case, half):
    """The guard bands of test_guards_linear around the nonlinear epilogues' tensors: C, aux_out (the saved pre-activation / derivative: same
    leading dimension as C) and the column sums written inside their regions only; aux read inside its region only."""
    _, tight, _, _ = run_nonlinear(ops, case, half, padded=False)
    _, wide, wrote, read = run_nonlinear(ops, case, half, padded=True)
    diff, n = 0, 0
    for kind in tight:
        if kind != "colsum":          # (float atomics of non-integers: order-dependent in the last bits; judged in test_nonlinear_epilogues_per_block)
            diff += int((wide[kind].contiguous().view(INT[wide[kind].element_size()]) != tight[kind].contiguous().view(INT[tight[kind].element_size()])).sum())
            n += tight[kind].numel()
    hit, hit_in = sum(x.outside_touched() for x in wrote), sum(x.outside_touched() for x in read)
    print(G.line(f"{case.name} {HALF_IDS[half]}", case.kernel, "guards", f"{diff} diff", f"{hit + hit_in} hit", n))
    assert diff == 0, f"{case.name}: the padded and the packed call differ in {diff} elements"
    assert hit == 0, f"{case.name}: {hit} elements outside the written tensors were written"
    assert hit_in == 0


# ---- the tile-blocked derivative images (act 5 / 6 and 7 / 8) -------------------------------------------------------------------------------
def _blocked_fixture(ops, case, half):
    """fc1 forward with the derivative saved row-major (act 3), blocked (act 5) and blocked in 8 bits (act 7), on guarded buffers.  The
    blocked epilogues require ldc == N: there are no pad columns, the guards are the rows before and behind."""
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in G.nl_inputs(case, half).items()}
    a, b = operands(d, case, half, False)
    bias = vec(case.N, torch.float32, d["bias"], True)
    M, N, K = case.M, case.N, case.K
    mk = lambda dt=half: Buf(M, N, dt, None, True, pad_cols=False)      # noqa: E731
    y3, d3, y5, d5, y7, d7 = mk(), mk(), mk(), mk(), mk(), mk(torch.uint8)
    assert gemm_call(ops, a, b, y3, M, N, K, 0, 0, bias=bias, act=3, aux_out=d3) == case.kernel
    assert gemm_call(ops, a, b, y5, M, N, K, 0, 0, bias=bias, act=5, aux_out=d5) == case.kernel
    assert gemm_call(ops, a, b, y7, M, N, K, 0, 0, bias=bias, act=7, aux_out=d7) == case.kernel
    return d, bias, y3, d3, y5, d5, y7, d7


@pytest.mark.parametrize("case,half", [pytest.param(c, h, id=f"{c.name}-{HALF_IDS[h]}") for c in G.NL_CASES if c.epi == "blocked56" for h in G.HALVES])
def test_blocked_image_equals_the_row_major_pair(ops, case, half):
    """act 5 / 6 against act 3 / 4 on the same kernel and inputs, bit for bit: the forward output; the image, read back through the layout
    of pp_epilogue_bf16, against the row-major derivative; and the dgrad product on operands in {-1, 0, 1} - the row-major act 4 rounds the
    matmul result to 16 bits before it multiplies and act 6 does not (both documented in pp_epilogue_bf16), so only a result that is
    already a 16-bit number makes the two the same arithmetic.  Kernel 10 has no row-major act 4 (it runs on kernel 3): there the product
    of act 6 is held against kernel 3's, which the integers make independent of the summation order."""
    from simseg_amd.lib import raw
    M, N, K = case.M, case.N, case.K
    assert raw("simseg_gemm_aux_blocked_ok", M, N, K) == 1
    forced(ops, case.kernel)
    try:
        d, bias, y3, d3, y5, d5, y7, d7 = _blocked_fixture(ops, case, half)
        assert torch.equal(y3.t.view(torch.int16), y5.t.view(torch.int16)) and torch.equal(y3.t.view(torch.int16), y7.t.view(torch.int16))
        idx = G.blocked_index(M, N).cuda()
        assert torch.equal(d5.t.reshape(-1)[idx.view(-1)].view(M, N).view(torch.int16), d3.t.contiguous().view(torch.int16)), "the image is not the row-major derivative in blk0's order"
        assert all(x.outside_intact() for x in (y3, d3, y5, d5, y7, d7))
        # the dgrad through fc2: g [M, K2] . w2 [K2, N] (NN), K2 = K, integers in {-1, 0, 1}: |sum| far below 256, so the product is a 16-bit number
        gen = torch.Generator().manual_seed(G.seed_of(case.name, 2))
        g_, w2 = G._randint(-1, 1, (M, K), gen).cuda(), G._randint(-1, 1, (K, N), gen).cuda()
        assert G.representable(g_ @ w2, half)
        ga, wb = Buf(M, K, half, g_.to(half), False), Buf(K, N, half, w2.to(half), False)
        x6, cs6 = Buf(M, N, half, None, True, pad_cols=False), vec(N, torch.float32, torch.zeros(N), True)
        assert gemm_call(ops, ga, wb, x6, M, N, K, 0, 1, act=6, aux=d5, colsum=cs6) == case.kernel
        ops.set_gemm_variant(3)
        x4, cs4 = Buf(M, N, half, None, True, pad_cols=False), vec(N, torch.float32, torch.zeros(N), True)
        assert gemm_call(ops, ga, wb, x4, M, N, K, 0, 1, act=4, aux=d3, colsum=cs4) == 3
    finally:
        ops.set_gemm_variant(0)
    wrong = int((x6.t.view(torch.int16) != x4.t.view(torch.int16)).sum())
    print(G.line(f"{case.name} {HALF_IDS[half]}", case.kernel, "act6==act4", "0 tol", f"{wrong} off", M * N))
    assert wrong == 0
    assert all(x.outside_intact() for x in (x6, cs6, x4, cs4, d5, d3))
    want = ((g_ @ w2).double() * d3.t.double())
    r = _judge(f"{case.name} {HALF_IDS[half]}", case.kernel, "colsum", cs6.t[0], want.sum(0), [((g_ @ w2) * d3.t.float()).sum(0)], torch.float32)
    _finish([(case.name, "colsum", r)])


@pytest.mark.parametrize("case,half", [pytest.param(c, h, id=f"{c.name}-{HALF_IDS[h]}") for c in G.NL_CASES if c.epi == "blocked78" for h in G.HALVES])
def test_blocked_images_per_block(ops, case, half):
    """The forward of act 5 / 7 and the products of act 6 / 8 on operands that are no integers, per block against float64.  The 8-bit image,
    read back through the layout, against float64 GELU' with the formula of include/simseg_hip.h - round((g + 0.132) * 255 / 1.264) in fp32
    torch - as the yardstick (the grid is the rounding this epilogue documents); the products against float64 on exactly the derivative
    values the call receives (the decoded image), yardstick: the same product in fp32, rounded once.  On kernel 10 the float64 products are
    formed on the device (3 x 2^32 multiply-adds each; the launches themselves take milliseconds)."""
    M, N, K = case.M, case.N, case.K
    name = f"{case.name} {HALF_IDS[half]}"
    R = (lambda t: t.to(half).float())
    forced(ops, case.kernel)
    try:
        d, bias, y3, d3, y5, d5, y7, d7 = _blocked_fixture(ops, case, half)
        idx = G.blocked_index(M, N).cuda().view(-1)
        q8 = d7.t.reshape(-1)[idx].view(M, N).float()
        gen = torch.Generator().manual_seed(G.seed_of(case.name, 3))
        g_ = (torch.randn(M, K, generator=gen) * G.ramp(M)[:, None]).to(half).cuda()
        w2 = (torch.randn(K, N, generator=gen) * K ** -0.5 * G.ramp(N)[None, :]).to(half).cuda()
        ga, wb = Buf(M, K, half, g_, False), Buf(K, N, half, w2, False)
        x6, cs6 = Buf(M, N, half, None, True, pad_cols=False), vec(N, torch.float32, torch.zeros(N), True)
        x8, cs8 = Buf(M, N, half, None, True, pad_cols=False), vec(N, torch.float32, torch.zeros(N), True)
        assert gemm_call(ops, ga, wb, x6, M, N, K, 0, 1, bias=bias, act=6, aux=d5, colsum=cs6) == case.kernel
        assert gemm_call(ops, ga, wb, x8, M, N, K, 0, 1, bias=bias, act=8, aux=d7, colsum=cs8) == case.kernel
        cross = []
        if case.kernel == 10:
            # the persistent kernel's act 8 against the per-tile kernel's on the same 8-bit image and operands in {-1, 0, 1}: the accumulators are
            # exact integers in any order and act 8 rounds once (fma(acc, alpha, bias) * g), so the two kernels must agree bit for bit
            gi, wi = G._randint(-1, 1, (M, K), gen).cuda().to(half), G._randint(-1, 1, (K, N), gen).cuda().to(half)
            gia, wib = Buf(M, K, half, gi, False), Buf(K, N, half, wi, False)
            xa, xb = Buf(M, N, half, None, True, pad_cols=False), Buf(M, N, half, None, True, pad_cols=False)
            assert gemm_call(ops, gia, wib, xa, M, N, K, 0, 1, bias=bias, act=8, aux=d7) == 10
            ops.set_gemm_variant(3)
            assert gemm_call(ops, gia, wib, xb, M, N, K, 0, 1, bias=bias, act=8, aux=d7) == 3
            cross = [xa, xb]
    finally:
        ops.set_gemm_variant(0)
    if cross:
        wrong = int((cross[0].t.view(torch.int16) != cross[1].t.view(torch.int16)).sum())
        print(G.line(name, case.kernel, "act8==k3", "0 tol", f"{wrong} off", M * N))
        assert wrong == 0
    assert all(x.outside_intact() for x in [y5, d5, y7, d7, x6, cs6, x8, cs8] + cross)
    p64, p32 = G.nl_pre(d, torch.float64), G.nl_pre(d, torch.float32)
    results = [(name, "out", _judge(name, case.kernel, "out", y5.t, G.gelu(p64), [R(G.gelu(p32)), R(G.gelu_poly(p32))], half)),
               (name, "image8", _judge(name, case.kernel, "image8", q8.double() / G.GELU8_SCALE - G.GELU8_OFF, G.dgelu(p64), [G.quant8(G.dgelu(p32)), G.quant8(G.gelu_poly(p32, grad=True))], half, prec=24))]
    q64 = g_.double() @ w2.double() + d["bias"].double()
    q32 = g_.float() @ w2.float() + d["bias"]
    for kind, x, cs, s64, s32 in (("prod6", x6, cs6, d3.t.double(), d3.t.float()),
                                  ("prod8", x8, cs8, q8.double() / G.GELU8_SCALE - G.GELU8_OFF, q8 / G.GELU8_SCALE - G.GELU8_OFF)):
        results.append((name, kind, _judge(name, case.kernel, kind, x.t, q64 * s64, [R(q32 * s32)], half)))
        results.append((name, kind + "cs", _judge(name, case.kernel, kind + "cs", cs.t[0], (q64 * s64).sum(0), [(q32 * s32).sum(0)], torch.float32)))
    _finish(results)
