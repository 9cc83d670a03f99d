"""Fused top-K retrieval search (csrc/search.hip) against CPU references.

Exact cases use integer-valued embeddings with entries in [-3, 3]: the values are exact in fp32 and in bf16 and every inner product is an
integer far below 2^24, so neither mode rounds anything and the kernel's (score, idx) must be BIT-identical to the first K columns of a
stable descending CPU sort of the exactly computed matrix - ties (plentiful) included.  Real-valued cases are checked row by row against a
float64 CPU product with the project's fp32 GEMM tolerance (1e-5 of the largest |score|, tests/test_gpu_kernels.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from simseg_amd import ops as o
    return o


def _int_emb(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (rows, D), generator=g).float()


def _exact_ref(q, g, K, offset=0):
    """First K columns of the stable descending sort of the exact matrix (float64 holds these integers exactly); -inf / -1 past N."""
    sim = q.double() @ g.double().T
    val, order = torch.sort(sim, dim=1, descending=True, stable=True)
    M, N = sim.shape
    score = torch.full((M, K), float("-inf"))
    idx = torch.full((M, K), -1, dtype=torch.int32)
    n = min(K, N)
    score[:, :n] = val[:, :n].float()
    idx[:, :n] = (order[:, :n] + offset).int()
    return score, idx


def _padded(t, pad, dtype):
    """The same matrix on the device in `dtype`, as a view with leading dimension D + pad."""
    t = t.to(dtype).cuda()
    if pad == 0:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + pad), 7.0, device="cuda", dtype=dtype)      # the padding must not be read as data
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _bits(t):
    return t.contiguous().view(torch.int32)


EXACT_SHAPES = [
    # M, N, D, K, ld padding, index_offset
    (130, 1000, 64, 10, 0, 0),          # M and N off the 64 x 128 tiles
    (3, 7, 64, 5, 0, 0),
    (3, 7, 64, 10, 0, 0),               # N < K: -inf / -1 tail
    (5, 100, 64, 128, 0, 0),            # N < K at the widest K
    (130, 1000, 64, 1, 0, 0),
    (130, 1000, 512, 5, 0, 0),
    (70, 3000, 64, 128, 0, 0),          # wide lists, several sorts per row
    (257, 700, 512, 128, 0, 0),
    (3, 200000, 64, 10, 0, 0),          # column-split path: 3 rows against 1563 column tiles
    (3, 200000, 64, 128, 0, 0),
    (130, 1000, 64, 10, 8, 0),          # ld > D
    (66, 515, 512, 5, 24, 1000),        # ld > D and an index offset
    (130, 1000, 64, 10, 0, 123456),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,N,D,K,pad,offset", EXACT_SHAPES)
def test_exact_cases_bit_identical(ops, dtype, M, N, D, K, pad, offset):
    q, g = _int_emb(M, D, 10 + M), _int_emb(N, D, 20 + K)
    want_s, want_i = _exact_ref(q, g, K, offset)
    dq, dg = _padded(q, pad, dtype), _padded(g, pad, dtype)
    if pad:
        assert dq.stride(0) == D + pad and not dq.is_contiguous()
    got_s, got_i = ops.topk_search(dq, dg, K, index_offset=offset)
    assert got_s.dtype == torch.float32 and got_i.dtype == torch.int32 and got_s.shape == (M, K) == got_i.shape
    got_s, got_i = got_s.cpu(), got_i.cpu()
    assert torch.equal(got_i, want_i), f"indices differ in {(got_i != want_i).sum().item()} slots"
    assert torch.equal(_bits(got_s), _bits(want_s))


def test_bad_inner_dim_raises(ops):
    q, g = torch.zeros(4, 45, device="cuda"), torch.zeros(9, 45, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.topk_search(q, g, 3)
    with pytest.raises(RuntimeError, match="1..128"):
        ops.topk_search(torch.zeros(4, 64, device="cuda"), torch.zeros(9, 64, device="cuda"), 129)


def _unit_rows(rows, D, seed):
    x = torch.randn(rows, D, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,N,D,K", [(1000, 5000, 512, 10), (5000, 25000, 512, 10)])
def test_real_valued_against_float64(ops, dtype, M, N, D, K):
    q, g = _unit_rows(M, D, 1), _unit_rows(N, D, 2)
    if dtype == torch.bfloat16:         # the reference sees the operands the kernel sees
        q, g = q.bfloat16().float(), g.bfloat16().float()
    score, idx = ops.topk_search(q.to(dtype).cuda(), g.to(dtype).cuda(), K)
    score2, idx2 = ops.topk_search(q.to(dtype).cuda(), g.to(dtype).cuda(), K)
    assert torch.equal(_bits(score), _bits(score2)) and torch.equal(idx, idx2), "two calls on the same inputs differ"
    score, idx = score.cpu().double(), idx.cpu().long()
    g64 = g.double()
    # every row is checked, 500 at a time; the tolerance (1e-5 of the reference's largest |score| over the whole matrix) is known after the
    # last chunk, so the worst figures are kept and compared at the end
    top, worst_gather, worst_left_out, checked = 0.0, 0.0, float("-inf"), 0
    for s in range(0, M, 500):
        ref = q[s:s + 500].double() @ g64.T                                   # [<=500, N] float64
        top = max(top, ref.abs().max().item())
        sc, ix = score[s:s + 500], idx[s:s + 500]
        assert (sc[:, 1:] <= sc[:, :-1]).all(), "scores are not non-increasing"
        assert (ix >= 0).all() and (ix < N).all(), "index out of range"
        assert (ix.sort(dim=1).values.diff(dim=1) != 0).all(), "an index is returned twice"
        gather_err = (sc - ref.gather(1, ix)).abs().max().item()
        worst_gather = max(worst_gather, gather_err)
        rest = ref.scatter(1, ix, float("-inf"))                              # the columns left out
        margin = (rest.max(dim=1).values - sc[:, K - 1]).max().item()
        worst_left_out = max(worst_left_out, margin)
        checked += ref.shape[0]
    tau = 1e-5 * top
    print(f"{M}x{N}x{D} K={K} {dtype}: tau {tau:.3e}, worst |score - ref| {worst_gather:.3e}, worst (left-out ref - K-th score) {worst_left_out:.3e}")
    assert checked == M
    assert worst_gather <= tau
    assert worst_left_out <= 2 * tau


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [10, 128])
def test_chunked_gallery_bit_identical(ops, dtype, K):
    from simseg_amd.retrieval import search
    M, N, D = 130, 3000, 64
    q, g = _int_emb(M, D, 5), _int_emb(N, D, 6)
    ids = torch.arange(N) // 5 + 100
    dq, dg = q.to(dtype).cuda(), g.to(dtype).cuda()
    one_s, one_i, one_id = search(dq, dg, K, gallery_ids=ids, compute_dtype=dtype)
    cuts = [0, 1000, 1007, 1900, 1903, 3000]                                 # uneven; 1000:1007 and 1900:1903 are shorter than K
    chunks = ((dg[a:b], a) for a, b in zip(cuts[:-1], cuts[1:]))
    got_s, got_i, got_id = search(dq, chunks, K, gallery_ids=ids, compute_dtype=dtype)
    assert one_i.dtype == torch.int64 and got_i.dtype == torch.int64
    assert torch.equal(_bits(got_s), _bits(one_s)) and torch.equal(got_i, one_i) and torch.equal(got_id, one_id)
    want_s, want_i = _exact_ref(q, g, K)
    assert torch.equal(got_i.cpu(), want_i.long()) and torch.equal(_bits(got_s.cpu()), _bits(want_s))
    assert torch.equal(got_id.cpu(), ids[want_i.long()])


def test_search_casts_fp32_operands_for_bf16_compute(ops):
    from simseg_amd.retrieval import search
    q, g = _int_emb(70, 64, 7), _int_emb(900, 64, 8)
    s, i = search(q.cuda(), g.cuda(), 5, compute_dtype=torch.bfloat16)
    want_s, want_i = _exact_ref(q, g, 5)
    assert torch.equal(i.cpu(), want_i.long()) and torch.equal(_bits(s.cpu()), _bits(want_s))


@pytest.mark.parametrize("k", [1, 5, 10])
def test_embann_topk_cuda_equals_ann(k):
    from simseg.tasks.clip.hooks.utils import EmbANN, IndexedEmbInfo
    M, N, D = 150, 1200, 64
    left = IndexedEmbInfo("image", torch.arange(M).cuda(), _int_emb(M, D, 1).cuda())
    right = IndexedEmbInfo("text", (torch.arange(N) // 5).cuda(), _int_emb(N, D, 2).cuda())
    ann = EmbANN()
    want_sorted, want_matched = ann._ann(left, right)
    got_sorted, got_matched = ann.topk(left, right, k)
    assert torch.equal(got_sorted, want_sorted[:, :k]) and torch.equal(got_matched, want_matched[:, :k])
    # and the CPU branch gives the same answer from the same embeddings
    cpu = ann.topk(IndexedEmbInfo("image", left.group_idx.cpu(), left.emb_mat.cpu()), IndexedEmbInfo("text", right.group_idx.cpu(), right.emb_mat.cpu()), k)
    assert torch.equal(got_sorted.cpu(), cpu[0]) and torch.equal(got_matched.cpu(), cpu[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_zero_shot_topk_equals_torch(dtype):
    from simseg_amd.heads import zero_shot_topk
    B, C, D = 300, 1000, 64
    img, cls = _int_emb(B, D, 3), _int_emb(C, D, 4)
    labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(5))
    order = torch.sort(img.double() @ cls.double().T, dim=1, descending=True, stable=True).indices
    labels[::3] = order[::3, 0]                      # a third of the labels are the top-1 class, some more sit within the top 5
    labels[1::7] = order[1::7, 3]
    pred, counts = zero_shot_topk(img.cuda(), cls.cuda(), labels.cuda(), ks=(1, 5), compute_dtype=dtype)
    assert pred.shape == (B, 5) and pred.dtype == torch.int64 and counts.is_cuda and counts.dtype == torch.int32
    assert torch.equal(pred.cpu(), order[:, :5])
    want = [(order[:, :k] == labels[:, None]).any(dim=1).sum().item() for k in (1, 5)]
    assert counts.cpu().tolist() == want and 0 < want[0] < want[1] < B
    assert torch.equal(zero_shot_topk(img.cuda(), cls.cuda(), ks=(1, 5), compute_dtype=dtype), pred)


def test_no_score_matrix(ops):
    from simseg_amd import lib
    M, N, D, K = 5000, 25000, 512, 10
    bound = M * N * 4 // 8
    for code in (0, 1):
        assert 0 <= lib.raw("simseg_topk_search_workspace_bytes", M, N, D, K, code) < bound
    q, g = _unit_rows(M, D, 1).cuda(), _unit_rows(N, D, 2).cuda()
    for dtype in DTYPES:
        a, b = q.to(dtype), g.to(dtype)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = ops.topk_search(a, b, K)
        torch.cuda.synchronize()
        delta = torch.cuda.max_memory_allocated() - before
        assert delta < bound, f"peak allocation grew by {delta} bytes across the call (bound {bound})"
        del out
