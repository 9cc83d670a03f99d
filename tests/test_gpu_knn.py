"""The weighted k-NN evaluation on the MI355X: simseg_knn_vote_rows against the float64 statement of tests/_knn_ref.py, then through the
fused search (knn_predict, FeatureBank) and the evaluator.

Bounds are derived, not measured (_knn_ref.allowance): the relative error of a vote is at most (3 max|x| + 2 + (k - 1)) * 2^-24 with
x = (s_j - s_0) / T, and the tests allow twice that - 2.1e-5 at k = 128 for scores in [-0.2, 0.9) and T = 0.07.  `pred` is compared
exactly on every row whose reference gap between neighbouring ranks is at least GAP_MIN = 1e-4; at most 2 % of a case's rows may fall
below it.  Counts are integers and exact.  Every test prints the largest error it saw beside its bound."""
import numpy as np
import pytest
import torch

from _knn_ref import CLASSES, GAP_MIN, KS, NEAR_TIE_CAP, SEEDS, T_DEFAULT, allowance, case_with_ref, host_counts, vote_ref
from conftest import tt

pytestmark = pytest.mark.gpu


def _run(score, idx, gallery_label, ks, T=T_DEFAULT, query_label=None, counts=None, idx_dtype=torch.int32):
    from simseg_amd import ops
    ql = None if query_label is None else tt(query_label).cuda()
    pred, vote, counts = ops.knn_vote(tt(score).cuda(), tt(idx).to(idx_dtype).cuda(), tt(gallery_label).cuda(), ks, T, query_label=ql, counts=counts)
    torch.cuda.synchronize()
    return pred.cpu().numpy(), vote.cpu().numpy(), counts


def _max_x(score, idx, T=T_DEFAULT):
    """Largest |(s_j - s_0) / T| over the valid entries."""
    s = np.where(np.asarray(idx) >= 0, np.asarray(score, dtype=np.float64), np.nan)
    d = (s[:, :1] - s) / np.float64(np.float32(T))
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def _compare(tag, got_pred, got_vote, want, ks, max_x, cap=NEAR_TIE_CAP):
    """Votes within the allowance of each k; pred exact on the rows whose reference gap is at least GAP_MIN.  -> largest error / allowance."""
    want_pred, want_vote, gap = want
    worst = 0.0
    for ki, k in enumerate(ks):
        tol = allowance(max_x, k)
        assert 4 * tol < GAP_MIN
        clear = gap[ki] >= GAP_MIN
        out = int((~clear).sum())
        assert out <= cap * clear.size, f"{tag} k={k}: {out} of {clear.size} rows are near-ties"
        # votes on EVERY row, slot by slot: slot r holds the r-th largest vote on both sides, and an order statistic moves by no more than
        # the values do, so the comparison holds on a near-tie row too, whichever of its two classes is listed first
        gv, wv = got_vote[ki].astype(np.float64), want_vote[ki]
        e = float((np.abs(gv - wv) / np.where(wv > 0, wv, 1.0)).max())
        print(f"{tag} k={k}: largest relative vote error {e:.3e} (allowance {tol:.3e}); {out} of {clear.size} rows below the gap")
        assert e <= tol, f"{tag} k={k}"
        assert np.array_equal(got_pred[ki][clear], want_pred[ki][clear]), f"{tag} k={k}"
        assert ((got_pred[ki] >= 0) == (want_pred[ki] >= 0)).all()              # the number of classes listed, on every row
        worst = max(worst, e / tol)
    return worst


# ---- 1. against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("seed", SEEDS)
def test_vote_against_float64(seed, C):
    offset = 37 if (seed, C) == (1, 1000) else 0                  # idx = class + offset into a gallery whose row offset + c has label c
    c = case_with_ref(seed, C, offset)
    pred, vote, counts = _run(c["score"], c["idx"], c["gallery_label"], KS, query_label=c["query_label"],
                              idx_dtype=torch.int64 if seed == 2 else torch.int32)
    _compare(f"seed={seed} C={C}", pred, vote, (c["pred"], c["vote"], c["gap"]), KS, 1.1 / 0.07)
    assert _max_x(c["score"], c["idx"]) <= 1.1 / 0.07
    assert (vote[0, :, 0] == 1.0).all() and np.array_equal(pred[0, :, 0], c["label"][:, 0])          # k = 1: the first label, vote exactly 1
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), host_counts(pred, c["query_label"]))
    again = _run(c["score"], c["idx"], c["gallery_label"], KS)                                       # same bits; nothing counted without labels
    assert again[2] is None and np.array_equal(again[0], pred) and np.array_equal(again[1].view(np.int32), vote.view(np.int32))


# ---- 2. exact ties ------------------------------------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_lower_class():
    score = np.array([[0.5, 0.5, 0.25, 0.25]], dtype=np.float32)
    pred, vote, counts = _run(score, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([9, 3, 3, 9]), (4,), query_label=np.array([9]))
    assert pred[0, 0].tolist() == [3, 9, -1, -1, -1]
    assert vote[0, 0, 0].view(np.int32) == vote[0, 0, 1].view(np.int32) and vote[0, 0, 0] > 1.0       # both classes sum the same two fp32 terms
    assert (vote[0, 0, 2:] == 0).all() and counts.tolist() == [[1, 0, 1]]


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------------
def _edge_case(M, K, C, seed):
    """Random descending rows whose valid counts cycle through {K, 0, 1, 3, K - 1, ...} (clipped to K): -1 / -inf tails as the search
    leaves them."""
    rng = np.random.default_rng(seed)
    score = -np.sort(-rng.uniform(-0.2, 0.9, (M, K)).astype(np.float32), axis=1)
    N = 50
    idx = rng.integers(0, N, (M, K)).astype(np.int32)
    gl = rng.integers(0, C, N).astype(np.int32)
    valid = np.array([[K, 0, 1, 3, K - 1, K // 2][m % 6] for m in range(M)]).clip(0, K)
    tail = np.arange(K)[None, :] >= valid[:, None]
    score[tail], idx[tail] = -np.inf, -1
    return score, idx, gl, valid, rng.integers(0, C, M).astype(np.int32)


@pytest.mark.parametrize("M,K,ks,C", [(1, 1, (1,), 3), (5, 1, (1,), 3), (67, 1, (1,), 40), (1, 128, (128,), 3), (5, 128, (1, 2, 64, 128), 3),
                                      (67, 128, (3, 10, 100, 128), 40), (67, 128, (50,), 4), (67, 70, (5, 64, 65, 70), 1000),
                                      (8197, 4, (2, 4), 3)])
def test_edges(M, K, ks, C):
    """Rows with fewer valid entries than k, rows with none, fewer than five classes, one to many rows (8197 rows: more than one row per
    wave of the capped grid), K = 1 and 128, one k and four, and counts that accumulate over two calls."""
    score, idx, gl, valid, ql = _edge_case(M, K, C, seed=M * 1000 + K)
    want = vote_ref(score, idx, gl, ks)
    pred, vote, counts = _run(score, idx, gl, ks, query_label=ql)
    _compare(f"M={M} K={K} ks={ks} C={C}", pred, vote, want, ks, 1.1 / 0.07, cap=1.0)
    none = valid == 0
    assert (pred[:, none] == -1).all() and (vote[:, none] == 0).all()                    # no neighbour: nothing listed ...
    n_classes = (pred >= 0).sum(2)
    for ki, k in enumerate(ks):
        assert (n_classes[ki] <= np.minimum(np.minimum(k, valid), min(C, 5))).all()
        assert (n_classes[ki][valid > 0] >= 1).all()
    hc = host_counts(pred, ql)
    assert (hc[:, 0] == M).all()                                                         # ... but the row is counted, as two misses
    assert np.array_equal(counts.cpu().numpy(), hc)
    _, _, counts2 = _run(score, idx, gl, ks, query_label=ql, counts=counts)
    assert counts2 is counts and np.array_equal(counts.cpu().numpy(), 2 * hc)


def test_an_index_past_the_gallery_ends_the_list():
    """idx >= N is never used to read a label: it ends the row's list like an empty slot."""
    score = np.array([[0.9, 0.8, 0.7, 0.6]], dtype=np.float32)
    pred, vote, _ = _run(score, np.array([[1, 0, 5, 2]], dtype=np.int32), np.array([4, 6, 8, 8, 8]), (4,))
    want = vote_ref(score, np.array([[1, 0, -1, -1]]), np.array([4, 6, 8, 8, 8]), (4,))
    assert np.array_equal(pred, want[0]) and pred[0, 0].tolist() == [6, 4, -1, -1, -1]


# ---- 4. through the search ----------------------------------------------------------------------------------------------------------
N_BANK, D_BANK, C_BANK, M_QUERY = 2000, 64, 10, 257


def _bank(feats, labels, dtype, splits=None):
    from simseg_amd.knn import FeatureBank
    bank = FeatureBank(feats.shape[1], dtype)
    lo = 0
    for n in splits or (feats.shape[0],):
        bank.add(feats[lo:lo + n], labels[lo:lo + n])
        lo += n
    assert lo == feats.shape[0] == len(bank)
    return bank


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_knn_predict_through_the_search(dtype):
    from simseg_amd import knn, retrieval
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(N_BANK, D_BANK, generator=g).cuda() * 3.0
    labels = torch.randint(0, C_BANK, (N_BANK,), generator=g)
    q = torch.randn(M_QUERY, D_BANK, generator=g).cuda() * 0.5
    ql = torch.randint(0, C_BANK, (M_QUERY,), generator=g)
    ks = (10, 20, 100)
    bank = _bank(feats, labels.cuda(), dtype)
    pred, vote, counts = knn.knn_predict(q, bank, ks, query_label=ql)
    # the reference on the search's own lists (the search is bit-reproducible, so this is the list knn_predict voted on)
    score, index = retrieval.search(knn.normalize_rows(q), bank.chunks(), ks[-1], compute_dtype=dtype)
    assert index.dtype == torch.int64 and (index >= 0).all()
    score, index = score.cpu().numpy(), index.cpu().numpy()
    want = vote_ref(score, index, labels.numpy(), ks)
    max_x = _max_x(score, index)
    pred, vote = pred.cpu().numpy(), vote.cpu().numpy()
    _compare(f"search {dtype} (max|x| {max_x:.2f})", pred, vote, want, ks, max_x)
    assert np.array_equal(counts.cpu().numpy(), host_counts(pred, ql.numpy()))
    # the same bank added as three unequal chunks (merged lists): identical results
    chunked = _bank(feats, labels.cuda(), dtype, splits=(700, 1, 1299))
    assert [o for _, o in chunked.chunks()] == [0, 700, 701]
    p3, v3, c3 = knn.knn_predict(q, chunked, ks, query_label=ql.cuda())
    assert torch.equal(p3.cpu(), tt(pred)) and torch.equal(v3.cpu(), tt(vote)) and torch.equal(c3, counts)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_well_separated_clusters_are_all_hits(dtype):
    from simseg_amd import knn
    g = torch.Generator().manual_seed(6)
    centres = torch.nn.functional.normalize(torch.randn(C_BANK, D_BANK, generator=g), dim=1)
    labels = torch.arange(N_BANK) % C_BANK
    ql = torch.randint(0, C_BANK, (M_QUERY,), generator=g)
    feats = centres[labels] + 0.01 * torch.randn(N_BANK, D_BANK, generator=g)
    q = centres[ql] + 0.01 * torch.randn(M_QUERY, D_BANK, generator=g)
    bank = _bank(feats.cuda(), labels, dtype, splits=(1200, 800))
    pred, _, counts = knn.knn_predict(q.cuda(), bank, (10, 20, 100), query_label=ql)
    assert counts.tolist() == [[M_QUERY, M_QUERY, M_QUERY]] * 3
    assert torch.equal(pred[:, :, 0].cpu(), ql.int().expand(3, -1))


# ---- 5. the evaluator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_evaluator_on_the_tiny_probe_model(bank_dtype):
    from simseg_amd.knn import KNNEvaluator, knn_predict
    from test_gpu_linear_probe import _batch, _build
    model, _ = _build(seed=3)
    ks = (1, 5, 20)                                                  # 20 > the 13 bank rows: the lists end in empty slots
    ev = KNNEvaluator(model, ks=ks, temperature=0.07, bank_dtype=bank_dtype)
    fit, held = [_batch(8, 41), _batch(5, 42)], [_batch(7, 43)]
    bank = ev.fit(fit)
    assert model.training and len(bank) == 13 and bank.dtype == bank_dtype and [o for _, o in bank.chunks()] == [0, 8]
    assert torch.equal(bank.labels.cpu(), torch.cat([b["label"] for b in fit]).int().cpu())
    # the bank rows: the float64 normalisation of the model's [cls] rows
    model.eval()
    with torch.no_grad():
        f = torch.cat([model.forward_image_feature(b["image"]) for b in fit])
    model.train()
    assert f.shape == (13, bank.dim) and not f.requires_grad
    f64 = f.double().cpu()
    want = f64 / f64.norm(dim=1, keepdim=True).clamp_min(1e-12)
    rows = torch.cat([c for c, _ in bank.chunks()]).double().cpu()
    # fp32 arithmetic: (D / 2 + 4) * 2^-24 relative to each element (the scale 1 / ||x|| carries the error of the sum of squares, the
    # square root, the division and the product).  A bf16 bank adds the rounding of an element of a unit row, |v| <= 1: at most half a
    # bf16 ulp below 1, 2^-9 - relative to the row's norm (1), not to the element: bf16's unit roundoff per element is 2^-8, which is
    # the tighter of the two for elements below 1/2, so the allowance is the smaller of the two.
    tol32 = (bank.dim / 2 + 4) * 2.0 ** -24
    slack = torch.zeros_like(want)
    if bank_dtype == torch.bfloat16:
        slack = (want.abs() * (2.0 ** -8 * (1 + tol32))).clamp_max(2.0 ** -9)
    excess = ((rows - want).abs() - slack).clamp_min(0.0)
    err = (excess / want.abs().clamp_min(1e-30)).max().item()
    print(f"bank rows ({bank_dtype}) vs the float64 normalisation: largest error {(rows - want).abs().max().item():.3e} absolute; beyond the "
          f"bf16 rounding allowance (largest {slack.max().item():.3e}): {err:.3e} relative (bound {tol32:.3e})")
    assert err <= tol32
    # the percentages: knn_predict on the same bank and features
    res = ev.evaluate(held)
    assert model.training and list(res) == list(ks) and all(set(v) == {"top1", "top5"} for v in res.values())
    _, _, counts = knn_predict(ev.features(held[0]["image"]), bank, ks, 0.07, query_label=held[0]["label"])
    for k, (n, h1, h5) in zip(ks, counts.tolist()):
        assert n == 7 and res[k] == {"top1": 100.0 * h1 / 7, "top5": 100.0 * h5 / 7}
    # feature_fn replaces the default feature
    calls = []
    ev2 = KNNEvaluator(model, ks=ks, bank_dtype=bank_dtype, feature_fn=lambda im: calls.append(im.shape[0]) or model.forward_image_feature(im))
    ev2.fit(fit)
    assert ev2.evaluate(held) == res and calls == [8, 5, 7]
