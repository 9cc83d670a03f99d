"""Host side of the weighted k-NN evaluation: the float64 reference's own properties, the C ABI entry and its argument checks (all made
before any device work, so they answer without a GPU), FeatureBank's bookkeeping and the refusals of simseg_amd.knn."""
import ctypes

import numpy as np
import pytest
import torch

from _knn_ref import CLASSES, GAP_MIN, KS, NEAR_TIE_CAP, SEEDS, allowance, case_with_ref, host_counts, vote_ref


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_reference_k1_predicts_the_first_label_with_vote_one():
    c = case_with_ref(0, 7)
    assert KS[0] == 1
    assert np.array_equal(c["pred"][0, :, 0], c["label"][:, 0]) and (c["vote"][0, :, 0] == 1.0).all()
    assert (c["pred"][0, :, 1:] == -1).all() and (c["vote"][0, :, 1:] == 0.0).all()


def test_reference_prefix_property():
    """The answer for k is the answer of a search that returned only k columns."""
    c = case_with_ref(1, 7)
    for ki, k in enumerate(KS):
        p, v, g = vote_ref(c["score"][:, :k], c["idx"][:, :k], c["gallery_label"], (k,))
        assert np.array_equal(p[0], c["pred"][ki]) and np.array_equal(v[0], c["vote"][ki]) and np.array_equal(g[0], c["gap"][ki])


def test_reference_ties_go_to_the_lower_class_and_tails_end_the_list():
    score = np.array([[0.5, 0.5, 0.25, 0.25], [0.5, 0.4, -np.inf, -np.inf], [-np.inf] * 4], dtype=np.float32)
    idx = np.array([[0, 1, 2, 3], [3, 2, -1, -1], [-1] * 4])
    gl = np.array([9, 3, 3, 9])
    pred, vote, gap = vote_ref(score, idx, gl, (2, 4))
    assert pred[1, 0].tolist() == [3, 9, -1, -1, -1] and vote[1, 0, 0] == vote[1, 0, 1] and gap[1, 0] == 0.0
    assert pred[0, 0].tolist() == [3, 9, -1, -1, -1] and vote[0, 0, 0] == 1.0 == vote[0, 0, 1]
    assert pred[1, 1].tolist() == [9, 3, -1, -1, -1] and np.array_equal(pred[1, 1], pred[0, 1])      # k = 4 with two valid entries
    assert vote[1, 1, 1] == np.exp((np.float64(np.float32(0.4)) - 0.5) / np.float64(np.float32(0.07)))
    assert (pred[:, 2] == -1).all() and (vote[:, 2] == 0).all() and np.isinf(gap[:, 2]).all()
    assert host_counts(pred, [3, 3, 3]).tolist() == [[3, 1, 2], [3, 1, 2]]


def test_allowance_for_the_issue_inputs():
    assert abs(allowance(1.1 / 0.07, 128) - 2.1e-5) < 5e-7 and 4 * allowance(1.1 / 0.07, 128) < GAP_MIN


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("seed", SEEDS)
def test_near_tie_rows_stay_within_the_cap(seed, C):
    gap = case_with_ref(seed, C)["gap"]
    for ki, k in enumerate(KS):
        out = int((gap[ki] < GAP_MIN).sum())
        assert out <= NEAR_TIE_CAP * gap.shape[1], (seed, C, k, out)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry():
    from simseg_amd import lib
    protos = lib.parse_header()
    assert "simseg_knn_vote_rows" in protos
    names = [n for _, n in protos["simseg_knn_vote_rows"][1]]
    assert names == ["score", "idx", "gallery_label", "query_label", "M", "N", "K", "ks", "nk", "temperature", "pred", "vote", "counts", "stream"]
    assert hasattr(lib.load(), "simseg_knn_vote_rows")


def _vote(M=1, N=10, K=8, ks=(1, 4), T=0.07, ptrs=None, qlabel=None, counts=None):
    from simseg_amd import lib
    l = lib.load()
    arr = (ctypes.c_int32 * max(1, len(ks)))(*ks) if ks is not None else None
    rc = l.simseg_knn_vote_rows(ptrs, ptrs, ptrs, qlabel, M, N, K, arr, len(ks) if ks is not None else 1, T, ptrs, ptrs, counts, None)
    return rc, l.simseg_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(K=0), "K = 0 outside 1..128"),
    (dict(K=129, ks=(1, 129)), "K = 129 outside 1..128"),
    (dict(ks=()), "0 values of k"),
    (dict(ks=(1, 2, 3, 4, 5)), "5 values of k"),
    (dict(ks=None), "null pointer (ks)"),
    (dict(ks=(0, 4)), "strictly ascending and >= 1 (ks[0] = 0)"),
    (dict(ks=(4, 4)), "strictly ascending and >= 1 (ks[1] = 4)"),
    (dict(ks=(5, 2)), "strictly ascending"),
    (dict(ks=(1, 9)), "ks[1] = 9 exceeds K = 8"),
    (dict(T=0.0), "temperature 0 is not a finite positive"),
    (dict(T=-1.0), "temperature -1 is not a finite positive"),
    (dict(T=float("inf")), "temperature inf"),
    (dict(T=float("nan")), "nan is not a finite positive"),
    (dict(M=-1), "M = -1, N = 10"),
    (dict(N=0), "M = 1, N = 0"),
    (dict(N=2 ** 31), "does not fit the int32 indices"),
    (dict(), "knn_vote_rows: null pointer"),
])
def test_argument_checks_answer_without_a_gpu(kw, msg):
    rc, err = _vote(**kw)
    assert rc != 0 and err.startswith("knn_vote_rows: ") and msg in err, err


def test_empty_call_returns_before_the_pointer_checks():
    rc, _ = _vote(M=0)
    assert rc == 0


def test_counts_are_required_with_query_labels():
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc, err = _vote(ptrs=p, qlabel=p, counts=None)            # refused on the host: nothing is launched
    assert rc != 0 and "null pointer (counts" in err


# ---- simseg_amd.knn and ops.knn_vote ------------------------------------------------------------------------------------------------
def test_feature_bank_offsets_and_labels_over_unequal_chunks(monkeypatch):
    from simseg_amd import knn
    monkeypatch.setattr(knn, "normalize_rows", lambda x: torch.nn.functional.normalize(x.float(), dim=1, eps=1e-12))
    bank = knn.FeatureBank(16)
    g = torch.Generator().manual_seed(0)
    sizes, dtypes = (5, 1, 11), (torch.int64, torch.uint8, torch.int32)
    feats = [torch.randn(n, 16, generator=g) for n in sizes]
    labs = [torch.randint(0, 100, (n,), generator=g).to(dt) for n, dt in zip(sizes, dtypes)]
    for f, l in zip(feats, labs):
        bank.add(f, l)
    bank.add(torch.zeros(0, 16), torch.zeros(0, dtype=torch.int64))          # an empty batch adds no chunk
    assert len(bank) == 17 and bank.dim == 16 and bank.dtype == torch.float32
    got = list(bank.chunks())
    assert [o for _, o in got] == [0, 5, 6] and [c.shape[0] for c, _ in got] == list(sizes)
    assert bank.labels.dtype == torch.int32 and torch.equal(bank.labels, torch.cat([l.int() for l in labs]))
    for (c, _), f in zip(got, feats):
        assert torch.equal(c, torch.nn.functional.normalize(f, dim=1, eps=1e-12))
    bank.add(feats[0], labs[0])                                               # the label vector follows a later add
    assert len(bank) == 22 and torch.equal(bank.labels[17:], labs[0].int()) and list(bank.chunks())[-1][1] == 17


def test_refusals():
    from simseg_amd import knn, ops
    with pytest.raises(ValueError, match="D % 8"):
        knn.FeatureBank(20)
    with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
        knn.FeatureBank(16, torch.float16)
    bank = knn.FeatureBank(16)
    q = torch.zeros(3, 16)
    with pytest.raises(ValueError, match="TOPK_MAX"):
        knn.knn_predict(q, bank, ks=(10, 200))
    with pytest.raises(ValueError, match="TOPK_MAX"):
        knn.KNNEvaluator(None, ks=(129,))
    with pytest.raises(ValueError, match="empty"):
        knn.knn_predict(q, bank)
    with pytest.raises(ValueError, match="empty"):
        bank.labels
    for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.bool), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(TypeError, match="integer class labels"):
            bank.add(q, bad)
    with pytest.raises(TypeError, match="integer class labels"):
        bank.add(q, [0, 1, 2])
    with pytest.raises(ValueError, match=r"\[0, 2\^31\)"):
        bank.add(q, torch.tensor([0, -1, 2]))
    with pytest.raises(ValueError, match=r"\[0, 2\^31\)"):
        bank.add(q, torch.tensor([0, 2 ** 31, 2]))
    with pytest.raises(ValueError, match="4 labels for 3 rows"):
        bank.add(q, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[B, 16\]"):
        bank.add(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64))
    assert len(bank) == 0
    for ks in ((), (1, 2, 3, 4, 5), (0, 1), (3, 3), (5, 2)):
        with pytest.raises(ValueError, match="knn_vote"):
            ops.check_knn_ks(ks)
    with pytest.raises(ValueError, match="exceeds the K = 8"):
        ops.check_knn_ks((1, 9), 8)
    assert ops.check_knn_ks([1, 10, 20, 128]) == (1, 10, 20, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_vote(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64), (1,))
