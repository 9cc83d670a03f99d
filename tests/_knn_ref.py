"""float64 statement of the weighted k-NN vote, written from the comment on simseg_knn_vote_rows in include/simseg_hip.h; it shares no
code with the device path.  Also the generator of the tests' cases and the error allowance.

Per row and k: the neighbours are the first n = min(k, valid) entries (valid = entries before the first idx < 0),
w_j = exp((s_j - s_0) / float64(float32(T))), vote(c) = sum of w_j with label c, classes with a neighbour ranked by vote descending and
equal votes by ascending class; the first five are reported, -1 / 0 beyond.  `gap` is the smallest relative gap (v_i - v_{i+1}) / v_i
among the first six ranked classes (inf when the row has fewer than two): below it a rounding of the fp32 votes may swap two classes."""
import functools

import numpy as np

TOP = 5
T_DEFAULT = 0.07
KS = (1, 10, 20, 128)
SEEDS, CLASSES = (0, 1, 2), (7, 1000)
GAP_MIN = 1e-4                  # rows whose reference gap is below this are left out of the pred comparison (more than 4 x the allowance)
NEAR_TIE_CAP = 0.02             # at most this share of a case's rows may be left out


def allowance(max_x, k):
    """Relative error allowed on a vote: the exponent (s_j - s_0) / T takes two fp32 roundings and expf at most 2 ulp - 3 |x| + 2 units
    of 2^-24 on a weight - and the sequential sum of k terms (k - 1) roundings; tests allow twice that."""
    return 2.0 * (3.0 * max_x + 2.0 + (k - 1)) * 2.0 ** -24


def vote_ref(score, idx, gallery_label, ks, temperature=T_DEFAULT):
    """score [M, K] float32, idx [M, K] integer, gallery_label [N] integer -> (pred [nk, M, 5] int64, vote [nk, M, 5] float64,
    gap [nk, M] float64)."""
    score = np.asarray(score)
    idx = np.asarray(idx).astype(np.int64)
    gl = np.asarray(gallery_label).astype(np.int64)
    assert score.dtype == np.float32
    M, K = score.shape
    T = np.float64(np.float32(temperature))
    pred = np.full((len(ks), M, TOP), -1, dtype=np.int64)
    vote = np.zeros((len(ks), M, TOP), dtype=np.float64)
    gap = np.full((len(ks), M), np.inf, dtype=np.float64)
    for m in range(M):
        empty = np.flatnonzero(idx[m] < 0)
        valid = int(empty[0]) if empty.size else K
        if valid == 0:
            continue
        s = score[m, :valid].astype(np.float64)
        w = np.exp((s - s[0]) / T)
        lab = gl[idx[m, :valid]]
        for ki, k in enumerate(ks):
            n = min(k, valid)
            classes, inv = np.unique(lab[:n], return_inverse=True)
            v = np.zeros(classes.size, dtype=np.float64)
            np.add.at(v, inv, w[:n])
            order = np.lexsort((classes, -v))                  # vote descending, then class ascending
            top = order[:TOP]
            pred[ki, m, :top.size] = classes[top]
            vote[ki, m, :top.size] = v[top]
            r = v[order[:TOP + 1]]
            if r.size >= 2:
                with np.errstate(divide="ignore", invalid="ignore"):
                    g = np.where(r[:-1] > 0, (r[:-1] - r[1:]) / r[:-1], 0.0)
                gap[ki, m] = g.min()
    return pred, vote, gap


def make_case(seed, C, offset=0):
    """The generator of the float64 test: 300 rows of 128 descending scores in [-0.2, 0.9) and labels in [0, C), taken as indices (plus
    `offset`) into a gallery whose row offset + c has label c.  -> dict(score, idx int32, gallery_label int32, label)."""
    rng = np.random.default_rng(seed)
    score = -np.sort(-rng.uniform(-0.2, 0.9, (300, 128)).astype(np.float32), axis=1)
    label = rng.integers(0, C, (300, 128))
    gallery_label = np.concatenate([np.full(offset, C - 1, dtype=np.int32), np.arange(C, dtype=np.int32)])
    query_label = rng.integers(0, C, 300).astype(np.int32)
    return dict(score=score, idx=(label + offset).astype(np.int32), gallery_label=gallery_label, label=label, query_label=query_label)


@functools.lru_cache(maxsize=None)
def case_with_ref(seed, C, offset=0):
    """make_case plus its reference (pred, vote, gap) for KS at T_DEFAULT, computed once per process and shared: treat as read-only."""
    c = make_case(seed, C, offset)
    c["pred"], c["vote"], c["gap"] = vote_ref(c["score"], c["idx"], c["gallery_label"], KS, T_DEFAULT)
    return c


def host_counts(pred, query_label):
    """[nk, 3] {rows, top-1 hits, top-5 hits} from a pred [nk, M, 5] array and the query labels [M]."""
    pred = np.asarray(pred)
    ql = np.asarray(query_label)[None, :, None]
    hit = (pred == ql) & (pred >= 0)
    return np.stack([np.full(pred.shape[0], pred.shape[1]), hit[:, :, 0].sum(1), hit.any(2).sum(1)], axis=1).astype(np.int64)
