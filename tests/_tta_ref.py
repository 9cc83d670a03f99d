"""NumPy restatement (float64) of the multi-scale / flip test-time augmentation contract (DESIGN.md "Multi-scale and flip test-time
augmentation"; include/simseg_hip.h simseg_slide_stitch_multi).  It shares no code with the device path: only segpost.slide_windows, the
window placement both sides are defined on."""
import math

import numpy as np


def pass_size(H, W, s):
    return max(1, int(math.floor(s * H + 0.5))), max(1, int(math.floor(s * W + 0.5)))


def nearest_index(L, Lp):
    """For every base index 0 .. L-1 the sampled index of a pass of extent Lp: min(((2i + 1) Lp) // (2L), Lp - 1), Python integers."""
    return np.array([min(((2 * i + 1) * Lp) // (2 * L), Lp - 1) for i in range(L)], dtype=np.int64)


def stitch_ref(sim, offs, H, W, win):
    """sim [nwin, n*n] (one class of one image's windows, window order) -> S [H, W] float64: per pixel the sum over the covering windows,
    in window order, of their cell ((y - y0) // 16, (x - x0) // 16), divided once by their number."""
    n = win // 16
    acc = np.zeros((H, W), np.float64)
    cnt = np.zeros((H, W), np.float64)
    for w, (y0, x0) in enumerate(offs):
        h, ww = min(win, H - y0), min(win, W - x0)
        up = sim[w].astype(np.float64).reshape(n, n).repeat(16, 0).repeat(16, 1)
        acc[y0:y0 + h, x0:x0 + ww] += up[:h, :ww]
        cnt[y0:y0 + h, x0:x0 + ww] += 1
    assert cnt.min() >= 1
    return acc / cnt


def fuse_ref(maps, flips, H, W):
    """maps[p] = S_p [H_p, W_p] (stitch_ref of the pass image, which is the MIRRORED image for a flipped pass) -> F [H, W] float64:
    S_p un-mirrored when flips[p], sampled at the nearest index, summed in pass order, divided once by the number of passes."""
    F = np.zeros((H, W), np.float64)
    for S, flip in zip(maps, flips):
        if flip:
            S = S[:, ::-1]
        F = F + S[nearest_index(H, S.shape[0])][:, nearest_index(W, S.shape[1])]
    return F / len(maps)


def normalise_ref(F):
    """-> (prob float64, mask uint8, (min, max))."""
    mn, mx = F.min(), F.max()
    prob = (F - mn) / (mx - mn)
    return prob, np.where(prob > 0.5, 255, 0).astype(np.uint8), (mn, mx)


def scores_ref(pass_scores):
    """pass_scores[p] = [nwin_p, C] window scores of one image -> [C] float64: per pass the window-order mean, summed over the passes in
    pass order, divided once."""
    tot = np.zeros(pass_scores[0].shape[1], np.float64)
    for sc in pass_scores:
        acc = np.zeros(sc.shape[1], np.float64)
        for row in sc:
            acc = acc + row.astype(np.float64)
        tot = tot + acc / sc.shape[0]
    return tot / len(pass_scores)


# ---- the seeded kernel-level case of tests/test_gpu_tta.py (its reference is computed once and shared) ----------------------------------
WIN, STRIDE, C, K = 32, 16, 7, 5
SIZES = [(40, 56), (32, 32), (19, 45), (75, 50)]
PASSES = [(1.0, False), (1.0, True), (0.5, False), (1.5, True), (0.75, True)]
CAND = [[3, -1, 5, 0, 6], [1, 2, -1, -1, 4], [-1, -1, -1, -1, -1], [6, 5, 4, 3, 2]]
_CASE = {}


def fusion_case(seed=20):
    """-> dict(sizes[p] per-pass image sizes, sims[p] fp32 [Nw_p, n*n, C] in [-1, 1), flips, cand, ref[(b, k)] = (prob, mask, (min, max),
    F) for the visited slots)."""
    if seed in _CASE:
        return _CASE[seed]
    from simseg_amd import segpost
    rng = np.random.default_rng(seed)
    n = WIN // 16
    sizes = [[pass_size(H, W, s) for H, W in SIZES] for s, _ in PASSES]
    flips = [f for _, f in PASSES]
    offs = [[segpost.slide_windows(h, w, WIN, STRIDE) for h, w in per] for per in sizes]
    sims = [rng.uniform(-1, 1, (sum(len(o) for o in per), n * n, C)).astype(np.float32) for per in offs]
    ref = {}
    for b, (H, W) in enumerate(SIZES):
        for k, c in enumerate(CAND[b]):
            if c < 0:
                continue
            maps = []
            for p in range(len(PASSES)):
                w0 = sum(len(o) for o in offs[p][:b])
                maps.append(stitch_ref(sims[p][w0:w0 + len(offs[p][b]), :, c], offs[p][b], *sizes[p][b], WIN))
            F = fuse_ref(maps, flips, H, W)
            ref[(b, k)] = normalise_ref(F) + (F,)
    _CASE[seed] = {"sizes": sizes, "sims": sims, "flips": flips, "cand": CAND, "ref": ref, "offs": offs}
    return _CASE[seed]
