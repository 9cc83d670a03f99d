"""PAMR (pixel-adaptive mask refinement, Araslanov & Roth, CVPR 2020) stated twice in float64, and the seeded scenes its tests use.

pamr_np      the definition of include/simseg_hip.h (simseg_pamr) in numpy: clamped neighbour coordinates, integer sums for the standard
             deviation, softmax with the maximum subtracted, iters averaging steps.
pamr_torch   the published form: F.pad(mode="replicate") + a dilated conv2d that unfolds the 3x3 neighbourhood, difference, absolute
             value, mean over channels, softmax, std over the 9 D stacked samples.
The two share no code; tests/test_pamr_ref.py holds them to 1e-12 of each other, tests/test_gpu_pamr.py holds the kernels to pamr_np."""
import numpy as np
import torch
import torch.nn.functional as F

DILATIONS = (1, 2, 4, 8, 12, 24)
OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _neighbour(H, W, d, oy, ox):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.clip(yy + d * oy, 0, H - 1), np.clip(xx + d * ox, 0, W - 1)


def weights_np(rgb, dilations=DILATIONS):
    """rgb [H,W,3] uint8 -> w [8 D, H, W] float64 (taps dilation-major, OFFSETS order)."""
    H, W, _ = rgb.shape
    x = rgb.astype(np.int64)
    n = 9 * len(dilations)
    s, q = np.zeros((H, W, 3), np.int64), np.zeros((H, W, 3), np.int64)
    for d in dilations:
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                v = x[_neighbour(H, W, d, oy, ox)]
                s += v
                q += v * v
    sigma = np.sqrt((n * q - s * s).astype(np.float64) / (n * (n - 1)))
    logits = np.empty((8 * len(dilations), H, W), np.float64)
    for j, d in enumerate(dilations):
        for i, (oy, ox) in enumerate(OFFSETS):
            diff = np.abs(x - x[_neighbour(H, W, d, oy, ox)]).astype(np.float64)
            logits[8 * j + i] = -(diff / (1e-8 + 0.1 * sigma)).sum(-1) / 3.0
    e = np.exp(logits - logits.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def propagate_np(w, m, dilations=DILATIONS):
    """One step: w [8 D, H, W], m [K, H, W] -> [K, H, W]."""
    H, W = m.shape[-2:]
    out = np.zeros_like(m)
    for j, d in enumerate(dilations):
        for i, (oy, ox) in enumerate(OFFSETS):
            qy, qx = _neighbour(H, W, d, oy, ox)
            out += w[8 * j + i] * m[:, qy, qx]
    return out


def pamr_np(rgb, m0, dilations=DILATIONS, iters=10):
    """rgb [H,W,3] uint8, m0 [K,H,W] -> the refined maps [K,H,W] float64."""
    m = np.asarray(m0, np.float64).copy()
    if iters:
        w = weights_np(rgb, dilations)
        for _ in range(iters):
            m = propagate_np(w, m, dilations)
    return m


def _unfold(x, d):
    """x [C,H,W] float64 -> the dilated 3x3 neighbourhood [C,9,H,W], replicate padded."""
    C, H, W = x.shape
    xp = F.pad(x[None], [d, d, d, d], mode="replicate")[0]
    k = torch.eye(9, dtype=x.dtype).view(9, 1, 3, 3)
    return F.conv2d(xp[:, None], k, dilation=d)


def weights_torch(rgb, dilations=DILATIONS):
    x = torch.as_tensor(np.asarray(rgb), dtype=torch.float64).permute(2, 0, 1)
    nb = torch.cat([_unfold(x, d) for d in dilations], 1)                                   # [3, 9 D, H, W]
    std = nb.std(1, keepdim=True)                                                           # unbiased, over the 9 D samples
    keep = [9 * j + t for j in range(len(dilations)) for t in range(9) if t != 4]           # drop the centres
    aff = -(nb[:, keep] - x[:, None]).abs() / (1e-8 + 0.1 * std)
    return torch.softmax(aff.mean(0), 0)                                                    # [8 D, H, W]


def pamr_torch(rgb, m0, dilations=DILATIONS, iters=10):
    m = torch.as_tensor(np.asarray(m0), dtype=torch.float64).clone()
    if iters:
        w = weights_torch(rgb, dilations)
        taps = [t for t in range(9) if t != 4]
        for _ in range(iters):
            nb = torch.cat([_unfold(m, d)[:, taps] for d in dilations], 1)                  # [K, 8 D, H, W]
            m = (nb * w[None]).sum(1)
    return m.numpy()


def scene(H, W, K, seed):
    """-> (rgb [H,W,3] uint8, maps [K,H,W] float32 in [0,1]).  A checkerboard of two colours with period (13, 11) pixels and channel
    offsets (0, +20, -30) plus uniform integer noise in [-12, 12]; maps are uniform random values on the ceil(H/16) x ceil(W/16) patch
    grid, upsampled x16 and cropped (per-pixel random values for an image of at most one patch)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    board = ((yy // 13 + xx // 11) % 2).astype(np.int64)
    base = np.where(board[..., None] == 0, 70, 170) + np.array([0, 20, -30])
    rgb = np.clip(base + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
    if H <= 16 and W <= 16:
        maps = rng.random((K, H, W))
    else:
        grid = rng.random((K, -(-H // 16), -(-W // 16)))
        maps = np.repeat(np.repeat(grid, 16, 1), 16, 2)[:, :H, :W]
    return rgb, np.ascontiguousarray(maps.astype(np.float32))
