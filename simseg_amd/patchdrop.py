"""Patch dropout of the image tower (timm's PatchDropout with ordered=True and one prefix token; FLIP, Li et al., CVPR'23; open_clip's
--force-patch-dropout): in train() mode every image keeps a random K of its N patch tokens and the tower runs on [cls] + the kept ones.

The draw is a pure function of (seed, b, N, K) - include/simseg_hip.h, simseg_patch_keep_sample:
  key(b, n) = hash_u32(seed, b * N + n)            (csrc/common.h; pipeline.hash_u32_ref is its numpy twin)
  image b keeps the K positions with the smallest keys, equal keys going to the lower n; keep[b] lists them ascending;
  inv[b, n] = the j with keep[b, j] == n, or -1.
`sample_keep_ref` states that in numpy, `sample_keep` runs it on the device (one block per image, no sort, no host read)."""
import numpy as np

MAX_PATCHES = 4096          # keys of one image in the sampler's LDS


def _check_rate(rate):
    rate = float(rate)
    if not 0.0 <= rate < 1.0:          # (also refuses nan)
        raise ValueError(f"patch_drop_rate must satisfy 0 <= rate < 1, got {rate}")
    return rate


def num_keep(N, rate):
    """Tokens kept out of N at drop rate `rate`: max(1, int(N * (1 - rate))), timm's count."""
    rate = _check_rate(rate)
    N = int(N)
    if N < 1:
        raise ValueError(f"num_keep: N must be positive, got {N}")
    return max(1, int(N * (1.0 - rate)))


def _check_shape(B, N, K):
    B, N, K = int(B), int(N), int(K)
    if not 1 <= K <= N <= MAX_PATCHES:
        raise ValueError(f"patch dropout: need 1 <= K <= N <= {MAX_PATCHES}, got K = {K}, N = {N}")
    if B < 1 or B * N >= 1 << 31:
        raise ValueError(f"patch dropout: need B >= 1 and B * N < 2^31 (the keys of a draw are distinct only below that), got B = {B}, N = {N}")
    return B, N, K


def sample_keep_ref(B, N, K, seed):
    """-> (keep int32 [B, K], inv int32 [B, N]) as numpy arrays: the statement the device sampler is tested against."""
    from .pipeline import hash_u32_ref
    B, N, K = _check_shape(B, N, K)
    keys = hash_u32_ref(int(seed) & 0xFFFFFFFFFFFFFFFF, np.arange(B * N, dtype=np.uint64)).reshape(B, N)
    order = np.argsort(keys, axis=1, kind="stable")              # (stable: equal keys go to the lower n)
    keep = np.sort(order[:, :K], axis=1).astype(np.int32)
    inv = np.full((B, N), -1, dtype=np.int32)
    inv[np.arange(B)[:, None], keep] = np.arange(K, dtype=np.int32)[None, :]
    return keep, inv


def sample_keep(B, N, K, seed, device):
    """-> (keep int32 [B, K], inv int32 [B, N]) device tensors, equal to sample_keep_ref's; nothing is read back to the host."""
    from . import ops
    B, N, K = _check_shape(B, N, K)
    return ops.patch_keep_sample(B, N, K, int(seed), device)
