#!/usr/bin/env python
"""Per-block timeline of the split-K weight-gradient GEMM (dW = dY^T . X, 256x256 ping-pong kernel, fp32 atomics): prologue / K loop /
epilogue (the atomic adds) of every block and the K loop's time per 64-deep K-tile.
    argv: [M N K]                  one problem as launched per GEMM (output M x N, contraction K)
    argv: group ROWS [SLICES] [D]  a transformer block's four problems (fc2, fc1, proj, qkv at width D = 768) as ONE grouped launch
                                   (ops.wgrad_group; SLICES defaults to the planner's choice); its adds are issued from the accumulator layout."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simseg_amd import ops  # noqa: E402
from simseg_amd.lib import call, ptr  # noqa: E402
from simseg_amd.towers import _splitk  # noqa: E402


def trace(launch, blocks):
    buf = torch.zeros(max(blocks, 4096) * 9 + 64, device="cuda", dtype=torch.int64)      # (5 + 4 stamps per block; room for any fallback launch)
    for _ in range(3):
        launch()
    call("simseg_debug_gemm_trace", ptr(buf))
    launch()
    call("simseg_debug_gemm_trace", None)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:blocks * 5].reshape(blocks, 5), e0.elapsed_time(e1) / 10 * 1e3


def report(t, ks, untraced_us):
    ok = t[:, 0] > 0
    us = (t[:, :4] - t[ok, 0].min()) / 100.0
    pro, loop, epi = us[:, 1] - us[:, 0], us[:, 2] - us[:, 1], us[:, 3] - us[:, 2]
    print(f"traced {int(ok.sum())} of {len(t)} blocks; {untraced_us:.1f} us per launch untraced")
    print(f"launch span {us[ok, 3].max():.1f} us; block start spread {us[ok, 0].max():.1f} us; per block: prologue {pro[ok].mean():.2f}, K loop {loop[ok].mean():.2f} "
          f"(p10 {np.percentile(loop[ok], 10):.1f}, p90 {np.percentile(loop[ok], 90):.1f}) = {loop[ok].mean() / ks:.3f} us per K-tile, epilogue (atomics) mean {epi[ok].mean():.2f}, "
          f"median {np.median(epi[ok]):.2f}, p90 {np.percentile(epi[ok], 90):.2f} us")
    print(f"block end times: p10 {np.percentile(us[ok, 3], 10):.1f}  p50 {np.percentile(us[ok, 3], 50):.1f}  p90 {np.percentile(us[ok, 3], 90):.1f}  max {us[ok, 3].max():.1f} us")


if len(sys.argv) > 1 and sys.argv[1] == "group":
    rows = int(sys.argv[2])
    D = int(sys.argv[4]) if len(sys.argv) > 4 else 768
    shapes = [(D, 4 * D), (4 * D, D), (D, D), (3 * D, D)]
    tiles = [(o // 256) * (i // 256) for o, i in shapes]
    nk = rows // 64
    sk = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) > 0 else ops.wgrad_group_plan(tiles, nk)
    ks = (nk + sk - 1) // sk
    z = (nk + ks - 1) // ks
    probs = [(torch.randn(rows, o, device="cuda").bfloat16(), torch.randn(rows, i, device="cuda").bfloat16(), torch.zeros(o, i, device="cuda")) for o, i in shapes]
    t, us_launch = trace(lambda: ops.wgrad_group(probs, slices=sk), sum(tiles) * z)
    assert ops.wgrad_group_last() == 4, "the group fell back to per-problem launches"
    print(f"grouped dW {shapes}, rows={rows}: {sum(tiles)} tiles x {z} K-ranges of {ks} K-tiles = {sum(tiles) * z} blocks")
    report(t, ks, us_launch)
else:
    M, N, K = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (2304, 768, 100864)
    dy = torch.randn(K, M, device="cuda").bfloat16()
    x = torch.randn(K, N, device="cuda").bfloat16()
    out = torch.zeros(M, N, device="cuda")
    sk = _splitk(M, N, K)
    kw = dict(trans_a=True, trans_b=True, out=out, accumulate=True, splitk=sk)
    # the slice count the library derives for the 256x256 kernel (dispatch_h16): one round of 256 blocks, slices at least 16 K-tiles deep
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    nk = K // 64
    sk256 = 256 // tiles
    if nk // sk256 < 16 and nk >= 64:
        sk256 = nk // 16
    ks = (nk + sk256 - 1) // sk256
    z = (nk + ks - 1) // ks
    t, us_launch = trace(lambda: ops.gemm(dy, x, **kw), tiles * z)
    print("kernel:", ops.gemm_last_variant())
    print(f"dW {M}x{N}, K={K}: {tiles} tiles x {z} K-ranges of {ks} K-tiles = {tiles * z} blocks")
    report(t, ks, us_launch)
