"""Tensor-level wrappers over the C ABI (include/simseg_hip.h).  PyTorch supplies device memory and the stream;
all arithmetic runs in libsimseg_hip.so.  No autograd here (see autograd.py) and no CPU fallback."""
import ctypes
import os
import threading

import torch

from .lib import call, ptr, require_gpu, stream, raw

F32, BF16 = 0, 1
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: BF16}       # code 1 = "the 16-bit type": bf16, or fp16 while the call's tensors are fp16 (lib.call)
HALF_TYPES = (torch.bfloat16, torch.float16)


def dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"simseg_amd supports fp32, bf16 and fp16 tensors, got {t.dtype}")


def _c(t):
    if t is not None and not t.is_contiguous():
        raise ValueError("simseg_amd ops need contiguous tensors")
    return t


# The library's kernel selectors are thread-local (include/simseg_hip.h: the compute entry points are re-entrant), and autograd runs
# backward on its own threads: the selection made here is kept in Python and pushed to whichever thread launches next.
_VARIANT = {"gemm": int(os.environ.get("SIMSEG_GEMM_VARIANT", "0")), "attention": int(os.environ.get("SIMSEG_ATTN_VARIANT", "0"))}     # (env: A/B runs)
_PUSHED = threading.local()


def _push_variant(kind):
    want = _VARIANT[kind]
    if getattr(_PUSHED, kind, 0) != want:
        call(f"simseg_set_{kind}_variant", want)
        setattr(_PUSHED, kind, want)


def set_gemm_variant(v):
    """0 auto, 1 = 128x128 register-staged kernel, 3 = 256x256 ping-pong kernel (one tile per block), 4 = small-problem kernel, 5 = 128x128
    tile on the four-stage direct-to-LDS ring, 10 = persistent 256x256 ping-pong kernel - each wherever it applies; a call it does not
    apply to is dispatched as under 0.  Every value selects between production kernels; any other value raises and leaves the previous
    selection in force (tests / benchmarks only)."""
    old, _VARIANT["gemm"] = _VARIANT["gemm"], int(v)
    try:
        _push_variant("gemm")
    except Exception:
        _VARIANT["gemm"] = old     # a value the library rejects must not stay: every later launch would raise again
        raise


def set_attention_variant(v):
    """0 auto (bf16 sequences of <= 256 tokens on the resident kernels, their backward as one kernel; unmasked 16-bit sequences of >= 512
    tokens on the 64-queries-per-wave forward, small launches on its one-query-block form), 1 = the streaming ring kernels wherever they
    apply, 6 / 7 = the long-sequence forward with one / two query blocks per wave whatever the launch size (unmasked sequences of >= 65
    tokens).  Every value selects between production kernels; any other value raises and leaves the previous selection in force
    (tests / benchmarks only)."""
    old, _VARIANT["attention"] = _VARIANT["attention"], int(v)
    try:
        _push_variant("attention")
    except Exception:
        _VARIANT["attention"] = old     # a value the library rejects must not stay: every later launch would raise again
        raise


PROFILE = None   # bench.py sets this to a list to time every GEMM launch with events on the launch stream


def gemm(a, b, *, trans_a=False, trans_b=False, out=None, out_dtype=None, alpha=1.0, bias=None, rowscale=None,
         residual=None, act=0, aux=None, aux_out=None, row_group=0, res_mod=False, accumulate=False, splitk=1,
         drop_seed=0, drop_p=0.0, out_rows=None, colsum=None):
    """C = epilogue(alpha * op(a) @ op(b)); a: [M,K] ([K,M] if trans_a); b: [N,K] ([K,N] if trans_b)."""
    require_gpu(a, b)
    _c(a); _c(b)
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N = b.shape[1] if trans_b else b.shape[0]
    kb = b.shape[0] if trans_b else b.shape[1]
    if kb != K:
        raise ValueError(f"gemm: inner dims differ ({K} vs {kb})")
    if act in (7, 8):       # the 8-bit tile-blocked derivative image (include/simseg_hip.h): an opaque [M, N] byte tensor
        t8 = aux_out if act == 7 else aux
        if t8 is None or t8.dtype != torch.uint8 or t8.numel() < a.shape[0] * (b.shape[1] if trans_b else b.shape[0]):
            raise TypeError("gemm: act 7 / 8 take the derivative image as a uint8 tensor of M x N bytes")
    if a.dtype != b.dtype or (aux is not None and act != 8 and aux.dtype not in (a.dtype, torch.float32)):
        raise TypeError(f"gemm: operands of different types ({a.dtype}, {b.dtype}{'' if aux is None else ', aux ' + str(aux.dtype)}): bf16 and fp16 do not mix in one call")
    if out is None:
        rows = out_rows if out_rows is not None else M
        out = torch.empty(rows, N, device=a.device, dtype=out_dtype or a.dtype)
    _c(out)
    ldr = residual.shape[-1] if residual is not None else 0
    _push_variant("gemm")
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("simseg_gemm", ptr(a), ptr(b), ptr(out), M, N, K, a.shape[1], b.shape[1], out.shape[-1], dt(a), dt(out),
         int(trans_a), int(trans_b), float(alpha), ptr(_c(bias)), ptr(_c(rowscale)), ptr(_c(residual)), ldr, int(act),
         ptr(_c(aux)), ptr(_c(aux_out)), int(row_group), int(res_mod), int(accumulate), int(splitk), int(drop_seed),
         float(drop_p), ptr(colsum), stream())
    if PROFILE is not None:
        e1.record()
        kind = ("f32" if a.dtype == torch.float32 else "bf16") + "_" + ("t" if trans_a else "n") + ("n" if trans_b else "t")
        kind += "_o32" if out.dtype == torch.float32 else "_o16"
        kind += {1: "", 3: "_P", 4: "_S", 5: "_R", 10: "_Q"}[raw("simseg_gemm_last_variant")]      # the kernel the library actually launched
        PROFILE.append((kind, 2.0 * M * N * K, e0, e1))
    return out


def gemm_last_variant():
    return raw("simseg_gemm_last_variant")


WGRAD_EPILOGUE_KTILES = 8      # a block's atomic epilogue in units of its K loop's time per K-tile (13-15 us against 1.6-1.8 us, profiles/r4_wgrad_block_timeline.txt)


def wgrad_group_plan(tiles, nk, cus=256):
    """Slice count of a grouped split-K weight-gradient launch: `tiles` = the 256x256 output tiles of each problem, nk = 64-row K-tiles of
    the shared contraction.  The launch runs ceil(sum(tiles) * sk / cus) rounds of blocks, each ceil(nk / sk) K-tiles of K loop plus one
    atomic epilogue: the sk that minimises rounds x (K-tiles + WGRAD_EPILOGUE_KTILES), among those that leave a slice at least 16
    K-tiles (sk = 1 always allowed); ties go to the smaller sk.  (Without the epilogue term the count of K-tiles alone prefers many thin
    slices - 26 at ViT-B's 1576 K-tiles, 671 against 678 K-tiles per CU - and pays for them with 26 adders per output tile.)"""
    total = int(sum(tiles))
    nk = int(nk)
    best, best_cost = 1, None
    for sk in range(1, max(1, nk // 16) + 1):
        cost = -(-total * sk // cus) * (-(-nk // sk) + WGRAD_EPILOGUE_KTILES)
        if best_cost is None or cost < best_cost:
            best, best_cost = sk, cost
    return best


_WG_LAST = threading.local()


def wgrad_group_last():
    """How many problems this thread's last wgrad_group() launched as ONE kernel (0: it fell back to per-problem GEMMs)."""
    return getattr(_WG_LAST, "n", 0)


def wgrad_group(problems, slices=None):
    """dW_i += dy_i^T . x_i for a list of (dy_i [rows, out_i], x_i [rows, in_i], dW_i [out_i, in_i] fp32) over the same rows - a
    transformer block's weight gradients - as one split-K launch (simseg_gemm_wgrad_group); per-problem split-K GEMMs when the group is
    not eligible.  slices=None: wgrad_group_plan's choice."""
    problems = list(problems)
    if not problems:
        return
    rows = problems[0][0].shape[0]
    ok = 1 <= len(problems) <= 8
    for dy, x, out in problems:
        require_gpu(dy, x, out)
        _c(dy); _c(x); _c(out)
        if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0] or tuple(out.shape) != (dy.shape[1], x.shape[1]) or out.dtype != torch.float32:
            raise ValueError("wgrad_group: need dy [rows, out], x [rows, in] and an fp32 dW [out, in]")
        if dy.dtype != x.dtype:
            raise TypeError(f"wgrad_group: operands of different types ({dy.dtype}, {x.dtype})")
        ok = ok and dy.shape[0] == rows and dy.dtype in HALF_TYPES and dy.dtype == problems[0][0].dtype
    nk = rows // 64
    if slices is None:
        slices = wgrad_group_plan([(dy.shape[1] // 256) * (x.shape[1] // 256) for dy, x, _ in problems], nk)
    _push_variant("gemm")
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    grouped = 0
    if ok:
        desc = []
        for dy, x, out in problems:
            desc += [ptr(dy), ptr(x), ptr(out), dy.shape[1], x.shape[1], dy.shape[1], x.shape[1], x.shape[1]]
        call("simseg_gemm_wgrad_group", (ctypes.c_int64 * len(desc))(*desc), len(problems), rows, int(slices), stream())
        grouped = raw("simseg_wgrad_group_last")
    _WG_LAST.n = grouped
    if not grouped:
        for dy, x, out in problems:
            t128 = -(-dy.shape[1] // 128) * -(-x.shape[1] // 128)       # (the slice count the per-problem dispatch is tuned for: 1024 blocks of 128x128)
            sk = max(1, min(-(-dy.shape[0] // 64), -(-1024 // t128), 64))
            if dy.dtype == torch.float32:        # (the fp32 kernel is row.row only)
                gemm(transpose_f32(dy), transpose_f32(x), out=out, accumulate=True, splitk=sk)
            else:
                gemm(dy, x, trans_a=True, trans_b=True, out=out, accumulate=True, splitk=sk)
        return
    if PROFILE is not None:
        e1.record()
        PROFILE.append(("bf16_tn_o32_P", sum(2.0 * dy.shape[1] * x.shape[1] * rows for dy, x, _ in problems), e0, e1))


_BLK_OK = {}


def gemm_aux_blocked_ok(M, N, K):
    """May the fc1 forward save GELU' as the tile-blocked accumulator image (act 5) for the dgrad through fc2 (act 6)?  (include/simseg_hip.h:
    full 256x256 tiles on the ping-pong kernels.)  SIMSEG_AMD_BLOCKED_AUX=0 keeps the row-major tensor (A/B runs)."""
    key = (int(M), int(N), int(K))
    r = _BLK_OK.get(key)
    if r is None:
        r = _BLK_OK[key] = os.environ.get("SIMSEG_AMD_BLOCKED_AUX", "1") != "0" and bool(raw("simseg_gemm_aux_blocked_ok", *key))
    return r


def layernorm_fwd(x, gamma, beta, eps, out_dtype=torch.float32, want_bf16_copy=False, save_stats=False):
    require_gpu(x)
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    # (want_bf16_copy: False, True = a bf16 copy, or the 16-bit dtype the copy should have)
    y16 = torch.empty(x.shape, device=x.device, dtype=want_bf16_copy if isinstance(want_bf16_copy, torch.dtype) else torch.bfloat16) if want_bf16_copy else None
    mean = torch.empty(rows, device=x.device, dtype=torch.float32) if save_stats else None
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32) if save_stats else None
    call("simseg_layernorm_fwd", ptr(_c(x)), ptr(gamma), ptr(beta), ptr(y), dt(y), ptr(y16), ptr(mean), ptr(rstd), rows, D,
         float(eps), stream())
    return y, y16, mean, rstd


def layernorm_bwd(x, mean, rstd, gamma, dgamma, dbeta, dy16=None, dy32=None, dres=None, want_f32=True, want_bf16=True,
                  dxsum=None, drop_seed=0, drop_p=0.0, dres16=None, y16=None, beta=None):
    require_gpu(x)
    D = x.shape[-1]
    rows = x.numel() // D
    dx32 = torch.empty(x.shape, device=x.device, dtype=torch.float32) if want_f32 else None
    h16 = dy16.dtype if dy16 is not None else (want_bf16 if isinstance(want_bf16, torch.dtype) else torch.bfloat16)
    dx16 = torch.empty(x.shape, device=x.device, dtype=h16) if want_bf16 else None
    partials = torch.empty(raw("simseg_layernorm_bwd_workspace_bytes", rows, D) // 4, device=x.device, dtype=torch.float32)
    call("simseg_layernorm_bwd", ptr(_c(dy16)), ptr(_c(dy32)), ptr(_c(dres)), ptr(_c(dres16)), ptr(_c(x)), ptr(_c(y16)), ptr(_c(beta)) if y16 is not None else None,
         ptr(mean), ptr(rstd), ptr(gamma),
         ptr(dx32), ptr(dx16), ptr(dgamma), ptr(dbeta), ptr(dxsum), ptr(partials), rows, D, int(drop_seed), float(drop_p), stream())
    return dx32, dx16


def colsum_accum(x2d, out):
    require_gpu(x2d)
    call("simseg_colsum_accum", ptr(_c(x2d)), dt(x2d), ptr(out), x2d.shape[0], x2d.shape[1], x2d.shape[1], stream())
    return out


def vit_im2col(image, out_dtype):
    require_gpu(image)
    B, C, H, W = image.shape
    if C != 3 or image.dtype != torch.float32:
        raise ValueError("vit_im2col expects fp32 [B,3,H,W]")
    cols = torch.empty(B * (H // 16) * (W // 16), 768, device=image.device, dtype=out_dtype)
    call("simseg_vit_im2col", ptr(_c(image)), ptr(cols), dt(cols), B, H, W, stream())
    return cols


def vit_cls_rows(cls, pos, x):
    B, T, D = x.shape
    call("simseg_vit_cls_rows", ptr(cls), ptr(pos), ptr(x), B, T, D, stream())


def vit_cls_grad(dx, dcls):
    B, T, D = dx.shape
    call("simseg_vit_cls_grad", ptr(_c(dx)), ptr(dcls), B, T, D, stream())


def _keep_table(t, name, B, cols):
    if t.dtype != torch.int32 or tuple(t.shape) != (B, cols):
        raise ValueError(f"{name}: int32 [{B}, {cols}] expected, got {t.dtype} {tuple(t.shape)}")
    require_gpu(t)
    return _c(t)


def patch_keep_sample(B, N, K, seed, device):
    """Patch dropout's draw (include/simseg_hip.h): -> keep int32 [B, K] (ascending per image), inv int32 [B, N] (-1 = dropped).  No host read."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("simseg_amd ops run on MI355X only (device is %s); there is no CPU fallback" % device)
    keep = torch.empty(int(B), int(K), device=device, dtype=torch.int32)
    inv = torch.empty(int(B), int(N), device=device, dtype=torch.int32)
    call("simseg_patch_keep_sample", ptr(keep), ptr(inv), int(B), int(N), int(K), int(seed) & 0xFFFFFFFFFFFFFFFF, stream())
    return keep, inv


def vit_im2col_keep(image, keep, out_dtype):
    """vit_im2col of the kept patches only: cols [B * K, 768], row b * K + j = patch keep[b, j] of image b."""
    require_gpu(image)
    B, C, H, W = image.shape
    if C != 3 or image.dtype != torch.float32:
        raise ValueError("vit_im2col_keep expects fp32 [B,3,H,W]")
    K = keep.shape[1]
    cols = torch.empty(B * K, 768, device=image.device, dtype=out_dtype)
    call("simseg_vit_im2col_keep", ptr(_c(image)), ptr(_keep_table(keep, "vit_im2col_keep: keep", B, K)), ptr(cols), dt(cols), B, H, W, K, stream())
    return cols


def vit_keep_rows(cls, pos, keep, x):
    """In place on the fp32 stream x [B, 1 + K, D]: x[b, 0] = cls + pos[0]; x[b, 1 + j] += pos[1 + keep[b, j]]  (pos [N + 1, D])."""
    require_gpu(x)
    B, T, D = x.shape
    if x.dtype != torch.float32 or cls.dtype != torch.float32 or pos.dtype != torch.float32 or cls.numel() != D or pos.dim() != 2 or pos.shape[1] != D:
        raise ValueError("vit_keep_rows: fp32 x [B, 1 + K, D], cls [D] and pos [N + 1, D] expected")
    call("simseg_vit_keep_rows", ptr(_c(cls)), ptr(_c(pos)), ptr(_keep_table(keep, "vit_keep_rows: keep", B, T - 1)), ptr(_c(x)), B, pos.shape[0] - 1, T - 1, D,
         stream())
    return x


def vit_keep_pos_grad(dx, inv):
    """dpos fp32 [N + 1, D] from dx [B, 1 + K, D] (fp32 or 16-bit) and inv [B, N]: row 0 = sum_b dx[b, 0] (the [cls] gradient as well), row
    1 + n = the sum of the rows of the images that kept n, in ascending b; exactly 0 where no image did."""
    require_gpu(dx)
    B, T, D = dx.shape
    N = inv.shape[1]
    dpos = torch.empty(N + 1, D, device=dx.device, dtype=torch.float32)
    call("simseg_vit_keep_pos_grad", ptr(_c(dx)), dt(dx), ptr(_keep_table(inv, "vit_keep_pos_grad: inv", B, N)), ptr(dpos), B, N, T - 1, D, stream())
    return dpos


def bert_embed_fwd(ids, word, pos, type_emb):
    require_gpu(ids, word)
    B, L = ids.shape
    D = word.shape[1]
    out = torch.empty(B, L, D, device=word.device, dtype=torch.float32)
    call("simseg_bert_embed_fwd", ptr(_c(ids)), ptr(word), ptr(pos), ptr(type_emb), ptr(out), B, L, D, word.shape[0], stream())
    return out


def bert_embed_bwd(ids, mask, dsum, dword):
    B, L = ids.shape
    call("simseg_bert_embed_bwd", ptr(_c(ids)), ptr(_c(mask)), ptr(_c(dsum)), ptr(dword), B, L, dsum.shape[-1], dword.shape[0], stream())


def topk_pool_l2norm_fwd(tok, k, mask=None, eps=1e-8, normalize=True):
    require_gpu(tok)
    B, N, P = tok.shape
    emb = torch.empty(B, P, device=tok.device, dtype=torch.float32)
    idx = torch.empty(B, k, P, device=tok.device, dtype=torch.int32)
    norm = torch.empty(B, device=tok.device, dtype=torch.float32)
    scratch = None
    if B <= 256 and N >= 256:        # long token axes: scan 32 token slices per image in parallel, then merge (tools/pool_bench.py, N = 1024: 141 vs
                                     # 522 us at B = 63, 244 vs 600 us at B = 128; one block per image walks its tokens serially)
        scratch = torch.empty(raw("simseg_topk_pool_workspace_bytes", B, P, int(k)) // 4, device=tok.device, dtype=torch.float32)
    call("simseg_topk_pool_l2norm_fwd", ptr(_c(tok)), dt(tok), ptr(_c(mask)), ptr(emb), ptr(idx), ptr(norm), ptr(scratch), B, N, P, int(k),
         float(eps), int(normalize), stream())
    return emb, idx, norm


def topk_pool_l2norm_bwd(demb, emb, norm, idx, N, dtype, eps=1e-8, normalize=True):
    B, k, P = idx.shape
    dtok = torch.empty(B, N, P, device=emb.device, dtype=dtype)
    call("simseg_topk_pool_l2norm_bwd", ptr(_c(demb)), ptr(emb), ptr(norm), ptr(idx), ptr(dtok), dt(dtok), B, N, P, int(k), float(eps), int(normalize), stream())
    return dtok


def attention_fwd(qkv, heads, mask=None, scale=0.125, save_lse=False, drop_seed=0, drop_p=0.0, skip_padded_rows=False, zero_skipped=True):
    """qkv [B,T,3*H*64] packed (3,H,64) -> ctx [B,T,H*64].
    skip_padded_rows: the kernels do not write the rows past a sequence's last unmasked key (include/simseg_hip.h).  Those rows of the
    returned tensors are zeros unless the caller passes zero_skipped=False because it provably never reads them (the packed text
    tower gathers the real rows only and saves a fill pass per layer)."""
    require_gpu(qkv)
    B, T, W = qkv.shape
    if W != 3 * heads * 64:
        raise ValueError("attention: qkv last dim must be 3*heads*64")
    alloc = torch.zeros if (skip_padded_rows and zero_skipped) else torch.empty
    out = alloc(B, T, heads * 64, device=qkv.device, dtype=qkv.dtype)
    lse = alloc(B, heads, T, device=qkv.device, dtype=torch.float32) if save_lse else None
    _push_variant("attention")
    call("simseg_attention_fwd", ptr(_c(qkv)), ptr(_c(mask)), ptr(out), ptr(lse), dt(qkv), B, T, heads, float(scale),
         int(drop_seed), float(drop_p), int(skip_padded_rows), stream())
    return out, lse


def attention_bwd(qkv, out, dout, lse, heads, mask=None, scale=0.125, drop_seed=0, drop_p=0.0, skip_padded_rows=False, colsum=None,
                  zero_skipped=True):
    """dqkv; colsum (optional fp32 [3*H*64]) += column sums of dqkv, the q/k/v bias gradient (formed inside the kernel for T <= 256).
    skip_padded_rows / zero_skipped: as in attention_fwd - the skipped rows of dqkv are zeros (their true gradient) unless the caller
    never reads them."""
    B, T, W = qkv.shape
    dqkv = torch.zeros_like(qkv) if (skip_padded_rows and zero_skipped) else torch.empty_like(qkv)
    ws = torch.empty(raw("simseg_attention_bwd_workspace_bytes", B, T, heads) // 4, device=qkv.device, dtype=torch.float32)
    _push_variant("attention")
    call("simseg_attention_bwd", ptr(_c(qkv)), ptr(_c(mask)), ptr(_c(out)), ptr(_c(dout)), ptr(lse), ptr(ws), ptr(dqkv), ptr(colsum),
         dt(qkv), B, T, heads, float(scale), int(drop_seed), float(drop_p), int(skip_padded_rows), stream())
    return dqkv


def attention_fwd_rows(qkv, heads, row_start, max_len, scale=0.125, save_lse=False, drop_seed=0, drop_p=0.0, n_real=None):
    """Ragged batch without padding: qkv [rows, 3*H*64] bf16, sequence b = rows [row_start[b], row_start[b+1]) (int32 [B+1]), at most
    max_len tokens each -> ctx [rows, H*64] (rows outside every sequence - a tile padding behind row n_real - are zeros), lse [B,H,max_len]."""
    require_gpu(qkv, row_start)
    if qkv.dtype not in HALF_TYPES or row_start.dtype != torch.int32:
        raise TypeError("attention_fwd_rows: bf16 qkv, int32 row_start")
    rows, W = qkv.shape
    B = row_start.numel() - 1
    out = torch.empty(rows, heads * 64, device=qkv.device, dtype=qkv.dtype)
    if n_real is not None and n_real < rows:
        out[n_real:].zero_()
    lse = torch.empty(B, heads, max_len, device=qkv.device, dtype=torch.float32) if save_lse else None
    _push_variant("attention")
    call("simseg_attention_fwd_rows", ptr(_c(qkv)), ptr(_c(row_start)), ptr(out), ptr(lse), B, int(max_len), heads, float(scale), int(drop_seed),
         float(drop_p), stream())
    return out, lse


def attention_bwd_rows(qkv, out, dout, lse, heads, row_start, max_len, scale=0.125, drop_seed=0, drop_p=0.0, colsum=None, n_real=None):
    """dqkv [rows, 3*H*64] for attention_fwd_rows (rows behind n_real zeroed); colsum (optional fp32 [3*H*64]) += its column sums."""
    rows, W = qkv.shape
    B = row_start.numel() - 1
    dqkv = torch.empty_like(qkv)
    if n_real is not None and n_real < rows:
        dqkv[n_real:].zero_()
    ws = torch.empty(raw("simseg_attention_bwd_workspace_bytes", B, int(max_len), heads) // 4, device=qkv.device, dtype=torch.float32)
    _push_variant("attention")
    call("simseg_attention_bwd_rows", ptr(_c(qkv)), ptr(_c(row_start)), ptr(_c(out)), ptr(_c(dout)), ptr(lse), ptr(ws), ptr(dqkv), ptr(colsum),
         B, int(max_len), heads, float(scale), int(drop_seed), float(drop_p), stream())
    return dqkv


def attention_fwd_planes(qkvp, heads, B, T, row_start=None, scale=0.125, save_lse=False, drop_seed=0, drop_p=0.0, n_real=None):
    """Plane-major operands: qkvp [3*H, rows, 64] (16-bit) -> ctx [rows, H*64], lse [B,H,T].  Sequence b = rows [b*T, (b+1)*T) (row_start None)
    or [row_start[b], row_start[b+1]) (int32 [B+1]); rows outside every sequence (behind n_real) are zeros."""
    require_gpu(qkvp)
    P3, rows, d = qkvp.shape
    if qkvp.dtype not in HALF_TYPES or P3 != 3 * heads or d != 64 or not qkvp.is_contiguous():
        raise ValueError("attention_fwd_planes: contiguous 16-bit [3*H, rows, 64]")
    out = torch.empty(rows, heads * 64, device=qkvp.device, dtype=qkvp.dtype)
    if n_real is not None and n_real < rows:
        out[n_real:].zero_()
    lse = torch.empty(B, heads, T, device=qkvp.device, dtype=torch.float32) if save_lse else None
    _push_variant("attention")
    call("simseg_attention_fwd_planes", ptr(qkvp), rows, ptr(_c(row_start)), ptr(out), ptr(lse), B, int(T), heads, float(scale), int(drop_seed),
         float(drop_p), stream())
    return out, lse


def attention_bwd_planes(qkvp, out, dout, lse, heads, B, T, row_start=None, scale=0.125, drop_seed=0, drop_p=0.0, colsum=None, n_real=None):
    """dqkv [3*H, rows, 64] for attention_fwd_planes (rows behind n_real zeroed); colsum (optional fp32 [3*H*64]) += its column sums."""
    P3, rows, d = qkvp.shape
    dqkv = torch.empty_like(qkvp)
    if n_real is not None and n_real < rows:
        dqkv[:, n_real:].zero_()
    ws = torch.empty(raw("simseg_attention_bwd_workspace_bytes", B, int(T), heads) // 4, device=qkvp.device, dtype=torch.float32)
    _push_variant("attention")
    call("simseg_attention_bwd_planes", ptr(qkvp), rows, ptr(_c(row_start)), ptr(_c(out)), ptr(_c(dout)), ptr(lse), ptr(ws), ptr(dqkv), ptr(colsum),
         B, int(T), heads, float(scale), int(drop_seed), float(drop_p), stream())
    return dqkv


def segment_mean_l2norm(x):
    """[S,P,D] fp32 -> [S,D]: unit-norm mean over P."""
    require_gpu(x)
    S, Pn, D = x.shape
    out = torch.empty(S, D, device=x.device, dtype=torch.float32)
    call("simseg_segment_mean_l2norm", ptr(_c(x)), ptr(out), S, Pn, D, stream())
    return out


def patch_text_sim(x2d, text, eps=1e-12, normalize=True):
    """Fused K14 kernel: x2d [M,K], text [C,K] (same dtype, C <= 256) -> fp32 [M,C] cosine map."""
    require_gpu(x2d, text)
    if x2d.dtype != text.dtype:
        raise TypeError("patch_text_sim: x and text must share a dtype")
    M, K = x2d.shape
    C = text.shape[0]
    out = torch.empty(M, C, device=x2d.device, dtype=torch.float32)
    call("simseg_patch_text_sim", ptr(_c(x2d)), ptr(_c(text)), ptr(out), M, C, K, dt(x2d), float(eps), int(normalize), stream())
    return out


def row_rnorm(x2d, eps=1e-12):
    require_gpu(x2d)
    rn = torch.empty(x2d.shape[0], device=x2d.device, dtype=torch.float32)
    call("simseg_row_rnorm", ptr(_c(x2d)), dt(x2d), ptr(rn), x2d.shape[0], x2d.shape[1], float(eps), stream())
    return rn


def cast(x, dtype, out=None):
    require_gpu(x)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    call("simseg_cast", ptr(_c(x)), ptr(out), x.numel(), int(dtype in HALF_TYPES), stream())
    return out


ATTN_QSCALED_MIN_T = 512       # W64_MINT in csrc/attn.hip


def attention_qscale(scale=0.125):
    """The factor attention_fwd_qscaled expects on the q columns of the projection: softmax scale times log2(e)."""
    return float(scale) * 1.4426950408889634


def attention_fwd_qscaled(qkv, heads, save_lse=False):
    """Long-sequence 16-bit attention forward (T >= 512, no mask / dropout) on a projection whose q columns already carry
    attention_qscale(scale): qkv [B,T,3*H*64] -> ctx [B,T,H*64] (include/simseg_hip.h: simseg_attention_fwd_qscaled)."""
    require_gpu(qkv)
    B, T, W = qkv.shape
    if W != 3 * heads * 64 or qkv.dtype not in HALF_TYPES or T < ATTN_QSCALED_MIN_T:
        raise ValueError("attention_fwd_qscaled: 16-bit qkv [B, T >= 512, 3*heads*64]")
    out = torch.empty(B, T, heads * 64, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(B, heads, T, device=qkv.device, dtype=torch.float32) if save_lse else None
    _push_variant("attention")
    call("simseg_attention_fwd_qscaled", ptr(_c(qkv)), ptr(out), ptr(lse), B, T, heads, stream())
    return out, lse


def attention_fwd_x3(qkv32, heads, scale=0.125):
    """Exact-mode attention forward on the bf16 matrix pipe: qkv32 fp32 [B, T, 3*H*64] -> ctx fp32 [B, T, H*64], every product formed from
    the three exact bf16 pieces of its fp32 operands (six leading piece products, fp32 accumulation: include/simseg_hip.h).  Evaluation
    only (no mask, dropout or saved log-sum-exp)."""
    require_gpu(qkv32)
    B, T, W = qkv32.shape
    if qkv32.dtype != torch.float32 or W != 3 * heads * 64:
        raise ValueError("attention_fwd_x3: fp32 [B, T, 3*H*64]")
    planes = split_bf16x3(_c(qkv32).view(B * T, W), planes=True)           # [3, B*T, W]
    out = torch.empty(B, T, heads * 64, device=qkv32.device, dtype=torch.float32)
    call("simseg_attention_fwd_x3", ptr(planes), B * T * W, ptr(out), B, T, heads, float(scale), stream())
    return out


def split_bf16x3(x2d, b_pattern=False, planes=False):
    """fp32 [rows, K] -> bf16 [rows, 6 K]: the hi / mid / lo bf16 pieces of every element along K, in the A-operand order (hi hi hi mid mid
    lo) or the B-operand order (hi mid lo hi mid hi): gemm(split(a), split(b, True)) is the fp32 product a @ b^T formed on the bf16 MFMA
    pipe in fp32 accumulators (include/simseg_hip.h: simseg_split_bf16x3)."""
    require_gpu(x2d)
    rows, K = x2d.shape
    if x2d.stride(1) != 1:
        raise ValueError("split_bf16x3 needs unit-stride rows")
    # planes: the three pieces as [3, rows, K] (operand form of attention_fwd_x3) instead of the six K-segments of the GEMM operands
    out = torch.empty((3, rows, K) if planes else (rows, 6 * K), device=x2d.device, dtype=torch.bfloat16)
    call("simseg_split_bf16x3", ptr(x2d), ptr(out), rows, K, x2d.stride(0), 2 if planes else int(bool(b_pattern)), stream())
    return out


def transpose_f32(x2d, out=None):
    require_gpu(x2d)
    R, C = x2d.shape
    if out is None:
        out = torch.empty(C, R, device=x2d.device, dtype=torch.float32)
    elif tuple(out.shape) != (C, R) or out.dtype != torch.float32:
        raise ValueError(f"transpose_f32: out must be fp32 [{C}, {R}], got {out.dtype} {tuple(out.shape)}")
    call("simseg_transpose_f32", ptr(_c(x2d)), ptr(_c(out)), R, C, stream())
    return out


def ragged_maps(mask, multiple, cap, expect=-1):
    """(idx int32 [cap], inv int32 [B*L], row_start int32 [B+1], info int32 [4]) of a [B, L] int64 0/1 mask - include/simseg_hip.h."""
    require_gpu(mask)
    if mask.dtype != torch.int64 or mask.dim() != 2:
        raise TypeError("ragged_maps: int64 [B, L] mask")
    B, L = mask.shape
    dev = mask.device
    idx = torch.empty(cap, device=dev, dtype=torch.int32)
    inv = torch.empty(B * L, device=dev, dtype=torch.int32)
    row_start = torch.empty(B + 1, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int32)
    call("simseg_ragged_maps", ptr(_c(mask)), B, L, int(multiple), int(cap), int(expect), ptr(idx), ptr(inv), ptr(row_start), ptr(info), stream())
    return idx, inv, row_start, info


def gather_rows(src2d, idx, out=None):
    """out[i] = src2d[idx[i]] (zero row where idx[i] < 0).  idx int32 on the device."""
    require_gpu(src2d, idx)
    if idx.dtype != torch.int32:
        raise TypeError("gather_rows: idx must be int32")
    n, w = idx.numel(), src2d.shape[-1]
    if out is None:
        out = torch.empty(n, w, device=src2d.device, dtype=src2d.dtype)
    call("simseg_gather_rows", ptr(_c(src2d)), ptr(_c(idx)), ptr(_c(out)), n, w * src2d.element_size(), stream())
    return out


def dropout_apply_(g, seed, p):
    call("simseg_dropout_apply", ptr(_c(g)), dt(g), g.numel(), int(seed), float(p), stream())
    return g


def _sim_block_check(who, sims, target0, blocks=False):
    require_gpu(sims)
    if sims.dim() != (3 if blocks else 2) or (blocks and sims.shape[0] not in (1, 2)):
        raise ValueError(f"{who}: sims [N1, N2]" + (" or [blocks, N1, N2] with 1 or 2 blocks" if blocks else "") + f", got {tuple(sims.shape)}")
    if sims.dtype != torch.float32:
        raise TypeError(f"{who}: sims must be fp32, got {sims.dtype}")
    _c(sims)
    return sims.shape[-2], sims.shape[-1]


def _one_f32_check(who, **tensors):
    """Each named tensor is an fp32 device tensor of one element."""
    require_gpu(*tensors.values())
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be fp32, got {t.dtype}")
        if t.numel() != 1:
            raise ValueError(f"{who}: {name} holds one element, got {tuple(t.shape)}")


def _rows_call(entry, sims, dims, *, head=(), tail, k, rows, n_out):
    """What the row wrappers share: k row arrays of `rows` floats each and the small `out`, then the C entry, whose arguments are all
    (sims, *head, row arrays, out, N1, N2, target0, *tail, stream).  -> (out, the row arrays [k, rows]: the first holds the row losses)"""
    scratch = torch.empty(k, rows, device=sims.device, dtype=torch.float32)
    out = torch.empty(n_out, device=sims.device, dtype=torch.float32)
    base = scratch.data_ptr()          # (the row arrays' addresses by arithmetic: no tensor is made per array; 0 stays 0 for an empty scratch)
    call(entry, ptr(sims), *head, *(base + 4 * rows * i for i in range(k)), ptr(out), *dims, *tail, stream())
    return out, scratch


def nce_rows(sims, temperature, target0, ignore_mask=None, smoothing=0.0, write_grad=True):
    """In place: sims <- dLoss/dsims.  Returns out3 = [loss, acc, dLoss/dT] (device tensor)."""
    N1, N2 = _sim_block_check("nce_rows", sims, target0)
    return _rows_call("simseg_nce_rows", sims, (N1, N2, int(target0)), head=(ptr(temperature), ptr(_c(ignore_mask))),
                      tail=(float(smoothing), int(write_grad)), k=3, rows=N1, n_out=3)[0]


def nce_pair(sims2, temperature, target0, smoothing=0.0, write_grad=True):
    """Both directions at once (include/simseg_hip.h simseg_nce_pair): sims2 [2, N1, N2] fp32, in place -> gradients w.r.t. the
    similarities.  Returns out4 = [loss, i2t acc, t2i acc, dLoss/dT] (device tensor)."""
    N1, N2 = _sim_block_check("nce_pair", sims2, target0, blocks=True)
    if sims2.shape[0] != 2:
        raise ValueError(f"nce_pair: sims2 [2, N1, N2], got {tuple(sims2.shape)}")
    # (one scratch pointer: the entry cuts its three row arrays of 2 N1 out of it)
    return _rows_call("simseg_nce_pair", sims2, (N1, N2, int(target0)), head=(ptr(temperature),), tail=(float(smoothing), int(write_grad)),
                      k=1, rows=6 * N1, n_out=4)[0]


def mix_nce_rows(sims, temperature, target0, alpha, ignore_mask=None, smoothing=0.0, write_grad=True):
    """nce_rows against the two targets a = target0 + i and b = target0 + (N1 - 1 - i) weighted alpha_i / 1 - alpha_i (include/simseg_hip.h
    simseg_mix_nce_rows).  In place: sims <- dLoss/dsims.  alpha: fp32 device tensor, one element (every row) or [N1].
    -> (out3 = [loss, acc, dLoss/dT], row losses [N1] - each already times its ignore weight)."""
    N1, N2 = _sim_block_check("mix_nce_rows", sims, target0)
    require_gpu(temperature, alpha, ignore_mask)
    if alpha.dtype != torch.float32:
        raise TypeError(f"mix_nce_rows: alpha must be fp32, got {alpha.dtype}")
    if alpha.numel() != 1 and tuple(alpha.shape) != (N1,):
        raise ValueError(f"mix_nce_rows: alpha holds one element or [{N1}], got {tuple(alpha.shape)}")
    if ignore_mask is not None and (ignore_mask.dtype != torch.float32 or tuple(ignore_mask.shape) != (N1,)):
        raise ValueError(f"mix_nce_rows: ignore_mask must be fp32 [{N1}], got {ignore_mask.dtype} {tuple(ignore_mask.shape)}")
    out3, rows = _rows_call("simseg_mix_nce_rows", sims, (N1, N2, int(target0)),
                            head=(ptr(temperature), ptr(_c(ignore_mask)), ptr(_c(alpha)), 0 if alpha.numel() == 1 else 1),
                            tail=(float(smoothing), int(bool(write_grad))), k=3, rows=N1, n_out=3)
    return out3, rows[0]


def triplet_rows(sims, target0, margin, reduce, mask_block, write_grad=True):
    """The max-violation hinge rows (include/simseg_hip.h simseg_triplet_rows) of sims [N1, N2], or of two stacked blocks [2, N1, N2] in
    one launch.  reduce: 0 / "mean", 1 / "max".  In place: sims <- d rowloss / d sims.  -> (out = [sum of the row losses, acc] - with two
    blocks [sum over both, acc0, acc1] -, row losses [N1] or [2, N1])."""
    stacked = sims.dim() == 3
    N1, N2 = _sim_block_check("triplet_rows", sims, target0, blocks=stacked)
    blocks = sims.shape[0] if stacked else 1
    reduce = {"mean": 0, "max": 1}.get(reduce, reduce)
    if reduce == 0 and N1 < 2:
        raise ValueError("triplet_rows: the mean over N1 - 1 negatives needs N1 >= 2 (the reference divides by zero here)")
    out, rows = _rows_call("simseg_triplet_rows", sims, (N1, N2, int(target0)),
                           tail=(float(margin), int(reduce), int(bool(mask_block)), blocks, int(bool(write_grad))),
                           k=2, rows=blocks * max(N1, 1), n_out=1 + blocks)
    return out, (rows[0].view(blocks, N1) if stacked else rows[0])


def siglip_rows(sims, temperature, bias, target0, write_grad=True):
    """The pairwise sigmoid rows of SigLIP (include/simseg_hip.h simseg_siglip_rows) of sims [N1, N2]: z = s / clamp(T, 1e-3, 0.5) + b,
    row i's positive is column target0 + i, every other column a negative.  In place: sims <- dLoss/dsims (write_grad=False leaves it).
    temperature, bias: fp32 device tensors of one element.  -> (out4 = [loss, acc, dLoss/dT, dLoss/db], row losses [N1])."""
    N1, N2 = _sim_block_check("siglip_rows", sims, target0)
    _one_f32_check("siglip_rows", temperature=temperature, bias=bias)
    out4, rows = _rows_call("simseg_siglip_rows", sims, (N1, N2, int(target0)), head=(ptr(temperature), ptr(bias)),
                            tail=(int(bool(write_grad)),), k=4, rows=max(N1, 1), n_out=4)
    return out4, rows[0]


def ntxent_rows(sims, temperature, target0, write_grad=True):
    """The NT-Xent rows of SimCLR / SLIP (include/simseg_hip.h simseg_ntxent_rows) of sims [N1, N2], N1 = 2B: rows [0, B) are view a, rows
    [B, 2B) view b, the own block is columns [target0, target0 + N1); row i leaves its own column target0 + i out of the softmax and has its
    positive at target0 + (i + B) mod N1.  In place: sims <- dLoss/dsims (write_grad=False leaves it).  temperature: fp32 device tensor of
    one element.  -> (out4 = [loss, acc of view a's rows, acc of view b's rows, dLoss/dT], row losses [N1])."""
    N1, N2 = _sim_block_check("ntxent_rows", sims, target0)
    _one_f32_check("ntxent_rows", temperature=temperature)
    if N1 % 2:
        raise ValueError(f"ntxent_rows: N1 = {N1} is odd; the rows are view a stacked on view b, N1 = 2B")
    out4, rows = _rows_call("simseg_ntxent_rows", sims, (N1, N2, int(target0)), head=(ptr(temperature),), tail=(int(bool(write_grad)),),
                            k=3, rows=max(N1, 1), n_out=4)
    return out4, rows[0]


def transpose_multi(mats, scale_flags, scalar=None, alpha=1.0, x0=None):
    """Transposes of up to six contiguous fp32 matrices in ONE launch; matrices whose flag is set are multiplied by alpha * scalar[0] in
    the copy and in place.  Returns (list of transposed tensors, scalar[0] * x0[0] as a 1-element tensor or None)."""
    import ctypes
    n = len(mats)
    for m in mats:
        require_gpu(m)
        if m.dtype != torch.float32 or m.dim() != 2:
            raise TypeError("transpose_multi: contiguous fp32 matrices")
        _c(m)
    outs = [torch.empty(m.shape[1], m.shape[0], device=m.device, dtype=torch.float32) for m in mats]
    y0 = torch.empty(1, device=mats[0].device, dtype=torch.float32) if x0 is not None else None
    PT, I64, I32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int32 * n
    call("simseg_transpose_multi", PT(*[m.data_ptr() for m in mats]), PT(*[o.data_ptr() for o in outs]), I64(*[m.shape[0] for m in mats]),
         I64(*[m.shape[1] for m in mats]), I32(*[int(bool(f)) for f in scale_flags]), n, ptr(scalar), float(alpha), ptr(x0), ptr(y0), stream())
    return outs, y0


def scale_rows(x, s=None, one_minus=False, alpha=1.0, out=None):
    require_gpu(x)
    if out is None:
        out = torch.empty_like(x)
    D = x.shape[-1]
    call("simseg_scale_rows", ptr(_c(x)), ptr(_c(s)), ptr(out), x.numel() // D, D, int(one_minus), float(alpha), stream())
    return out


def scale_by_scalar(x, scalar, alpha=1.0, out=None):
    if out is None:
        out = torch.empty_like(x)
    call("simseg_scale_by_scalar", ptr(_c(x)), ptr(scalar), ptr(out), x.numel(), float(alpha), stream())
    return out


def retrieval_rank(sim, left_gid, right_gid):
    require_gpu(sim)
    M, N = sim.shape
    has = torch.empty(M, device=sim.device, dtype=torch.int32)
    rank = torch.empty(M, device=sim.device, dtype=torch.int32)
    call("simseg_retrieval_rank", ptr(_c(sim)), ptr(_c(left_gid)), ptr(_c(right_gid)), ptr(has), ptr(rank), M, N, N, stream())
    return has, rank


def retrieval_rank_cols(sim, row_gid, col_gid):
    """Column j of sim [M,N] retrieves rows: (has [N], rank [N]) from the same matrix the row direction used."""
    require_gpu(sim)
    M, N = sim.shape
    has = torch.empty(N, device=sim.device, dtype=torch.int32)
    rank = torch.empty(N, device=sim.device, dtype=torch.int32)
    scratch = torch.empty(N, device=sim.device, dtype=torch.int32)
    call("simseg_retrieval_rank_cols", ptr(_c(sim)), ptr(_c(row_gid)), ptr(_c(col_gid)), ptr(has), ptr(rank), ptr(scratch), M, N, N, stream())
    return has, rank


def recall_counts(has, rank, bounds=(1, 5, 10)):
    counts = torch.empty(4, device=has.device, dtype=torch.int32)
    call("simseg_recall_counts", ptr(has), ptr(rank), has.numel(), int(bounds[0]), int(bounds[1]), int(bounds[2]), ptr(counts), stream())
    return counts


TOPK_MAX = 128                 # simseg_topk_search / simseg_topk_merge: 1 <= K <= 128


def _search_operand(t, dtype):
    """[rows, D] operand of topk_search in `dtype` (fp32 or bf16): unit stride along D, any leading dimension that keeps rows 16-byte aligned."""
    if t.dim() != 2:
        raise ValueError("topk_search: operands are [rows, D] matrices")
    if t.dtype != dtype:
        if dtype == torch.bfloat16 and t.dtype == torch.float32:
            t = cast(t.contiguous(), torch.bfloat16)
        elif dtype == torch.float32 and t.dtype in HALF_TYPES:
            t = t.float()
        else:
            raise TypeError(f"topk_search: cannot take {t.dtype} operands as {dtype}")
    epc = 16 // t.element_size()
    if t.stride(1) != 1 or (t.shape[0] > 1 and (t.stride(0) < t.shape[1] or t.stride(0) % epc)):
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def topk_search(q, g, k, index_offset=0, dtype=None):
    """The k best rows of g [N, D] for every row of q [M, D] by inner product, fused (no M x N matrix): (score [M, k] fp32 descending,
    idx [M, k] int32 = gallery row + index_offset); equal scores by ascending index, the order of a stable descending argsort; N < k
    leaves -inf / -1 in the tail.  dtype: torch.float32 (fp32 products) or torch.bfloat16 (exact bf16 products, fp32 accumulation);
    None takes q's.  D % 8 == 0."""
    require_gpu(q, g)
    dtype = dtype or q.dtype
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"topk_search: fp32 or bf16 operands, got {dtype}")
    q, g = _search_operand(q, dtype), _search_operand(g, dtype)
    M, D = q.shape
    N = g.shape[0]
    if g.shape[1] != D:
        raise ValueError(f"topk_search: inner dims differ ({D} vs {g.shape[1]})")
    k = int(k)
    code = F32 if dtype == torch.float32 else BF16
    score = torch.empty(M, k, device=q.device, dtype=torch.float32)
    idx = torch.empty(M, k, device=q.device, dtype=torch.int32)
    nbytes = raw("simseg_topk_search_workspace_bytes", M, N, D, k, code) if 1 <= k <= TOPK_MAX else 0
    ws = torch.empty(nbytes // 8, device=q.device, dtype=torch.int64) if nbytes else None
    ldq = q.stride(0) if M > 1 else D
    ldg = g.stride(0) if N > 1 else D
    call("simseg_topk_search", ptr(q), ptr(g), code, M, N, D, ldq, ldg, k, int(index_offset), ptr(score), ptr(idx), ptr(ws), nbytes, stream())
    return score, idx


def topk_merge(score_a, idx_a, score_b, idx_b):
    """The k best of the union of two finished lists [M, k] of topk_search (same order, idx < 0 = empty slot)."""
    require_gpu(score_a, idx_a, score_b, idx_b)
    if not (score_a.shape == idx_a.shape == score_b.shape == idx_b.shape) or score_a.dim() != 2:
        raise ValueError("topk_merge: four [M, k] tensors")
    if score_a.dtype != torch.float32 or score_b.dtype != torch.float32 or idx_a.dtype != torch.int32 or idx_b.dtype != torch.int32:
        raise TypeError("topk_merge: fp32 scores and int32 indices")
    M, k = score_a.shape
    score, idx = torch.empty_like(score_a), torch.empty_like(idx_a)
    call("simseg_topk_merge", ptr(_c(score_a)), ptr(_c(idx_a)), ptr(_c(score_b)), ptr(_c(idx_b)), ptr(score), ptr(idx), M, k, stream())
    return score, idx


KNN_KS_MAX = 4                 # simseg_knn_vote_rows: up to four neighbourhood sizes per launch
_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def _labels_i32(who, t, device):
    """Class labels of any integer dtype -> a contiguous int32 vector on `device`.  Values are checked (>= 0, < 2^31) where that reads no
    device memory: always for a host tensor, by the dtype's range alone for a device one."""
    if not torch.is_tensor(t) or t.dtype not in _INT_DTYPES:
        raise TypeError(f"{who}: integer class labels, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if t.dim() != 1:
        raise ValueError(f"{who}: a vector of labels, got shape {tuple(t.shape)}")
    if not t.is_cuda and t.numel():
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi > 0x7fffffff:
            raise ValueError(f"{who}: labels must lie in [0, 2^31), got {lo} .. {hi}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def check_knn_ks(ks, K=None):
    """ks as simseg_knn_vote_rows takes them: 1 to 4 strictly ascending integers >= 1, the last at most TOPK_MAX (and K when given)."""
    ks = tuple(int(k) for k in ks)
    if not 1 <= len(ks) <= KNN_KS_MAX:
        raise ValueError(f"knn_vote: 1 to {KNN_KS_MAX} values of k, got {len(ks)}")
    if ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"knn_vote: ks must be strictly ascending and >= 1, got {ks}")
    if ks[-1] > TOPK_MAX:
        raise ValueError(f"knn_vote: max(ks) = {ks[-1]} exceeds TOPK_MAX = {TOPK_MAX}, the longest list the search returns")
    if K is not None and ks[-1] > K:
        raise ValueError(f"knn_vote: max(ks) = {ks[-1]} exceeds the K = {K} neighbours given")
    return ks


def knn_vote(score, idx, gallery_label, ks, temperature=0.07, query_label=None, counts=None):
    """Temperature-weighted k-NN vote over the (score, idx) [M, K] lists of topk_search / topk_merge / retrieval.search (idx int32 or
    int64, -1 in empty slots), for every k of `ks` from one launch (include/simseg_hip.h: simseg_knn_vote_rows):
    -> (pred [len(ks), M, 5] int32, vote [len(ks), M, 5] fp32, counts).  gallery_label [N] / query_label [M]: integer labels of any
    dtype.  With query_label, counts [len(ks), 3] int64 += {rows, top-1 hits, top-5 hits}; pass the returned tensor back in to accumulate
    over calls (None starts at zero).  Without query_label nothing is counted and counts is returned as given."""
    require_gpu(score, idx)
    if score.dim() != 2 or score.shape != idx.shape:
        raise ValueError("knn_vote: score and idx are [M, K] tensors of one shape")
    if score.dtype != torch.float32 or idx.dtype not in (torch.int32, torch.int64):
        raise TypeError("knn_vote: fp32 scores and int32 / int64 indices")
    M, K = score.shape
    ks = check_knn_ks(ks, K)
    dev = score.device
    glabel = _labels_i32("knn_vote: gallery_label", gallery_label, dev)
    qlabel = None
    if query_label is not None:
        qlabel = _labels_i32("knn_vote: query_label", query_label, dev)
        if qlabel.numel() != M:
            raise ValueError(f"knn_vote: {qlabel.numel()} query labels for {M} rows")
        if counts is None:
            counts = torch.zeros(len(ks), 3, device=dev, dtype=torch.int64)
        elif counts.shape != (len(ks), 3) or counts.dtype != torch.int64 or not counts.is_cuda or not counts.is_contiguous():
            raise ValueError(f"knn_vote: counts is a contiguous int64 [{len(ks)}, 3] tensor on the device")
    idx32 = idx if idx.dtype == torch.int32 else idx.to(torch.int32)
    pred = torch.empty(len(ks), M, 5, device=dev, dtype=torch.int32)
    vote = torch.empty(len(ks), M, 5, device=dev, dtype=torch.float32)
    call("simseg_knn_vote_rows", ptr(_c(score)), ptr(_c(idx32)), ptr(glabel), ptr(qlabel), M, glabel.numel(), K,
         (ctypes.c_int32 * len(ks))(*ks), len(ks), float(temperature), ptr(pred), ptr(vote), ptr(counts) if qlabel is not None else None, stream())
    return pred, vote, counts


def adamw_step(p, g, m, v, p16, lr, betas, eps, weight_decay, step, grad_scale=1.0):
    call("simseg_adamw_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), p.numel(), float(lr), float(betas[0]), float(betas[1]),
         float(eps), float(weight_decay), int(step), float(grad_scale), stream())


def tr16_probe():
    out = torch.empty(256, device="cuda", dtype=torch.int32)
    call("simseg_debug_tr16_probe", ptr(out), stream())
    return out.cpu().view(64, 4)


# ---- zero-shot segmentation post-processing (tools/seg_evaluation.py:112-170) ------------------------------------------------
def seg_select(scores, top_cls_num, ncand=5):
    """scores [B,C] fp32 -> (cand_idx [B,ncand] int32 (-1 = slot skipped), cand_score [B,ncand] fp32, threshold [B] fp32)."""
    require_gpu(scores)
    B, C = scores.shape
    idx = torch.empty(B, ncand, device=scores.device, dtype=torch.int32)
    sc = torch.empty(B, ncand, device=scores.device, dtype=torch.float32)
    thr = torch.empty(B, device=scores.device, dtype=torch.float32)
    call("simseg_seg_select", ptr(_c(scores.float())), ptr(idx), ptr(sc), ptr(thr), B, C, int(top_cls_num), int(ncand), stream())
    return idx, sc, thr


def seg_masks(sim, cand_idx, n, want_prob=False):
    """sim [B,nh*nw,C] fp32, cand_idx [B,ncand] -> mask [B,ncand,16nh,16nw] uint8 (0/255; skipped slots all zero), prob or None.
    n: the patch grid - an int (n x n, one resized image) or (nh, nw) (a stitched sliding-window map)."""
    require_gpu(sim, cand_idx)
    B, N, C = sim.shape
    nh, nw = (n, n) if isinstance(n, int) else (int(n[0]), int(n[1]))
    if N != nh * nw:
        raise ValueError(f"seg_masks: sim has {N} patches, expected {nh}x{nw}")
    ncand = cand_idx.shape[1]
    mask = torch.zeros(B, ncand, 16 * nh, 16 * nw, device=sim.device, dtype=torch.uint8)
    prob = torch.zeros(B, ncand, N, device=sim.device, dtype=torch.float32) if want_prob else None
    call("simseg_seg_masks_rect", ptr(_c(sim)), ptr(_c(cand_idx)), ptr(prob) if want_prob else None, ptr(mask), B, nh, nw, C, ncand, stream())
    return mask, prob


def stitch_windows(win, wy, wx, n, step):
    """win [B*wy*wx, n*n, C] fp32 (per-window maps, windows of an image consecutive, row-major over the window grid) -> [B, nh*nw, C]:
    the overlap-average on the source image's patch grid, nh = n + (wy-1)*step, nw = n + (wx-1)*step (simseg_stitch_windows)."""
    require_gpu(win)
    M, N, C = win.shape
    if win.dtype != torch.float32 or N != n * n or M % (wy * wx):
        raise ValueError(f"stitch_windows: fp32 [B*{wy}*{wx}, {n}*{n}, C] maps expected, got {tuple(win.shape)} {win.dtype}")
    B = M // (wy * wx)
    nh, nw = n + (wy - 1) * step, n + (wx - 1) * step
    out = torch.empty(B, nh * nw, C, device=win.device, dtype=torch.float32)
    call("simseg_stitch_windows", ptr(_c(win)), ptr(out), B, wy, wx, n, step, C, stream())
    return out


def morph7(img, erode):
    """7x7 dilate (erode=False) / erode (True), one iteration, on uint8 [..., H, W]."""
    require_gpu(img)
    if img.dtype != torch.uint8:
        raise TypeError("morph7: uint8 images")
    x = _c(img)
    H, W = x.shape[-2:]
    out = torch.empty_like(x)
    call("simseg_morph7", ptr(x), ptr(out), x.numel() // (H * W), H, W, int(bool(erode)), stream())
    return out


def close7(img, valid=None):
    """cv2.dilate then cv2.erode (7x7, one iteration each) in one pass on uint8 [..., H, W]; `valid` (int32, one per image): images
    with a negative entry are skipped and come back zero."""
    require_gpu(img)
    if img.dtype != torch.uint8:
        raise TypeError("close7: uint8 images")
    x = _c(img)
    H, W = x.shape[-2:]
    out = torch.zeros_like(x) if valid is not None else torch.empty_like(x)
    call("simseg_close7", ptr(x), ptr(out), ptr(_c(valid)) if valid is not None else None, x.numel() // (H * W), H, W, stream())
    return out


def seg_predict(masks, cand_idx, cand_score, labels, num_classes, ignore_index=255, hist=None, want_pred=True):
    """masks [B,ncand,Hm,Wm] uint8, labels [B,H,W] uint8 -> (pred [B,H,W] int32 or None, hist [3,C] int64 accumulated:
    rows = intersect, pred area, label area)."""
    require_gpu(masks, labels)
    B, ncand, Hm, Wm = masks.shape
    _, H, W = labels.shape
    if hist is None:
        hist = torch.zeros(3, num_classes, device=masks.device, dtype=torch.int64)
    pred = torch.empty(B, H, W, device=masks.device, dtype=torch.int32) if want_pred else None
    call("simseg_seg_predict", ptr(_c(masks)), ptr(_c(cand_idx)), ptr(_c(cand_score)), ptr(_c(labels)), ptr(pred) if want_pred else None,
         ptr(hist), B, ncand, Hm, Wm, H, W, int(num_classes), int(ignore_index), stream())
    return pred, hist


_CRF_WS = {}
_CRF_SPATIAL = {}      # (device, stream) -> (workspace address, H, W, sxy_g) of the spatial lattice that workspace holds


def dense_crf(rgb, prob, sxy_g=3.0, compat_g=3.0, sxy_b=40.0, srgb=13.0, compat_b=10.0, iters=3, want_q=False):
    """tools/seg_evaluation.py:31-54 for the C candidate maps of each image of a batch.  rgb [B,H,W,3] (or [H,W,3]) uint8 (RGB), prob
    [B,C,H,W] (or [C,H,W]) fp32 in [0,1] -> (mask uint8 0/255, Q(label 1) fp32 or None), shaped like prob."""
    require_gpu(rgb, prob)
    if rgb.dtype != torch.uint8 or prob.dtype != torch.float32:
        raise TypeError("dense_crf: rgb uint8 [B,H,W,3], prob fp32 [B,C,H,W]")
    single = prob.dim() == 3
    if single:
        rgb, prob = rgb[None], prob[None]
    B, C, H, W = prob.shape
    if tuple(rgb.shape) != (B, H, W, 3):
        raise ValueError(f"dense_crf: images {tuple(rgb.shape)} do not match the maps {tuple(prob.shape)}")
    nbytes = raw("simseg_dense_crf_workspace_bytes", B, H, W, C)
    if nbytes < 0:
        raise ValueError(f"dense_crf: 1..8 candidate maps per image (got {C})")
    key = (rgb.device, torch.cuda.current_stream().cuda_stream)
    ws = _CRF_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        _CRF_WS.pop(key, None)
        _CRF_SPATIAL.pop(key, None)
        ws = _CRF_WS[key] = torch.empty(nbytes, device=rgb.device, dtype=torch.uint8)
    mask = torch.empty(B, C, H, W, device=rgb.device, dtype=torch.uint8)
    q = torch.empty(B, C, H, W, device=rgb.device, dtype=torch.float32) if want_q else None
    # the spatial (Gaussian) lattice depends on H, W and sxy only and lives at the head of the workspace: a call with the same three on the
    # same workspace (this module owns it - nobody else writes there) finds it built
    sig = (ws.data_ptr(), int(H), int(W), float(sxy_g))
    reuse = _CRF_SPATIAL.get(key) == sig and os.environ.get("SIMSEG_CRF_SPATIAL_CACHE", "1") != "0"
    call("simseg_dense_crf", ptr(_c(rgb)), ptr(_c(prob)), ptr(mask), ptr(q), B, C, H, W, float(sxy_g), float(compat_g), float(sxy_b), float(srgb),
         float(compat_b), int(iters), ptr(ws), nbytes, int(reuse), stream())
    _CRF_SPATIAL[key] = sig
    if single:
        return mask[0], (q[0] if want_q else None)
    return mask, q


_PAMR_WS = {}          # (device, stream) -> workspace
PAMR_DILATIONS = (1, 2, 4, 8, 12, 24)


def pamr_check(dilations, iters, K=1, scale=1):
    """The ranges simseg_pamr accepts, checked before a device is needed -> the dilations as a tuple of ints."""
    try:
        given = list(dilations)
        dil = tuple(int(d) for d in given)
    except (TypeError, ValueError):
        raise ValueError(f"pamr: dilations are a sequence of 1..8 integers in 1..64, got {dilations!r}")
    if not 1 <= len(dil) <= 8 or any(d < 1 or d > 64 or d != f for d, f in zip(dil, given)):
        raise ValueError(f"pamr: dilations are a sequence of 1..8 integers in 1..64, got {dilations!r}")
    if int(iters) != iters or not 0 <= iters <= 64:
        raise ValueError(f"pamr: 0..64 iterations (got {iters!r})")
    if not 1 <= K <= 8:
        raise ValueError(f"pamr: 1..8 candidate maps per image (got {K})")
    if int(scale) != scale or scale < 1:
        raise ValueError(f"pamr: the map scale is a positive integer (got {scale!r})")
    return dil


def pamr(rgb, prob, cand_idx=None, dilations=PAMR_DILATIONS, iters=10, scale=1, want_m=False):
    """Pixel-adaptive mask refinement (include/simseg_hip.h simseg_pamr) of the K candidate maps of each image of a batch.  rgb
    [B,H,W,3] (or [H,W,3]) uint8, prob [B,K,H/scale,W/scale] (or [K,...]) fp32 in [0,1], cand_idx (optional) [B,K] (or [K]) int32: slots
    with a negative entry are skipped and come back zero -> (mask uint8 0/255 [B,K,H,W], refined map fp32 or None)."""
    if rgb.dtype != torch.uint8 or prob.dtype != torch.float32 or rgb.dim() not in (3, 4) or prob.dim() != rgb.dim():
        raise TypeError("pamr: rgb uint8 [B,H,W,3], prob fp32 [B,K,H/scale,W/scale]")
    single = prob.dim() == 3
    if single:
        rgb, prob = rgb[None], prob[None]
        cand_idx = cand_idx[None] if cand_idx is not None else None
    B, K, h, w = prob.shape
    dil = pamr_check(dilations, iters, K, scale)
    H, W = h * int(scale), w * int(scale)
    if tuple(rgb.shape) != (B, H, W, 3):
        raise ValueError(f"pamr: images {tuple(rgb.shape)} do not match the maps {tuple(prob.shape)} at scale {scale}")
    if cand_idx is not None and (cand_idx.dtype != torch.int32 or tuple(cand_idx.shape) != (B, K)):
        raise ValueError(f"pamr: cand_idx int32 [{B},{K}] expected, got {cand_idx.dtype} {tuple(cand_idx.shape)}")
    require_gpu(rgb, prob, cand_idx)
    nbytes = raw("simseg_pamr_workspace_bytes", B, K, H, W, len(dil)) if iters else 0
    key = (rgb.device, torch.cuda.current_stream().cuda_stream)
    ws = _PAMR_WS.get(key)
    if nbytes and (ws is None or ws.numel() < nbytes):
        _PAMR_WS.pop(key, None)
        ws = None                  # (the old workspace is released before the new one is requested)
        ws = _PAMR_WS[key] = torch.empty(nbytes, device=rgb.device, dtype=torch.uint8)
    mask = torch.empty(B, K, H, W, device=rgb.device, dtype=torch.uint8)
    m = torch.empty(B, K, H, W, device=rgb.device, dtype=torch.float32) if want_m else None
    call("simseg_pamr", ptr(_c(rgb)), ptr(_c(prob)), ptr(_c(cand_idx)), ptr(mask), ptr(m), B, K, H, W, (ctypes.c_int * len(dil))(*dil), len(dil),
         int(iters), int(scale), ptr(ws) if nbytes else None, nbytes, stream())
    if single:
        return mask[0], (m[0] if want_m else None)
    return mask, m


# ---- sliding windows over images of any size (segpost.slide_windows; include/simseg_hip.h simseg_slide_*) ---------------------------------
def slide_plan(sizes, win, stride, device, ncand=5):
    """Host geometry + device tables of a sliding-window pass over images of sizes [(H, W), ...]: windows at segpost.slide_windows offsets,
    an image's windows consecutive.  -> dict(img_tab int64 [B,8], win_tab int64 [Nw,3] (device), windows [(image, y0, x0)], src_off, out_off
    (element offsets of each image in the packed [3,H,W] images and in the [ncand,H,W] stitched planes), out_numel, sizes, win, ncand)."""
    from .segpost import slide_windows
    it, wt, src_off, out_off = [], [], [], []
    s = o = 0
    for b, (H, W) in enumerate(sizes):
        offs = slide_windows(H, W, win, stride)
        ny = len({y for y, _ in offs})
        nx = len(offs) // ny
        it.append([s, H, W, o, len(wt), ny, nx, 0])
        wt.extend([b, y, x] for y, x in offs)
        src_off.append(s); out_off.append(o)
        s += 3 * H * W
        o += (ncand * H * W + 15) // 16 * 16            # planes of the next image start 16-aligned (16-byte mask stores)
    dev = torch.device(device)
    return {"img_tab": to_device_async(it, dev), "win_tab": to_device_async(wt, dev),
            "windows": [tuple(w) for w in wt], "src_off": src_off, "out_off": out_off, "out_numel": max(o, 16), "src_numel": s,
            "sizes": [(int(H), int(W)) for H, W in sizes], "win": int(win), "stride": int(stride), "ncand": int(ncand)}


def to_device_async(rows, device, dtype=torch.int64):
    """A small host table -> device tensor without a host wait: a copy from pageable memory makes the host wait for the stream's queued
    work (which would stall the evaluation pipeline's next encoder behind this batch), one from pinned memory does not."""
    t = torch.tensor(rows, dtype=dtype)
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else t


def slide_extract(images_flat, plan, start=0, count=None):
    """images_flat: the images' [3,H,W] fp32 pixels packed at plan['src_off'] -> windows start .. start+count-1 as [count, 3, win, win]
    (zero past an image's border)."""
    require_gpu(images_flat)
    if images_flat.dtype != torch.float32 or images_flat.numel() != plan["src_numel"]:
        raise ValueError(f"slide_extract: {plan['src_numel']} packed fp32 pixels expected, got {images_flat.numel()} {images_flat.dtype}")
    count = len(plan["windows"]) - start if count is None else count
    if count <= 0 or start < 0 or start + count > len(plan["windows"]):
        raise ValueError(f"slide_extract: windows {start}..{start + count - 1} of {len(plan['windows'])}")
    win = plan["win"]
    out = torch.empty(count, 3, win, win, device=images_flat.device, dtype=torch.float32)
    call("simseg_slide_extract", ptr(_c(images_flat)), ptr(plan["img_tab"]), ptr(plan["win_tab"][start:]), ptr(out), count, win, stream())
    return out


def slide_scores(win_scores, plan):
    """win_scores [Nw, C] fp32 -> [B, C]: per image the mean of its windows' rows (fp32 sum in window order, divided once)."""
    require_gpu(win_scores)
    Nw, C = win_scores.shape
    if win_scores.dtype != torch.float32 or Nw != len(plan["windows"]):
        raise ValueError(f"slide_scores: fp32 [{len(plan['windows'])}, C] expected, got {tuple(win_scores.shape)} {win_scores.dtype}")
    B = len(plan["sizes"])
    out = torch.empty(B, C, device=win_scores.device, dtype=torch.float32)
    call("simseg_slide_scores", ptr(_c(win_scores)), ptr(plan["img_tab"]), ptr(out), B, C, stream())
    return out


def slide_stitch(sim_w, plan, cand_idx):
    """sim_w [Nw, n*n, C] fp32 per-window maps, cand_idx [B, ncand] -> (prob fp32, mask uint8, minmax [B, ncand, 2]): prob / mask flat,
    image b's [ncand, H, W] planes at plan['out_off'][b] (slide_planes() cuts the views); visited slots only (the others stay zero)."""
    require_gpu(sim_w, cand_idx)
    Nw, N, C = sim_w.shape
    win, K, B = plan["win"], plan["ncand"], len(plan["sizes"])
    n = win // 16
    if sim_w.dtype != torch.float32 or Nw != len(plan["windows"]) or N != n * n or tuple(cand_idx.shape) != (B, K):
        raise ValueError(f"slide_stitch: fp32 [{len(plan['windows'])}, {n * n}, C] maps and [{B}, {K}] candidates expected, "
                         f"got {tuple(sim_w.shape)} {sim_w.dtype}, {tuple(cand_idx.shape)}")
    dev = sim_w.device
    max_h = max(h for h, _ in plan["sizes"]); max_w = max(w for _, w in plan["sizes"]); max_hw = max(h * w for h, w in plan["sizes"])
    prob = torch.zeros(plan["out_numel"], device=dev, dtype=torch.float32)
    mask = torch.zeros(plan["out_numel"], device=dev, dtype=torch.uint8)
    minmax = torch.zeros(B, K, 2, device=dev, dtype=torch.float32)
    ws = torch.empty(raw("simseg_slide_stitch_workspace_bytes", B, K, max_h, max_w) // 4, device=dev, dtype=torch.float32)
    call("simseg_slide_stitch", ptr(_c(sim_w)), ptr(plan["img_tab"]), ptr(plan["win_tab"]), ptr(_c(cand_idx)), ptr(prob), ptr(mask), ptr(minmax),
         ptr(ws), B, K, n, C, win, max_h, max_w, max_hw, stream())
    return prob, mask, minmax


def slide_planes(flat, plan, b):
    """Image b's [ncand, H, W] view of a flat slide_stitch output."""
    H, W = plan["sizes"][b]
    o = plan["out_off"][b]
    return flat[o:o + plan["ncand"] * H * W].view(plan["ncand"], H, W)


# ---- multi-scale / flip test-time augmentation over sliding windows (segpost.encode_images_multiscale; include/simseg_hip.h) ------------
def slide_extract_flip(images_flat, plan, start=0, count=None, flip=True):
    """slide_extract() on the left-to-right MIRRORED images (flip=True): the windows of `plan` cut from torch.flip(image, [-1]) without
    that copy being made; flip=False is slide_extract()."""
    require_gpu(images_flat)
    if images_flat.dtype != torch.float32 or images_flat.numel() != plan["src_numel"]:
        raise ValueError(f"slide_extract_flip: {plan['src_numel']} packed fp32 pixels expected, got {images_flat.numel()} {images_flat.dtype}")
    count = len(plan["windows"]) - start if count is None else count
    if count <= 0 or start < 0 or start + count > len(plan["windows"]):
        raise ValueError(f"slide_extract_flip: windows {start}..{start + count - 1} of {len(plan['windows'])}")
    win = plan["win"]
    out = torch.empty(count, 3, win, win, device=images_flat.device, dtype=torch.float32)
    call("simseg_slide_extract_flip", ptr(_c(images_flat)), ptr(plan["img_tab"]), ptr(plan["win_tab"][start:]), ptr(out), count, win, int(bool(flip)),
         stream())
    return out


def slide_stitch_multi(sims, plans, flips, base_plan, cand_idx):
    """The fused map of P passes (DESIGN.md "Multi-scale and flip test-time augmentation"): sims[p] [Nw_p, n*n, C] fp32 = pass p's per-window
    maps over its slide_plan plans[p] (the same images at the pass's scale, mirrored when flips[p]); base_plan: the slide_plan of the images
    at their base sizes; cand_idx [B, ncand].  -> (prob, mask, minmax) in slide_stitch's layout for base_plan.  The number of passes is
    bounded by the library (16), which refuses more before any launch."""
    P = len(sims)
    if P == 0 or len(plans) != P or len(flips) != P:
        raise ValueError(f"slide_stitch_multi: {P} maps, {len(plans)} plans and {len(flips)} flip flags: one of each per pass expected")
    require_gpu(cand_idx, *sims)
    win, K, B = base_plan["win"], base_plan["ncand"], len(base_plan["sizes"])
    n = win // 16
    C = sims[0].shape[2] if sims[0].dim() == 3 else -1
    if tuple(cand_idx.shape) != (B, K):
        raise ValueError(f"slide_stitch_multi: [{B}, {K}] candidates expected, got {tuple(cand_idx.shape)}")
    for p, (s, pl) in enumerate(zip(sims, plans)):
        if len(pl["sizes"]) != B or pl["win"] != win:
            raise ValueError(f"slide_stitch_multi: pass {p} has {len(pl['sizes'])} images and {pl['win']}-pixel windows, the base plan {B} and {win}")
        if s.dtype != torch.float32 or s.dim() != 3 or tuple(s.shape) != (len(pl["windows"]), n * n, C):
            raise ValueError(f"slide_stitch_multi: pass {p}: fp32 [{len(pl['windows'])}, {n * n}, {C}] maps expected, got {tuple(s.shape)} {s.dtype}")
    dev = cand_idx.device
    sims = [_c(s) for s in sims]                        # (kept until the launch is queued: the table below holds their addresses)
    tab = to_device_async([[s.data_ptr(), pl["img_tab"].data_ptr(), pl["win_tab"].data_ptr(), int(bool(f))] for s, pl, f in zip(sims, plans, flips)], dev)
    sizes = base_plan["sizes"]
    max_h = max(h for h, _ in sizes); max_w = max(w for _, w in sizes); max_hw = max(h * w for h, w in sizes)
    prob = torch.zeros(base_plan["out_numel"], device=dev, dtype=torch.float32)
    mask = torch.zeros(base_plan["out_numel"], device=dev, dtype=torch.uint8)
    minmax = torch.zeros(B, K, 2, device=dev, dtype=torch.float32)
    ws = torch.empty(raw("simseg_slide_stitch_multi_workspace_bytes", B, K, max_h, max_w) // 4, device=dev, dtype=torch.float32)
    call("simseg_slide_stitch_multi", ptr(tab), P, ptr(base_plan["img_tab"]), ptr(_c(cand_idx)), ptr(prob), ptr(mask), ptr(minmax), ptr(ws), B, K, n, C,
         win, max_h, max_w, max_hw, stream())
    return prob, mask, minmax


# ---- image preprocessing and training augmentation on the device (simseg_amd/preproc.py, augment.py, pipeline.py; include/simseg_hip.h) -----------------------
def _check_packed_batch(who, src, plan, lut, cols, need_2d=False):
    """What image_preprocess and train_augment ask of their arguments: the packed source, the look-up table, and host copies of the
    tables ([B, cols] image table) that the C entry point can read.  -> (img_tab_host, tab_host)."""
    require_gpu(src, lut, plan["img_tab"], plan["tab"])
    if src.dtype != torch.uint8 or src.numel() != plan["src_bytes"]:
        raise ValueError(f"{who}: {plan['src_bytes']} packed uint8 bytes expected, got {src.numel()} {src.dtype}")
    if lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256):
        raise ValueError(f"{who}: fp32 [3, 256] look-up table expected, got {tuple(lut.shape)} {lut.dtype}")
    it, th = plan["img_tab_host"], plan["tab_host"]
    if it.dtype != "int64" or th.dtype != "int32" or not it.flags.c_contiguous or not th.flags.c_contiguous or \
            (need_2d and it.ndim != 2) or tuple(plan["img_tab"].shape) != it.shape or plan["tab"].numel() != th.size:
        raise ValueError(f"{who}: the host copies of the tables are contiguous int64 [B, {cols}] / int32 arrays of the device tables' sizes")
    return it, th


def image_preprocess(src, plan, lut, want_u8=False):
    """src: the batch's uint8 [H, W, 3] images packed at plan['src_off'] (preproc.plan) -> (fp32 flat, image b's [3, OH, OW] planes at
    plan['out_off'][b]; uint8 flat with its [OH, OW, 3] bytes at the same offset, or None).  The tables are checked on their host copies
    before the launch."""
    it, th = _check_packed_batch("image_preprocess", src, plan, lut, 16)
    out = torch.empty(plan["out_numel"], device=src.device, dtype=torch.float32)
    u8 = torch.empty(plan["out_numel"], device=src.device, dtype=torch.uint8) if want_u8 else None
    call("simseg_image_preprocess", ptr(_c(src)), src.numel(), ptr(plan["img_tab"]), it.ctypes.data, it.shape[0], ptr(plan["tab"]), th.ctypes.data,
         th.size, ptr(_c(lut)), ptr(out), out.numel(), ptr(u8), 0 if u8 is None else u8.numel(), stream())
    return out, u8


def train_augment(src, plan, lut, want_u8=False):
    """src: the batch's uint8 [H, W, 3] images packed at plan['src_off'] (augment.plan) -> (fp32 [B, 3, S, S], uint8 [B, S, S, 3] or
    None).  Two launches; the tables and parameters are checked on their host copies before them."""
    it, th = _check_packed_batch("train_augment", src, plan, lut, 30, need_2d=True)
    B, S = it.shape[0], plan["size"]
    dev = src.device
    scratch = torch.empty(max(raw("simseg_train_augment_scratch_bytes", B, S), 16), device=dev, dtype=torch.uint8)
    out = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32)
    u8 = torch.empty(B, S, S, 3, device=dev, dtype=torch.uint8) if want_u8 else None
    call("simseg_train_augment", ptr(_c(src)), src.numel(), ptr(plan["img_tab"]), it.ctypes.data, B, ptr(plan["tab"]), th.ctypes.data, th.size,
         ptr(_c(lut)), S, ptr(scratch), scratch.numel(), ptr(out), out.numel(), ptr(u8), 0 if u8 is None else u8.numel(), stream())
    return out, u8


def train_transforms(src, plan, lut, want_u8=False):
    """src: the batch's uint8 [H, W, 3] images packed at plan['src_off'] (pipeline.plan_pipeline) -> (fp32 [B, 3, S, S], uint8
    [B, S, S, 3] = the bytes before normalisation and erasing, or None).  Two launches; every field of the table is checked on its host
    copy before them."""
    it, th = _check_packed_batch("train_transforms", src, plan, lut, 81, need_2d=True)
    B, S = it.shape[0], plan["size"]
    dev = src.device
    scratch = torch.empty(max(raw("simseg_train_transforms_scratch_bytes", B, S), 16), device=dev, dtype=torch.uint8)
    out = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32)
    u8 = torch.empty(B, S, S, 3, device=dev, dtype=torch.uint8) if want_u8 else None
    call("simseg_train_transforms", ptr(_c(src)), src.numel(), ptr(plan["img_tab"]), it.ctypes.data, B, ptr(plan["tab"]), th.ctypes.data,
         th.size, ptr(_c(lut)), S, ptr(scratch), scratch.numel(), ptr(out), out.numel(), ptr(u8), 0 if u8 is None else u8.numel(), stream())
    return out, u8


def train_chain(src, plan, lut, want_u8=False):
    """train_transforms for a chain of the full grammar (pipeline.parse_chain(full=True)): the 144-column table with up to twelve ops,
    grayscale, hue shift and Gaussian blur among them.  Same arguments, same results, same two launches."""
    it, th = _check_packed_batch("train_chain", src, plan, lut, 144, need_2d=True)
    if it.shape[1] != 144:
        raise ValueError(f"train_chain: the image table has 144 columns, got {it.shape[1]} (a plan of the old grammar goes to train_transforms)")
    B, S = it.shape[0], plan["size"]
    dev = src.device
    scratch = torch.empty(max(raw("simseg_train_chain_scratch_bytes", B, S), 16), device=dev, dtype=torch.uint8)
    out = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32)
    u8 = torch.empty(B, S, S, 3, device=dev, dtype=torch.uint8) if want_u8 else None
    call("simseg_train_chain", ptr(_c(src)), src.numel(), ptr(plan["img_tab"]), it.ctypes.data, B, ptr(plan["tab"]), th.ctypes.data,
         th.size, ptr(_c(lut)), S, ptr(scratch), scratch.numel(), ptr(out), out.numel(), ptr(u8), 0 if u8 is None else u8.numel(), stream())
    return out, u8


# ---- linear-probe task (csrc/probe.hip; LARS: csrc/optim.hip) --------------------------------------------------------------------
CE_MAX_CLASSES = 65536         # simseg_ce_rows: 1 <= C <= 65536


def ce_rows(logits, labels, write_grad=True):
    """Cross-entropy with integer class labels, top-1 / top-5 hits and the logit gradient of the MEAN loss in one pass over logits [B, C]
    (fp32, bf16 or fp16; labels int64 [B] on the device).  -> (out3, loss_rows, ranks, dlogits): out3 fp32 [3] = {mean loss, top-1 count,
    top-5 count}, loss_rows fp32 [B], ranks int32 [B] (how many classes rank ahead of the label's; equal logits by ascending class id),
    dlogits fp32 [B, C] = (softmax - onehot) / B, or None when write_grad is False.  A label outside [0, C): NaN loss row, rank
    2^31 - 1, zero gradient row (include/simseg_hip.h)."""
    require_gpu(logits, labels)
    if logits.dim() != 2 or labels.shape != logits.shape[:1]:
        raise ValueError(f"ce_rows: logits [B, C] and labels [B], got {tuple(logits.shape)} and {tuple(labels.shape)}")
    if labels.dtype != torch.int64:
        raise TypeError(f"ce_rows: labels must be int64, got {labels.dtype}")
    B, C = logits.shape
    dev = logits.device
    loss_rows = torch.empty(B, device=dev, dtype=torch.float32)
    ranks = torch.empty(B, device=dev, dtype=torch.int32)
    out3 = torch.empty(3, device=dev, dtype=torch.float32)
    dlogits = torch.empty(B, C, device=dev, dtype=torch.float32) if write_grad else None
    call("simseg_ce_rows", ptr(_c(logits)), dt(logits), ptr(_c(labels)), ptr(loss_rows), ptr(ranks), ptr(dlogits), ptr(out3), B, C,
         1.0 / max(B, 1), int(bool(write_grad)), stream())
    return out3, loss_rows, ranks, dlogits


def soft_ce_rows(logits, labels_a, labels_b, lam, smoothing=0.0, write_grad=True):
    """ce_rows against the two-label soft target t = lam * s(a) + (1 - lam) * s(b), s(y) = (1 - smoothing) * onehot(y) + smoothing / C
    (timm's mixup_target; a == b, lam = 1: label smoothing), with no dense target: labels_a / labels_b int64 [B], lam fp32 [B], all on the
    device.  -> (out3, loss_rows, ranks, dlogits) laid out as ce_rows'; ranks and the two counts are those of labels_a; dlogits =
    (softmax - t) / B.  lam = 1, smoothing = 0 gives ce_rows' bits.  A label outside [0, C) in either vector: NaN loss row, rank
    2^31 - 1, zero gradient row (include/simseg_hip.h)."""
    require_gpu(logits, labels_a, labels_b, lam)
    if logits.dim() != 2 or labels_a.shape != logits.shape[:1] or labels_b.shape != logits.shape[:1] or lam.shape != logits.shape[:1]:
        raise ValueError(f"soft_ce_rows: logits [B, C] and labels_a, labels_b, lam [B], got {tuple(logits.shape)}, {tuple(labels_a.shape)}, "
                         f"{tuple(labels_b.shape)} and {tuple(lam.shape)}")
    if labels_a.dtype != torch.int64 or labels_b.dtype != torch.int64:
        raise TypeError(f"soft_ce_rows: labels must be int64, got {labels_a.dtype} and {labels_b.dtype}")
    if lam.dtype != torch.float32:
        raise TypeError(f"soft_ce_rows: lam must be fp32, got {lam.dtype}")
    B, C = logits.shape
    dev = logits.device
    loss_rows = torch.empty(B, device=dev, dtype=torch.float32)
    ranks = torch.empty(B, device=dev, dtype=torch.int32)
    out3 = torch.empty(3, device=dev, dtype=torch.float32)
    dlogits = torch.empty(B, C, device=dev, dtype=torch.float32) if write_grad else None
    call("simseg_soft_ce_rows", ptr(_c(logits)), dt(logits), ptr(_c(labels_a)), ptr(_c(labels_b)), ptr(_c(lam)), float(smoothing), ptr(loss_rows),
         ptr(ranks), ptr(dlogits), ptr(out3), B, C, 1.0 / max(B, 1), int(bool(write_grad)), stream())
    return out3, loss_rows, ranks, dlogits


# ---- Mixup / CutMix (csrc/mixup.hip; simseg_amd/mixup.py) --------------------------------------------------------------------------------
def mix_batch(images, table_dev, table_host):
    """Mixup / CutMix of images [B, C, H, W] (fp32, bf16 or fp16; contiguous; B even) with its flipped self, IN PLACE, one launch.
    table_dev int32 [B, 8] on the device and table_host, its host copy (a contiguous int32 numpy array): per sample {kind, yl, yh, xl,
    xh, lam bits, om bits, 0} (simseg_amd.mixup; include/simseg_hip.h).  The host copy is checked before the launch.  -> images."""
    require_gpu(images, table_dev)
    if images.dim() != 4:
        raise ValueError(f"mix_batch: images [B, C, H, W] expected, got {tuple(images.shape)}")
    B, C, H, W = images.shape
    if table_dev.dtype != torch.int32 or tuple(table_dev.shape) != (B, 8):
        raise ValueError(f"mix_batch: int32 [{B}, 8] device table expected, got {tuple(table_dev.shape)} {table_dev.dtype}")
    if getattr(table_host, "dtype", None) != "int32" or table_host.shape != (B, 8) or not table_host.flags.c_contiguous:
        raise ValueError(f"mix_batch: the host copy of the table is a contiguous int32 [{B}, 8] numpy array")
    if not images.is_contiguous():
        raise RuntimeError("mix_batch: the batch must be contiguous [B, C, H, W] (it is mixed in place)")
    call("simseg_mix_batch", ptr(images), dt(images), ptr(_c(table_dev)), table_host.ctypes.data, B, C, H, W, stream())
    return images


def lars_norm_partials(tab, partials):
    """partials float64 [n_chunks, 2] <- per chunk {sum p^2, sum g^2} of the tensor table `tab` (a simseg_amd.optim.TensorTable with
    LARS's rows)."""
    if partials.dtype != torch.float64 or partials.numel() < 2 * tab.n_chunks:
        raise TypeError("lars_norm_partials: partials must be float64 [n_chunks, 2]")
    call("simseg_lars_norm_partials", *tab.launch_args(host=True), ptr(partials), stream())
    return partials


def lars_finish(tab, partials, eta, eps, local_lr):
    """local_lr fp32 [n_tensors] <- eta * |p| / (|g| + weight_decay * |p| + eps) per tensor (1 where a norm is zero or the tensor is
    lars_exclude), from the partials of lars_norm_partials.  No host read."""
    if local_lr.dtype != torch.float32 or local_lr.numel() < tab.n_tensors:
        raise TypeError("lars_finish: local_lr must be fp32 [n_tensors]")
    call("simseg_lars_finish", ptr(tab.table), ptr(tab.first), tab.first_host.ctypes.data, ptr(partials), tab.n_tensors, tab.n_chunks,
         float(eta), float(eps), ptr(local_lr), stream())
    return local_lr


def lars_multi_step(tab, local_lr, momentum, dampening, nesterov):
    """The LARS update of every tensor of the table in one launch (masters, momentum buffers and 16-bit copies in place)."""
    call("simseg_lars_multi_step", *tab.launch_args(host=True), ptr(local_lr), float(momentum), float(dampening), int(bool(nesterov)), stream())
