// Row kernels of the encoder path that do not depend on the selected 16-bit type: [cls]+pos rows (K2), BERT embedding gather/scatter (K9),
// the prompt-ensemble mean, the fp32 transpose, the fp32 -> three-bf16-pieces split (always bf16) and the byte-wise row gather.
// Compiled ONCE; the kernels with a bf16 / fp16 flavour are in rowops.hip.
#include "common.h"

namespace {

// x[b, 0, :] = cls + pos[0]   (vit_builder.py:15-17; the patch rows are written by the patch GEMM epilogue)
__global__ void vit_cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x,
                                    int B, int T, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, d = i % D;
    x[(long)b * T * D + d] = cls[d] + pos[d];
}
// backward: dcls += sum_b dx[b,0,:],  dpos[0] handled by the position column-sum over all rows
// (blockIdx.y: slices of 16 images - three blocks walking all 512 rows serially, each load a DRAM latency, took 195 us; one atomic per
//  column and slice)
__global__ void vit_cls_grad_kernel(const float* __restrict__ dx, float* __restrict__ dcls, int B, int T, int D) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const int b0 = blockIdx.y * 16, b1 = min(B, b0 + 16);
    float s = 0.f;
#pragma unroll 8
    for (int b = b0; b < b1; ++b) s += dx[(long)b * T * D + d];
    atomicAdd(dcls + d, s);
}

// ---------------------------------------------------------------------------------------------
// BERT embeddings (HF BertEmbeddings): sum[b,l,:] = word[id] + pos[l] + type[0]     (LayerNorm runs next)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bert_embed_kernel(const long* __restrict__ ids, const float* __restrict__ word,
                                                         const float* __restrict__ pos, const float* __restrict__ type0,
                                                         float* __restrict__ out, int rows, int L, int D, int vocab) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    long id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const int l = row % L;
    for (int c = lane; c < (D >> 2); c += 64) {
        float a[4], b[4], t[4], o[4];
        load4<float>(word + id * D + c * 4, a);
        load4<float>(pos + (long)l * D + c * 4, b);
        load4<float>(type0 + c * 4, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = a[j] + t[j] + b[j];
        store4<float>(out + (long)row * D + c * 4, o);
    }
}
// backward: dword[id] += dsum[row] for valid (unmasked) tokens.  Masked tokens carry an exactly-zero gradient
// (they are masked as keys and overwritten before pooling), so they are skipped.
__global__ __launch_bounds__(256) void bert_embed_bwd_kernel(const long* __restrict__ ids, const long* __restrict__ mask,
                                                             const float* __restrict__ dsum, float* __restrict__ dword,
                                                             int rows, int D, int vocab) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    if (mask && mask[row] == 0) return;
    long id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    for (int c = lane; c < D; c += 64) atomicAdd(dword + id * D + c, dsum[(long)row * D + c]);
}

// Prompt-ensemble reduction of the zero-shot classifier (tools/seg_evaluation.py:71-73): out[s,:] = normalize(mean_p x[s,p,:])
__global__ void segment_mean_l2norm_kernel(const float* __restrict__ x, float* __restrict__ out, int Pn, int D) {
    __shared__ float sh[16];
    const int sgm = blockIdx.x, c = threadIdx.x;
    const float* base = x + (long)sgm * Pn * D + c;
    float acc = 0.f;
    for (int i = 0; i < Pn; ++i) acc += base[(long)i * D];
    acc /= Pn;
    const float nrm = sqrtf(block_sum(acc * acc, sh));
    out[(long)sgm * D + c] = acc / nrm;
}

// out[c, r] = in[r, c]  (fp32, 32x32 LDS tiles)
__global__ void transpose_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) t[j][tx] = in[(long)(r0 + j) * C + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) out[(long)(c0 + j) * R + r0 + tx] = t[tx][j];
}

// ---- fp32 operand -> three bf16 pieces, laid out for ONE bf16 GEMM that reproduces the fp32 product -----------------------------
// x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): three round-to-nearest pieces of 8 significant
// bits each carry x's 24 (bf16 has fp32's exponent range, so the residuals are exact and in range).  A product a.b is then the sum
// of nine piece products; the three smallest (mid.lo, lo.mid, lo.lo <= 2^-24 |a||b|) are dropped, like the rounding of the fp32 FMA
// chain they replace.  The six kept ones are laid out along K - the A operand as [hi | hi | hi | mid | mid | lo], the B operand as
// [hi | mid | lo | hi | mid | hi], K' = 6 K - so that one launch of the bf16 MFMA kernel (v_mfma_f32_32x32x16_bf16, fp32 accumulate)
// forms all of them in its accumulators: six times the MFMA work at sixteen times the matrix rate of v_mfma_f32_32x32x2_f32.
// One thread per 8 consecutive k of a row: 32 B in, six 16-byte stores out.  The pieces are bf16 whatever 16-bit type the caller has
// selected (fp16's five exponent bits could not hold the residuals).
__global__ __launch_bounds__(256) void split_bf16x3_kernel(const float* __restrict__ in, __bf16* __restrict__ out, long rows, int K, long ld_in, int bpat) {
    const int kc = K >> 3;
    const long total = rows * kc;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const long r = t / kc;
        const int k0 = (int)(t - r * kc) << 3;
        const float4 a = *reinterpret_cast<const float4*>(in + r * ld_in + k0), b = *reinterpret_cast<const float4*>(in + r * ld_in + k0 + 4);
        const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        union { __bf16 h[8]; u32x4 v; } hi, mid, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi.h[e] = (__bf16)x[e];
            const float r1 = x[e] - (float)hi.h[e];
            mid.h[e] = (__bf16)r1;
            lo.h[e] = (__bf16)(r1 - (float)mid.h[e]);
        }
        if (bpat == 2) {                                 // three planes [piece][row][K] (the attention kernel's operand form)
            __bf16* o = out + r * (long)K + k0;
            *reinterpret_cast<u32x4*>(o) = hi.v;
            *reinterpret_cast<u32x4*>(o + rows * (long)K) = mid.v;
            *reinterpret_cast<u32x4*>(o + 2 * rows * (long)K) = lo.v;
            continue;
        }
        __bf16* o = out + r * (6L * K) + k0;
        // A pattern: hi hi hi mid mid lo;  B pattern: hi mid lo hi mid hi
        *reinterpret_cast<u32x4*>(o) = hi.v;
        *reinterpret_cast<u32x4*>(o + K) = bpat ? mid.v : hi.v;
        *reinterpret_cast<u32x4*>(o + 2L * K) = bpat ? lo.v : hi.v;
        *reinterpret_cast<u32x4*>(o + 3L * K) = bpat ? hi.v : mid.v;
        *reinterpret_cast<u32x4*>(o + 4L * K) = mid.v;
        *reinterpret_cast<u32x4*>(o + 5L * K) = bpat ? hi.v : lo.v;
    }
}

// Row gather: dst[i,:] = src[idx[i],:] for i < n (idx < 0: a zero row).  Rows are `chunks` 16-byte pieces wide; dtype-agnostic.
// The text tower uses it to drop the padded token rows of a ragged caption batch before its GEMMs / LayerNorms and to put rows back
// (idx = inverse map, -1 at padded positions -> zeros) around the attention kernels, which keep the dense [B, L] layout.
__global__ __launch_bounds__(256) void gather_rows_kernel(const u32x4* __restrict__ src, const int* __restrict__ idx, u32x4* __restrict__ dst,
                                                          long n, int chunks) {
    const long total = n * chunks;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const long i = t / chunks;
        const int c = (int)(t - i * chunks);
        const int r = idx[i];
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r >= 0) v = src[(long)r * chunks + c];
        dst[t] = v;
    }
}

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" int simseg_vit_cls_rows(const float* cls, const float* pos, float* x, int64_t B, int64_t T, int64_t D, void* stream) {
    SS_CHECK(cls && pos && x, "vit_cls_rows: null pointer");
    if (B <= 0) return 0;
    hipLaunchKernelGGL(vit_cls_rows_kernel, dim3((unsigned)((B * D + 255) / 256)), dim3(256), 0, STREAM, cls, pos, x, (int)B, (int)T, (int)D);
    SS_LAUNCH_CHECK("vit_cls_rows");
    return 0;
}

extern "C" int simseg_vit_cls_grad(const float* dx, float* dcls, int64_t B, int64_t T, int64_t D, void* stream) {
    SS_CHECK(dx && dcls, "vit_cls_grad: null pointer");
    if (B <= 0 || D <= 0) return 0;
    hipLaunchKernelGGL(vit_cls_grad_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)((B + 15) / 16)), dim3(256), 0, STREAM, dx, dcls, (int)B, (int)T, (int)D);
    SS_LAUNCH_CHECK("vit_cls_grad");
    return 0;
}

extern "C" int simseg_bert_embed_fwd(const int64_t* ids, const float* word, const float* pos, const float* type0, float* out,
                                     int64_t B, int64_t L, int64_t D, int64_t vocab, void* stream) {
    SS_CHECK(ids && word && pos && type0 && out, "bert_embed_fwd: null pointer");
    SS_CHECK(D % 4 == 0, "bert_embed_fwd: D must be a multiple of 4");
    const long rows = B * L;
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(bert_embed_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, STREAM, (const long*)ids, word, pos, type0, out,
                       (int)rows, (int)L, (int)D, (int)vocab);
    SS_LAUNCH_CHECK("bert_embed_fwd");
    return 0;
}

extern "C" int simseg_bert_embed_bwd(const int64_t* ids, const int64_t* mask, const float* dsum, float* dword, int64_t B,
                                     int64_t L, int64_t D, int64_t vocab, void* stream) {
    SS_CHECK(ids && dsum && dword, "bert_embed_bwd: null pointer");
    const long rows = B * L;
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(bert_embed_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, STREAM, (const long*)ids, (const long*)mask, dsum,
                       dword, (int)rows, (int)D, (int)vocab);
    SS_LAUNCH_CHECK("bert_embed_bwd");
    return 0;
}

extern "C" int simseg_segment_mean_l2norm(const float* x, float* out, int64_t S, int64_t P, int64_t D, void* stream) {
    SS_CHECK(x && out, "segment_mean_l2norm: null pointer");
    SS_CHECK(D % 64 == 0 && D <= 1024 && P >= 1, "segment_mean_l2norm: D must be a multiple of 64 and <= 1024");
    if (S <= 0) return 0;
    hipLaunchKernelGGL(segment_mean_l2norm_kernel, dim3((unsigned)S), dim3((unsigned)D), 0, STREAM, x, out, (int)P, (int)D);
    SS_LAUNCH_CHECK("segment_mean_l2norm");
    return 0;
}

extern "C" int simseg_split_bf16x3(const float* in, void* out, int64_t rows, int64_t K, int64_t ld_in, int b_pattern, void* stream) {
    SS_CHECK(in && out, "split_bf16x3: null pointer");
    SS_CHECK(K > 0 && K % 8 == 0 && ld_in >= K && ld_in % 4 == 0, "split_bf16x3: K must be a multiple of 8 (got %lld)", (long long)K);
    SS_CHECK(((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0, "split_bf16x3: operands must be 16-byte aligned");
    if (rows <= 0) return 0;
    const int grid = grid_for(rows * (K / 8), 256, 16384);
    hipLaunchKernelGGL(split_bf16x3_kernel, dim3(grid), dim3(256), 0, STREAM, in, (__bf16*)out, (long)rows, (int)K, (long)ld_in, b_pattern);
    SS_LAUNCH_CHECK("split_bf16x3");
    return 0;
}

extern "C" int simseg_transpose_f32(const float* in, float* out, int64_t R, int64_t C, void* stream) {
    SS_CHECK(in && out, "transpose: null pointer");
    if (R <= 0 || C <= 0) return 0;
    dim3 grid((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32));
    hipLaunchKernelGGL(transpose_f32_kernel, grid, dim3(256), 0, STREAM, in, out, (int)R, (int)C);
    SS_LAUNCH_CHECK("transpose");
    return 0;
}

extern "C" int simseg_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n, int64_t row_bytes, void* stream) {
    SS_CHECK(src && idx && dst, "gather_rows: null pointer");
    SS_CHECK(row_bytes > 0 && row_bytes % 16 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0,
             "gather_rows: rows must be multiples of 16 bytes and 16-byte aligned");
    if (n <= 0) return 0;
    const long total = n * (row_bytes / 16);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)grid_for(total, 256, 16384)), dim3(256), 0, STREAM, (const u32x4*)src, idx, (u32x4*)dst,
                       (long)n, (int)(row_bytes / 16));
    SS_LAUNCH_CHECK("gather_rows");
    return 0;
}
