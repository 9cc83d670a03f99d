// Linear-probe task (simseg/tasks/linear_prob, simseg/models/pipelines/linear_prob.py of the reference): cross-entropy rows over integer
// class labels with top-1 / top-5 hits and the logit gradient in one pass - also against the two-label soft target of a Mixup / CutMix
// batch (the same kernels, SOFT).  (The task's optimizer, LARS, is in optim.hip.)  Compiled ONCE: the 16-bit flavour (bf16 / fp16) is a
// template argument chosen from the calling thread's simseg_set_half_type, so dtype code 1 means "the selected 16-bit type" as
// everywhere else in the ABI.
#include <float.h>
#include <limits.h>

#include "common.h"

namespace {

// 16 bytes of a row as floats: 4 fp32 or 8 16-bit elements per lane and load.
template <typename T>
struct Chunk;
template <>
struct Chunk<float> {
    static constexpr int VW = 4;
    static __device__ __forceinline__ void load(const float* p, float* v) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = t[e];
    }
};
template <typename H>
struct Chunk16 {
    static constexpr int VW = 8;
    typedef H h8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ void load(const H* p, float* v) {
        const h8 t = *reinterpret_cast<const h8*>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
    }
};
template <>
struct Chunk<__bf16> : Chunk16<__bf16> {};
template <>
struct Chunk<_Float16> : Chunk16<_Float16> {};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Does column j with value x rank ahead of the label's column y with value xy?  Strictly larger, or equal with a smaller class id
// (the order of search.hip: descending score, ascending index).
__device__ __forceinline__ int ahead(float x, int j, float xy, int y) { return (x > xy || (x == xy && j < y)) ? 1 : 0; }

// The two-label target of one row: t_c = wa [c == a] + wb [c == b] + u with wa = lam (1 - eps), wb = (1 - lam) (1 - eps), u = eps / C.
// The loss is formed relative to the row maximum m like the hard one (no rounded lse):
//   -sum_c t_c log softmax(x)_c = log(sum) + (1 - eps) (lam (m - x_a) + (1 - lam) (m - x_b)) - eps * mean_c(x_c - m).
struct SoftRow {
    float xb, la, om, conf, eps, u;
    __device__ SoftRow() {}
    __device__ SoftRow(float xb_, float lam, float eps_, int C) : xb(xb_), la(lam), om(1.f - lam), conf(1.f - eps_), eps(eps_), u(eps_ / (float)C) {}
    __device__ __forceinline__ float loss(float lsum, float m, float xa, float mean_rel) const {
        return lsum + conf * (la * (m - xa) + om * (m - xb)) - eps * mean_rel;
    }
    __device__ __forceinline__ float target(int c, int a, int b) const { return (c == a ? la * conf : 0.f) + (c == b ? om * conf : 0.f) + u; }
};

constexpr int CE_WAVE_MAXC = 1024;      // up to here a row is 16 values per lane: one wave keeps it in registers and reads it once
constexpr int CE_SLOTS = CE_WAVE_MAXC / 64;

// One WAVE per row, four rows per block, C <= 1024: the row is loaded once into registers (16 bytes per lane and load when the rows are
// 16-byte aligned: VEC), and max, sum of exponentials, rank count and the gradient all come from those registers; reductions are wave64
// butterflies, no LDS and no barrier.
// SOFT (simseg_soft_ce_rows): the target row is lam * s(a) + (1 - lam) * s(b), s(y) = (1 - eps) * onehot(y) + eps / C, with a = labels,
// b = labels_b; ranks stay those of a.  Every SOFT statement reduces to the hard one's value at lam = 1, eps = 0 (products with 1 and sums
// with 0 are exact), which the tests pin bit for bit; the hard instantiation compiles none of it.
template <typename T, bool VEC, bool SOFT>
__global__ __launch_bounds__(256) void ce_rows_wave_kernel(const T* __restrict__ logits, const long* __restrict__ labels,
                                                           const long* __restrict__ labels_b, const float* __restrict__ lam, float eps,
                                                           float* __restrict__ loss_rows, int* __restrict__ ranks,
                                                           float* __restrict__ dlogits, int B, int C, float gscale, int write_grad) {
    constexpr int VW = Chunk<T>::VW;
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;                                  // (wave-uniform)
    const T* row = logits + i * C;
    float v[CE_SLOTS];
    int col[CE_SLOTS];                                   // slot -> column (compile-time pattern, folded after unrolling)
#pragma unroll
    for (int s = 0; s < CE_SLOTS; ++s) col[s] = VEC ? ((s / VW) * 64 + lane) * VW + (s % VW) : s * 64 + lane;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < CE_SLOTS / VW; ++k) {
            const int j0 = (k * 64 + lane) * VW;         // (C % VW == 0: a chunk is inside the row or outside it)
            if (j0 < C) {
                Chunk<T>::load(row + j0, v + k * VW);
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e) v[k * VW + e] = -FLT_MAX;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < CE_SLOTS; ++s) v[s] = col[s] < C ? (float)row[col[s]] : -FLT_MAX;
    }
    const long y64 = labels[i];
    const long yb64 = SOFT ? labels_b[i] : y64;
    const bool ok = y64 >= 0 && y64 < C && yb64 >= 0 && yb64 < C;      // a label outside [0, C) never indexes the row
    const int y = ok ? (int)y64 : 0, yb = ok ? (int)yb64 : 0;
    const float xy = ok ? (float)row[y] : 0.f;
    const SoftRow sr = SOFT ? SoftRow(ok ? (float)row[yb] : 0.f, lam[i], eps, C) : SoftRow();
    float m = -FLT_MAX;
#pragma unroll
    for (int s = 0; s < CE_SLOTS; ++s) m = fmaxf(m, v[s]);
    m = wave_max(m);
    float se = 0.f, sd = 0.f;                            // (sd: sum of x_j - m, for the uniform part of a smoothed target)
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < CE_SLOTS; ++s) {
        if (col[s] < C) {
            se += expf(v[s] - m);
            cnt += ahead(v[s], col[s], xy, y);
            if (SOFT) sd += v[s] - m;
        }
    }
    se = wave_sum(se);
    cnt = wave_sum_int(cnt);
    if (SOFT) sd = wave_sum(sd);
    // lse = m + log(se) is never rounded on its own: loss = lse - x_y is formed as log(se) + (m - x_y) and exp(x_j - lse) as
    // exp((x_j - m) - log(se)) - the same values without an error of half an ulp of |lse| in each (for the columns that carry the
    // probability mass x_j - m is small and exact)
    const float lsum = logf(se);
    if (lane == 0) {
        const float loss = SOFT ? sr.loss(lsum, m, xy, sd / (float)C) : lsum + (m - xy);
        loss_rows[i] = ok ? loss : __int_as_float(0x7fc00000);
        ranks[i] = ok ? cnt : INT_MAX;
    }
    if (!write_grad) return;
    float* drow = dlogits + i * C;
    float g[CE_SLOTS];
#pragma unroll
    for (int s = 0; s < CE_SLOTS; ++s) {
        const float t = SOFT ? sr.target(col[s], y, yb) : (col[s] == y ? 1.f : 0.f);
        g[s] = ok ? (expf((v[s] - m) - lsum) - t) * gscale : 0.f;
    }
    if (VEC) {
#pragma unroll
        for (int k = 0; k < CE_SLOTS / VW; ++k) {
            const int j0 = (k * 64 + lane) * VW;
            if (j0 < C) {
#pragma unroll
                for (int q = 0; q < VW / 4; ++q) {
                    const f32x4 o = {g[k * VW + 4 * q], g[k * VW + 4 * q + 1], g[k * VW + 4 * q + 2], g[k * VW + 4 * q + 3]};
                    *reinterpret_cast<f32x4*>(drow + j0 + 4 * q) = o;
                }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < CE_SLOTS; ++s)
            if (col[s] < C) drow[col[s]] = g[s];
    }
}

// One BLOCK per row, C > 1024: pass 1 reads the row once and keeps a running maximum and a sum of exponentials relative to it per lane
// (rescaled when the maximum moves) beside the rank count; the lanes' pairs are merged against the block maximum in a fixed order (wave
// butterfly, then the four waves through LDS).  Pass 2 (write_grad) re-reads the row - it was just read, so from cache - and writes the
// gradient.
// SOFT: as in the wave kernel; the sum of the row for the uniform part is kept per lane in double (the maximum it is taken relative to is
// only known after the pass) and merged in the same fixed order.
template <typename T, bool VEC, bool SOFT>
__global__ __launch_bounds__(256) void ce_rows_block_kernel(const T* __restrict__ logits, const long* __restrict__ labels,
                                                            const long* __restrict__ labels_b, const float* __restrict__ lam, float eps,
                                                            float* __restrict__ loss_rows, int* __restrict__ ranks,
                                                            float* __restrict__ dlogits, int C, float gscale, int write_grad) {
    constexpr int VW = Chunk<T>::VW;
    __shared__ float shf[4];
    __shared__ int shi[4];
    __shared__ double shd[4];
    const int tid = threadIdx.x;
    const long i = blockIdx.x;
    const T* row = logits + i * C;
    const long y64 = labels[i];
    const long yb64 = SOFT ? labels_b[i] : y64;
    const bool ok = y64 >= 0 && y64 < C && yb64 >= 0 && yb64 < C;
    const int y = ok ? (int)y64 : 0, yb = ok ? (int)yb64 : 0;
    const float xy = ok ? (float)row[y] : 0.f;
    const SoftRow sr = SOFT ? SoftRow(ok ? (float)row[yb] : 0.f, lam[i], eps, C) : SoftRow();
    float m = -FLT_MAX, se = 0.f;
    double sx = 0.0;
    int cnt = 0;
    if (VEC) {
        for (int j0 = tid * VW; j0 < C; j0 += 256 * VW) {
            float v[VW];
            Chunk<T>::load(row + j0, v);
            float vm = v[0];
#pragma unroll
            for (int e = 1; e < VW; ++e) vm = fmaxf(vm, v[e]);
            if (vm > m) {
                se *= expf(m - vm);
                m = vm;
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                se += expf(v[e] - m);
                cnt += ahead(v[e], j0 + e, xy, y);
                if (SOFT) sx += (double)v[e];
            }
        }
    } else {
        for (int j = tid; j < C; j += 256) {
            const float x = (float)row[j];
            if (x > m) {
                se *= expf(m - x);
                m = x;
            }
            se += expf(x - m);
            cnt += ahead(x, j, xy, y);
            if (SOFT) sx += (double)x;
        }
    }
    float bm = wave_max(m);
    if ((tid & 63) == 0) shf[tid >> 6] = bm;
    __syncthreads();
    bm = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
    __syncthreads();
    se = wave_sum(se * expf(m - bm));
    cnt = wave_sum_int(cnt);
    if (SOFT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o, 64);
    }
    if ((tid & 63) == 0) {
        shf[tid >> 6] = se;
        shi[tid >> 6] = cnt;
        if (SOFT) shd[tid >> 6] = sx;
    }
    __syncthreads();
    se = (shf[0] + shf[1]) + (shf[2] + shf[3]);
    cnt = (shi[0] + shi[1]) + (shi[2] + shi[3]);
    const float lsum = logf(se);                         // (lse = bm + lsum is not rounded on its own: see the wave kernel)
    if (tid == 0) {
        float loss = lsum + (bm - xy);
        if (SOFT) loss = sr.loss(lsum, bm, xy, (float)(((shd[0] + shd[1]) + (shd[2] + shd[3])) / (double)C - (double)bm));
        loss_rows[i] = ok ? loss : __int_as_float(0x7fc00000);
        ranks[i] = ok ? cnt : INT_MAX;
    }
    if (!write_grad) return;
    float* drow = dlogits + i * C;
    if (VEC) {
        for (int j0 = tid * VW; j0 < C; j0 += 256 * VW) {
            float v[VW];
            Chunk<T>::load(row + j0, v);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const float t = SOFT ? sr.target(j0 + e, y, yb) : (j0 + e == y ? 1.f : 0.f);
                v[e] = ok ? (expf((v[e] - bm) - lsum) - t) * gscale : 0.f;
            }
#pragma unroll
            for (int q = 0; q < VW / 4; ++q) {
                const f32x4 o = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
                *reinterpret_cast<f32x4*>(drow + j0 + 4 * q) = o;
            }
        }
    } else {
        for (int j = tid; j < C; j += 256) {
            const float t = SOFT ? sr.target(j, y, yb) : (j == y ? 1.f : 0.f);
            drow[j] = ok ? (expf(((float)row[j] - bm) - lsum) - t) * gscale : 0.f;
        }
    }
}

// One block: out3 = {mean loss, top-1 count, top-5 count}.  The loss rows are summed in INDEX order in double precision by one thread
// (the block stages 1024 rows at a time in LDS for it), so the value is the same on every run and equals a sequential host sum; the
// counts are integers, reduced by the whole block.
__global__ __launch_bounds__(256) void ce_finish_kernel(const float* __restrict__ loss_rows, const int* __restrict__ ranks,
                                                        float* __restrict__ out3, int B) {
    __shared__ float stage[1024];
    __shared__ int sh1[4], sh5[4];
    const int tid = threadIdx.x;
    int h1 = 0, h5 = 0;
    double acc = 0.0;
    for (int base = 0; base < B; base += 1024) {
        const int n = min(1024, B - base);
        for (int k = tid; k < n; k += 256) {
            stage[k] = loss_rows[base + k];
            const int r = ranks[base + k];
            h1 += r < 1 ? 1 : 0;
            h5 += r < 5 ? 1 : 0;
        }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < n; ++k) acc += (double)stage[k];
        __syncthreads();
    }
    h1 = wave_sum_int(h1);
    h5 = wave_sum_int(h5);
    if ((tid & 63) == 0) {
        sh1[tid >> 6] = h1;
        sh5[tid >> 6] = h5;
    }
    __syncthreads();
    if (tid == 0) {
        out3[0] = (float)(acc / (double)B);
        out3[1] = (float)((sh1[0] + sh1[1]) + (sh1[2] + sh1[3]));
        out3[2] = (float)((sh5[0] + sh5[1]) + (sh5[2] + sh5[3]));
    }
}

}  // namespace

#define STREAM ((hipStream_t)stream)

template <typename T, bool SOFT>
static int ce_rows_launch(const void* logits, const int64_t* labels, const int64_t* labels_b, const float* lam, float eps, float* loss_rows,
                          int32_t* ranks, float* dlogits, int64_t B, int64_t C, float gscale, int write_grad, hipStream_t s) {
    const bool vec = C % Chunk<T>::VW == 0 && ((uintptr_t)logits % 16) == 0 && (!write_grad || ((uintptr_t)dlogits % 16) == 0);
    const T* x = (const T*)logits;
    const long* y = (const long*)labels;
    const long* yb = (const long*)labels_b;
    if (C <= CE_WAVE_MAXC) {
        const dim3 grid((unsigned)((B + 3) / 4));
        if (vec) hipLaunchKernelGGL((ce_rows_wave_kernel<T, true, SOFT>), grid, dim3(256), 0, s, x, y, yb, lam, eps, loss_rows, ranks, dlogits, (int)B, (int)C, gscale, write_grad);
        else hipLaunchKernelGGL((ce_rows_wave_kernel<T, false, SOFT>), grid, dim3(256), 0, s, x, y, yb, lam, eps, loss_rows, ranks, dlogits, (int)B, (int)C, gscale, write_grad);
    } else {
        const dim3 grid((unsigned)B);
        if (vec) hipLaunchKernelGGL((ce_rows_block_kernel<T, true, SOFT>), grid, dim3(256), 0, s, x, y, yb, lam, eps, loss_rows, ranks, dlogits, (int)C, gscale, write_grad);
        else hipLaunchKernelGGL((ce_rows_block_kernel<T, false, SOFT>), grid, dim3(256), 0, s, x, y, yb, lam, eps, loss_rows, ranks, dlogits, (int)C, gscale, write_grad);
    }
    SS_LAUNCH_CHECK(SOFT ? "soft_ce_rows" : "ce_rows");
    return 0;
}

extern "C" int simseg_ce_rows(const void* logits, int dt, const int64_t* labels, float* loss_rows, int32_t* ranks, float* dlogits,
                              float* out3, int64_t B, int64_t C, float gscale, int write_grad, void* stream) {
    SS_CHECK(logits && labels && loss_rows && ranks && out3, "ce_rows: null pointer");
    SS_CHECK(!write_grad || dlogits, "ce_rows: write_grad needs dlogits");
    SS_CHECK(dt == 0 || dt == 1, "ce_rows: dt must be 0 (fp32) or 1 (the selected 16-bit type), got %d", dt);
    SS_CHECK(C >= 1 && C <= 65536, "ce_rows: need 1 <= C <= 65536 (got C=%lld)", (long long)C);
    SS_CHECK(B >= 1 && B < (1ll << 31), "ce_rows: need 1 <= B < 2^31 (got B=%lld)", (long long)B);
    SS_CHECK(((uintptr_t)logits % (dt == 0 ? 4 : 2)) == 0 && ((uintptr_t)labels % 8) == 0, "ce_rows: misaligned operand");
    int rc;
    if (dt == 0) rc = ce_rows_launch<float, false>(logits, labels, nullptr, nullptr, 0.f, loss_rows, ranks, dlogits, B, C, gscale, write_grad, STREAM);
    else if (g_ss_half == 2) rc = ce_rows_launch<_Float16, false>(logits, labels, nullptr, nullptr, 0.f, loss_rows, ranks, dlogits, B, C, gscale, write_grad, STREAM);
    else rc = ce_rows_launch<__bf16, false>(logits, labels, nullptr, nullptr, 0.f, loss_rows, ranks, dlogits, B, C, gscale, write_grad, STREAM);
    if (rc) return rc;
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, STREAM, loss_rows, ranks, out3, (int)B);
    SS_LAUNCH_CHECK("ce_rows");
    return 0;
}

extern "C" int simseg_soft_ce_rows(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam, float smoothing,
                                   float* loss_rows, int32_t* ranks, float* dlogits, float* out3, int64_t B, int64_t C, float gscale,
                                   int write_grad, void* stream) {
    SS_CHECK(logits && labels_a && labels_b && lam && loss_rows && ranks && out3, "soft_ce_rows: null pointer");
    SS_CHECK(!write_grad || dlogits, "soft_ce_rows: write_grad needs dlogits");
    SS_CHECK(dt == 0 || dt == 1, "soft_ce_rows: dt must be 0 (fp32) or 1 (the selected 16-bit type), got %d", dt);
    SS_CHECK(C >= 1 && C <= 65536, "soft_ce_rows: need 1 <= C <= 65536 (got C=%lld)", (long long)C);
    SS_CHECK(B >= 1 && B < (1ll << 31), "soft_ce_rows: need 1 <= B < 2^31 (got B=%lld)", (long long)B);
    SS_CHECK(smoothing >= 0.f && smoothing < 1.f, "soft_ce_rows: smoothing %g is outside [0, 1) (or nan)", (double)smoothing);
    SS_CHECK(((uintptr_t)logits % (dt == 0 ? 4 : 2)) == 0 && ((uintptr_t)labels_a % 8) == 0 && ((uintptr_t)labels_b % 8) == 0 && ((uintptr_t)lam % 4) == 0,
             "soft_ce_rows: misaligned operand");
    int rc;
    if (dt == 0) rc = ce_rows_launch<float, true>(logits, labels_a, labels_b, lam, smoothing, loss_rows, ranks, dlogits, B, C, gscale, write_grad, STREAM);
    else if (g_ss_half == 2) rc = ce_rows_launch<_Float16, true>(logits, labels_a, labels_b, lam, smoothing, loss_rows, ranks, dlogits, B, C, gscale, write_grad, STREAM);
    else rc = ce_rows_launch<__bf16, true>(logits, labels_a, labels_b, lam, smoothing, loss_rows, ranks, dlogits, B, C, gscale, write_grad, STREAM);
    if (rc) return rc;
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, STREAM, loss_rows, ranks, out3, (int)B);
    SS_LAUNCH_CHECK("soft_ce_rows");
    return 0;
}
