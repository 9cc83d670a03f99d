// Shared device/host helpers for libsimseg_hip.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

// The 16-bit operand type is __bf16 (the headline mode) or _Float16 (the IEEE fp16 the reference's AMP mode uses: fp16 autocast + a live
// GradScaler, clip_runner.py:226-230).  Every source is compiled ONCE.  A kernel or device helper that touches 16-bit data takes the type
// as its leading template argument `H`; an entry point picks it per call from g_ss_half - what the calling thread selected with
// simseg_set_half_type - through with_h16 below, and dtype code 1 always means "the selected 16-bit type".  Host state (selectors, trace
// pointers, last-variant values) exists once per thread; fp32 kernels have one instantiation whatever the thread selected.
extern thread_local int g_ss_half;          // 1 = bf16 (default), 2 = fp16: simseg_set_half_type
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define WAVE 64

// ---- error plumbing (no exceptions cross the C ABI) -------------------------------------------
extern thread_local char g_simseg_err[512];
int simseg_set_error(const char* fmt, ...);

#define SS_CHECK(cond, ...)                          \
    do {                                             \
        if (!(cond)) return simseg_set_error(__VA_ARGS__); \
    } while (0)

#define SS_LAUNCH_CHECK(name)                                                         \
    do {                                                                              \
        hipError_t e__ = hipGetLastError();                                           \
        if (e__ != hipSuccess) return simseg_set_error("%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

// ---- numeric helpers --------------------------------------------------------------------------
// Element type of a buffer where a call states it outright instead of through dtype code 1: the values g_ss_half takes, and 0 for fp32.
enum { SS_ELEM_F32 = 0, SS_ELEM_BF16 = 1, SS_ELEM_FP16 = 2 };
template <typename H> struct h16_tag { typedef H type; };
// f(h16_tag<H>()) for the 16-bit type `half` names (g_ss_half at an entry point): `[&](auto tag) { typedef typename decltype(tag)::type H; ... }`;
// returns what f returns (an entry point's int status, or nothing)
template <typename F> inline auto with_h16(int half, F&& f) {
    if (half == SS_ELEM_FP16) return f(h16_tag<_Float16>());
    return f(h16_tag<__bf16>());
}
template <typename H> using h16x4 = H __attribute__((ext_vector_type(4)));
template <typename H> using h16x8 = H __attribute__((ext_vector_type(8)));

// acc + a . b on the 32x32x16 MFMA of the operands' type: v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16
__device__ __forceinline__ f32x16 mfma_32x32x16(h16x8<__bf16> a, h16x8<__bf16> b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_32x32x16(h16x8<_Float16> a, h16x8<_Float16> b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
}

// 16 bytes (fp32) / 8 bytes (16-bit) of a row to and from four floats: the row kernels' unit of access (rowops.hip, patchdrop.hip)
template <typename TO> __device__ __forceinline__ void store4(TO* p, const float (&v)[4]);
template <> __device__ __forceinline__ void store4<float>(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <typename H> __device__ __forceinline__ void store4_h16(H* p, const float (&v)[4]) {
    h16x4<H> o = {(H)v[0], (H)v[1], (H)v[2], (H)v[3]};
    *reinterpret_cast<h16x4<H>*>(p) = o;
}
template <> __device__ __forceinline__ void store4<__bf16>(__bf16* p, const float (&v)[4]) { store4_h16(p, v); }
template <> __device__ __forceinline__ void store4<_Float16>(_Float16* p, const float (&v)[4]) { store4_h16(p, v); }
template <typename TI> __device__ __forceinline__ void load4(const TI* p, float (&v)[4]);
template <> __device__ __forceinline__ void load4<float>(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <typename H> __device__ __forceinline__ void load4_h16(const H* p, float (&v)[4]) {
    const h16x4<H> t = *reinterpret_cast<const h16x4<H>*>(p);
    v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
}
template <> __device__ __forceinline__ void load4<__bf16>(const __bf16* p, float (&v)[4]) { load4_h16(p, v); }
template <> __device__ __forceinline__ void load4<_Float16>(const _Float16* p, float (&v)[4]) { load4_h16(p, v); }

// out[n] += sum_r in[r, n] over a [rows, N] block with row stride ld, `elem` one of SS_ELEM_*: the body of simseg_colsum_accum
// (rowops.hip), for callers inside the library that know their operand's type - attn.hip folds the qkv bias gradient with it.
int ss_colsum_accum(const void* in, int elem, float* out, int64_t rows, int64_t N, int64_t ld, void* stream);

// Normal CDF for the erf-GELU epilogues.  libm's erff costs ~30 VALU instructions per element, which made the GELU / GELU'
// epilogues of the MLP GEMMs as long as their K loops (measured: +40 % / +60 % on [100864,768]x[3072,768]^T).  Abramowitz &
// Stegun 7.1.26 needs one exp, one reciprocal and five FMAs, and its exp(-x^2/2) is the Gaussian the derivative needs anyway:
//   erf(z) = 1 - (a1 t + ... + a5 t^5) e^{-z^2},  t = 1 / (1 + p z),  z >= 0,   |error| <= 1.5e-7
// The lower tail is formed as 0.5 * poly * e directly (no 1 - 1 cancellation).  `gauss` returns exp(-x^2/2).
__device__ __forceinline__ float norm_cdf(float x, float& gauss) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
    gauss = __expf(-z * z);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float tail = 0.5f * poly * gauss;               // = 0.5 * erfc(|x| / sqrt 2)
    return x >= 0.f ? 1.0f - tail : tail;
}
__device__ __forceinline__ float gelu_erf(float x) {
    float g;
    return x * norm_cdf(x, g);
}
// y = gelu(x) and dy = gelu'(x) from one CDF / Gaussian evaluation (forward epilogue that stores the derivative for backward)
__device__ __forceinline__ float gelu_erf_grad(float x, float& dy) {
    float g;
    const float cdf = norm_cdf(x, g);
    dy = cdf + x * 0.39894228040143268f * g;
    return x * cdf;
}
// bf16 epilogues only: erf-GELU and its derivative from an odd degree-15 polynomial fit of the normal CDF on |x| <= 3.5 (argument
// clamped beyond: the CDF is then within 2.4e-4 of 0 / 1), no transcendental instruction.  v_exp / v_rcp issue at a quarter of the FMA
// rate, and the fc1-forward epilogue (GELU + GELU' of 64 K values per tile) was bound by exactly that arithmetic: 66 -> ~40 issue cycles
// per element.  Fit error (fp32 Horner): CDF 7e-6, GELU 1.3e-5, GELU' 4.4e-4 - below bf16's 4e-3 relative rounding of the stored values.
// The exact-fp32 path keeps norm_cdf above.
__device__ __forceinline__ float gelu_poly_grad(float x, float& dy) {
    const float xc = __builtin_amdgcn_fmed3f(x, -3.5f, 3.5f);
    const float s = xc * xc;
    float q = -2.815794181e-09f, dq = -4.223691272e-08f;
    q = fmaf(q, s, 1.818798183e-07f);   dq = fmaf(dq, s, 2.364437638e-06f);
    q = fmaf(q, s, -5.270657400e-06f);  dq = fmaf(dq, s, -5.797723140e-05f);
    q = fmaf(q, s, 9.220430572e-05f);   dq = fmaf(dq, s, 8.298387515e-04f);
    q = fmaf(q, s, -1.108776002e-03f);  dq = fmaf(dq, s, -7.761432013e-03f);
    q = fmaf(q, s, 9.826695057e-03f);   dq = fmaf(dq, s, 4.913347528e-02f);
    q = fmaf(q, s, -6.636358108e-02f);  dq = fmaf(dq, s, -1.990907432e-01f);
    q = fmaf(q, s, 3.989096663e-01f);   dq = fmaf(dq, s, 3.989096663e-01f);
    const float cdf = fmaf(xc, q, 0.5f);
    dy = fmaf(xc, dq, cdf);
    return x * cdf;
}
__device__ __forceinline__ float gelu_poly(float x) {
    const float xc = __builtin_amdgcn_fmed3f(x, -3.5f, 3.5f);
    const float s = xc * xc;
    float q = -2.815794181e-09f;
    q = fmaf(q, s, 1.818798183e-07f);
    q = fmaf(q, s, -5.270657400e-06f);
    q = fmaf(q, s, 9.220430572e-05f);
    q = fmaf(q, s, -1.108776002e-03f);
    q = fmaf(q, s, 9.826695057e-03f);
    q = fmaf(q, s, -6.636358108e-02f);
    q = fmaf(q, s, 3.989096663e-01f);
    return x * fmaf(xc, q, 0.5f);
}
// The same two polynomials on PAIRS of elements (round 4): gfx950's v_pk_fma_f32 / v_pk_mul_f32 do two fp32 operations per lane in the issue
// slot of one, the constants ride along as scalar operands broadcast to both halves.  Same operations in the same order per element -
// bit-identical to the scalar forms above - at 21 instead of 38 VALU instructions per pair (alpha * acc + bias included): the fc1-forward
// epilogue computes GELU and GELU' of 128 values per lane and tile.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, float c) { return __builtin_elementwise_fma(a, b, (f32x2){c, c}); }
__device__ __forceinline__ f32x2 gelu_poly_grad2(f32x2 x, f32x2& dy) {
    const f32x2 xc = {__builtin_amdgcn_fmed3f(x.x, -3.5f, 3.5f), __builtin_amdgcn_fmed3f(x.y, -3.5f, 3.5f)};
    const f32x2 s = xc * xc;
    f32x2 q = {-2.815794181e-09f, -2.815794181e-09f}, dq = {-4.223691272e-08f, -4.223691272e-08f};
    q = pk_fma(q, s, 1.818798183e-07f);   dq = pk_fma(dq, s, 2.364437638e-06f);
    q = pk_fma(q, s, -5.270657400e-06f);  dq = pk_fma(dq, s, -5.797723140e-05f);
    q = pk_fma(q, s, 9.220430572e-05f);   dq = pk_fma(dq, s, 8.298387515e-04f);
    q = pk_fma(q, s, -1.108776002e-03f);  dq = pk_fma(dq, s, -7.761432013e-03f);
    q = pk_fma(q, s, 9.826695057e-03f);   dq = pk_fma(dq, s, 4.913347528e-02f);
    q = pk_fma(q, s, -6.636358108e-02f);  dq = pk_fma(dq, s, -1.990907432e-01f);
    q = pk_fma(q, s, 3.989096663e-01f);   dq = pk_fma(dq, s, 3.989096663e-01f);
    const f32x2 cdf = pk_fma(xc, q, 0.5f);
    dy = __builtin_elementwise_fma(xc, dq, cdf);
    return x * cdf;
}
__device__ __forceinline__ f32x2 gelu_poly2(f32x2 x) {
    const f32x2 xc = {__builtin_amdgcn_fmed3f(x.x, -3.5f, 3.5f), __builtin_amdgcn_fmed3f(x.y, -3.5f, 3.5f)};
    const f32x2 s = xc * xc;
    f32x2 q = {-2.815794181e-09f, -2.815794181e-09f};
    q = pk_fma(q, s, 1.818798183e-07f);
    q = pk_fma(q, s, -5.270657400e-06f);
    q = pk_fma(q, s, 9.220430572e-05f);
    q = pk_fma(q, s, -1.108776002e-03f);
    q = pk_fma(q, s, 9.826695057e-03f);
    q = pk_fma(q, s, -6.636358108e-02f);
    q = pk_fma(q, s, 3.989096663e-01f);
    return x * pk_fma(xc, q, 0.5f);
}
__device__ __forceinline__ float dgelu_erf(float x) {
    float g;
    const float cdf = norm_cdf(x, g);
    return cdf + x * 0.39894228040143268f * g;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Full-wave sum through the DPP network (no LDS crossbar, no index registers): quad butterflies, half-row / row mirrors, then the two
// row broadcasts that gfx9-family DPP offers; the total arrives in lane 63 and is returned as a wave-uniform (scalar) value.
// All 64 lanes must be active.
__device__ __forceinline__ float wave_sum_uniform(float v) {
#define SS_DPP_ADD(ctrl, rmask) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xf, true))
    SS_DPP_ADD(0xB1, 0xf);      // quad_perm [1,0,3,2]
    SS_DPP_ADD(0x4E, 0xf);      // quad_perm [2,3,0,1]
    SS_DPP_ADD(0x141, 0xf);     // row_half_mirror
    SS_DPP_ADD(0x140, 0xf);     // row_mirror
    SS_DPP_ADD(0x142, 0xa);     // row_bcast15 -> rows 1, 3
    SS_DPP_ADD(0x143, 0xc);     // row_bcast31 -> rows 2, 3
#undef SS_DPP_ADD
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
// Sum over the block (any whole number of waves), through sh[blockDim.x / 64]; every thread gets the total.
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += sh[i];
    return s;
}

// Blocks of `block` threads for n items, at least one and at most `cap` (the grid-stride kernels' launch size).
inline int grid_for(long n, int block, int cap = 4096) {
    long g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// counter-based RNG for dropout: one 32-bit hash per element index, reproducible in backward.  32-bit arithmetic only (the
// 64-bit splitmix used first cost ~35 VALU instructions per element - more than the GELU it sat next to): the index and
// seed halves are folded with odd multipliers, then the two-round "lowbias32" finaliser (bias < 0.11 bits / output bit).
__device__ __forceinline__ uint32_t hash_u32(uint64_t seed, uint64_t idx) {
    uint32_t x = (uint32_t)idx * 0x9E3779B1u + (uint32_t)(idx >> 32) * 0x85EBCA77u + (uint32_t)seed + (uint32_t)(seed >> 32) * 0xC2B2AE3Du;
    x ^= x >> 16; x *= 0x21F0AAADu;
    x ^= x >> 15; x *= 0x735A2D97u;
    x ^= x >> 15;
    return x;
}
// the same hash for an index known to fit 32 bits, with the seed folded once per kernel (seed_fold): one multiply-add
// plus the finaliser per element and no 64-bit temporaries (the attention backward kernels have no registers to spare)
__device__ __forceinline__ uint32_t seed_fold(uint64_t seed) { return (uint32_t)seed + (uint32_t)(seed >> 32) * 0xC2B2AE3Du; }
__device__ __forceinline__ bool dropout_keep32(uint32_t seedf, uint32_t idx, uint32_t thresh) {
    uint32_t x = idx * 0x9E3779B1u + seedf;
    x ^= x >> 16; x *= 0x21F0AAADu;
    x ^= x >> 15; x *= 0x735A2D97u;
    x ^= x >> 15;
    return x >= thresh;
}
// keep-probability test: keep iff hash >= p * 2^32
__device__ __forceinline__ bool dropout_keep(uint64_t seed, uint64_t idx, uint32_t thresh) {
    return hash_u32(seed, idx) >= thresh;
}

// XCD-aware, bijective block remap: XCD x (= bid % 8, observed dispatch) gets a contiguous chunk of tiles
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7, j = bid >> 3;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + j;
}
