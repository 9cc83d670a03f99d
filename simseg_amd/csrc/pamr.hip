// PAMR - pixel-adaptive mask refinement (Araslanov & Roth, "Single-stage semantic segmentation from image labels", CVPR 2020) - as the
// device alternative to the DenseCRF of crf.hip: a fixed number of local, affinity-weighted averaging steps over dilated 3x3
// neighbourhoods.  No lattice, no hash table, no host read, no atomics and no dependence between blocks: the whole call is a fixed
// sequence of launches and replays in a captured graph.
//
//   taps       t = (dilation j, offset i), dilation-major; offsets (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1)
//   neighbour  q_t(p) = (clamp(y + d_j * oy_i, 0, H-1), clamp(x + d_j * ox_i, 0, W-1))                         (replicate padding)
//   sigma_c(p) = unbiased std over the n = 9 D samples of the D dilated 3x3 neighbourhoods (centre included each time); the sums over
//                bytes are exact 32-bit integers: sigma^2 = (n Sum x^2 - (Sum x)^2) / (n (n - 1))
//   logit      l_t(p) = -(1/3) Sum_c |rgb_c(p) - rgb_c(q_t)| / (1e-8 + 0.1 sigma_c(p));   w_t(p) = softmax_t l_t(p)
//   step       m_k(p) <- Sum_t w_t(p) m_k(q_t(p)),   iters times;   mask_k(p) = 255 if m_k(p) > 0.5 else 0
//
// pamr_affinity_kernel: one thread per pixel, weights stored plane-major [B][8D][H][W] fp32 (a wave's 64 pixels of a row = 256
// contiguous bytes per tap).  The bytes of an image are gathered straight from global memory: a 512^2 image is 768 KB and stays in
// the XCD's L2; an LDS stage for the 24-pixel halo (80x80x3 bytes per 32x32 tile) would serve 6.25 bytes per pixel to save reads
// that already hit a cache, and this kernel runs once per `iters` propagation steps.
// pamr_propagate_kernel: one thread per pixel; each weight is loaded once and applied to every visited slot of the image (the slot
// list is uniform per block: block z = image), neighbours gathered with clamped coordinates, sequential fused multiply-adds in tap
// order - so a pixel's result depends on its own image only, never on the batch position or the chunking.
#include <algorithm>

#include "common.h"

namespace {

constexpr int PAMR_MAXD = 8;       // dilations per call
constexpr int PAMR_MAXK = 8;       // candidate maps per image
constexpr int PAMR_BX = 64, PAMR_BY = 4;
constexpr int64_t PAMR_GROUP_BYTES = 160ll << 20;       // weights of the images that go through the iterations together (simseg_pamr)

struct PamrDil {
    int n;
    int d[PAMR_MAXD];
};

__device__ __forceinline__ int pamr_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// bit k set = slot k of image b is visited (cand == nullptr: all K are)
__device__ __forceinline__ unsigned pamr_visited(const int* __restrict__ cand, int b, int K) {
    unsigned vm = 0;
    for (int k = 0; k < K; ++k)
        if (!cand || cand[(size_t)b * K + k] >= 0) vm |= 1u << k;
    return vm;
}

// offsets 0..7 -> index (0 = minus, 1 = centre, 2 = plus) into the three clamped rows / columns of a dilation
__device__ __forceinline__ constexpr int pamr_oy(int o) { return o < 3 ? 0 : (o < 5 ? 1 : 2); }
__device__ __forceinline__ constexpr int pamr_ox(int o) { return o < 3 ? o : (o == 3 ? 0 : (o == 4 ? 2 : o - 5)); }

__global__ __launch_bounds__(PAMR_BX * PAMR_BY) void pamr_affinity_kernel(const uint8_t* __restrict__ rgb, const int* __restrict__ cand,
                                                                        float* __restrict__ wgt, int K, int H, int W, PamrDil dil) {
    const int b = blockIdx.z;
    if (!pamr_visited(cand, b, K)) return;                 // an image none of whose slots is visited
    const int x = blockIdx.x * PAMR_BX + threadIdx.x, y = blockIdx.y * PAMR_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t HW = (size_t)H * W;
    const uint8_t* __restrict__ im = rgb + (size_t)b * HW * 3;
    const int p = y * W + x;
    const int c0 = im[3 * (size_t)p], c1 = im[3 * (size_t)p + 1], c2 = im[3 * (size_t)p + 2];
    int s0 = 0, s1 = 0, s2 = 0, q0 = 0, q1 = 0, q2 = 0;
    unsigned ad[8 * PAMR_MAXD];                            // |centre - neighbour| of the three channels, one byte each
#pragma unroll
    for (int j = 0; j < PAMR_MAXD; ++j) {
        if (j < dil.n) {
            const int d = dil.d[j];
            const int ry[3] = {pamr_clamp(y - d, H - 1) * W, y * W, pamr_clamp(y + d, H - 1) * W};
            const int cx[3] = {pamr_clamp(x - d, W - 1), x, pamr_clamp(x + d, W - 1)};
            s0 += c0; s1 += c1; s2 += c2;                  // the centre is a sample of every dilation
            q0 += c0 * c0; q1 += c1 * c1; q2 += c2 * c2;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const uint8_t* __restrict__ q = im + 3 * (size_t)(ry[pamr_oy(o)] + cx[pamr_ox(o)]);
                const int v0 = q[0], v1 = q[1], v2 = q[2];
                s0 += v0; s1 += v1; s2 += v2;
                q0 += v0 * v0; q1 += v1 * v1; q2 += v2 * v2;
                ad[j * 8 + o] = (unsigned)abs(v0 - c0) | ((unsigned)abs(v1 - c1) << 8) | ((unsigned)abs(v2 - c2) << 16);
            }
        }
    }
    const int n = 9 * dil.n;                               // n Sum x^2 <= 72 * 72 * 255^2 = 3.4e8: exact in 32 bits
    const float den = (float)(n * (n - 1));
    const float i0 = 1.0f / (1e-8f + 0.1f * sqrtf((float)(n * q0 - s0 * s0) / den));
    const float i1 = 1.0f / (1e-8f + 0.1f * sqrtf((float)(n * q1 - s1 * s1) / den));
    const float i2 = 1.0f / (1e-8f + 0.1f * sqrtf((float)(n * q2 - s2 * s2) / den));
    float l[8 * PAMR_MAXD];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < PAMR_MAXD; ++j) {
        if (j < dil.n) {
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const unsigned a = ad[j * 8 + o];
                const float t = (float)(a & 255u) * i0 + (float)((a >> 8) & 255u) * i1 + (float)(a >> 16) * i2;
                l[j * 8 + o] = t * (-1.0f / 3.0f);
                mx = fmaxf(mx, l[j * 8 + o]);
            }
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < PAMR_MAXD; ++j) {
        if (j < dil.n) {
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                l[j * 8 + o] = __expf(l[j * 8 + o] - mx);
                sum += l[j * 8 + o];
            }
        }
    }
    const float inv = 1.0f / sum;
    float* __restrict__ wp = wgt + (size_t)b * 8 * dil.n * HW + p;
#pragma unroll
    for (int j = 0; j < PAMR_MAXD; ++j) {
        if (j < dil.n) {
#pragma unroll
            for (int o = 0; o < 8; ++o) wp[(size_t)(j * 8 + o) * HW] = l[j * 8 + o] * inv;
        }
    }
}

// One propagation step of pixel (y, x) for the NS visited slots ko[0..NS) of its image.  src planes are [sh, sw] = [H, W] / scale:
// SCALED reads them through (y / scale, x / scale) - the nearest upsampling of the low-resolution maps, never materialised.
template <int NS, bool SCALED>
__device__ __forceinline__ void pamr_pixel(const float* __restrict__ wp, const float* __restrict__ src, float* __restrict__ dst,
                                           uint8_t* __restrict__ mask, const int (&ko)[PAMR_MAXK], size_t plane0, int x, int y, int H, int W,
                                           int scale, const PamrDil& dil) {
    const size_t HW = (size_t)H * W;
    const int sw = SCALED ? W / scale : W;
    const size_t sHW = SCALED ? (size_t)(H / scale) * sw : HW;
    const float* __restrict__ sp[NS];
    float acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        sp[s] = src + (plane0 + ko[s]) * sHW;
        acc[s] = 0.f;
    }
    for (int j = 0; j < dil.n; ++j) {
        const int d = dil.d[j];
        int ry[3] = {pamr_clamp(y - d, H - 1), y, pamr_clamp(y + d, H - 1)};
        int cx[3] = {pamr_clamp(x - d, W - 1), x, pamr_clamp(x + d, W - 1)};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (SCALED) {
                ry[i] /= scale;
                cx[i] /= scale;
            }
            ry[i] *= sw;
        }
        const float* __restrict__ wj = wp + (size_t)j * 8 * HW;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const float w = wj[(size_t)o * HW];
            const int q = ry[pamr_oy(o)] + cx[pamr_ox(o)];
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] = fmaf(w, sp[s][q], acc[s]);
        }
    }
    const int p = y * W + x;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const size_t at = (plane0 + ko[s]) * HW + p;
        if (dst) dst[at] = acc[s];
        if (mask) mask[at] = acc[s] > 0.5f ? 255 : 0;
    }
}

template <bool SCALED>
__global__ __launch_bounds__(PAMR_BX * PAMR_BY) void pamr_propagate_kernel(const float* __restrict__ wgt, const float* __restrict__ src,
                                                                         float* __restrict__ dst, uint8_t* __restrict__ mask,
                                                                         const int* __restrict__ cand, int K, int H, int W, int scale, PamrDil dil) {
    const int b = blockIdx.z;
    const unsigned vm = pamr_visited(cand, b, K);
    if (!vm) return;
    // the visited slots, in slot order (uniform per block; static indices only, so the list stays in registers)
    int ko[PAMR_MAXK] = {0, 0, 0, 0, 0, 0, 0, 0};
    int nvis = 0;
#pragma unroll
    for (int k = 0; k < PAMR_MAXK; ++k) {
        const bool v = (vm >> k) & 1u;
#pragma unroll
        for (int s = 0; s < PAMR_MAXK; ++s)
            if (v && nvis == s) ko[s] = k;
        nvis += v;
    }
    const int x = blockIdx.x * PAMR_BX + threadIdx.x, y = blockIdx.y * PAMR_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t HW = (size_t)H * W;
    const float* __restrict__ wp = wgt + (size_t)b * 8 * dil.n * HW + (y * W + x);
    const size_t plane0 = (size_t)b * K;
    switch (nvis) {
    case 1: pamr_pixel<1, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    case 2: pamr_pixel<2, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    case 3: pamr_pixel<3, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    case 4: pamr_pixel<4, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    case 5: pamr_pixel<5, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    case 6: pamr_pixel<6, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    case 7: pamr_pixel<7, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    default: pamr_pixel<8, SCALED>(wp, src, dst, mask, ko, plane0, x, y, H, W, scale, dil); break;
    }
}

// iters = 0: the unary decision prob > 0.5 (and the upsampled map itself) for every visited slot
__global__ __launch_bounds__(PAMR_BX * PAMR_BY) void pamr_unary_kernel(const float* __restrict__ prob, float* __restrict__ m_out,
                                                                     uint8_t* __restrict__ mask, const int* __restrict__ cand, int K, int H, int W,
                                                                     int scale) {
    const int b = blockIdx.z;
    const unsigned vm = pamr_visited(cand, b, K);
    const int x = blockIdx.x * PAMR_BX + threadIdx.x, y = blockIdx.y * PAMR_BY + threadIdx.y;
    if (!vm || x >= W || y >= H) return;
    const size_t HW = (size_t)H * W;
    const int sw = W / scale;
    const size_t sHW = (size_t)(H / scale) * sw;
    const int q = (y / scale) * sw + x / scale, p = y * W + x;
    for (int k = 0; k < K; ++k) {
        if (!((vm >> k) & 1u)) continue;
        const float v = prob[((size_t)b * K + k) * sHW + q];
        const size_t at = ((size_t)b * K + k) * HW + p;
        if (m_out) m_out[at] = v;
        mask[at] = v > 0.5f ? 255 : 0;
    }
}

}  // namespace

extern "C" int64_t simseg_pamr_workspace_bytes(int64_t B, int64_t K, int64_t H, int64_t W, int n_dil) {
    if (B <= 0 || K <= 0 || K > PAMR_MAXK || H <= 0 || W <= 0 || n_dil < 1 || n_dil > PAMR_MAXD) return -1;
    return (int64_t)sizeof(float) * B * H * W * (8 * (int64_t)n_dil + 2 * K);       // the weights [B][8D][H][W] + two map buffers [B][K][H][W]
}

extern "C" int simseg_pamr(const uint8_t* rgb, const float* prob, const int* cand_idx, uint8_t* mask, float* m_out, int64_t B, int64_t K,
                           int64_t H, int64_t W, const int* dilations, int n_dil, int iters, int64_t scale, void* ws, int64_t ws_bytes,
                           void* stream) {
    SS_CHECK(rgb && prob && mask && dilations, "pamr: null pointer");
    SS_CHECK(B >= 1 && B < (1 << 14), "pamr: 1..16383 images per call (got %lld)", (long long)B);
    SS_CHECK(H > 0 && W > 0 && H <= (1 << 14) && W <= (1 << 14) && H * W <= (1ll << 26) && B * K * H * W < (1ll << 40),
             "pamr: batch of %lld images of %lld x %lld pixels is out of range", (long long)B, (long long)H, (long long)W);
    SS_CHECK(K >= 1 && K <= PAMR_MAXK, "pamr: 1..%d candidate maps per image (got %lld)", PAMR_MAXK, (long long)K);
    SS_CHECK(n_dil >= 1 && n_dil <= PAMR_MAXD, "pamr: 1..%d dilations (got %d)", PAMR_MAXD, n_dil);
    PamrDil dil;
    dil.n = n_dil;
    for (int j = 0; j < PAMR_MAXD; ++j) {
        dil.d[j] = j < n_dil ? dilations[j] : 1;
        SS_CHECK(dil.d[j] >= 1 && dil.d[j] <= 64, "pamr: dilations are 1..64 pixels (got %d)", dil.d[j]);
    }
    SS_CHECK(iters >= 0 && iters <= 64, "pamr: 0..64 iterations (got %d)", iters);
    SS_CHECK(scale >= 1 && H % scale == 0 && W % scale == 0, "pamr: %lld x %lld pixels are no multiple of the map scale %lld", (long long)H,
             (long long)W, (long long)scale);
    const int64_t need = iters ? simseg_pamr_workspace_bytes(B, K, H, W, n_dil) : 0;
    SS_CHECK(ws_bytes >= need && (need == 0 || ws), "pamr: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)need);
    SS_CHECK(((uintptr_t)ws % 16) == 0, "pamr: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t maps = (size_t)B * K * H * W;
    const int Ki = (int)K, Hi = (int)H, Wi = (int)W, sc = (int)scale;
    // slots the reference never visits (and whole images without a visited slot) are not computed: their outputs are the zeros set here
    (void)hipMemsetAsync(mask, 0, maps, s);
    if (m_out) (void)hipMemsetAsync(m_out, 0, maps * sizeof(float), s);
    const dim3 block(PAMR_BX, PAMR_BY);
    const unsigned gx = (unsigned)((W + PAMR_BX - 1) / PAMR_BX), gy = (unsigned)((H + PAMR_BY - 1) / PAMR_BY);
    if (iters == 0) {
        hipLaunchKernelGGL(pamr_unary_kernel, dim3(gx, gy, (unsigned)B), block, 0, s, prob, m_out, mask, cand_idx, Ki, Hi, Wi, sc);
        SS_LAUNCH_CHECK("pamr");
        return 0;
    }
    // Every iteration re-reads the weights of its images (50 MB per 512^2 image at the defaults), so the batch goes through `group`
    // images at a time, all iterations of a group before the next: a group's weights (<= PAMR_GROUP_BYTES) plus the maps it moves per
    // step stay in the 256 MiB Infinity Cache between two steps instead of streaming from HBM ten times.  Images are independent: the
    // grouping changes no result.
    const size_t HW = (size_t)H * W, wimg = (size_t)8 * n_dil * HW, sHW = HW / (size_t)(scale * scale);
    const int64_t group = std::max<int64_t>(1, PAMR_GROUP_BYTES / (int64_t)(wimg * sizeof(float)));
    float* wgt = static_cast<float*>(ws);
    float* buf[2] = {wgt + (size_t)B * wimg, wgt + (size_t)B * wimg + maps};
    for (int64_t b0 = 0; b0 < B; b0 += group) {
        const dim3 grid(gx, gy, (unsigned)std::min<int64_t>(group, B - b0));
        const size_t m0 = (size_t)b0 * K * HW;                         // first map of the group in the full-resolution buffers
        const int* cg = cand_idx ? cand_idx + b0 * K : nullptr;
        float* wg = wgt + (size_t)b0 * wimg;
        hipLaunchKernelGGL(pamr_affinity_kernel, grid, block, 0, s, rgb + (size_t)b0 * HW * 3, cg, wg, Ki, Hi, Wi, dil);
        for (int it = 0; it < iters; ++it) {
            const bool last = it + 1 == iters;
            float* dst = last ? (m_out ? m_out + m0 : nullptr) : buf[it & 1] + m0;
            uint8_t* mk = last ? mask + m0 : nullptr;
            if (it == 0 && scale > 1)
                hipLaunchKernelGGL(pamr_propagate_kernel<true>, grid, block, 0, s, wg, prob + (size_t)b0 * K * sHW, dst, mk, cg, Ki, Hi, Wi, sc, dil);
            else
                hipLaunchKernelGGL(pamr_propagate_kernel<false>, grid, block, 0, s, wg, it == 0 ? prob + m0 : buf[(it - 1) & 1] + m0, dst, mk, cg, Ki,
                                   Hi, Wi, 1, dil);
        }
    }
    SS_LAUNCH_CHECK("pamr");
    return 0;
}
