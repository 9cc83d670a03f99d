// Training augmentation on the device: decoded uint8 [H, W, 3] images -> RandomResizedCrop (Pillow's bilinear uint8 resize of a crop
// box) -> up to two AutoAugment ops -> normalised fp32 [3, S, S], bit-identical to the same parameters applied with Pillow
// (simseg_amd/augment.py apply_pil).  TWO launches per batch, whatever its size and whichever ops were drawn.  DESIGN.md "Device-side
// training augmentation" states every op's arithmetic.
//
// Launch 1 (augment_resize_kernel): resample.h's pp_resample_tile, one 256-thread workgroup per output tile, on the crop box of the source
// image (a source pointer at the box's origin and the image's row pitch), writing packed uint8 [S, S, 3] into a scratch slot per image
// (slots 16-byte aligned).
// Launch 2 (augment_ops_kernel): one workgroup of 1024 threads per image.  With S <= AG_LDS_MAX_S the image is copied into LDS (150,528
// bytes at S = 224) and every op works there; larger images are worked on in their scratch slot, with a second slot as the target of the
// geometric ops.  Point ops (posterize, solarize, invert, autocontrast, equalize) build a per-channel [3, 256] byte table (the last two
// from per-channel histograms) and map every byte; colour and contrast blend each pixel with its degenerate value; sharpness, rotate and
// shearX read neighbours or other pixels, so each thread first writes all its results to global memory (the image's own scratch slot
// once the image is in LDS), the workgroup waits at a barrier, and the results are copied back.  The normalised output goes through the
// host-filled [3, 256] fp32 table.
//
// simseg_train_transforms (DESIGN.md "Device-side training transforms") is the general chain on the same two kernels, instantiated for
// its wider table (WIDE = 1): launch 1 resamples the source box with either filter to RH x RW, keeps the S x S output window and mirrors its
// columns for a flip; launch 2 runs a chain of up to five ops (brightness added) and replaces the look-up value inside the image's erase
// boxes by the fill of the mode.  The WIDE = 0 instances are simseg_train_augment's, as they were.
//
// simseg_train_chain (DESIGN.md "SimCLR colour distortion and Gaussian blur") is the third layout (WIDE = 2): the same geometry and erase
// columns, twelve ops, and three more op codes: grayscale, the hue shift (Pillow's RGB -> HSV -> RGB round trip per pixel) and the Gaussian
// blur (Pillow's three box passes along the rows, then along the columns; one thread per (line, channel) runs a pass in place, the R + 1
// bytes behind its position kept in a 64-bit register, so every byte of a pass is read before it is overwritten).
//
// Exactness: the blends, the 3x3 smoothing, autocontrast's scale and the bicubic shear must round as Pillow's C code does, so floating-
// point contraction is off for this file (build.py compiles with -O3 and the default contraction, which would form FMAs).
#pragma clang fp contract(off)
#include <math.h>

#include "resample.h"

constexpr int AG_COLS = 30, AG_SLOTS = 8;
enum { AG_SRC = 0, AG_H, AG_W, AG_TOP, AG_LEFT, AG_CH, AG_CW, AG_HOFF, AG_HKS, AG_VOFF, AG_VKS, AG_RSV, AG_OP1, AG_OP2, AG_P1 };
enum { OP_NONE = 0, OP_POSTERIZE, OP_SOLARIZE, OP_INVERT, OP_AUTOCONTRAST, OP_EQUALIZE, OP_COLOR, OP_CONTRAST, OP_SHARPNESS, OP_ROTATE,
       OP_SHEARX, OP_COUNT, OP_BRIGHTNESS = OP_COUNT, OP_COUNT_WIDE };   // OP_COUNT: the AutoAugment set simseg_train_augment takes
// the wider table of simseg_train_transforms: columns 0 .. AG_VKS as above, then
constexpr int TT_COLS = 81, TT_MAX_OPS = 5, TT_MAX_ERASE = 4;
enum { TT_RH = 11, TT_RW, TT_WTOP, TT_WLEFT, TT_FLIP, TT_NOPS, TT_NERASE, TT_MODE, TT_SEED, TT_BOX = 20, TT_OP = 36, TT_P = 41 };
enum { ER_CONST = 0, ER_RAND, ER_PIXEL, ER_MODES };
// the table of simseg_train_chain: columns 0 .. 35 as TT's, then
constexpr int TC_COLS = 144, TC_MAX_OPS = 12, TC_P = 48;
enum { OP_GRAY = OP_COUNT_WIDE, OP_HUE, OP_BLUR, OP_COUNT_CHAIN };
constexpr int AG_BLUR_MAX_R = 7;                                    // R + 1 bytes of a line fit one 64-bit register
__host__ __device__ constexpr int ag_cols(int wide) { return wide == 2 ? TC_COLS : wide ? TT_COLS : AG_COLS; }
__host__ __device__ constexpr int ag_slot0(int wide) { return wide == 2 ? TC_P : wide ? TT_P : AG_P1; }
constexpr int AG_MIN_S = 32, AG_MAX_S = 384;
constexpr int AG_THREADS = 1024;
constexpr int AG_LDS_MAX_S = 230;                                   // 230 * 230 * 3 = 158,700 bytes + the static LDS below <= 160 KiB
constexpr uint32_t AG_FILL = 128u | (128u << 8) | (128u << 16);

__host__ __device__ inline int64_t ag_slot_bytes(int64_t S) { return (3 * S * S + 15) / 16 * 16; }
static inline bool ag_in_lds(int64_t S) { return S <= AG_LDS_MAX_S; }

// ---- launch 1: crop + resize -------------------------------------------------------------------------------------------------------------
template <int WIDE>
__global__ __launch_bounds__(256) void augment_resize_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ img_tab,
                                                             const int* __restrict__ tab, uint8_t* __restrict__ scratch, int S,
                                                             int tiles_per_image) {
    __shared__ uint32_t hbuf[PP_CR * PP_TW];
    const int b = blockIdx.x / tiles_per_image, tile = blockIdx.x % tiles_per_image;
    const int64_t* it = img_tab + (long)b * ag_cols(WIDE);
    const long pitch = it[AG_W];
    const int* __restrict__ hb = tab + it[AG_HOFF];               // bounds [RW, 2] inside the crop, then coefficients [RW, hks]
    const int* __restrict__ vb = tab + it[AG_VOFF];
    const int tiles_x = (S + PP_TW - 1) / PP_TW;
    const int x0 = (tile % tiles_x) * PP_TW, y0 = (tile / tiles_x) * PP_TH;
    uint8_t* __restrict__ dst = scratch + b * ag_slot_bytes(S);
    // WIDE: the S x S window of the RH x RW resized box; a flip writes column x of the window to column S - 1 - x
    const long RW = WIDE ? it[TT_RW] : S, RH = WIDE ? it[TT_RH] : S;
    const int wx = WIDE ? (int)it[TT_WLEFT] : 0, wy = WIDE ? (int)it[TT_WTOP] : 0;
    const int xs = WIDE && it[TT_FLIP] ? -1 : 1, xb = xs < 0 ? S - 1 - x0 : x0;
    pp_resample_tile(hbuf, src + it[AG_SRC] + (it[AG_TOP] * pitch + it[AG_LEFT]) * 3, pitch, hb, hb + 2 * RW, (int)it[AG_HKS], vb,
                     vb + 2 * RH, (int)it[AG_VKS], wx + x0, wy + y0, min(PP_TW, S - x0), min(PP_TH, S - y0),
                     [=](int yy, int lane, int c0, int c1, int c2) {
        uint8_t* q = dst + ((long)(y0 + yy) * S + xb + xs * lane) * 3;
        q[0] = (uint8_t)c0; q[1] = (uint8_t)c1; q[2] = (uint8_t)c2;
    });
}

// ---- launch 2: the ops ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ag_px(const uint8_t* buf, int p) {
    return (uint32_t)buf[3 * p] | ((uint32_t)buf[3 * p + 1] << 8) | ((uint32_t)buf[3 * p + 2] << 16);
}
__device__ __forceinline__ void ag_put(uint8_t* buf, int p, uint32_t v) {
    buf[3 * p] = (uint8_t)v; buf[3 * p + 1] = (uint8_t)(v >> 8); buf[3 * p + 2] = (uint8_t)(v >> 16);
}
// Image.blend(degenerate, image, f) on one byte: float32 deg + f * (im - deg), truncated, clamped
__device__ __forceinline__ uint32_t ag_blend(int deg, int im, float f) {
    const int v = (int)((float)deg + f * (float)(im - deg));
    return (uint32_t)min(max(v, 0), 255);
}
__device__ __forceinline__ int ag_luma(uint32_t v) {            // convert("L"): ITU-R 601-2 in 16-bit fixed point
    return (int)((19595u * (v & 255u) + 38470u * ((v >> 8) & 255u) + 7471u * ((v >> 16) & 255u) + 0x8000u) >> 16);
}
__device__ __forceinline__ double ag_cubic(double v1, double v2, double v3, double v4, double d) {   // Pillow's BICUBIC, a = -1
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}
__device__ __forceinline__ double ag_f64(int64_t bits) { return __longlong_as_double((long long)bits); }
__device__ __forceinline__ float ag_f32(int64_t bits) { return __int_as_float((int)bits); }

// One standard normal of the erase noise: the counter-based hash of common.h through Box-Muller (the index is stated in
// include/simseg_hip.h and restated in float64 by pipeline.erase_noise_ref).  u1 in (0, 1] and 2 u2 in [0, 2) are exact in fp32.
__device__ __forceinline__ float ag_normal(uint64_t seed, uint64_t i) {
    const float u1 = (float)((hash_u32(seed, 2 * i) >> 8) + 1u) * 0x1p-24f;
    const float u2x2 = (float)(hash_u32(seed, 2 * i + 1) >> 8) * 0x1p-23f;
    return sqrtf(-2.0f * logf(u1)) * cospif(u2x2);
}

// torchvision's adjust_hue on one pixel: Pillow's convert("HSV") (float32 quotients; h in float32 when red is the maximum, else formed in
// double; fmod(h / 6 + 1, 1) in double, h / 6 + 1 lying in [5/6, 11/6]), H + shift modulo 256, Pillow's convert("RGB") (all in double)
__device__ __forceinline__ uint32_t ag_hue(uint32_t v, int shift) {
    const int r = v & 255u, g = (v >> 8) & 255u, b = (v >> 16) & 255u;
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int H = 0, Sv = 0;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = cr / (float)mx;
        const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
        float h;
        if (r == mx) h = bc - gc;
        else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double t = (double)h / 6.0 + 1.0;
        const float hh = (float)(t >= 1.0 ? t - 1.0 : t);
        H = min(max((int)((double)hh * 255.0), 0), 255);
        Sv = min(max((int)((double)s * 255.0), 0), 255);
    }
    H = (H + shift) & 255;
    const uint32_t V = (uint32_t)mx;
    if (Sv == 0) return V | (V << 8) | (V << 16);
    const double fv = (double)mx, fs = (double)Sv / 255.0, h6 = (double)H * 6.0 / 255.0;
    const double fi = floor(h6), f = h6 - fi;
    const uint32_t p = (uint32_t)min((int)(fv * (1.0 - fs) + 0.5), 255);
    const uint32_t q = (uint32_t)min((int)(fv * (1.0 - fs * f) + 0.5), 255);
    const uint32_t t = (uint32_t)min((int)(fv * (1.0 - fs * (1.0 - f)) + 0.5), 255);
    switch ((int)fi % 6) {
        case 0: return V | (t << 8) | (p << 16);
        case 1: return q | (V << 8) | (p << 16);
        case 2: return p | (V << 8) | (t << 16);
        case 3: return p | (q << 8) | (V << 16);
        case 4: return t | (p << 8) | (V << 16);
        default: return V | (p << 8) | (q << 16);
    }
}

// One box pass of Pillow's Gaussian blur over a line of n bytes (q, stride st), in place, by one thread:
// out[x] = (ww * sum_{|d| <= R} in[x + d] + fw * (in[x - R - 1] + in[x + R + 1]) + 2^23) >> 24, indices clamped to the line; the sum
// slides.  Byte j of `hist` is in[x - 1 - j] as it was before the pass (in[0] left of the line), bytes at and right of x are still
// unwritten, so every input is read before it is overwritten.  R <= AG_BLUR_MAX_R; (2R + 1) ww + 2 fw <= 2^24, so uint32 holds it.
__device__ __forceinline__ void ag_box_line(uint8_t* q, int n, int st, int R, uint32_t ww, uint32_t fw) {
    const uint32_t first = q[0];
    uint64_t hist = (uint64_t)first * 0x0101010101010101ull;
    uint32_t W = (uint32_t)(R + 1) * first;
    for (int d = 1; d <= R; ++d) W += q[min(d, n - 1) * st];
    for (int x = 0; x < n; ++x) {
        const uint32_t cur = q[x * st];
        const uint32_t er = q[min(x + R + 1, n - 1) * st];
        const uint32_t el = (uint32_t)(hist >> (8 * R)) & 255u;
        q[x * st] = (uint8_t)((ww * W + fw * (el + er) + (1u << 23)) >> 24);
        hist = (hist << 8) | cur;
        W += er - ((uint32_t)(hist >> (8 * R)) & 255u);
    }
}

// Every pixel through f(p) -> packed RGB, all reads before any write: the results go to `alt` (global memory), the workgroup waits, and
// then the LDS path copies them back into LDS (16-byte pieces) while the global path makes `alt` the image.  (Keeping them in registers
// instead - 52 pixels per thread at S = 230 - spills the bicubic's working set at 1024 threads.)
template <bool LDS, class F>
__device__ __forceinline__ void ag_gather(uint8_t*& buf, uint8_t*& alt, int n, long slot, F f) {
    const int tid = threadIdx.x;
    for (int p = tid; p < n; p += AG_THREADS) ag_put(alt, p, f(p));
    __syncthreads();
    if constexpr (LDS) {
        const uint4* s4 = reinterpret_cast<const uint4*>(alt);
        uint4* d4 = reinterpret_cast<uint4*>(buf);
        for (int i = tid; i < (int)(slot / 16); i += AG_THREADS) d4[i] = s4[i];
    } else {
        uint8_t* t = buf; buf = alt; alt = t;
    }
}

template <bool LDS, int WIDE>
__global__ __launch_bounds__(AG_THREADS) void augment_ops_kernel(const int64_t* __restrict__ img_tab, uint8_t* __restrict__ scratch,
                                                                 uint8_t* __restrict__ scratch2, int S, const float* __restrict__ lut,
                                                                 float* __restrict__ out, uint8_t* __restrict__ out_u8) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ag_lds[];
    __shared__ int hist[3][256];
    __shared__ uint8_t tlut[3][256];
    __shared__ int lsum;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t* it = img_tab + (long)b * ag_cols(WIDE);
    const int n = S * S;
    const long slot = ag_slot_bytes(S);
    const int nops = WIDE ? (int)it[TT_NOPS] : 2;
    uint8_t* buf;
    uint8_t* alt = nullptr;
    if constexpr (LDS) {
        buf = ag_lds;
        alt = scratch + b * slot;                                // free once copied: the target of the geometric ops
        const uint4* s4 = reinterpret_cast<const uint4*>(scratch + b * slot);
        uint4* d4 = reinterpret_cast<uint4*>(ag_lds);
        for (int i = tid; i < (int)(slot / 16); i += AG_THREADS) d4[i] = s4[i];
    } else {
        buf = scratch + b * slot;
        alt = scratch2 + b * slot;
    }
    for (int k = 0; k < nops; ++k) {
        const int op = (int)it[(WIDE ? TT_OP : AG_OP1) + k];                  // (TT_OP in both wide layouts)
        const int64_t* P = it + ag_slot0(WIDE) + k * AG_SLOTS;
        __syncthreads();                                         // the image as the last step left it
        if (op == OP_NONE) continue;
        if (op <= OP_EQUALIZE) {
            // ---- byte -> byte tables per channel
            if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
                for (int i = tid; i < 768; i += AG_THREADS) (&hist[0][0])[i] = 0;
                __syncthreads();
                for (int p = tid; p < n; p += AG_THREADS) {
                    atomicAdd(&hist[0][buf[3 * p]], 1);
                    atomicAdd(&hist[1][buf[3 * p + 1]], 1);
                    atomicAdd(&hist[2][buf[3 * p + 2]], 1);
                }
                __syncthreads();
                if (tid < 3) {
                    const int c = tid;
                    bool ident = false;
                    if (op == OP_AUTOCONTRAST) {                 // ImageOps.autocontrast(cutoff = 0): scale and offset in double
                        int lo = 0, hi = 255;
                        while (lo < 255 && !hist[c][lo]) ++lo;
                        while (hi > 0 && !hist[c][hi]) --hi;
                        if (hi <= lo) {
                            ident = true;
                        } else {
                            const double scale = 255.0 / (double)(hi - lo);
                            const double offset = (double)(-lo) * scale;
                            for (int i = 0; i < 256; ++i) {
                                const int v = (int)((double)i * scale + offset);
                                tlut[c][i] = (uint8_t)min(max(v, 0), 255);
                            }
                        }
                    } else {                                     // ImageOps.equalize: integer arithmetic, the table clipped to 255
                        int cnt = 0, last = 0;
                        long sum = 0;
                        for (int i = 0; i < 256; ++i) {
                            const int h = hist[c][i];
                            if (h) { ++cnt; sum += h; last = h; }
                        }
                        const long step = cnt <= 1 ? 0 : (sum - last) / 255;
                        if (step == 0) {
                            ident = true;
                        } else {
                            long acc = step / 2;
                            for (int i = 0; i < 256; ++i) {
                                tlut[c][i] = (uint8_t)(acc / step < 255 ? acc / step : 255);
                                acc += hist[c][i];
                            }
                        }
                    }
                    if (ident)
                        for (int i = 0; i < 256; ++i) tlut[c][i] = (uint8_t)i;
                }
            } else {
                const int a = (int)P[0];
                for (int i = tid; i < 768; i += AG_THREADS) {
                    const int v = i & 255;
                    (&tlut[0][0])[i] = (uint8_t)(op == OP_POSTERIZE ? (v & a) : op == OP_SOLARIZE ? (v < a ? v : 255 - v) : 255 - v);
                }
            }
            __syncthreads();
            for (int p = tid; p < n; p += AG_THREADS) {
                buf[3 * p] = tlut[0][buf[3 * p]];
                buf[3 * p + 1] = tlut[1][buf[3 * p + 1]];
                buf[3 * p + 2] = tlut[2][buf[3 * p + 2]];
            }
        } else if (op == OP_COLOR) {                             // blend with the image's L replicated
            const float f = ag_f32(P[0]);
            for (int p = tid; p < n; p += AG_THREADS) {
                const uint32_t v = ag_px(buf, p);
                const int L = ag_luma(v);
                ag_put(buf, p, ag_blend(L, v & 255u, f) | (ag_blend(L, (v >> 8) & 255u, f) << 8) | (ag_blend(L, (v >> 16) & 255u, f) << 16));
            }
        } else if (WIDE && op == OP_BRIGHTNESS) {                // blend with black
            const float f = ag_f32(P[0]);
            for (int i = tid; i < 3 * n; i += AG_THREADS) buf[i] = (uint8_t)ag_blend(0, buf[i], f);
        } else if (op == OP_CONTRAST) {                          // blend with the L mean, int(sum / n + 0.5)
            const float f = ag_f32(P[0]);
            if (tid == 0) lsum = 0;
            __syncthreads();
            int s = 0;
            for (int p = tid; p < n; p += AG_THREADS) s += ag_luma(ag_px(buf, p));
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if ((tid & 63) == 0) atomicAdd(&lsum, s);
            __syncthreads();
            const int mean = (int)((double)lsum / (double)n + 0.5);
            for (int p = tid; p < n; p += AG_THREADS) {
                const uint32_t v = ag_px(buf, p);
                ag_put(buf, p, ag_blend(mean, v & 255u, f) | (ag_blend(mean, (v >> 8) & 255u, f) << 8) | (ag_blend(mean, (v >> 16) & 255u, f) << 16));
            }
        } else if (op == OP_SHARPNESS) {                         // blend with ImageFilter.SMOOTH (border pixels copied)
            const float f = ag_f32(P[0]);
            constexpr float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
            const uint8_t* img = buf;
            ag_gather<LDS>(buf, alt, n, slot, [&](int p) -> uint32_t {
                const int y = p / S, x = p - y * S;
                const uint32_t v = ag_px(img, p);
                if (x == 0 || y == 0 || x == S - 1 || y == S - 1) return v;
                uint32_t r = 0;
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    float acc = 0.0f;
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx)
                            acc = acc + (dx == 0 && dy == 0 ? k5 : k1) * (float)img[3 * ((y + dy) * S + x + dx) + c];
                    const int deg = acc <= 0.0f ? 0 : acc >= 255.0f ? 255 : (int)((double)acc + 0.5);
                    r |= ag_blend(deg, (v >> (8 * c)) & 255u, f) << (8 * c);
                }
                return r;
            });
        } else if (op == OP_ROTATE) {                            // Image.rotate, NEAREST: Pillow's 16.16 fixed-point coordinates
            const long a0 = P[0], a1 = P[1], a3 = P[2], a4 = P[3], xo = P[4], yo = P[5];
            const uint8_t* img = buf;
            ag_gather<LDS>(buf, alt, n, slot, [&](int p) -> uint32_t {
                const int y = p / S, x = p - y * S;
                const long xs = (xo + a0 * x + a1 * y) >> 16, ys = (yo + a3 * x + a4 * y) >> 16;
                return (xs >= 0 && xs < S && ys >= 0 && ys < S) ? ag_px(img, (int)ys * S + (int)xs) : AG_FILL;
            });
        } else if (op == OP_SHEARX) {                            // Image.transform(AFFINE, BICUBIC), fill outside the image
            const double a0 = ag_f64(P[0]), a1 = ag_f64(P[1]), a2 = ag_f64(P[2]), a3 = ag_f64(P[3]), a4 = ag_f64(P[4]), a5 = ag_f64(P[5]);
            const uint8_t* img = buf;
            ag_gather<LDS>(buf, alt, n, slot, [&](int p) -> uint32_t {
                const int y = p / S, x = p - y * S;
                double xin = a0 * (x + 0.5) + a1 * (y + 0.5) + a2;
                double yin = a3 * (x + 0.5) + a4 * (y + 0.5) + a5;
                if (!(xin >= 0.0 && xin < (double)S && yin >= 0.0 && yin < (double)S)) return AG_FILL;
                xin -= 0.5;
                yin -= 0.5;
                const int xf = (int)floor(xin), yf = (int)floor(yin);
                const double dx = xin - xf, dy = yin - yf;
                int xs[4], ys[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    xs[j] = min(max(xf - 1 + j, 0), S - 1);
                    ys[j] = min(max(yf - 1 + j, 0), S - 1) * S;
                }
                uint32_t r = 0;
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    double row[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint8_t* q = img + 3 * ys[j] + c;
                        row[j] = ag_cubic(q[3 * xs[0]], q[3 * xs[1]], q[3 * xs[2]], q[3 * xs[3]], dx);
                    }
                    const double v = ag_cubic(row[0], row[1], row[2], row[3], dy);
                    r |= (uint32_t)(v <= 0.0 ? 0 : v >= 255.0 ? 255 : (int)v) << (8 * c);
                }
                return r;
            });
        } else if (WIDE == 2 && op == OP_GRAY) {                 // convert("L") in all three channels
            for (int p = tid; p < n; p += AG_THREADS) {
                const uint32_t L = (uint32_t)ag_luma(ag_px(buf, p));
                ag_put(buf, p, L | (L << 8) | (L << 16));
            }
        } else if (WIDE == 2 && op == OP_HUE) {
            const int shift = (int)P[0];
            for (int p = tid; p < n; p += AG_THREADS) ag_put(buf, p, ag_hue(ag_px(buf, p), shift));
        } else if (WIDE == 2 && op == OP_BLUR) {                 // three passes along the rows, a barrier, three along the columns
            const int R = (int)P[0];
            const uint32_t ww = (uint32_t)P[1], fw = (uint32_t)P[2];
            for (int dir = 0; dir < 2; ++dir) {
                // task 3 * line + channel: along the columns a wave's bytes are contiguous, along the rows 3 lanes share a pixel
                for (int t = tid; t < 3 * S; t += AG_THREADS) {
                    const int line = t / 3;
                    uint8_t* q = buf + (dir == 0 ? 3 * line * S + (t - 3 * line) : t);
                    for (int pass = 0; pass < 3; ++pass) ag_box_line(q, S, dir == 0 ? 3 : 3 * S, R, ww, fw);
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    float* __restrict__ o = out + (long)b * 3 * n;
    uint8_t* __restrict__ q = out_u8 ? out_u8 + (long)b * 3 * n : nullptr;
    const int nerase = WIDE ? (int)it[TT_NERASE] : 0;
    if (nerase == 0) {
        for (int p = tid; p < n; p += AG_THREADS) {
            const uint32_t v = ag_px(buf, p);
            const int c0 = v & 255u, c1 = (v >> 8) & 255u, c2 = (v >> 16) & 255u;
            o[p] = lut[c0];
            o[n + p] = lut[256 + c1];
            o[2 * n + p] = lut[512 + c2];
            if (q) ag_put(q, p, v);
        }
        return;
    }
    // random erasing, fused into the write: inside a box the fill replaces the look-up value, the last box that holds the pixel wins
    // (moving this loop out of line did not bring the no-box path closer to simseg_train_augment's and cost the erased lists 4 %)
    const int mode = (int)it[TT_MODE];
    const uint64_t seed = (uint64_t)it[TT_SEED];
    for (int p = tid; p < n; p += AG_THREADS) {
        const uint32_t v = ag_px(buf, p);
        const int y = p / S, x = p - y * S;
        int box = -1;
        for (int k = 0; k < nerase; ++k) {
            const int64_t* e = it + TT_BOX + 4 * k;
            if (y >= e[0] && y < e[0] + e[2] && x >= e[1] && x < e[1] + e[3]) box = k;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float r = lut[256 * c + ((v >> (8 * c)) & 255u)];
            if (box >= 0) {
                const uint64_t i = (uint64_t)(((long)b * TT_MAX_ERASE + box) * 3 + c) << 18;
                r = mode == ER_CONST ? 0.0f : ag_normal(seed, mode == ER_PIXEL ? i + (uint64_t)(y * 512 + x) : i);
            }
            o[c * n + p] = r;
        }
        if (q) ag_put(q, p, v);
    }
}

// ---- C entry points -----------------------------------------------------------------------------------------------------------------------
extern "C" int64_t simseg_train_augment_scratch_bytes(int64_t B, int64_t S) {
    if (B < 1 || S < AG_MIN_S || S > AG_MAX_S) return 0;
    return B * ag_slot_bytes(S) * (ag_in_lds(S) ? 1 : 2);
}
extern "C" int64_t simseg_train_transforms_scratch_bytes(int64_t B, int64_t S) { return simseg_train_augment_scratch_bytes(B, S); }
extern "C" int64_t simseg_train_chain_scratch_bytes(int64_t B, int64_t S) { return simseg_train_augment_scratch_bytes(B, S); }

static bool ag_finite(double v) { return v == v && v - v == 0.0; }

// One op of image b's chain (its code, its slots) is one the kernel can run: 0, or what is wrong was reported under `who`.
static int ag_check_op(const char* who, int64_t b, int k, int64_t op, const int64_t* P, int64_t count) {
    SS_CHECK(op >= 0 && op < count, "%s: image %ld: op %d has code %ld", who, (long)b, k + 1, (long)op);
    if (op == OP_POSTERIZE) SS_CHECK(P[0] >= 0 && P[0] <= 255, "%s: image %ld: posterize mask %ld", who, (long)b, (long)P[0]);
    if (op == OP_SOLARIZE) SS_CHECK(P[0] >= 0 && P[0] <= 256, "%s: image %ld: solarize threshold %ld", who, (long)b, (long)P[0]);
    if (op == OP_COLOR || op == OP_CONTRAST || op == OP_SHARPNESS || op == OP_BRIGHTNESS) {
        float f;
        const int32_t bits = (int32_t)P[0];
        memcpy(&f, &bits, 4);
        SS_CHECK(P[0] == bits && ag_finite(f), "%s: image %ld: the blend factor is not a finite float", who, (long)b);
    }
    if (op == OP_ROTATE)
        for (int i = 0; i < 6; ++i)
            SS_CHECK(P[i] > -(1ll << 40) && P[i] < (1ll << 40), "%s: image %ld: rotate coefficient %d out of range", who, (long)b, i);
    if (op == OP_SHEARX)
        for (int i = 0; i < 6; ++i) {
            double v;
            memcpy(&v, &P[i], 8);
            SS_CHECK(ag_finite(v) && fabs(v) < 1e6, "%s: image %ld: affine coefficient %d is not finite and small", who, (long)b, i);
        }
    if (op == OP_HUE) SS_CHECK(P[0] >= 0 && P[0] <= 255, "%s: image %ld: hue shift %ld, a byte is needed", who, (long)b, (long)P[0]);
    if (op == OP_BLUR) {                                         // fw = (2^24 - (2R + 1) ww) // 2: the weights sum to 2^24 or 2^24 - 1
        const int64_t R = P[0], ww = P[1], fw = P[2];
        SS_CHECK(R >= 0 && R <= AG_BLUR_MAX_R, "%s: image %ld: blur box radius %ld, 0 .. %d", who, (long)b, (long)R, AG_BLUR_MAX_R);
        SS_CHECK(ww > 0 && ww <= (1 << 24) && fw >= 0 && fw <= (1 << 23), "%s: image %ld: blur weights ww %ld, fw %ld out of range", who,
                 (long)b, (long)ww, (long)fw);
        const int64_t rest = (1 << 24) - (2 * R + 1) * ww - 2 * fw;
        SS_CHECK(rest == 0 || rest == 1, "%s: image %ld: blur weights ww %ld, fw %ld do not sum to 2^24 with R %ld", who, (long)b, (long)ww,
                 (long)fw, (long)R);
    }
    return 0;
}

// The entry points: every field of the host copy is checked, then the two launches.  WIDE: 1 the table of simseg_train_transforms,
// 2 that of simseg_train_chain.
template <int WIDE>
static int ag_run(const char* who, const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                  const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, int64_t S, void* scratch,
                  int64_t scratch_bytes, float* out, int64_t out_numel, void* out_u8, int64_t u8_bytes, void* stream) {
    SS_CHECK(src && img_tab && img_tab_host && tab && tab_host && lut && out && scratch, "%s: null pointer", who);
    SS_CHECK(B >= 1 && B < (1 << 20) && src_bytes > 0 && tab_numel > 0, "%s: bad sizes", who);
    SS_CHECK(S >= AG_MIN_S && S <= AG_MAX_S, "%s: the output size is %d .. %d, got %ld", who, AG_MIN_S, AG_MAX_S, (long)S);
    SS_CHECK(out_numel == B * 3 * S * S, "%s: out holds %ld floats, expected %ld", who, (long)out_numel, (long)(B * 3 * S * S));
    SS_CHECK(!out_u8 || u8_bytes == B * 3 * S * S, "%s: out_u8 holds %ld bytes, expected %ld", who, (long)u8_bytes, (long)(B * 3 * S * S));
    SS_CHECK(scratch_bytes >= simseg_train_augment_scratch_bytes(B, S), "%s: scratch of %ld bytes, %ld needed", who, (long)scratch_bytes,
             (long)simseg_train_augment_scratch_bytes(B, S));
    PpAxisCache axes{tab_host, tab_numel};                       // (a batch shares few axes)
    for (int64_t b = 0; b < B; ++b) {
        const int64_t* it = img_tab_host + b * ag_cols(WIDE);
        const int64_t H = it[AG_H], W = it[AG_W], top = it[AG_TOP], left = it[AG_LEFT], ch = it[AG_CH], cw = it[AG_CW];
        const int64_t RH = WIDE ? it[TT_RH] : S, RW = WIDE ? it[TT_RW] : S;
        SS_CHECK(pp_extent_ok(H, W), "%s: image %ld: bad source extent %ld x %ld", who, (long)b, (long)H, (long)W);
        SS_CHECK(pp_offset_ok(it[AG_SRC], H, W, src_bytes), "%s: image %ld: source offset out of range", who, (long)b);
        SS_CHECK(top >= 0 && left >= 0 && ch > 0 && cw > 0 && top + ch <= H && left + cw <= W,
                 "%s: image %ld: the crop box does not lie inside the image", who, (long)b);
        if (WIDE) {
            SS_CHECK(pp_extent_ok(RH, RW), "%s: image %ld: bad resized extent %ld x %ld", who, (long)b, (long)RH, (long)RW);
            SS_CHECK(it[TT_WTOP] >= 0 && it[TT_WLEFT] >= 0 && it[TT_WTOP] + S <= RH && it[TT_WLEFT] + S <= RW,
                     "%s: image %ld: the output window does not lie inside the resized %ld x %ld image", who, (long)b, (long)RH, (long)RW);
            SS_CHECK(it[TT_FLIP] == 0 || it[TT_FLIP] == 1, "%s: image %ld: flip is 0 or 1, got %ld", who, (long)b, (long)it[TT_FLIP]);
        }
        const char* e = axes.check(it[AG_HOFF], it[AG_HKS], cw, RW);
        SS_CHECK(!e, "%s: image %ld, horizontal: %s", who, (long)b, e);
        e = axes.check(it[AG_VOFF], it[AG_VKS], ch, RH);
        SS_CHECK(!e, "%s: image %ld, vertical: %s", who, (long)b, e);
        const int64_t nops = WIDE ? it[TT_NOPS] : 2;
        constexpr int max_ops = WIDE == 2 ? TC_MAX_OPS : TT_MAX_OPS;
        SS_CHECK(nops >= 0 && nops <= max_ops, "%s: image %ld: a chain of %ld ops, at most %d", who, (long)b, (long)nops, max_ops);
        for (int k = 0; k < (int)nops; ++k)
            if (int rc = ag_check_op(who, b, k, it[(WIDE ? TT_OP : AG_OP1) + k], it + ag_slot0(WIDE) + k * AG_SLOTS,
                                     WIDE == 2 ? OP_COUNT_CHAIN : WIDE ? OP_COUNT_WIDE : OP_COUNT))
                return rc;
        if (WIDE) {
            const int64_t ne = it[TT_NERASE];
            SS_CHECK(ne >= 0 && ne <= TT_MAX_ERASE, "%s: image %ld: %ld erase boxes, at most %d", who, (long)b, (long)ne, TT_MAX_ERASE);
            SS_CHECK(it[TT_MODE] >= 0 && it[TT_MODE] < ER_MODES, "%s: image %ld: erase mode %ld", who, (long)b, (long)it[TT_MODE]);
            for (int k = 0; k < (int)ne; ++k) {
                const int64_t* r = it + TT_BOX + 4 * k;
                SS_CHECK(r[0] >= 0 && r[1] >= 0 && r[2] > 0 && r[3] > 0 && r[2] <= S && r[3] <= S && r[0] + r[2] <= S && r[1] + r[3] <= S,
                         "%s: image %ld: erase box %d does not lie inside the %ld x %ld output", who, (long)b, k, (long)S, (long)S);
            }
        }
    }
    const int tiles = ((int)S + PP_TW - 1) / PP_TW * (((int)S + PP_TH - 1) / PP_TH);
    hipLaunchKernelGGL(augment_resize_kernel<WIDE>, dim3((unsigned)(B * tiles)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint8_t*>(src), img_tab, tab, static_cast<uint8_t*>(scratch), (int)S, tiles);
    SS_LAUNCH_CHECK(WIDE == 2 ? "train_chain (resize)" : WIDE ? "train_transforms (resize)" : "train_augment (resize)");
    uint8_t* s1 = static_cast<uint8_t*>(scratch);
    if (ag_in_lds(S)) {
        static bool attr = false;                                // (one per instance of this template)
        if (!attr) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(augment_ops_kernel<true, WIDE>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)ag_slot_bytes(AG_LDS_MAX_S));
            SS_CHECK(e == hipSuccess, "%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e));
            attr = true;
        }
        hipLaunchKernelGGL((augment_ops_kernel<true, WIDE>), dim3((unsigned)B), dim3(AG_THREADS), (size_t)ag_slot_bytes(S), (hipStream_t)stream,
                           img_tab, s1, nullptr, (int)S, lut, out, static_cast<uint8_t*>(out_u8));
    } else {
        hipLaunchKernelGGL((augment_ops_kernel<false, WIDE>), dim3((unsigned)B), dim3(AG_THREADS), 0, (hipStream_t)stream, img_tab, s1,
                           s1 + B * ag_slot_bytes(S), (int)S, lut, out, static_cast<uint8_t*>(out_u8));
    }
    SS_LAUNCH_CHECK(WIDE == 2 ? "train_chain (ops)" : WIDE ? "train_transforms (ops)" : "train_augment (ops)");
    return 0;
}

extern "C" int simseg_train_augment(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                                    const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, int64_t S,
                                    void* scratch, int64_t scratch_bytes, float* out, int64_t out_numel, void* out_u8, int64_t u8_bytes,
                                    void* stream) {
    return ag_run<0>("train_augment", src, src_bytes, img_tab, img_tab_host, B, tab, tab_host, tab_numel, lut, S, scratch, scratch_bytes, out,
                     out_numel, out_u8, u8_bytes, stream);
}

extern "C" int simseg_train_transforms(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                                       const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, int64_t S,
                                       void* scratch, int64_t scratch_bytes, float* out, int64_t out_numel, void* out_u8, int64_t u8_bytes,
                                       void* stream) {
    return ag_run<1>("train_transforms", src, src_bytes, img_tab, img_tab_host, B, tab, tab_host, tab_numel, lut, S, scratch,
                     scratch_bytes, out, out_numel, out_u8, u8_bytes, stream);
}

extern "C" int simseg_train_chain(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                                  const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, int64_t S, void* scratch,
                                  int64_t scratch_bytes, float* out, int64_t out_numel, void* out_u8, int64_t u8_bytes, void* stream) {
    return ag_run<2>("train_chain", src, src_bytes, img_tab, img_tab_host, B, tab, tab_host, tab_numel, lut, S, scratch, scratch_bytes, out,
                     out_numel, out_u8, u8_bytes, stream);
}
