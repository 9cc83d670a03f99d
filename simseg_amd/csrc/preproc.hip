// Image preprocessing on the device: decoded uint8 [H, W, 3] images -> Pillow's uint8 resize (bilinear / bicubic, optional crop
// rectangle) -> normalised fp32 [3, OH, OW] planes, for a whole batch of images of different sizes in ONE launch.
//
// The arithmetic is Pillow's (ImagingResample, 8 bits per channel) and is stated in DESIGN.md "Device-side image preprocessing" and in
// simseg_amd/preproc.py (resample_ref): per axis a table of bounds (xmin, n) and 22-bit fixed-point coefficients, computed in float64
// on the host; one pass = clamp((2^21 + sum_i pixel[xmin + i] * k[i]) >> 22, 0, 255) in int32; horizontal pass first, its uint8 result
// is the input of the vertical pass; an axis whose length does not change gets the identity table (n = 1, k = 2^22: exactly the input
// byte).  The fp32 value is LUT[channel][byte], a table the host fills with its own normalisation arithmetic, so nothing here divides.
//
// Shape: a workgroup of 256 threads owns a PP_TH x PP_TW output tile of one image (found by a binary search of the tile index in the image
// table's tile_start column).  The input rows the tile needs, [ymin(first row), ymin + n of the last row), pass through LDS in chunks of
// PP_CR rows: a wave resamples one input row horizontally, lane = output column, reading the contiguous RGB run [xmin, xmin + n) of the
// source row and writing R | G << 8 | B << 16 as ONE dword at hbuf[row][column]; then every thread adds the chunk's rows into the int32
// accumulators of its PP_RPT output pixels (rows wave + 4 r of the tile, column = lane) and the next chunk follows.  Accumulators live
// across chunks, so the downscale ratio is not capped: a larger ratio is more chunks.  LDS: hbuf is written and read as dwords at
// consecutive addresses by consecutive lanes (ds_write_b32 / ds_read_b32: bank (a / 4) % 32 per 32-lane half, conflict-free), one read
// serves the three channels; 12 KiB of hbuf + 3 KiB of LUT per workgroup leaves ten workgroups per CU by LDS.  The vertical pass's row,
// bounds and coefficients are uniform over a wave (scalar loads).  Stores: a wave writes 64 consecutive floats of one plane row, two
// whole 128-byte lines when the plane's rows are 128-byte aligned ([B, 3, S, S] with S % 32 == 0); ragged planes lie back to back
// unpadded, their rows start anywhere, and the same 256-byte run then straddles three lines.
#include <vector>

#include "common.h"

constexpr int PP_IT = 16;        // int64 columns of the image table
constexpr int PP_TW = 64, PP_TH = 32, PP_CR = 48, PP_RPT = PP_TH / 4;
constexpr int PP_BITS = 22;

enum { PP_SRC = 0, PP_H, PP_W, PP_OUT, PP_OH, PP_OW, PP_TOP, PP_LEFT, PP_HOFF, PP_HKS, PP_VOFF, PP_VKS, PP_RH, PP_RW, PP_U8, PP_TILE };

__device__ __forceinline__ int pp_clip8(int acc) { return min(max(acc >> PP_BITS, 0), 255); }

__global__ __launch_bounds__(256) void image_preprocess_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ img_tab,
                                                               const int* __restrict__ tab, const float* __restrict__ lut,
                                                               float* __restrict__ out, uint8_t* __restrict__ out_u8, int B) {
    __shared__ uint32_t hbuf[PP_CR * PP_TW];
    __shared__ float slut[3 * 256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 3 * 256; i += 256) slut[i] = lut[i];
    // the image of this tile: the last one whose first tile is not behind blockIdx.x
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (img_tab[(long)mid * PP_IT + PP_TILE] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int64_t* it = img_tab + (long)lo * PP_IT;
    const long src_off = it[PP_SRC], out_off = it[PP_OUT], u8_off = it[PP_U8];
    const int W = (int)it[PP_W], OH = (int)it[PP_OH], OW = (int)it[PP_OW], top = (int)it[PP_TOP], left = (int)it[PP_LEFT];
    const int hks = (int)it[PP_HKS], vks = (int)it[PP_VKS], RH = (int)it[PP_RH], RW = (int)it[PP_RW];
    const int* __restrict__ hb = tab + it[PP_HOFF];          // bounds [RW, 2], then coefficients [RW, hks]
    const int* __restrict__ hk = hb + 2 * (long)RW;
    const int* __restrict__ vb = tab + it[PP_VOFF];          // bounds [RH, 2], then coefficients [RH, vks]
    const int* __restrict__ vk = vb + 2 * (long)RH;
    const int tile = (int)((int64_t)blockIdx.x - it[PP_TILE]);
    const int tiles_x = (OW + PP_TW - 1) / PP_TW;
    const int x0 = (tile % tiles_x) * PP_TW, y0 = (tile / tiles_x) * PP_TH;
    const int nx = min(PP_TW, OW - x0), ny = min(PP_TH, OH - y0);
    if (ny <= 0) return;                                     // (a tile index past the image's tiles: never launched by a validated table)
    // this lane's column of the horizontal pass
    const bool xin = lane < nx;
    const int X = left + x0 + lane;                          // column of the resized image
    const int hx = xin ? hb[2 * X] : 0, hn = xin ? hb[2 * X + 1] : 0;
    const int* __restrict__ hkx = hk + (long)(xin ? X : 0) * hks;
    // this wave's rows of the vertical pass (uniform over the wave)
    const int Y0 = top + y0;
    const int rmin = vb[2 * Y0], rmax = vb[2 * (Y0 + ny - 1)] + vb[2 * (Y0 + ny - 1) + 1];
    int acc[PP_RPT][3];
#pragma unroll
    for (int r = 0; r < PP_RPT; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (PP_BITS - 1);
    __syncthreads();                                         // LUT in place
    for (int r0 = rmin; r0 < rmax; r0 += PP_CR) {
        const int rows = min(PP_CR, rmax - r0);
        // horizontal pass: input rows r0 .. r0 + rows - 1 at the tile's columns -> LDS, one packed RGB dword per (row, column)
        for (int rr = wave; rr < rows; rr += 4) {
            const uint8_t* __restrict__ p = src + src_off + ((long)(r0 + rr) * W + hx) * 3;
            int a0 = 1 << (PP_BITS - 1), a1 = a0, a2 = a0;
            for (int i = 0; i < hn; ++i) {
                const int k = hkx[i];
                a0 += (int)p[3 * i] * k;
                a1 += (int)p[3 * i + 1] * k;
                a2 += (int)p[3 * i + 2] * k;
            }
            hbuf[rr * PP_TW + lane] = (uint32_t)pp_clip8(a0) | ((uint32_t)pp_clip8(a1) << 8) | ((uint32_t)pp_clip8(a2) << 16);
        }
        __syncthreads();
        // vertical pass: every output row takes the rows of this chunk that lie inside its bounds
#pragma unroll
        for (int r = 0; r < PP_RPT; ++r) {
            const int yy = wave + 4 * r;
            if (yy < ny) {
                const int Y = Y0 + yy;
                const int ymin = vb[2 * Y], yn = vb[2 * Y + 1];
                const int* __restrict__ vky = vk + (long)Y * vks;
                const int jlo = max(ymin, r0), jhi = min(ymin + yn, r0 + rows);
                for (int j = jlo; j < jhi; ++j) {
                    const int k = vky[j - ymin];
                    const uint32_t v = hbuf[(j - r0) * PP_TW + lane];
                    acc[r][0] += (int)(v & 255u) * k;
                    acc[r][1] += (int)((v >> 8) & 255u) * k;
                    acc[r][2] += (int)((v >> 16) & 255u) * k;
                }
            }
        }
        __syncthreads();
    }
    if (!xin) return;
    const long plane = (long)OH * OW;
#pragma unroll
    for (int r = 0; r < PP_RPT; ++r) {
        const int yy = wave + 4 * r;
        if (yy < ny) {
            const long at = (long)(y0 + yy) * OW + x0 + lane;
            const int c0 = pp_clip8(acc[r][0]), c1 = pp_clip8(acc[r][1]), c2 = pp_clip8(acc[r][2]);
            out[out_off + at] = slut[c0];
            out[out_off + plane + at] = slut[256 + c1];
            out[out_off + 2 * plane + at] = slut[512 + c2];
            if (out_u8) {
                uint8_t* q = out_u8 + u8_off + at * 3;
                q[0] = (uint8_t)c0; q[1] = (uint8_t)c1; q[2] = (uint8_t)c2;
            }
        }
    }
}

// One axis table on the host copy: bounds inside the input, n <= ksize, monotone (the kernel takes a tile's input span from its first and
// last row), and 255 * sum|k| + 2^21 inside int32.  Also used by augment.hip.
const char* pp_check_axis(const int32_t* tab_host, int64_t tab_numel, int64_t off, int64_t ks, int64_t n_in, int64_t n_out) {
    if (off < 0 || ks < 1 || n_out < 1 || n_in < 1 || ks > (1 << 24) || off + n_out * (2 + ks) > tab_numel) return "axis table out of range";
    const int32_t* b = tab_host + off;
    const int32_t* k = b + 2 * n_out;
    int64_t pmin = 0, pmax = 0;
    for (int64_t x = 0; x < n_out; ++x) {
        const int64_t xmin = b[2 * x], n = b[2 * x + 1];
        if (xmin < 0 || n < 1 || n > ks || xmin + n > n_in) return "axis bounds outside the input (0 <= xmin, 1 <= n <= ksize, xmin + n <= in)";
        if (xmin < pmin || xmin + n < pmax) return "axis bounds are not monotone";
        pmin = xmin; pmax = xmin + n;
        int64_t s = 0;
        for (int64_t i = 0; i < n; ++i) s += k[x * ks + i] < 0 ? -(int64_t)k[x * ks + i] : (int64_t)k[x * ks + i];
        if (255 * s + (1 << (PP_BITS - 1)) >= (1ll << 31)) return "axis coefficients overflow the int32 accumulator";
    }
    return nullptr;
}

extern "C" int simseg_image_preprocess(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                                       const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, float* out,
                                       int64_t out_numel, void* out_u8, int64_t u8_bytes, void* stream) {
    SS_CHECK(src && img_tab && img_tab_host && tab && tab_host && lut && out, "image_preprocess: null pointer");
    SS_CHECK(B >= 1 && B < (1 << 24) && src_bytes > 0 && tab_numel > 0 && out_numel > 0, "image_preprocess: bad sizes");
    SS_CHECK(!out_u8 || u8_bytes > 0, "image_preprocess: a uint8 output needs its size");
    struct Axis { int64_t off, ks, n_in, n_out; };
    std::vector<Axis> seen;
    auto axis = [&](int64_t off, int64_t ks, int64_t n_in, int64_t n_out) -> const char* {
        for (const Axis& a : seen)
            if (a.off == off && a.ks == ks && a.n_in == n_in && a.n_out == n_out) return nullptr;
        const char* e = pp_check_axis(tab_host, tab_numel, off, ks, n_in, n_out);
        if (!e) seen.push_back({off, ks, n_in, n_out});
        return e;
    };
    int64_t tiles = 0;
    const int64_t lim = 1ll << 30;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t* it = img_tab_host + b * PP_IT;
        const int64_t H = it[PP_H], W = it[PP_W], OH = it[PP_OH], OW = it[PP_OW], RH = it[PP_RH], RW = it[PP_RW];
        SS_CHECK(H > 0 && W > 0 && H < lim && W < lim && H * W < lim, "image_preprocess: image %ld: bad source extent %ld x %ld", (long)b, (long)H, (long)W);
        SS_CHECK(OH > 0 && OW > 0 && RH > 0 && RW > 0 && RH < lim && RW < lim && OH * OW < lim, "image_preprocess: image %ld: OH, OW, RH, RW must be positive", (long)b);
        SS_CHECK(it[PP_TOP] >= 0 && it[PP_LEFT] >= 0 && it[PP_TOP] + OH <= RH && it[PP_LEFT] + OW <= RW,
                 "image_preprocess: image %ld: the output rectangle does not lie inside the resized image", (long)b);
        SS_CHECK(it[PP_SRC] >= 0 && it[PP_SRC] + H * W * 3 <= src_bytes, "image_preprocess: image %ld: source offset out of range", (long)b);
        SS_CHECK(it[PP_OUT] >= 0 && it[PP_OUT] + 3 * OH * OW <= out_numel, "image_preprocess: image %ld: output offset out of range", (long)b);
        SS_CHECK(!out_u8 || (it[PP_U8] >= 0 && it[PP_U8] + 3 * OH * OW <= u8_bytes), "image_preprocess: image %ld: uint8 output offset out of range", (long)b);
        SS_CHECK(it[PP_TILE] == tiles, "image_preprocess: image %ld: tile_start %ld, expected %ld", (long)b, (long)it[PP_TILE], (long)tiles);
        const char* e = axis(it[PP_HOFF], it[PP_HKS], W, RW);
        SS_CHECK(!e, "image_preprocess: image %ld, horizontal: %s", (long)b, e);
        e = axis(it[PP_VOFF], it[PP_VKS], H, RH);
        SS_CHECK(!e, "image_preprocess: image %ld, vertical: %s", (long)b, e);
        tiles += ((OW + PP_TW - 1) / PP_TW) * ((OH + PP_TH - 1) / PP_TH);
        SS_CHECK(tiles < (1ll << 31), "image_preprocess: too many tiles in one call");
    }
    hipLaunchKernelGGL(image_preprocess_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t*>(src), img_tab,
                       tab, lut, out, static_cast<uint8_t*>(out_u8), (int)B);
    SS_LAUNCH_CHECK("image_preprocess");
    return 0;
}
