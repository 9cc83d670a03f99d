// Image preprocessing on the device: decoded uint8 [H, W, 3] images -> Pillow's uint8 resize (bilinear / bicubic, optional crop
// rectangle) -> normalised fp32 [3, OH, OW] planes, for a whole batch of images of different sizes in ONE launch.
//
// The resample itself - its arithmetic, the PP_TH x PP_TW output tile of a 256-thread workgroup and the passes through LDS - is
// resample.h's pp_resample_tile.  This kernel finds its tile's image by a binary search of the tile index in the image table's
// tile_start column, places the tile inside the resized image (the optional crop rectangle is an offset into the axis tables) and takes
// each finished pixel: the fp32 value is LUT[channel][byte], a table the host fills with its own normalisation arithmetic, so nothing
// here divides.  12 KiB of hbuf + 3 KiB of LUT per workgroup leaves ten workgroups per CU by LDS.  Stores: a wave writes 64 consecutive
// floats of one plane row, two whole 128-byte lines when the plane's rows are 128-byte aligned ([B, 3, S, S] with S % 32 == 0); ragged
// planes lie back to back unpadded, their rows start anywhere, and the same 256-byte run then straddles three lines.
#include "resample.h"

constexpr int PP_IT = 16;        // int64 columns of the image table

enum { PP_SRC = 0, PP_H, PP_W, PP_OUT, PP_OH, PP_OW, PP_TOP, PP_LEFT, PP_HOFF, PP_HKS, PP_VOFF, PP_VKS, PP_RH, PP_RW, PP_U8, PP_TILE };

__global__ __launch_bounds__(256) void image_preprocess_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ img_tab,
                                                               const int* __restrict__ tab, const float* __restrict__ lut,
                                                               float* __restrict__ out, uint8_t* __restrict__ out_u8, int B) {
    __shared__ uint32_t hbuf[PP_CR * PP_TW];
    __shared__ float slut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) slut[i] = lut[i];
    // the image of this tile: the last one whose first tile is not behind blockIdx.x
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (img_tab[(long)mid * PP_IT + PP_TILE] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int64_t* it = img_tab + (long)lo * PP_IT;
    const long out_off = it[PP_OUT], u8_off = it[PP_U8];
    const int W = (int)it[PP_W], OH = (int)it[PP_OH], OW = (int)it[PP_OW];
    const int RH = (int)it[PP_RH], RW = (int)it[PP_RW];
    const int* __restrict__ hb = tab + it[PP_HOFF];          // bounds [RW, 2], then coefficients [RW, hks]
    const int* __restrict__ vb = tab + it[PP_VOFF];          // bounds [RH, 2], then coefficients [RH, vks]
    const int tile = (int)((int64_t)blockIdx.x - it[PP_TILE]);
    const int tiles_x = (OW + PP_TW - 1) / PP_TW;
    const int x0 = (tile % tiles_x) * PP_TW, y0 = (tile / tiles_x) * PP_TH;
    const int nx = min(PP_TW, OW - x0), ny = min(PP_TH, OH - y0);
    if (ny <= 0) return;                                     // (a tile index past the image's tiles: never launched by a validated table)
    const long plane = (long)OH * OW;
    __syncthreads();                                         // LUT in place
    pp_resample_tile(hbuf, src + it[PP_SRC], W, hb, hb + 2 * (long)RW, (int)it[PP_HKS], vb, vb + 2 * (long)RH, (int)it[PP_VKS],
                     (int)it[PP_LEFT] + x0, (int)it[PP_TOP] + y0, nx, ny, [=](int yy, int lane, int c0, int c1, int c2) {
        const long at = (long)(y0 + yy) * OW + x0 + lane;
        out[out_off + at] = slut[c0];
        out[out_off + plane + at] = slut[256 + c1];
        out[out_off + 2 * plane + at] = slut[512 + c2];
        if (out_u8) {
            uint8_t* q = out_u8 + u8_off + at * 3;
            q[0] = (uint8_t)c0; q[1] = (uint8_t)c1; q[2] = (uint8_t)c2;
        }
    });
}

// One axis table on the host copy: bounds inside the input, n <= ksize, monotone (the kernel takes a tile's input span from its first and
// last row), and 255 * sum|k| + 2^21 inside int32.  Both entry points call it through resample.h's PpAxisCache.
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
    PpAxisCache axes{tab_host, tab_numel};
    int64_t tiles = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t* it = img_tab_host + b * PP_IT;
        const int64_t H = it[PP_H], W = it[PP_W], OH = it[PP_OH], OW = it[PP_OW], RH = it[PP_RH], RW = it[PP_RW];
        SS_CHECK(pp_extent_ok(H, W), "image_preprocess: image %ld: bad source extent %ld x %ld", (long)b, (long)H, (long)W);
        SS_CHECK(OH > 0 && OW > 0 && RH > 0 && RW > 0 && RH < PP_LIM && RW < PP_LIM && OH * OW < PP_LIM, "image_preprocess: image %ld: OH, OW, RH, RW must be positive", (long)b);
        SS_CHECK(it[PP_TOP] >= 0 && it[PP_LEFT] >= 0 && it[PP_TOP] + OH <= RH && it[PP_LEFT] + OW <= RW,
                 "image_preprocess: image %ld: the output rectangle does not lie inside the resized image", (long)b);
        SS_CHECK(pp_offset_ok(it[PP_SRC], H, W, src_bytes), "image_preprocess: image %ld: source offset out of range", (long)b);
        SS_CHECK(it[PP_OUT] >= 0 && it[PP_OUT] + 3 * OH * OW <= out_numel, "image_preprocess: image %ld: output offset out of range", (long)b);
        SS_CHECK(!out_u8 || (it[PP_U8] >= 0 && it[PP_U8] + 3 * OH * OW <= u8_bytes), "image_preprocess: image %ld: uint8 output offset out of range", (long)b);
        SS_CHECK(it[PP_TILE] == tiles, "image_preprocess: image %ld: tile_start %ld, expected %ld", (long)b, (long)it[PP_TILE], (long)tiles);
        const char* e = axes.check(it[PP_HOFF], it[PP_HKS], W, RW);
        SS_CHECK(!e, "image_preprocess: image %ld, horizontal: %s", (long)b, e);
        e = axes.check(it[PP_VOFF], it[PP_VKS], H, RH);
        SS_CHECK(!e, "image_preprocess: image %ld, vertical: %s", (long)b, e);
        tiles += ((OW + PP_TW - 1) / PP_TW) * ((OH + PP_TH - 1) / PP_TH);
        SS_CHECK(tiles < (1ll << 31), "image_preprocess: too many tiles in one call");
    }
    hipLaunchKernelGGL(image_preprocess_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t*>(src), img_tab,
                       tab, lut, out, static_cast<uint8_t*>(out_u8), (int)B);
    SS_LAUNCH_CHECK("image_preprocess");
    return 0;
}
