// Pillow's uint8 resample (ImagingResample, 8 bits per channel) for one output tile, shared by image_preprocess_kernel (preproc.hip) and
// augment_resize_kernel (augment.hip), plus the host checks of the axis tables both entry points run before they launch.
//
// The arithmetic (per axis a host-made table of bounds (xmin, n) and 22-bit coefficients; one pass = clamp((2^21 + sum_i pixel[xmin + i] *
// k[i]) >> 22, 0, 255) in int32; horizontal pass first) is stated in DESIGN.md "Device-side image preprocessing" and preproc.resample_ref.
//
// Shape: a workgroup of 256 threads owns a PP_TH x PP_TW output tile.  The input rows the tile needs, [ymin(first row), ymin + n of the
// last row), pass through LDS in chunks of PP_CR rows: a wave resamples one input row horizontally, lane = output column, reading the
// contiguous RGB run [xmin, xmin + n) of the source row and writing R | G << 8 | B << 16 as ONE dword at hbuf[row][column]; then every
// thread adds the chunk's rows into the int32 accumulators of its PP_RPT output pixels (rows wave + 4 r of the tile, column = lane) and
// the next chunk follows.  Accumulators live across chunks, so the downscale ratio is not capped: a larger ratio is more chunks.  LDS:
// hbuf is written and read as dwords at consecutive addresses by consecutive lanes (ds_write_b32 / ds_read_b32: bank (a / 4) % 32 per
// 32-lane half, conflict-free), one read serves the three channels.  The vertical pass's row, bounds and coefficients are uniform over a
// wave (scalar loads).
#pragma once
#include <vector>

#include "common.h"

constexpr int PP_TW = 64, PP_TH = 32, PP_CR = 48, PP_RPT = PP_TH / 4;
constexpr int PP_BITS = 22;

__device__ __forceinline__ int pp_clip8(int acc) { return min(max(acc >> PP_BITS, 0), 255); }

// One tile.  hbuf: the caller's __shared__ uint32_t [PP_CR * PP_TW]; src: the pixel that column 0 / row 0 of the axis tables name, rows
// `pitch` pixels apart; hb / vb: bounds [n_out, 2] of the two axes, hk / vk: their coefficients [n_out, hks / vks]; X0, Y0: the tile's
// first column and row in those tables; nx <= PP_TW, 1 <= ny <= PP_TH: its valid extent.  sink(yy, lane, c0, c1, c2) receives every
// finished pixel (row yy, column lane of the tile) once; let it capture by copy (through a by-reference capture the compiler re-reads
// the captured values after every store and no longer hoists a test such as "is there a uint8 output" out of the rows).  All 256 threads
// call pp_resample_tile (it waits at barriers); the caller's own LDS writes need their barrier before the call.
template <class Sink>
__device__ __forceinline__ void pp_resample_tile(uint32_t* hbuf, const uint8_t* __restrict__ src, long pitch, const int* __restrict__ hb,
                                                 const int* __restrict__ hk, int hks, const int* __restrict__ vb, const int* __restrict__ vk,
                                                 int vks, int X0, int Y0, int nx, int ny, Sink sink) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // this lane's column of the horizontal pass
    const bool xin = lane < nx;
    const int X = X0 + lane;
    const int hx = xin ? hb[2 * X] : 0, hn = xin ? hb[2 * X + 1] : 0;
    const int* __restrict__ hkx = hk + (long)(xin ? X : 0) * hks;
    // the tile's input rows (uniform over the workgroup)
    const int rmin = vb[2 * Y0], rmax = vb[2 * (Y0 + ny - 1)] + vb[2 * (Y0 + ny - 1) + 1];
    int acc[PP_RPT][3];
#pragma unroll
    for (int r = 0; r < PP_RPT; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (PP_BITS - 1);
    for (int r0 = rmin; r0 < rmax; r0 += PP_CR) {
        const int rows = min(PP_CR, rmax - r0);
        // horizontal pass: input rows r0 .. r0 + rows - 1 at the tile's columns -> LDS, one packed RGB dword per (row, column)
        for (int rr = wave; rr < rows; rr += 4) {
            const uint8_t* __restrict__ p = src + ((long)(r0 + rr) * pitch + hx) * 3;
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
#pragma unroll
    for (int r = 0; r < PP_RPT; ++r) {
        const int yy = wave + 4 * r;
        if (yy < ny) sink(yy, lane, pp_clip8(acc[r][0]), pp_clip8(acc[r][1]), pp_clip8(acc[r][2]));
    }
}

// ---- host checks, on the host copies of the tables, before any launch ------------------------------------------------------------------------
// One axis table is sound (preproc.hip): nullptr, or what is wrong with it.
const char* pp_check_axis(const int32_t* tab_host, int64_t tab_numel, int64_t off, int64_t ks, int64_t n_in, int64_t n_out);

// pp_check_axis once per distinct axis of a call (a batch shares few).
struct PpAxisCache {
    const int32_t* tab_host;
    int64_t tab_numel;
    struct Axis { int64_t off, ks, n_in, n_out; };
    std::vector<Axis> seen;
    const char* check(int64_t off, int64_t ks, int64_t n_in, int64_t n_out) {
        for (const Axis& a : seen)
            if (a.off == off && a.ks == ks && a.n_in == n_in && a.n_out == n_out) return nullptr;
        const char* e = pp_check_axis(tab_host, tab_numel, off, ks, n_in, n_out);
        if (!e) seen.push_back({off, ks, n_in, n_out});
        return e;
    }
};

// What both entry points ask of image b's packed source before anything reads it: an extent that is positive and bounded (so that
// H * W * 3 cannot overflow), at an offset inside the src_bytes of the batch.  Each reports a failure under its own name.
constexpr int64_t PP_LIM = 1ll << 30;
inline bool pp_extent_ok(int64_t H, int64_t W) { return H > 0 && W > 0 && H < PP_LIM && W < PP_LIM && H * W < PP_LIM; }
inline bool pp_offset_ok(int64_t off, int64_t H, int64_t W, int64_t src_bytes) { return off >= 0 && off + H * W * 3 <= src_bytes; }
