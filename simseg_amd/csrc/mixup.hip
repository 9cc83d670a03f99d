// Mixup / CutMix of an image batch in place (timm's Mixup, the batch-level transform of ViT fine-tuning recipes): one launch per batch,
// driven by a per-sample table.  Compiled ONCE: the 16-bit flavour (bf16 / fp16) is a template argument chosen from the calling thread's
// simseg_set_half_type, as in probe.hip.
//
// The partner of sample i is j = B - 1 - i (x.flip(0)); both are rewritten by the same launch, so the unit of work is the PAIR (i, j),
// i < B / 2: whoever forms out_i at a position also forms out_j there, from values it loaded before it stores either.  No position of
// a pair is visited by two threads, so every element is read at most once and written at most once, and the result cannot depend on
// the order in which blocks run.
#include "common.h"

namespace {

// One table row (eight int32 words; include/simseg_hip.h).
struct MixRow { int kind, yl, yh, xl, xh; float lam, om; int pad; };
static_assert(sizeof(MixRow) == 32, "table rows are eight 4-byte words");

// VW consecutive elements moved as one access (16 bytes when VW is the type's full width).
template <typename T, int VW>
struct alignas(sizeof(T) * VW) Pack { T v[VW]; };

template <typename T>
struct Full { static constexpr int VW = 16 / sizeof(T); };

constexpr int MIX_TILE = 1024;          // chunks per work item: 256 lanes x 4

__device__ __forceinline__ bool in_box(const MixRow& r, int y, int x) { return y >= r.yl && y < r.yh && x >= r.xl && x < r.xh; }

// out = fl32(fl32(lam * own) + fl32(om * other)), rounded once to the storage type: two rounded products and a rounded sum, never an FMA.
// (HIP's __fmul_rn / __fadd_rn are plain * and + that the compiler's default contraction would fuse: contraction is switched off for
// these statements instead, and the flag stays on the instructions through inlining.)
template <typename T>
__device__ __forceinline__ T blend(const MixRow& r, T own, T other) {
#pragma clang fp contract(off)
    const float a = r.lam * (float)own;
    const float b = r.om * (float)other;
    return (T)(a + b);
}

// A pair with a mixup row: every element of both samples is loaded (four chunks per lane in flight), both results are formed, and each
// side that changes is stored.  A cutmix partner (elem mode) selects per element by its own box; a kind-0 partner is not stored.
template <typename T, int VW>
__device__ __forceinline__ void flat_tile(T* xi, T* xj, const MixRow& ri, const MixRow& rj, int H, int W, long nchunks, int tile) {
    typedef Pack<T, VW> P;
    const long q0 = (long)tile * MIX_TILE + threadIdx.x;
    P a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long q = q0 + k * 256;
        if (q < nchunks) {
            a[k] = *reinterpret_cast<const P*>(xi + q * VW);
            b[k] = *reinterpret_cast<const P*>(xj + q * VW);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long q = q0 + k * 256;
        if (q >= nchunks) continue;
        P oi, oj;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            int y = 0, x = 0;
            if (ri.kind == 2 || rj.kind == 2) {          // (block-uniform; only an elem-mode pair pays for the coordinates)
                const unsigned idx = (unsigned)(q * VW + e), row = idx / (unsigned)W;
                x = (int)(idx - row * (unsigned)W);
                y = (int)(row % (unsigned)H);
            }
            const T va = a[k].v[e], vb = b[k].v[e];
            oi.v[e] = ri.kind == 1 ? blend(ri, va, vb) : (in_box(ri, y, x) ? vb : va);
            oj.v[e] = rj.kind == 1 ? blend(rj, vb, va) : (in_box(rj, y, x) ? va : vb);
        }
        if (ri.kind != 0) *reinterpret_cast<P*>(xi + q * VW) = oi;
        if (rj.kind != 0) *reinterpret_cast<P*>(xj + q * VW) = oj;
    }
}

// A pair without a mixup row: only the boxes move.  The work is the hull of the (non-empty) boxes over every channel, in chunks of VW
// along a row (W % VW == 0, so a chunk never leaves its row); a chunk outside both boxes touches no memory, a chunk inside one is moved
// whole, a chunk across an edge is loaded whole and stored element by element.  Side i needs x_j where box_i covers, side j needs x_i
// where box_j covers: a position in neither box is neither read for a result nor written.
template <typename T, int VW>
__device__ __forceinline__ void box_tile(T* xi, T* xj, const MixRow& ri, const MixRow& rj, int C, int H, int W, int tile) {
    typedef Pack<T, VW> P;
    const bool ai = ri.kind == 2 && ri.yl < ri.yh && ri.xl < ri.xh, aj = rj.kind == 2 && rj.yl < rj.yh && rj.xl < rj.xh;
    if (!ai && !aj) return;
    const int ylo = ai && aj ? min(ri.yl, rj.yl) : ai ? ri.yl : rj.yl, yhi = ai && aj ? max(ri.yh, rj.yh) : ai ? ri.yh : rj.yh;
    const int xlo = ai && aj ? min(ri.xl, rj.xl) : ai ? ri.xl : rj.xl, xhi = ai && aj ? max(ri.xh, rj.xh) : ai ? ri.xh : rj.xh;
    const int cx0 = xlo / VW, hw = (xhi + VW - 1) / VW - cx0, hh = yhi - ylo;
    const unsigned plane = (unsigned)hh * (unsigned)hw;
    const long hull = (long)C * plane;
    constexpr unsigned FULL = (1u << VW) - 1u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long idx = (long)tile * MIX_TILE + k * 256 + threadIdx.x;
        if (idx >= hull) continue;
        const unsigned c = (unsigned)(idx / plane), r = (unsigned)(idx - (long)c * plane), ry = r / (unsigned)hw;
        const int y = ylo + (int)ry, x0 = (cx0 + (int)(r - ry * (unsigned)hw)) * VW;
        unsigned mi = 0, mj = 0;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            mi |= (ai && in_box(ri, y, x0 + e) ? 1u : 0u) << e;
            mj |= (aj && in_box(rj, y, x0 + e) ? 1u : 0u) << e;
        }
        if (!(mi | mj)) continue;
        const long off = ((long)c * H + y) * W + x0;
        P a, b;
        if (mj) a = *reinterpret_cast<const P*>(xi + off);
        if (mi) b = *reinterpret_cast<const P*>(xj + off);
        if (mi == FULL) {
            *reinterpret_cast<P*>(xi + off) = b;
        } else if (mi) {
#pragma unroll
            for (int e = 0; e < VW; ++e)
                if ((mi >> e) & 1u) xi[off + e] = b.v[e];
        }
        if (mj == FULL) {
            *reinterpret_cast<P*>(xj + off) = a;
        } else if (mj) {
#pragma unroll
            for (int e = 0; e < VW; ++e)
                if ((mj >> e) & 1u) xj[off + e] = a.v[e];
        }
    }
}

// Work item = (pair, tile of MIX_TILE chunks), grid-stride.  VF: chunk width of a pair with a mixup row (the flat sample), VB: of a
// box-only pair (along a row); 1 is the scalar path.
template <typename T, int VF, int VB>
__global__ __launch_bounds__(256) void mix_batch_kernel(T* images, const MixRow* __restrict__ table, int B, int C, int H, int W, long n,
                                                        int tiles, long total) {
    for (long work = blockIdx.x; work < total; work += gridDim.x) {
        const int pair = (int)(work / tiles), tile = (int)(work - (long)pair * tiles);
        const MixRow ri = table[pair], rj = table[B - 1 - pair];
        T* xi = images + (long)pair * n;
        T* xj = images + (long)(B - 1 - pair) * n;
        if (ri.kind == 1 || rj.kind == 1) flat_tile<T, VF>(xi, xj, ri, rj, H, W, n / VF, tile);
        else if (ri.kind == 2 || rj.kind == 2) box_tile<T, VB>(xi, xj, ri, rj, C, H, W, tile);
    }
}

template <typename T>
int mix_batch_launch(void* images, const int32_t* table, int64_t B, int64_t C, int64_t H, int64_t W, hipStream_t s) {
    constexpr int VW = Full<T>::VW;
    const long n = (long)(C * H * W);
    const bool vf = n % VW == 0 && ((uintptr_t)images % 16) == 0;       // every sample then starts on 16 bytes
    const bool vb = vf && W % VW == 0;
    const long chunks = n / (vb ? VW : 1);                              // (VB <= VF: the box walk has the most chunks)
    const int tiles = (int)((chunks + MIX_TILE - 1) / MIX_TILE);
    const long total = (B / 2) * tiles;
    const dim3 grid((unsigned)(total < 2048 ? total : 2048));
    T* x = (T*)images;
    const MixRow* t = (const MixRow*)table;
    if (vb) hipLaunchKernelGGL((mix_batch_kernel<T, VW, VW>), grid, dim3(256), 0, s, x, t, (int)B, (int)C, (int)H, (int)W, n, tiles, total);
    else if (vf) hipLaunchKernelGGL((mix_batch_kernel<T, VW, 1>), grid, dim3(256), 0, s, x, t, (int)B, (int)C, (int)H, (int)W, n, tiles, total);
    else hipLaunchKernelGGL((mix_batch_kernel<T, 1, 1>), grid, dim3(256), 0, s, x, t, (int)B, (int)C, (int)H, (int)W, n, tiles, total);
    SS_LAUNCH_CHECK("mix_batch");
    return 0;
}

}  // namespace

extern "C" int simseg_mix_batch(void* images, int dt, const int32_t* table, const int32_t* table_host, int64_t B, int64_t C, int64_t H,
                                int64_t W, void* stream) {
    SS_CHECK(images && table && table_host, "mix_batch: null pointer");
    SS_CHECK(dt == 0 || dt == 1, "mix_batch: dt must be 0 (fp32) or 1 (the selected 16-bit type), got %d", dt);
    SS_CHECK(B >= 2 && B % 2 == 0 && B < (1ll << 31), "mix_batch: the batch is mixed with its flipped self in pairs (i, B-1-i): B must be even and >= 2, got %lld",
             (long long)B);
    SS_CHECK(C >= 1 && H >= 1 && W >= 1 && C < (1ll << 31) && H < (1ll << 31) && W < (1ll << 31) && (double)C * (double)H * (double)W < 2147483648.0,
             "mix_batch: need 1 <= C*H*W < 2^31 (got %lld x %lld x %lld)", (long long)C, (long long)H, (long long)W);
    SS_CHECK(((uintptr_t)images % (dt == 0 ? 4 : 2)) == 0 && ((uintptr_t)table % 4) == 0 && ((uintptr_t)table_host % 4) == 0, "mix_batch: misaligned pointer");
    bool any = false;
    for (int64_t i = 0; i < B; ++i) {
        const int32_t* r = table_host + 8 * i;
        float lam, om;
        memcpy(&lam, r + 5, 4);
        memcpy(&om, r + 6, 4);
        SS_CHECK(r[0] >= 0 && r[0] <= 2, "mix_batch: sample %lld has kind %d (0 untouched, 1 mixup, 2 cutmix)", (long long)i, r[0]);
        SS_CHECK(0 <= r[1] && r[1] <= r[2] && r[2] <= H && 0 <= r[3] && r[3] <= r[4] && r[4] <= W,
                 "mix_batch: the box of sample %lld, rows [%d, %d) x columns [%d, %d), is not inside the %lld x %lld image", (long long)i, r[1], r[2],
                 r[3], r[4], (long long)H, (long long)W);
        SS_CHECK(lam >= 0.f && lam <= 1.f && om >= 0.f && om <= 1.f, "mix_batch: sample %lld has lam %g / 1 - lam %g outside [0, 1] (or not finite)",
                 (long long)i, (double)lam, (double)om);
        any = any || r[0] != 0;
    }
    if (!any) return 0;
    if (dt == 0) return mix_batch_launch<float>(images, table, B, C, H, W, (hipStream_t)stream);
    if (g_ss_half == 2) return mix_batch_launch<_Float16>(images, table, B, C, H, W, (hipStream_t)stream);
    return mix_batch_launch<__bf16>(images, table, B, C, H, W, (hipStream_t)stream);
}
