// Patch dropout of the ViT image tower (timm's PatchDropout, ordered, one prefix token; FLIP, Li et al. CVPR'23): in training every image
// keeps a random K of its N patch tokens and the tower runs on [cls] + the kept ones.  Four small kernels around the existing GEMM - the
// on-device draw, the im2col of the kept patches, the rest of the token embedding, and the gradient of the position table.  Compiled ONCE:
// the 16-bit flavour (bf16 / fp16) is a template argument chosen from the calling thread's simseg_set_half_type, as in mixup.hip.
//
// Every index a kernel reads from device memory (keep, inv) is range-checked before it becomes an address: a table that did not come from
// the sampler can give wrong rows, never an access outside the tensors.
#include "common.h"

namespace {

constexpr int PD_MAX_N = 4096;          // keys of one image in LDS: 16 KiB
constexpr int PD_BLOCK = 256;

// VW consecutive elements moved as one access
template <typename T, int VW>
struct alignas(sizeof(T) * VW) Pack { T v[VW]; };

// Exclusive prefix count of `flag` over the block's threads in thread order, and the block's total.  wsum: PD_BLOCK / 64 ints of LDS;
// the caller keeps a __syncthreads() between two calls that share wsum (the one at the top of this function serves that).
__device__ __forceinline__ int block_prefix_count(bool flag, int* wsum, int& total) {
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < PD_BLOCK / 64; ++i) {
        const int c = wsum[i];
        before += i < w ? c : 0;
        all += c;
    }
    total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// ---- 1. the draw: one block per image ---------------------------------------------------------------------------------------------
// key(b, n) = hash_u32(seed, b * N + n); a position is kept iff fewer than K positions of its image order before it ((key, n)
// lexicographic); its slot is the number of kept positions below it.  N^2 / 256 LDS reads per thread (broadcast: every lane of a wave
// reads the same four keys), 150 at N = 196.
__global__ __launch_bounds__(PD_BLOCK) void keep_sample_kernel(int* __restrict__ keep, int* __restrict__ inv, int N, int K, uint64_t seed) {
    __shared__ __attribute__((aligned(16))) uint32_t keys[PD_MAX_N];
    __shared__ int wsum[PD_BLOCK / 64];
    const int b = blockIdx.x;
    const uint64_t base = (uint64_t)b * (uint64_t)N;
    const int n4 = (N + 3) & ~3;
    for (int n = threadIdx.x; n < n4; n += PD_BLOCK) keys[n] = n < N ? hash_u32(seed, base + n) : 0xFFFFFFFFu;      // (the tail never orders before a real position: m < N below)
    __syncthreads();
    int kept_below = 0;                 // kept positions in the chunks before this one
    for (int n0 = 0; n0 < N; n0 += PD_BLOCK) {
        const int n = n0 + threadIdx.x;
        bool kept = false;
        if (n < N) {
            const uint32_t mine = keys[n];
            int rank = 0;
            for (int m = 0; m < n4; m += 4) {
                const u32x4 k4 = *reinterpret_cast<const u32x4*>(keys + m);
#pragma unroll
                for (int e = 0; e < 4; ++e) rank += (m + e < N && (k4[e] < mine || (k4[e] == mine && m + e < n))) ? 1 : 0;
            }
            kept = rank < K;
        }
        int total;
        const int j = kept_below + block_prefix_count(kept, wsum, total);
        if (n < N) {
            inv[base + n] = kept ? j : -1;
            if (kept) keep[(uint64_t)b * (uint64_t)K + j] = n;        // (exactly K positions have rank < K, so j < K)
        }
        kept_below += total;
    }
}

// ---- 2. im2col of the kept patches --------------------------------------------------------------------------------------------------
// One work item = 16 bytes of a cols row: 4 fp32 or 8 16-bit values, i.e. 4 / 8 consecutive pixels of one row of one channel of one patch
// (16 / 32 bytes of the image, contiguous and 16-byte aligned).  Consecutive lanes write consecutive 16-byte pieces of cols.
template <typename TO>
__global__ __launch_bounds__(PD_BLOCK) void im2col_keep_kernel(const float* __restrict__ img, const int* __restrict__ keep, TO* __restrict__ cols,
                                                               long rows, int H, int W, int K) {
    constexpr int VW = 16 / sizeof(TO), CH = 768 / VW;     // elements per piece, pieces per row
    typedef Pack<TO, VW> P;
    const int gw = W >> 4, N = gw * (H >> 4);
    const long total = rows * CH;
    for (long i = (long)blockIdx.x * PD_BLOCK + threadIdx.x; i < total; i += (long)gridDim.x * PD_BLOCK) {
        const long pr = i / CH;                             // cols row b * K + j
        const int ch = (int)(i - pr * CH);
        const int e0 = ch * VW, c = e0 >> 8, kh = (e0 >> 4) & 15, kw = e0 & 15;
        const long b = pr / K;
        const int patch = keep[pr];
        P o;
        if ((unsigned)patch < (unsigned)N) {
            const int ph = patch / gw, pw = patch - ph * gw;
            const float* src = img + ((b * 3 + c) * H + ph * 16 + kh) * (long)W + pw * 16 + kw;
#pragma unroll
            for (int q = 0; q < VW / 4; ++q) {
                const float4 t = *reinterpret_cast<const float4*>(src + 4 * q);
                o.v[4 * q + 0] = (TO)t.x; o.v[4 * q + 1] = (TO)t.y; o.v[4 * q + 2] = (TO)t.z; o.v[4 * q + 3] = (TO)t.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) o.v[e] = (TO)0.f;
        }
        *reinterpret_cast<P*>(cols + pr * 768 + e0) = o;
    }
}

// ---- 3. [cls] row and position rows of the kept tokens, in place -----------------------------------------------------------------
__global__ __launch_bounds__(PD_BLOCK) void keep_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos, const int* __restrict__ keep,
                                                             float* __restrict__ x, long rows, int N, int K, int D4) {
    const long total = rows * D4;
    for (long i = (long)blockIdx.x * PD_BLOCK + threadIdx.x; i < total; i += (long)gridDim.x * PD_BLOCK) {
        const long r = i / D4;                              // row b * (1 + K) + t of x
        const int c = (int)(i - r * D4) * 4;
        const long b = r / (K + 1);
        const int t = (int)(r - b * (K + 1));
        float4* xp = reinterpret_cast<float4*>(x + r * (long)D4 * 4 + c);
        if (t == 0) {
            const float4 a = *reinterpret_cast<const float4*>(cls + c), p = *reinterpret_cast<const float4*>(pos + c);
            *xp = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
            continue;
        }
        const int n = keep[b * K + t - 1];
        if ((unsigned)n >= (unsigned)N) continue;
        const float4 p = *reinterpret_cast<const float4*>(pos + (long)(1 + n) * D4 * 4 + c);
        float4 v = *xp;
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        *xp = v;
    }
}

// ---- 4. gradient of the position table (row 0: also the gradient of [cls]) ----------------------------------------------------------
// blockIdx.x = table row; a thread owns four columns and ONE accumulator per column, which takes its terms in ascending b.  The images are
// walked in chunks of PD_BLOCK: the block reads the chunk's inv entries (one per thread), compacts the rows of dx that contribute - in
// order, by a prefix count - into LDS, and then every thread streams its columns of those rows with unconditional, unrolled loads (a
// branch per image around the load would serialise the loop on one memory latency per image).
template <typename T>
__device__ __forceinline__ void load4f(const T* p, float (&v)[4]) {
    const Pack<T, 4> t = *reinterpret_cast<const Pack<T, 4>*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)t.v[e];
}

template <typename T>
__global__ __launch_bounds__(PD_BLOCK) void keep_pos_grad_kernel(const T* __restrict__ dx, const int* __restrict__ inv, float* __restrict__ dpos,
                                                                 int B, int N, int K, int D4) {
    __shared__ unsigned rowlist[PD_BLOCK];
    __shared__ int wsum[PD_BLOCK / 64];
    const int pr = blockIdx.x;                              // 0: [cls]; 1 + n: position n
    const int c4 = blockIdx.y * PD_BLOCK + threadIdx.x;
    const bool active = c4 < D4;
    const long ld = (long)D4 * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += PD_BLOCK) {
        const int b = b0 + threadIdx.x;
        int j = -1;
        if (b < B) j = pr == 0 ? 0 : 1 + inv[(long)b * N + pr - 1];          // row of image b's dx that lands here (inv = -1: none)
        const bool has = b < B && j >= (pr == 0 ? 0 : 1) && j <= K;
        int cnt;
        const int slot = block_prefix_count(has, wsum, cnt);
        if (has) rowlist[slot] = (unsigned)b * (unsigned)(K + 1) + (unsigned)j;      // (B * (K + 1) <= B * N + B < 2^32)
        __syncthreads();
        if (active) {
            const T* col = dx + (long)c4 * 4;
            int i = 0;
            for (; i + 8 <= cnt; i += 8) {
                float v[8][4];
#pragma unroll
                for (int u = 0; u < 8; ++u) load4f<T>(col + (long)rowlist[i + u] * ld, v[u]);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += v[u][e];
                }
            }
            for (; i < cnt; ++i) {
                float v[4];
                load4f<T>(col + (long)rowlist[i] * ld, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += v[e];
            }
        }
        // (the next chunk's block_prefix_count starts with a __syncthreads(): rowlist is not rewritten before every thread has left the loop)
    }
    if (active) *reinterpret_cast<float4*>(dpos + (long)pr * ld + (long)c4 * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
#define PD_CHECK_BNK(name)                                                                                                              \
    SS_CHECK(N >= 1 && N <= PD_MAX_N && K >= 1 && K <= N, name ": need 1 <= K <= N <= %d (got K = %lld, N = %lld)", PD_MAX_N, (long long)K, \
             (long long)N);                                                                                                             \
    SS_CHECK(B >= 1 && B < (1ll << 31) && B * N < (1ll << 31), name ": need B >= 1 and B * N < 2^31 (got B = %lld, N = %lld)", (long long)B, (long long)N)

template <typename TO>
int im2col_keep_launch(const float* image, const int32_t* keep, void* cols, int64_t B, int64_t H, int64_t W, int64_t K, hipStream_t s) {
    const long rows = (long)(B * K);
    const int grid = grid_for(rows * (768 / (16 / (long)sizeof(TO))), PD_BLOCK, 8192);
    hipLaunchKernelGGL(im2col_keep_kernel<TO>, dim3(grid), dim3(PD_BLOCK), 0, s, image, (const int*)keep, (TO*)cols, rows, (int)H, (int)W, (int)K);
    SS_LAUNCH_CHECK("vit_im2col_keep");
    return 0;
}

template <typename T>
int keep_pos_grad_launch(const void* dx, const int32_t* inv, float* dpos, int64_t B, int64_t N, int64_t K, int64_t D, hipStream_t s) {
    const int D4 = (int)(D / 4);
    hipLaunchKernelGGL(keep_pos_grad_kernel<T>, dim3((unsigned)(N + 1), (unsigned)((D4 + PD_BLOCK - 1) / PD_BLOCK)), dim3(PD_BLOCK), 0, s, (const T*)dx,
                       (const int*)inv, dpos, (int)B, (int)N, (int)K, D4);
    SS_LAUNCH_CHECK("vit_keep_pos_grad");
    return 0;
}

}  // namespace

extern "C" int simseg_patch_keep_sample(int32_t* keep, int32_t* inv, int64_t B, int64_t N, int64_t K, uint64_t seed, void* stream) {
    SS_CHECK(keep && inv, "patch_keep_sample: null pointer");
    PD_CHECK_BNK("patch_keep_sample");
    SS_CHECK(((uintptr_t)keep % 4) == 0 && ((uintptr_t)inv % 4) == 0, "patch_keep_sample: misaligned pointer");
    hipLaunchKernelGGL(keep_sample_kernel, dim3((unsigned)B), dim3(PD_BLOCK), 0, (hipStream_t)stream, (int*)keep, (int*)inv, (int)N, (int)K, seed);
    SS_LAUNCH_CHECK("patch_keep_sample");
    return 0;
}

extern "C" int simseg_vit_im2col_keep(const float* image, const int32_t* keep, void* cols, int out_dtype, int64_t B, int64_t H, int64_t W,
                                      int64_t K, void* stream) {
    SS_CHECK(image && keep && cols, "vit_im2col_keep: null pointer");
    SS_CHECK(out_dtype == 0 || out_dtype == 1, "vit_im2col_keep: out_dtype must be 0 (fp32) or 1 (the selected 16-bit type), got %d", out_dtype);
    SS_CHECK(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 && H < (1ll << 20) && W < (1ll << 20),
             "vit_im2col_keep: H, W must be multiples of the 16x16 patch (got %lld x %lld)", (long long)H, (long long)W);
    const int64_t N = (H / 16) * (W / 16);
    PD_CHECK_BNK("vit_im2col_keep");
    SS_CHECK(((uintptr_t)image % 16) == 0 && ((uintptr_t)cols % 16) == 0 && ((uintptr_t)keep % 4) == 0, "vit_im2col_keep: image and cols must be 16-byte aligned");
    if (out_dtype == 0) return im2col_keep_launch<float>(image, keep, cols, B, H, W, K, (hipStream_t)stream);
    if (g_ss_half == 2) return im2col_keep_launch<_Float16>(image, keep, cols, B, H, W, K, (hipStream_t)stream);
    return im2col_keep_launch<__bf16>(image, keep, cols, B, H, W, K, (hipStream_t)stream);
}

extern "C" int simseg_vit_keep_rows(const float* cls, const float* pos, const int32_t* keep, float* x, int64_t B, int64_t N, int64_t K, int64_t D,
                                    void* stream) {
    SS_CHECK(cls && pos && keep && x, "vit_keep_rows: null pointer");
    PD_CHECK_BNK("vit_keep_rows");
    SS_CHECK(D >= 4 && D % 4 == 0 && D < (1ll << 20), "vit_keep_rows: D must be a positive multiple of 4 (got %lld)", (long long)D);
    SS_CHECK(((uintptr_t)cls % 16) == 0 && ((uintptr_t)pos % 16) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)keep % 4) == 0,
             "vit_keep_rows: cls, pos and x must be 16-byte aligned");
    const long rows = (long)(B * (K + 1));
    hipLaunchKernelGGL(keep_rows_kernel, dim3(grid_for(rows * (D / 4), PD_BLOCK, 8192)), dim3(PD_BLOCK), 0, (hipStream_t)stream, cls, pos, (const int*)keep, x,
                       rows, (int)N, (int)K, (int)(D / 4));
    SS_LAUNCH_CHECK("vit_keep_rows");
    return 0;
}

extern "C" int simseg_vit_keep_pos_grad(const void* dx, int dx_dtype, const int32_t* inv, float* dpos, int64_t B, int64_t N, int64_t K, int64_t D,
                                        void* stream) {
    SS_CHECK(dx && inv && dpos, "vit_keep_pos_grad: null pointer");
    SS_CHECK(dx_dtype == 0 || dx_dtype == 1, "vit_keep_pos_grad: dx_dtype must be 0 (fp32) or 1 (the selected 16-bit type), got %d", dx_dtype);
    PD_CHECK_BNK("vit_keep_pos_grad");
    SS_CHECK(D >= 4 && D % 4 == 0 && D < (1ll << 20), "vit_keep_pos_grad: D must be a positive multiple of 4 (got %lld)", (long long)D);
    SS_CHECK(((uintptr_t)dx % (dx_dtype == 0 ? 16 : 8)) == 0 && ((uintptr_t)dpos % 16) == 0 && ((uintptr_t)inv % 4) == 0,
             "vit_keep_pos_grad: dx must be aligned to four of its elements and dpos to 16 bytes");
    if (dx_dtype == 0) return keep_pos_grad_launch<float>(dx, inv, dpos, B, N, K, D, (hipStream_t)stream);
    if (g_ss_half == 2) return keep_pos_grad_launch<_Float16>(dx, inv, dpos, B, N, K, D, (hipStream_t)stream);
    return keep_pos_grad_launch<__bf16>(dx, inv, dpos, B, N, K, D, (hipStream_t)stream);
}
