// Fused top-K retrieval search: q [M, D] against g [N, D] -> the K best gallery rows of every query, without the M x N score matrix.
//
// A block of 4 waves owns 64 query rows and streams 128-column gallery tiles through LDS (k chunks of 128 bytes, register-staged like the
// 128 x 128 GEMM of gemm.hip); wave (wr, wc) keeps the 32 x 64 score block of rows 32 wr, columns 64 wc in two 32 x 32 MFMA accumulators.
// Selection runs on the accumulators:
//   - every row has a candidate list of CAP 64-bit keys in LDS, a count and a threshold key (the row's K-th best as of its last sort);
//   - key = (order-preserving bits of the score << 32) | ~column, so a larger key is a larger score or, among equal scores, a smaller
//     column: the order of a stable descending argsort.  Keys of one row are distinct; 0 is no key of a finite score and marks "empty";
//   - a lane appends an accumulator value only when its key beats the row's threshold (slot = integer LDS add on the row's count);
//   - when a row's list is full, one wave sorts it (bitonic network over LDS), keeps K and raises the threshold; lanes that found no
//     slot append again.  Which values reach the list before a sort depends on lane timing, which values SURVIVE does not: a value is only
//     ever dropped when K larger keys are present, so the final list is the exact top K whatever the order - bit-reproducible, no floating
//     point atomics, nothing depends on the order of atomics.
// With too few row tiles to fill the chip the gallery's column tiles are split over blockIdx.y; every split writes its K keys per row to the
// workspace and topk_merge_kernel (one wave per row) reduces them - the same kernel merges two finished (score, idx) lists.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int TM = 64, TN = 128, NTHR = 256, PITCH = 144, KBYTES = 128;      // LDS row pitch: 128 B of k + 16 B pad (conflict-free b128 reads)
constexpr int OPA_BYTES = TM * PITCH, OPB_BYTES = TN * PITCH;
constexpr int MERGE_CAP = 256;

#define SS_LDS_WAVE_SYNC()                                   \
    do {                                                     \
        __builtin_amdgcn_wave_barrier();                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
    } while (0)

__device__ __forceinline__ u64 make_key(float s, unsigned col) {
    unsigned u = __float_as_uint(s + 0.0f);                  // -0.0 -> +0.0: the two compare equal in a sort of the scores
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (unsigned)~col;
}
__device__ __forceinline__ float key_score(u64 k) {
    unsigned u = (unsigned)(k >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ void emit(u64 key, long offset, float* score, int* idx) {
    *score = key ? key_score(key) : -__builtin_inff();
    *idx = key ? (int)((long)(unsigned)~(unsigned)key + offset) : -1;
}

// Descending bitonic sort of CAP keys in LDS by ONE wave (CAP a power of two >= 64).
template <int CAP>
__device__ __forceinline__ void wave_sort_desc(u64* buf, int lane) {
    for (int k = 2; k <= CAP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < CAP / 2; t += WAVE) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const u64 a = buf[i], b = buf[p];
                const bool desc = (i & k) == 0;
                if ((a < b) == desc) {
                    buf[i] = b;
                    buf[p] = a;
                }
            }
            SS_LDS_WAVE_SYNC();
        }
    }
}

// Sort a row's list, keep its K best, raise its threshold.  Called by one whole wave.
template <int CAP>
__device__ __forceinline__ void flush_row(u64* buf, int* cnt, u64* thr, int row, int K, int lane) {
    int n = __builtin_amdgcn_readfirstlane(cnt[row]);
    n = n < CAP ? n : CAP;                                   // failed appends counted past the end
    u64* b = buf + row * CAP;
    for (int t = lane; t < CAP; t += WAVE)
        if (t >= n) b[t] = 0;
    SS_LDS_WAVE_SYNC();
    wave_sort_desc<CAP>(b, lane);
    if (lane == 0) {
        cnt[row] = n < K ? n : K;
        if (n >= K) thr[row] = b[K - 1];
    }
    SS_LDS_WAVE_SYNC();
}

struct SearchParams {
    const void* q; const void* g;
    long M, N, D, ldq, ldg;
    int K, tiles_per_split;
    long ntiles;
    long index_offset;
    float* score; int* idx;
    u64* ws;                 // null: one split, results go to score / idx
};

template <typename T> struct Op;
template <> struct Op<float> { static constexpr int EPC = 4; };
template <> struct Op<__bf16> { static constexpr int EPC = 8; };

template <typename T>
__device__ __forceinline__ void mma(f32x16& acc, const u32x4& a, const u32x4& b) {
    if constexpr (sizeof(T) == 2) {
        union { u32x4 v; h16x8<__bf16> h; } ua, ub;
        ua.v = a; ub.v = b;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ua.h, ub.h, acc, 0, 0, 0);
    } else {
        union { u32x4 v; float f[4]; } ua, ub;
        ua.v = a; ub.v = b;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua.f[j], ub.f[j], acc, 0, 0, 0);
    }
}

// (two blocks per CU wanted at K <= 32, where the lists leave LDS for them: at most 256 registers, which the unrolled selection fills)
template <typename T, int CAP>
__global__ __launch_bounds__(NTHR, 2) void topk_search_kernel(SearchParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* opa = lds;
    char* opb = lds + OPA_BYTES;
    u64* thr = reinterpret_cast<u64*>(lds + OPA_BYTES + OPB_BYTES);
    int* cnt = reinterpret_cast<int*>(thr + TM);
    u64* buf = reinterpret_cast<u64*>(cnt + TM);
    constexpr int EPC = Op<T>::EPC, BK = KBYTES / (int)sizeof(T);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const long row0 = (long)blockIdx.x * TM;
    const long tile_lo = (long)blockIdx.y * p.tiles_per_split;
    long tile_hi = tile_lo + p.tiles_per_split;
    if (tile_hi > p.ntiles) tile_hi = p.ntiles;
    const int nk = (int)((p.D + BK - 1) / BK);
    const long total = (tile_hi - tile_lo) * nk;
    const T* Q = static_cast<const T*>(p.q);
    const T* G = static_cast<const T*>(p.g);

    if (tid < TM) {
        thr[tid] = 0;
        cnt[tid] = 0;
    }
    __syncthreads();

    // operand staging: a k chunk is 8 16-byte pieces per row; 64 query rows = 2 pieces per thread, 128 gallery rows = 4
    u32x4 ra[2], rb[4];
    auto fetch = [&](long tile, int kc) {
        const long k0 = (long)kc * BK;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + NTHR * i;
            const long r = row0 + (id >> 3), kk = k0 + (id & 7) * EPC;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (r < p.M && kk < p.D) v = *reinterpret_cast<const u32x4*>(Q + r * p.ldq + kk);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = tid + NTHR * i;
            const long r = tile * TN + (id >> 3), kk = k0 + (id & 7) * EPC;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (r < p.N && kk < p.D) v = *reinterpret_cast<const u32x4*>(G + r * p.ldg + kk);
            rb[i] = v;
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

    const int h2 = lane >> 5, cl = lane & 31;
    const int rl0 = wr * 32 + 4 * h2;                        // accumulator element r is tile row rl0 + (r & 3) + 8 * (r >> 2), column cl

    long tile = tile_lo;
    int kc = 0;
    if (total > 0) fetch(tile, 0);
    for (long it = 0; it < total; ++it) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + NTHR * i;
            *reinterpret_cast<u32x4*>(opa + (id >> 3) * PITCH + (id & 7) * 16) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = tid + NTHR * i;
            *reinterpret_cast<u32x4*>(opb + (id >> 3) * PITCH + (id & 7) * 16) = rb[i];
        }
        __syncthreads();
        const bool last_k = kc == nk - 1;
        if (it + 1 < total) fetch(last_k ? tile + 1 : tile, last_k ? 0 : kc + 1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int ko = (2 * kk + h2) * 16;
            const u32x4 a = *reinterpret_cast<const u32x4*>(opa + (wr * 32 + cl) * PITCH + ko);
            const u32x4 b0 = *reinterpret_cast<const u32x4*>(opb + (wc * 64 + cl) * PITCH + ko);
            const u32x4 b1 = *reinterpret_cast<const u32x4*>(opb + (wc * 64 + 32 + cl) * PITCH + ko);
            mma<T>(acc[0], a, b0);
            mma<T>(acc[1], a, b1);
        }
        if (!last_k) {
            ++kc;
            continue;
        }
        // ---- selection on the finished 64 x 128 score tile ----
        const long colbase = tile * TN + wc * 64 + cl;
        unsigned pend = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = rl0 + (r & 3) + 8 * (r >> 2);
            const u64 t = thr[rl];
            const bool rowok = row0 + rl < p.M;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const long col = colbase + 32 * a;
                if (rowok && col < p.N && make_key(acc[a][r], (unsigned)col) > t) pend |= 1u << (a * 16 + r);
            }
        }
        while (true) {
            bool fail = false;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = rl0 + (r & 3) + 8 * (r >> 2);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if (pend & (1u << (a * 16 + r))) {
                        const int slot = atomicAdd(&cnt[rl], 1);
                        if (slot < CAP) {
                            buf[rl * CAP + slot] = make_key(acc[a][r], (unsigned)(colbase + 32 * a));
                            pend &= ~(1u << (a * 16 + r));
                        } else {
                            fail = true;
                        }
                    }
                }
            }
            if (!__syncthreads_or(fail)) break;
            for (int row = wave; row < TM; row += 4)
                if (__builtin_amdgcn_readfirstlane(cnt[row]) >= CAP) flush_row<CAP>(buf, cnt, thr, row, p.K, lane);
            __syncthreads();
            if (pend) {                                      // what is still waiting meets the raised thresholds
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = rl0 + (r & 3) + 8 * (r >> 2);
                    const u64 t = thr[rl];
#pragma unroll
                    for (int a = 0; a < 2; ++a)
                        if ((pend & (1u << (a * 16 + r))) && !(make_key(acc[a][r], (unsigned)(colbase + 32 * a)) > t))
                            pend &= ~(1u << (a * 16 + r));
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
        kc = 0;
        ++tile;
    }

    __syncthreads();
    for (int row = wave; row < TM; row += 4) {
        flush_row<CAP>(buf, cnt, thr, row, p.K, lane);
        const long grow = row0 + row;
        if (grow >= p.M) continue;
        for (int j = lane; j < p.K; j += WAVE) {
            const u64 key = buf[row * CAP + j];              // slots past the row's count were zeroed and sorted to the end
            if (p.ws) p.ws[((long)blockIdx.y * p.M + grow) * p.K + j] = key;
            else emit(key, p.index_offset, p.score + grow * p.K + j, p.idx + grow * p.K + j);
        }
    }
}

// One wave per row: the K best of (a) S partial key lists ws[s][row][K] of a split search, or (b) two finished lists (score, idx).
__global__ __launch_bounds__(NTHR) void topk_merge_kernel(const u64* __restrict__ ws, long S, const float* __restrict__ sa,
                                                         const int* __restrict__ ia, const float* __restrict__ sb,
                                                         const int* __restrict__ ib, long M, int K, long offset, float* __restrict__ score,
                                                         int* __restrict__ idx) {
    __shared__ u64 lbuf[4 * MERGE_CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= M) return;                                    // whole waves leave; nothing below synchronises the block
    u64* buf = lbuf + wave * MERGE_CAP;
    if (ws) {
        const long total = S * K;
        long pos = 0;
        int have = 0;
        while (pos < total) {
            const long left = total - pos;
            const int m = (int)(left < MERGE_CAP - have ? left : MERGE_CAP - have);
            for (int t = lane; t < MERGE_CAP; t += WAVE) {
                if (t < have) continue;
                const long e = pos + (t - have);
                buf[t] = (t - have < m) ? ws[((e / K) * M + row) * K + e % K] : 0;
            }
            SS_LDS_WAVE_SYNC();
            wave_sort_desc<MERGE_CAP>(buf, lane);
            have = have + m < K ? have + m : K;
            pos += m;
        }
    } else {
        for (int t = lane; t < MERGE_CAP; t += WAVE) {
            u64 key = 0;
            if (t < 2 * K) {
                const int j = t < K ? t : t - K;
                const int id = (t < K ? ia : ib)[row * K + j];
                if (id >= 0) key = make_key((t < K ? sa : sb)[row * K + j], (unsigned)id);
            }
            buf[t] = key;
        }
        SS_LDS_WAVE_SYNC();
        wave_sort_desc<MERGE_CAP>(buf, lane);
    }
    for (int j = lane; j < K; j += WAVE) emit(buf[j], offset, score + row * K + j, idx + row * K + j);
}

// Column splits: row tiles alone fill the chip (two blocks per CU, 256 CUs) or the gallery's tiles are divided until they do.
void pick_splits(long M, long N, long* ntiles, int* tiles_per_split, long* S) {
    const long rt = (M + TM - 1) / TM, ct = (N + TN - 1) / TN;
    long s = rt >= 512 ? 1 : (512 + rt - 1) / rt;
    if (s > ct) s = ct;
    if (s > 1024) s = 1024;
    if (s < 1) s = 1;
    const long tps = (ct + s - 1) / s;
    *ntiles = ct;
    *tiles_per_split = (int)tps;
    *S = (ct + tps - 1) / tps;
}

template <int CAP> constexpr int search_smem() { return OPA_BYTES + OPB_BYTES + TM * 12 + TM * CAP * 8; }

template <typename T, int CAP>
int launch_search(const SearchParams& p, long S, hipStream_t st) {
    constexpr int SMEM = search_smem<CAP>();
    static_assert(SMEM <= 163840, "LDS budget");
    static bool attr = false;
    if (!attr) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(topk_search_kernel<T, CAP>), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
        if (e != hipSuccess) return simseg_set_error("topk_search: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr = true;
    }
    const long rt = (p.M + TM - 1) / TM;
    hipLaunchKernelGGL((topk_search_kernel<T, CAP>), dim3((unsigned)rt, (unsigned)S), dim3(NTHR), SMEM, st, p);
    SS_LAUNCH_CHECK("topk_search");
    return 0;
}

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" int64_t simseg_topk_search_workspace_bytes(int64_t M, int64_t N, int64_t D, int K, int dtype) {
    (void)D; (void)dtype;
    if (M < 1 || N < 1 || K < 1) return 0;
    long ntiles, S;
    int tps;
    pick_splits(M, N, &ntiles, &tps, &S);
    return S > 1 ? (int64_t)S * M * K * 8 : 0;
}

extern "C" int simseg_topk_search(const void* q, const void* g, int dtype, int64_t M, int64_t N, int64_t D, int64_t ldq, int64_t ldg, int K,
                                  int64_t index_offset, float* score, int32_t* idx, void* workspace, int64_t workspace_bytes, void* stream) {
    SS_CHECK(dtype == 0 || dtype == 1, "topk_search: dtype %d (0 = fp32, 1 = bf16)", dtype);
    SS_CHECK(K >= 1 && K <= 128, "topk_search: K = %d outside 1..128", K);
    SS_CHECK(M >= 0 && N >= 1, "topk_search: M = %lld, N = %lld", (long long)M, (long long)N);
    SS_CHECK(D >= 8 && D % 8 == 0, "topk_search: D = %lld is not a positive multiple of 8", (long long)D);
    const int epc = dtype == 0 ? 4 : 8;
    SS_CHECK(ldq >= D && ldg >= D && ldq % epc == 0 && ldg % epc == 0, "topk_search: leading dimensions %lld / %lld must be >= D and keep rows 16-byte aligned",
             (long long)ldq, (long long)ldg);
    SS_CHECK(index_offset >= 0 && N + index_offset <= 0x7fffffffLL, "topk_search: N + index_offset = %lld does not fit int32", (long long)(N + index_offset));
    SS_CHECK((M + TM - 1) / TM <= 0x7fffffffLL, "topk_search: M too large");
    if (M == 0) return 0;
    SS_CHECK(q && g && score && idx, "topk_search: null pointer");
    SS_CHECK(((uintptr_t)q & 15) == 0 && ((uintptr_t)g & 15) == 0, "topk_search: q and g must be 16-byte aligned");
    long ntiles, S;
    int tps;
    pick_splits(M, N, &ntiles, &tps, &S);
    const int64_t need = S > 1 ? (int64_t)S * M * K * 8 : 0;
    SS_CHECK(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
             "topk_search: workspace of %lld bytes (8-byte aligned) needed, %lld given", (long long)need, (long long)workspace_bytes);
    SearchParams p;
    p.q = q; p.g = g; p.M = M; p.N = N; p.D = D; p.ldq = ldq; p.ldg = ldg; p.K = K; p.tiles_per_split = tps; p.ntiles = ntiles;
    p.index_offset = index_offset; p.score = score; p.idx = idx; p.ws = S > 1 ? static_cast<u64*>(workspace) : nullptr;
    int rc;
    if (dtype == 0) rc = K <= 32 ? launch_search<float, 64>(p, S, STREAM) : launch_search<float, 256>(p, S, STREAM);
    else rc = K <= 32 ? launch_search<__bf16, 64>(p, S, STREAM) : launch_search<__bf16, 256>(p, S, STREAM);
    if (rc != 0) return rc;
    if (S > 1) {
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((M + 3) / 4)), dim3(NTHR), 0, STREAM, p.ws, S, nullptr, nullptr, nullptr, nullptr,
                           (long)M, K, (long)index_offset, score, idx);
        SS_LAUNCH_CHECK("topk_search (merge)");
    }
    return 0;
}

extern "C" int simseg_topk_merge(const float* score_a, const int32_t* idx_a, const float* score_b, const int32_t* idx_b, float* score, int32_t* idx,
                                 int64_t M, int K, void* stream) {
    SS_CHECK(K >= 1 && K <= 128, "topk_merge: K = %d outside 1..128", K);
    SS_CHECK(M >= 0, "topk_merge: M = %lld", (long long)M);
    if (M == 0) return 0;
    SS_CHECK(score_a && idx_a && score_b && idx_b && score && idx, "topk_merge: null pointer");
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((M + 3) / 4)), dim3(NTHR), 0, STREAM, nullptr, 0L, score_a, idx_a, score_b, idx_b,
                       (long)M, K, 0L, score, idx);
    SS_LAUNCH_CHECK("topk_merge");
    return 0;
}
