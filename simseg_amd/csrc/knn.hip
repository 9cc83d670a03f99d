// Weighted k-nearest-neighbour vote over the lists of the fused search (search.hip): score / idx [M, K] -> the five best classes of every
// query row and their votes, for up to four neighbourhood sizes k from ONE launch (include/simseg_hip.h: simseg_knn_vote_rows).
//
// One wave owns a row at a time (four rows per 256-thread block, rows strided over the grid).  Lane l holds list entries l and l + 64; it
// gathers their gallery labels itself and leaves the (weight, label) pairs of the row in 1 KiB of LDS.  Every lane then walks the list
// from the front - all lanes read the same LDS word, a broadcast - and adds the weights that carry ITS entry's label, in ascending
// position: the vote of its class, in the one summation order the contract fixes.  Because the neighbourhoods are prefixes of one sorted
// list and the order is ascending, the sum for ks[i + 1] continues the sum for ks[i]: the walk is made once, with a ranking at every
// ks[i].  An entry is its class's LEADER when no earlier entry carries its label; the leaders' 64-bit keys (order-preserving bits of the
// vote, then ~label: the key of search.hip) go through five wave-wide maximum reductions, each winner leaving the pool.  Larger key =
// larger vote or, among equal votes, smaller class.  Hit counts collect in lane 0's registers over the wave's rows and reach `counts` as
// integer atomics at the end: exact, order-free.  No floating-point atomics anywhere.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int NTHR = 256, KMAX = 128, NK_MAX = 4, TOP = 5, MAX_BLOCKS = 2048;

#define SS_LDS_WAVE_SYNC()                                   \
    do {                                                     \
        __builtin_amdgcn_wave_barrier();                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
    } while (0)

struct VoteParams {
    const float* score; const int* idx; const int* glabel; const int* qlabel;
    long M, N;
    int K, nk;
    int ks[NK_MAX];
    float T;
    int* pred; float* vote; u64* counts;
};

__device__ __forceinline__ u64 vote_key(float v, int label) {        // v >= 0: the sign branch of search.hip's key is never taken
    return ((u64)(__float_as_uint(v) | 0x80000000u) << 32) | (unsigned)~(unsigned)label;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

__global__ __launch_bounds__(NTHR) void knn_vote_kernel(VoteParams p) {
    __shared__ float wts[4 * KMAX];
    __shared__ int lbl[4 * KMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* w_ = wts + wave * KMAX;
    int* l_ = lbl + wave * KMAX;
    const int K = p.K, e0 = lane, e1 = lane + 64;
    u64 hit1[NK_MAX] = {0, 0, 0, 0}, hit5[NK_MAX] = {0, 0, 0, 0}, nrows = 0;       // lane 0's; indexed by unrolled constants only

    for (long row = (long)blockIdx.x * 4 + wave; row < p.M; row += (long)gridDim.x * 4) {      // whole waves leave; nothing synchronises the block
        const float* s = p.score + row * K;
        const int* id = p.idx + row * K;
        // the valid neighbours are the entries before the first empty slot (idx < 0; an index past the gallery ends the list as well,
        // so that no label is ever read out of bounds)
        const int i0 = e0 < K ? id[e0] : -1, i1 = e1 < K ? id[e1] : -1;
        const bool ok0 = i0 >= 0 && i0 < p.N, ok1 = i1 >= 0 && i1 < p.N;
        const u64 bad0 = __ballot(!ok0), bad1 = __ballot(!ok1);
        const int valid = bad0 ? __builtin_ctzll(bad0) : (bad1 ? 64 + __builtin_ctzll(bad1) : 128);
        const float s0 = s[0];
        const int my0 = e0 < valid ? p.glabel[i0] : -1, my1 = e1 < valid ? p.glabel[i1] : -1;
        if (e0 < K) {
            w_[e0] = e0 < valid ? expf((s[e0] - s0) / p.T) : 0.f;
            l_[e0] = my0;
        }
        if (e1 < K) {
            w_[e1] = e1 < valid ? expf((s[e1] - s0) / p.T) : 0.f;
            l_[e1] = my1;
        }
        SS_LDS_WAVE_SYNC();
        const int ql = p.qlabel ? p.qlabel[row] : -1;
        float tot0 = 0.f, tot1 = 0.f;
        bool dup0 = false, dup1 = false;                      // an earlier entry carries this entry's label
        int j = 0;
#pragma unroll
        for (int ki = 0; ki < NK_MAX; ++ki) {
            if (ki >= p.nk) break;
            const int n = p.ks[ki] < valid ? p.ks[ki] : valid;
            for (; j < n; ++j) {                              // ascending j: the summation order of the contract
                const int l = l_[j];
                const float w = w_[j];
                if (l == my0) {
                    tot0 += w;
                    dup0 |= j < e0;
                }
                if (l == my1) {
                    tot1 += w;
                    dup1 |= j < e1;
                }
            }
            u64 k0 = (e0 < n && !dup0) ? vote_key(tot0, my0) : 0, k1 = (e1 < n && !dup1) ? vote_key(tot1, my1) : 0;
            bool h1 = false, h5 = false;
            const long o = ((long)ki * p.M + row) * TOP;
#pragma unroll
            for (int r = 0; r < TOP; ++r) {
                const u64 m = wave_max_u64(k0 > k1 ? k0 : k1);            // 0: no class left
                const int c = m ? (int)~(unsigned)m : -1;
                if (lane == 0) {
                    p.pred[o + r] = c;
                    p.vote[o + r] = m ? __uint_as_float((unsigned)(m >> 32) & 0x7fffffffu) : 0.f;
                }
                const bool hit = m != 0 && c == ql;
                h1 |= hit && r == 0;
                h5 |= hit;
                if (k0 == m) k0 = 0;
                if (k1 == m) k1 = 0;
            }
            hit1[ki] += h1;
            hit5[ki] += h5;
        }
        ++nrows;
        SS_LDS_WAVE_SYNC();                                   // the next row overwrites the pairs
    }
    if (p.qlabel && lane == 0 && nrows) {
#pragma unroll
        for (int ki = 0; ki < NK_MAX; ++ki) {
            if (ki >= p.nk) break;
            atomicAdd(p.counts + ki * 3, nrows);
            if (hit1[ki]) atomicAdd(p.counts + ki * 3 + 1, hit1[ki]);
            if (hit5[ki]) atomicAdd(p.counts + ki * 3 + 2, hit5[ki]);
        }
    }
}

}  // namespace

extern "C" int simseg_knn_vote_rows(const float* score, const int32_t* idx, const int32_t* gallery_label, const int32_t* query_label, int64_t M,
                                    int64_t N, int K, const int32_t* ks, int nk, float temperature, int32_t* pred, float* vote, int64_t* counts,
                                    void* stream) {
    SS_CHECK(K >= 1 && K <= KMAX, "knn_vote_rows: K = %d outside 1..128", K);
    SS_CHECK(nk >= 1 && nk <= NK_MAX, "knn_vote_rows: %d values of k (1..4 are taken)", nk);
    SS_CHECK(ks, "knn_vote_rows: null pointer (ks)");
    for (int i = 0; i < nk; ++i) {
        SS_CHECK(ks[i] >= 1 && (i == 0 || ks[i] > ks[i - 1]), "knn_vote_rows: ks must be strictly ascending and >= 1 (ks[%d] = %d)", i, ks[i]);
    }
    SS_CHECK(ks[nk - 1] <= K, "knn_vote_rows: ks[%d] = %d exceeds K = %d", nk - 1, ks[nk - 1], K);
    SS_CHECK(temperature > 0.f && temperature <= 3.4028234e38f, "knn_vote_rows: temperature %g is not a finite positive number", (double)temperature);
    SS_CHECK(M >= 0 && N >= 1, "knn_vote_rows: M = %lld, N = %lld", (long long)M, (long long)N);
    SS_CHECK(N <= 0x7fffffffLL, "knn_vote_rows: N = %lld does not fit the int32 indices", (long long)N);
    if (M == 0) return 0;
    SS_CHECK(score && idx && gallery_label && pred && vote, "knn_vote_rows: null pointer");
    SS_CHECK(!query_label || counts, "knn_vote_rows: null pointer (counts, with query_label given)");
    VoteParams p;
    p.score = score; p.idx = idx; p.glabel = gallery_label; p.qlabel = query_label; p.M = M; p.N = N; p.K = K; p.nk = nk;
    for (int i = 0; i < NK_MAX; ++i) p.ks[i] = i < nk ? ks[i] : 0;
    p.T = temperature; p.pred = pred; p.vote = vote; p.counts = reinterpret_cast<u64*>(counts);
    const long blocks = (M + 3) / 4;
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS)), dim3(NTHR), 0, (hipStream_t)stream, p);
    SS_LAUNCH_CHECK("knn_vote_rows");
    return 0;
}
