// Row kernels behind the similarity matrices: InfoNCE / MixUpNCE cross-entropy rows (K13), Triplet hinge rows, SigLIP pairwise-sigmoid rows, NT-Xent rows, the loss head's transposes
// and scales, retrieval first-match ranks (K16) and recall counts.  fp32 and integers only: compiled ONCE, no 16-bit flavour.
#include "common.h"

namespace {

// Every kernel of this file is launched with 256 threads, so a block is 4 waves: the reducers add the per-wave partials in the fixed order
// 0, wave 0, 1, 2, 3 and have no blockDim loop.
constexpr int kWaves = 4;

__device__ __forceinline__ float block_reduce_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < kWaves; ++i) s += sh[i];
    return s;
}
__device__ __forceinline__ float block_reduce_max(float v, float* sh) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = -INFINITY;
    for (int i = 0; i < kWaves; ++i) s = fmaxf(s, sh[i]);
    return s;
}
__device__ __forceinline__ int block_reduce_min_int(int v, int* shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = v;
    __syncthreads();
    int b = 0x7fffffff;
    for (int w = 0; w < kWaves; ++w) b = min(b, shi[w]);
    return b;
}
// The block's maximum of the per-thread maxima mx, and in `best` the FIRST index attaining it (arg: the thread's first index attaining mx).
__device__ __forceinline__ float block_first_argmax(float mx, int arg, float* sh, int* shi, int& best) {
    const float bmx = block_reduce_max(mx, sh);
    best = block_reduce_min_int(mx == bmx ? arg : 0x7fffffff, shi);
    return bmx;
}

// temp = clamp(T, 1e-3, 0.5), the temperature every row kernel divides by; and d/dT of a loss in z = s / temp from num = -sum dz s:
// num / temp^2 where T lies inside the clamp, 0 outside.  (Comparisons and one division each: nothing here can contract.)
__device__ __forceinline__ float clamp_temp(float T) { return fminf(fmaxf(T, 0.001f), 0.5f); }
__device__ __forceinline__ float inv_temp(float T) { return 1.0f / clamp_temp(T); }
__device__ __forceinline__ float temp_grad(float T, float num) {
    const float temp = clamp_temp(T);
    return (T >= 0.001f && T <= 0.5f) ? num / (temp * temp) : 0.f;
}

// One block per local row i of sims[N1,N2] = feat1 . feat2_global^T  (mml_loss.py:73-77, 89-95, 350-376).
//   z = s / clamp(T, 1e-3, 0.5);  loss_i = (1-eps) * nll_i + eps * mean_j(-logp_ij);  weight w_i = 1 - ignore_i
//   total loss = (1/N1) sum_i w_i loss_i.   Writes (in place) dS_ij = dLoss/ds_ij, and per-row partials.
// MIX (simseg_mix_nce_rows, mml_loss.py:146-197): row i has a second target b = target0 + (N1 - 1 - i) (targets.flip(0)) and a weight
// al = alpha[i * alpha_stride] read on the device: nll_i becomes al * nll_a + (1 - al) * nll_b and the one-hot of the gradient
// al [j == a] + (1 - al) [j == b].  A template flag, not a multiply by 1.0f: the instantiation without it is the kernel as it was, and at
// al = 1 the MIX statements reproduce its bits (products with 1 and sums with 0 are exact).
template <bool MIX>
__global__ __launch_bounds__(256) void nce_rows_kernel(float* __restrict__ sims, const float* __restrict__ temperature,
                                                       const float* __restrict__ ignore, float* __restrict__ row_loss,
                                                       float* __restrict__ row_correct, float* __restrict__ row_tdot,
                                                       int N1, int N2, int target0, float smoothing, int write_grad,
                                                       const float* __restrict__ alpha, int alpha_stride) {
    // (the pair form - simseg_nce_pair - launches 2 N1 blocks over two stacked [N1, N2] matrices: row i of matrix i / N1)
    // Every pass forms z = s * inv_t as the SAME rounded product: contracted into the subtractions below, one pass would see the exact
    // product and another the rounded one, and they would disagree about z - bmx by half an ulp of z.
#pragma clang fp contract(off)
    __shared__ float sh[8];
    __shared__ int shi[8];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* row = sims + (long)i * N2;
    const float inv_t = inv_temp(temperature[0]);
    const int il = i % N1;
    const int tgt = target0 + il;
    float mx = -INFINITY;
    int arg = 0x7fffffff, best;
    for (int j = tid; j < N2; j += 256) {
        const float z = row[j] * inv_t;
        if (z > mx) { mx = z; arg = j; }
    }
    const float bmx = block_first_argmax(mx, arg, sh, shi, best);
    float se = 0.f, sz = 0.f;
    for (int j = tid; j < N2; j += 256) {
        const float z = row[j] * inv_t;
        se += __expf(z - bmx);
        sz += z;
    }
    se = block_reduce_sum(se, sh);
    sz = block_reduce_sum(sz, sh);
    // lse = bmx + lg is never formed: where the target dominates its row (bmx = zt ~ 20, nll = lg = log(1 + 1e-5)) the rounding of that
    // sum, half an ulp of 20, is a tenth of nll and of 1 - p_target.  Differences from the maximum first, then the small logarithm.
    const float lg = __logf(se);
    const float zt = row[tgt] * inv_t;
    float nll = (bmx - zt) + lg;
    const float smooth = (bmx - sz / N2) + lg;          // -mean_j logp_ij
    const float w = ignore ? 1.0f - ignore[il] : 1.0f;
    const int tgt_b = MIX ? target0 + (N1 - 1 - il) : tgt;
    const float al = MIX ? alpha[(long)il * alpha_stride] : 1.0f;
    if (MIX) {
        const float nll_b = (bmx - row[tgt_b] * inv_t) + lg;
        nll = al * nll + (1.0f - al) * nll_b;
    }
    const float loss = (1.0f - smoothing) * nll + smoothing * smooth;
    __syncthreads();
    float tdot = 0.f;
    if (write_grad) {
        const float c = w / N1;
        for (int j = tid; j < N2; j += 256) {
            const float s = row[j];
            const float pj = __expf((s * inv_t - bmx) - lg);
            float dz = pj - smoothing / N2;
            if (MIX) {
                if (j == tgt) dz -= (1.0f - smoothing) * al;
                if (j == tgt_b) dz -= (1.0f - smoothing) * (1.0f - al);      // (a == b, the middle row of an odd N1: both land here)
            } else {
                if (j == tgt) dz -= (1.0f - smoothing);
            }
            dz *= c;
            tdot += dz * s;
            row[j] = dz * inv_t;
        }
        tdot = block_reduce_sum(tdot, sh);
    }
    if (tid == 0) {
        row_loss[i] = loss * w;
        row_correct[i] = (best == tgt) ? 1.f : 0.f;
        row_tdot[i] = tdot;
    }
}

// The one-block finalize of every row kernel above and below - what nce_finalize_kernel, nce_finalize_pair_kernel, triplet_finalize_kernel,
// siglip_finalize_kernel and ntxent_finalize_kernel were, the names in the profiles taken before - a fixed order of additions over the per-row arrays, then
//   out = {loss, top-1 acc of rows [0, split) [, of rows [split, rows) when split < rows] [, dLoss/dT when there is a row_tdot]
//          [, dLoss/db when there is a row_bdot]}
//   loss = (factor * sum_i row_loss_i) / divisor;  acc = hits / kept rows of its segment (kept: ignore_i < 1; without a mask the segment's
//   size);  dLoss/dT = temp_grad(T, -factor * sum_i row_tdot_i): z = s / temp -> -(1 / temp) sum_ij dz_ij s_ij / temp;  dLoss/db = sum_i row_bdot_i.
// Products with 1 and divisions by 1 are exact, so the entries whose loss has no factor or divisor pass 1.
struct Finalize {
    const float *row_loss, *row_correct, *row_tdot, *row_bdot, *ignore, *temperature;      // row_tdot (with temperature), row_bdot, ignore: null where absent
    float* out;
    int rows, split;
    float factor, divisor;
};
__global__ __launch_bounds__(256) void rows_finalize_kernel(Finalize F) {
    __shared__ float sh[8];
    const bool two = F.split < F.rows;
    float l = 0.f, t = 0.f, d = 0.f, c0 = 0.f, k0 = 0.f, c1 = 0.f, k1 = 0.f;
    for (int i = threadIdx.x; i < F.rows; i += 256) {
        l += F.row_loss[i];
        if (F.row_tdot) t += F.row_tdot[i];
        if (F.row_bdot) d += F.row_bdot[i];
        if (!F.ignore || F.ignore[i] < 1.0f) {
            if (i < F.split) { c0 += F.row_correct[i]; k0 += 1.f; } else { c1 += F.row_correct[i]; k1 += 1.f; }
        }
    }
    l = block_reduce_sum(l, sh); c0 = block_reduce_sum(c0, sh); k0 = block_reduce_sum(k0, sh);
    if (two) { c1 = block_reduce_sum(c1, sh); k1 = block_reduce_sum(k1, sh); }
    if (F.row_tdot) t = block_reduce_sum(t, sh);
    if (F.row_bdot) d = block_reduce_sum(d, sh);
    if (threadIdx.x == 0) {
        float* o = F.out;
        *o++ = (F.factor * l) / F.divisor;
        *o++ = c0 / k0;
        if (two) *o++ = c1 / k1;
        if (F.row_tdot) *o++ = temp_grad(F.temperature[0], -F.factor * t);
        if (F.row_bdot) *o++ = d;
    }
}

// Max-violation hinge rows of VSE++ (mml_loss.py:280-347).  One block per row of `blocks` stacked [N1, N2] matrices (row i of matrix
// i / N1), d = s[i, target0 + i]:
//   pre_j = fl32(fl32(margin + s_j) - d)   (two rounded operations in torch's order; no contraction in this kernel)
//   cost_j = max(pre_j, 0), 0 at masked columns: the own-rank block [target0, target0 + N1) with mask_block, else the target column alone
//   reduce 0: row loss = sum_j cost_j / (N1 - 1);  reduce 1: max_j cost_j, its arg the FIRST unmasked column attaining it
// and the top-1 hit over ALL columns (first index attaining the maximum, as nce_rows_kernel).  write_grad: the row becomes
// d rowloss / d s_j, gradient passing the clamp iff pre_j > 0 - mean: 1 / (N1 - 1) at unmasked j with pre_j > 0 and -count / (N1 - 1) at
// the target (each ONE rounded division); max: +1 at the arg and -1 at the target when the maximum is > 0, else a zero row.
__global__ __launch_bounds__(256) void triplet_rows_kernel(float* __restrict__ sims, float* __restrict__ row_loss,
                                                           float* __restrict__ row_correct, int N1, int N2, int target0, float margin,
                                                           int reduce, int mask_block, int write_grad) {
#pragma clang fp contract(off)
    __shared__ float sh[8];
    __shared__ int shi[8];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* row = sims + (long)i * N2;
    const int il = i % N1;
    const int tgt = target0 + il;
    const int m0 = mask_block ? target0 : tgt, m1 = mask_block ? target0 + N1 : tgt + 1;      // masked columns [m0, m1)
    const float d = row[tgt];
    float mx = -INFINITY, cmx = 0.f, sum = 0.f, cnt = 0.f;
    int arg = 0x7fffffff, carg = 0x7fffffff, best;
    for (int j = tid; j < N2; j += 256) {
        const float s = row[j];
        if (s > mx) { mx = s; arg = j; }
        const float pre = (margin + s) - d;
        if ((j < m0 || j >= m1) && pre > 0.f) {
            sum += pre;
            cnt += 1.f;
            if (pre > cmx) { cmx = pre; carg = j; }
        }
    }
    block_first_argmax(mx, arg, sh, shi, best);
    float loss;
    int carg_b = 0x7fffffff;
    if (reduce == 0) {
        sum = block_reduce_sum(sum, sh);
        cnt = block_reduce_sum(cnt, sh);          // (an integer below 2^24: exact)
        loss = sum / (float)(N1 - 1);
    } else {
        // (>= 0: the masked columns cost 0.  At 0 no thread has set its carg, and carg_b stays "no column")
        loss = block_first_argmax(cmx, carg, sh, shi, carg_b);
    }
    __syncthreads();       // (every thread holds d = row[tgt] and its pass-1 values before any thread rewrites the row)
    if (write_grad) {
        if (reduce == 0) {
            const float den = (float)(N1 - 1);
            const float g = 1.0f / den, gt = cnt > 0.f ? -cnt / den : 0.f;
            for (int j = tid; j < N2; j += 256) {
                const float pre = (margin + row[j]) - d;
                row[j] = j == tgt ? gt : ((j < m0 || j >= m1) && pre > 0.f) ? g : 0.f;
            }
        } else {
            for (int j = tid; j < N2; j += 256) row[j] = j == carg_b ? 1.f : (j == tgt && loss > 0.f) ? -1.f : 0.f;
        }
    }
    if (tid == 0) {
        row_loss[i] = loss;
        row_correct[i] = (best == tgt) ? 1.f : 0.f;
    }
}

// Pairwise sigmoid rows of SigLIP (Zhai et al., ICCV'23).  One block per local row i of sims[N1,N2], tgt = target0 + i,
// temp = clamp(T, 1e-3f, 0.5f) as nce_rows_kernel, inv_t = 1 / temp, b = bias[0]:
//   z_j = fl32(fl32(s_j * inv_t) + b);  y_j = +1 at j == tgt, else -1;  x_j = -y_j z_j;  e_j = exp(-|x_j|)
//   l_j = softplus(x_j) = max(x_j, 0) + log1p(e_j);  row loss = sum_j l_j;  loss = (1 / N1) sum_i row loss_i
//   dz_j = -y_j sigmoid(x_j) / N1, sigmoid(x) = x >= 0 ? 1 / (1 + e) : e / (1 + e) from the same e;  write_grad: row_j <- dz_j * inv_t
//   row_tdot = sum_j dz_j s_j, row_bdot = sum_j dz_j;  top-1 hit on s itself (z is increasing in s), first index attaining the maximum.
// No term depends on a row-wide quantity - there is no softmax normalisation -, so ONE pass reads s_j, scores it and overwrites it: z is
// formed once per element, as a rounded product and a rounded sum (no contraction: an fma here would make z another number than the
// one the header states).  log1p, not log(1 + e): at the default init (t = 10, b = -10) the negatives' e_j are 1e-5 .. 1e-3 and
// hundreds of them make up the row's sum beside the target's term; 1 + e_j would drop their low bits.  exp(-|x|) <= 1 and underflows to 0
// at |z| ~ 1000, where l = max(x, 0) and sigmoid = 0 or 1 exactly: nothing overflows.  The sums are computed whether or not the gradient is
// written: write_grad = 0 gives the same loss and accuracy bits and leaves the row alone.
__global__ __launch_bounds__(256) void siglip_rows_kernel(float* __restrict__ sims, const float* __restrict__ temperature,
                                                          const float* __restrict__ bias, float* __restrict__ row_loss,
                                                          float* __restrict__ row_correct, float* __restrict__ row_tdot,
                                                          float* __restrict__ row_bdot, int N1, int N2, int target0, int write_grad) {
#pragma clang fp contract(off)
    __shared__ float sh[8];
    __shared__ int shi[8];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* row = sims + (long)i * N2;
    const float inv_t = inv_temp(temperature[0]);
    const float b = bias[0];
    const float n1 = (float)N1;
    const int tgt = target0 + i;
    float mx = -INFINITY, loss = 0.f, tdot = 0.f, bdot = 0.f;
    int arg = 0x7fffffff, best;
    for (int j = tid; j < N2; j += 256) {
        const float s = row[j];
        if (s > mx) { mx = s; arg = j; }
        const float z = s * inv_t + b;
        const float x = (j == tgt) ? -z : z;
        const float e = expf(-fabsf(x));
        loss += fmaxf(x, 0.f) + log1pf(e);
        const float sig = (x >= 0.f) ? 1.0f / (1.0f + e) : e / (1.0f + e);
        // (one rounded division per element: sig * fl32(1 / N1) would lean every term of tdot and bdot the same way)
        const float dz = ((j == tgt) ? -sig : sig) / n1;
        tdot += dz * s;
        bdot += dz;
        if (write_grad) row[j] = dz * inv_t;
    }
    block_first_argmax(mx, arg, sh, shi, best);
    loss = block_reduce_sum(loss, sh);
    tdot = block_reduce_sum(tdot, sh);
    bdot = block_reduce_sum(bdot, sh);
    if (tid == 0) {
        row_loss[i] = loss;
        row_correct[i] = (best == tgt) ? 1.f : 0.f;
        row_tdot[i] = tdot;
        row_bdot[i] = bdot;
    }
}

// NT-Xent rows (SimCLR, Chen et al., ICML'20; SLIP's SIMCLRLoss): NCE over the stacked [2B, 2B W] self-similarity block.  One block per row i
// of sims[N1, N2], N1 = 2B: rows [0, B) are view a, rows [B, 2B) view b, this rank's own rows are columns [target0, target0 + N1).
//   self = target0 + i  (the row's own column, s = 1.0, always the row maximum): left out of the maximum, the sum and the top-1, gradient 0
//   pos  = target0 + (i + B) mod N1  (the other view of the same image)
//   z_j = fl32(s_j * inv_t), temp and inv_t as nce_rows_kernel;  m = max_{j != self} z_j;  lg = log(sum_{j != self} exp(z_j - m))
//   row loss = (m - z_pos) + lg  (the difference from the maximum first, for nce_rows_kernel's reason);  loss = (1 / N1) sum_i row loss
//   dz_j = (exp((z_j - m) - lg) - [j == pos]) / N1, 0 at self;  write_grad: row_j <- dz_j * inv_t;  row_tdot = sum_j dz_j s_j
// A kernel of its own, not a third flag on nce_rows_kernel: the skipped column sits in every loop, and the existing instantiations keep
// their instructions.  The self column is never loaded; with write_grad it is only stored to.
__global__ __launch_bounds__(256) void ntxent_rows_kernel(float* __restrict__ sims, const float* __restrict__ temperature,
                                                          float* __restrict__ row_loss, float* __restrict__ row_correct,
                                                          float* __restrict__ row_tdot, int N1, int N2, int target0, int write_grad) {
    // (z = s * inv_t is the SAME rounded product in every pass, see nce_rows_kernel)
#pragma clang fp contract(off)
    __shared__ float sh[8];
    __shared__ int shi[8];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* row = sims + (long)i * N2;
    const float inv_t = inv_temp(temperature[0]);
    const int half = N1 >> 1;
    const int self = target0 + i;
    const int pos = target0 + (i < half ? i + half : i - half);
    float mx = -INFINITY;
    int arg = 0x7fffffff, best;
    for (int j = tid; j < N2; j += 256) {
        if (j == self) continue;
        const float z = row[j] * inv_t;
        if (z > mx) { mx = z; arg = j; }
    }
    const float bmx = block_first_argmax(mx, arg, sh, shi, best);       // (N2 >= N1 >= 2: at least one column is not the row's own)
    float se = 0.f;
    for (int j = tid; j < N2; j += 256) {
        if (j == self) continue;
        se += __expf(row[j] * inv_t - bmx);
    }
    se = block_reduce_sum(se, sh);
    const float lg = __logf(se);
    const float loss = (bmx - row[pos] * inv_t) + lg;
    __syncthreads();       // (every thread holds z_pos before any thread rewrites the row)
    float tdot = 0.f;
    if (write_grad) {
        const float n1 = (float)N1;
        for (int j = tid; j < N2; j += 256) {
            if (j == self) { row[j] = 0.f; continue; }
            const float s = row[j];
            const float pj = __expf((s * inv_t - bmx) - lg);
            // (one rounded division per element, as siglip_rows_kernel)
            const float dz = (j == pos ? pj - 1.0f : pj) / n1;
            tdot += dz * s;
            row[j] = dz * inv_t;
        }
        tdot = block_reduce_sum(tdot, sh);
    }
    if (tid == 0) {
        row_loss[i] = loss;
        row_correct[i] = (best == pos) ? 1.f : 0.f;
        row_tdot[i] = tdot;
    }
}

// The loss head's backward preparation in ONE launch: up to six fp32 matrices are transposed (32 x 32 LDS tiles), the ones flagged `scale`
// are multiplied by alpha * scalar[0] on the way - in the transposed copy AND in place - and y0[0] = scalar[0] * x0[0].  (The fp32
// GEMM kernel contracts row . row: its transposed operands are made here, together with the upstream-gradient scale the round-3 loss head
// applied in separate passes.)
struct TransposeJob { const float* in; float* out; int R, C, scale, tiles_c, tile0; };
struct TransposeJobs { TransposeJob j[6]; int n; const float* scalar; float alpha; const float* x0; float* y0; };
__global__ __launch_bounds__(256) void transpose_multi_kernel(TransposeJobs J) {
    __shared__ float t[32][33];
    int k = 0;
    while (k + 1 < J.n && (int)blockIdx.x >= J.j[k + 1].tile0) ++k;
    const TransposeJob jb = J.j[k];
    const int tile = blockIdx.x - jb.tile0;
    const int c0 = (tile % jb.tiles_c) * 32, r0 = (tile / jb.tiles_c) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float f = jb.scale ? J.alpha * J.scalar[0] : 1.0f;
    float* inw = const_cast<float*>(jb.in);
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < jb.R && c0 + tx < jb.C) {
            const float v = jb.in[(long)(r0 + j) * jb.C + c0 + tx] * f;
            t[j][tx] = v;
            if (jb.scale) inw[(long)(r0 + j) * jb.C + c0 + tx] = v;
        }
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < jb.C && r0 + tx < jb.R) jb.out[(long)(c0 + j) * jb.R + r0 + tx] = t[tx][j];
    if (blockIdx.x == 0 && threadIdx.x == 0 && J.y0) J.y0[0] = J.scalar[0] * J.x0[0];
}

// y[r,:] = x[r,:] * (one_minus ? 1 - s[r] : s[r]) * alpha
__global__ void scale_rows_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, long rows,
                                  int D, int one_minus, float alpha) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows * D; i += (long)gridDim.x * blockDim.x) {
        const float f = s ? (one_minus ? 1.0f - s[i / D] : s[i / D]) : 1.0f;
        y[i] = x[i] * f * alpha;
    }
}

// y[i] = x[i] * scalar[0] * alpha  (upstream scalar gradient applied without a host round trip)
__global__ void scale_by_scalar_kernel(const float* __restrict__ x, const float* __restrict__ scalar, float* __restrict__ y, long n,
                                       float alpha) {
    const float f = scalar[0] * alpha;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = x[i] * f;
}

// Retrieval (hooks/utils.py:36-42, 64-66): for left row i, best = max_j{sim_ij : gid match}; rank = #{j : sim_ij > best}.
__global__ __launch_bounds__(256) void retrieval_rank_kernel(const float* __restrict__ sim, const long* __restrict__ lgid,
                                                             const long* __restrict__ rgid, int* __restrict__ has,
                                                             int* __restrict__ rank, int N, long ld) {
    __shared__ float sh[8];
    const long i = blockIdx.x;
    const float* row = sim + i * ld;
    const long g = lgid[i];
    float best = -INFINITY;
    for (int j = threadIdx.x; j < N; j += 256)
        if (rgid[j] == g) best = fmaxf(best, row[j]);
    best = block_reduce_max(best, sh);
    float cnt = 0.f;
    for (int j = threadIdx.x; j < N; j += 256) cnt += (row[j] > best) ? 1.f : 0.f;
    cnt = block_reduce_sum(cnt, sh);
    if (threadIdx.x == 0) {
        has[i] = best > -INFINITY ? 1 : 0;
        rank[i] = (int)cnt;
    }
}

// The reverse direction from the SAME similarity matrix (columns retrieve rows): for column j, best = max_i{sim_ij : gid match},
// rank = #{i : sim_ij > best}.  Two row-major passes over the matrix (thread per column, a block covers 256 columns x a band of rows;
// per-column partial results meet in one atomic per block) instead of a second M x N GEMM on swapped operands.
__device__ __forceinline__ int ord_f32(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float unord_f32(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }
__global__ __launch_bounds__(256) void retrieval_cols_init_kernel(int* __restrict__ best, int* __restrict__ rank, int N) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < N) { best[j] = ord_f32(-INFINITY); rank[j] = 0; }
}
template <int PASS>
__global__ __launch_bounds__(256) void retrieval_cols_kernel(const float* __restrict__ sim, const long* __restrict__ rgid_rows,
                                                             const long* __restrict__ cgid, int* __restrict__ best, int* __restrict__ has,
                                                             int* __restrict__ rank, int M, int N, long ld, int band) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * band, r1 = min(M, r0 + band);
    if (j >= N) return;
    const float* col = sim + j;
    if (PASS == 0) {
        const long g = cgid[j];
        float b = -INFINITY;
        for (int r = r0; r < r1; ++r)
            if (rgid_rows[r] == g) b = fmaxf(b, col[(long)r * ld]);
        if (b > -INFINITY) atomicMax(best + j, ord_f32(b));
    } else {
        const float b = unord_f32(best[j]);
        int cnt = 0;
        for (int r = r0; r < r1; ++r) cnt += col[(long)r * ld] > b ? 1 : 0;
        if (cnt) atomicAdd(rank + j, cnt);
        if (blockIdx.y == 0) has[j] = b > -INFINITY ? 1 : 0;
    }
}

// counts[0] = #rows with a match, counts[1..nb] = #rows with a match and rank < bound_b
__global__ __launch_bounds__(256) void recall_count_kernel(const int* __restrict__ has, const int* __restrict__ rank, long M,
                                                           int b0, int b1, int b2, int* __restrict__ counts) {
    int c[4] = {0, 0, 0, 0};
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (long)gridDim.x * blockDim.x) {
        if (has[i]) {
            c[0]++;
            c[1] += rank[i] < b0; c[2] += rank[i] < b1; c[3] += rank[i] < b2;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int v = c[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(counts + k, v);
    }
}

}  // namespace

#define STREAM ((hipStream_t)stream)

// The argument check the six row entries share: the own columns [target0, target0 + N1) lie inside the N2 columns of a non-empty block.
// `what` is the entry's word for those columns in its message.
#define SS_CHECK_OWN_COLUMNS(who, what)                                                                                   \
    SS_CHECK(N1 >= 1 && N2 >= 1 && target0 >= 0 && target0 + N1 <= N2, who ": " what " [%lld, %lld) outside [0, %lld)", \
             (long long)target0, (long long)(target0 + N1), (long long)N2)

static void launch_finalize(const Finalize& F, void* stream) {
    hipLaunchKernelGGL(rows_finalize_kernel, dim3(1), dim3(256), 0, STREAM, F);
}

extern "C" int simseg_nce_rows(float* sims, const float* temperature, const float* ignore_mask, float* row_loss, float* row_correct,
                               float* row_tdot, float* out3, int64_t N1, int64_t N2, int64_t target0, float smoothing,
                               int write_grad, void* stream) {
    SS_CHECK(sims && temperature && row_loss && row_correct && row_tdot && out3, "nce_rows: null pointer");
    SS_CHECK_OWN_COLUMNS("nce_rows", "targets");
    hipLaunchKernelGGL(nce_rows_kernel<false>, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, ignore_mask, row_loss, row_correct,
                       row_tdot, (int)N1, (int)N2, (int)target0, smoothing, write_grad, (const float*)nullptr, 0);
    launch_finalize({row_loss, row_correct, row_tdot, nullptr, ignore_mask, temperature, out3, (int)N1, (int)N1, 1.f, (float)N1}, stream);
    SS_LAUNCH_CHECK("nce_rows");
    return 0;
}

// Both directions of the CLIP loss at once (pipelines/clip.py:129-140: 0.5 (i2t + t2i)): rows [0, N1) are the image -> text matrix, rows
// [N1, 2 N1) the text -> image one.
extern "C" int simseg_nce_pair(float* sims2, const float* temperature, float* row_scratch, float* out4, int64_t N1, int64_t N2, int64_t target0,
                               float smoothing, int write_grad, void* stream) {
    SS_CHECK(sims2 && temperature && row_scratch && out4, "nce_pair: null pointer");
    SS_CHECK_OWN_COLUMNS("nce_pair", "targets");
    float* rl = row_scratch; float* rc = rl + 2 * N1; float* rt = rc + 2 * N1;
    hipLaunchKernelGGL(nce_rows_kernel<false>, dim3((unsigned)(2 * N1)), dim3(256), 0, STREAM, sims2, temperature, (const float*)nullptr, rl, rc, rt, (int)N1,
                       (int)N2, (int)target0, smoothing, write_grad, (const float*)nullptr, 0);
    launch_finalize({rl, rc, rt, nullptr, nullptr, temperature, out4, 2 * (int)N1, (int)N1, 0.5f, (float)N1}, stream);
    SS_LAUNCH_CHECK("nce_pair");
    return 0;
}

extern "C" int simseg_mix_nce_rows(float* sims, const float* temperature, const float* ignore_mask, const float* alpha, int alpha_stride,
                                   float* row_loss, float* row_correct, float* row_tdot, float* out3, int64_t N1, int64_t N2,
                                   int64_t target0, float smoothing, int write_grad, void* stream) {
    SS_CHECK(sims && temperature && alpha && row_loss && row_correct && row_tdot && out3, "mix_nce_rows: null pointer");
    SS_CHECK(alpha_stride == 0 || alpha_stride == 1, "mix_nce_rows: alpha_stride %d is neither 0 (scalar) nor 1 (per row)", alpha_stride);
    SS_CHECK_OWN_COLUMNS("mix_nce_rows", "targets");
    hipLaunchKernelGGL(nce_rows_kernel<true>, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, ignore_mask, row_loss, row_correct,
                       row_tdot, (int)N1, (int)N2, (int)target0, smoothing, write_grad, alpha, alpha_stride);
    launch_finalize({row_loss, row_correct, row_tdot, nullptr, ignore_mask, temperature, out3, (int)N1, (int)N1, 1.f, (float)N1}, stream);
    SS_LAUNCH_CHECK("mix_nce_rows");
    return 0;
}

// The loss is a SUM over rows, as in the reference (loss.sum()): no divisor.  blocks = 2: the second accuracy is the second matrix's.
extern "C" int simseg_triplet_rows(float* sims, float* row_loss, float* row_correct, float* out, int64_t N1, int64_t N2, int64_t target0,
                                   float margin, int reduce, int mask_block, int blocks, int write_grad, void* stream) {
    SS_CHECK(sims && row_loss && row_correct && out, "triplet_rows: null pointer");
    SS_CHECK(blocks == 1 || blocks == 2, "triplet_rows: blocks %d is neither 1 nor 2", blocks);
    SS_CHECK(reduce == 0 || reduce == 1, "triplet_rows: reduce %d is neither 0 (mean) nor 1 (max)", reduce);
    SS_CHECK_OWN_COLUMNS("triplet_rows", "targets");
    SS_CHECK(!(reduce == 0 && N1 < 2), "triplet_rows: the mean over N1 - 1 negatives needs N1 >= 2");
    hipLaunchKernelGGL(triplet_rows_kernel, dim3((unsigned)(blocks * N1)), dim3(256), 0, STREAM, sims, row_loss, row_correct, (int)N1, (int)N2,
                       (int)target0, margin, reduce, mask_block ? 1 : 0, write_grad);
    launch_finalize({row_loss, row_correct, nullptr, nullptr, nullptr, nullptr, out, blocks * (int)N1, (int)N1, 1.f, 1.f}, stream);
    SS_LAUNCH_CHECK("triplet_rows");
    return 0;
}

extern "C" int simseg_siglip_rows(float* sims, const float* temperature, const float* bias, float* row_loss, float* row_correct,
                                  float* row_tdot, float* row_bdot, float* out4, int64_t N1, int64_t N2, int64_t target0, int write_grad,
                                  void* stream) {
    SS_CHECK(sims && temperature && bias && row_loss && row_correct && row_tdot && row_bdot && out4, "siglip_rows: null pointer");
    SS_CHECK_OWN_COLUMNS("siglip_rows", "targets");
    SS_CHECK(N2 <= 0x7fffffffLL, "siglip_rows: N2 = %lld columns do not fit the kernel's 32-bit indices", (long long)N2);      // (N1, target0 <= N2)
    hipLaunchKernelGGL(siglip_rows_kernel, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, bias, row_loss, row_correct, row_tdot,
                       row_bdot, (int)N1, (int)N2, (int)target0, write_grad);
    launch_finalize({row_loss, row_correct, row_tdot, row_bdot, nullptr, temperature, out4, (int)N1, (int)N1, 1.f, (float)N1}, stream);
    SS_LAUNCH_CHECK("siglip_rows");
    return 0;
}

// The two accuracies are view a's rows [0, B) and view b's rows [B, 2B).
extern "C" int simseg_ntxent_rows(float* sims, const float* temperature, float* row_loss, float* row_correct, float* row_tdot, float* out4,
                                  int64_t N1, int64_t N2, int64_t target0, int write_grad, void* stream) {
    SS_CHECK(N1 >= 2, "ntxent_rows: N1 = %lld rows; two views of at least one image need N1 >= 2", (long long)N1);
    SS_CHECK(N1 % 2 == 0, "ntxent_rows: N1 = %lld is odd; the rows are view a stacked on view b, N1 = 2B", (long long)N1);
    SS_CHECK_OWN_COLUMNS("ntxent_rows", "own block");
    SS_CHECK(N2 <= 0x7fffffffLL, "ntxent_rows: N2 = %lld columns do not fit the kernel's 32-bit indices", (long long)N2);      // (N1, target0 <= N2)
    SS_CHECK(sims && temperature && row_loss && row_correct && row_tdot && out4, "ntxent_rows: null pointer");
    hipLaunchKernelGGL(ntxent_rows_kernel, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, row_loss, row_correct, row_tdot,
                       (int)N1, (int)N2, (int)target0, write_grad);
    launch_finalize({row_loss, row_correct, row_tdot, nullptr, nullptr, temperature, out4, (int)N1, (int)N1 / 2, 1.f, (float)N1}, stream);
    SS_LAUNCH_CHECK("ntxent_rows");
    return 0;
}

extern "C" int simseg_transpose_multi(const void* const* in, void* const* out, const int64_t* rows, const int64_t* cols, const int32_t* scale,
                                      int64_t n, const float* scalar, float alpha, const float* x0, float* y0, void* stream) {
    SS_CHECK(in && out && rows && cols && scale && n >= 1 && n <= 6, "transpose_multi: 1..6 jobs");
    TransposeJobs J;
    memset(&J, 0, sizeof(J));
    int tile0 = 0, any = 0;
    for (int k = 0; k < (int)n; ++k) {
        SS_CHECK(in[k] && out[k] && rows[k] > 0 && cols[k] > 0, "transpose_multi: job %d is empty", k);
        TransposeJob& j = J.j[k];
        j.in = (const float*)in[k]; j.out = (float*)out[k]; j.R = (int)rows[k]; j.C = (int)cols[k]; j.scale = scale[k];
        j.tiles_c = (j.C + 31) / 32; j.tile0 = tile0;
        tile0 += j.tiles_c * ((j.R + 31) / 32);
        any |= scale[k];
    }
    SS_CHECK(!(any || y0) || scalar, "transpose_multi: a scaled job needs the scalar");
    SS_CHECK(!y0 || x0, "transpose_multi: y0 needs x0");
    J.n = (int)n; J.scalar = scalar; J.alpha = alpha; J.x0 = x0; J.y0 = y0;
    hipLaunchKernelGGL(transpose_multi_kernel, dim3((unsigned)tile0), dim3(256), 0, STREAM, J);
    SS_LAUNCH_CHECK("transpose_multi");
    return 0;
}

extern "C" int simseg_scale_rows(const float* x, const float* s, float* y, int64_t rows, int64_t D, int one_minus, float alpha,
                                 void* stream) {
    SS_CHECK(x && y, "scale_rows: null pointer");
    if (rows * D <= 0) return 0;
    long blocks = (rows * D + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, STREAM, x, s, y, (long)rows, (int)D, one_minus, alpha);
    SS_LAUNCH_CHECK("scale_rows");
    return 0;
}

extern "C" int simseg_scale_by_scalar(const float* x, const float* scalar, float* y, int64_t n, float alpha, void* stream) {
    SS_CHECK(x && scalar && y, "scale_by_scalar: null pointer");
    if (n <= 0) return 0;
    long blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(scale_by_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, STREAM, x, scalar, y, (long)n, alpha);
    SS_LAUNCH_CHECK("scale_by_scalar");
    return 0;
}

extern "C" int simseg_retrieval_rank(const float* sim, const int64_t* left_gid, const int64_t* right_gid, int32_t* has_match,
                                     int32_t* rank, int64_t M, int64_t N, int64_t ld, void* stream) {
    SS_CHECK(sim && left_gid && right_gid && has_match && rank, "retrieval_rank: null pointer");
    if (M <= 0) return 0;
    hipLaunchKernelGGL(retrieval_rank_kernel, dim3((unsigned)M), dim3(256), 0, STREAM, sim, (const long*)left_gid, (const long*)right_gid,
                       has_match, rank, (int)N, (long)ld);
    SS_LAUNCH_CHECK("retrieval_rank");
    return 0;
}

extern "C" int simseg_retrieval_rank_cols(const float* sim, const int64_t* row_gid, const int64_t* col_gid, int32_t* has_match,
                                          int32_t* rank, int32_t* scratch, int64_t M, int64_t N, int64_t ld, void* stream) {
    SS_CHECK(sim && row_gid && col_gid && has_match && rank && scratch, "retrieval_rank_cols: null pointer");
    if (N <= 0 || M <= 0) return 0;
    const int band = 128;
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)((M + band - 1) / band));
    hipLaunchKernelGGL(retrieval_cols_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, STREAM, scratch, rank, (int)N);
    hipLaunchKernelGGL(retrieval_cols_kernel<0>, grid, dim3(256), 0, STREAM, sim, (const long*)row_gid, (const long*)col_gid, scratch, has_match, rank,
                       (int)M, (int)N, (long)ld, band);
    hipLaunchKernelGGL(retrieval_cols_kernel<1>, grid, dim3(256), 0, STREAM, sim, (const long*)row_gid, (const long*)col_gid, scratch, has_match, rank,
                       (int)M, (int)N, (long)ld, band);
    SS_LAUNCH_CHECK("retrieval_rank_cols");
    return 0;
}

extern "C" int simseg_recall_counts(const int32_t* has_match, const int32_t* rank, int64_t M, int b0, int b1, int b2,
                                    int32_t* counts4, void* stream) {
    SS_CHECK(has_match && rank && counts4, "recall_counts: null pointer");
    (void)hipMemsetAsync(counts4, 0, 4 * sizeof(int), STREAM);
    long blocks = (M + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(recall_count_kernel, dim3((unsigned)blocks), dim3(256), 0, STREAM, has_match, rank, (long)M, b0, b1, b2, counts4);
    SS_LAUNCH_CHECK("recall_counts");
    return 0;
}
