// Row kernels behind the similarity matrices: InfoNCE / MixUpNCE cross-entropy rows (K13), Triplet hinge rows, SigLIP pairwise-sigmoid rows, NT-Xent rows, the loss head's transposes
// and scales, retrieval first-match ranks (K16) and recall counts.  fp32 and integers only: compiled ONCE, no 16-bit flavour.
#include "common.h"

namespace {

__device__ __forceinline__ float block_reduce_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
    return s;
}
__device__ __forceinline__ float block_reduce_max(float v, float* sh) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = -INFINITY;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s = fmaxf(s, sh[i]);
    return s;
}
__device__ __forceinline__ int block_reduce_min_int(int v, int* shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = v;
    __syncthreads();
    int b = 0x7fffffff;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) b = min(b, shi[w]);
    return b;
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
    const float temp = fminf(fmaxf(temperature[0], 0.001f), 0.5f);
    const float inv_t = 1.0f / temp;
    const int il = i % N1;
    const int tgt = target0 + il;
    float mx = -INFINITY;
    int arg = 0x7fffffff;
    for (int j = tid; j < N2; j += 256) {
        const float z = row[j] * inv_t;
        if (z > mx) { mx = z; arg = j; }
    }
    const float bmx = block_reduce_max(mx, sh);
    // first index attaining the maximum
    // (block_reduce_min_int with the wave count fixed at 4: the helper's blockDim loop makes this kernel 101 instructions longer)
    int cand = (mx == bmx) ? arg : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) shi[tid >> 6] = cand;
    __syncthreads();
    int best = 0x7fffffff;
    for (int w = 0; w < 4; ++w) best = min(best, shi[w]);
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

// out[0] = loss = mean_i row_loss ; out[1] = top-1 acc over kept rows ; out[2] = dLoss/dTemperature
__global__ __launch_bounds__(256) void nce_finalize_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_correct,
                                                           const float* __restrict__ row_tdot, const float* __restrict__ ignore,
                                                           const float* __restrict__ temperature, float* __restrict__ out, int N1) {
    __shared__ float sh[8];
    float l = 0.f, c = 0.f, k = 0.f, t = 0.f;
    for (int i = threadIdx.x; i < N1; i += 256) {
        const bool keep = !ignore || ignore[i] < 1.0f;
        l += row_loss[i];
        t += row_tdot[i];
        if (keep) { c += row_correct[i]; k += 1.f; }
    }
    l = block_reduce_sum(l, sh); c = block_reduce_sum(c, sh); k = block_reduce_sum(k, sh); t = block_reduce_sum(t, sh);
    if (threadIdx.x == 0) {
        const float T = temperature[0];
        const float temp = fminf(fmaxf(T, 0.001f), 0.5f);
        out[0] = l / N1;
        out[1] = c / k;
        // z = s / temp  ->  dL/dtemp = -(1/temp) * sum_ij dz_ij * s_ij / temp ... with tdot = sum dz*s:  -tdot / temp^2
        out[2] = (T >= 0.001f && T <= 0.5f) ? -t / (temp * temp) : 0.f;
    }
}

// Both directions of the CLIP loss at once (pipelines/clip.py:129-140: 0.5 (i2t + t2i)): rows [0, N1) are the image -> text matrix, rows
// [N1, 2 N1) the text -> image one.  out = {loss, i2t acc, t2i acc, dLoss/dTemperature}.
__global__ __launch_bounds__(256) void nce_finalize_pair_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_correct,
                                                                const float* __restrict__ row_tdot, const float* __restrict__ temperature,
                                                                float* __restrict__ out, int N1) {
    __shared__ float sh[8];
    float l = 0.f, c0 = 0.f, c1 = 0.f, t = 0.f;
    for (int i = threadIdx.x; i < 2 * N1; i += 256) {
        l += row_loss[i];
        t += row_tdot[i];
        if (i < N1) c0 += row_correct[i]; else c1 += row_correct[i];
    }
    l = block_reduce_sum(l, sh); c0 = block_reduce_sum(c0, sh); c1 = block_reduce_sum(c1, sh); t = block_reduce_sum(t, sh);
    if (threadIdx.x == 0) {
        const float T = temperature[0];
        const float temp = fminf(fmaxf(T, 0.001f), 0.5f);
        out[0] = 0.5f * l / N1;
        out[1] = c0 / N1;
        out[2] = c1 / N1;
        out[3] = (T >= 0.001f && T <= 0.5f) ? -0.5f * t / (temp * temp) : 0.f;
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
    int arg = 0x7fffffff, carg = 0x7fffffff;
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
    const float bmx = block_reduce_max(mx, sh);
    const int best = block_reduce_min_int(mx == bmx ? arg : 0x7fffffff, shi);
    float loss;
    int carg_b = 0x7fffffff;
    if (reduce == 0) {
        sum = block_reduce_sum(sum, sh);
        cnt = block_reduce_sum(cnt, sh);          // (an integer below 2^24: exact)
        loss = sum / (float)(N1 - 1);
    } else {
        loss = block_reduce_max(cmx, sh);         // >= 0: the masked columns cost 0
        carg_b = block_reduce_min_int((loss > 0.f && cmx == loss) ? carg : 0x7fffffff, shi);
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

// out = {sum of the row losses, top-1 acc} (blocks = 1) or {sum over both matrices' rows, acc of matrix 0, acc of matrix 1} (blocks = 2).
// The loss is a SUM over rows, as in the reference (loss.sum()).
__global__ __launch_bounds__(256) void triplet_finalize_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_correct,
                                                               float* __restrict__ out, int N1, int blocks) {
    __shared__ float sh[8];
    float l = 0.f, c0 = 0.f, c1 = 0.f;
    for (int i = threadIdx.x; i < blocks * N1; i += 256) {
        l += row_loss[i];
        if (i < N1) c0 += row_correct[i]; else c1 += row_correct[i];
    }
    l = block_reduce_sum(l, sh); c0 = block_reduce_sum(c0, sh); c1 = block_reduce_sum(c1, sh);
    if (threadIdx.x == 0) {
        out[0] = l;
        out[1] = c0 / N1;
        if (blocks == 2) out[2] = c1 / N1;
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
    const float temp = fminf(fmaxf(temperature[0], 0.001f), 0.5f);
    const float inv_t = 1.0f / temp;
    const float b = bias[0];
    const float n1 = (float)N1;
    const int tgt = target0 + i;
    float mx = -INFINITY, loss = 0.f, tdot = 0.f, bdot = 0.f;
    int arg = 0x7fffffff;
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
    const float bmx = block_reduce_max(mx, sh);
    const int best = block_reduce_min_int(mx == bmx ? arg : 0x7fffffff, shi);
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

// out = {loss = sum_i row_loss / N1, top-1 acc = hits / N1, dLoss/dT, dLoss/db}; one block, a fixed order of additions.
// z = s / temp + b  ->  dLoss/dtemp = -sum_ij dz_ij s_ij / temp^2 (0 outside the clamp, as nce_finalize_kernel);  dLoss/db = sum_ij dz_ij.
__global__ __launch_bounds__(256) void siglip_finalize_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_correct,
                                                              const float* __restrict__ row_tdot, const float* __restrict__ row_bdot,
                                                              const float* __restrict__ temperature, float* __restrict__ out, int N1) {
    __shared__ float sh[8];
    float l = 0.f, c = 0.f, t = 0.f, d = 0.f;
    for (int i = threadIdx.x; i < N1; i += 256) {
        l += row_loss[i];
        c += row_correct[i];
        t += row_tdot[i];
        d += row_bdot[i];
    }
    l = block_reduce_sum(l, sh); c = block_reduce_sum(c, sh); t = block_reduce_sum(t, sh); d = block_reduce_sum(d, sh);
    if (threadIdx.x == 0) {
        const float T = temperature[0];
        const float temp = fminf(fmaxf(T, 0.001f), 0.5f);
        out[0] = l / N1;
        out[1] = c / N1;
        out[2] = (T >= 0.001f && T <= 0.5f) ? -t / (temp * temp) : 0.f;
        out[3] = d;
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
    const float temp = fminf(fmaxf(temperature[0], 0.001f), 0.5f);
    const float inv_t = 1.0f / temp;
    const int half = N1 >> 1;
    const int self = target0 + i;
    const int pos = target0 + (i < half ? i + half : i - half);
    float mx = -INFINITY;
    int arg = 0x7fffffff;
    for (int j = tid; j < N2; j += 256) {
        if (j == self) continue;
        const float z = row[j] * inv_t;
        if (z > mx) { mx = z; arg = j; }
    }
    const float bmx = block_reduce_max(mx, sh);       // (N2 >= N1 >= 2: at least one column is not the row's own)
    const int best = block_reduce_min_int(mx == bmx ? arg : 0x7fffffff, shi);          // first index attaining the maximum
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

// out = {loss = sum_i row_loss / N1, top-1 acc of view a's rows [0, B), of view b's rows [B, 2B), dLoss/dT}; one block, a fixed order of
// additions.  dLoss/dT as nce_finalize_kernel: -sum_i row_tdot_i / temp^2, 0 outside the clamp.
__global__ __launch_bounds__(256) void ntxent_finalize_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_correct,
                                                              const float* __restrict__ row_tdot, const float* __restrict__ temperature,
                                                              float* __restrict__ out, int N1) {
    __shared__ float sh[8];
    const int half = N1 >> 1;
    float l = 0.f, c0 = 0.f, c1 = 0.f, t = 0.f;
    for (int i = threadIdx.x; i < N1; i += 256) {
        l += row_loss[i];
        t += row_tdot[i];
        if (i < half) c0 += row_correct[i]; else c1 += row_correct[i];
    }
    l = block_reduce_sum(l, sh); c0 = block_reduce_sum(c0, sh); c1 = block_reduce_sum(c1, sh); t = block_reduce_sum(t, sh);
    if (threadIdx.x == 0) {
        const float T = temperature[0];
        const float temp = fminf(fmaxf(T, 0.001f), 0.5f);
        out[0] = l / N1;
        out[1] = c0 / half;
        out[2] = c1 / half;
        out[3] = (T >= 0.001f && T <= 0.5f) ? -t / (temp * temp) : 0.f;
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

extern "C" int simseg_nce_rows(float* sims, const float* temperature, const float* ignore_mask, float* row_loss, float* row_correct,
                               float* row_tdot, float* out3, int64_t N1, int64_t N2, int64_t target0, float smoothing,
                               int write_grad, void* stream) {
    SS_CHECK(sims && temperature && row_loss && row_correct && row_tdot && out3, "nce_rows: null pointer");
    SS_CHECK(N1 > 0 && N2 > 0 && target0 >= 0 && target0 + N1 <= N2, "nce_rows: targets [%lld, %lld) outside [0, %lld)",
             (long long)target0, (long long)(target0 + N1), (long long)N2);
    hipLaunchKernelGGL(nce_rows_kernel<false>, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, ignore_mask, row_loss, row_correct,
                       row_tdot, (int)N1, (int)N2, (int)target0, smoothing, write_grad, (const float*)nullptr, 0);
    hipLaunchKernelGGL(nce_finalize_kernel, dim3(1), dim3(256), 0, STREAM, row_loss, row_correct, row_tdot, ignore_mask, temperature,
                       out3, (int)N1);
    SS_LAUNCH_CHECK("nce_rows");
    return 0;
}

extern "C" int simseg_nce_pair(float* sims2, const float* temperature, float* row_scratch, float* out4, int64_t N1, int64_t N2, int64_t target0,
                               float smoothing, int write_grad, void* stream) {
    SS_CHECK(sims2 && temperature && row_scratch && out4, "nce_pair: null pointer");
    SS_CHECK(N1 > 0 && N2 > 0 && target0 >= 0 && target0 + N1 <= N2, "nce_pair: targets [%lld, %lld) outside [0, %lld)",
             (long long)target0, (long long)(target0 + N1), (long long)N2);
    float* rl = row_scratch; float* rc = rl + 2 * N1; float* rt = rc + 2 * N1;
    hipLaunchKernelGGL(nce_rows_kernel<false>, dim3((unsigned)(2 * N1)), dim3(256), 0, STREAM, sims2, temperature, (const float*)nullptr, rl, rc, rt, (int)N1,
                       (int)N2, (int)target0, smoothing, write_grad, (const float*)nullptr, 0);
    hipLaunchKernelGGL(nce_finalize_pair_kernel, dim3(1), dim3(256), 0, STREAM, rl, rc, rt, temperature, out4, (int)N1);
    SS_LAUNCH_CHECK("nce_pair");
    return 0;
}

extern "C" int simseg_mix_nce_rows(float* sims, const float* temperature, const float* ignore_mask, const float* alpha, int alpha_stride,
                                   float* row_loss, float* row_correct, float* row_tdot, float* out3, int64_t N1, int64_t N2,
                                   int64_t target0, float smoothing, int write_grad, void* stream) {
    SS_CHECK(sims && temperature && alpha && row_loss && row_correct && row_tdot && out3, "mix_nce_rows: null pointer");
    SS_CHECK(alpha_stride == 0 || alpha_stride == 1, "mix_nce_rows: alpha_stride %d is neither 0 (scalar) nor 1 (per row)", alpha_stride);
    SS_CHECK(N1 > 0 && N2 > 0 && target0 >= 0 && target0 + N1 <= N2, "mix_nce_rows: targets [%lld, %lld) outside [0, %lld)",
             (long long)target0, (long long)(target0 + N1), (long long)N2);
    hipLaunchKernelGGL(nce_rows_kernel<true>, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, ignore_mask, row_loss, row_correct,
                       row_tdot, (int)N1, (int)N2, (int)target0, smoothing, write_grad, alpha, alpha_stride);
    hipLaunchKernelGGL(nce_finalize_kernel, dim3(1), dim3(256), 0, STREAM, row_loss, row_correct, row_tdot, ignore_mask, temperature,
                       out3, (int)N1);
    SS_LAUNCH_CHECK("mix_nce_rows");
    return 0;
}

extern "C" int simseg_triplet_rows(float* sims, float* row_loss, float* row_correct, float* out, int64_t N1, int64_t N2, int64_t target0,
                                   float margin, int reduce, int mask_block, int blocks, int write_grad, void* stream) {
    SS_CHECK(sims && row_loss && row_correct && out, "triplet_rows: null pointer");
    SS_CHECK(blocks == 1 || blocks == 2, "triplet_rows: blocks %d is neither 1 nor 2", blocks);
    SS_CHECK(reduce == 0 || reduce == 1, "triplet_rows: reduce %d is neither 0 (mean) nor 1 (max)", reduce);
    SS_CHECK(N1 >= 1 && N2 >= 1 && target0 >= 0 && target0 + N1 <= N2, "triplet_rows: targets [%lld, %lld) outside [0, %lld)",
             (long long)target0, (long long)(target0 + N1), (long long)N2);
    SS_CHECK(!(reduce == 0 && N1 < 2), "triplet_rows: the mean over N1 - 1 negatives needs N1 >= 2");
    hipLaunchKernelGGL(triplet_rows_kernel, dim3((unsigned)(blocks * N1)), dim3(256), 0, STREAM, sims, row_loss, row_correct, (int)N1, (int)N2,
                       (int)target0, margin, reduce, mask_block ? 1 : 0, write_grad);
    hipLaunchKernelGGL(triplet_finalize_kernel, dim3(1), dim3(256), 0, STREAM, row_loss, row_correct, out, (int)N1, blocks);
    SS_LAUNCH_CHECK("triplet_rows");
    return 0;
}

extern "C" int simseg_siglip_rows(float* sims, const float* temperature, const float* bias, float* row_loss, float* row_correct,
                                  float* row_tdot, float* row_bdot, float* out4, int64_t N1, int64_t N2, int64_t target0, int write_grad,
                                  void* stream) {
    SS_CHECK(sims && temperature && bias && row_loss && row_correct && row_tdot && row_bdot && out4, "siglip_rows: null pointer");
    SS_CHECK(N1 >= 1 && N2 >= 1 && target0 >= 0 && target0 + N1 <= N2, "siglip_rows: targets [%lld, %lld) outside [0, %lld)",
             (long long)target0, (long long)(target0 + N1), (long long)N2);
    SS_CHECK(N2 <= 0x7fffffffLL, "siglip_rows: N2 = %lld columns do not fit the kernel's 32-bit indices", (long long)N2);      // (N1, target0 <= N2)
    hipLaunchKernelGGL(siglip_rows_kernel, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, bias, row_loss, row_correct, row_tdot,
                       row_bdot, (int)N1, (int)N2, (int)target0, write_grad);
    hipLaunchKernelGGL(siglip_finalize_kernel, dim3(1), dim3(256), 0, STREAM, row_loss, row_correct, row_tdot, row_bdot, temperature, out4,
                       (int)N1);
    SS_LAUNCH_CHECK("siglip_rows");
    return 0;
}

extern "C" int simseg_ntxent_rows(float* sims, const float* temperature, float* row_loss, float* row_correct, float* row_tdot, float* out4,
                                  int64_t N1, int64_t N2, int64_t target0, int write_grad, void* stream) {
    SS_CHECK(N1 >= 2, "ntxent_rows: N1 = %lld rows; two views of at least one image need N1 >= 2", (long long)N1);
    SS_CHECK(N1 % 2 == 0, "ntxent_rows: N1 = %lld is odd; the rows are view a stacked on view b, N1 = 2B", (long long)N1);
    SS_CHECK(target0 >= 0 && target0 + N1 <= N2, "ntxent_rows: own block [%lld, %lld) outside [0, %lld)", (long long)target0,
             (long long)(target0 + N1), (long long)N2);
    SS_CHECK(N2 <= 0x7fffffffLL, "ntxent_rows: N2 = %lld columns do not fit the kernel's 32-bit indices", (long long)N2);      // (N1, target0 <= N2)
    SS_CHECK(sims && temperature && row_loss && row_correct && row_tdot && out4, "ntxent_rows: null pointer");
    hipLaunchKernelGGL(ntxent_rows_kernel, dim3((unsigned)N1), dim3(256), 0, STREAM, sims, temperature, row_loss, row_correct, row_tdot,
                       (int)N1, (int)N2, (int)target0, write_grad);
    hipLaunchKernelGGL(ntxent_finalize_kernel, dim3(1), dim3(256), 0, STREAM, row_loss, row_correct, row_tdot, temperature, out4, (int)N1);
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
