// Zero-shot segmentation post-processing on the GPU: everything the reference's evaluate_benchmark does
// per image AFTER the similarity map and BEFORE / AFTER its CPU DenseCRF (tools/seg_evaluation.py:112-170):
//   K17 seg_select   : top-`top_cls_num` class scores, threshold = mean + std, first five candidates (:112-124,:127-143)
//   K18 seg_masks    : per candidate: column of the similarity map -> min-max normalise (:145-146) -> binary (unary argmax,
//                      i.e. prob > 0.5: what dense_crf(:30-54) returns with its pairwise terms switched off) -> x16 nearest (:132)
//   K19 morph7       : 7x7 dilate / erode, one iteration each, borders ignored (cv2 defaults; :153-156)
//   K20 seg_predict  : nearest resize to the label size (:158), score-weighted argmax over classes (:159,:162), and the
//                      intersect / pred / label histograms of mean_iou (simseg/utils/metrics.py:5-75) in the same pass
// All of it is byte / index work bound by HBM traffic; nothing here touches MFMA.
#include "common.h"

namespace {

constexpr int SEL_MAXC = 2048;   // classes per image handled by the selection kernel
constexpr int SEL_MAXTOP = 64;

// K17: one block per image
__global__ __launch_bounds__(256) void seg_select_kernel(const float* __restrict__ scores, int C, int topn, int ncand,
                                                         int* __restrict__ cand_idx, float* __restrict__ cand_score,
                                                         float* __restrict__ threshold) {
    __shared__ float sc[SEL_MAXC];
    __shared__ float topv[SEL_MAXTOP];
    __shared__ int topi[SEL_MAXTOP];
    __shared__ float wv[4];
    __shared__ int wi[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < C; j += 256) sc[j] = scores[(long)b * C + j];
    __syncthreads();
    for (int t = 0; t < topn; ++t) {
        float mv = -INFINITY;
        int mi = 0x7fffffff;
        for (int j = tid; j < C; j += 256) {
            const float v = sc[j];
            if (v > mv || (v == mv && j < mi)) { mv = v; mi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(mv, o, 64);
            const int oi = __shfl_xor(mi, o, 64);
            if (ov > mv || (ov == mv && oi < mi)) { mv = ov; mi = oi; }
        }
        if ((tid & 63) == 0) { wv[tid >> 6] = mv; wi[tid >> 6] = mi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (wv[w] > mv || (wv[w] == mv && wi[w] < mi)) { mv = wv[w]; mi = wi[w]; }
            topv[t] = mv; topi[t] = mi;
            if (mi < C) sc[mi] = -INFINITY;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float mean = 0.f;
        for (int t = 0; t < topn; ++t) mean += topv[t];
        mean /= (float)topn;
        float var = 0.f;
        for (int t = 0; t < topn; ++t) var += (topv[t] - mean) * (topv[t] - mean);
        var /= (float)(topn - 1);                        // torch.std(): unbiased
        const float thr = mean + sqrtf(var);
        if (threshold) threshold[b] = thr;
        for (int i = 0; i < ncand; ++i) {
            int idx = -1;
            float s = 0.f;
            if (i < topn) {
                s = topv[i];
                // `continue` on class 0 / 255, `break` below the threshold: the scores are sorted, so both reduce to a per-slot test
                if (topi[i] != 0 && topi[i] != 255 && !(s < thr)) idx = topi[i];
            }
            cand_idx[b * ncand + i] = idx;
            cand_score[b * ncand + i] = s;
        }
    }
}

// K18: one block per (candidate, image).  sim [B, N, C] fp32; prob [B, ncand, N] (optional); mask [B, ncand, 16n, 16n] bytes.
constexpr int MASK_MAXN = 4096;
__global__ __launch_bounds__(256) void seg_mask_kernel(const float* __restrict__ sim, const int* __restrict__ cand_idx, int N, int n,
                                                       int C, int ncand, float* __restrict__ prob, unsigned char* __restrict__ mask) {
    // (n = patch columns, N / n = patch rows: square for one resized image, nh x nw for a stitched sliding-window map)
    __shared__ float v[MASK_MAXN];
    __shared__ float rmin[4], rmax[4];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int idx = cand_idx[b * ncand + c];
    if (idx < 0) return;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < N; i += 256) {
        const float x = sim[((long)b * N + i) * C + idx];
        v[i] = x;
        mn = fminf(mn, x); mx = fmaxf(mx, x);
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if ((tid & 63) == 0) { rmin[tid >> 6] = mn; rmax[tid >> 6] = mx; }
    __syncthreads();
    mn = fminf(fminf(rmin[0], rmin[1]), fminf(rmin[2], rmin[3]));
    mx = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
    const float range = mx - mn;
    for (int i = tid; i < N; i += 256) {
        const float pr = (v[i] - mn) / range;            // a constant map gives 0/0 = NaN as in the reference: never > 0.5
        if (prob) prob[((long)b * ncand + c) * N + i] = pr;
        v[i] = pr > 0.5f ? 1.f : 0.f;
    }
    __syncthreads();
    // x16 nearest: every 16-byte store is one pixel row of one patch cell
    const int Hm = (N / n) * 16, Wm = n * 16;
    uint4* out = reinterpret_cast<uint4*>(mask + ((long)b * ncand + c) * Hm * Wm);
    const long segs = (long)Hm * n;
    for (long s = tid; s < segs; s += 256) {
        const int y = (int)(s / n), px = (int)(s % n);
        const unsigned w = v[(y >> 4) * n + px] != 0.f ? 0xffffffffu : 0u;
        out[s] = make_uint4(w, w, w, w);
    }
}

// K18b (round 5, BASELINE configs[3] "slide-window 512x512"): overlap-average of per-window maps on the source image's patch grid.
// win [B, wy, wx, n, n, C]: window (i, j) covers source patch rows i*step .. i*step+n-1 and columns j*step .. j*step+n-1 (512-pixel
// windows at stride 256 on 16-pixel patches: n = 32, step = 16); out [B, nh, nw, C] with nh = n + (wy-1)*step: the mean over the windows
// that cover each cell, summed in window order (i, then j) - the order the oracle's loop uses, so fp32 results agree bit for bit.
// step = 0 averages all windows cell by cell (n = 1: the mean of per-window class scores).  HBM-bound, read-once / write-once: one
// thread per output element, consecutive threads on consecutive classes (the contiguous axis of both tensors).
__global__ __launch_bounds__(256) void stitch_windows_kernel(const float* __restrict__ win, float* __restrict__ out, int B, int wy, int wx,
                                                             int n, int step, int C, int nh, int nw) {
    const long total = (long)B * nh * nw * C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        long r = e / C;
        const int x = (int)(r % nw); r /= nw;
        const int y = (int)(r % nh);
        const int b = (int)(r / nh);
        // windows covering row y: i*step <= y <= i*step + n - 1
        int i0 = 0, i1 = wy - 1, j0 = 0, j1 = wx - 1;
        if (step > 0) {
            i0 = max(0, (y - n + step) / step); i1 = min(wy - 1, y / step);
            j0 = max(0, (x - n + step) / step); j1 = min(wx - 1, x / step);
        }
        float acc = 0.f;
        int cnt = 0;
        for (int i = i0; i <= i1; ++i)
            for (int j = j0; j <= j1; ++j) {
                const int ly = y - i * step, lx = x - j * step;
                acc += win[((((long)b * wy + i) * wx + j) * n * n + (long)ly * n + lx) * C + c];
                ++cnt;
            }
        out[e] = acc / (float)cnt;
    }
}

// K19: 7x7 max (dilate) / min (erode) filter on byte images [M, H, W]; pixels outside the image never win.
constexpr int MT = 64, MR = 3, MTP = MT + 2 * MR;
__global__ __launch_bounds__(256) void morph7_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int H, int W,
                                                     int erode) {
    __shared__ unsigned char tile[MTP][MTP + 2];
    __shared__ unsigned char hrow[MTP][MT];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MT;
    const unsigned char* src = in + (long)blockIdx.z * H * W;
    unsigned char* dst = out + (long)blockIdx.z * H * W;
    const unsigned char neutral = erode ? 255 : 0;
    for (int i = tid; i < MTP * MTP; i += 256) {
        const int ty = i / MTP, tx = i % MTP;
        const int y = y0 + ty - MR, x = x0 + tx - MR;
        tile[ty][tx] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(long)y * W + x] : neutral;
    }
    __syncthreads();
    for (int i = tid; i < MTP * MT; i += 256) {
        const int ty = i / MT, tx = i % MT;
        unsigned char m = tile[ty][tx];
#pragma unroll
        for (int d = 1; d <= 2 * MR; ++d) {
            const unsigned char t = tile[ty][tx + d];
            m = erode ? (t < m ? t : m) : (t > m ? t : m);
        }
        hrow[ty][tx] = m;
    }
    __syncthreads();
    for (int i = tid; i < MT * MT; i += 256) {
        const int ty = i / MT, tx = i % MT;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        unsigned char m = hrow[ty][tx];
#pragma unroll
        for (int d = 1; d <= 2 * MR; ++d) {
            const unsigned char t = hrow[ty + d][tx];
            m = erode ? (t < m ? t : m) : (t > m ? t : m);
        }
        dst[(long)y * W + x] = m;
    }
}

// K19b: cv2.dilate followed by cv2.erode (7x7, one iteration each) in ONE pass: a 64x64 output tile needs the input with a
// halo of 6; the dilated intermediate (halo 3) lives only in LDS, and positions of it outside the image are set to 255 so
// the erosion ignores them exactly as cv2's border rule does.  `valid` (optional, one int per image) < 0 skips the image:
// slots the reference never visits (most of the five candidates of an image) cost nothing.
constexpr int CT = 64, CH = 6, CIN = CT + 2 * CH, CMID = CT + 2 * MR;
__global__ __launch_bounds__(256) void close7_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const int* __restrict__ valid,
                                                     int H, int W) {
    __shared__ unsigned char A[CIN][CIN + 4];
    __shared__ unsigned char Bh[CIN][CMID + 2];
    __shared__ unsigned char C[CMID][CMID + 2];
    __shared__ unsigned char D[CMID][CT];
    if (valid && valid[blockIdx.z] < 0) return;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * CT, y0 = blockIdx.y * CT;
    const unsigned char* src = in + (long)blockIdx.z * H * W;
    unsigned char* dst = out + (long)blockIdx.z * H * W;
    for (int i = tid; i < CIN * CIN; i += 256) {
        const int ty = i / CIN, tx = i % CIN;
        const int y = y0 + ty - CH, x = x0 + tx - CH;
        A[ty][tx] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(long)y * W + x] : 0;
    }
    __syncthreads();
    for (int i = tid; i < CIN * CMID; i += 256) {            // horizontal max: Bh[y][x] covers input columns x .. x+6
        const int ty = i / CMID, tx = i % CMID;
        unsigned char m = A[ty][tx];
#pragma unroll
        for (int d = 1; d <= 2 * MR; ++d) { const unsigned char t = A[ty][tx + d]; m = t > m ? t : m; }
        Bh[ty][tx] = m;
    }
    __syncthreads();
    for (int i = tid; i < CMID * CMID; i += 256) {           // vertical max -> dilated value at (y0 - 3 + ty, x0 - 3 + tx)
        const int ty = i / CMID, tx = i % CMID;
        unsigned char m = Bh[ty][tx];
#pragma unroll
        for (int d = 1; d <= 2 * MR; ++d) { const unsigned char t = Bh[ty + d][tx]; m = t > m ? t : m; }
        const int y = y0 - MR + ty, x = x0 - MR + tx;
        C[ty][tx] = (y >= 0 && y < H && x >= 0 && x < W) ? m : 255;
    }
    __syncthreads();
    for (int i = tid; i < CMID * CT; i += 256) {             // horizontal min
        const int ty = i / CT, tx = i % CT;
        unsigned char m = C[ty][tx];
#pragma unroll
        for (int d = 1; d <= 2 * MR; ++d) { const unsigned char t = C[ty][tx + d]; m = t < m ? t : m; }
        D[ty][tx] = m;
    }
    __syncthreads();
    for (int i = tid; i < CT * CT; i += 256) {               // vertical min -> output
        const int ty = i / CT, tx = i % CT;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        unsigned char m = D[ty][tx];
#pragma unroll
        for (int d = 1; d <= 2 * MR; ++d) { const unsigned char t = D[ty + d][tx]; m = t < m ? t : m; }
        dst[(long)y * W + x] = m;
    }
}

// K20: masks [B, ncand, Hm, Wm] -> pred [B, H, W] (optional) + hist [3, C] += (intersect, pred, label) pixel counts.
constexpr int HIST_MAXC = 1024;
__global__ __launch_bounds__(256) void seg_predict_kernel(const unsigned char* __restrict__ masks, const int* __restrict__ cand_idx,
                                                          const float* __restrict__ cand_score, const unsigned char* __restrict__ labels,
                                                          int ncand, int Hm, int Wm, int H, int W, int C, int ignore,
                                                          int* __restrict__ pred, unsigned long long* __restrict__ hist) {
    __shared__ unsigned int lh[3 * HIST_MAXC];
    __shared__ int cidx[8];
    __shared__ double cval[8];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 3 * C; i += 256) lh[i] = 0u;
    if (tid < ncand) {
        cidx[tid] = cand_idx[b * ncand + tid];
        cval[tid] = (double)cand_score[b * ncand + tid];
    }
    __syncthreads();
    const double fy = (double)Hm / (double)H, fx = (double)Wm / (double)W;      // cv2.resize INTER_NEAREST: src = floor(dst * scale)
    const long npix = (long)H * W;
    if (Hm == H && Wm == W && (npix & 3) == 0 && !pred) {
        // same-size maps (windowed evaluation), histograms only: four pixels per thread, one 32-bit load per candidate map
        const unsigned int* lab4 = reinterpret_cast<const unsigned int*>(labels + (long)b * npix);
        for (long i = (long)blockIdx.x * 256 + tid; i < (npix >> 2); i += (long)gridDim.x * 256) {
            unsigned int mk[8];
            for (int k = 0; k < ncand; ++k)
                mk[k] = cidx[k] >= 0 ? reinterpret_cast<const unsigned int*>(masks + ((long)b * ncand + k) * npix)[i] : 0u;
            const unsigned int lw = lab4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double best = 0.0;
                int bi = 0;
                for (int k = 0; k < ncand; ++k) {
                    const int ci = cidx[k];
                    if (ci < 0) continue;
                    const double val = (double)((mk[k] >> (8 * e)) & 0xffu) * cval[k];
                    if (val > best || (val == best && ci < bi)) { best = val; bi = ci; }
                }
                const int l = (int)((lw >> (8 * e)) & 0xffu);
                // label maps are spatially coherent: most waves see ONE (prediction, label) pair, which would be a 64-way
                // conflict on three LDS counters.  Lanes agreeing with the first lane are counted by one lane.
                const int key = (bi << 8) | l;
                const int k0 = __builtin_amdgcn_readfirstlane(key);
                const unsigned long long same = __ballot(key == k0);
                const bool leader = (key == k0) && (__builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u)) == 0);
                const unsigned cnt = (key == k0) ? (leader ? (unsigned)__popcll(same) : 0u) : 1u;
                if (cnt && l != ignore) {
                    atomicAdd(&lh[C + bi], cnt);
                    if (l < C) {
                        atomicAdd(&lh[2 * C + l], cnt);
                        if (l == bi) atomicAdd(&lh[l], cnt);
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < 3 * C; i += 256)
            if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
        return;
    }
    for (long i = (long)blockIdx.x * 256 + tid; i < npix; i += (long)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i % W);
        int sy = (int)floor(y * fy), sx = (int)floor(x * fx);
        sy = sy < Hm - 1 ? sy : Hm - 1; sx = sx < Wm - 1 ? sx : Wm - 1;
        // temp_pred[class] = mask * score (float64), argmax over classes = first class attaining the maximum; class 0 is
        // never a candidate and holds 0, so only strictly positive values can beat it
        double best = 0.0;
        int bi = 0;
        for (int k = 0; k < ncand; ++k) {
            const int ci = cidx[k];
            if (ci < 0) continue;
            const unsigned char m = masks[(((long)b * ncand + k) * Hm + sy) * Wm + sx];
            const double val = (double)m * cval[k];
            if (val > best || (val == best && ci < bi)) { best = val; bi = ci; }
        }
        if (pred) pred[(long)b * npix + i] = bi;
        const int l = labels[(long)b * npix + i];
        if (l != ignore) {                                                       // metrics.py:60-66
            atomicAdd(&lh[C + bi], 1u);
            if (l < C) {
                atomicAdd(&lh[2 * C + l], 1u);
                if (l == bi) atomicAdd(&lh[l], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 3 * C; i += 256)
        if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

// ---- sliding windows over images of any size (segpost.slide_windows; DESIGN.md "Sliding windows on any image size") -----------------
// Tables shared by the three kernels below (built on the host by ops.slide_plan):
//   img_tab int64 [B, SLIDE_IT]: src_off (element offset of image b in the packed fp32 [3, H, W] images), H, W, out_off (element offset of
//     image b's [ncand, H, W] planes in the stitched outputs, a multiple of 16), wstart (its first window), ny, nx (its window grid), 0
//   win_tab int64 [Nw, 3]: image, y0, x0 - an image's windows consecutive, row-major over its grid, y0 / x0 strictly increasing.
constexpr int SLIDE_IT = 8;

// K21 extract: out [Nw, 3, win, win] fp32 = the window cut from its image, zero where it runs past the bottom / right border.  One float4
// store per thread and step (win is a multiple of 16: every output row is 64-byte aligned); source rows are unaligned when x0 % 4 != 0,
// so the load is one float4 only where the four source floats are aligned and inside the row, else four scalar loads.
__global__ __launch_bounds__(256) void slide_extract_kernel(const float* __restrict__ src, const int64_t* __restrict__ img_tab,
                                                            const int64_t* __restrict__ win_tab, float* __restrict__ out, long n4, int win) {
    const int q = win >> 2;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
        const int c4 = (int)(e % q);
        long r = e / q;
        const int row = (int)(r % win); r /= win;
        const int ch = (int)(r % 3);
        const long w = r / 3;
        const int64_t* wt = win_tab + w * 3;
        const int64_t* it = img_tab + wt[0] * SLIDE_IT;
        const long H = it[1], W = it[2];
        const long y = wt[1] + row, x = wt[2] + 4 * c4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (y < H) {
            const long s = it[0] + (ch * H + y) * W + x;
            if (x + 3 < W && (s & 3) == 0) {
                v = *reinterpret_cast<const f32x4*>(src + s);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k < W) v[k] = src[s + k];
            }
        }
        *reinterpret_cast<f32x4*>(out + e * 4) = v;
    }
}

// K22 scores: out [B, C] = the fp32 sum of the image's window score rows in window order, divided once by the window count (the order
// of simseg_stitch_windows with n = 1, step = 0).  One thread per (image, class).
__global__ __launch_bounds__(256) void slide_scores_kernel(const float* __restrict__ sc, const int64_t* __restrict__ img_tab, float* __restrict__ out,
                                                           int B, int C) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * C) return;
    const int b = (int)(e / C), c = (int)(e % C);
    const int64_t* it = img_tab + (long)b * SLIDE_IT;
    const long w0 = it[4], nwin = it[5] * it[6];
    float acc = 0.f;
    for (long w = 0; w < nwin; ++w) acc += sc[(w0 + w) * C + c];
    out[e] = acc / (float)nwin;
}

// K23 stitch, pass 1: one block per (64 x 64 pixel tile, candidate slot, image); visited slots only.  Each pixel (y, x) sums sim_w[w, cell, c]
// over the windows w that cover it, in window order, cell = ((y - y0) / 16, (x - x0) / 16), and divides once by their count.  A window's
// candidate column is n*n floats at a stride of C; the tile needs at most 5 x 5 of its cells, gathered ONCE per block into LDS (chunks of
// ST_WCH windows, in window order), so every pixel reads at most ceil(win / stride)^2 LDS values.  The stitched value goes to `prob` (pass 3
// normalises it in place) and the tile's min / max to `partial`.  Thread t owns columns 4 (t % 16) .. +3 of rows t / 16 + 16 r, r < 4.
constexpr int ST_T = 64, ST_CELLS = ST_T / 16 + 1, ST_WCH = 16;
__global__ __launch_bounds__(256) void slide_stitch_kernel(const float* __restrict__ sim, const int64_t* __restrict__ img_tab,
                                                           const int64_t* __restrict__ win_tab, const int* __restrict__ cand_idx, int K, int C,
                                                           int win, int n, int tiles_max, float* __restrict__ prob, float* __restrict__ partial) {
    __shared__ float vals[ST_WCH][ST_CELLS][ST_CELLS];
    __shared__ int meta[ST_WCH][4];                // y0, x0, first cell row, first cell column
    __shared__ int range[4];                       // window rows i0..i1, columns j0..j1 touching the tile
    __shared__ float red[2][4];
    const int t = blockIdx.x, k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int idx = cand_idx[b * K + k];
    if (idx < 0) return;
    const int64_t* it = img_tab + (long)b * SLIDE_IT;
    const int H = (int)it[1], W = (int)it[2], ny = (int)it[5], nx = (int)it[6];
    const long wstart = it[4];
    const int tw = (W + ST_T - 1) / ST_T, th = (H + ST_T - 1) / ST_T;
    if (t >= tw * th) return;
    const int ty0 = (t / tw) * ST_T, tx0 = (t % tw) * ST_T;
    const int ty1 = min(ty0 + ST_T, H), tx1 = min(tx0 + ST_T, W);
    if (tid == 0) { range[0] = 0x7fffffff; range[1] = -1; range[2] = 0x7fffffff; range[3] = -1; }
    __syncthreads();
    for (int i = tid; i < ny; i += 256) {
        const int y0 = (int)win_tab[(wstart + (long)i * nx) * 3 + 1];
        if (y0 < ty1 && y0 + win > ty0) { atomicMin(&range[0], i); atomicMax(&range[1], i); }
    }
    for (int j = tid; j < nx; j += 256) {
        const int x0 = (int)win_tab[(wstart + j) * 3 + 2];
        if (x0 < tx1 && x0 + win > tx0) { atomicMin(&range[2], j); atomicMax(&range[3], j); }
    }
    __syncthreads();
    const int i0 = range[0], nj = range[3] - range[2] + 1, j0 = range[2];
    const int nwin = (range[1] - i0 + 1) * nj;
    const int lx = 4 * (tid & 15), ly = tid >> 4;
    float acc[4][4];
    int cnt[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) { acc[r][q] = 0.f; cnt[r][q] = 0; }
    const long nn = (long)n * n;
    for (int c0 = 0; c0 < nwin; c0 += ST_WCH) {
        const int m = min(ST_WCH, nwin - c0);
        if (tid < m) {
            const int wl = c0 + tid;
            const long w = wstart + (long)(i0 + wl / nj) * nx + (j0 + wl % nj);
            const int y0 = (int)win_tab[w * 3 + 1], x0 = (int)win_tab[w * 3 + 2];
            meta[tid][0] = y0; meta[tid][1] = x0;
            meta[tid][2] = max(ty0 - y0, 0) >> 4; meta[tid][3] = max(tx0 - x0, 0) >> 4;
        }
        __syncthreads();
        for (int e = tid; e < m * ST_CELLS * ST_CELLS; e += 256) {
            const int wl = e / (ST_CELLS * ST_CELLS), cy = meta[wl][2] + (e / ST_CELLS) % ST_CELLS, cx = meta[wl][3] + e % ST_CELLS;
            const long w = wstart + (long)(i0 + (c0 + wl) / nj) * nx + (j0 + (c0 + wl) % nj);
            vals[wl][(e / ST_CELLS) % ST_CELLS][e % ST_CELLS] = (cy < n && cx < n) ? sim[(w * nn + (long)cy * n + cx) * C + idx] : 0.f;
        }
        __syncthreads();
        for (int wl = 0; wl < m; ++wl) {
            const int y0 = meta[wl][0], x0 = meta[wl][1], cy0 = meta[wl][2], cx0 = meta[wl][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int dy = ty0 + ly + 16 * r - y0;
                if (dy < 0 || dy >= win) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int dx = tx0 + lx + q - x0;
                    if (dx < 0 || dx >= win) continue;
                    acc[r][q] += vals[wl][(dy >> 4) - cy0][(dx >> 4) - cx0];
                    cnt[r][q] += 1;
                }
            }
        }
        __syncthreads();
    }
    float mn = INFINITY, mx = -INFINITY;
    float* plane = prob + it[3] + (long)k * H * W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = ty0 + ly + 16 * r, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = acc[r][q] / (float)cnt[r][q];
            if (x + q < W) { mn = fminf(mn, v[q]); mx = fmaxf(mx, v[q]); }
        }
        float* dst = plane + (long)y * W + x;
        if (x + 3 < W && ((uintptr_t)dst & 15) == 0) {
            *reinterpret_cast<f32x4*>(dst) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x + q < W) dst[q] = v[q];
        }
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        float* p = partial + (((long)b * K + k) * tiles_max + t) * 2;
        p[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        p[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}

// K23 pass 2: one block per (slot, image): the min / max of the stitched map over the image's H x W pixels from the tiles' partials.
__global__ __launch_bounds__(256) void slide_minmax_kernel(const int64_t* __restrict__ img_tab, const int* __restrict__ cand_idx, int K, int tiles_max,
                                                           const float* __restrict__ partial, float* __restrict__ minmax) {
    __shared__ float red[2][4];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (cand_idx[b * K + k] < 0) return;
    const int64_t* it = img_tab + (long)b * SLIDE_IT;
    const int tiles = (int)(((it[1] + ST_T - 1) / ST_T) * ((it[2] + ST_T - 1) / ST_T));
    const float* p = partial + ((long)b * K + k) * tiles_max * 2;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < tiles; i += 256) { mn = fminf(mn, p[2 * i]); mx = fmaxf(mx, p[2 * i + 1]); }
    mn = wave_min(mn); mx = wave_max(mx);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        minmax[((long)b * K + k) * 2] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        minmax[((long)b * K + k) * 2 + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}

// K23 pass 3: prob = (S - min) / (max - min) in place (a constant map gives 0/0 = NaN, never > 0.5, as seg_mask_kernel), mask = prob > 0.5
// ? 255 : 0.  A thread takes 16 elements at a 16-aligned flat position: four float4 loads / stores and one 16-byte mask store inside the
// plane (planes start at multiples of 16 elements only per image, so a plane's first and last chunks may be partial: element by element).
__global__ __launch_bounds__(256) void slide_norm_kernel(const int64_t* __restrict__ img_tab, const int* __restrict__ cand_idx, int K,
                                                         const float* __restrict__ minmax, float* __restrict__ prob, unsigned char* __restrict__ mask) {
    const int k = blockIdx.y, b = blockIdx.z;
    if (cand_idx[b * K + k] < 0) return;
    const int64_t* it = img_tab + (long)b * SLIDE_IT;
    const long HW = it[1] * it[2];
    const long p0 = it[3] + (long)k * HW, p1 = p0 + HW;
    const float mn = minmax[((long)b * K + k) * 2], range = minmax[((long)b * K + k) * 2 + 1] - mn;
    for (long a = (p0 & ~15L) + 16 * ((long)blockIdx.x * 256 + threadIdx.x); a < p1; a += 16L * gridDim.x * 256) {
        if (a >= p0 && a + 16 <= p1) {
            unsigned int mw[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v = *reinterpret_cast<const f32x4*>(prob + a + 4 * g);
                unsigned int bits = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = (v[q] - mn) / range;
                    bits |= (v[q] > 0.5f ? 0xffu : 0u) << (8 * q);
                }
                *reinterpret_cast<f32x4*>(prob + a + 4 * g) = v;
                mw[g] = bits;
            }
            u32x4 m4 = {mw[0], mw[1], mw[2], mw[3]};
            *reinterpret_cast<u32x4*>(mask + a) = m4;
        } else {
            for (long e = max(a, p0); e < min(a + 16, p1); ++e) {
                const float pr = (prob[e] - mn) / range;
                prob[e] = pr;
                mask[e] = pr > 0.5f ? 255 : 0;
            }
        }
    }
}

// ---- multi-scale / flip test-time augmentation over sliding windows (DESIGN.md "Multi-scale and flip test-time augmentation") --------
// K21f extract from the MIRRORED image: window (image, y0, x0) column j reads source column W - 1 - (x0 + j); zero past the border of the
// mirrored image (x0 + j >= W or y0 + i >= H).  The reads of a thread run backwards, so they are four scalar loads; the store is K21's.
__global__ __launch_bounds__(256) void slide_extract_flip_kernel(const float* __restrict__ src, const int64_t* __restrict__ img_tab,
                                                                 const int64_t* __restrict__ win_tab, float* __restrict__ out, long n4, int win) {
    const int q = win >> 2;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
        const int c4 = (int)(e % q);
        long r = e / q;
        const int row = (int)(r % win); r /= win;
        const int ch = (int)(r % 3);
        const long w = r / 3;
        const int64_t* wt = win_tab + w * 3;
        const int64_t* it = img_tab + wt[0] * SLIDE_IT;
        const long H = it[1], W = it[2];
        const long y = wt[1] + row, x = wt[2] + 4 * c4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (y < H) {
            const float* line = src + it[0] + (ch * H + y) * W;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < W) v[k] = line[W - 1 - (x + k)];
        }
        *reinterpret_cast<f32x4*>(out + e * 4) = v;
    }
}

// K24 fused stitch of P passes, pass 1: one block per (64 x 64 pixel tile of the BASE image, candidate slot, image), visited slots only;
// the thread-to-pixel map and the stores are K23's.  pass_tab int64 [P, SLIDE_PT] = (sim_w pointer, img_tab pointer, win_tab pointer, flip)
// per pass.  Per pass the base pixel (y, x) samples the pass's stitched map at y_p = min(((2y + 1) H_p) / (2H), H_p - 1), x_p likewise
// (integer division), mirrored to W_p - 1 - x_p for a flipped pass; that value is K23's: the sum over the covering windows in window
// order of their cell, divided once by their count.  Only the windows touching the tile's sample rectangle are walked (their offsets
// staged in LDS, SM_WCH at a time); the cells are read from global memory - neighbouring pixels share them, so a wave's 64 loads fall on
// a handful of addresses - which puts no bound on the scale of a pass.  The pass values are summed in pass order and divided once by P.
constexpr int SLIDE_MAXP = 16, SLIDE_PT = 4, SM_WCH = 64;
__global__ __launch_bounds__(256) void slide_stitch_multi_kernel(const int64_t* __restrict__ pass_tab, int P, const int64_t* __restrict__ img_tab,
                                                                 const int* __restrict__ cand_idx, int K, int C, int win, int n, int tiles_max,
                                                                 float* __restrict__ prob, float* __restrict__ partial) {
    __shared__ int meta[SM_WCH][2];                // y0, x0
    __shared__ int range[4];                       // window rows i0..i1, columns j0..j1 touching the tile's sample rectangle
    __shared__ float red[2][4];
    const int t = blockIdx.x, k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int idx = cand_idx[b * K + k];
    if (idx < 0) return;
    const int64_t* it = img_tab + (long)b * SLIDE_IT;
    const int H = (int)it[1], W = (int)it[2];
    const int tw = (W + ST_T - 1) / ST_T, th = (H + ST_T - 1) / ST_T;
    if (t >= tw * th) return;
    const int ty0 = (t / tw) * ST_T, tx0 = (t % tw) * ST_T;
    const int ty1 = min(ty0 + ST_T, H), tx1 = min(tx0 + ST_T, W);
    const int lx = 4 * (tid & 15), ly = tid >> 4;
    const long nn = (long)n * n;
    float tot[4][4];
    for (int p = 0; p < P; ++p) {
        const float* __restrict__ sim = reinterpret_cast<const float*>(pass_tab[p * SLIDE_PT]);
        const int64_t* pit = reinterpret_cast<const int64_t*>(pass_tab[p * SLIDE_PT + 1]) + (long)b * SLIDE_IT;
        const int64_t* __restrict__ win_tab = reinterpret_cast<const int64_t*>(pass_tab[p * SLIDE_PT + 2]);
        const bool flip = pass_tab[p * SLIDE_PT + 3] != 0;
        const long Hp = pit[1], Wp = pit[2];
        const int ny = (int)pit[5], nx = (int)pit[6];
        const long wstart = pit[4];
        // this thread's sample rows / columns in the pass (pixels past the tile's border clamp into it: computed, never stored)
        int sy[4], sx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) sy[r] = (int)min(((2L * min(ty0 + ly + 16 * r, ty1 - 1) + 1) * Hp) / (2L * H), Hp - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int xp = (int)min(((2L * min(tx0 + lx + q, tx1 - 1) + 1) * Wp) / (2L * W), Wp - 1);
            sx[q] = flip ? (int)Wp - 1 - xp : xp;
        }
        // the tile's sample rectangle (inclusive): the index maps are monotone, so its corners are the tile's
        const int ry0 = (int)min(((2L * ty0 + 1) * Hp) / (2L * H), Hp - 1), ry1 = (int)min(((2L * (ty1 - 1) + 1) * Hp) / (2L * H), Hp - 1);
        const int xa = (int)min(((2L * tx0 + 1) * Wp) / (2L * W), Wp - 1), xb = (int)min(((2L * (tx1 - 1) + 1) * Wp) / (2L * W), Wp - 1);
        const int rx0 = flip ? (int)Wp - 1 - xb : xa, rx1 = flip ? (int)Wp - 1 - xa : xb;
        __syncthreads();                           // the previous pass has read range / meta
        if (tid == 0) { range[0] = 0x7fffffff; range[1] = -1; range[2] = 0x7fffffff; range[3] = -1; }
        __syncthreads();
        for (int i = tid; i < ny; i += 256) {
            const int y0 = (int)win_tab[(wstart + (long)i * nx) * 3 + 1];
            if (y0 <= ry1 && y0 + win > ry0) { atomicMin(&range[0], i); atomicMax(&range[1], i); }
        }
        for (int j = tid; j < nx; j += 256) {
            const int x0 = (int)win_tab[(wstart + j) * 3 + 2];
            if (x0 <= rx1 && x0 + win > rx0) { atomicMin(&range[2], j); atomicMax(&range[3], j); }
        }
        __syncthreads();
        const int i0 = range[0], nj = range[3] - range[2] + 1, j0 = range[2];
        const int nwin = (range[1] - i0 + 1) * nj;
        float acc[4][4];
        int cnt[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) { acc[r][q] = 0.f; cnt[r][q] = 0; }
        for (int c0 = 0; c0 < nwin; c0 += SM_WCH) {
            const int m = min(SM_WCH, nwin - c0);
            if (tid < m) {
                const int wl = c0 + tid;
                const long w = wstart + (long)(i0 + wl / nj) * nx + (j0 + wl % nj);
                meta[tid][0] = (int)win_tab[w * 3 + 1]; meta[tid][1] = (int)win_tab[w * 3 + 2];
            }
            __syncthreads();
            for (int wl = 0; wl < m; ++wl) {
                const int y0 = meta[wl][0], x0 = meta[wl][1];
                const float* col = sim + (wstart + (long)(i0 + (c0 + wl) / nj) * nx + (j0 + (c0 + wl) % nj)) * nn * C + idx;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int dy = sy[r] - y0;
                    if (dy < 0 || dy >= win) continue;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int dx = sx[q] - x0;
                        if (dx < 0 || dx >= win) continue;
                        acc[r][q] += col[(long)((dy >> 4) * n + (dx >> 4)) * C];
                        cnt[r][q] += 1;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float s = acc[r][q] / (float)cnt[r][q];
                tot[r][q] = p == 0 ? s : tot[r][q] + s;
            }
    }
    float mn = INFINITY, mx = -INFINITY;
    float* plane = prob + it[3] + (long)k * H * W;
    const float fp = (float)P;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = ty0 + ly + 16 * r, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = tot[r][q] / fp;
            if (x + q < W) { mn = fminf(mn, v[q]); mx = fmaxf(mx, v[q]); }
        }
        float* dst = plane + (long)y * W + x;
        if (x + 3 < W && ((uintptr_t)dst & 15) == 0) {
            *reinterpret_cast<f32x4*>(dst) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x + q < W) dst[q] = v[q];
        }
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        float* pp = partial + (((long)b * K + k) * tiles_max + t) * 2;
        pp[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        pp[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}

}  // namespace

extern "C" int simseg_seg_select(const float* scores, int* cand_idx, float* cand_score, float* threshold, int64_t B, int64_t C,
                                 int64_t top_cls_num, int64_t ncand, void* stream) {
    SS_CHECK(scores && cand_idx && cand_score, "seg_select: null pointer");
    SS_CHECK(B > 0 && C > 1 && C <= SEL_MAXC, "seg_select: need 1 < C <= %d", SEL_MAXC);
    SS_CHECK(ncand >= 1 && ncand <= 8, "seg_select: 1 <= ncand <= 8");
    const int topn = (int)(top_cls_num < C ? top_cls_num : C);
    SS_CHECK(topn >= 2 && topn <= SEL_MAXTOP, "seg_select: 2 <= min(top_cls_num, C) <= %d", SEL_MAXTOP);
    hipLaunchKernelGGL(seg_select_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, scores, (int)C, topn, (int)ncand, cand_idx,
                       cand_score, threshold);
    SS_LAUNCH_CHECK("seg_select");
    return 0;
}

extern "C" int simseg_seg_masks_rect(const float* sim, const int* cand_idx, float* prob, void* mask, int64_t B, int64_t nh, int64_t nw,
                                     int64_t C, int64_t ncand, void* stream) {
    SS_CHECK(sim && cand_idx && mask, "seg_masks: null pointer");
    SS_CHECK(B > 0 && nh > 0 && nw > 0 && nh * nw <= MASK_MAXN && C > 0 && ncand >= 1 && ncand <= 8, "seg_masks: bad shape (nh*nw <= %d)", MASK_MAXN);
    SS_CHECK(((uintptr_t)mask % 16) == 0, "seg_masks: mask must be 16-byte aligned");
    hipLaunchKernelGGL(seg_mask_kernel, dim3((unsigned)ncand, (unsigned)B), dim3(256), 0, (hipStream_t)stream, sim, cand_idx, (int)(nh * nw),
                       (int)nw, (int)C, (int)ncand, prob, static_cast<unsigned char*>(mask));
    SS_LAUNCH_CHECK("seg_masks");
    return 0;
}

extern "C" int simseg_seg_masks(const float* sim, const int* cand_idx, float* prob, void* mask, int64_t B, int64_t n, int64_t C,
                                int64_t ncand, void* stream) {
    return simseg_seg_masks_rect(sim, cand_idx, prob, mask, B, n, n, C, ncand, stream);
}

extern "C" int simseg_stitch_windows(const float* win, float* out, int64_t B, int64_t wy, int64_t wx, int64_t n, int64_t step, int64_t C,
                                     void* stream) {
    SS_CHECK(win && out && win != out, "stitch_windows: null or aliased pointers");
    SS_CHECK(B > 0 && wy > 0 && wx > 0 && n > 0 && step >= 0 && step <= n && C > 0, "stitch_windows: bad shape (0 <= step <= n)");
    const long nh = n + (wy - 1) * step, nw = n + (wx - 1) * step;
    const long total = (long)B * nh * nw * C;
    SS_CHECK(total < (1ll << 40), "stitch_windows: problem too large");
    long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(stitch_windows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, win, out, (int)B, (int)wy, (int)wx, (int)n,
                       (int)step, (int)C, (int)nh, (int)nw);
    SS_LAUNCH_CHECK("stitch_windows");
    return 0;
}

extern "C" int simseg_morph7(const void* in, void* out, int64_t M, int64_t H, int64_t W, int erode, void* stream) {
    SS_CHECK(in && out && in != out, "morph7: null or aliased pointers");
    SS_CHECK(M > 0 && M < 65536 && H > 0 && W > 0, "morph7: bad shape");
    dim3 grid((unsigned)((W + MT - 1) / MT), (unsigned)((H + MT - 1) / MT), (unsigned)M);
    hipLaunchKernelGGL(morph7_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned char*>(in),
                       static_cast<unsigned char*>(out), (int)H, (int)W, erode);
    SS_LAUNCH_CHECK("morph7");
    return 0;
}

extern "C" int simseg_close7(const void* in, void* out, const int* valid, int64_t M, int64_t H, int64_t W, void* stream) {
    SS_CHECK(in && out && in != out, "close7: null or aliased pointers");
    SS_CHECK(M > 0 && M < 65536 && H > 0 && W > 0, "close7: bad shape");
    dim3 grid((unsigned)((W + CT - 1) / CT), (unsigned)((H + CT - 1) / CT), (unsigned)M);
    hipLaunchKernelGGL(close7_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned char*>(in),
                       static_cast<unsigned char*>(out), valid, (int)H, (int)W);
    SS_LAUNCH_CHECK("close7");
    return 0;
}

extern "C" int simseg_seg_predict(const void* masks, const int* cand_idx, const float* cand_score, const void* labels, int* pred,
                                  void* hist, int64_t B, int64_t ncand, int64_t Hm, int64_t Wm, int64_t H, int64_t W, int64_t C,
                                  int64_t ignore_index, void* stream) {
    SS_CHECK(masks && cand_idx && cand_score && labels && hist, "seg_predict: null pointer");
    SS_CHECK(B > 0 && B < 65536 && ncand >= 1 && ncand <= 8 && Hm > 0 && Wm > 0 && H > 0 && W > 0, "seg_predict: bad shape");
    SS_CHECK(C > 0 && C <= HIST_MAXC, "seg_predict: C <= %d", HIST_MAXC);
    const long npix = (long)H * W;
    long blocks = (npix + 256 * 8 - 1) / (256 * 8);          // ~8 pixels per thread: the LDS histogram flush stays small
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(seg_predict_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(masks), cand_idx, cand_score, static_cast<const unsigned char*>(labels), (int)ncand,
                       (int)Hm, (int)Wm, (int)H, (int)W, (int)C, (int)ignore_index, pred, static_cast<unsigned long long*>(hist));
    SS_LAUNCH_CHECK("seg_predict");
    return 0;
}

extern "C" int simseg_slide_extract(const float* images, const int64_t* img_tab, const int64_t* win_tab, float* out, int64_t Nw, int64_t win,
                                    void* stream) {
    SS_CHECK(images && img_tab && win_tab && out, "slide_extract: null pointer");
    SS_CHECK(Nw > 0 && win > 0 && win % 16 == 0, "slide_extract: Nw > 0 and win a positive multiple of 16");
    SS_CHECK(((uintptr_t)out % 16) == 0, "slide_extract: out must be 16-byte aligned");
    const long n4 = (long)Nw * 3 * win * win / 4;
    long blocks = (n4 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(slide_extract_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, images, img_tab, win_tab, out, n4, (int)win);
    SS_LAUNCH_CHECK("slide_extract");
    return 0;
}

extern "C" int simseg_slide_scores(const float* win_scores, const int64_t* img_tab, float* out, int64_t B, int64_t C, void* stream) {
    SS_CHECK(win_scores && img_tab && out, "slide_scores: null pointer");
    SS_CHECK(B > 0 && C > 0 && B * C < (1ll << 31), "slide_scores: bad shape");
    hipLaunchKernelGGL(slide_scores_kernel, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, win_scores, img_tab, out, (int)B,
                       (int)C);
    SS_LAUNCH_CHECK("slide_scores");
    return 0;
}

extern "C" int64_t simseg_slide_stitch_workspace_bytes(int64_t B, int64_t ncand, int64_t max_h, int64_t max_w) {
    if (B <= 0 || ncand <= 0 || max_h <= 0 || max_w <= 0) return -1;
    return B * ncand * ((max_h + ST_T - 1) / ST_T) * ((max_w + ST_T - 1) / ST_T) * 2 * (int64_t)sizeof(float);
}

extern "C" int simseg_slide_stitch(const float* sim_w, const int64_t* img_tab, const int64_t* win_tab, const int* cand_idx, float* prob, void* mask,
                                   float* minmax, float* workspace, int64_t B, int64_t ncand, int64_t n, int64_t C, int64_t win, int64_t max_h,
                                   int64_t max_w, int64_t max_hw, void* stream) {
    SS_CHECK(sim_w && img_tab && win_tab && cand_idx && prob && mask && minmax && workspace, "slide_stitch: null pointer");
    SS_CHECK(B > 0 && B < 65536 && ncand >= 1 && ncand <= 8 && C > 0 && win > 0 && win % 16 == 0 && n == win / 16,
             "slide_stitch: bad shape (n = win / 16, 1 <= ncand <= 8)");
    SS_CHECK(max_h > 0 && max_w > 0 && max_h < (1 << 20) && max_w < (1 << 20) && max_hw >= 1 && max_hw <= max_h * max_w,
             "slide_stitch: bad image extents");
    SS_CHECK(((uintptr_t)prob % 16) == 0 && ((uintptr_t)mask % 16) == 0, "slide_stitch: prob and mask must be 16-byte aligned");
    const long tiles = ((max_h + ST_T - 1) / ST_T) * ((max_w + ST_T - 1) / ST_T);
    SS_CHECK(tiles < (1l << 31), "slide_stitch: image too large");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(slide_stitch_kernel, dim3((unsigned)tiles, (unsigned)ncand, (unsigned)B), dim3(256), 0, s, sim_w, img_tab, win_tab, cand_idx,
                       (int)ncand, (int)C, (int)win, (int)n, (int)tiles, prob, workspace);
    SS_LAUNCH_CHECK("slide_stitch");
    hipLaunchKernelGGL(slide_minmax_kernel, dim3((unsigned)ncand, (unsigned)B), dim3(256), 0, s, img_tab, cand_idx, (int)ncand, (int)tiles, workspace,
                       minmax);
    SS_LAUNCH_CHECK("slide_stitch (min / max)");
    long blocks = (max_hw / 16 + 2 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(slide_norm_kernel, dim3((unsigned)blocks, (unsigned)ncand, (unsigned)B), dim3(256), 0, s, img_tab, cand_idx, (int)ncand, minmax,
                       prob, static_cast<unsigned char*>(mask));
    SS_LAUNCH_CHECK("slide_stitch (normalise)");
    return 0;
}

extern "C" int simseg_slide_extract_flip(const float* images, const int64_t* img_tab, const int64_t* win_tab, float* out, int64_t Nw, int64_t win,
                                         int flip, void* stream) {
    if (!flip) return simseg_slide_extract(images, img_tab, win_tab, out, Nw, win, stream);
    SS_CHECK(images && img_tab && win_tab && out, "slide_extract_flip: null pointer");
    SS_CHECK(Nw > 0 && win > 0 && win % 16 == 0, "slide_extract_flip: Nw > 0 and win a positive multiple of 16");
    SS_CHECK(((uintptr_t)out % 16) == 0, "slide_extract_flip: out must be 16-byte aligned");
    const long n4 = (long)Nw * 3 * win * win / 4;
    long blocks = (n4 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(slide_extract_flip_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, images, img_tab, win_tab, out, n4,
                       (int)win);
    SS_LAUNCH_CHECK("slide_extract_flip");
    return 0;
}

extern "C" int64_t simseg_slide_stitch_multi_workspace_bytes(int64_t B, int64_t ncand, int64_t max_h, int64_t max_w) {
    return simseg_slide_stitch_workspace_bytes(B, ncand, max_h, max_w);
}

extern "C" int simseg_slide_stitch_multi(const int64_t* pass_tab, int64_t P, const int64_t* img_tab, const int* cand_idx, float* prob, void* mask,
                                         float* minmax, float* workspace, int64_t B, int64_t ncand, int64_t n, int64_t C, int64_t win,
                                         int64_t max_h, int64_t max_w, int64_t max_hw, void* stream) {
    SS_CHECK(P >= 1 && P <= SLIDE_MAXP, "slide_stitch_multi: %lld passes, 1 <= P <= %d", (long long)P, SLIDE_MAXP);
    SS_CHECK(pass_tab && img_tab && cand_idx && prob && mask && minmax && workspace, "slide_stitch_multi: null pointer");
    SS_CHECK(B > 0 && B < 65536 && ncand >= 1 && ncand <= 8 && C > 0 && win > 0 && win % 16 == 0 && n == win / 16,
             "slide_stitch_multi: bad shape (n = win / 16, 1 <= ncand <= 8)");
    SS_CHECK(max_h > 0 && max_w > 0 && max_h < (1 << 20) && max_w < (1 << 20) && max_hw >= 1 && max_hw <= max_h * max_w,
             "slide_stitch_multi: bad image extents");
    SS_CHECK(((uintptr_t)prob % 16) == 0 && ((uintptr_t)mask % 16) == 0, "slide_stitch_multi: prob and mask must be 16-byte aligned");
    const long tiles = ((max_h + ST_T - 1) / ST_T) * ((max_w + ST_T - 1) / ST_T);
    SS_CHECK(tiles < (1l << 31), "slide_stitch_multi: image too large");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(slide_stitch_multi_kernel, dim3((unsigned)tiles, (unsigned)ncand, (unsigned)B), dim3(256), 0, s, pass_tab, (int)P, img_tab,
                       cand_idx, (int)ncand, (int)C, (int)win, (int)n, (int)tiles, prob, workspace);
    SS_LAUNCH_CHECK("slide_stitch_multi");
    // passes 2 and 3 are K23's, on the base image table: the fused map lies where the single-pass stitch puts its own
    hipLaunchKernelGGL(slide_minmax_kernel, dim3((unsigned)ncand, (unsigned)B), dim3(256), 0, s, img_tab, cand_idx, (int)ncand, (int)tiles, workspace,
                       minmax);
    SS_LAUNCH_CHECK("slide_stitch_multi (min / max)");
    long blocks = (max_hw / 16 + 2 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(slide_norm_kernel, dim3((unsigned)blocks, (unsigned)ncand, (unsigned)B), dim3(256), 0, s, img_tab, cand_idx, (int)ncand, minmax,
                       prob, static_cast<unsigned char*>(mask));
    SS_LAUNCH_CHECK("slide_stitch_multi (normalise)");
    return 0;
}
