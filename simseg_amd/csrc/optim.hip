// Everything that walks a tensor table (tensor_table.h): the fused AdamW step and its gradient checks (overflow flag, global norm and
// clipping coefficient), and LARS as three launches.  Compiled ONCE: the kernels that refresh the 16-bit compute copy of the weights take
// its type (bf16 / fp16) as a template argument chosen from the calling thread's simseg_set_half_type; everything else here is fp32.
#include "common.h"
#include "tensor_table.h"

namespace {

// torch.optim.AdamW step on a flat fp32 segment, optionally refreshing the bf16 compute copy of the weights.
template <typename H>
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             H* __restrict__ p16, long n, float lr, float b1, float b2, float eps, float wd, float bc1,
                             float bc2_sqrt, float grad_scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gi = g[i] * grad_scale;
        float pi = p[i] * (1.0f - lr * wd);
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi -= (lr / bc1) * (mi / denom);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (p16) p16[i] = (H)pi;
    }
}

// Multi-tensor form: one launch for every parameter tensor over a tensor table (tensor_table.h).  table[t] = {p, g, m, v, p16, lr,
// weight_decay}: five device pointers and the tensor's own learning rate / weight decay (the reference builds one param group per
// parameter, tasks/clip/hooks/optimizer.py:18-36).  p16 (may be null) is the 16-bit compute copy (type H of the kernel) the next forward's
// GEMMs read: refreshed here, so no per-step cast kernels.
struct AdamTensors { float* p; const float* g; float* m; float* v; void* p16; float lr; float wd; };
static_assert(sizeof(AdamTensors) == 48, "table rows are six 8-byte words");
// AMP form (round 4): the loss scale, the overflow flag and the count of steps actually taken live on the DEVICE (amp.scale / amp.found_inf:
// torch.amp.GradScaler's tensors, handed over through its `optimizer.grad_scale` / `optimizer.found_inf` contract; amp.step_in / step_out:
// this optimizer's own two-slot counter).  The gradients are unscaled here (g / scale), and a step whose gradients held an inf / nan updates
// nothing - the decision never travels to the host, so the reference's fp16 iteration (clip_runner.py:226-230, core/hooks/optimizer.py:73-82)
// runs without the host read torch's scaler.step() makes for an optimizer that cannot skip by itself.  Bias corrections come from the device
// counter (skipped steps do not count, as in torch's own fused Adam).
struct AdamAmp { const float* scale; const float* found_inf; const float* step_in; float* step_out; };
// CLIP (simseg_adamw_multi_step_clip / _amp_clip): every gradient element is also multiplied by coef[0], the global-norm clipping
// coefficient simseg_grads_norm_finish left on the device - AFTER the unscale, the reference's order (core/hooks/optimizer.py:45-47:
// scaler.unscale_ then clip_grad_norm_).  A template flag, not a multiply by 1.0f: the instantiation without it is the kernel as it was.
template <bool CLIP, typename H>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const AdamTensors* __restrict__ table, const long* __restrict__ sizes,
                                                          const int* __restrict__ chunk_tid, const long* __restrict__ chunk_off,
                                                          int chunk, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                          float grad_scale, AdamAmp amp, const float* __restrict__ coef) {
    const int c = blockIdx.x;
    if (amp.step_in) {
        const bool skip = amp.found_inf && amp.found_inf[0] != 0.f;
        const float st = amp.step_in[0] + (skip ? 0.f : 1.f);
        if (c == 0 && threadIdx.x == 0) amp.step_out[0] = st;      // (the other slot: nobody reads it during this launch)
        if (skip) return;
        bc1 = 1.0f - powf(b1, st);
        bc2_sqrt = sqrtf(1.0f - powf(b2, st));
        if (amp.scale) grad_scale /= amp.scale[0];
    }
    const auto ch = table_chunk(table, sizes, chunk_tid, chunk_off, chunk);
    const AdamTensors T = ch.T;      // (plain locals, not structured bindings: with them the compiler emits the loops below differently)
    const long lo = ch.lo, hi = ch.hi;
    H* p16 = reinterpret_cast<H*>(T.p16);
    const float decay = 1.0f - T.lr * T.wd;
    const float step_size = T.lr / bc1;
    const float clip = CLIP ? coef[0] : 1.0f;
    auto one = [&](float g_, float& pi, float& mi, float& vi) {
        float gi = g_ * grad_scale;
        if (CLIP) gi *= clip;
        pi *= decay;
        mi = b1 * mi + (1.0f - b1) * gi;
        vi = b2 * vi + (1.0f - b2) * gi * gi;
        pi -= step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    };
    // 16 bytes per lane and streaming (non-temporal) accesses when the chunk allows it: every array is touched exactly once per step
    // (30 bytes per parameter, 5.9 GB for ViT-B + BERT-base)
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef H h4 __attribute__((ext_vector_type(4)));
    const bool vec = (((uintptr_t)(T.g + lo) | (uintptr_t)(T.p + lo) | (uintptr_t)(T.m + lo) | (uintptr_t)(T.v + lo)) % 16 == 0) &&
                     (!p16 || (uintptr_t)(p16 + lo) % 8 == 0);
    long i0 = lo;
    if (vec) {
        const long n4 = (hi - lo) / 4;
        for (long q = threadIdx.x; q < n4; q += 256) {
            const long i = lo + 4 * q;
            const f4 g4 = __builtin_nontemporal_load(reinterpret_cast<const f4*>(T.g + i));
            f4 p4 = __builtin_nontemporal_load(reinterpret_cast<const f4*>(T.p + i));
            f4 m4 = __builtin_nontemporal_load(reinterpret_cast<const f4*>(T.m + i));
            f4 v4 = __builtin_nontemporal_load(reinterpret_cast<const f4*>(T.v + i));
#pragma unroll
            for (int e = 0; e < 4; ++e) { float pe = p4[e], me = m4[e], ve = v4[e]; one(g4[e], pe, me, ve); p4[e] = pe; m4[e] = me; v4[e] = ve; }
            __builtin_nontemporal_store(p4, reinterpret_cast<f4*>(T.p + i));
            __builtin_nontemporal_store(m4, reinterpret_cast<f4*>(T.m + i));
            __builtin_nontemporal_store(v4, reinterpret_cast<f4*>(T.v + i));
            if (p16) {
                h4 o = {(H)p4[0], (H)p4[1], (H)p4[2], (H)p4[3]};
                *reinterpret_cast<h4*>(p16 + i) = o;                   // (read by the next step's GEMMs: default policy)
            }
        }
        i0 = lo + 4 * n4;
    }
    for (long i = i0 + threadIdx.x; i < hi; i += 256) {
        float pi = T.p[i], mi = T.m[i], vi = T.v[i];
        one(T.g[i], pi, mi, vi);
        T.p[i] = pi; T.m[i] = mi; T.v[i] = vi;
        if (p16) p16[i] = (H)pi;
    }
}

// found[0] = 1 if any gradient element of the table's tensors is inf / nan (read-only pass, 16 bytes per lane, one store per block that
// sees one): the overflow check of torch.amp.GradScaler (`_amp_foreach_non_finite_check_and_unscale_` with inverse scale 1: a read-modify-
// write pass over every gradient tensor) as ONE launch over the optimizer's own tensor table; the unscaling itself rides on the AdamW kernel.
__global__ __launch_bounds__(256) void grads_nonfinite_kernel(const AdamTensors* __restrict__ table, const long* __restrict__ sizes,
                                                              const int* __restrict__ chunk_tid, const long* __restrict__ chunk_off,
                                                              int chunk, float* __restrict__ found) {
    const auto [t, T, lo, hi] = table_chunk(table, sizes, chunk_tid, chunk_off, chunk);
    const float* g = T.g;
    unsigned bad = 0;
    long i0 = lo;
    if ((uintptr_t)(g + lo) % 16 == 0) {
        const long n4 = (hi - lo) / 4;
        for (long q = threadIdx.x; q < n4; q += 256) {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g + lo + 4 * q));
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= ((v[e] & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
        }
        i0 = lo + 4 * n4;
    }
    for (long i = i0 + threadIdx.x; i < hi; i += 256) bad |= ((__float_as_uint(g[i]) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
    if (__any(bad != 0) && (threadIdx.x & 63) == 0) found[0] = 1.0f;
}

// Global gradient norm, pass 1: partials[c] = sum of g^2 (norm_type 2) or max |g| (norm_type 0 = infinity) over chunk c of the table's
// gradient tensors - the same read-only walk as grads_nonfinite_kernel (16 bytes per lane, streaming loads, scalar tail / unaligned
// chunks).  fp32 sums: four independent accumulators per lane (<= 64 terms each for a 65536-element chunk), combined pairwise, a wave
// butterfly, then LDS across the four waves in a fixed order; one plain store per block and no atomics, so a call is bit-reproducible.
// inf and nan propagate through the sums by themselves.  The maximum is taken on the bit patterns of |g| as unsigned integers: for
// non-negative floats that is the floating-point order, and every nan pattern lies above +inf, so a nan wins (fmaxf would drop it).
__global__ __launch_bounds__(256) void grads_norm_partials_kernel(const AdamTensors* __restrict__ table, const long* __restrict__ sizes,
                                                                  const int* __restrict__ chunk_tid, const long* __restrict__ chunk_off,
                                                                  int chunk, int norm_type, float* __restrict__ partials) {
    __shared__ float sh[4];
    const int c = blockIdx.x;
    const auto [t, T, lo, hi] = table_chunk(table, sizes, chunk_tid, chunk_off, chunk);
    const float* g = T.g;
    const bool vec = (uintptr_t)(g + lo) % 16 == 0;
    const long n4 = vec ? (hi - lo) / 4 : 0;
    const long i0 = lo + 4 * n4;
    float r;
    if (norm_type == 2) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (long q = threadIdx.x; q < n4; q += 256) {
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + lo + 4 * q));
            a0 += v[0] * v[0]; a1 += v[1] * v[1]; a2 += v[2] * v[2]; a3 += v[3] * v[3];
        }
        for (long i = i0 + threadIdx.x; i < hi; i += 256) a0 += g[i] * g[i];
        r = wave_sum((a0 + a1) + (a2 + a3));
    } else {
        unsigned m = 0;
        for (long q = threadIdx.x; q < n4; q += 256) {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(g + lo + 4 * q));
#pragma unroll
            for (int e = 0; e < 4; ++e) m = max(m, v[e] & 0x7fffffffu);
        }
        for (long i = i0 + threadIdx.x; i < hi; i += 256) m = max(m, __float_as_uint(g[i]) & 0x7fffffffu);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
        r = __uint_as_float(m);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (norm_type == 2) r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        else r = __uint_as_float(max(max(__float_as_uint(sh[0]), __float_as_uint(sh[1])), max(__float_as_uint(sh[2]), __float_as_uint(sh[3]))));
        partials[c] = r;
    }
}

// Pass 2, one block: the partials of every bucket reduced in double precision (fixed order: strided per lane, wave butterfly, LDS).
// out2[0] = the total norm, divided by loss_scale[0] when given (the norm of the UNSCALED gradients, which is what the reference clips);
// out2[1] = min(1, max_norm / (total_norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s coefficient (a nan norm gives a nan coefficient, as
// torch's clamp does).  Everything stays on the device.
__global__ __launch_bounds__(256) void grads_norm_finish_kernel(const float* __restrict__ partials, long n, int norm_type, float max_norm,
                                                                const float* __restrict__ loss_scale, float* __restrict__ out2) {
    __shared__ double shd[4];
    double acc = 0.0;
    if (norm_type == 2) {
        for (long i = threadIdx.x; i < n; i += 256) acc += (double)partials[i];
    } else {
        unsigned m = 0;
        for (long i = threadIdx.x; i < n; i += 256) m = max(m, __float_as_uint(partials[i]));
        acc = (double)m;          // (exact: the bit patterns are ordered like the values; turned back into a float below)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(acc, o, 64);
        acc = norm_type == 2 ? acc + other : fmax(acc, other);
    }
    if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total;
        if (norm_type == 2) total = sqrt((shd[0] + shd[1]) + (shd[2] + shd[3]));
        else total = (double)__uint_as_float((unsigned)fmax(fmax(shd[0], shd[1]), fmax(shd[2], shd[3])));
        if (loss_scale) total /= (double)loss_scale[0];
        double coef = (double)max_norm / (total + 1e-6);
        if (coef > 1.0) coef = 1.0;
        out2[0] = (float)total;
        out2[1] = (float)coef;
    }
}

// ---- LARS over a tensor table (tensor_table.h) ---------------------------------------------------------------------------------------
// table[t] = {p, g, buf, p16, (float lr, float weight_decay), flags}: fp32 master, fp32 gradient, fp32 momentum buffer (0 when momentum
// == 0), the 16-bit compute copy to refresh (or 0), the tensor's learning rate and weight decay, and flags: bit 0 = lars_exclude (local
// lr 1), bit 1 = first step of this tensor (no momentum buffer yet: buf = d).
struct LarsTensors { float* p; const float* g; float* buf; void* p16; float lr; float wd; long flags; };
static_assert(sizeof(LarsTensors) == 48, "table rows are six 8-byte words");

// partials[2c] = sum of p^2, partials[2c + 1] = sum of g^2 over chunk c.  Read-only on p and g; double accumulators (the pass is bound by
// its 8 bytes per element, not by the FMAs), wave butterfly, the four waves through LDS in a fixed order, one plain store per sum.
__global__ __launch_bounds__(256) void lars_norm_partials_kernel(const LarsTensors* __restrict__ table, const long* __restrict__ sizes,
                                                                 const int* __restrict__ chunk_tid, const long* __restrict__ chunk_off,
                                                                 int chunk, double* __restrict__ partials) {
    __shared__ double sh[8];
    const int c = blockIdx.x;
    const auto [t, T, lo, hi] = table_chunk(table, sizes, chunk_tid, chunk_off, chunk);
    const float* p = T.p;
    const float* g = T.g;
    const bool vec = (((uintptr_t)(p + lo) | (uintptr_t)(g + lo)) % 16) == 0;
    const long n4 = vec ? (hi - lo) / 4 : 0;
    double pp = 0.0, gg = 0.0;
    for (long q = threadIdx.x; q < n4; q += 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + lo + 4 * q);
        const f32x4 b = *reinterpret_cast<const f32x4*>(g + lo + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            pp = fma((double)a[e], (double)a[e], pp);
            gg = fma((double)b[e], (double)b[e], gg);
        }
    }
    for (long i = lo + 4 * n4 + threadIdx.x; i < hi; i += 256) {
        pp = fma((double)p[i], (double)p[i], pp);
        gg = fma((double)g[i], (double)g[i], gg);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pp += __shfl_xor(pp, o, 64);
        gg += __shfl_xor(gg, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = pp;
        sh[4 + (threadIdx.x >> 6)] = gg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * (long)c] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        partials[2 * (long)c + 1] = (sh[4] + sh[5]) + (sh[6] + sh[7]);
    }
}

// One block (one wave) per tensor: its chunks' partials, [tensor_first[t], tensor_first[t + 1]), are summed in CHUNK order in double
// precision (the lanes fetch 64 at a time, the additions run in order), then
//   local_lr[t] = eta * wn / (gn + weight_decay * wn + eps)   when wn != 0 and gn != 0, else 1;   1 for a lars_exclude tensor.
// The reference reads both norms on the host (two .item() calls per tensor, lars.py:104-105); here nothing leaves the device.
__global__ __launch_bounds__(64) void lars_finish_kernel(const LarsTensors* __restrict__ table, const int* __restrict__ tensor_first,
                                                         const double* __restrict__ partials, float eta, float eps,
                                                         float* __restrict__ local_lr) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const int c0 = tensor_first[t], c1 = tensor_first[t + 1];
    double sp = 0.0, sg = 0.0;
    for (int base = c0; base < c1; base += 64) {
        const int k = base + lane;
        const double a = k < c1 ? partials[2 * (long)k] : 0.0;
        const double b = k < c1 ? partials[2 * (long)k + 1] : 0.0;
        const int n = min(64, c1 - base);
        for (int j = 0; j < n; ++j) {
            sp += __shfl(a, j, 64);
            sg += __shfl(b, j, 64);
        }
    }
    if (lane == 0) {
        float out = 1.0f;
        if (!(table[t].flags & 1)) {
            const double wn = sqrt(sp), gn = sqrt(sg);
            if (wn != 0.0 && gn != 0.0) out = (float)((double)eta * wn / (gn + (double)table[t].wd * wn + (double)eps));
        }
        local_lr[t] = out;
    }
}

// The update, per element (lars.py:113-127 restated):
//   d = (g + weight_decay * p) * (local_lr[t] * lr)
//   momentum != 0:  buf = d on the tensor's first step, else momentum * buf + (1 - dampening) * d;   d = nesterov ? d + momentum * buf : buf
//   p -= d;  p16 = p rounded to the 16-bit type
// The arithmetic runs in double between the fp32 loads and stores (20 bytes of traffic per element: the kernel is bound by memory, and the
// result is then the correctly rounded value of the law above rather than a chain of fp32 roundings); buf is rounded to fp32 BEFORE it
// enters d, as the stored buffer is what the reference's update reads.
template <typename H>
__global__ __launch_bounds__(256) void lars_multi_kernel(const LarsTensors* __restrict__ table, const long* __restrict__ sizes,
                                                         const int* __restrict__ chunk_tid, const long* __restrict__ chunk_off, int chunk,
                                                         const float* __restrict__ local_lr, float momentum, float dampening,
                                                         int nesterov) {
    const auto ch = table_chunk(table, sizes, chunk_tid, chunk_off, chunk);
    const LarsTensors T = ch.T;      // (plain locals, as in adamw_multi_kernel)
    const int t = ch.t;
    const long lo = ch.lo, hi = ch.hi;
    H* p16 = reinterpret_cast<H*>(T.p16);
    const double scale = (double)local_lr[t] * (double)T.lr;
    const double wd = (double)T.wd, mom = (double)momentum, keep = 1.0 - (double)dampening;
    const bool first = (T.flags & 2) != 0;
    const bool use_buf = momentum != 0.f && T.buf != nullptr;
    auto one = [&](float g_, float& pi, float& bi) {
        double d = ((double)g_ + wd * (double)pi) * scale;
        if (use_buf) {
            bi = (float)(first ? d : mom * (double)bi + keep * d);
            d = nesterov ? d + mom * (double)bi : (double)bi;
        }
        pi = (float)((double)pi - d);
    };
    const bool vec = (((uintptr_t)(T.g + lo) | (uintptr_t)(T.p + lo)) % 16 == 0) && (!use_buf || (uintptr_t)(T.buf + lo) % 16 == 0) &&
                     (!p16 || (uintptr_t)(p16 + lo) % 8 == 0);
    long i0 = lo;
    if (vec) {
        typedef H h4 __attribute__((ext_vector_type(4)));
        const long n4 = (hi - lo) / 4;
        for (long q = threadIdx.x; q < n4; q += 256) {
            const long i = lo + 4 * q;
            const f32x4 g4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(T.g + i));
            f32x4 p4 = *reinterpret_cast<const f32x4*>(T.p + i);
            f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
            if (use_buf && !first) b4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(T.buf + i));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p4[e], be = b4[e];
                one(g4[e], pe, be);
                p4[e] = pe;
                b4[e] = be;
            }
            *reinterpret_cast<f32x4*>(T.p + i) = p4;
            if (use_buf) __builtin_nontemporal_store(b4, reinterpret_cast<f32x4*>(T.buf + i));
            if (p16) {
                const h4 o = {(H)p4[0], (H)p4[1], (H)p4[2], (H)p4[3]};
                *reinterpret_cast<h4*>(p16 + i) = o;
            }
        }
        i0 = lo + 4 * n4;
    }
    for (long i = i0 + threadIdx.x; i < hi; i += 256) {
        float pi = T.p[i], bi = (use_buf && !first) ? T.buf[i] : 0.f;
        one(T.g[i], pi, bi);
        T.p[i] = pi;
        if (use_buf) T.buf[i] = bi;
        if (p16) p16[i] = (H)pi;
    }
}

// The chunk tables as the HOST sees them, checked before anything is launched (the kernels index with them).
int lars_check_tables(const char* who, const int64_t* sizes_host, const int32_t* chunk_tid_host, const int64_t* chunk_off_host,
                      int64_t n_tensors, int64_t n_chunks, int chunk) {
    SS_CHECK(sizes_host && chunk_tid_host && chunk_off_host, "%s: null host table", who);
    SS_CHECK(n_tensors >= 1 && n_tensors < (1ll << 31) && n_chunks >= 0 && n_chunks < (1ll << 31) && chunk > 0,
             "%s: bad table extents (%lld tensors, %lld chunks of %d)", who, (long long)n_tensors, (long long)n_chunks, chunk);
    for (int64_t t = 0; t < n_tensors; ++t)
        SS_CHECK(sizes_host[t] >= 0, "%s: tensor %lld has a negative size (%lld)", who, (long long)t, (long long)sizes_host[t]);
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t t = chunk_tid_host[c];
        SS_CHECK(t >= 0 && t < n_tensors, "%s: chunk %lld names tensor id %lld, outside [0, %lld)", who, (long long)c, (long long)t,
                 (long long)n_tensors);
        SS_CHECK(chunk_off_host[c] >= 0 && chunk_off_host[c] < sizes_host[t], "%s: chunk offset %lld of chunk %lld is past the end of tensor %lld (%lld elements)",
                 who, (long long)chunk_off_host[c], (long long)c, (long long)t, (long long)sizes_host[t]);
    }
    return 0;
}

}  // namespace

#define STREAM ((hipStream_t)stream)

// The launch of the four simseg_adamw_multi_step* entry points: `step` is the host's count (bias corrections formed here), or the
// device counter travels in `amp`; grad_coef selects CLIP, the calling thread's 16-bit type the p16 stores.
static int adamw_multi_launch(const char* who, const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                              int64_t n_chunks, int chunk, float beta1, float beta2, float eps, int64_t step, AdamAmp amp, float grad_scale,
                              const float* grad_coef, void* stream) {
    if (amp.step_in) SS_CHECK(chunk > 0, "%s: bad chunk", who);
    else SS_CHECK(step >= 1 && chunk > 0, "%s: bad step/chunk", who);
    if (n_chunks <= 0) return 0;
    const float bc1 = amp.step_in ? 1.0f : 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = amp.step_in ? 1.0f : sqrtf(1.0f - powf(beta2, (float)step));
    const auto kernel = g_ss_half == 2 ? (grad_coef ? adamw_multi_kernel<true, _Float16> : adamw_multi_kernel<false, _Float16>)
                                       : (grad_coef ? adamw_multi_kernel<true, __bf16> : adamw_multi_kernel<false, __bf16>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_chunks), dim3(256), 0, STREAM, (const AdamTensors*)table, (const long*)sizes,
                       (const int*)chunk_tid, (const long*)chunk_off, chunk, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale, amp, grad_coef);
    SS_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int simseg_adamw_multi_step(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                       int64_t n_chunks, int chunk, float beta1, float beta2, float eps, int64_t step,
                                       float grad_scale, void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off, "adamw_multi_step: null pointer");
    return adamw_multi_launch("adamw_multi_step", table, sizes, chunk_tid, chunk_off, n_chunks, chunk, beta1, beta2, eps, step, AdamAmp{},
                              grad_scale, nullptr, stream);
}

extern "C" int simseg_adamw_multi_step_clip(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                            int64_t n_chunks, int chunk, float beta1, float beta2, float eps, int64_t step,
                                            float grad_scale, const float* grad_coef, void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off && grad_coef, "adamw_multi_step_clip: null pointer");
    return adamw_multi_launch("adamw_multi_step_clip", table, sizes, chunk_tid, chunk_off, n_chunks, chunk, beta1, beta2, eps, step, AdamAmp{},
                              grad_scale, grad_coef, stream);
}

extern "C" int simseg_adamw_multi_step_amp(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                           int64_t n_chunks, int chunk, float beta1, float beta2, float eps, float grad_scale,
                                           const float* loss_scale, const float* found_inf, const float* step_in, float* step_out, void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off && step_in && step_out && step_in != step_out, "adamw_multi_step_amp: null / aliased pointer");
    return adamw_multi_launch("adamw_multi_step_amp", table, sizes, chunk_tid, chunk_off, n_chunks, chunk, beta1, beta2, eps, 0,
                              AdamAmp{loss_scale, found_inf, step_in, step_out}, grad_scale, nullptr, stream);
}

extern "C" int simseg_adamw_multi_step_amp_clip(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                                int64_t n_chunks, int chunk, float beta1, float beta2, float eps, float grad_scale,
                                                const float* loss_scale, const float* found_inf, const float* step_in, float* step_out,
                                                const float* grad_coef, void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off && step_in && step_out && step_in != step_out && grad_coef,
             "adamw_multi_step_amp_clip: null / aliased pointer");
    return adamw_multi_launch("adamw_multi_step_amp_clip", table, sizes, chunk_tid, chunk_off, n_chunks, chunk, beta1, beta2, eps, 0,
                              AdamAmp{loss_scale, found_inf, step_in, step_out}, grad_scale, grad_coef, stream);
}

extern "C" int simseg_grads_nonfinite(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                      int64_t n_chunks, int chunk, float* found_inf, void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off && found_inf, "grads_nonfinite: null pointer");
    SS_CHECK(chunk > 0, "grads_nonfinite: bad chunk");
    if (n_chunks <= 0) return 0;
    hipLaunchKernelGGL(grads_nonfinite_kernel, dim3((unsigned)n_chunks), dim3(256), 0, STREAM, (const AdamTensors*)table, (const long*)sizes,
                       (const int*)chunk_tid, (const long*)chunk_off, chunk, found_inf);
    SS_LAUNCH_CHECK("grads_nonfinite");
    return 0;
}

extern "C" int simseg_grads_norm_partials(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                          int64_t n_chunks, int chunk, int norm_type, float* partials, void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off && partials, "grads_norm_partials: null pointer");
    SS_CHECK(chunk > 0 && (norm_type == 2 || norm_type == 0), "grads_norm_partials: chunk > 0, norm_type 2 or 0 (infinity)");
    if (n_chunks <= 0) return 0;
    hipLaunchKernelGGL(grads_norm_partials_kernel, dim3((unsigned)n_chunks), dim3(256), 0, STREAM, (const AdamTensors*)table,
                       (const long*)sizes, (const int*)chunk_tid, (const long*)chunk_off, chunk, norm_type, partials);
    SS_LAUNCH_CHECK("grads_norm_partials");
    return 0;
}

extern "C" int simseg_grads_norm_finish(const float* partials, int64_t n_partials, int norm_type, float max_norm, const float* loss_scale,
                                        float* out2, void* stream) {
    SS_CHECK(out2 && (partials || n_partials <= 0), "grads_norm_finish: null pointer");
    SS_CHECK(norm_type == 2 || norm_type == 0, "grads_norm_finish: norm_type 2 or 0 (infinity)");
    SS_CHECK(max_norm >= 0.f, "grads_norm_finish: max_norm %g is negative (or nan)", (double)max_norm);
    hipLaunchKernelGGL(grads_norm_finish_kernel, dim3(1), dim3(256), 0, STREAM, partials, (long)(n_partials > 0 ? n_partials : 0), norm_type,
                       max_norm, loss_scale, out2);
    SS_LAUNCH_CHECK("grads_norm_finish");
    return 0;
}

extern "C" int simseg_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* stream) {
    SS_CHECK(p && g && m && v, "adamw_step: null pointer");
    SS_CHECK(step >= 1, "adamw_step: step counts from 1");
    if (n <= 0) return 0;
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2 = 1.0f - powf(beta2, (float)step);
    long blocks = (n + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (g_ss_half == 2)
        hipLaunchKernelGGL(adamw_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, STREAM, p, g, m, v, (_Float16*)p_bf16, (long)n, lr, beta1,
                           beta2, eps, weight_decay, bc1, sqrtf(bc2), grad_scale);
    else
        hipLaunchKernelGGL(adamw_kernel<__bf16>, dim3((unsigned)blocks), dim3(256), 0, STREAM, p, g, m, v, (__bf16*)p_bf16, (long)n, lr, beta1,
                           beta2, eps, weight_decay, bc1, sqrtf(bc2), grad_scale);
    SS_LAUNCH_CHECK("adamw_step");
    return 0;
}

extern "C" int simseg_lars_norm_partials(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                         const int64_t* sizes_host, const int32_t* chunk_tid_host, const int64_t* chunk_off_host,
                                         int64_t n_tensors, int64_t n_chunks, int chunk, double* partials, void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off && partials, "lars_norm_partials: null pointer");
    if (int rc = lars_check_tables("lars_norm_partials", sizes_host, chunk_tid_host, chunk_off_host, n_tensors, n_chunks, chunk)) return rc;
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(lars_norm_partials_kernel, dim3((unsigned)n_chunks), dim3(256), 0, STREAM, (const LarsTensors*)table, (const long*)sizes,
                       chunk_tid, (const long*)chunk_off, chunk, partials);
    SS_LAUNCH_CHECK("lars_norm_partials");
    return 0;
}

extern "C" int simseg_lars_finish(const void* table, const int32_t* tensor_first, const int32_t* tensor_first_host, const double* partials,
                                  int64_t n_tensors, int64_t n_chunks, float eta, float eps, float* local_lr, void* stream) {
    SS_CHECK(table && tensor_first && tensor_first_host && partials && local_lr, "lars_finish: null pointer");
    SS_CHECK(n_tensors >= 1 && n_tensors < (1ll << 31) && n_chunks >= 0 && n_chunks < (1ll << 31), "lars_finish: bad table extents (%lld tensors, %lld chunks)",
             (long long)n_tensors, (long long)n_chunks);
    SS_CHECK(eta >= 0.f && eps >= 0.f, "lars_finish: eta %g / eps %g is negative (or nan)", (double)eta, (double)eps);
    SS_CHECK(tensor_first_host[0] == 0 && tensor_first_host[n_tensors] == n_chunks, "lars_finish: the tensors' chunk ranges cover [%d, %d), not [0, %lld)",
             tensor_first_host[0], tensor_first_host[n_tensors], (long long)n_chunks);
    for (int64_t t = 0; t < n_tensors; ++t)
        SS_CHECK(tensor_first_host[t] <= tensor_first_host[t + 1], "lars_finish: the chunk range of tensor %lld is reversed", (long long)t);
    hipLaunchKernelGGL(lars_finish_kernel, dim3((unsigned)n_tensors), dim3(64), 0, STREAM, (const LarsTensors*)table, tensor_first, partials, eta, eps,
                       local_lr);
    SS_LAUNCH_CHECK("lars_finish");
    return 0;
}

extern "C" int simseg_lars_multi_step(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                      const int64_t* sizes_host, const int32_t* chunk_tid_host, const int64_t* chunk_off_host, int64_t n_tensors,
                                      int64_t n_chunks, int chunk, const float* local_lr, float momentum, float dampening, int nesterov,
                                      void* stream) {
    SS_CHECK(table && sizes && chunk_tid && chunk_off && local_lr, "lars_multi_step: null pointer");
    SS_CHECK(momentum >= 0.f, "lars_multi_step: momentum %g is negative (or nan)", (double)momentum);
    SS_CHECK(!nesterov || (momentum > 0.f && dampening == 0.f), "lars_multi_step: Nesterov momentum requires a momentum and zero dampening");
    if (int rc = lars_check_tables("lars_multi_step", sizes_host, chunk_tid_host, chunk_off_host, n_tensors, n_chunks, chunk)) return rc;
    if (n_chunks == 0) return 0;
    const dim3 grid((unsigned)n_chunks);
    if (g_ss_half == 2)
        hipLaunchKernelGGL(lars_multi_kernel<_Float16>, grid, dim3(256), 0, STREAM, (const LarsTensors*)table, (const long*)sizes, chunk_tid,
                           (const long*)chunk_off, chunk, local_lr, momentum, dampening, nesterov);
    else
        hipLaunchKernelGGL(lars_multi_kernel<__bf16>, grid, dim3(256), 0, STREAM, (const LarsTensors*)table, (const long*)sizes, chunk_tid,
                           (const long*)chunk_off, chunk, local_lr, momentum, dampening, nesterov);
    SS_LAUNCH_CHECK("lars_multi_step");
    return 0;
}
