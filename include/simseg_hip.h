/* libsimseg_hip.so -- C ABI of the MI355X-native SimSeg hot path (gfx950 only).
 *
 * The reference (muyangyi/SimSeg) has no native boundary: its hot path is torch/timm/HF Python.  This header is
 * the boundary our Python mirror of `simseg.models` binds through ctypes; each entry point names the reference
 * code it replaces (paths relative to /root/reference, or the third-party module the reference calls).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (PyTorch-ROCm tensors); the library never
 *     allocates, frees or retains device memory;
 *   - all work is enqueued on the caller's `stream` (a hipStream_t passed as void*); nothing synchronises;
 *   - return 0 on success, negative on error; the message is in simseg_last_error() (thread-local);
 *   - dtype codes: 0 = fp32, 1 = bf16.  Matrices are row-major.
 *   - the compute entry points are stateless and re-entrant: everything a call needs is in its arguments.  The only library state
 *     is per THREAD (thread_local): the last error string and the test / benchmark selectors `simseg_set_gemm_variant`,
 *     `simseg_set_attention_variant` (default 0 = auto), which affect only later calls made by the thread that set them.
 */
#ifndef SIMSEG_HIP_H
#define SIMSEG_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int simseg_version(void);
/* Which 16-bit type the calling thread's next calls compute in: 1 = bf16 (default), 2 = IEEE fp16 - the type of the reference's AMP mode
 * (torch.cuda.amp.autocast() + GradScaler, simseg/tasks/clip/clip_runner.py:226-230, core/hooks/optimizer.py:73-82).  dtype code 1
 * ("bf16") in every signature below means "the selected 16-bit type"; both flavours are the same kernels (v_mfma_f32_32x32x16_bf16 /
 * _f16, fp32 accumulation).  Thread-local. */
int simseg_set_half_type(int t);
const char* simseg_last_error(void);

/* C[M,N] = epilogue(alpha * opA(A) . opB(B)).  transA=0: A is [M,K]; 1: [K,M].  transB=0: B is [N,K] (nn.Linear
 * weight layout); 1: [K,N].  Epilogue order: *rowscale[row], +bias[col], (save pre-activation to aux_out),
 * act (1 = erf-GELU, 2 = multiply by GELU'(aux); 3 = erf-GELU with aux_out receiving GELU'(pre-activation) instead of the
 * pre-activation, 4 = multiply by aux: the training pair, no transcendental work in backward), dropout(p, seed), +residual.  row_group=G>0 writes row r to
 * (r/G)*(G+1)+1+r%G (ViT patch rows behind [cls]); res_mod reads the residual at row 1+r%G (pos_embed).
 * splitk>1 accumulates fp32 partials atomically into C (C must hold the value to accumulate onto).
 * colsum (optional, [N]) += column sums of the stored output: the bias gradient of the layer that produced C's input.
 * Replaces: nn.Linear inside timm Block / HF BertLayer (called via simseg/models/backbones/mml/vit_builder.py:18,
 * huggingface_builder.py:16-17), Conv2d patch embed (vit_builder.py:14), SimpleProjection
 * (simseg/models/components/projection.py:45-46), the logits matmul (simseg/models/criteria/losses/mml_loss.py:73),
 * the patch x text contraction (tools/seg_evaluation.py:136) and emb_sim (simseg/tasks/clip/hooks/utils.py:36). */
int simseg_gemm(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                int64_t ldc, int in_dtype, int out_dtype, int transA, int transB, float alpha, const float* bias,
                const float* rowscale, const float* residual, int64_t ldr, int act, const void* aux, void* aux_out,
                int row_group, int res_mod, int accumulate, int splitk, uint64_t drop_seed, float drop_p, float* colsum,
                void* stream);
/* act codes 5 / 6 of simseg_gemm = 3 / 4 (GELU with its derivative saved / times the saved derivative + column sums) with the saved tensor in
 * a tile-blocked layout private to the two calls: the fc1 forward and the dgrad through fc2 are the same M x N x K problem on the same
 * 256x256 tiling, so the derivative is stored as it lies in the accumulator registers and read back the same way (no transposition on
 * either side).  Allowed when this returns 1 for the problem (full tiles on the ping-pong kernels); aux / aux_out stay [M, N] 16-bit
 * allocations whose content is opaque.
 * act codes 7 / 8 (round 4) = 5 / 6 with that image in ONE BYTE per element (aux / aux_out: M x N bytes): GELU' lies in [-0.129, 1.129] and is
 * stored as round((g + 0.132) * 255 / 1.264), a uniform grid of 0.005 - finer than a 16-bit float's spacing where most of the gradient's
 * energy is (g in [0.5, 1.13]) and coarser where |g| is small; the product dY * g it feeds is as accurate against the exact derivative as
 * with the 16-bit image (relative RMS error 2.7e-3 against 2.5e-3, the product's own 16-bit rounding being 1.7e-3; tests/test_gpu_kernels.py)
 * at half of the largest epilogue stream of a training step. */
int simseg_gemm_aux_blocked_ok(int64_t M, int64_t N, int64_t K);

/* K14, the dense zero-shot segmentation map: out[m,c] = < x[m,:] / max(||x[m,:]||, eps), text[c,:] > for every patch row m
 * and every class c (C <= 256) in one pass over x, the row L2-normalisation (F.normalize, tools/seg_evaluation.py:112) fused
 * into the MFMA kernel; normalize=0 gives the plain x . text^T.  Replaces the per-class GEMV loop of
 * tools/seg_evaluation.py:128-139.  x[M,K], text[C,K] in `dtype` (0 fp32 exact, 1 bf16), out fp32 [M,C]. */
int simseg_patch_text_sim(const void* x, const void* text, float* out, int64_t M, int64_t C, int64_t K, int dtype, float eps,
                          int normalize, void* stream);

/* Kernel selection for benchmarking / tests (thread-local; production callers never call it).  Every value forces a choice among the
 * kernels the automatic dispatch itself uses, where that kernel applies to the call; where it does not, the call is dispatched as under 0:
 *   0  auto
 *   1  128x128 register-staged kernel
 *   3  256x256 ping-pong kernel, one tile per block (never the persistent kernel)
 *   4  small-problem kernel (32x64 / 64x64 tiles, intra-block split-K) wherever it applies
 *   5  128x128 tile on the four-stage direct-to-LDS ring (k-contiguous operands, K % 64 == 0, M, N >= 128, no split-K)
 *   10 persistent 256x256 ping-pong kernel wherever it applies (full tiles, more than one round, the epilogue kinds auto puts on it)
 * Any other value is an error and leaves the previous selection in force. */
int simseg_set_gemm_variant(int v);
/* Which of those kernels (1 / 3 / 4 / 5 / 10) the calling thread's last simseg_gemm launched. */
int simseg_gemm_last_variant(void);

/* A transformer block's split-K weight gradients as ONE launch of the 256x256 ping-pong kernel: n (1..8) problems
 * dW_i[out_i, in_i] += dY_i^T . X_i, dY_i [rows, out_i] and X_i [rows, in_i] in the selected 16-bit type, dW_i fp32 (zero-filled or holding
 * a partial sum), all over the same `rows`, each cut into the same `slices` K-slices.  problems: n host-side records of 8 x int64
 * {dY, X, dW, out, in, ld_dY, ld_X, ld_dW}.  Eligible when every out_i / in_i is a multiple of 256, rows % 64 == 0, the operands are
 * 16-byte aligned and rows / 64 / slices >= 16; otherwise nothing is launched, the call still returns 0, and simseg_wgrad_group_last()
 * reads 0 - the caller then issues per-problem simseg_gemm calls.  After a grouped launch simseg_gemm_last_variant() reads 3. */
int simseg_gemm_wgrad_group(const int64_t* problems, int n, int64_t rows, int slices, void* stream);
/* How many problems the calling thread's last simseg_gemm_wgrad_group launched as one group (0 = it fell back). */
int simseg_wgrad_group_last(void);

/* LayerNorm over the last dim of x[rows,D] (fp32 residual stream) -> y (out_dtype) and optionally a bf16 copy.
 * Saves mean/rstd when non-null.  Replaces nn.LayerNorm in timm Block.norm1/norm2/VisionTransformer.norm
 * (eps 1e-6) and HF Bert*Output.LayerNorm / BertEmbeddings.LayerNorm (eps 1e-12). */
int simseg_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int out_dtype, void* y_bf16,
                         float* mean, float* rstd, int64_t rows, int64_t D, float eps, void* stream);
/* dx = LN'(dy_bf16 + dy_f32) + dres + dres_bf16; writes dx_f32 and/or dx_bf16 (the bf16 copy optionally with the dropout mask
 * (drop_seed, drop_p) of the producing dense layer re-applied); dgamma/dbeta and dxsum (column sums of dx_bf16's values,
 * optional) are ACCUMULATED.  dres_bf16 (round 4, optional): the residual-stream gradient as the 16-bit copy the previous
 * call wrote - in the 16-bit training modes the ViT blocks hand it from LayerNorm backward to LayerNorm backward in that form
 * and no fp32 image of it is written (dx_f32 = NULL): every GEMM that consumes it reads 16-bit operands anyway.
 * y_bf16 + beta (round 4, optional): the layer's saved 16-bit OUTPUT y = xhat * gamma + beta; the normalised value xhat is then taken from it
 * ((y - beta) / gamma) instead of from the fp32 input x for every 4-channel chunk with |gamma| >= 0.05 and |beta| <= 4 |gamma| (half the bytes
 * of the kernel's largest read); the other chunks - and everything when y_bf16 is NULL - read x, which must always be given. */
int simseg_layernorm_bwd(const void* dy_bf16, const float* dy_f32, const float* dres, const void* dres_bf16, const float* x,
                         const void* y_bf16, const float* beta, const float* mean,
                         const float* rstd, const float* gamma, float* dx_f32, void* dx_bf16, float* dgamma,
                         float* dbeta, float* dxsum, float* partials, int64_t rows, int64_t D, uint64_t drop_seed, float drop_p,
                         void* stream);
/* Bytes of the `partials` workspace of simseg_layernorm_bwd: per-block column sums, folded by a second small kernel
 * (one add per column) instead of one atomic per column per block.  partials = NULL selects the atomic path. */
int64_t simseg_layernorm_bwd_workspace_bytes(int64_t rows, int64_t D);

/* out[n] += sum_r in[r,n]  (bias / embedding-table gradients). */
int simseg_colsum_accum(const void* in, int in_dtype, float* out, int64_t rows, int64_t N, int64_t ld, void* stream);

/* timm PatchEmbed (Conv2d 3->D, k16 s16) as a GEMM: gathers image[B,3,H,W] into cols[B*N,768] in (c,kh,kw) order. */
int simseg_vit_im2col(const float* image, void* cols, int out_dtype, int64_t B, int64_t H, int64_t W, void* stream);
/* x[b,0,:] = cls + pos[0] (vit_builder.py:15-17) and its gradient dcls += sum_b dx[b,0,:]. */
int simseg_vit_cls_rows(const float* cls, const float* pos, float* x, int64_t B, int64_t T, int64_t D, void* stream);
int simseg_vit_cls_grad(const float* dx, float* dcls, int64_t B, int64_t T, int64_t D, void* stream);

/* Patch dropout of the image tower (csrc/patchdrop.hip; DESIGN.md "Patch dropout"): during training every image keeps a random subset of
 * K of its N patch tokens (timm's PatchDropout, ordered, one prefix token) and the tower runs on [cls] + the kept ones.  All four entry
 * points check their arguments on the host before any device work: null pointers, 1 <= K <= N <= 4096, B >= 1, B * N < 2^31, and where
 * they apply H, W positive multiples of 16 with (H / 16) * (W / 16) <= 4096 and D a positive multiple of 4.
 *
 * The draw.  keep[B, K] and inv[B, N] (int32) are a pure function of (seed, b, N, K): key(b, n) = hash_u32(seed, b * N + n) (csrc/common.h;
 * simseg_amd.pipeline.hash_u32_ref in numpy); image b keeps the K positions with the smallest keys, equal keys going to the lower n (for a
 * fixed seed the hash is a bijection of 32-bit indices, so with B * N < 2^31 there are none); keep[b, 0] < ... < keep[b, K - 1];
 * inv[b, n] = the j with keep[b, j] == n, or -1 for a dropped position.  Every K-subset is equally likely as far as the keys are
 * independent uniform words.  One block per image: keys in LDS, the rank of a key by counting the smaller ones, the slot j by a
 * block-wide prefix count of the kept positions below n - no sort, no host read. */
int simseg_patch_keep_sample(int32_t* keep, int32_t* inv, int64_t B, int64_t N, int64_t K, uint64_t seed, void* stream);
/* simseg_vit_im2col of the kept patches only: cols[b * K + j, :] = patch keep[b, j] of image b in (c, kh, kw) order, out_dtype 0 fp32 /
 * 1 the selected 16-bit type (the same rounding as simseg_vit_im2col: the bits of that call's rows, selected).  A keep entry outside
 * [0, (H / 16) * (W / 16)) gives a zero row and reads nothing. */
int simseg_vit_im2col_keep(const float* image, const int32_t* keep, void* cols, int out_dtype, int64_t B, int64_t H, int64_t W, int64_t K,
                           void* stream);
/* The rest of the token embedding, in place on the fp32 stream x[B, 1 + K, D] whose patch rows hold fl(acc + bias) (simseg_gemm with bias
 * and row_group = K, no residual): x[b, 0] = cls + pos[0];  x[b, 1 + j] += pos[1 + keep[b, j]] (pos [N + 1, D]) - the two fp32 additions
 * of the full path's epilogue (+ bias, + residual) in the same order.  A keep entry outside [0, N) leaves its row as it is. */
int simseg_vit_keep_rows(const float* cls, const float* pos, const int32_t* keep, float* x, int64_t B, int64_t N, int64_t K, int64_t D,
                         void* stream);
/* Gradient of the position table - and of [cls], its row 0 - from dx[B, 1 + K, D] (dx_dtype 0 fp32 / 1 the selected 16-bit type: the
 * gradient or its 16-bit shadow).  Writes ALL N + 1 rows of fp32 dpos[N + 1, D] (nothing is accumulated, the buffer need not be zeroed):
 *   dpos[0]     = sum_b dx[b, 0],
 *   dpos[1 + n] = sum over the images b with inv[b, n] >= 0 of dx[b, 1 + inv[b, n]];   a position no image kept: exactly 0.
 * Every sum is one fp32 accumulator per element that takes its terms in ascending b - the order is part of the contract, so the result is
 * a function of the inputs alone (no atomics, nothing depends on how blocks are scheduled).  An inv entry >= K counts as dropped. */
int simseg_vit_keep_pos_grad(const void* dx, int dx_dtype, const int32_t* inv, float* dpos, int64_t B, int64_t N, int64_t K, int64_t D,
                             void* stream);

/* HF BertEmbeddings: out[b,l,:] = word[ids[b,l]] + pos[l] + type[0] (LayerNorm is a separate call).
 * bwd: dword[ids] += dsum for unmasked tokens (masked tokens carry an exactly-zero gradient). */
int simseg_bert_embed_fwd(const int64_t* ids, const float* word, const float* pos, const float* type0, float* out,
                          int64_t B, int64_t L, int64_t D, int64_t vocab, void* stream);
int simseg_bert_embed_bwd(const int64_t* ids, const int64_t* mask, const float* dsum, float* dword, int64_t B, int64_t L,
                          int64_t D, int64_t vocab, void* stream);

/* LoDA pooling + L2norm: emb[b,:] = l2norm(mean over the k largest tokens per channel) with the reference's
 * -10000 overwrite of masked tokens.  simseg/models/components/pooling.py:52-65 + normalization.py:6-11
 * (pipelines/clip.py:87-93,111-120).  idx[B,k,P] and norm[B] are saved for the backward.  normalize=0 returns the
 * pooled vector itself (TopKPooling used on its own). */
int simseg_topk_pool_l2norm_fwd(const void* tok, int dtype, const int64_t* mask, float* emb, int32_t* idx, float* norm,
                                float* scratch, int64_t B, int64_t N, int64_t P, int k, float eps, int normalize, void* stream);
/* bytes of the optional `scratch` workspace: with it the tokens of an image are scanned by 32 blocks in parallel and merged (same
 * result, ties included) - for small batches, where one block per image leaves the GPU empty; NULL = one block per image. */
int64_t simseg_topk_pool_workspace_bytes(int64_t B, int64_t P, int k);
int simseg_topk_pool_l2norm_bwd(const float* demb, const float* emb, const float* norm, const int32_t* idx, void* dtok,
                                int dtype, int64_t B, int64_t N, int64_t P, int k, float eps, int normalize, void* stream);

/* Kernel selection for benchmarking / tests (thread-local, consumed by the host-side dispatch only): 0 auto (16-bit sequences of <= 256
 * tokens run the "resident" kernels that hold a whole head's operands in LDS; unmasked ones of >= 512 tokens the 64-queries-per-wave
 * forward), 1 = the streaming ring kernels wherever they apply, 6 / 7 = the 64-queries-per-wave forward with one / two query blocks per
 * wave (unmasked sequences of >= 65 tokens).  Every value selects between production kernels; any other value is an error and leaves
 * the previous selection in force. */
int simseg_set_attention_variant(int v);
/* debug (thread-local): the one-kernel backward writes 4 x uint64 per block (start / operands landed / tile loop done / end, 100 MHz wall
 * clock); NULL switches it off. */
int simseg_debug_attn_trace(void* buf);
/* debug (thread-local): the per-tile ping-pong GEMM kernel writes 5 x uint64 per block into buf (wall-clock stamps at 100 MHz of block
 * start, K loop start, K loop end, block end; HW_ID) - tools/dbg_gemm_trace.py, tools/dbg_wgrad_trace.py; NULL switches it off.  A traced
 * call never runs on the persistent kernel. */
int simseg_debug_gemm_trace(void* buf);

/* Fused softmax attention, head_dim 64, from the packed projection qkv[B,T,3,H,64] to ctx[B,T,H*64].
 * key_mask[B,T] (1 = attend, 0 = padding; may be NULL) reproduces HF's additive key-padding mask; lse[B,H,T]
 * (log2 domain, optional) is saved for the backward.  dtype 0 = exact fp32 MFMA, 1 = bf16 MFMA.  drop_p > 0 applies
 * HF attention_probs dropout.  Replaces timm Attention.forward (q@k^T*scale, softmax, @v) and HF
 * BertSelfAttention.forward as reached through vit_builder.py:18 / huggingface_builder.py:16-17.
 * A sequence with NO unmasked key gets finite but otherwise unspecified out / lse / dqkv: the kernels add -1e30 to a masked score rather
 * than HF's -10000, so in such a row the tile-padding keys behind T carry weight too (the reference's tokenizer never produces one: every
 * caption has its [CLS]). */
/* skip_padded_rows (bf16, T <= 256, with a key mask): the caller neither reads the outputs nor uses the gradients of the rows past a
 * sequence's last unmasked key (the packed text tower): the kernels then work on 1 + that key's index rows of each sequence only and
 * leave the other rows of out / lse / dqkv untouched. */
int simseg_attention_fwd(const void* qkv, const int64_t* key_mask, void* out, float* lse, int dtype, int64_t B, int64_t T,
                         int64_t H, float scale, uint64_t drop_seed, float drop_p, int skip_padded_rows, void* stream);
/* The same forward for long 16-bit sequences (T >= 512, no mask, no dropout: timm Attention.forward at img_size 384 / 512,
 * vit_builder.py:18 via pipelines/clip.py:193-194) on a projection whose q columns already carry scale * log2(e): the caller folds the
 * factor into the q rows of Attention.qkv's weight and bias BEFORE rounding them to 16 bits, so q * scale is rounded once - exactly as q
 * alone would have been - and the kernel's exponent is the MFMA output itself (no multiply per score). */
int simseg_attention_fwd_qscaled(const void* qkv, void* out, float* lse, int64_t B, int64_t T, int64_t H, void* stream);
/* Backward: dqkv[B,T,3,H,64] from qkv, ctx, dctx and lse, all in `dtype` (0 = fp32: the exact mode of a non-AMP run,
 * simseg/core/hooks/optimizer.py:76-77; 1 = bf16).  workspace: caller-provided fp32 scratch of simseg_attention_bwd_workspace_bytes(B, T, H).
 * dqkv_colsum (optional, [3*H*64] fp32) += column sums of dqkv over all B*T rows: the bias gradient of the q/k/v projection (timm
 * Attention.qkv.bias, HF BertSelfAttention.{query,key,value}.bias), formed inside the one-kernel bf16 backward (T <= 256) and by a
 * column-sum pass over dqkv otherwise. */
int64_t simseg_attention_bwd_workspace_bytes(int64_t B, int64_t T, int64_t H);
int simseg_attention_bwd(const void* qkv, const int64_t* key_mask, const void* out, const void* dout, const float* lse,
                         float* workspace, void* dqkv, float* dqkv_colsum, int dtype, int64_t B, int64_t T, int64_t H, float scale,
                         uint64_t drop_seed, float drop_p, int skip_padded_rows, void* stream);

/* The same attention for a ragged batch stored WITHOUT its padding (bf16, at most T <= 256 tokens per sequence): sequence b is rows
 * [row_start[b], row_start[b+1]) of qkv [rows,3,H,64] / out, dout [rows,H*64] / dqkv (row_start: B+1 ascending int32 on the device),
 * every stored token is real.  Attention has no notion of position, so this IS HF BertSelfAttention with its key-padding mask
 * (huggingface_builder.py:16-17) evaluated on the unmasked tokens; the rows a padded layout would carry are never formed.  lse
 * [B,H,T] (log2 domain).  Rows outside every sequence (a caller's tile padding) are not touched.  workspace / dqkv_colsum as in
 * simseg_attention_bwd. */
int simseg_attention_fwd_rows(const void* qkv, const int32_t* row_start, void* out, float* lse, int64_t B, int64_t T, int64_t H, float scale,
                              uint64_t drop_seed, float drop_p, void* stream);
int simseg_attention_bwd_rows(const void* qkv, const int32_t* row_start, const void* out, const void* dout, const float* lse,
                              float* workspace, void* dqkv, float* dqkv_colsum, int64_t B, int64_t T, int64_t H, float scale, uint64_t drop_seed,
                              float drop_p, void* stream);

/* The same attention on PLANE-MAJOR projection operands (round 4; 16-bit, T <= 256): qkv / dqkv are [3*H][plane_rows][64] - plane
 * which*H + h holds the 64 channels of head h of q (which = 0), k (1) or v (2) of every token row, i.e. the packed projection
 * [rows,3,H,64] with the (3,H) axes moved in front of the rows.  It is what simseg_gemm writes with c_planes = plane_rows and reads with
 * a_planes (the A operand's K-tiles are the planes), so the layout never leaves the three kernels; a head's operand rows are one
 * contiguous run instead of T cache lines 6*H*64 bytes apart.  Sequence b = rows [b*T, (b+1)*T) when row_start is NULL (timm
 * Attention.forward, vit_builder.py:18), else [row_start[b], row_start[b+1]) as in simseg_attention_fwd_rows (HF BertSelfAttention,
 * huggingface_builder.py:16-17).  out / dout [rows,H*64], lse [B,H,T], workspace / dqkv_colsum as in simseg_attention_bwd. */
int simseg_attention_fwd_planes(const void* qkv, int64_t plane_rows, const int32_t* row_start, void* out, float* lse, int64_t B, int64_t T,
                                int64_t H, float scale, uint64_t drop_seed, float drop_p, void* stream);
int simseg_attention_bwd_planes(const void* qkv, int64_t plane_rows, const int32_t* row_start, const void* out, const void* dout,
                                const float* lse, float* workspace, void* dqkv, float* dqkv_colsum, int64_t B, int64_t T, int64_t H,
                                float scale, uint64_t drop_seed, float drop_p, void* stream);

/* Prompt ensemble of the zero-shot classifier: out[s,:] = normalize(mean over the P prompt embeddings x[s,:,:]).
 * tools/seg_evaluation.py:71-73 (class_embeddings.mean(dim=0); /= norm()).  A zero mean yields NaN, as the reference's division does. */
int simseg_segment_mean_l2norm(const float* x, float* out, int64_t S, int64_t P, int64_t D, void* stream);

/* rnorm[r] = 1 / max(||x_r||_2, eps): the F.normalize of tools/seg_evaluation.py:112 as a GEMM row scale. */
int simseg_row_rnorm(const void* x, int dtype, float* rnorm, int64_t rows, int64_t D, float eps, void* stream);

/* InfoNCE rows over sims[N1,N2] = feat1 . feat2_global^T (fp32, from simseg_gemm): z = s / clamp(T,1e-3,0.5),
 * per-row cross-entropy against target column target0 + i with optional label smoothing and ignore weights, top-1
 * hit, and (write_grad) dLoss/ds written IN PLACE over sims.  out3 = {loss, top-1 acc, dLoss/dT}.
 * Top-1 rule: the FIRST index attaining the row maximum is the prediction - a target tied with an earlier column is a miss, a target
 * tied only with later columns is a hit.
 * simseg/models/criteria/losses/mml_loss.py:56,73-77,89-95 (+ :350-376 LabelSmoothingCrossEntropy,
 * simseg/utils/misc.py:462-478 calc_topk_accuracy). */
int simseg_nce_rows(float* sims, const float* temperature, const float* ignore_mask, float* row_loss, float* row_correct,
                    float* row_tdot, float* out3, int64_t N1, int64_t N2, int64_t target0, float smoothing, int write_grad,
                    void* stream);
/* y[r,:] = alpha * x[r,:] * (one_minus ? 1 - s[r] : s[r])  -- feat2_global * (1 - ignore_mask), mml_loss.py:70-71. */
int simseg_scale_rows(const float* x, const float* s, float* y, int64_t rows, int64_t D, int one_minus, float alpha, void* stream);

/* y[i] = alpha * scalar[0] * x[i] with the scalar read on the device (upstream loss gradient, no host sync). */
int simseg_scale_by_scalar(const float* x, const float* scalar, float* y, int64_t n, float alpha, void* stream);

/* Both directions of the CLIP loss (simseg/models/pipelines/clip.py:129-140: 0.5 * (NCE(image, text) + NCE(text, image)), each as
 * simseg_nce_rows without an ignore mask) in two launches: sims2 = the two [N1, N2] similarity blocks stacked (image -> text first), overwritten
 * by their gradients w.r.t. the similarities when write_grad; row_scratch: 6 * N1 floats; out4 = {loss, i2t top-1 acc, t2i top-1 acc,
 * dLoss/dTemperature}. */
int simseg_nce_pair(float* sims2, const float* temperature, float* row_scratch, float* out4, int64_t N1, int64_t N2, int64_t target0,
                    float smoothing, int write_grad, void* stream);
/* MixUpNCE rows (mml_loss.py:146-197): simseg_nce_rows with TWO target columns per row, a = target0 + i and b = target0 + (N1 - 1 - i)
 * (targets.flip(0)), and the weight alpha_i = alpha[i * alpha_stride] read on the device (alpha_stride 0: one scalar for every row,
 * 1: a vector of N1; no host read either way):
 *   loss_i = (1 - eps) * (alpha_i * nll_a + (1 - alpha_i) * nll_b) + eps * smooth_i,
 *   dz_ij  = p_ij - eps / N2 - (1 - eps) * (alpha_i [j == a] + (1 - alpha_i) [j == b])     (a == b, the middle row of an odd N1: both
 *            terms land on that column).
 * Ignore weights, the mean over N1, dLoss/dT, z as the same rounded product in every pass, differences from the row maximum before the
 * logarithm and the top-1 hit (against a, first-index rule) are simseg_nce_rows'.  out3 = {loss, top-1 acc, dLoss/dT}.  The same kernel
 * instantiated with the mix terms: at alpha = 1 every output equals simseg_nce_rows' bit for bit (products with 1 and sums with 0 are
 * exact).  alpha_stride outside {0, 1} and targets outside [0, N2) are refused before a launch. */
int simseg_mix_nce_rows(float* sims, const float* temperature, const float* ignore_mask, const float* alpha, int alpha_stride,
                        float* row_loss, float* row_correct, float* row_tdot, float* out3, int64_t N1, int64_t N2, int64_t target0,
                        float smoothing, int write_grad, void* stream);
/* Triplet rows: the max-violation hinge of VSE++ (mml_loss.py:280-347) over `blocks` (1 or 2) stacked sims[N1,N2] (fp32, from
 * simseg_gemm), one block per row.  For row i of a matrix, with d_i = s[i, target0 + i]:
 *   pre_ij  = fl32(fl32(margin + s_ij) - d_i)      two rounded fp32 operations in torch's order, never contracted;
 *   cost_ij = max(pre_ij, 0), and 0 at masked columns;
 *   mask_block = 1 (the reference's global_reduce branch): the whole own-rank block [target0, target0 + N1) is masked - the reference's
 *     behaviour, quirk included: with ONE rank (N2 == N1) every column is masked, and the loss and all gradients are exactly 0;
 *   mask_block = 0 (the local branch): only column target0 + i is masked;
 *   reduce = 0 ("mean"): rowloss_i = sum_j cost_ij / (N1 - 1);   reduce = 1 ("max"): rowloss_i = max_j cost_ij, its arg the FIRST unmasked
 *     column attaining the maximum;
 *   top-1 hit over ALL columns against target0 + i with simseg_nce_rows' first-index rule (the same quantity it returns).
 * write_grad: the row is overwritten IN PLACE by d rowloss_i / d s_ij.  Gradient flows through the clamp iff pre_ij > 0, which deviates
 * from torch's subgradient (clamp(min=0) passes it where pre_ij >= 0) only at pre_ij == 0 exactly:
 *   mean: fl32(1 / (N1 - 1)) at every unmasked j with pre_ij > 0 and fl32(-count_i / (N1 - 1)) at the target column (count_i = the number
 *         of such j; each entry ONE rounded division, 0 when count_i = 0);
 *   max:  +1 at the arg and -1 at the target column if the maximum is > 0, otherwise a zero row.
 * A second launch gives out = {sum_i rowloss_i, top-1 acc} (blocks = 1) or {the sum over both matrices' rows, acc of matrix 0, acc of
 * matrix 1} (blocks = 2, row i of matrix i / N1): the loss is a SUM over rows, not a mean, as in the reference.  row_loss / row_correct:
 * blocks * N1 floats each.  Refused before any launch: N1 < 1, target0 + N1 > N2, reduce outside {0, 1}, blocks outside {1, 2}, and
 * N1 < 2 with the mean (the reference's / (N1 - 1) would give NaN). */
int simseg_triplet_rows(float* sims, float* row_loss, float* row_correct, float* out, int64_t N1, int64_t N2, int64_t target0, float margin,
                        int reduce, int mask_block, int blocks, int write_grad, void* stream);
/* SigLIP rows: the pairwise sigmoid loss of Zhai et al. (ICCV'23; open_clip's SigLipLoss) over sims[N1,N2] (fp32, from simseg_gemm), one
 * block per row, fp32 only.  Every (row, column) pair is a binary problem - no row-wise softmax.  For row i, with tgt = target0 + i,
 * temp = clamp(T, 1e-3f, 0.5f) (temperature[0] = T; the fp32 constants of simseg_nce_rows), inv_t = fl32(1 / temp), b = bias[0]:
 *   z_ij = fl32(fl32(s_ij * inv_t) + b)            a rounded product and a rounded sum, never contracted;
 *   y_ij = +1 at j == tgt, otherwise -1;   x_ij = -y_ij * z_ij;   e_ij = exp(-|x_ij|)
 *   l_ij = softplus(x_ij) = -log sigmoid(y_ij z_ij) = max(x_ij, 0) + log1p(e_ij)      (log1p: the small e_ij of the negatives keep
 *          their low bits; e <= 1 and underflows to 0, so nothing overflows at |z| ~ 1000)
 *   rowloss_i = sum_j l_ij;   loss = (1 / N1) * sum_i rowloss_i                      (SigLIP's normalisation by the LOCAL batch)
 *   dz_ij = -y_ij * sigmoid(x_ij) / N1,  sigmoid(x) = x >= 0 ? 1 / (1 + e) : e / (1 + e)  from the same e
 *   write_grad: the row is overwritten IN PLACE by dLoss/ds_ij = dz_ij * inv_t; write_grad = 0 leaves sims bit for bit and gives the
 *   same out4[0:2] and row losses
 *   row_tdot_i = sum_j dz_ij * s_ij;   row_bdot_i = sum_j dz_ij
 *   top-1 hit: the FIRST index attaining the row maximum of s itself (z is increasing in s) against tgt - simseg_triplet_rows' rule.
 * A second, one-block launch sums the rows in a fixed order (no atomics: the same input gives the same bits):
 *   out4 = {loss, top-1 acc = hits / N1, dLoss/dT, dLoss/db},
 *   dLoss/dT = -sum_i row_tdot_i / temp^2 when 1e-3f <= T <= 0.5f and exactly 0 outside the clamp (as simseg_nce_rows),
 *   dLoss/db = sum_i row_bdot_i, always.
 * row_loss / row_correct / row_tdot / row_bdot: N1 floats each.  Refused before any launch: N1 < 1, N2 < 1, target0 < 0,
 * target0 + N1 > N2 and N2 >= 2^31 (the kernel's column and row indices are 32-bit). */
int simseg_siglip_rows(float* sims, const float* temperature, const float* bias, float* row_loss, float* row_correct, float* row_tdot,
                       float* row_bdot, float* out4, int64_t N1, int64_t N2, int64_t target0, int write_grad, void* stream);
/* NT-Xent rows: the normalised temperature-scaled cross-entropy of SimCLR (Chen et al., ICML'20) in the global form of SLIP's SIMCLRLoss
 * (Mu et al., ECCV'22) over sims[N1,N2] (fp32, from simseg_gemm), one block of 256 threads per row, fp32 only.  N1 = 2B is even: rows
 * [0, B) are view a and rows [B, 2B) view b of the local batch, the columns are the gathered stacked embeddings, and this rank's own 2B
 * rows are columns [target0, target0 + N1).  It is simseg_nce_rows over that block with two changes: the row's own column takes no part,
 * and the positive sits half a block away.  For row i, with temp = clamp(T, 1e-3f, 0.5f) (temperature[0] = T; the fp32 constants of
 * simseg_nce_rows) and inv_t = fl32(1 / temp):
 *   self_i = target0 + i;   pos_i = target0 + (i + B) mod N1
 *   z_ij = fl32(s_ij * inv_t)                      the same rounded product in every pass, never contracted into a subtraction
 *   m_i  = max over j != self_i of z_ij;   lg_i = log(sum over j != self_i of exp(z_ij - m_i))
 *          (the self column - its value is 1.0, always the row maximum - is in neither: it is never read as a value that matters)
 *   rowloss_i = (m_i - z_i,pos) + lg_i             the difference from the maximum first, then the small logarithm (simseg_nce_rows)
 *   loss = (1 / N1) * sum_i rowloss_i
 *   dz_ij = (p_ij - [j == pos_i]) / N1 with p_ij = exp((z_ij - m_i) - lg_i) for j != self_i, and exactly 0 at j == self_i
 *   write_grad: the row is overwritten IN PLACE by dLoss/ds_ij = dz_ij * inv_t; write_grad = 0 leaves sims bit for bit and gives the
 *   same out4[0:3] and row losses
 *   row_tdot_i = sum_j dz_ij * s_ij
 *   top-1 hit: the FIRST index attaining m_i among j != self_i, against pos_i - simseg_nce_rows' rule.
 * A second, one-block launch sums the rows in a fixed order (no atomics: the same input gives the same bits):
 *   out4 = {loss, acc_a = hits of rows [0, B) / B, acc_b = hits of rows [B, 2B) / B, dLoss/dT},
 *   dLoss/dT = -sum_i row_tdot_i / temp^2 when 1e-3f <= T <= 0.5f and exactly 0 outside the clamp.
 * No label smoothing and no ignore mask.  row_loss / row_correct / row_tdot: N1 floats each.  Refused before any launch: N1 < 2, N1 odd,
 * target0 < 0, target0 + N1 > N2 and N2 >= 2^31 (the kernel's column and row indices are 32-bit). */
int simseg_ntxent_rows(float* sims, const float* temperature, float* row_loss, float* row_correct, float* row_tdot, float* out4, int64_t N1,
                       int64_t N2, int64_t target0, int write_grad, void* stream);
/* n <= 6 fp32 transposes in ONE launch (out[k][c, r] = in[k][r, c], in[k] [rows[k], cols[k]] contiguous); jobs with scale[k] != 0 are
 * multiplied by alpha * scalar[0] - in the transposed copy and IN PLACE; y0[0] = scalar[0] * x0[0] when y0 is given.  The loss head's
 * backward (mml_loss.py:73 differentiated) needs dS, dS^T and the transposed embeddings as row . row GEMM operands, all times the upstream
 * gradient: one launch instead of the round-3 head's four transposes and three scale passes per direction. */
int simseg_transpose_multi(const void* const* in, void* const* out, const int64_t* rows, const int64_t* cols, const int32_t* scale, int64_t n,
                           const float* scalar, float alpha, const float* x0, float* y0, void* stream);
/* Retrieval: rank[i] = #{j : sim_ij > max_{j': gid match} sim_ij'}, has_match[i] = any gid match.  Equals the
 * argsort/gather/first-match rank of simseg/tasks/clip/hooks/utils.py:36-42,64-66 on tie-free scores. */
int simseg_retrieval_rank(const float* sim, const int64_t* left_gid, const int64_t* right_gid, int32_t* has_match, int32_t* rank,
                          int64_t M, int64_t N, int64_t ld, void* stream);
/* The reverse direction from the SAME matrix: column j retrieves rows (best = max over rows with row_gid == col_gid[j], rank = rows
 * scoring strictly higher) - two row-major passes instead of a second GEMM on swapped operands.  scratch: N int32. */
int simseg_retrieval_rank_cols(const float* sim, const int64_t* row_gid, const int64_t* col_gid, int32_t* has_match, int32_t* rank,
                               int32_t* scratch, int64_t M, int64_t N, int64_t ld, void* stream);
/* counts4 = {#has_match, #rank<b0, #rank<b1, #rank<b2}  (hooks/utils.py:69-71). */
int simseg_recall_counts(const int32_t* has_match, const int32_t* rank, int64_t M, int b0, int b1, int b2, int32_t* counts4,
                         void* stream);

/* Fused top-K retrieval search (search.hip): score[m, j] = the j-th largest <q[m,:], g[n,:]> over n, idx[m, j] = n + index_offset, rows
 * ordered by descending score and equal scores by ascending index - the first K columns of a stable descending argsort of q @ g^T
 * (EmbANN._ann, simseg/tasks/clip/hooks/utils.py) - without the M x N matrix: the score tiles stay in MFMA accumulators and only values
 * that beat a row's running K-th best leave them (into a per-row candidate list in LDS).  q [M, D] / g [N, D] row-major with leading
 * dimensions ldq / ldg (elements), both in `dtype`: 0 = fp32 operands and products, 1 = bf16 operands, exact products, fp32 accumulation
 * (always bf16: this entry point has no fp16 flavour).  1 <= K <= 128, D % 8 == 0, 16-byte aligned rows.  N < K: the tail slots hold
 * -inf / -1.  Inputs are taken to be finite; -0.0 scores are returned as +0.0.  When M has too few row tiles to fill the chip the gallery
 * is split over blocks and the partial lists (in `workspace`, simseg_topk_search_workspace_bytes: 8 * M * K bytes per column split, 0
 * when there is one) are merged by a second launch.  Bit-reproducible: the result does not depend on the order in which lanes append. */
int64_t simseg_topk_search_workspace_bytes(int64_t M, int64_t N, int64_t D, int K, int dtype);
int simseg_topk_search(const void* q, const void* g, int dtype, int64_t M, int64_t N, int64_t D, int64_t ldq, int64_t ldg, int K,
                       int64_t index_offset, float* score, int32_t* idx, void* workspace, int64_t workspace_bytes, void* stream);
/* The same merge for two finished lists [M, K] (score descending, idx < 0 = empty slot): the K best of their union under the same order.
 * A gallery larger than memory goes through simseg_topk_search in chunks with index_offset and is reduced with this. */
int simseg_topk_merge(const float* score_a, const int32_t* idx_a, const float* score_b, const int32_t* idx_b, float* score, int32_t* idx,
                      int64_t M, int K, void* stream);

/* Weighted k-nearest-neighbour vote (knn.hip) over the lists of simseg_topk_search / simseg_topk_merge: score [M, K] fp32 descending,
 * idx [M, K] int32 with -1 (and -inf) in empty tail slots, 1 <= K <= 128.  gallery_label [N] int32 (>= 0) is gathered by the kernel:
 * entry j of a row has the label gallery_label[idx[j]].  The row's valid entries are those before its first empty slot; an index outside
 * [0, N) ends the list like an empty slot.  ks (HOST pointer): nk = 1..4 strictly ascending neighbourhood sizes, ks[nk - 1] <= K, all
 * answered by one launch - the neighbours of size k are the first n = min(k, valid) entries, a prefix of the one sorted list.
 * Per row and k, in fp32:
 *   w_j = expf((s_j - s_0) / temperature)              (relative to the best neighbour: <= 1 at every temperature, no ranking changes),
 *   vote(c) = sum of w_j over j < n with label c, ADDED IN ASCENDING j starting from 0 (the order is part of the contract: the result
 *             does not depend on lanes or launch geometry),
 *   classes with at least one neighbour, ranked by vote descending and equal votes by ascending class:
 *   pred[ki, m, r] = the r-th class, vote[ki, m, r] = its vote, r < 5; -1 / 0 where the row has fewer than five classes.
 * pred [nk, M, 5] int32, vote [nk, M, 5] fp32.  query_label [M] int32 or NULL; when given, counts [nk, 3] int64 +=
 * {rows, rows with pred[.., 0] == label, rows with the label among pred[.., :5]} by integer atomics (exact, order-free): the caller
 * zeroes counts and may accumulate over calls.  A row without a valid neighbour counts as a row and as two misses.  temperature > 0 and
 * finite.  Refused before any device work: K, nk / ks, temperature, M < 0, N < 1 or N >= 2^31, null pointers. */
int simseg_knn_vote_rows(const float* score, const int32_t* idx, const int32_t* gallery_label, const int32_t* query_label, int64_t M,
                         int64_t N, int K, const int32_t* ks, int nk, float temperature, int32_t* pred, float* vote, int64_t* counts,
                         void* stream);

/* ---- optimizer steps and gradient checks (csrc/optim.hip; the 16-bit copies are written in the selected 16-bit type) ----------------
 * torch.optim.AdamW (configs/clip/simseg.vit-b.yaml:31-36) over a flat fp32 segment; refreshes the bf16 compute copy. */
int simseg_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int64_t step, float grad_scale, void* stream);

/* Same update for every parameter tensor in ONE launch.  table[t] = six 8-byte words {p, g, m, v, p16, (float lr, float wd)}: five
 * device pointers (p16 = bf16 compute copy to refresh, or 0) and the tensor's own learning rate / weight decay packed as two floats
 * (the reference's ClipOptimizerHook makes one param group per parameter, tasks/clip/hooks/optimizer.py:18-36); sizes[t] elements;
 * chunk c covers [chunk_off[c], chunk_off[c]+chunk) of tensor chunk_tid[c]. */
int simseg_adamw_multi_step(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                            int64_t n_chunks, int chunk, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                            void* stream);

/* The same launch inside the reference's fp16 AMP iteration (clip_runner.py:226-230; core/hooks/optimizer.py:73-82: scaler.scale(loss)
 * .backward(), scaler.step(optimizer), scaler.update()) WITHOUT the host read torch's scaler.step makes for an optimizer that cannot skip
 * a step by itself: loss_scale / found_inf are torch.amp.GradScaler's device tensors (its `optimizer.grad_scale` / `optimizer.found_inf`
 * contract; either may be null).  Gradients are used as g * grad_scale / loss_scale[0]; when found_inf[0] != 0 nothing is updated.  The
 * count of steps actually taken lives on the device: step_in[0] is read, step_out[0] = step_in[0] + (skipped ? 0 : 1) is written (two
 * distinct slots) and supplies the bias corrections. */
int simseg_adamw_multi_step_amp(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                int64_t n_chunks, int chunk, float beta1, float beta2, float eps, float grad_scale,
                                const float* loss_scale, const float* found_inf, const float* step_in, float* step_out, void* stream);
/* found_inf[0] = 1 if any gradient element addressed by the table (same layout as above; only the g pointers are read) is inf / nan,
 * else unchanged: GradScaler's overflow check (torch._amp_foreach_non_finite_check_and_unscale_ with inverse scale 1) as one read-only
 * launch; the unscaling rides on simseg_adamw_multi_step_amp. */
int simseg_grads_nonfinite(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off, int64_t n_chunks,
                           int chunk, float* found_inf, void* stream);

/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, as the reference's OptimizerHook applies it: core/hooks/optimizer.py:45-47)
 * over the same tensor table, without touching the gradients: a read-only norm pass, a one-block finish, and AdamW launches that multiply
 * every gradient element by the coefficient the finish left on the device.  Nothing is read on the host.
 * simseg_grads_norm_partials: partials[c] = sum of g^2 (norm_type 2, fp32) or max |g| (norm_type 0 = infinity) over chunk c, one block
 * per chunk, one plain store per block, no atomics (bit-reproducible); inf / nan propagate.  The caller offsets `partials` per bucket.
 * simseg_grads_norm_finish: reduces n_partials values in double precision.  out2[0] = total norm (sqrt of the sum for type 2), divided
 * by loss_scale[0] when loss_scale is not null - the norm of the unscaled gradients; out2[1] = min(1, max_norm / (out2[0] + 1e-6)). */
int simseg_grads_norm_partials(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off, int64_t n_chunks,
                               int chunk, int norm_type, float* partials, void* stream);
int simseg_grads_norm_finish(const float* partials, int64_t n_partials, int norm_type, float max_norm, const float* loss_scale, float* out2,
                             void* stream);
/* simseg_adamw_multi_step / simseg_adamw_multi_step_amp with every gradient element also multiplied by grad_coef[0] (a device scalar:
 * out2 + 1 of simseg_grads_norm_finish), after grad_scale and after the division by the loss scale: unscale, clip, update. */
int simseg_adamw_multi_step_clip(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                 int64_t n_chunks, int chunk, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                                 const float* grad_coef, void* stream);
int simseg_adamw_multi_step_amp_clip(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                                     int64_t n_chunks, int chunk, float beta1, float beta2, float eps, float grad_scale,
                                     const float* loss_scale, const float* found_inf, const float* step_in, float* step_out,
                                     const float* grad_coef, void* stream);

/* ---- linear-probe task (loss rows: csrc/probe.hip, LARS: csrc/optim.hip; DESIGN.md "Linear probe") ------------------------------
 * Cross-entropy over integer class labels, top-k hits and the logit gradient in one pass over logits [B, C] (dt: 0 fp32, 1 the selected
 * 16-bit type; labels int64 on the device): nn.CrossEntropyLoss(reduction='mean') + accuracy(topk=(1, 5)) of the reference's
 * LinearProbModel.forward (simseg/models/pipelines/linear_prob.py:61-71, tasks/linear_prob/hooks/utils.py).  Per row i with label y, in fp32:
 *   m = max_j x_j,  lse = m + log(sum_j exp(x_j - m)),  loss_rows[i] = lse - x_y,
 *   ranks[i] = #{j : x_j > x_y} + #{j < y : x_j == x_y}      (equal logits rank by ascending class id, the order of simseg_topk_search),
 *   write_grad: dlogits[i, j] = (exp(x_j - lse) - [j == y]) * gscale   (fp32 [B, C]; gscale = 1 / B for the mean loss).
 * (lse is not rounded on its own: the loss is formed as log(sum) + (m - x_y) and the exponent as (x_j - m) - log(sum).)
 * A label outside [0, C) never indexes the row: loss_rows[i] = NaN, ranks[i] = INT32_MAX (a miss at every k), gradient row zero.
 * out3 = {mean of loss_rows, #{ranks < 1}, #{ranks < 5}} from a one-block second launch that adds the rows in index order in double
 * precision (bit-reproducible, no atomics).  C <= 1024: one wave per row, the row held in registers; larger: one block per row.
 * 1 <= C <= 65536, B >= 1; anything else is refused before a launch. */
int simseg_ce_rows(const void* logits, int dt, const int64_t* labels, float* loss_rows, int32_t* ranks, float* dlogits, float* out3,
                   int64_t B, int64_t C, float gscale, int write_grad, void* stream);
/* simseg_ce_rows against a two-label soft target (timm's mixup_target; with labels_a == labels_b the reference's
 * LabelSmoothingCrossEntropy, mml_loss.py:350-376), still one pass and no dense [B, C] target.  Per row i with a = labels_a[i],
 * b = labels_b[i], lam = lam[i] (fp32 on the device), eps = smoothing (0 <= eps < 1):
 *   t_c = lam * s_c(a) + (1 - lam) * s_c(b),   s_c(y) = (1 - eps) * [c == y] + eps / C,
 *   loss_rows[i] = -sum_c t_c log softmax(x)_c
 *                = log(sum_j exp(x_j - m)) + (1 - eps) * (lam * (m - x_a) + (1 - lam) * (m - x_b)) - eps * mean_c(x_c - m)
 *     (relative to the row maximum m, never through a rounded lse),
 *   ranks[i] as in simseg_ce_rows for the label a (training accuracy is reported against the sample's own label),
 *   write_grad: dlogits[i, c] = (softmax(x)_c - t_c) * gscale.
 * With lam = 1 and eps = 0 every output equals simseg_ce_rows' on (logits, labels_a) bit for bit (the same kernels, instantiated with
 * the soft terms).  A label outside [0, C) in EITHER vector: NaN loss row, rank INT32_MAX, zero gradient row.  out3, the limits on B and
 * C and the two regimes as in simseg_ce_rows. */
int simseg_soft_ce_rows(const void* logits, int dt, const int64_t* labels_a, const int64_t* labels_b, const float* lam, float smoothing,
                        float* loss_rows, int32_t* ranks, float* dlogits, float* out3, int64_t B, int64_t C, float gscale, int write_grad,
                        void* stream);
/* Mixup / CutMix of a batch with its flipped self, in place and in ONE launch (csrc/mixup.hip; DESIGN.md "Mixup / CutMix").  images
 * [B, C, H, W] contiguous (dt: 0 fp32, 1 the selected 16-bit type), B even; the partner of sample i is j = B - 1 - i.  table[i] = eight
 * int32 words {kind, yl, yh, xl, xh, lam, om, 0} with lam and om (= float32(1.0 - double(lam)), formed by the caller) as fp32 bits.  With
 * x the values before the call:
 *   kind 0: sample i keeps its bits and is not written;
 *   kind 1 (mixup): out_i = fl32(fl32(lam_i * x_i) + fl32(om_i * x_j)) - two rounded products and a rounded sum, no FMA: on fp32 storage
 *           the bits of torch's x * lam + x.flip(0) * (1 - lam); on 16-bit storage the same fp32 arithmetic on the widened values,
 *           rounded once (to nearest even) to the storage type;
 *   kind 2 (cutmix): out_i = x_j inside rows [yl, yh) x columns [xl, xh) of every channel, x_i elsewhere (lam_i is not read; an empty
 *           box is legal).
 * out_i is formed from the partner's ORIGINAL values although the partner is rewritten by the same launch (also when i is a mixup row and
 * j a cutmix row with another box): the unit of work is the pair.  Every element is read at most once and written at most once; a pair of
 * cutmix rows moves only its boxes.  table_host is a HOST copy of table: before anything is launched an odd B, a kind outside 0..2, a
 * box outside 0 <= yl <= yh <= H, 0 <= xl <= xh <= W, a lam or om that is not finite or outside [0, 1], and a null or misaligned pointer
 * are refused with a message naming the sample. */
int simseg_mix_batch(void* images, int dt, const int32_t* table, const int32_t* table_host, int64_t B, int64_t C, int64_t H, int64_t W,
                     void* stream);
/* LARS (simseg/core/optimizer/lars.py:86-127) as three launches over a tensor table, whatever the number of tensors.  table[t] = six
 * 8-byte words {p, g, buf, p16, (float lr, float weight_decay), flags}: fp32 master, fp32 gradient, fp32 momentum buffer (0 when momentum
 * is 0), the 16-bit compute copy to refresh (or 0), the tensor's learning rate and weight decay packed as two floats, flags bit 0 =
 * lars_exclude, bit 1 = the tensor's first step (no momentum buffer yet).  sizes[t] elements; chunk c covers [chunk_off[c],
 * chunk_off[c] + chunk) of tensor chunk_tid[c] (one block per chunk), a tensor's chunks are consecutive: [tensor_first[t],
 * tensor_first[t + 1]).  The *_host arguments are HOST copies of the device tables of the same name: sizes, tensor ids, offsets and
 * ranges are checked on them and an error returned before anything is launched; the caller guarantees that they hold what the device
 * tables hold.
 * norm_partials: partials[2c] = sum of p^2, partials[2c + 1] = sum of g^2 over chunk c (double; one plain store each; p, g read-only).
 * finish: one block per tensor adds its partials in chunk order in double precision; local_lr[t] = eta * wn / (gn + weight_decay * wn
 *   + eps) when wn != 0 and gn != 0, else 1; 1 for a lars_exclude tensor.  Nothing is read on the host.
 * multi_step, per element: d = (g + weight_decay * p) * (local_lr[t] * lr); momentum != 0: buf = d on the tensor's first step, else
 *   momentum * buf + (1 - dampening) * d, and d = nesterov ? d + momentum * buf : buf; p -= d; p16 = p rounded. */
int simseg_lars_norm_partials(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                              const int64_t* sizes_host, const int32_t* chunk_tid_host, const int64_t* chunk_off_host, int64_t n_tensors,
                              int64_t n_chunks, int chunk, double* partials, void* stream);
int simseg_lars_finish(const void* table, const int32_t* tensor_first, const int32_t* tensor_first_host, const double* partials,
                       int64_t n_tensors, int64_t n_chunks, float eta, float eps, float* local_lr, void* stream);
int simseg_lars_multi_step(const void* table, const int64_t* sizes, const int32_t* chunk_tid, const int64_t* chunk_off,
                           const int64_t* sizes_host, const int32_t* chunk_tid_host, const int64_t* chunk_off_host, int64_t n_tensors,
                           int64_t n_chunks, int chunk, const float* local_lr, float momentum, float dampening, int nesterov, void* stream);

int simseg_cast(const void* in, void* out, int64_t n, int to_bf16, void* stream);
int simseg_transpose_f32(const float* in, float* out, int64_t R, int64_t C, void* stream);
/* fp32 [rows, K] (row stride ld_in) -> bf16 [rows, 6 K]: the three round-to-nearest bf16 pieces hi / mid / lo of every element
 * (hi + mid + lo == x), laid out along K as [hi|hi|hi|mid|mid|lo] (b_pattern = 0, the A operand) or [hi|mid|lo|hi|mid|hi] (b_pattern = 1,
 * the B operand; b_pattern = 2: three planes bf16 [3][rows, K] instead, the operand form of simseg_attention_fwd_x3), so that ONE simseg_gemm call on the two bf16 images forms the six leading piece products of the fp32 product in its
 * fp32 accumulators - the exact-mode nn.Linear of the evaluation tools (torch fp32 matmul, vit_builder.py:18 / huggingface_builder.py:16-17
 * without autocast) at the bf16 MFMA rate; the three dropped products are <= 2^-24 |a||b|, the size of an fp32 FMA's own rounding. */
int simseg_split_bf16x3(const float* in, void* out, int64_t rows, int64_t K, int64_t ld_in, int b_pattern, void* stream);
/* Exact-mode attention forward (timm Attention.forward in fp32, vit_builder.py:18, as the evaluation tools run it) on the bf16 matrix pipe:
 * qkv3 = the three bf16 pieces of the fp32 packed projection as planes (simseg_split_bf16x3 with b_pattern = 2: bf16 [3][B, T, 3, H, 64],
 * piece p at qkv3 + p * plane_elems); scores and outputs accumulate the six leading piece products in fp32 (fp32-grade accuracy, like
 * the split GEMM).  out fp32 [B, T, H*64].  No mask / dropout / log-sum-exp: evaluation only. */
int simseg_attention_fwd_x3(const void* qkv3, int64_t plane_elems, float* out, int64_t B, int64_t T, int64_t H, float scale, void* stream);
/* dst[i,:] = src[idx[i],:] (idx[i] < 0: a zero row); rows of row_bytes (a multiple of 16) bytes, any dtype.  Drops / restores the padded
 * token rows of ragged caption batches around the text tower's GEMMs (HF BertModel computes them: huggingface_builder.py:16-17). */
int simseg_gather_rows(const void* src, const int32_t* idx, void* dst, int64_t n, int64_t row_bytes, void* stream);
/* Row maps of a ragged caption batch from its 0/1 attention mask [B, L] (int64, as the reference's tokenizer delivers it:
 * simseg/datasets/clip/clip_dataset.py:127-133), in one launch and without a host read: idx int32 [cap] = flat positions b*L+l of the real
 * tokens in raster order, then -1 up to the next multiple of `multiple` (or cap); inv int32 [B*L] = packed row of every position (-1 at
 * padded positions); row_start int32 [B+1]; info int32 [4] = {real tokens, 1 if a sequence has a real token behind a padded one,
 * 1 if they did not fit cap rows or differ from `expect` (>= 0: the count the caller sized its buffers for, e.g. from the loader's
 * caption lengths; -1: unknown), rows of idx written}.  What the text tower needs to skip the padded token rows HF's BertModel computes
 * (huggingface_builder.py:16-17) - replaces ~15 torch index kernels and two host reads per step.  B <= 8192. */
int simseg_ragged_maps(const int64_t* mask, int64_t B, int64_t L, int64_t multiple, int64_t cap, int64_t expect, int32_t* idx, int32_t* inv,
                       int32_t* row_start, int32_t* info, void* stream);
/* g[i] = keep(seed, i) ? g[i] / (1-p) : 0 -- regenerates the forward dropout mask of simseg_gemm for the backward. */
int simseg_dropout_apply(void* g, int dtype, int64_t n, uint64_t seed, float p, void* stream);

/* ---- zero-shot segmentation post-processing (tools/seg_evaluation.py:112-170) ---------------------------------
 * scores [B,C] = pooled . text^T.  Top `top_cls_num` classes (:121), threshold = mean + unbiased std of those (:122-123); the
 * first `ncand` (reference: 5, :128-130) become candidates.  cand_idx[b,i] = class index, or -1 where the reference skips the
 * slot (class 0 / 255 :132-133, or score < threshold :145-146); cand_score[b,i] = its score; threshold[b] optional. */
int simseg_seg_select(const float* scores, int* cand_idx, float* cand_score, float* threshold, int64_t B, int64_t C,
                      int64_t top_cls_num, int64_t ncand, void* stream);
/* sim [B, n*n, C] fp32 (simseg_patch_text_sim).  Per valid candidate: its column, min-max normalised (:148-149) -> prob
 * [B,ncand,n*n] (optional, the DenseCRF unary input) and the binary map prob > 0.5 scaled to 255 (what dense_crf :30-54 returns
 * with its pairwise terms off), nearest-upsampled x16 (:137) -> mask [B,ncand,16n,16n] bytes.  Invalid slots are not written. */
int simseg_seg_masks(const float* sim, const int* cand_idx, float* prob, void* mask, int64_t B, int64_t n, int64_t C, int64_t ncand,
                     void* stream);
/* The same on a rectangular patch grid: sim [B, nh*nw, C] (row-major patch rows), mask [B,ncand,16nh,16nw] - the stitched map of a
 * sliding-window evaluation (BASELINE configs[3]); simseg_seg_masks is the nh = nw case. */
int simseg_seg_masks_rect(const float* sim, const int* cand_idx, float* prob, void* mask, int64_t B, int64_t nh, int64_t nw, int64_t C,
                          int64_t ncand, void* stream);
/* Sliding-window stitch (BASELINE configs[3] / SURVEY.md 8d cfg 4: 512x512 windows at stride 256 over a larger image, "overlap-average
 * sim maps"; the reference tool itself resizes to one window, tools/seg_evaluation.py:84-85,109).  win [B, wy, wx, n*n, C] fp32 = the
 * per-window similarity maps (simseg_patch_text_sim), window (i, j) at patch offset (i*step, j*step); out [B, nh*nw, C] with
 * nh = n + (wy-1)*step, nw = n + (wx-1)*step: per cell the mean over the covering windows, summed in (i, j) order.  step = 0: the plain
 * mean over all windows (with n = 1: image-level class scores from per-window scores). */
int simseg_stitch_windows(const float* win, float* out, int64_t B, int64_t wy, int64_t wx, int64_t n, int64_t step, int64_t C, void* stream);
/* Sliding windows over B images of ANY sizes (segpost.slide_windows, DESIGN.md "Sliding windows on any image size").  Tables (device,
 * built by simseg_amd.ops.slide_plan): img_tab int64 [B, 8] = (src_off, H, W, out_off, wstart, ny, nx, 0) per image - element offset of
 * its [3, H, W] pixels in `images`, its extent, element offset (a multiple of 16) of its [ncand, H, W] planes in prob / mask, its first
 * window and its window grid; win_tab int64 [Nw, 3] = (image, y0, x0) per window, an image's windows consecutive and row-major.
 * extract: out [Nw, 3, win, win] fp32 = the windows of win_tab, zero where a window runs past the image. */
int simseg_slide_extract(const float* images, const int64_t* img_tab, const int64_t* win_tab, float* out, int64_t Nw, int64_t win, void* stream);
/* out [B, C] = per image, the fp32 sum of its windows' rows of win_scores [Nw, C] in window order, divided once by their count. */
int simseg_slide_scores(const float* win_scores, const int64_t* img_tab, float* out, int64_t B, int64_t C, void* stream);
/* For every visited slot (cand_idx [B, ncand] >= 0) of every image: the pixel-resolution stitch of sim_w [Nw, n*n, C] fp32 (pixel (y, x)
 * = the mean over its covering windows, summed in window order, of their cell ((y - y0) / 16, (x - x0) / 16)), min-max normalised over the
 * image -> prob (fp32) and mask (uint8 0 / 255, prob > 0.5) at out_off + k*H*W; minmax [B, ncand, 2] = the stitched map's min and max.
 * Unvisited slots are not written.  max_h / max_w / max_hw: the largest H, W and H*W over the images; workspace: fp32, of
 * simseg_slide_stitch_workspace_bytes(B, ncand, max_h, max_w) bytes.  No limit on the number of patches of an image. */
int64_t simseg_slide_stitch_workspace_bytes(int64_t B, int64_t ncand, int64_t max_h, int64_t max_w);
int simseg_slide_stitch(const float* sim_w, const int64_t* img_tab, const int64_t* win_tab, const int* cand_idx, float* prob, void* mask,
                        float* minmax, float* workspace, int64_t B, int64_t ncand, int64_t n, int64_t C, int64_t win, int64_t max_h,
                        int64_t max_w, int64_t max_hw, void* stream);
/* Multi-scale and flip test-time augmentation over sliding windows (DESIGN.md "Multi-scale and flip test-time augmentation").
 * extract_flip: simseg_slide_extract with a per-call flag; flip != 0 cuts the windows of win_tab from the left-to-right MIRRORED images:
 * window (image, y0, x0), row i, column j reads source row y0 + i, column W - 1 - (x0 + j), zero where x0 + j >= W or y0 + i >= H. */
int simseg_slide_extract_flip(const float* images, const int64_t* img_tab, const int64_t* win_tab, float* out, int64_t Nw, int64_t win, int flip,
                              void* stream);
/* stitch_multi: the fused map of P passes over the same B images, written in the layout of simseg_slide_stitch for the BASE image table
 * img_tab (sizes H x W).  pass_tab (device, built on the host) int64 [P, 4] = (sim_w pointer, img_tab pointer, win_tab pointer, flip)
 * per pass: the pass's per-window maps [Nw_p, n*n, C] fp32 and its own simseg_slide_* tables over its B images of sizes H_p x W_p, all with
 * the same win.  S_p = the pass's pixel-resolution stitched map as simseg_slide_stitch defines it before its min-max step, un-mirrored
 * (S_p(y', W_p - 1 - x')) when flip != 0.  Fused map at base pixel (y, x): nearest sampling with pixel centres in integers,
 * y_p = min(((2y + 1) H_p) / (2H), H_p - 1), x_p likewise with W; F(y, x) = (sum over p in pass order, fp32, of S_p(y_p, x_p)) / P,
 * divided once.  prob = F min-max normalised over the image, mask = prob > 0.5 ? 255 : 0, minmax [B, ncand, 2] = min and max of F, for
 * visited slots (cand_idx [B, ncand] >= 0) at out_off + k*H*W; unvisited slots are not written.  With P = 1, H_p = H, W_p = W, flip = 0 the
 * three outputs are simseg_slide_stitch's bit for bit.  At most 16 passes (1 <= P <= 16; a larger P is refused with an error before any launch);
 * no limit on image sizes, scales or window counts; no host read.  max_h / max_w / max_hw: of the base images; workspace: fp32, of
 * simseg_slide_stitch_multi_workspace_bytes(B, ncand, max_h, max_w) bytes. */
int64_t simseg_slide_stitch_multi_workspace_bytes(int64_t B, int64_t ncand, int64_t max_h, int64_t max_w);
int simseg_slide_stitch_multi(const int64_t* pass_tab, int64_t P, const int64_t* img_tab, const int* cand_idx, float* prob, void* mask,
                              float* minmax, float* workspace, int64_t B, int64_t ncand, int64_t n, int64_t C, int64_t win, int64_t max_h,
                              int64_t max_w, int64_t max_hw, void* stream);
/* Image preprocessing (simseg_amd/preproc.py, DESIGN.md "Device-side image preprocessing"): B decoded uint8 [H, W, 3] images packed in
 * `src` -> Pillow's uint8 resize (its integer arithmetic, bit for bit) restricted to an output rectangle -> out fp32 [3, OH, OW] planes
 * = lut [3, 256] at the resized byte; optionally (out_u8 != NULL) also the resized bytes as [OH, OW, 3].  ONE launch for the batch.
 * img_tab int64 [B, 16] = (src byte offset, H, W, out element offset, OH, OW, crop top, crop left, offset and ksize of the horizontal
 * axis table, offset and ksize of the vertical one, resized RH, RW, out_u8 byte offset, first tile = the sum over the earlier images of
 * ceil(OW / 64) * ceil(OH / 32)); an axis table at int32 offset `off` of `tab` = bounds [out, 2] (xmin, n) then coefficients
 * [out, ksize] (22 fractional bits), out = RW / RH.  img_tab_host and tab_host are HOST copies of the two device tables: every offset,
 * extent and bound is checked on them (offsets in range, OH, OW > 0, 1 <= n <= ksize, xmin + n <= in, monotone bounds, no int32
 * overflow) and an error returned before anything is launched.  The kernel reads the DEVICE tables and nothing compares the two: the
 * CALLER GUARANTEES that each host copy holds exactly what its device table holds (or will hold once the copies queued before this call
 * on `stream`, or made visible to it, have run) - simseg_amd.preproc.plan builds both from one array. */
int simseg_image_preprocess(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                            const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, float* out,
                            int64_t out_numel, void* out_u8, int64_t u8_bytes, void* stream);
/* Training augmentation (simseg_amd/augment.py, DESIGN.md "Device-side training augmentation"): B decoded uint8 [H, W, 3] images packed
 * in `src` -> crop box -> Pillow's bilinear uint8 resize to S x S -> op1, op2 of the AutoAugment set (Pillow's arithmetic, bit for bit)
 * -> out fp32 [B, 3, S, S] = lut [3, 256] at the final byte; optionally (out_u8 != NULL) also the final bytes as [B, S, S, 3].  TWO
 * launches for the batch, 32 <= S <= 384.  img_tab int64 [B, 30] = (src byte offset, H, W, crop top, crop left, crop h, crop w, offset
 * and ksize of the horizontal axis table (crop w -> S), offset and ksize of the vertical one (crop h -> S), 0, op1 code, op2 code,
 * 8 parameter slots of op1, 8 of op2); op codes 0 none, 1 posterize (mask), 2 solarize (bytes below the threshold kept), 3 invert,
 * 4 autocontrast, 5 equalize, 6 color, 7 contrast, 8 sharpness (float bits of the blend factor), 9 rotate (16.16 fixed-point a0, a1,
 * a3, a4, x start, y start), 10 shearX (double bits of the affine a0..a5); the axis tables are preproc's (simseg_image_preprocess).
 * scratch: at least simseg_train_augment_scratch_bytes(B, S) device bytes.  Every offset, extent, table and parameter is checked on
 * the HOST copies before anything is launched; the caller guarantees that they hold what the device tables hold. */
int64_t simseg_train_augment_scratch_bytes(int64_t B, int64_t S);
int simseg_train_augment(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                         const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, int64_t S, void* scratch,
                         int64_t scratch_bytes, float* out, int64_t out_numel, void* out_u8, int64_t u8_bytes, void* stream);
/* Training transforms (simseg_amd/pipeline.py, DESIGN.md "Device-side training transforms"): the general chain behind
 * simseg_train_augment's special case, on the same packed source, axis tables, look-up table and scratch rule, in TWO launches.  Per
 * image: integer source box -> Pillow's uint8 resize of the box to RH x RW (either filter; RH = box h and RW = box w copy the box) ->
 * the S x S output window of the resized image at (window top, window left), its columns mirrored when flip != 0 -> a chain of up to 5
 * ops in order (the codes of simseg_train_augment plus 11 brightness: float bits of the blend factor with black) -> out fp32
 * [B, 3, S, S] = lut at the final byte, EXCEPT inside the image's erase boxes (later boxes win), where the value is the fill of the
 * mode: 0 const 0.0, 1 rand one normal per (image, box, channel), 2 pixel one normal per (image, box, channel, y, x).  A normal is
 * sqrt(-2 ln u1) cos(2 pi u2), u1 = ((h1 >> 8) + 1) 2^-24, u2 = (h2 >> 8) 2^-24, h1 = hash_u32(seed, 2 i), h2 = hash_u32(seed, 2 i + 1),
 * i = ((b * 4 + box) * 3 + channel) * 2^18 + y * 512 + x (y = x = 0 in mode 1; b = the image's row in the table).  out_u8 (optional)
 * receives the bytes after the chain, before the look-up and the erasing.
 * img_tab int64 [B, 81] = (0 src byte offset, 1 H, 2 W, 3..6 box top, left, h, w, 7..10 offset and ksize of the horizontal axis table
 * (box w -> RW) and of the vertical one (box h -> RH), 11 RH, 12 RW, 13 window top, 14 window left, 15 flip, 16 number of ops,
 * 17 number of erase boxes (0..4), 18 erase mode, 19 noise seed, 20..35 four erase boxes (top, left, h, w) in output coordinates,
 * 36..40 op codes, 41..80 eight parameter slots per op).  Every field is checked on the HOST copies before anything is launched; the
 * caller guarantees that they hold what the device tables hold. */
int64_t simseg_train_transforms_scratch_bytes(int64_t B, int64_t S);
int simseg_train_transforms(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                            const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, int64_t S, void* scratch,
                            int64_t scratch_bytes, float* out, int64_t out_numel, void* out_u8, int64_t u8_bytes, void* stream);
/* Training chain (simseg_amd/pipeline.py parse_chain(full = True), DESIGN.md "SimCLR colour distortion and Gaussian blur"):
 * simseg_train_transforms with room for the whole transform registry, on the same two kernels, arguments, scratch rule and erase noise.
 * A chain of up to 12 ops; the codes of simseg_train_transforms plus 12 grayscale (Pillow's convert("L") in all three channels), 13 hue
 * (slot 0 = the byte 0..255 added to H modulo 256 between Pillow's convert("HSV") and convert("RGB"); 0 still makes the round trip),
 * 14 Gaussian blur (slots R, ww, fw of ImageFilter.GaussianBlur's box passes: three along the rows, then three along the columns, each
 * out[x] = (ww * sum_{|d| <= R} in[x + d] + fw * (in[x - R - 1] + in[x + R + 1]) + 2^23) >> 24 with indices clamped to the line).
 * img_tab int64 [B, 144] = columns 0..35 as simseg_train_transforms', 36..47 op codes, 48..143 eight parameter slots per op.  Checked
 * on the HOST copy before anything is launched, besides what simseg_train_transforms checks: at most 12 ops, codes 0..14, the hue byte,
 * 0 <= R <= 7, ww > 0, fw >= 0 and (2R + 1) ww + 2 fw = 2^24 or 2^24 - 1 (fw is the floor of a half). */
int64_t simseg_train_chain_scratch_bytes(int64_t B, int64_t S);
int simseg_train_chain(const void* src, int64_t src_bytes, const int64_t* img_tab, const int64_t* img_tab_host, int64_t B,
                       const int32_t* tab, const int32_t* tab_host, int64_t tab_numel, const float* lut, int64_t S, void* scratch,
                       int64_t scratch_bytes, float* out, int64_t out_numel, void* out_u8, int64_t u8_bytes, void* stream);
/* cv2.dilate / cv2.erode with a 7x7 ones kernel, ONE iteration (the third positional argument in :156-157 is `dst`, not
 * `iterations`), default border (never wins) on byte images [M,H,W]; erode = 0 dilate, 1 erode.  out must not alias in. */
int simseg_morph7(const void* in, void* out, int64_t M, int64_t H, int64_t W, int erode, void* stream);
/* cv2.dilate followed by cv2.erode (:156-157) in one pass over byte images [M,H,W] (the dilated image never leaves LDS); same
 * border rules as simseg_morph7 applied twice.  valid (optional, [M] ints): images with valid[m] < 0 are skipped and their
 * output left untouched (candidate slots the reference never visits). */
int simseg_close7(const void* in, void* out, const int* valid, int64_t M, int64_t H, int64_t W, void* stream);
/* masks [B,ncand,Hm,Wm] bytes -> nearest resize to (H,W) (cv2.INTER_NEAREST :159) -> temp_pred[class] = mask * score (:160) ->
 * argmax over classes (:163; first maximum, class 0 when nothing is positive) -> pred [B,H,W] int32 (optional) and
 * hist [3,C] uint64 += {intersect, pred area, label area} over pixels whose label != ignore_index (utils/metrics.py:60-74).
 * labels [B,H,W] bytes. */
int simseg_seg_predict(const void* masks, const int* cand_idx, const float* cand_score, const void* labels, int* pred, void* hist,
                       int64_t B, int64_t ncand, int64_t Hm, int64_t Wm, int64_t H, int64_t W, int64_t C, int64_t ignore_index,
                       void* stream);

/* The fully connected CRF the reference applies to every visited candidate map (tools/seg_evaluation.py:31-54, called at :153:
 * pydensecrf DenseCRF2D with 2 labels, U = -log([1-p, p] + 1e-8), addPairwiseGaussian(sxy=3, compat=3), addPairwiseBilateral(sxy=40,
 * srgb=13, rgbim, compat=10), inference(3), argmax), as mean-field inference on two permutohedral lattices built on the device.
 * rgb [B,H,W,3] bytes (the de-normalised network inputs, RGB order), prob [B,C,H,W] fp32 in [0,1] (C <= 8 candidate maps per image:
 * an image's maps share its lattices; the images of a batch are independent problems solved side by side in the same launches) ->
 * mask [B,C,H,W] bytes (255 where the pixel is labelled as the class); q_out (optional) [B,C,H,W] fp32 = Q(label 1) after the last
 * iteration.  workspace: caller-allocated, 256-byte aligned, simseg_dense_crf_workspace_bytes(B, H, W, C).  reuse_spatial != 0: the caller
 * vouches that the previous call on this workspace had the same H, W and sxy_g and that the workspace is untouched since - the spatial
 * (Gaussian) lattice, which depends on nothing else, is then not rebuilt. */
int64_t simseg_dense_crf_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C);
int simseg_dense_crf(const uint8_t* rgb, const float* prob, uint8_t* mask, float* q_out, int64_t B, int64_t C, int64_t H, int64_t W, float sxy_g,
                     float compat_g, float sxy_b, float srgb, float compat_b, int iters, void* workspace, int64_t workspace_bytes,
                     int reuse_spatial, void* stream);

/* PAMR, pixel-adaptive mask refinement (Araslanov & Roth, CVPR 2020) - the device alternative to the DenseCRF above; the reference has
 * none.  rgb [B,H,W,3] bytes, prob [B,K,H/scale,W/scale] fp32 in [0,1] (scale > 1: the first iteration reads it through (y / scale,
 * x / scale) - the tool's nearest upsampling, never materialised; H and W are then multiples of scale), cand_idx (optional) [B,K] ints:
 * slots with a negative entry are not computed and come back zero; NULL = every slot is visited.  dilations: n_dil (1..8) HOST ints in
 * 1..64; taps = (dilation, offset) dilation-major over the offsets (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1), neighbours
 * with replicate padding.  Per pixel and channel sigma = the unbiased standard deviation over the 9 n_dil samples of the dilated 3x3
 * neighbourhoods (integer sums), logit_t = -(1/3) sum_c |rgb_c(p) - rgb_c(q_t)| / (1e-8 + 0.1 sigma_c(p)), w = softmax over the taps;
 * m <- sum_t w_t m(q_t), iters (0..64) times in fp32 with a fixed tap order (a result does not depend on the batch position) ->
 * mask [B,K,H,W] bytes (255 where m > 0.5) and, optionally, m_out [B,K,H,W] fp32.  iters = 0: the unary decision prob > 0.5.
 * ws: caller-allocated, 16-byte aligned, simseg_pamr_workspace_bytes(...) = the weights [B][8 n_dil][H][W] fp32 plus two map buffers
 * (-1 for arguments out of range).  A refused call launches nothing and leaves the outputs untouched.  No atomics, no host read and
 * no inter-block dependence: the call may be captured in a graph. */
int64_t simseg_pamr_workspace_bytes(int64_t B, int64_t K, int64_t H, int64_t W, int n_dil);
int simseg_pamr(const uint8_t* rgb, const float* prob, const int* cand_idx, uint8_t* mask, float* m_out, int64_t B, int64_t K, int64_t H,
                int64_t W, const int* dilations, int n_dil, int iters, int64_t scale, void* ws, int64_t ws_bytes, void* stream);

/* debug: bf16 attention forward that also writes a 5-entry cycle-counter timeline of block (0,0) to dbg (tools/dbg_attn_timeline.py). */
int simseg_debug_attention_timeline(const void* qkv, void* out, float* lse, void* dbg, int64_t B, int64_t T, int64_t H, void* stream);

/* hardware probe used by tests: lane/element map of ds_read_b64_tr_b16. */
int simseg_debug_tr16_probe(int* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
