/* titok_hip.h - C-ABI of libtitok_hip.so: the MI355X (gfx950) compute path of the TiTok-Video tokenizer.
 *
 * The reference (NilanEkanayake/TiTok-Video) exposes this path as a Python nn.Module API, not an FFI
 * (SURVEY.md section 8b).  The Python mirror in titok_video_amd/model/ keeps that API and binds these
 * entry points with ctypes; every entry point below names the reference code it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, ints, floats, an opaque hipStream_t passed as void*.  No torch types.
 *   - every call only ENQUEUES work on `stream` and never synchronises; no hidden global state, no allocation:
 *     the caller owns all buffers including the workspace (size from ttv_tower_workspace_bytes).
 *   - return value: 0 = TTV_OK, otherwise a TTV_ERR_* code; ttv_error_string() explains the last error of
 *     the calling thread.  The Python shim raises RuntimeError on any non-zero code.
 *   - activations/weights of linear layers are in the compute dtype (TTV_BF16 or TTV_F32); RMSNorm gains,
 *     mask_token, rope tables and all statistics are fp32; matrix products accumulate in fp32.
 *   - rows of a packed batch: for clip b, rows [cu[b], cu[b]+K_b) are its latent tokens, rows
 *     [cu[b]+K_b, cu[b+1]) its patch tokens in (t,h,w) raster order (model/base/blocks.py:85-86).
 */
#ifndef TITOK_HIP_H
#define TITOK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTV_OK 0
#define TTV_ERR_INVALID 1      /* bad argument / unsupported shape */
#define TTV_ERR_LAUNCH 2       /* hip launch error */
#define TTV_ERR_UNSUPPORTED 3

#define TTV_BF16 0
#define TTV_F32 1

#define TTV_ENCODER 0
#define TTV_DECODER 1

#define TTV_MAX_FSQ 8
#define TTV_MAX_TOKEN 64       /* widest latent token (encoder proj_out rows / decoder proj_in columns): FSQ needs <= TTV_MAX_FSQ, the
                                  nearest-codebook-entry quantiser of BASELINE configs #4 / #5 uses 32 / 64 */
#define TTV_MAX_CLIPS_PER_LAUNCH 64

const char* ttv_error_string(void);
int ttv_version(void);

/* ---- deterministic mode: fixed-order sums in place of every float atomic onto a shared address ----------------------------------------
 * Process-wide, off by default; ttv_set_deterministic returns the previous value.  Launchers read it when they launch, so under a
 * graph capture it is the value at capture.  Off: nothing changes - the same kernels, launch geometry and workspace sizes.  On: two
 * runs of a training step on the same inputs give the same bits (the order of a cross-rank all-reduce is outside this mode).
 *   Row reductions into a vector or scalar (RMSNorm gain gradients, bias / column sums, the mask-token sum, the d <-> token_size
 *   projection gradients, ttv_l1_loss, ttv_sq_err_accumulate): every block writes its partial to scratch as [block][element] with
 *   plain stores; a second kernel, one thread per element, adds the partials of an element in ascending block index starting from
 *   block 0's (fp32; double for the squared-error sums) and adds that total onto the destination with a plain load / add / store.
 *   The block's own arithmetic is what it is with the mode off.
 *   Weight gradients (ttv_linear_wgrad and the towers): the split partial tiles with their fixed-order sum where the workspace has
 *   room; otherwise (no or too little workspace, an operand off 16 bytes, TTV_WGRAD_TILE64, fp32) one token range per output tile:
 *   a single writer per address.
 *   fp32 attention backward: dK / dV by an owner per (key row, kv-head) that adds over the sequence's query rows, and for each over
 *   the q-heads of its group, in ascending order.  Codebook gradient: an owner per codebook entry adds its token rows in ascending order.
 * Scratch: the tower backward entry points take the partials from their workspace - ttv_tower_bwd_workspace_bytes[_ex] returns the
 * larger size while the mode is on.  The four ops without a workspace argument have a sibling *_det that takes (scratch,
 * scratch_bytes) - device memory, 16-byte aligned, at least the size function beside it - and with the mode on the plain entry point
 * returns TTV_ERR_INVALID before any launch, naming the sibling.  A sibling called with the mode off runs the plain path and
 * ignores its scratch.  Size functions return -1 (message set) on refused input. */
int ttv_set_deterministic(int on);
int ttv_get_deterministic(void);

/* ---- FSQ (model/quantizer/fsq.py) -------------------------------------------------------------------- */
typedef struct ttv_fsq_params {
  int32_t n;                        /* codebook_dim = len(levels)                         fsq.py:69 */
  int32_t levels[TTV_MAX_FSQ];      /* _levels                                            fsq.py:63 */
  int32_t basis[TTV_MAX_FSQ];       /* _basis = cumprod([1]+levels[:-1])                  fsq.py:66 */
  float half_l[TTV_MAX_FSQ];        /* (levels-1)*(1+eps)/2, fp32, computed by the host   fsq.py:80 */
  float offset[TTV_MAX_FSQ];        /* 0.5 for even levels                                fsq.py:81 */
  float shift[TTV_MAX_FSQ];         /* atanh(offset/half_l)                               fsq.py:82 */
  float half_width[TTV_MAX_FSQ];    /* levels // 2                                        fsq.py:89 */
} ttv_fsq_params;

/* FSQ.forward (fsq.py:123-135): z [rows,n] (dtype) -> codes [rows,n] (dtype), indices int32 [rows];
 * bounded (fp32 [rows,n], value before rounding) is optional (NULL to skip). */
int ttv_fsq_forward(const ttv_fsq_params* p, const void* z, int z_dtype, int rows, void* codes, int codes_dtype,
                    int32_t* indices, float* bounded, void* stream);
/* FSQ.indices_to_codes (fsq.py:100-121): int32 [rows] -> codes [rows,n] (dtype). */
int ttv_fsq_indices_to_codes(const ttv_fsq_params* p, const int32_t* indices, int rows, void* codes, int codes_dtype,
                             void* stream);

/* ---- nearest-codebook-entry (L2) quantiser ---------------------------------------------------------------
 * Not a reference component (the reference quantises with FSQ only); BASELINE.json's north_star / configs #4, #5 ask for it.  On
 * the FSQ lattice implicit_codebook * (levels // 2) (fsq.py:73-76) applied to FSQ.bound(z) (fsq.py:78-83) it returns FSQ's indices
 * (fsq.py:105-109) away from rounding ties; for learned / synthetic codebooks it is argmin_n ||z - c_n||^2 with the LOWEST index on
 * exact ties (torch.argmin's rule).  z [rows, C], codebook [N, C] in `dtype` (fp32: exact-fp32 MFMA; bf16: bf16 MFMA, fp32 sums),
 * C <= 64.  cnorm: fp32 [N] = ||c_n||^2 from ttv_vq_codebook_norms (once per codebook).  best_dist (optional) fp32 [rows]. */
int ttv_vq_codebook_norms(const void* codebook, int dtype, int ld, int N, int C, float* cnorm, void* stream);
/* workspace: ttv_vq_workspace_bytes(rows) bytes, 8-byte aligned (per-row merge keys of the codebook splits; cleared by the call). */
int64_t ttv_vq_workspace_bytes(int rows);
int ttv_vq_l2_argmin(const void* z, int dtype, int ldz, const void* codebook, int ldc, const float* cnorm, int rows, int N, int C,
                     int32_t* indices, float* best_dist, void* workspace, int64_t workspace_bytes, void* stream);
/* straight-through lookup: codes[r] = codebook[indices[r]] (the value the decoder sees; gradients pass to z unchanged). */
int ttv_vq_lookup(const void* codebook, int dtype, int ldc, const int32_t* indices, int rows, int C, void* codes, int ldo, void* stream);
/* Backward of the lookup with respect to the codebook: dcodebook[indices[r], :] += dcodes[r, :] (fp32 accumulation, float atomics; the
 * caller zeroes dcodebook [N, C], ldc).  With codes = codebook[idx] + (z - stopgrad(z)) this is the codebook's gradient of the
 * straight-through quantiser named by BASELINE.json's north_star; the encoder's is the identity (FSQ's round_ste, fsq.py:48-51, is the
 * reference's instance of the same estimator). */
int ttv_vq_lookup_backward(const void* dcodes, int dtype, int ld, const int32_t* indices, int rows, int C, float* dcodebook, int ldc, void* stream);
/* Deterministic sibling (see ttv_set_deterministic): N = codebook entries; an owner per entry walks the token rows in ascending order
 * and adds the rows that chose it one after the other in fp32, then adds that sum onto dcodebook[entry] (an entry no row chose is not
 * written; an index outside [0, N) contributes nothing).  No partials: the size function returns 0 and scratch may be NULL. */
int64_t ttv_vq_lookup_backward_det_scratch_bytes(int rows, int N, int C);
int ttv_vq_lookup_backward_det(const void* dcodes, int dtype, int ld, const int32_t* indices, int rows, int N, int C, float* dcodebook, int ldc,
                               void* scratch, int64_t scratch_bytes, void* stream);

/* ---- training the L2 quantiser: commitment term, EMA codebook, restart of dead entries (ttv_vq_train.hip) ----------------------------
 * Not reference components (the reference trains FSQ, which has no codebook).  Every sum below has a fixed order and no float atomic:
 * two calls on the same inputs give the same bits, whatever the grid.  z [rows, C] in `dtype` (TTV_BF16 or TTV_F32), 1 <= rows < 2^24,
 * C <= 64; z, codebook and workspace 16-byte aligned (rows need no alignment of their own).  All work is enqueued on `stream`.
 * workspace: ttv_vq_train_workspace_bytes(rows, N) bytes, shared by the four calls of one step. */
int64_t ttv_vq_train_workspace_bytes(int rows, int N);
/* loss[0] = mean over rows and C of (z - e)^2 in fp32, e = codebook[indices[r]] read from the compute-dtype codebook the argmin read.
 * Order: a block of 256 threads owns 64 consecutive rows; thread t folds elements t, t + 256, .. of that stretch (row-major) with
 * acc = fmaf(d, d, acc); the 256 values meet by halves (t += t + 128, then 64, .., 1).  One block then folds the per-block sums the same
 * way (thread t takes partials t, t + 256, ..) and multiplies by (float)(1 / (rows C)). */
int ttv_vq_commit_forward(const void* z, int dtype, int ldz, const void* codebook, int ldc, const int32_t* indices, int rows, int N, int C,
                          float* loss, void* workspace, int64_t workspace_bytes, void* stream);
/* dz = grad + scale (z - e) per element, all four [rows, C] in `dtype`; e = the rows the lookup returned.  Formed in fp64 and rounded
 * once to fp32 (bf16: once more, to bf16).  scale = commitment_weight 2 / (rows C) for the mean above. */
int ttv_vq_commit_backward(const void* grad, int ldg, const void* z, int ldz, const void* e, int lde, int dtype, int rows, int C, double scale,
                           void* dz, int ldd, void* stream);
/* stats: fp32 [N (2 C + 1)] = count [N] | sum [N, C] | cand [N, C], every element written.  count[n] = rows with indices[r] == n (an
 * index outside [0, N) is counted nowhere); sum[n, :] = those rows of z as fp32, added one after the other in ascending row order
 * starting from 0 (float32 np.add.at).  cand is zero unless cluster_size is given and cluster_size[n] < dead_threshold: then Philox4x32-10
 * (the generator of ttv_gp_noise_add) of counter (n, 0, step low, step high), step = ema_step[0] read on the device, under key (seed low,
 * seed high) gives words w; if w[0] % world_size == rank, cand[n, :] = z[w[1] % rows, :] as fp32. */
int ttv_vq_ema_stats(const void* z, int dtype, int ldz, const int32_t* indices, int rows, int N, int C, const float* cluster_size,
                     float dead_threshold, uint64_t seed, const int64_t* ema_step, int rank, int world_size, float* stats, void* workspace,
                     int64_t workspace_bytes, void* stream);
/* The update, in place, from `stats` (summed over ranks by the caller).  With d = decay, m = one_minus_decay (1 - d formed by the caller
 * in double), t = dead_threshold and dead[n] = cluster_size[n] < t before the call, in fp32:
 *   cluster_size[n] = dead ? t : fmaf(d, cluster_size[n], m count[n]);   total = their sum (thread u of 1024 folds n = u, u + 1024, ..,
 *   then by halves 512, 256, .., 1);   live: embed_avg = fmaf(d, embed_avg, m sum), smoothed = (cluster_size + eps) / fmaf(N, eps, total) total,
 *   codebook = embed_avg / smoothed (IEEE divisions);   dead: embed_avg = t cand, codebook = cand;   ema_step[0] += 1.
 * codebook is the fp32 master [N, C]; codebook_copy the compute-dtype copy the next argmin reads (TTV_BF16: written too, rounded once;
 * TTV_F32: must be `codebook` itself); cnorm [N] = ||copy_n||^2 with the fmaf chain of ttv_vq_codebook_norms - the same bits.
 * eps > 0 (with eps = 0 an entry whose cluster size is 0 would divide by smoothed = 0).
 * workspace: (N + 1) floats at least; ttv_vq_train_workspace_bytes covers it. */
int ttv_vq_ema_update(const float* stats, float* cluster_size, float* embed_avg, float* codebook, void* codebook_copy, int copy_dtype,
                      float* cnorm, int64_t* ema_step, int N, int C, float decay, float one_minus_decay, float eps, float dead_threshold,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- mixed bf16 / fp8 linears (BASELINE config #5; not a reference feature: the reference runs bf16 autocast) -------------
 * Row-wise OCP e4m3 quantisation: y = gain ? RMSNorm(x) * gain (eps) : x;  scales[r] = max|y_r| / 448;  out[r] = e4m3(y_r / scales[r]).
 * in [rows, width] (dtype, leading dim ld_in), out uint8 [rows, ld_out], width % 4 == 0, width <= 1024. */
int ttv_quant_rows_fp8(const void* in, int dtype, int ld_in, const float* gain, float eps, void* out, int ld_out, float* scales, int rows,
                       int width, void* stream);
/* y[M,N] (bf16) = (xq * x_scale[:,None]) @ (wq * w_scale[:,None])^T on v_mfma_scale_f32_16x16x128_f8f6f4 (fp32 accumulation), K % 128 == 0.
 * epilogue: 0 plain store; 1 to_qkv + rotary (rope_cs, d_model, gqa_dim as ttv_linear_qkv_rope; N = 2 d_model + 2 gqa_dim);
 * 2 GEGLU (wq [2N, K], y[:, f] = gelu(acc[:, N+f]) * acc[:, f], as ttv_linear_geglu). */
int ttv_linear_fp8(const void* xq, int ldx, const float* x_scale, const void* wq, int ldw, const float* w_scale, void* y, int ldy, int M, int N,
                   int K, int epilogue, const float* rope_cs, int d_model, int gqa_dim, void* stream);

/* Split image of an fp32 matrix [rows, K] (K % 4 == 0) for the three-pass bf16 linears (ttv_tower_weights.f32_split3): for every aligned
 * group of four k values the 16 bytes (hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3) with hi = bf16(x), lo = bf16(x - hi) (round to nearest even).
 * out has the size and leading dimension (in fp32 elements) of the input.  The image is what k_gemm_f32<.., SPLIT> stages with the copies
 * of the fp32 kernel; no reference counterpart (the reference computes in the parameter dtype, titok.py:61). */
int ttv_split3_pack(const float* w, int ldw, void* out, int ldo, int rows, int K, void* stream);
/* y[M,N] fp32 = x[M,K] fp32 @ W^T (+ bias fp32) with W given as its split image: the three-pass bf16 linear on its own (tests; the towers
 * reach the same kernel with their own epilogues).  Replaces nn.Linear (blocks.py:49,93; transformer.py:73-76) in the split-bf16 mode. */
int ttv_linear_split3(const float* x, int ldx, const void* w_image, int ldw, const float* bias, float* y, int ldy, int M, int N, int K, void* stream);

/* Block-scaled (OCP MX) e4m3 quantisation of rows [rows, width] (dtype bf16 / fp32, width % 128 == 0): q[r, k] = round_e4m3(y / 2^E),
 * one E8M0 byte E + 127 per 32 consecutive k, E = ceil(log2(max|block| / 448)); with row_scales != NULL (weights) y = in / row_scales[r],
 * row_scales[r] = max|row| / 448, else y = in.  mx: ttv_mx_scale_bytes_per_row(width) bytes per row, block b = k / 32 at byte
 * (b & 3) * nkp + (b >> 2), nkp = round_up(width / 128, 4) (the order the MFMA lanes of ttv_linear_fp8_mx read them in).
 * Not a reference feature (the reference runs bf16 autocast, configs/tiny.yaml:70): BASELINE.json configs[4] "mixed bf16/fp8 MFMA". */
int64_t ttv_mx_scale_bytes_per_row(int width);
int ttv_quant_mx_fp8(const void* in, int dtype, int ld_in, void* out, int ld_out, void* mx, float* row_scales, int rows, int width, void* stream);
/* y[M,N] (bf16) = epilogue( (xq * 2^Ex) (wq * 2^Ew)^T * x_row_scale[m] * w_row_scale[n] ) on v_mfma_scale_f32_16x16x128_f8f6f4 with the
 * block scales as the instruction's scale operands; x_row_scale / w_row_scale may be NULL (= 1).  epilogue 0 store, 1 qkv + rotary
 * (as ttv_linear_fp8), 2 GEGLU (wq [2N, K]), 3 y = alpha * resid + acc (resid [M,N] bf16, ldr; y may alias resid).
 * Replaces the linears of transformer.py:47-56,86-104 in the mixed-precision configuration. */
int ttv_linear_fp8_mx(const void* xq, int ldx, const void* x_mx, const float* x_row_scale, const void* wq, int ldw, const void* w_mx,
                      const float* w_row_scale, void* y, int ldy, int M, int N, int K, int epilogue, const float* rope_cs, int d_model,
                      int gqa_dim, const void* resid, int ldr, float alpha, void* stream);

/* ---- single ops (exported for parity tests; the tower entry points below chain them) ------------------ */

/* RMSNorm (flash_attn RMSNorm as used at blocks.py:51-52,66 / transformer.py:42,77,122-123):
 * out[dst_rows[i]] = in[src_rows[i]] * rsqrt(mean(in^2)+eps) * gain, fp32 math.  Row maps may be NULL (identity). */
int ttv_rmsnorm(const void* in, int in_dtype, int ld_in, const int32_t* src_rows, void* out, int out_dtype, int ld_out,
                const int32_t* dst_rows, const float* gain, int rows, int width, float eps, void* stream);

/* apply_rotary_emb (model/base/rope.py:19-27) on x [rows, heads, 64] in place; rope_cs fp32 [rows,64] =
 * (cos[32] | sin[32]) per row, entries 30,31 = (1,0) so the last 4 dims of a head stay untouched. */
int ttv_rope_apply(void* x, int dtype, int ld, int rows, int heads, const float* rope_cs, void* stream);
/* The inverse rotation (by -theta: the sine half of rope_cs negated), in place: what the fp32 attention backward applies to dq and dk.
 * Same arguments; ld a multiple of 4 and >= heads * 64, x aligned to 4 elements, else TTV_ERR_INVALID. */
int ttv_rope_apply_conj(void* x, int dtype, int ld, int rows, int heads, const float* rope_cs, void* stream);

/* y[M,N] = x[M,K] @ w[N,K]^T (+ bias[N]) (+ *add_scalar): nn.Linear (blocks.py:93,166,173; transformer.py:49,55,87,104). */
int ttv_linear(const void* x, int ldx, const void* w, int ldw, const void* bias, const float* add_scalar, void* y, int ldy,
               int M, int N, int K, int dtype, void* stream);

/* to_qkv + rotary (transformer.py:87,97-98): y[M, 2d+2g] = x @ w^T with apply_rotary_emb fused on the q columns
 * [0,d) and k columns [2d,2d+g); rope_cs as in ttv_rope_apply. */
int ttv_linear_qkv_rope(const void* x, int ldx, const void* w, int ldw, void* y, int ldy, int M, int d_model, int gqa_dim,
                        const float* rope_cs, int dtype, void* stream);
/* GEGLU w12 + activation (transformer.py:49-52): w [2I,K]; y[M,I] = gelu_erf(x@w[I:]^T) * (x@w[:I]^T). */
int ttv_linear_geglu(const void* x, int ldx, const void* w, int ldw, void* y, int ldy, int M, int I, int K, int dtype,
                     void* stream);
/* out_proj / w3 + residual (transformer.py:129-130,141,144): y = alpha*resid + x@w^T; y is fp32 when y_f32 != 0
 * (the KEEL pre-norm sum), else dtype (in-place on resid allowed). */
int ttv_linear_residual(const void* x, int ldx, const void* w, int ldw, const void* resid, int ldr, float alpha, void* y,
                        int ldy, int y_f32, int M, int N, int K, int dtype, void* stream);

/* The whole KEEL step of one sub-layer (transformer.py:141-142 / 144-145) in one kernel:
 * y = RMSNorm(alpha*resid + x@w^T) * gain, stored in dtype (y may alias resid).  Returns TTV_ERR_UNSUPPORTED unless a
 * full-row kernel exists for the shape (bf16, N == 256, K % 8 == 0); callers then use ttv_linear_residual + ttv_rmsnorm. */
int ttv_linear_residual_norm(const void* x, int ldx, const void* w, int ldw, const void* resid, int ldr, float alpha,
                             const float* gain, float eps, void* y, int ldy, int M, int N, int K, int dtype, void* stream);

/* Whole GEGLU sub-layer (transformer.py:47-56) + residual/KEEL step (:130, :144-145) in one kernel, bf16, width 256:
 * y = [RMSNorm](alpha*x + (gelu(xn@w12[I:]^T) * (xn@w12[:I]^T)) @ w3^T) [* post_gain], xn = RMSNorm(x)*norm_gain.
 * mlp_packed = ttv_mlp_pack(w12 * norm_gain[None,:], w3, out_proj, next_qkv_folded, next_qkv_rows): the panel images the
 * kernels stream by LDS-DMA (built once per weight version, ttv_mlp_pack_bytes(inner, next_qkv_rows) bytes; out_proj and
 * next_qkv_folded may be NULL / 0 when the parts that use them are not); post_gain NULL = plain residual (layer 0).
 * y may alias x.  TTV_ERR_UNSUPPORTED for other dtypes/widths. */
int64_t ttv_mlp_pack_bytes(int inner, int next_qkv_rows);
int ttv_mlp_pack(const void* w12_folded, const void* w3, const void* out_proj, const void* next_qkv_folded, int next_qkv_rows, int inner,
                 int width, int dtype, void* mlp_packed, void* stream);
int ttv_mlp_fused(const void* x, int ldx, const void* mlp_packed, int inner, void* y, int ldy, const float* post_gain, float alpha,
                  float eps, int M, int width, int dtype, void* stream);
/* Optional last part of ttv_layer_tail_fused: the NEXT layer's attention input (transformer.py:86-98),
 * qkv = rotary(RMSNorm(y) @ (to_qkv * pre_ln_gain)^T), rows = 2d+2g of the folded weight packed by ttv_mlp_pack. */
typedef struct ttv_next_qkv {
  void* qkv; int32_t ld;        /* [M, ld] output (q | gate | k | v) */
  const float* rope_cs;         /* [M, 64] (cos | sin) */
  int32_t rows;                 /* % 64 == 0 */
  int32_t rope_q_end, rope_k_begin, rope_k_end;   /* rotary applies to features [0, q_end) and [k_begin, k_end); whole heads */
} ttv_next_qkv;
/* Everything of a transformer layer after the attention kernel (transformer.py:104, 129-130 / 141-145) in one kernel:
 *   x1 = [RMSNorm](attn_alpha*x + ao@out_proj^T) [* attn_post_gain]          (gain NULL = plain residual, layer 0)
 *   y  = [RMSNorm](ffd_alpha*x1 + GEGLU-feed-forward(x1)) [* ffd_post_gain]   (as ttv_mlp_fused)
 *   next->qkv = the next layer's rotated qkv projection of y                  (next NULL = not computed)
 * y may alias x (it is also used to hand x1 from one wave to its partner inside a workgroup).  Same support as ttv_mlp_fused. */
int ttv_layer_tail_fused(const void* ao, int ldao, const float* attn_post_gain, float attn_alpha, const void* x, int ldx,
                         const void* mlp_packed, int inner, void* y, int ldy, const float* ffd_post_gain, float ffd_alpha, float eps,
                         int M, int width, int dtype, const ttv_next_qkv* next, void* stream);

/* Token / patch initialisation of the towers (blocks.py:95-97 encoder, :165-167 decoder), exported for parity tests:
 * constant rows x[rows_map[i]] = RMSNorm(mask_token * 1_d) * gain - the encoder's latent rows (ln_pre_t) and the decoder's patch
 * rows (ln_pre_p); */
int ttv_fill_const_rows(void* x, int dtype, int ld, const int32_t* rows_map, int rows, int width, const float* mask_token,
                        const float* gain, float eps, void* stream);
/* the decoder's latent rows x[rows_map[i]] = RMSNorm(proj_in(codes[i]) + mask_token) * gain (blocks.py:125,165-166):
 * codes [rows, token_size] (dtype), w [width, token_size], bias [width] (dtype). */
int ttv_decoder_embed(const void* codes, int token_size, const void* w, const void* bias, const float* mask_token, const float* gain,
                      void* x, int dtype, int ld, const int32_t* rows_map, int rows, int width, float eps, void* stream);
/* The same, also writing the training tape's pre-norm row hpre [rows, width] (dtype, dense, row i of codes; NULL: not written) =
 * round_T(round_T(proj_in(codes[i]) + bias) + (T) mask_token): x is bit for bit what ttv_decoder_embed writes. */
int ttv_decoder_embed_tape(const void* codes, int token_size, const void* w, const void* bias, const float* mask_token, const float* gain,
                           void* x, int dtype, int ld, const int32_t* rows_map, int rows, int width, float eps, void* hpre, void* stream);

/* flash_attn_varlen_func as called at transformer.py:100, fused with the sigmoid gate of transformer.py:103:
 * qkvg [L, 2d+2g] packed (q | gate | k | v) with RoPE already applied to q,k; out [L,d] = attn * sigmoid(gate).
 * Non-causal, block-diagonal over cu_seqlens (device int32 [n_seq+1]), GQA, softmax scale head_dim^-0.5.
 * qblocks: device int32 [n_qblocks,4] work table = (sequence id, first query row within the sequence, q-head, mode), one
 * entry per query block per q-head; sequence id -1 = padding.  mode 0: 128 query rows; mode 1 ("half item"): 64 query rows
 * with the key range split between the two wave pairs of the block and merged at the end - about half the duration of a
 * full item, used by the host to fill the tail of the grid at a finer grain.  The host orders the table so that
 * entries i, i+8, i+16, ... (one XCD under round-robin dispatch) share a (sequence, kv-head): its K/V are then fetched into
 * one L2 only; half items come last.
 * flags: bit 0 (TTV_ATTN_GATE) multiply by sigmoid(gate), else the raw attention output is written; bit 1 (TTV_ATTN_PAIRED,
 * bf16 only) the table is PAIRED: with the flat table read as rows of 8 list slots (entry i belongs to list i % 8), entries
 * 2j and 2j+1 of a list describe the same (sequence, query rows, mode) for two q-heads of one kv-head; one 8-wave block then
 * computes both and stages every K / V tile once for the two heads. */
#define TTV_ATTN_GATE 1
#define TTV_ATTN_PAIRED 2
#define TTV_ATTN_QSCALED 4   /* bf16: the q columns already carry the factor head_dim^-0.5 * log2(e) (see ttv_layer_weights.qkv_q_prescaled) */
#define TTV_ATTN_ALLFULL 8   /* the table holds full items only (mode 0 everywhere, padding entries allowed) */
#define TTV_ATTN_PIPE 16     /* bf16, with TTV_ATTN_QSCALED | TTV_ATTN_ALLFULL and no tape: run the software-pipelined kernel (opt-in: measured
                                slower than the plain loop, see ttv_attn.hip; the towers set it under the environment switch TTV_ATTN_PIPE=1) */
#define TTV_ATTN_SPLIT3 32   /* fp32: the split-bf16 ("three-pass") kernel - operands hi + lo in bf16, three bf16 MFMA passes per product, fp32
                                softmax and accumulation (~2^-17 relative per product); the towers set it with ttv_tower_weights.f32_split3 */
#define TTV_ATTN_SPLIT_OUT 64 /* with TTV_ATTN_SPLIT3: the output is written as the split image of the following linear's operand (ttv_split3_pack's
                                format, same bytes as the fp32 output) */
#define TTV_ATTN_SPLIT_IN 128 /* with TTV_ATTN_SPLIT3: q, k and v arrive as planar split images (per 8 features hi0..7 | lo0..7, what the to_qkv linear
                                 of a split tower writes; the gate columns fp32): staged by LDS-DMA */
int ttv_attention(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* qblocks,
                  int n_qblocks, int q_heads, int kv_heads, int head_dim, int flags, int dtype, void* stream);
/* The same operator (transformer.py:100,103) on the 64-query-rows-per-wave kernel: bf16, head_dim 64, q pre-scaled (flags must carry
 * TTV_ATTN_QSCALED; TTV_ATTN_GATE as above).  One workgroup = 4 waves (two workgroups per CU), each wave with 64 query rows (two 32-row tiles that
 * share every K / V fragment read) of any q-head of ONE (sequence, kv-head).  items: device int32 [n_items, 8] =
 * (sequence id, kv-head, wave 0..3: q-head | (first query row / 64) << 8, or -1 for an idle wave, cu_seqlens[sequence], sequence length);
 * sequence id -1 = padding.
 * The host orders the table so that entries i, i+8, ... (one XCD under round-robin dispatch) share a (sequence, kv-head). */
int ttv_attention64(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* items, int n_items,
                    int q_heads, int kv_heads, int head_dim, int flags, int dtype, void* stream);

/* OPT-IN, INFERENCE: the same operator with its second product in 8 bits (bf16 rows, head_dim 64, q pre-scaled).  S = Q K^T and the
 * softmax are ttv_attention's (bf16 operands, fp32); P enters P.V as e4m3_rne(p * 2^6) against a running reference that lags the row
 * maximum by at most 2 log2 units (never saturated), V as an OCP-MX e4m3 image - one E8M0 scale per 32 keys (the natural halves of a
 * 64-key tile counted from the sequence's first row) and head-dim column, scale rule of ttv_quant_mx_fp8 - and the product runs on
 * v_mfma_scale_f32_32x32x64_f8f6f4 with fp32 accumulation; row sums add the fp32 p.  Accuracy price: ~2^-5 relative per p (e4m3's three
 * mantissa bits) and per v instead of bf16's 2^-9 - DESIGN.md section 4z has the bound and the measured figures.
 *   ttv_attention_pv8_bytes: size of the image for a packed batch ((total_rows / 64 + n_seqs) * kv_heads tiles of 4 224 bytes); -1 for
 *     negative sizes.
 *   ttv_quant_v_pv8: writes the image of the v columns of qkvg [total_rows, ld] (layout: csrc/ttv_attn_pv8.hip, restated in
 *     tests/pv8_ref.py); `image` 16-byte aligned; cu_seqlens device int32 [n_seqs + 1] with cu_seqlens[n_seqs] == total_rows.
 *   ttv_attention_pv8: ttv_attention's arguments and work tables (mode-1 entries run without the key split; a paired table is walked
 *     entry by entry); flags MUST carry TTV_ATTN_QSCALED (the caller's statement that q is pre-scaled) and may carry TTV_ATTN_GATE,
 *     nothing else; `image` is what ttv_quant_v_pv8 wrote for the same qkvg, cu_seqlens and head counts.  TTV_ERR_INVALID with a
 *     message and nothing launched: head_dim other than 64, q not pre-scaled, any other flag, qkvg / out / image not 16-byte aligned,
 *     ld or ldo not a multiple of 8 or too small. */
int64_t ttv_attention_pv8_bytes(int total_rows, int n_seqs, int kv_heads);
int ttv_quant_v_pv8(const void* qkvg, int ld, const int32_t* cu_seqlens, int n_seqs, int total_rows, int q_heads, int kv_heads, void* image,
                    void* stream);
int ttv_attention_pv8(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* qblocks, int n_qblocks,
                      int q_heads, int kv_heads, int head_dim, int flags, const void* image, void* stream);

/* The three producers of the block-scaled fp8 layers that write the next linear's operand themselves, each on its own.  FOR TESTS
 * ONLY (tests/test_hip_fp8_blocks.py): the towers reach the same kernels inside ttv_encoder_forward / ttv_decoder_forward; no caller
 * needs them one by one.  Each image must equal ttv_quant_mx_fp8 of the bf16 rows its plain twin stores, bit for bit: elements
 * [rows, width] bytes (leading dimension = width), scales ttv_mx_scale_bytes_per_row(width) bytes per row in ttv_quant_mx_fp8's layout.
 *   ttv_rmsnorm_mx: ttv_rmsnorm without row maps; next_rstd fp32 [rows] (may be NULL) receives rsqrt(mean(out^2) + eps) of the rows as
 *     stored; mx_q / mx_s (both or neither; width % 128 == 0) the image of the rows as stored.
 *   ttv_attention_mxout: ttv_attention (bf16, head_dim 64, TTV_ATTN_GATE | TTV_ATTN_QSCALED, unpaired table) whose output leaves only
 *     as the image out_q / out_mx (ld_mx = ttv_mx_scale_bytes_per_row(64 * q_heads)).
 *   ttv_linear_fp8_mx_geglu_q: ttv_linear_fp8_mx with epilogue 2 whose output h [M, N] leaves only as the image hq / hq_mx (N % 128 == 0). */
int ttv_rmsnorm_mx(const void* in, int in_dtype, int ld_in, void* out, int out_dtype, int ld_out, const float* gain, int rows, int width,
                   float eps, float* next_rstd, void* mx_q, void* mx_s, void* stream);
int ttv_attention_mxout(const void* qkvg, int ld, void* out_q, void* out_mx, int ld_mx, const int32_t* cu_seqlens, const int32_t* qblocks,
                        int n_qblocks, int q_heads, int kv_heads, void* stream);
int ttv_linear_fp8_mx_geglu_q(const void* xq, int ldx, const void* x_mx, const float* x_row_scale, const void* wq, int ldw, const void* w_mx,
                              const float* w_row_scale, void* hq, void* hq_mx, int M, int N, int K, void* stream);

/* The folded pre-norm of the wide bf16 layer (widths other than 256: the gain lives in the weight, the row statistic multiplies the
 * GEMM's output rows), launch by launch.  FOR TESTS ONLY (tests/test_hip_wide_layer.py): the towers make the same launches inside
 * ttv_encoder_forward / ttv_decoder_forward; the public linears carry no row scale.
 *   ttv_row_rstd: rstd[r] = rsqrt(mean(x[r, :width]^2) + eps), fp32 [rows]; x bf16 or fp32, ldx >= width, width % 8 == 0.
 *   ttv_linear_rowscale: y = epilogue((x @ w^T) * row_scale[:, None]); epilogue 0 = store, 1 = to_qkv + rotary (ttv_linear_qkv_rope:
 *     N = 2 d_model + 2 gqa_dim, K = d_model), 2 = GEGLU (ttv_linear_geglu: w holds 2N rows, y [M, N]).  row_scale fp32 [M] or NULL
 *     (then the launch is the public linear's).  The kernel is chosen as for the public linears (ttv_debug_set forces one). */
int ttv_row_rstd(const void* x, int dtype, int ldx, float* rstd, int rows, int width, float eps, void* stream);
int ttv_linear_rowscale(const void* x, int ldx, const void* w, int ldw, const float* row_scale, int epilogue, const float* rope_cs, int d_model,
                        int gqa_dim, void* y, int ldy, int M, int N, int K, int dtype, void* stream);

/* patch_rearrange (model/base/utils.py:26-34) for up to TTV_MAX_CLIPS_PER_LAUNCH clips per call.
 * clips: HOST array of device pointers [n_clips] to [C,T,H,W] tensors; clip_desc: DEVICE int32 [n_clips,8] =
 * (T,H,W, gt,gh,gw, first patch row, C).  Output rows hold the patch vector in (c,pt,ph,pw) order - the
 * reference's (pt,ph,pw,c) order is folded into the packed proj_in / proj_out weight (see weights.py). */
int ttv_patch_gather(const void* const* clips, const int32_t* clip_desc, int clip0, int n_clips, int patch_t, int patch_h,
                     int patch_w, int channels, void* patches, int ld, int dtype, int max_patches_per_clip, void* stream);
/* The encoder's front in one kernel (blocks.py:91-97): x[patch_rows[t]] = RMSNorm(bf16(bf16(patch t . w^T + bias) + mask_token)) * gain
 * for the `rows` patches of n_clips clips (<= TTV_MAX_CLIPS_PER_LAUNCH), read straight from the clips - what ttv_patch_gather, ttv_linear
 * (bias, mask token as add_scalar) and ttv_rmsnorm (dst_rows = patch_rows) compute as three launches, bit for bit (the k order of
 * those GEMM kernels and the row kernel's summation order are kept).  w [width, C*pt*ph*pw] in (c,pt,ph,pw) order, bias [width] (dtype), gain fp32 [width];
 * row_seq [L] = clip of every packed row (ttv_batch.row_seq).  bf16, width 256, patch_w 8, power-of-two patch_t / patch_h and a patch
 * vector that is a multiple of 64; anything else returns TTV_ERR_UNSUPPORTED. */
int ttv_patch_embed_norm(const void* const* clips, const int32_t* clip_desc, const int32_t* patch_rows, const int32_t* row_seq, int n_clips,
                         int patch_t, int patch_h, int patch_w, int channels, const void* w, int ldw, const void* bias,
                         const float* mask_token, const float* gain, float eps, void* x, int ldx, int rows, int width, int dtype,
                         void* stream);
/* unpatch_rearrange (model/base/utils.py:37-51); same descriptors, clips are written. */
int ttv_patch_scatter(const void* patches, int ld, const int32_t* clip_desc, int clip0, int n_clips, int patch_t, int patch_h,
                      int patch_w, int channels, void* const* clips, int dtype, int max_patches_per_clip, void* stream);

/* ---- towers (model/base/blocks.py TiTokEncoder 31-104 / TiTokDecoder 108-177) ------------------------- */
typedef struct ttv_tower_dims {
  int32_t kind;          /* TTV_ENCODER / TTV_DECODER */
  int32_t dtype;         /* compute dtype */
  int32_t width;         /* d                                   utils.py:22 */
  int32_t layers;        /*                                     utils.py:9-14 */
  int32_t q_heads, kv_heads, head_dim;   /*                     utils.py:15-20, transformer.py:73-75 */
  int32_t inner;         /* GEGLU hidden I                      transformer.py:39-40 */
  int32_t patch_t, patch_h, patch_w;
  int32_t pix_channels;  /* 3 */
  int32_t token_size;    /* len(fsq_levels) (encoder out / decoder in); 1 for the discriminator use; up to TTV_MAX_TOKEN for the
                            towers in front of / behind ttv_vq_l2_argmin, inference and training alike (the L2 quantiser trains since
                            round 4: ttv_train.hip's check() accepts token_size <= TTV_MAX_TOKEN) */
  float eps;             /* RMSNorm eps 1e-5 */
  float alpha;           /* KEEL residual scale 2*layers        transformer.py:117 */
} ttv_tower_dims;

typedef struct ttv_layer_weights {
  const float* pre_ln;        /* attn_layer.i.pre_ln.weight [d]            */
  const void* to_qkv;         /* attn_layer.i.to_qkv.weight [2d+2g, d]     */
  const void* out_proj;       /* attn_layer.i.out_proj.weight [d, d]       */
  const float* ffd_norm;      /* ffd_layer.i.norm.weight [d]               */
  const void* w12;            /* ffd_layer.i.w12.weight [2I, d]            */
  const void* w3;             /* ffd_layer.i.w3.weight [d, I]              */
  const float* attn_post_ln;  /* attn_post_ln.(i-1).weight, NULL for i==0  */
  const float* ffd_post_ln;   /* ffd_post_ln.(i-1).weight, NULL for i==0   */
  /* optional (bf16, width 256): to_qkv / w12 with the preceding RMSNorm gain folded into the columns
   * (w * gain[None,:]); when non-NULL the pre-norm runs inside the GEMM (rstd from the register-resident row) */
  const void* to_qkv_pn;
  const void* w12_pn;
  /* optional (bf16, width 256): ttv_mlp_pack(w12_pn, w3, out_proj, NEXT layer's to_qkv_pn, rows) - panel images of the fused
   * layer-tail kernel; mlp_pack_qkv_rows = rows of the next layer's to_qkv packed into it (0 = none, e.g. last layer) */
  const void* mlp_pack;
  int32_t mlp_pack_qkv_rows;
  /* 1: the q rows of to_qkv_pn (and of the next-layer image inside the previous layer's mlp_pack) are multiplied by
   * head_dim^-0.5 * log2(e): the projection then emits the softmax exponent directly and the attention kernel runs with
   * TTV_ATTN_QSCALED (one multiply-add less per score).  Inference towers only; `to_qkv` itself is never scaled. */
  int32_t qkv_q_prescaled;
  /* optional (bf16, any width; used where to_qkv_pn is not): an inference copy of to_qkv whose q rows carry the same factor;
   * NULL = use to_qkv and the plain attention kernel */
  const void* to_qkv_qs;
  /* optional mixed bf16 / fp8 linears (BASELINE config #5; bf16 towers, width % 128 == 0, used where the folded width-256 kernels are
   * not): to_qkv (its q rows pre-scaled like to_qkv_qs when that is given) and w12 in OCP e4m3 with one fp32 scale per weight row
   * (ttv_quant_rows_fp8).  When non-NULL the pre-norm output is quantised per token and the two projections run on the fp8 MFMA. */
  const void* to_qkv_f8; const float* to_qkv_f8_scale;
  const void* w12_f8; const float* w12_f8_scale;
  /* optional block-scaled (MX) fp8 linears - ALL FOUR linears of the layer on the fp8 MFMA (round 4): when every pointer below and the
   * four e4m3 images are non-NULL (bf16 towers, width != 256, width % 128 == 0, inner % 128 == 0) the layer quantises each linear's
   * input with ttv_quant_mx_fp8 (one E8M0 scale per 32 consecutive elements) and runs ttv_linear_fp8_mx.  The images then hold
   * ttv_quant_mx_fp8(W', row factors) with W' = to_qkv * pre_ln gain (q rows pre-scaled) / w12 * ffd_norm gain / out_proj / w3: the
   * pre-norm is folded (its rstd is the activation's per-row factor in the epilogue), `*_f8_scale` are the weight rows' fp32 factors,
   * `*_mx` the block scales in ttv_quant_mx_fp8's layout. */
  const void* to_qkv_mx; const void* w12_mx;
  const void* out_proj_f8; const float* out_proj_f8_scale; const void* out_proj_mx;
  const void* w3_f8; const float* w3_f8_scale; const void* w3_mx;
} ttv_layer_weights;

typedef struct ttv_tower_weights {
  const void* proj_in_w;      /* enc: [d, C*pt*ph*pw] columns in (c,pt,ph,pw) order; dec: [d, token_size] */
  const void* proj_in_b;      /* [d] */
  const float* mask_token;    /* [1] */
  const float* ln_pre_t;      /* [d] */
  const float* ln_pre_p;      /* [d] */
  const float* ln_post;       /* [d] */
  const void* proj_out_w;     /* enc: [token_size, d]; dec: [C*pt*ph*pw, d] rows in (c,pt,ph,pw) order */
  const void* proj_out_b;     /* enc: [token_size]; dec: [C*pt*ph*pw] same order */
  const ttv_layer_weights* layers;   /* HOST array [layers] */
  /* optional (decoder, bf16, width 256): proj_out_w * ln_post gain[None,:]; when non-NULL the ln_post RMSNorm runs inside the
   * proj_out GEMM (rows gathered through patch_rows, rstd from the register-resident row) */
  const void* proj_out_pn;
  /* fp32 towers, inference: 1 = "split-bf16" arithmetic (round 4).  proj_in_w and the layers' to_qkv / out_proj / w12 / w3 then point at
   * SPLIT IMAGES made by ttv_split3_pack (same bytes and leading dimension as the fp32 matrix), every linear runs as three bf16 MFMA
   * passes on hi + lo operands (fp32 accumulation) and the attention kernel with TTV_ATTN_SPLIT3; norms, rotary, softmax, GELU, the
   * residual stream, the encoder tail and FSQ stay exact fp32.  Measured: every token index of the reference's fp32 run is kept on the
   * benchmark fixture (max |pre-rounding FSQ value error| ~6e-4) at about a third of the exact-fp32 MFMA kernels' time. */
  int32_t f32_split3;
  /* bf16 towers, inference: 1 = every layer's attention runs ttv_quant_v_pv8 + ttv_attention_pv8 (e4m3 P.V, see there) in place of the
   * bf16 kernels - the plain, the wide and the block-scaled fp8 layer paths alike; the image lives in the workspace's GEGLU buffer,
   * which is dead during attention (ttv_tower_workspace_bytes is unchanged; a batch whose image does not fit is refused).  The decoder's
   * layer-0 constant block and the software-pipelined kernel stay off.  TTV_ERR_INVALID: fp32 and split-bf16 towers, a layer whose q is
   * not pre-scaled.  The *_forward_train* entry points ignore the field.  (Sits in the struct's tail padding: sizeof is unchanged.) */
  int32_t attn_pv8;
} ttv_tower_weights;

/* Per-batch metadata, built on the host from Python ints (replaces the device-side bookkeeping and its
 * host syncs at blocks.py:80-88 / 154-162 and rope.py:57-71).  All pointers are DEVICE pointers. */
typedef struct ttv_batch {
  int32_t n_clips;
  int32_t total_rows;          /* L = sum(K_b + P_b) */
  int32_t sum_tokens;          /* sum K_b */
  int32_t sum_patches;         /* sum P_b */
  int32_t max_patches_per_clip;
  int32_t n_qblocks;
  const int32_t* cu_seqlens;   /* [n_clips+1] */
  const int32_t* latent_rows;  /* [sum_tokens]  packed row of every latent token, clip-major */
  const int32_t* patch_rows;   /* [sum_patches] packed row of every patch token, clip-major */
  const int32_t* clip_desc;    /* [n_clips,8] see ttv_patch_gather */
  const int32_t* qblocks;      /* [n_qblocks,4] see ttv_attention (built for this tower's head counts) */
  const float* rope_cs;        /* [L,64] cos|sin, fp64-evaluated on the host as rope.py:48-54 */
  /* training only (may be NULL for inference): */
  const int32_t* blocks64;     /* [n_blocks64,2] (sequence, first row) of every 64-row block (attention backward) */
  const int32_t* row_seq;      /* [L] sequence id of every packed row */
  int32_t n_blocks64;
  int32_t qblocks_paired;      /* 1: entries 2j, 2j+1 of every XCD list of `qblocks` are the same query rows of two q-heads sharing
                                  a kv-head (ttv_attention flag TTV_ATTN_PAIRED); 0: no such guarantee */
  int32_t qblocks_all_full;    /* 1: `qblocks` holds full items only (ttv_attention flag TTV_ATTN_ALLFULL) */
  /* optional: the work table of ttv_attention64 for this tower's head counts (NULL / 0: the towers use `qblocks` only).  When given,
   * inference forwards of bf16 towers whose q columns are pre-scaled run ttv_attention64 instead of ttv_attention. */
  const int32_t* items64;
  int32_t n_items64;
  /* optional: the rotary factors as indices instead of a [L,64] fp32 table (NULL: every kernel reads `rope_cs`).  rope_ids [L,2] int32 =
   * four uint16 per packed row: the position id of axes t, h, w (rope.py:59-67: latent i -> (i,i,i), patch (t,h,w) -> (t,h,w) + K) and
   * the index of the identity row; rope_base fp32 [n_ids + 1, 10, 2] = (cos, sin) of inv_freq[f] * id for every id < n_ids (the values
   * ttv_rope_table_build gathers from) with row n_ids = (1, 0).  8 bytes per row instead of 256: the width-256 to_qkv kernel gathers
   * its factors from the L2-resident base table (bit-identical values). */
  const int32_t* rope_ids;
  const float* rope_base;
  /* optional (NULL / 0: off): an attention work table (format of `qblocks`, full items only) whose entries cover just the query rows of
   * the LATENT tokens of every sequence (rows [0, K_b): the latent tokens come first, blocks.py:85-86).  The encoder's output is read
   * from its latent rows alone (blocks.py:101-103), so with this table ttv_encoder_forward runs the LAST layer's attention for those
   * query rows only (keys / values: every row, as before) and everything behind it - out_proj, KEEL norms, the feed-forward - on the
   * sum K_b latent rows instead of all L: the same values for the rows that are used, the patch rows of the last layer's output are
   * never computed.  Ignored by the decoder and by the training entry points. */
  const int32_t* qblocks_latent;
  int32_t n_qblocks_latent;
  /* optional (NULL / 0: off), the decoder-side twin: an attention work table (format of `qblocks`, full items only) without the query
   * blocks that hold latent rows ONLY (block q of a sequence with (q + 1) * 128 <= K_b).  The decoder's output is read from its patch
   * rows alone (blocks.py:171), so with this table ttv_decoder_forward runs the LAST layer's attention without those blocks: the rows
   * it skips keep the previous layer's attention output, everything behind the attention is row-wise, and no patch row changes a bit.
   * Ignored by the encoder and by the training entry points. */
  const int32_t* qblocks_patch;
  int32_t n_qblocks_patch;
  /* optional (0: no such promise): K when EVERY clip of the batch has K_b = K latent tokens and the same number of patches.  With it,
   * K and the patches per clip multiples of 128 and the width-256 bf16 kernels, the encoder's last layer - whose queries are the latent
   * rows (qblocks_latent) - computes the q | gate columns of to_qkv for the latent token tiles only; k | v for every row, as before. */
  int32_t tokens_per_clip;
} ttv_batch;

/* Fill ttv_batch.rope_cs [L,64] on the device: rows are gathered from base_cos/base_sin fp32 [n_ids, n_freqs] =
 * cos/sin(inv_freq[f] * n), evaluated once on the host in fp64 exactly as rope.py:40-54 (position ids are small integers,
 * rope.py:59-67: latent i -> (i,i,i); patch (t,h,w) -> (t,h,w) + K).  Replaces RoPE.forward's per-sample loop (rope.py:57-71). */
int ttv_rope_table_build(const float* base_cos, const float* base_sin, int n_ids, int n_freqs, const int32_t* clip_desc,
                         const int32_t* cu_seqlens, const int32_t* row_seq, float* rope_cs, int total_rows, void* stream);

/* ---- batch plans: a ttv_batch without Python ---------------------------------------------------------------
 * Everything a ttv_batch points at, from three host arrays: pixel_dims int32 [n_clips,3] = (T, H, W) of every clip, token_counts int32
 * [n_clips] = K_b, patch int32 [3] = (pt, ph, pw).  The tables are the ones titok_video_amd/plan.py (BatchPlan) builds, element for
 * element.  A host makes five calls per batch shape (plus one ttv_rope_base_table per table size, once):
 *
 *   ttv_plan_rows_sizes  -> ttv_plan_sizes (counts, word offsets)               host only
 *   ttv_plan_rows_fill   -> the HOST SEGMENT in the caller's pinned buffer      host only
 *   ttv_plan_rows_build  -> async copy + fill kernel + rope_cs, fills ttv_batch enqueues on `stream`
 *   ttv_plan_attn_sizes / ttv_plan_attn_fill -> the attention work tables of one (q_heads, kv_heads) in a pinned buffer   host only
 *   ttv_plan_attn_set    -> async copy, sets the qblocks* fields of the ttv_batch  enqueues on `stream`
 *
 * The host-only calls touch no device and read no environment variable: they work where there is no GPU, like
 * ttv_tower_workspace_bytes.  Invalid input (a null pointer, n_clips < 1, a clip dimension that is not a positive multiple of the patch,
 * a negative token count, an empty sequence, a position id table that does not fit rope_ids' uint16 slots) returns TTV_ERR_INVALID with
 * a message in ttv_error_string() and writes nothing.
 *
 * Segments are arrays of int32 words; every table in them starts 16-byte aligned (offsets are multiples of 4 words, the words between
 * a table's end and the next table are zero in the host segment and never written in the device part).
 *   HOST SEGMENT [host_words]: cu_seqlens [n_clips+1] | clip_desc [n_clips,8] (see ttv_patch_gather) | blocks64 [n_blocks64,2].
 *     blocks64 = (sequence, first row) of every 64-row block for the attention backward: whole sequences are dealt over 8 lists (longest
 *     first, stable; each to the first list with the fewest blocks), entry i comes from list i % 8 while every list has one, the rest
 *     follows list by list (no padding entries).  bwd_xcd = 0 gives the sequence-major order instead.
 *   DEVICE SEGMENT [dev_words]: the host segment's words at the same offsets, then latent_rows [sum_tokens] | patch_rows [sum_patches]
 *     | row_seq [total_rows] | rope_ids [total_rows,2], written by the fill kernel from cu_seqlens and clip_desc alone.
 * n_rope_ids is the smallest power of two that is >= 512 and > max_b(K_b + max(grid_b)). */
typedef struct ttv_plan_sizes {
  int32_t n_clips, total_rows, sum_tokens, sum_patches, max_patches_per_clip, max_seqlen, n_rope_ids, n_blocks64;
  int64_t host_words;                                    /* int32 words of the host segment */
  int64_t off_cu_seqlens, off_clip_desc, off_blocks64;   /* word offsets, the same in the host and in the device segment */
  int64_t dev_words;                                     /* int32 words of the device segment (>= host_words) */
  int64_t off_latent_rows, off_patch_rows, off_row_seq, off_rope_ids;   /* word offsets in the device segment */
} ttv_plan_sizes;

int ttv_plan_rows_sizes(const int32_t* pixel_dims, const int32_t* token_counts, int n_clips, const int32_t* patch, ttv_plan_sizes* sizes);
/* host_segment: at least sizes.host_words words (given as host_words).  For ttv_plan_rows_build it must be pinned host memory. */
int ttv_plan_rows_fill(const int32_t* pixel_dims, const int32_t* token_counts, int n_clips, const int32_t* patch, int bwd_xcd,
                       int32_t* host_segment, int64_t host_words);

/* Enqueues on `stream`: the copy of host_segment [sizes.host_words] to the head of dev_segment [sizes.dev_words, 16-byte aligned], one
 * kernel that writes latent_rows, patch_rows, row_seq and rope_ids, and the kernel of ttv_rope_table_build for rope_cs fp32
 * [total_rows,64] (base_cos / base_sin fp32 [n_rope_ids, n_freqs] on the DEVICE: ttv_rope_base_table's values).  Then fills *batch (a
 * HOST struct) with the counts and the device pointers; the qblocks* fields and items64 are left NULL / 0 for ttv_plan_attn_set.
 * rope_base: NULL (the towers read rope_cs), or the DEVICE table fp32 [n_rope_ids+1, n_freqs, 2] = (cos, sin) of ttv_rope_base_table
 * with row n_rope_ids = (1, 0); then batch.rope_ids / rope_base are set.  No allocation and no synchronisation: the caller promises
 * that host_segment is pinned and stays unchanged until the stream has passed the copy (an event recorded behind this call). */
int ttv_plan_rows_build(const ttv_plan_sizes* sizes, const int32_t* host_segment, int32_t* dev_segment, const float* base_cos,
                        const float* base_sin, int n_freqs, float* rope_cs, const float* rope_base, ttv_batch* batch, void* stream);

/* The attention work tables of one (q_heads, kv_heads) (entry format: ttv_attention), int32 [words] = qblocks [n_qblocks,4] |
 * qblocks_latent [n_qblocks_latent,4] | qblocks_patch [n_qblocks_patch,4] | the decoder's layer-0 table [n_qblocks_l0,4]
 * (ttv_dec_l0_const.qblocks: every list holds the latent-only query blocks of its units first, the others behind them).
 * Every table: the blocks of one (sequence, kv-head) unit share K / V, so units are dealt over 8 lists (heaviest first, stable; weight
 * 2 * full + half items; each to the first list of least weight), a list holds the full items of its units and behind all of them
 * their half items, entry i of the table belongs to list i % 8, shorter lists are padded with (-1,-1,-1,-1) and only the padding
 * entries at the end of the table are dropped.  Half items: split = 1 every item, 0 never, -1 the rule - with fewer than 1024 items
 * (sum of 128-row blocks * q_heads) the last third of every sequence's blocks, otherwise the last 1 / tail_div of them (tail_div <= 0:
 * none).  qblocks_latent is absent (0 entries) when sum K_b = 0; qblocks_patch exists only beside a `qblocks` of full items, and only
 * when at least one latent-only block is dropped and at least one block remains.  cu_seqlens: HOST [n_clips+1]. */
typedef struct ttv_plan_attn {
  int32_t n_qblocks, qblocks_all_full, n_qblocks_latent, n_qblocks_patch, n_qblocks_l0;
  int32_t tokens_per_clip;   /* K when every clip has K_b = K and the same number of rows, else 0 (ttv_batch.tokens_per_clip) */
  int64_t words;                                                              /* int32 words of the four tables together */
  int64_t off_qblocks, off_qblocks_latent, off_qblocks_patch, off_qblocks_l0; /* word offsets (multiples of 4) */
} ttv_plan_attn;

int ttv_plan_attn_sizes(const int32_t* cu_seqlens, const int32_t* token_counts, int n_clips, int q_heads, int kv_heads, int split,
                        int tail_div, ttv_plan_attn* sizes);
int ttv_plan_attn_fill(const int32_t* cu_seqlens, const int32_t* token_counts, int n_clips, int q_heads, int kv_heads, int split,
                       int tail_div, int32_t* host_tables, int64_t host_words);
/* Enqueues the copy of host_tables [sizes.words] (pinned, unchanged until the stream has passed it) to dev_tables (16-byte aligned) and
 * sets batch.qblocks / n_qblocks / qblocks_all_full / qblocks_latent / qblocks_patch and their counts and tokens_per_clip;
 * qblocks_paired = 0, items64 = NULL.  The layer-0 table is at dev_tables + off_qblocks_l0 for ttv_dec_l0_const.qblocks. */
int ttv_plan_attn_set(const ttv_plan_attn* sizes, const int32_t* host_tables, int32_t* dev_tables, ttv_batch* batch, void* stream);

/* base_cos / base_sin fp32 [n_ids, F], F = head_dim / (2 * nd): cos / sin of inv_freq[f] * n for every position id n < n_ids, evaluated
 * as rope.py:40-54 does - float64 theta ** linspace(0, 1, F) * pi / 2 (torch's linspace: step * i below the middle, 1 - step * (F-1-i)
 * above), float64 product with the id, cast to fp32.  Host only (libm).  ttv_batch.rope_base is these values interleaved,
 * rope_base[n][f] = (cos[n][f], sin[n][f]), with one more row n_ids = (1, 0). */
int ttv_rope_base_table(int head_dim, int nd, int n_ids, double theta, float* base_cos, float* base_sin);

/* bytes of scratch a tower forward needs for this batch */
int64_t ttv_tower_workspace_bytes(const ttv_tower_dims* dims, const ttv_batch* batch);

/* TiTokEncoder.forward (blocks.py:71-104) + FSQ.forward (fsq.py:123-135) fused at the tail:
 * clips (HOST array of device ptrs) -> z [sum_tokens, token_size] fp32 (pre-quantisation, may be NULL),
 * codes [sum_tokens, token_size] (dtype), indices int32 [sum_tokens], bounded fp32 (may be NULL).
 * If fsq == NULL only z is produced (used for the discriminator's encoder, loss_module.py:96-101). */
int ttv_encoder_forward(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_batch* batch,
                        const void* const* clips, const ttv_fsq_params* fsq, float* z, void* codes, int32_t* indices,
                        float* bounded, void* workspace, int64_t workspace_bytes, void* stream);

/* TiTokDecoder.forward (blocks.py:148-177): codes [sum_tokens, token_size] (dtype) -> clips_out
 * (HOST array of device ptrs to [C,T,H,W] buffers, dtype). */
int ttv_decoder_forward(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_batch* batch, const void* codes,
                        void* const* clips_out, void* workspace, int64_t workspace_bytes, void* stream);

/* The decoder's patch rows enter layer 0 as one constant vector, ln_pre_p(mask_token) (blocks.py:165-167): their q | gate | k | v in
 * layer 0 depend on the weights and on the rows' rotary positions only, so they are the same for every clip of one geometry (pixel grid
 * and latent count) on every call.  A CONSTANT BLOCK holds them once per (weights, geometry): `rows` bf16 [patch_rows, 2d+2g], written by
 * the kernels the forward itself runs (ttv_fill_const_rows, then layer 0's to_qkv with the folded pre-norm, the q pre-scale and the
 * rotary factors of one clip's patch rows), hence the bits the forward would write into its own workspace.  With it layer 0's to_qkv
 * computes only the 128-row token tiles that hold latent rows, and its attention reads the patch rows' q, gate, k and v from the block.
 * `state`: for every (128-row patch query block, q-head) the raw fp32 accumulators and row sums of the attention kernel (k_attn_swp keeps
 * no softmax reference: O and l are plain sums of 2^score terms) over the PATCH keys, in the kernel's register layout.  With it a patch
 * query block loops over the latent keys only and adds the state once: one fp32 addition per accumulator in another place of the sum.
 * The builder's flag word (int32 at flag_offset, device) is nonzero when one of those row sums left the kernel's 2^-60 .. 2^60 window:
 * pass state = NULL then (the attention then still reads the rows, over every key).
 * bf16 decoders of width 256, head_dim 64, with ttv_layer_weights.to_qkv_pn and qkv_q_prescaled on layer 0.
 * ttv_dec_l0_const_bytes: bytes of the block (the rows first, then the builder's scratch); -1 when the tower is not of that kind.
 * ttv_dec_l0_const_build: iota = device int32 [patch_rows] 0, 1, ..; rope_cs [patch_rows, 64] / rope_ids [patch_rows, 2] (optional, with
 * rope_base) = the rows of ttv_batch.rope_cs / rope_ids that belong to the patch rows of ONE clip of the geometry; block 256-byte aligned.
 * Rebuild after any change of the weights. */
typedef struct ttv_dec_l0_const {
  const void* rows;       /* the block (its first patch_rows * (2d+2g) bf16 are the rows) */
  int32_t latent_rows;    /* K: latent rows of every clip of the batch (they come first in a sequence) */
  int32_t patch_rows;     /* P: patch rows of every clip of the batch */
  const float* state;     /* block + state_offset, or NULL (flag set, or A/B) */
  const int32_t* qblocks; /* optional attention work table for layer 0 (format of ttv_batch.qblocks, full items): the batch's items with */
  int32_t n_qblocks;      /* the latent query blocks - the long ones - first; NULL / 0: ttv_batch.qblocks */
} ttv_dec_l0_const;
int64_t ttv_dec_l0_const_bytes(const ttv_tower_dims* dims, int patch_rows);
int ttv_dec_l0_const_build(const ttv_tower_dims* dims, const ttv_tower_weights* w, const int32_t* iota, const float* rope_cs,
                           const int32_t* rope_ids, const float* rope_base, int patch_rows, void* block, int64_t block_bytes,
                           int64_t* state_offset, int64_t* flag_offset, void* stream);
/* ttv_decoder_forward with the constant block of this batch's geometry (NULL: ttv_decoder_forward).  The caller promises that EVERY clip
 * of the batch has the geometry the block was built for and that the block belongs to `w`.  The block is used when K and P are multiples
 * of 128, the batch's table holds full unpaired items and layer 0 runs the width-256 bf16 kernels; otherwise, and with TTV_DEC_L0_CONST=0,
 * the call is ttv_decoder_forward.  Without `state` the output is the same bits; with it the patch query rows of layer 0's attention
 * differ by the re-association of one fp32 sum. */
int ttv_decoder_forward_const(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_batch* batch, const void* codes,
                              void* const* clips_out, void* workspace, int64_t workspace_bytes, const ttv_dec_l0_const* l0, void* stream);

/* ---- training step: tape-recording forward + backward (reference train.py:65-83 = autograd through the towers) ------- */
/* Transposed linear weights for the data-gradient GEMMs (dX = dY W is run as dY (W^T)^T), compute dtype. */
typedef struct ttv_layer_weights_t {
  const void* to_qkv_t;    /* [d, 2d+2g]  */
  const void* out_proj_t;  /* [d, d]      */
  const void* w12_t;       /* [d, 2I]     */
  const void* w3_t;        /* [I, d]      */
} ttv_layer_weights_t;
typedef struct ttv_tower_weights_t {
  const void* proj_in_t;   /* encoder: [C*pt*ph*pw, d] (packed order); decoder: unused (NULL) */
  const void* proj_out_t;  /* decoder: [d, C*pt*ph*pw] (packed order); encoder: unused (NULL) */
  const ttv_layer_weights_t* layers;   /* HOST array [layers] */
} ttv_tower_weights_t;
/* fp32 gradient buffers, same shapes/layout as the PACKED weights of ttv_tower_weights; zeroed by the caller, accumulated into. */
typedef struct ttv_layer_grads {
  float* pre_ln; float* to_qkv; float* out_proj; float* ffd_norm; float* w12; float* w3; float* attn_post_ln; float* ffd_post_ln;
} ttv_layer_grads;
typedef struct ttv_tower_grads {
  float* proj_in_w; float* proj_in_b; float* mask_token; float* ln_pre_t; float* ln_pre_p; float* ln_post; float* proj_out_w;
  float* proj_out_b;
  const ttv_layer_grads* layers;       /* HOST array [layers] */
  /* optional HOST array [layers] of hipEvent_t (created by the caller): event i is recorded on `stream` right after the last kernel
   * that writes layer i's gradients (the backward visits the layers top down, so these complete in the order layers-1 .. 0).  A
   * data-parallel caller makes its communication stream wait for event i and all-reduces layer i's gradient slice while the
   * backward of the layers below is still running (reference step: train.py:75-83).  NULL = no events. */
  void** layer_done_events;
} ttv_tower_grads;

int64_t ttv_tower_tape_bytes(const ttv_tower_dims* dims, const ttv_batch* batch);
int64_t ttv_tower_bwd_workspace_bytes(const ttv_tower_dims* dims, const ttv_batch* batch);
/* Tape modes of the *_ex entry points below (each plain entry point is its _ex with TTV_TAPE_STORED; a forward and its backward take the
 * same mode and the same tape).
 * TTV_TAPE_STORED   : the forward writes, for every layer, every tensor the backward reads.
 * TTV_TAPE_RECOMPUTE: the tape holds the tower's head / tail buffers, the residual stream at the layers + 1 layer boundaries and
 *   min(2, layers) layer slots (each the size of one layer's region of the stored tape, for a layer > 0).  The forward runs the same
 *   kernels with layer i writing slot i & 1; the backward rebuilds layer i's tape from boundary i with that same one-layer forward just
 *   before it reads it (the two top layers are still in their slots), so every output has the bits of the stored mode wherever the
 *   stored mode itself is reproducible.  Costs the forward of layers - 2 layers per backward; no allocation, synchronisation or host
 *   read, so the step stays capturable into a HIP graph.  Not combinable with TTV_TRAIN_FUSED_NORMS=1 (there a layer's first norm is
 *   written by the layer below, which a rebuilt layer cannot repeat): TTV_ERR_INVALID.
 * Any other mode: TTV_ERR_INVALID from the entry points, -1 from the size functions.  The backward workspace is the same in both modes. */
#define TTV_TAPE_STORED 0
#define TTV_TAPE_RECOMPUTE 1
int64_t ttv_tower_tape_bytes_ex(const ttv_tower_dims* dims, const ttv_batch* batch, int tape_mode);
int64_t ttv_tower_bwd_workspace_bytes_ex(const ttv_tower_dims* dims, const ttv_batch* batch, int tape_mode);
int ttv_encoder_forward_train_ex(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_batch* batch, const void* const* clips,
                                 float* z, void* tape, int64_t tape_bytes, void* stream, int tape_mode);
int ttv_encoder_backward_ex(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* batch,
                            const float* dz, void* tape, const ttv_tower_grads* grads, void* const* dclips, void* workspace,
                            int64_t workspace_bytes, void* stream, int tape_mode);
int ttv_decoder_forward_train_ex(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_batch* batch, const void* codes,
                                 void* const* clips_out, void* tape, int64_t tape_bytes, void* workspace, int64_t workspace_bytes,
                                 void* stream, int tape_mode);
int ttv_decoder_backward_ex(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* batch,
                            const void* codes, const void* const* dclips_out, void* tape, const ttv_tower_grads* grads, float* dcodes,
                            void* workspace, int64_t workspace_bytes, void* stream, int tape_mode);
/* TiTokEncoder.forward recording a tape; z fp32 [sum_tokens, token_size] (FSQ is a separate differentiable op). */
int ttv_encoder_forward_train(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_batch* batch, const void* const* clips,
                              float* z, void* tape, int64_t tape_bytes, void* stream);
/* Backward of the above: dz fp32 -> parameter gradients (accumulated) and, if dclips != NULL, gradients w.r.t. the input
 * clips (HOST array of device ptrs, compute dtype; needed by the discriminator path, loss_module.py:149-152).
 * grads == NULL (then dclips must be given): all parameters frozen - the generator step through the discriminator,
 * loss_module.py:144-151 - only the input gradient is computed, the weight-gradient GEMMs and gain / bias reductions are
 * skipped. */
int ttv_encoder_backward(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* batch,
                         const float* dz, void* tape, const ttv_tower_grads* grads, void* const* dclips, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* TiTokDecoder.forward recording a tape (workspace >= sum_patches * C*pt*ph*pw elements). */
int ttv_decoder_forward_train(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_batch* batch, const void* codes,
                              void* const* clips_out, void* tape, int64_t tape_bytes, void* workspace, int64_t workspace_bytes,
                              void* stream);
/* Backward: dclips_out (HOST array of device ptrs to d loss / d reconstruction, compute dtype) -> parameter gradients and
 * dcodes fp32 [sum_tokens, token_size] (may be NULL). */
int ttv_decoder_backward(const ttv_tower_dims* dims, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* batch,
                         const void* codes, const void* const* dclips_out, void* tape, const ttv_tower_grads* grads, float* dcodes,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* Straight-through FSQ backward (fsq.py:48-51,78-90): dz = dcodes * half_l/half_width * (1 - tanh^2(z + shift)). */
int ttv_fsq_backward(const ttv_fsq_params* p, const float* z, const void* dcodes, int dcodes_dtype, float* dz, int rows, void* stream);

/* The elementwise and small-projection ops of the training tape, one launch each (tests: the towers call the same launchers, so every
 * check below holds for them too).  T is `dtype` (TTV_BF16 or TTV_F32); arithmetic is fp32 with one rounding to T at the store.  rows == 0
 * (n == 0) is a no-op that accepts NULL pointers.  The 4-wide ops (gate, geglu, scale_cast, cast_to_f32) move whole 4-element vectors:
 * the width, every leading dimension (>= the width it spans) and every pointer must be a multiple of 4 elements, n a multiple of 4;
 * anything else is TTV_ERR_INVALID before any launch. */
/* ag[r, 0:width] = a * sigmoid(gate) (transformer.py:103; the gate sits inside a q|gate|k|v row).  ag may be a itself (same pointer and
 * leading dimension): every element is read and written exactly once. */
int ttv_gate_forward(const void* a, int lda, const void* gate, int ldg, void* ag, int ldo, int rows, int width, int dtype, void* stream);
/* da = dag * sigmoid(gate), dgate = dag * a * sigmoid(gate) * (1 - sigmoid(gate)).  delta (may be NULL; fp32 [rows, width / 64], needs
 * width % 64 == 0): the attention backward's delta[r, h] = sum over head h's 64 dims of da * a with da AS STORED (rounded to T), every
 * element written exactly once. */
int ttv_gate_backward(const void* dag, int lddag, const void* a, int lda, const void* gate, int ldg, void* da, int ldda, void* dgate,
                      int lddg, int rows, int width, int dtype, float* delta, void* stream);
/* h[r, 0:inner] = gelu_erf(u[r, inner:2 inner]) * u[r, 0:inner] (erff() for both dtypes). */
int ttv_geglu_forward(const void* u, int ldu, void* h, int ldh, int rows, int inner, int dtype, void* stream);
/* du[:, 0:inner] = dh * gelu(g), du[:, inner:2 inner] = dh * x * gelu'(g) with x | g = u.  fp32: erff() / expf().  bf16: the 8-wide
 * kernel with the fast Phi of the forward GEMM epilogue (|g Phi - gelu| <= 2.6e-5, |Phi + g phi - gelu'| <= 5.1e-5 for |g| <= 2^20) when
 * inner and all three leading dimensions are multiples of 8 and all three pointers 16-byte aligned, the 4-wide erff() kernel otherwise
 * (and always when TTV_GEGLU_BWD_ERF=1, read once per process). */
int ttv_geglu_backward(const void* u, int ldu, const void* dh, int lddh, void* du, int lddu, int rows, int inner, int dtype, void* stream);
/* b = alpha * a (fp32, NULL: skipped, may alias a) and c = (T) a (NULL: skipped) over n contiguous fp32 elements. */
int ttv_scale_cast(const float* a, float alpha, float* b, void* c, int dtype, int64_t n, void* stream);
/* b = (float) a, or b += (float) a when accumulate != 0, over n contiguous elements of T. */
int ttv_cast_to_f32(const void* a, int dtype, float* b, int64_t n, int accumulate, void* stream);
/* out[r, f] = sum_{c < C} a[r, c] * w[c, f] (w_cf = 1) or w[f, c] (w_cf = 0), f < width: the wide side of a width <-> token_size
 * projection, summed in fp32 in the order of c.  (a, w, out) dtypes: (f32, bf16, bf16), (f32, f32, f32) or (f32, bf16, f32); any other
 * triple is TTV_ERR_INVALID.  No alignment demands (scalar accesses). */
int ttv_expand_small(const void* a, int a_dtype, int lda, int C, const void* w, int w_dtype, int ldw, int w_cf, void* out, int out_dtype,
                     int ldo, int rows, int width, void* stream);
/* out[r, c] (fp32) = sum_{f < width} a[a_rows ? a_rows[r] : r][f] * w[f, c], c < C: one wave per row, 64 interleaved partial sums and a
 * 6-step wave sum.  (a, w) dtypes: (bf16, bf16), (f32, f32) or (f32, bf16); any other pair is TTV_ERR_INVALID. */
int ttv_reduce_small(const void* a, int a_dtype, int lda, const int32_t* a_rows, const void* w, int w_dtype, int ldw, int C, float* out,
                     int ldo, int rows, int width, void* stream);
/* Backward of the constant mask-token rows v[f] = m * rsqrt(m^2 + eps) * gain[f], m = (T) mask_token[0] straight through, given
 * colsum[f] = the sum of the incoming gradient over those rows (all fp32 [width] / [1]): dgain[f] += colsum[f] * m * rsqrt(m^2 + eps),
 * dmask[0] += sum_f colsum[f] * gain[f] * eps * (m^2 + eps)^-1.5.  dgain and dmask both NULL: a no-op; exactly one NULL:
 * TTV_ERR_INVALID (the kernel writes both; the towers always pass both or neither). */
int ttv_const_rows_backward(const float* colsum, const float* mask_token, const float* gain, int dtype, float eps, float* dgain,
                            float* dmask, int width, void* stream);

/* Optimizer step of the training loop (reference train.py:76-77 clip_gradients + :183-190 optim.AdamW; the arithmetic of
 * torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW, fp32 whatever the tensors' dtype) over a list of tensors, in two launches.
 * table  : device array of n entries {void* param; const void* grad; void* exp_avg; void* exp_avg_sq; int64 numel} (40 bytes each; param,
 *          exp_avg and exp_avg_sq of one dtype - TTV_F32 or TTV_BF16 - which is also the gradient's);
 * chunks : device int32 [n_chunks][2] = (entry index, first element): one block per chunk of up to 8192 elements.
 * ttv_opt_grad_sumsq writes partials[c] = sum of grad^2 over chunk c.  ttv_opt_adamw_step sums partials[0 .. n_partials) in a fixed order
 * (all chunks of ALL tensor lists of the step: the global gradient norm, written to out_norm when not NULL), scales the gradients by
 * min(1, max_norm / (norm + 1e-6)) in registers (NaN when the norm is NaN, as torch's clamp: every updated element becomes NaN;
 * max_norm <= 0 or n_partials == 0: no clipping; p.grad is NOT rewritten) and applies
 * AdamW with the given complements 1 - beta1, 1 - beta2 and bias corrections 1 - beta1^t, sqrt(1 - beta2^t): all four are formed in
 * double by the caller and rounded to float once (1.0f - (float)beta2 would be 1.3e-5 off at beta2 = 0.999). */
int ttv_opt_grad_sumsq(const void* table, const int32_t* chunks, int n_chunks, int dtype, float* partials, void* stream);
int ttv_opt_adamw_step(const void* table, const int32_t* chunks, int n_chunks, int dtype, const float* partials, int n_partials, float lr,
                       float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                       float bias_correction1, float bias_correction2_sqrt, float max_norm, float* out_norm, void* stream);

/* The same step with its scalar state on the device (optim.HipAdamW(capturable=True) / (skip_nonfinite=True)): the update count, both
 * bias corrections and the learning rate are formed by one tiny launch per parameter group and read by the update kernel from a
 * 48-byte block, so a captured step replays with the count it finds, a schedule costs the host nothing per step, and a step whose
 * gradient norm is not finite can be dropped without a host round trip.
 * ttv_opt_state   : one per parameter group, device memory, 8-byte aligned, zero before the first update (or filled by the caller
 *                   when training resumes).  `updates` counts the updates applied, `skipped` the calls dropped; the rest describes
 *                   the last ttv_opt_prepare: skip_now (1: the update kernels of this step return at once), the floats the update
 *                   uses and the schedule index they were formed at.
 * ttv_opt_schedule: passed by value.  TTV_OPT_SCHEDULE_NONE: lr = lr_constant.  TTV_OPT_SCHEDULE_COSINE: the reference's
 *                   get_cosine_schedule_with_warmup (train_utils/lr_schedulers.py:55-61) times LambdaLR's initial_lr, at
 *                   index = max(0, first + stride * updates): index < warmup_steps ? index / max(1, warmup_steps) :
 *                   (end_lr + (base_lr - end_lr) * max(0, 0.5 * (1 + cos(pi * num_cycles * 2 * progress)))) / base_lr with
 *                   progress = (index - warmup_steps) / max(1, training_steps - warmup_steps); every operation in double, in that
 *                   order, without contraction.
 * ttv_opt_prepare : one block.  Sums partials[0 .. n_partials) in the order ttv_opt_adamw_step does (the same bits), writes the norm
 *                   to out_norm (when not NULL and n_partials > 0) and forms the clip factor by the same rule (max_norm <= 0 or
 *                   n_partials == 0: 1).  With TTV_OPT_SKIP_NONFINITE in flags and a norm that is NaN or infinite: skip_now = 1,
 *                   skipped += 1; norm and clip_coef are written, updates and the other fields stay.  Otherwise skip_now = 0, t = updates + 1, bc1 = 1 - beta1^t,
 *                   bc2_sqrt = sqrt(1 - beta2^t) and lr in double, each rounded to float once, and updates = t.
 * ttv_opt_adamw_step_dev: ttv_opt_adamw_step's update of one tensor list with lr, bc1, bc2_sqrt and the clip factor read from
 *                   the block; with skip_now set no block reads or writes a tensor.
 * Both return TTV_ERR_INVALID and launch nothing for a NULL state (partials with n_partials > 0, table, chunks), an unknown
 * schedule kind, training_steps < warmup_steps, stride < 1, n_partials < 0 or an unknown dtype. */
typedef struct ttv_opt_state {
  int64_t updates;
  int64_t skipped;
  int64_t schedule_index;
  int32_t skip_now;
  float lr, bc1, bc2_sqrt, clip_coef, norm;
} ttv_opt_state;
#define TTV_OPT_SCHEDULE_NONE 0
#define TTV_OPT_SCHEDULE_COSINE 1
typedef struct ttv_opt_schedule {
  int32_t kind;
  int32_t reserved;
  int64_t warmup_steps, training_steps;
  double base_lr, end_lr, num_cycles, initial_lr;
  int64_t first, stride;
} ttv_opt_schedule;
#define TTV_OPT_SKIP_NONFINITE 1
int ttv_opt_prepare(ttv_opt_state* state, ttv_opt_schedule schedule, double beta1, double beta2, double lr_constant, float max_norm,
                    const float* partials, int n_partials, int flags, float* out_norm, void* stream);
int ttv_opt_adamw_step_dev(const void* table, const int32_t* chunks, int n_chunks, int dtype, const ttv_opt_state* state, float beta1,
                           float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay, void* stream);

/* Per-parameter gradient norms of one tensor list (the log of reference train.py:78-79, :102-103: lightning.pytorch.utilities.grad_norm
 * with norm_type 2) from the partials ttv_opt_grad_sumsq has written for the same table, in one launch.  `chunks` (device, n_chunks x
 * (entry, first element)) lists every entry's chunks together and the entries in ascending order, as ttv_opt_grad_sumsq's caller builds
 * it; partials[c] belongs to chunks[c].  norms[e] = sqrtf(sum of the partials of entry e, added in ascending chunk order, fp32), 0 for an
 * entry without chunks; norms[n_entries] = sqrtf(sum of partials[0 .. n_chunks), added in ascending order, fp32).  A fixed order and
 * no atomics: identical calls give identical bits.  `table` is the entry table of the other two calls (not read: the chunk table
 * names the entries).  Reads nothing but chunks and partials, writes nothing but norms[0 .. n_entries]. */
int ttv_opt_param_norms(const void* table, const int32_t* chunks, int n_chunks, int n_entries, const float* partials, float* norms,
                        void* stream);

/* Exponential moving average of a parameter list in fp32 shadow tensors (titok_video_amd/ema.py; not in the reference, which validates
 * its raw weights), on the table layout of the optimizer step: entries of 40 bytes, `chunks` = device int32 [n_chunks][2] = (entry index,
 * first element), one block per chunk of up to 8192 elements.  dtype (TTV_F32 or TTV_BF16) is the PARAMETERS' type; a shadow is float
 * whatever the dtype.  16-byte accesses when every pointer of an entry that the call touches is 16-byte aligned, element by element
 * otherwise.  n_chunks == 0: TTV_OK and no launch.
 * ttv_opt_ema_update  : entries {const void* param; unused (0); float* shadow; unused (0); int64 numel}.  Per element, in fp32 and in
 *          this order: d = (float)param - shadow ; shadow = shadow + weight * d.  weight = 1 - decay, formed in double by the caller and
 *          rounded to float once (1.0f - (float)0.9999 is 1.7e-8 off 1e-4: 1.7e-4 of the weight).  weight == 0: no launch, every shadow bit stays.  Reads the
 *          parameters, writes elements [0, numel) of the shadows and nothing else.
 * ttv_opt_ema_exchange: entries {void* param; unused (0); const float* shadow; void* backup (the parameter's type and size); int64 numel}.
 *          mode 0 (apply): backup = param (its bits), then param = shadow cast to dtype (bf16: round to nearest even, NaN stays NaN);
 *          mode 1 (restore): param = backup (its bits).  The shadows are only read. */
int ttv_opt_ema_update(const void* table, const int32_t* chunks, int n_chunks, int dtype, float weight, void* stream);
int ttv_opt_ema_exchange(const void* table, const int32_t* chunks, int n_chunks, int dtype, int mode, void* stream);

/* Single backward ops, exported for parity tests. */
/* dW[N,K] (fp32, accumulated) += dY[L,N]^T X[L,K]  (weight gradient of y = x w^T; what autograd computes for the
 * nn.Linear weights of base/blocks.py:70-84,147-148).  The token range is split over blocks; with a workspace of
 * ttv_linear_wgrad_workspace_bytes(L, N, K) bytes the split partial tiles are summed in a fixed order (bit-reproducible),
 * with workspace == NULL (workspace_bytes == 0) they are accumulated with fp32 atomics. */
int64_t ttv_linear_wgrad_workspace_bytes(int L, int N, int K);
int ttv_linear_wgrad(const void* dy, int lddy, const void* x, int ldx, float* dw, int lddw, int L, int N, int K, int dtype,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* Layer-boundary backward in one row-local pass (base/blocks.py:139-168: x1 = attn_post_ln(alpha*x + attn(pre_ln(x))), the
 * same shape around the feed-forward): A = dx + rmsnorm_bwd(x, gain1, dy) joins a sub-layer's pre-norm gradient with the
 * residual gradient; B = rmsnorm_bwd(y, gain2, A) takes it through the KEEL post-norm of the sub-layer below (y = that norm's
 * fp32 input; y == NULL: B = A).  dx (fp32, in/out) = out_scale * B; cast_out (dtype, may be NULL) = B.  dgain1 / dgain2 fp32
 * [width], accumulated, may be NULL. */
int ttv_rmsnorm_backward_chain(const void* x, int ldx, const void* dy, int lddy, const float* gain1, float* dgain1, float* dx, int lddx,
                               const float* y, int ldy, const float* gain2, float* dgain2, float out_scale, void* cast_out, int ldc, int rows,
                               int width, float eps, int dtype, void* stream);
/* RMSNorm backward: dx (dtype), dgain fp32 [width] (accumulated; may be NULL). */
int ttv_rmsnorm_backward(const void* x, int ldx, const void* dy, int lddy, const float* gain, void* dx, int lddx, float* dgain, int rows,
                         int width, float eps, int dtype, void* stream);
/* Deterministic siblings of the two above (see ttv_set_deterministic).  Partial layout: fp32 [blocks][width], blocks =
 * scratch_bytes / (4 * width) of ttv_rmsnorm_backward_det_scratch_bytes(rows, width); block b holds the sum over its rows of dy * xhat.
 * The chain takes two such arrays, gain 1's at the scratch's start and gain 2's right behind it (at half of
 * ttv_rmsnorm_backward_chain_det_scratch_bytes).  ttv_rmsnorm_backward_det also takes the row maps of the tower backward (int32
 * [rows] each, NULL = row r): row r reads x[x_rows[r]], dy[dy_rows[r]] and writes dx[dx_rows[r]]. */
int64_t ttv_rmsnorm_backward_det_scratch_bytes(int rows, int width);
int64_t ttv_rmsnorm_backward_chain_det_scratch_bytes(int rows, int width);
int ttv_rmsnorm_backward_chain_det(const void* x, int ldx, const void* dy, int lddy, const float* gain1, float* dgain1, float* dx, int lddx,
                                   const float* y, int ldy, const float* gain2, float* dgain2, float out_scale, void* cast_out, int ldc, int rows,
                                   int width, float eps, int dtype, void* scratch, int64_t scratch_bytes, void* stream);
int ttv_rmsnorm_backward_det(const void* x, int ldx, const void* dy, int lddy, const float* gain, void* dx, int lddx, float* dgain, int rows,
                             int width, float eps, int dtype, const int32_t* x_rows, const int32_t* dy_rows, const int32_t* dx_rows, void* scratch,
                             int64_t scratch_bytes, void* stream);
/* The tower backward's three small reductions on their own, for tests (either mode; the scratch is looked at with the deterministic
 * mode on only).  All accumulate into fp32 destinations.
 *   ttv_colsum_accumulate      out[c] += sum_r a[rows_map ? rows_map[r] : r][c], c < n (bias gradients).  Partials: fp32 [row blocks][n],
 *                              64 rows per block (the last one short): ttv_colsum_det_scratch_bytes(rows, n) = blocks * n * 4.
 *   ttv_sumall_accumulate      out[0] += scale * sum of a[rows, 0:n] (mask-token gradient).  Partials: fp32 [blocks], block b's sum already
 *                              scaled: ttv_sumall_det_scratch_bytes(rows, n) = blocks * 4.
 *   ttv_outer_small_accumulate dw[c][f] (transpose_out: dw[f][c]) += sum_r a[r][c] * b[r][f], c < C <= TTV_MAX_TOKEN, f < d (the
 *                              d <-> token_size projections).  Partials: fp32 [row blocks][cn][d], 32 rows per block, for one chunk of
 *                              cn <= TTV_MAX_FSQ columns c at a time (the chunks reuse the scratch; after the call it holds the last
 *                              chunk's): ttv_outer_small_det_scratch_bytes(rows, C, d) = blocks * min(C, TTV_MAX_FSQ) * d * 4. */
int64_t ttv_colsum_det_scratch_bytes(int rows, int n);
int64_t ttv_sumall_det_scratch_bytes(int rows, int n);
int64_t ttv_outer_small_det_scratch_bytes(int rows, int C, int d);
int ttv_colsum_accumulate(const void* a, int dtype, int lda, const int32_t* rows_map, int rows, int n, float* out, void* scratch,
                          int64_t scratch_bytes, void* stream);
int ttv_sumall_accumulate(const void* a, int dtype, int lda, int rows, int n, float scale, float* out, void* scratch, int64_t scratch_bytes,
                          void* stream);
int ttv_outer_small_accumulate(const void* a, int a_dtype, int lda, int C, const void* b, int b_dtype, int ldb, float* dw, int lddw,
                               int transpose_out, int rows, int d, void* scratch, int64_t scratch_bytes, void* stream);
/* Attention backward (flash-style recompute from the forward's LSE): qkvg as in ttv_attention, o / dout [L,d], lse fp32
 * [L,q_heads] -> dqkvg [L,2d+2g] (q, k, v column ranges written; gate range untouched).  delta: fp32 [L,q_heads] scratch;
 * dkv_scratch: fp32 [L,2g] scratch (fp32 dtype only). blocks64 / row_seq as in ttv_batch.  rope_cs (fp32 [L,64] cos|sin as in
 * ttv_batch, may be NULL): when given, dq and dk are returned as gradients w.r.t. the q / k BEFORE the rotary embedding
 * (rope.py:19-27), i.e. the transposed rotation is applied in fp32 before the store. */
int ttv_attention_backward(const void* qkvg, int ld, const void* o, int ldo, const void* dout, int ldd, const float* lse, float* delta,
                           const int32_t* cu_seqlens, const int32_t* blocks64, int n_blocks64, const int32_t* row_seq, void* dqkvg,
                           int ldg, float* dkv_scratch, int total_rows, int q_heads, int kv_heads, int dtype, const float* rope_cs,
                           void* stream);
/* ttv_attention_backward with the towers' rule for query rows the forward did not compute (the encoder's last layer, whose attention
 * runs for the latent query rows only), for tests.  clip_desc: int32 [n_seqs][8] as in ttv_batch (entries 3 - 5 of a clip: its patch
 * grid gt, gh, gw; the latent tokens are the K = S - gt * gh * gw rows in front of the patches); NULL = every row.  Of a sequence
 * only the query rows [0, min(S, ceil(K / 128) * 128)) take part: the rows behind get dq = 0 and add nothing to dk / dv (their lse
 * and dout are not read). */
int ttv_attention_backward_qlim(const void* qkvg, int ld, const void* o, int ldo, const void* dout, int ldd, const float* lse, float* delta,
                                const int32_t* cu_seqlens, const int32_t* blocks64, int n_blocks64, const int32_t* row_seq, void* dqkvg,
                                int ldg, float* dkv_scratch, int total_rows, int q_heads, int kv_heads, int dtype, const float* rope_cs,
                                const int32_t* clip_desc, void* stream);
/* ttv_attention with an extra fp32 [L,q_heads] log-sum-exp output (training forward). */
int ttv_attention_lse(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* qblocks, int n_qblocks,
                      int q_heads, int kv_heads, int head_dim, int flags, int dtype, float* lse, void* stream);

/* ---- codebook statistics (train_utils/codebook_logging.py:19-32) -------------------------------------- */
/* counts[idx] += 1 for every index (int64 device histogram, atomics); usage/entropy are finished on the host. */
int ttv_codebook_histogram(const int32_t* indices, int n, int64_t* counts, int codebook_size, void* stream);

/* L1 reconstruction term of the generator loss (loss_module.py:118 per clip, mean over clips - train.py:70), value and
 * gradient in one launch: *loss += mean_c mean_i |recon_c[i] - target_c[i]| (caller zeroes it);
 * grad_c[i] = sign(recon - target) / (sizes[c] * n_clips) in `dtype` (grad NULL = value only).  Host arrays of device pointers. */
int ttv_l1_loss(void* const* recon, void* const* target, void* const* grad, const int32_t* sizes, int n_clips, int dtype, float* loss,
                void* stream);
/* Deterministic sibling (see ttv_set_deterministic).  Partial layout: fp32 [clip][block], blocks per clip = scratch bytes / (4 * n_clips)
 * for n_clips <= TTV_MAX_CLIPS_PER_LAUNCH; a partial is the block's sum of |recon - target| times 1 / (sizes[clip] * n_clips).  More
 * clips run in groups of TTV_MAX_CLIPS_PER_LAUNCH that reuse the scratch (the size is the largest group's). */
int64_t ttv_l1_loss_det_scratch_bytes(const int32_t* sizes, int n_clips);
int ttv_l1_loss_det(void* const* recon, void* const* target, void* const* grad, const int32_t* sizes, int n_clips, int dtype, float* loss,
                    void* scratch, int64_t scratch_bytes, void* stream);

/* The loader's tail on the device (dataset/video_dataset.py:116-119: ToDtype(scale=True) + Normalize(0.5, 0.5) on channel-first
 * frames): decoded frames uint8 [T,H,W,3] (device memory, what the decoder / a shard hands over) -> clip [3,T,H,W] in `dtype`,
 * value u8 / 127.5 - 1 evaluated in fp32 and rounded once.  T*H*W % 4 == 0 (patch-aligned clips always are). */
int ttv_clip_from_u8(const void* frames_thwc, int T, int H, int W, void* clip_cthw, int dtype, void* stream);

/* The loader's front on the device (dataset/video_dataset.py:96-119: v2.RandomResizedCrop / v2.Resize + CenterCrop with BICUBIC and
 * antialias=True, RandomHorizontalFlip, then the tail above), up to TTV_MAX_CLIPS_PER_LAUNCH clips in ONE launch.  Host arrays:
 * frames_thwc[i] uint8 [T][Hs][Ws][3] (device, contiguous, any alignment; the whole array is the resampling domain - a crop is made
 * by handing over the crop box only), clips_cthw[i] [3][T][Ho][Wo] in `dtype` (device, 16-byte aligned), geom = n_clips x
 * (T, Hs, Ws, Hr, Wr, oy, ox, Ho, Wo, flip): the frame is resampled to the virtual size Hr x Wr, of which the window of Ho x Wo at
 * (oy, ox) is produced (oy + Ho <= Hr, ox + Wo <= Wr), mirrored along W when flip = 1.
 * Value, per channel and frame (aten's _upsample_bicubic2d_aa, the float path of torchvision's resize): along an axis n_in -> n_out,
 * scale = n_in / n_out, support = 2 scale if scale >= 1 else 2, inv = 1 / scale if scale >= 1 else 1; output i has the centre
 * c = scale (i + 0.5) and the taps lo = max(0, int(c - support + 0.5)) <= j < hi = min(int(c + support + 0.5), n_in) with weights
 * cubic((j - c + 0.5) inv) (Keys, a = -0.5) divided by their sum.  Width pass, then height pass, fp32, no rounding in between;
 * level = clamp(round_half_even(v), 0, 255); stored value level / 127.5 - 1 as ttv_clip_from_u8 forms it, rounded once to `dtype`.
 * (aten's native uint8 kernel, which torchvision picks for uint8 input on an AVX2 host, rounds and clamps between the passes and
 * uses fixed-point weights; this is the float path.)  A scale above 8 on an axis, a window outside the resized frame, a
 * misaligned destination, more clips than the limit or a bad dtype return TTV_ERR_INVALID and launch nothing. */
int ttv_clip_resample_u8(void* const* frames_thwc, void* const* clips_cthw, const int32_t* geom, int n_clips, int dtype, void* stream);

/* The logged side-by-side videos of the validation step (reference train.py:141-142:
 * torch.cat((y, x.clamp(-1, 1)), dim=-1).permute(1, 0, 2, 3).cpu().float().numpy(), then ((v + 1) / 2 * 255).astype(np.uint8)), for any
 * number of clips (host arrays of device pointers; launches of up to TTV_MAX_CLIPS_PER_LAUNCH clips inside).  target[i] (y) and recon[i]
 * (x): contiguous [3][T][H][W] in `dtype` (TTV_BF16 or TTV_F32), dims = n_clips x (T, H, W) (host); panels[i]: uint8 [T][3][H][2W],
 * columns 0 .. W-1 from the target, columns W .. 2W-1 from the reconstruction clamped to [-1, 1] (a NaN stays a NaN).
 * Value of a byte, from its element v widened exactly to fp32: t = v + 1.0f; t = t / 2.0f; t = t * 255.0f, each step rounded to fp32 on
 * its own (no fused multiply-add, no folding into * 127.5f), then truncated toward zero: numpy's fp32 arithmetic, so every byte is
 * defined bit for bit.  Where numpy leaves the conversion to the platform this defines it: t < 0 gives 0, t >= 255 gives 255 (a
 * target outside [-1, 1] saturates) and NaN gives 0.
 * Any T, H, W >= 1 with a panel below 2^31 bytes, any alignment of the panels; clips with W % 8 == 0, 16-byte aligned sources and an
 * 8-byte aligned panel move 16 bytes per load and 8 per store, the others 4 bytes per store.  Every input element is read once and
 * every output byte written once; nothing outside the panels is written.  TTV_ERR_INVALID with nothing launched: a bad dtype or
 * shape, a null pointer, a source not aligned to its element size.  Work is enqueued on `stream` only. */
int ttv_recon_panels_u8(void* const* target, void* const* recon, const int32_t* dims, int n_clips, int dtype, void* const* panels,
                        void* stream);

/* ---- whole videos: overlapped 3-D tiles in, blended uint8 frames out (titok_video_amd/video.py) -----------------------------
 * A decoded video uint8 [T][H][W][3] is cut into equal tiles that overlap, each tile goes through the tokenizer on its own, and the
 * reconstructions are blended back into frames.  The plan is the same for both directions.
 * Timeline: output frame j is source frame frame_stride * j, j = 0 .. T' - 1, T' = ceil(T / frame_stride); axes below are (T', H, W).
 * Per axis a (length n, tile[a], overlap[a], count[a]): stride = tile - overlap; tile k of the axis starts at k * stride for
 * k < count - 1 and the last one at max(n - tile, 0), so it ends at the border.  count is 1 when n < tile (the tile is then longer
 * than the axis: samples beyond n - 1 are edge-clamped on the way in and dropped on the way out) and ceil((n - tile) / stride) + 1
 * otherwise; a point may lie in up to three tiles of an axis.  Tile index = (kt * count[1] + kh) * count[2] + kw.
 * Weight of a tile at local coordinate u of an axis: the integer min(u + 1, tile - u, overlap + 1); at an element the product of
 * the three.  TTV_ERR_INVALID for a plan with T, H, W, frame_stride or a tile below 1, overlap < 0, overlap > tile / 2 on an axis
 * with more than one tile, a count that is not the rule's (it would put an origin outside the timeline),
 * (overlap[0] + 1)(overlap[1] + 1)(overlap[2] + 1) >= 2^24, a tile of 2^31 elements or more, or 2^31 tiles or more. */
typedef struct ttv_video_plan {
  int32_t T, H, W;          /* the decoded video */
  int32_t frame_stride;
  int32_t tile[3];          /* (Tt, Ht, Wt), the effective tile: a multiple of the patch, never more than one patch beyond a short axis */
  int32_t overlap[3];
  int32_t count[3];         /* tiles per axis */
} ttv_video_plan;

/* Gather: tiles [tile_begin, tile_end) of the plan -> `tiles`, one contiguous buffer [tile_end - tile_begin][3][Tt][Ht][Wt] in `dtype`
 * (TTV_BF16 or TTV_F32), 16-byte aligned.  Element (c, i, y, x) of the tile with origin (t0, h0, w0) is
 *   frames[frame_stride * min(t0 + i, T' - 1)][min(h0 + y, H - 1)][min(w0 + x, W - 1)][c] / 127.5 - 1
 * evaluated in fp32 (one division, one subtraction) and rounded once to `dtype`: ttv_clip_from_u8's expression, so the bits are those
 * ttv_clip_from_u8 gives for the same pixels.  Any H, W >= 1 and any alignment of `frames_thwc`: with Wt % 8 == 0 a thread takes 8
 * pixels of a tile row with 4-byte loads of the aligned words that hold their 24 bytes and writes three 16-byte (bf16) or six
 * 16-byte (fp32) vectors; at the ends of the video (words that leave the array, clamped columns) and for other Wt it goes byte by byte.
 * Every source byte inside a tile is read once per tile that covers it (the aligned words of neighbouring threads share bytes, which
 * the cache serves).  TTV_ERR_INVALID with nothing launched: a bad dtype, a null pointer, a destination off the 16-byte grid, a tile
 * range outside [0, tiles of the plan], a bad plan.  An empty range does nothing.  Work is enqueued on `stream` only. */
int ttv_video_tiles_u8(const void* frames_thwc, const ttv_video_plan* plan, int tile_begin, int tile_end, void* tiles, int dtype,
                       void* stream);

/* Blend: frames [t0, t1) of the timeline -> frames_out uint8 [t1 - t0][H][W][3] from reconstructed tiles [3][Tt][Ht][Wt] in `dtype`.
 * tiles: HOST array of the plan's tile count of device pointers in tile order (what the checks read); tiles_dev: the same table in
 * device memory (what the kernel reads).  A tile that covers no frame of the range may be NULL.
 * Value of byte (t, y, x, c), from the tiles that cover (t, y, x) in ascending tile index:
 *   v = the tile's element (c, t - t0_tile, y - h0, x - w0) widened exactly to fp32 and clamped to [-1, 1] (a NaN stays a NaN);
 *   one covering tile: q = v.  More: num = 0.0f, then num = num + (w * v) per tile with the product and the sum each rounded to fp32
 *   on their own (no fused multiply-add), w the tile's integer weight at the element; den = the integer sum of the weights,
 *   converted to fp32 once; q = num / den, correctly rounded;
 *   t = q + 1.0f; t = t * 127.5f, each rounded on its own; level = round-half-even(t), with t < 0 -> 0, t >= 255 -> 255, NaN -> 0.
 * A gather per output element, no atomics: identical calls give identical bits.  Any H, W >= 1 and any alignment of frames_out; a
 * thread owns 4 consecutive pixels of a row, reads each tile that holds them once (one 8- or 16-byte vector per channel where the
 * four lie in the tile on a vector boundary, single elements otherwise) and stores their 12 bytes as three words where they lie on
 * the 4-byte grid, byte by byte otherwise and at the end of a row.  Every byte of the range is written once and nothing outside it.
 * TTV_ERR_INVALID with nothing launched: a bad dtype or plan, a null table or output, t0 < 0, t1 > T', t0 > t1, a covering tile whose
 * pointer is NULL or not aligned to its element size.  An empty range does nothing.  Work is enqueued on `stream` only. */
int ttv_video_blend_u8(void* const* tiles, void* const* tiles_dev, const ttv_video_plan* plan, int t0, int t1, int dtype,
                       void* frames_out, void* stream);

/* Measured distortion: per tile of [tile_begin, tile_end) the sum of squared level differences between a reconstruction of the tile
 * and the source pixels it was cut from (video.py: tile_sse, the rate table of VideoTokenizer.rate_distortion).
 * recon: HOST array of tile_end - tile_begin device pointers (what the checks read), recon_dev: the same table in device memory
 * (what the kernel reads), the blend's convention; entry j is tile tile_begin + j, [3][Tt][Ht][Wt] in `dtype` (TTV_BF16 or TTV_F32).
 * sse: device memory, uint64 [tile_end - tile_begin], 8-byte aligned.  For tile j of the range with origin (t0, h0, w0):
 *   sse[j] = sum over c < 3, i < min(Tt, T' - t0), y < min(Ht, H - h0), x < min(Wt, W - w0) of
 *            (level(recon_j[c][i][y][x]) - frames[frame_stride * (t0 + i)][h0 + y][w0 + x][c])^2
 *   level(v): the blend's rule for a pixel that one tile covers: v widened exactly to fp32 and clamped to [-1, 1] (a NaN stays a NaN);
 *   t = v + 1.0f; t = t * 127.5f, each rounded on its own; round-half-even(t), with t < 0 -> 0, t >= 255 -> 255, NaN -> 0.
 * Samples a tile holds beyond a short axis (the edge-clamped ones, which the blend drops) are not counted.  sse[j] is written, not
 * accumulated: the entry point clears the sums on `stream` and the blocks of a tile add their partial sums (each below 2^32) with
 * one 64-bit atomic per block.  An exact integer, so the same bits in any order of summation, with or without the deterministic mode.
 * Any H, W >= 1 and any alignment of `frames_thwc`.  With Wt % 8 == 0 a thread takes 8 pixels of a tile row (the gather's geometry
 * and its source load: aligned words, byte by byte at the array's ends and on clamped columns) and reads one 16-byte (bf16) or two
 * 16-byte (fp32) vectors per channel plane from a tile on the 16-byte grid, single elements from any other; for other Wt a thread
 * takes one pixel.  Nothing but sse[0 .. tile_end - tile_begin) is written.  TTV_ERR_INVALID with nothing launched and nothing
 * written: a bad dtype or plan, a null frames_thwc, table (either) or sse, a tile range outside [0, tiles of the plan], a tile pointer
 * of the range that is NULL or not aligned to its element size, sse off the 8-byte grid.  An empty range does nothing.  Work is
 * enqueued on `stream` only. */
int ttv_video_tile_sse_u8(const void* frames_thwc, const ttv_video_plan* plan, int tile_begin, int tile_end, void* const* recon,
                          void* const* recon_dev, int dtype, uint64_t* sse, void* stream);

/* ---- whole videos: Y'CbCr 4:2:0 frames in and out (I420, NV12, NV21; video.py: YUV420Frames) -------------------------------------
 * The three entry points above with 8-bit 4:2:0 planes in place of packed RGB: what video decoders hand out and encoders take.  A frame
 * of H x W has a luma plane of H x W and chroma planes of Hc x Wc, Hc = ceil(H / 2), Wc = ceil(W / 2).  Any H, W >= 1, any pointer
 * alignment, any pitch at or above the minimum.  TTV_ERR_INVALID, nothing launched and nothing written: a null description or plane,
 * c_step not 1 or 2, an enum out of range, y_pitch < W, c_pitch < c_step * Wc, y_frame < (H - 1) * y_pitch + W,
 * c_frame < (Hc - 1) * c_pitch + c_step * (Wc - 1) + 1 (a frame's samples end before the next frame's begin).
 *
 * Everything is integer arithmetic up to the last two fp32 operations.  Every integer coefficient is round-half-up of the real value.
 * (Kr, Kb) = (0.299, 0.114) for BT.601 and (0.2126, 0.0722) for BT.709, Kg = 1 - Kr - Kb; limited range: sy = 255/219, sc = 255/224,
 * ys = 219/255, cs = 224/255, y0 = 16; full range: all four scales 1, y0 = 0.
 *   to RGB, at 2^-12:    ky = sy 4096; rv = 2 (1 - Kr) sc 4096; bu = 2 (1 - Kb) sc 4096;
 *                        gu = -round(2 (1 - Kb) Kb / Kg sc 4096); gv = -round(2 (1 - Kr) Kr / Kg sc 4096)
 *   from RGB, at 2^-16:  ytot = ys 65536; yr = Kr ys 65536; yb = Kb ys 65536; yg = ytot - yr - yb;
 *                        ub = vr = cs 32768; ur = -round(Kr / (2 (1 - Kb)) cs 65536); ug = -(ur + ub);
 *                        vb = -round(Kb / (2 (1 - Kr)) cs 65536); vg = -(vr + vb)      (so every grey has chroma exactly 128)
 * Chroma at a luma position (y, x): row y reads chroma rows j - 1 and j with weights 1 and 3 when y is even, j and j + 1 with weights
 * 3 and 1 when y is odd, j = y >> 1.  Column x under TTV_YUV_CENTER follows the same rule; under TTV_YUV_LEFT an even x reads column
 * x >> 1 with weight 4, an odd x columns x >> 1 and (x >> 1) + 1 with weights 2 and 2.  Indices are clamped to the plane.
 * C16 = sum of row weight * column weight * sample (the weights sum to 16: 0 <= C16 <= 4080).
 * Source pixel: Yc = 16 ky (Y - y0), u = U16 - 2048, v = V16 - 2048; N_R = Yc + rv v, N_G = Yc + gu u + gv v, N_B = Yc + bu u, each
 * clamped to [0, 255 * 65536] (below 2^24: exact in fp32; the intermediates fit int32).  Source level of channel c: (N_c + 32768) >> 16. */
enum { TTV_YUV_BT601 = 0, TTV_YUV_BT709 = 1 };
enum { TTV_YUV_LIMITED = 0, TTV_YUV_FULL = 1 };
enum { TTV_YUV_LEFT = 0, TTV_YUV_CENTER = 1 };
typedef struct ttv_yuv420 {
  void* y; void* u; void* v;       /* first byte of each plane's first sample; NV12: v = u + 1, NV21: u = v + 1 */
  int64_t y_frame, c_frame;        /* bytes between frames of the luma / chroma planes */
  int32_t y_pitch, c_pitch;        /* bytes between rows; y_pitch >= W, c_pitch >= c_step * Wc */
  int32_t c_step;                  /* bytes between chroma samples of a row: 1 planar, 2 interleaved */
  int32_t matrix;                  /* TTV_YUV_BT601 | TTV_YUV_BT709 */
  int32_t range;                   /* TTV_YUV_LIMITED | TTV_YUV_FULL */
  int32_t siting;                  /* TTV_YUV_LEFT (horizontally co-sited, H.264/HEVC default) | TTV_YUV_CENTER */
} ttv_yuv420;

/* Gather: ttv_video_tiles_u8 with `frames` (plan->T frames of plan->H x plan->W) in place of frames_thwc: the same plan, tile order,
 * edge clamping on all three axes, frame stride, destination [n][3][Tt][Ht][Wt], dtypes and refusals.  Element (c, i, y, x) of the tile
 * with origin (t0, h0, w0) is
 *   float(N_c) / 8355840.0f - 1.0f      (one correctly rounded division, one subtraction, rounded once to `dtype`)
 * with N of the pixel (frame_stride * min(t0 + i, T' - 1), min(h0 + y, H - 1), min(w0 + x, W - 1)): the coordinates are clamped
 * before the chroma rule is applied, so a clamped column repeats the edge pixel's value.  N is not rounded to 8 bits first.
 * The description is checked even for an empty tile range. */
int ttv_video_tiles_yuv420(const ttv_yuv420* frames, const ttv_video_plan* plan, int tile_begin, int tile_end, void* tiles, int dtype,
                           void* stream);

/* Blend: frames [t0, t1) of the timeline into the planes of `frames_out`, whose plane pointers address frame t0.  Per pixel the RGB
 * levels L_R, L_G, L_B are exactly the bytes ttv_video_blend_u8 defines (the same clamp, weighted mean in ascending tile index,
 * rounding).  Y = y0 + ((yr L_R + yg L_G + yb L_B + 32768) >> 16).  Chroma sample (j, i): S_c = the sum of L_c over rows 2j, 2j + 1
 * and, under TTV_YUV_CENTER, columns 2i, 2i + 1 (D = 4); under TTV_YUV_LEFT columns 2i - 1, 2i, 2i + 1 with weights 1, 2, 1 (D = 8);
 * rows and columns clamped to the picture.  U = 128 + floor((ur S_R + ug S_G + ub S_B + D 32768) / (D 65536)), V likewise with
 * vr, vg, vb.  Limited range clamps Y to [16, 235] and U, V to [16, 240]; full range clamps all to [0, 255].
 * One launch, no RGB frame in memory, no atomics: identical calls give identical bits.  Every plane byte of the range inside the
 * picture is written once; pitch padding and everything else is left alone.  The tables and the refusals are ttv_video_blend_u8's. */
int ttv_video_blend_yuv420(void* const* tiles, void* const* tiles_dev, const ttv_video_plan* plan, int t0, int t1, int dtype,
                           const ttv_yuv420* frames_out, void* stream);

/* Measured distortion: ttv_video_tile_sse_u8 with the source level (N_c + 32768) >> 16 of pixel (frame_stride * (t0 + i), h0 + y,
 * w0 + x) in place of the source byte; level(recon), the samples that count, the exact 64-bit integer (written, not accumulated, the
 * same bits in every order of summation) and the refusals are as there. */
int ttv_video_tile_sse_yuv420(const ttv_yuv420* frames, const ttv_video_plan* plan, int tile_begin, int tile_end, void* const* recon,
                              void* const* recon_dev, int dtype, uint64_t* sse, void* stream);

/* ---- whole videos: per-frame quality of what comes back (video.py: frame_sse, frame_ssim, VideoQuality) ---------------------------------
 * `a` holds the n pictures under test, frame j at index j; `b` is the yardstick: frame j of `a` is compared with frame j * b_stride of
 * `b`, b_stride >= 1.  Both pointers (plane descriptions) address the first compared frame, and the caller guarantees that `b` holds
 * (n - 1) * b_stride + 1 frames.
 *   RGB:   a_thwc, b_thwc uint8 [.][H][W][3], any alignment.  Components 0, 1, 2 = R, G, B, each of H x W samples.
 *   4:2:0: two ttv_yuv420; layouts, pitches and frame strides may differ between `a` and `b`.  Components 0, 1, 2 = Y (H x W), U, V
 *          (Hc x Wc, Hc = ceil(H / 2), Wc = ceil(W / 2)); the planes are compared sample by sample.  matrix, range and siting are not
 *          read (video.py refuses a mismatch).
 * Pitch padding and the bytes between the samples of an interleaved chroma plane never count.
 * TTV_ERR_INVALID with nothing launched and nothing written, for all four entry points: a null pointer or description, n < 0,
 * b_stride < 1, H or W below the minimum, a ttv_yuv420 that fails the checks above for the frames its side holds (a null plane, c_step,
 * pitches, frame strides), an output off the 8-byte grid, a workspace that is too small or off the 8-byte grid.  n == 0 passes the
 * same checks and does nothing.  Work is enqueued on `stream` only.
 *
 * Squared error.  sse: device memory, uint64 [n][3], 8-byte aligned.
 *   sse[j][c] = sum over the samples (y, x) of component c of (a_j[c][y][x] - b_{j * b_stride}[c][y][x])^2
 * written, not accumulated: the entry point clears the sums on `stream`, a block's partial sum stays below 2^32 and is added with one
 * 64-bit atomic per block and component.  An exact integer, so the same bits in any order of summation, with or without the
 * deterministic mode.  Any H, W >= 1.  RGB: a thread takes 12 bytes (4 pixels) of a frame from the 4 aligned words that hold them on
 * each side; 4:2:0: 8 samples of a plane row from 3 aligned words (5 for interleaved chroma).  The ends of the arrays (words that
 * would leave them), the last, shorter group of a frame or a row go byte by byte; rows off the word grid are shifted into place.
 * Nothing but sse[0 .. n)[0 .. 3) is written. */
int ttv_video_frame_sse_u8(const void* a_thwc, const void* b_thwc, int n, int b_stride, int H, int W, uint64_t* sse, void* stream);
int ttv_video_frame_sse_yuv420(const ttv_yuv420* a, const ttv_yuv420* b, int n, int b_stride, int H, int W, uint64_t* sse, void* stream);

/* SSIM.  ssim: device memory, double [n][3], 8-byte aligned, written.  For component c of h x w samples,
 *   ssim[j][c] = mean over the (h - 10)(w - 10) windows wholly inside the plane of
 *                ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2))
 * on the levels 0 .. 255: C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; window = the 11-tap Gaussian, sigma 1.5, normalised to sum 1, in
 * both directions; mx, my the windowed means of a and b, sx^2 = max(E[x^2] - mx^2, 0), sy^2 likewise, sxy = E[xy] - mx my.  This is
 * torchmetrics' StructuralSimilarityIndexMeasure(data_range=255) per plane, restricted to the windows its reflect-pad and crop keeps
 * (the rule of ttv_ssim_accumulate below).  Every compared plane needs h, w >= 11: H, W >= 11 for RGB, H, W >= 21 for 4:2:0.
 * fp32 arithmetic after subtracting one sample of the block's tile from each plane (exact for integer levels; E[x^2] - mx^2 then
 * cancels on the local spread, not on the value).  One double per 32 x 32 tile of a plane's valid region goes into the caller-owned
 * workspace (ttv_video_frame_ssim_workspace_bytes(n, H, W, yuv420) bytes - yuv420 != 0 for the 4:2:0 entry point -, 8-byte aligned;
 * -1 with the error set for n < 0 or H, W below the minimum), and a second launch adds each plane's tiles in tile order: no
 * floating-point atomics, identical calls give identical bits. */
int64_t ttv_video_frame_ssim_workspace_bytes(int n, int H, int W, int yuv420);
int ttv_video_frame_ssim_u8(const void* a_thwc, const void* b_thwc, int n, int b_stride, int H, int W, double* ssim, void* workspace,
                            int64_t workspace_bytes, void* stream);
int ttv_video_frame_ssim_yuv420(const ttv_yuv420* a, const ttv_yuv420* b, int n, int b_stride, int H, int W, double* ssim, void* workspace,
                                int64_t workspace_bytes, void* stream);

/* PSNR statistic of the evaluation loop (model/metrics/eval_metrics.py:19,32-36: x.clamp(-1, 1), torchmetrics
 * PeakSignalNoiseRatio(data_range=2) = running sum of squared errors + element count): acc[0] += sum (clamp(recon) - target)^2,
 * acc[1] += number of elements, both double, device memory, over the clips of the call (host arrays of device pointers, `dtype`).
 * PSNR = 10 log10(4 * acc[1] / acc[0]) is finished on the host (one read when the score is wanted, none per step). */
int ttv_sq_err_accumulate(void* const* recon, void* const* target, const int32_t* sizes, int n_clips, int dtype, int clamp, double* acc,
                          void* stream);
/* Deterministic sibling (see ttv_set_deterministic).  Partial layout: double [clip][block][2] = (the block's sum of squared errors,
 * formed in fp32 as with the mode off; the clip's element count in its block 0 and zero in its other blocks), blocks per clip =
 * scratch bytes / (16 * n_clips) for n_clips <= TTV_MAX_CLIPS_PER_LAUNCH; groups as for ttv_l1_loss_det. */
int64_t ttv_sq_err_accumulate_det_scratch_bytes(const int32_t* sizes, int n_clips);
int ttv_sq_err_accumulate_det(void* const* recon, void* const* target, const int32_t* sizes, int n_clips, int dtype, int clamp, double* acc,
                              void* scratch, int64_t scratch_bytes, void* stream);

/* SSIM statistic of the evaluation loop (model/metrics/eval_metrics.py:20-21,32-37: x.clamp(-1, 1), CTHW -> TCHW, torchmetrics
 * StructuralSimilarityIndexMeasure(data_range=2) = running sum of per-frame SSIM + frame count): for up to
 * TTV_MAX_CLIPS_PER_LAUNCH contiguous clip pairs [C,T,H,W] (host arrays of device pointers, `dtype`; dims = n_clips x (C,T,H,W),
 * host), acc[0] += sum over frames of mean_{C x (H-10) x (W-10)} ssim (the windows wholly inside the frame, which is what the
 * reference's reflect-pad + crop keeps), acc[1] += number of frames, both double, device memory.  `clamp` clamps the
 * reconstruction only.  fp32 arithmetic for both dtypes; H and W must be >= 11.  The workspace (ttv_ssim_workspace_bytes(dims,
 * n_clips) bytes, 8-byte aligned, caller-owned) holds the per-tile partial sums, reduced by a second launch in a fixed order:
 * identical inputs give identical bits.  SSIM = acc[0] / acc[1] is finished on the host. */
int64_t ttv_ssim_workspace_bytes(const int32_t* dims, int n_clips);
int ttv_ssim_accumulate(void* const* recon, void* const* target, const int32_t* dims, int n_clips, int dtype, int clamp, double* acc,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---- LPIPS / Gram perceptual terms (model/metrics/lpips_gram.py LPIPS.forward, model/losses/loss_module.py:121-138) ----------
 * VGG16 features[0:30] (13 3x3 convolutions with bias + ReLU, 4 2x2 max-pools) on n reconstruction and n target crops, the LPIPS
 * head on the taps relu1_2 .. relu5_3 (lin weights applied with eval semantics: no dropout) and the optional Gram term; the
 * input-gradient backward into the reconstruction crops.  Weights are frozen (no weight gradients).  Activations NHWC in the
 * compute dtype (TTV_BF16: MFMA implicit GEMM with fp32 accumulation; TTV_F32: exact fp32); head, Gram and losses in fp32.
 *
 * Weight images (built once per weight version by the caller from W[co][ci][kh][kw], tap t = 3 kh + kw), compute dtype:
 *   direct image  [9][Cin][Cout]            = W[co][ci][kh][kw]
 *   dgrad direct  [9][Cout][Cin]            = W[co][ci][2-kh][2-kw]
 *   MFMA image    [Cin/32][9][Cout][32]     (the direct image with Cin split into 32-channel chunks, innermost)
 *   dgrad MFMA    [Cout/32][9][Cin][32]
 * A convolution takes the MFMA images when dtype == TTV_BF16, Cin % 32 == 0 and Cout % 64 == 0, the direct images otherwise (so
 * every fp32 layer, and conv1_1 plus its dgrad in bf16).  b[l]: fp32 bias [Cout]; lin[k]: fp32 [C_k] (lin{k}.model.1.weight). */
typedef struct {
  const void* w[13];     /* forward image of conv layer l (features index 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28) */
  const void* wd[13];    /* dgrad image of conv layer l */
  const float* b[13];
  const float* lin[5];
} ttv_lpips_weights;

/* Sizes for n image pairs of H x W (multiples of 16, 16 .. 2048), -1 on a bad shape or dtype.  The tape holds every activation of
 * the 2n-image stack (reconstruction images first); the workspace holds partial sums, head gradients and dgrad buffers. */
int64_t ttv_lpips_tape_bytes(int n, int H, int W, int dtype);
int64_t ttv_lpips_workspace_bytes(int n, int H, int W, int dtype);

/* recon, target: [n][3][H][W] (dtype, contiguous).  lpips[n] (fp32, device) = per-image LPIPS (sum over taps of the spatial mean of
 * sum_c lin_c (n0 - n1)^2); gram[n] (fp32, device, or NULL to skip the Gram term) = mean over taps of mse(G0, G1), G = F F^T / hw on
 * the un-normalised features.  tape and workspace: caller-owned, 256-byte aligned; the tape is kept for ttv_lpips_backward.
 * Partial sums are reduced in a fixed order: identical inputs give identical bits. */
int ttv_lpips_forward(const ttv_lpips_weights* w, const void* recon, const void* target, int n, int H, int W, int dtype, float* lpips,
                      float* gram, void* tape, void* workspace, int64_t workspace_bytes, void* stream);

/* d recon [n][3][H][W] (dtype) from the upstream gradients glpips[n] and ggram[n] (fp32, device; ggram NULL = Gram term off), using
 * the tape of the forward call with the same n, H, W, dtype and weights.  Max-pool gradients go to the first maximum of each window
 * in row-major order (torch max_pool2d). */
int ttv_lpips_backward(const ttv_lpips_weights* w, const void* tape, int n, int H, int W, int dtype, const float* glpips,
                       const float* ggram, void* drecon, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-frame LPIPS of whole frames for evaluation (EvalMetrics 'lpips'): no tape, no backward, any frame size.
 * Host arrays: recon_clips[i], target_clips[i] = contiguous clips [3][frames[i]][H][W] in `dtype` (device), all n_clips of ONE frame
 * size H x W, each in 16 .. 2048 and not necessarily a multiple of anything.  Frame t of a clip is read in place (channel stride
 * frames[i] * H * W); with clamp_recon != 0 the reconstruction is clamped to [-1, 1] in `dtype` before the scaling layer, the target
 * never.  Every frame pair is a batch entry of its own of the network above; the max-pools floor (torch MaxPool2d(2, 2): an odd stage
 * loses its last row or column), so stage s is (H >> s) x (W >> s) and tap k is averaged over its true (H >> k) * (W >> k) pixels.
 * TTV_F32 runs the exact-fp32 kernels, TTV_BF16 the MFMA path with the first convolution's scaled input rounded to bf16, as
 * ttv_lpips_forward does; for H and W multiples of 16 a call whose frames fit one pass gives ttv_lpips_forward's bits.
 * Outputs, either may be NULL but not both: per_frame (fp32, device) = one value per frame in clip then frame order
 * (sum of frames[] values); acc (double[2], device): acc[0] += every value, added one by one in that order by one thread,
 * acc[1] += the frame count.  No atomics: identical calls give identical bits.
 * The workspace (caller-owned, 256-byte aligned) holds two activation buffers for the largest stage, the head partials and the
 * split-K partials of one pass; the frames are worked through in passes of the largest size that workspace_bytes holds (at most
 * 2048 frames).  ttv_lpips_eval_workspace_bytes gives the size for passes of `frames` frames (1 .. 2048), -1 on a bad argument; less
 * than its value for one frame is TTV_ERR_INVALID.  Values of a frame may differ in the last bits between pass sizes in bf16 (the
 * split-K factor of a layer follows the stack's size).  Errors in the arguments return before any launch.
 * Work is enqueued on `stream` only; no synchronisation, no library state. */
int64_t ttv_lpips_eval_workspace_bytes(int frames, int H, int W, int dtype);
int ttv_lpips_eval_accumulate(const ttv_lpips_weights* w, void* const* recon_clips, void* const* target_clips, const int32_t* frames,
                              int n_clips, int H, int W, int dtype, int clamp_recon, float* per_frame, double* acc, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* The perceptual crops of the generator step (model/losses/loss_module.py:59-93) and their backward: what lies between the towers
 * and ttv_lpips_forward / ttv_lpips_backward.  Host arrays: recon_clips[i], target_clips[i] = contiguous clips [3][T][H][W] in `dtype`
 * (device), clip_dims = n_clips x (T, H, W), crops = n_crops x (clip, frame, H, W, Hr, Wr, oy, ox): the crop is cut from that frame
 * of that clip ((H, W) repeats the clip's size), Hr x Wr is the virtual resized frame - equal to H x W when the frame is not resized
 * (a resize that keeps the size, e.g. of a 128 x 128 frame at size 128, has the weights (0, 1, 0, 0) exactly and is taken as a copy too:
 * the same values for finite pixels; -0.0 stays -0.0 and an Inf / NaN does not spread to its neighbours as 0 * Inf would),
 * otherwise the short edge becomes `size` and the long edge int(size * long / short) (torchvision's resize(size)) - and (oy, ox) is the
 * origin of the size x size window in it.  n_clips and n_crops are any counts >= 1 (tables are split into launches inside), `size` a
 * multiple of 16 (16 .. 2048).  Outputs recon_crops, target_crops [n_crops][3][size][size] in `dtype`, 16-byte aligned.
 * Value of output element (c, i, j) of a crop, with v = min(max(x, -1), 1) for the reconstruction and v = x for the target:
 *   not resized: v at (oy + i, ox + j) of the frame, a copy;
 *   resized: torch's upsample_bicubic2d(align_corners=False), no antialiasing, at (oy + i, ox + j) of the resized frame.  Per axis
 *     n_in -> n_out: scale = (float)n_in / (float)n_out, src = fmaf(scale, dst + 0.5f, -0.5f), i0 = floor(src), t = src - i0, taps
 *     i0 - 1 .. i0 + 2 clamped to [0, n_in - 1], weights (Keys, A = -0.75, fp32) c2(t + 1), c1(t), c1(1 - t), c2(2 - t) with
 *     c1(x) = ((A + 2) x - (A + 3)) x x + 1 and c2(x) = ((A x - 5 A) x + 8 A) x - 4 A.  Rows are the outer loop and columns the
 *     inner: h_r = sum_k wx_k v[iy_r][ix_k], out = sum_r wy_r h_r, each sum an fmaf chain in ascending tap order from 0, fp32,
 *     rounded once to `dtype`.
 * ttv_lpips_crops_backward: from g [n_crops][3][size][size] (`dtype`, the gradient of recon_crops) the whole gradient of every
 * reconstruction clip, grad_clips[i] [3][T][H][W] in `dtype` (16-byte aligned), written once, with no memset: frames no crop names
 * are zeros; a sampled frame gets 1[-1 <= x <= 1] (R^T g), R the forward operator of its crop (pixels outside the window's
 * footprint: zeros; the mask is inclusive, torch's clamp backward).  R^T g is formed as a gather: an input pixel sums over the
 * output pixels whose clamped taps touch it - output rows ascending, per row columns ascending, taps ascending, fmaf in fp32, one
 * rounding - so there are no atomics and identical calls give identical bits.  A frame is sampled at most once.
 * TTV_ERR_INVALID with nothing launched: a bad dtype or size, a clip / frame index or (H, W) that does not match clip_dims, Hr x Wr
 * that is neither H x W nor the resize rule's, a window outside the virtual frame, a frame named twice, a misaligned destination.
 * Work is enqueued on `stream` only; no synchronisation, no library state. */
int ttv_lpips_crops_forward(void* const* recon_clips, void* const* target_clips, const int32_t* clip_dims, int n_clips, const int32_t* crops,
                            int n_crops, int size, void* recon_crops, void* target_crops, int dtype, void* stream);
int ttv_lpips_crops_backward(void* const* recon_clips, void* const* grad_clips, const int32_t* clip_dims, int n_clips, const int32_t* crops,
                             int n_crops, int size, const void* g, int dtype, void* stream);

/* ---- discriminator step: R1 / R2 noise and logit head (model/losses/loss_module.py:165-213) ------------- */
/* out_real = real + s and out_fake = fake + s for every element of every clip, the SAME s for both (:189-191), in one launch.
 * table  : DEVICE array of n_clips entries {const void* real; const void* fake; void* out_real; void* out_fake; const void* noise;
 *          int64 numel; int64 element_offset} (56 bytes each; tensors contiguous, in `dtype` = TTV_BF16 or TTV_F32; numel < 2^31);
 * chunks : DEVICE int32 [n_chunks][2] = (entry index, first element), first element a multiple of 8192: a chunk is up to 8192 elements.
 * Accesses are 16 bytes wide where the entry's pointers are 16-byte aligned, element by element otherwise and for the last
 * numel % (16 / element size) elements of a clip.
 * generate == 0: s = noise[i] (already scaled; `noise` must be given); out = one rounding of the exact sum, what torch's add gives.
 * generate != 0: `noise` is ignored and s is drawn, never stored.  Element i of an entry belongs to block (element_offset + i) / 4
 *   and is lane (element_offset + i) % 4 of it; element_offset must be a multiple of 4 (lay the clips end to end and round each
 *   clip's offset up).  The block's four words are Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 *   0xBB67AE85) of counter (block low, block high, draw low, draw high) under key (seed low, seed high).  A word x gives
 *   u = ((x >> 9) + 0.5) * 2^-23, exact in fp32 and strictly inside (0, 1).  Words (0, 1) and (2, 3) are one Box-Muller pair each:
 *   r = sqrt(-2 ln u_a), lanes (r cos 2 pi u_b, r sin 2 pi u_b), in fp32 (logf, sqrtf, sincospif).  A normal n is rounded to `dtype`
 *   (randn_like), s = n * gp_noise is rounded to `dtype`, and the sum is rounded to `dtype`.
 * Work is enqueued on `stream` only; no synchronisation, no library state. */
int ttv_gp_noise_add(const void* table, int n_clips, const int32_t* chunks, int n_chunks, int generate, uint64_t seed, uint64_t draw,
                     float gp_noise, int dtype, void* stream);

/* The logit head of either step and its gradient, one launch of one block.  per_token: the tower's per-token outputs [groups][n_clips]
 * [tokens_per_clip] in `dtype` (TTV_BF16 or TTV_F32), groups in the order real, fake (, real + noise, fake + noise); per_token_b, when
 * not NULL, holds the second half of the groups and per_token_a the first.  A clip's logit is the fp32 mean of its tokens rounded once
 * to `dtype`; everything after is fp32.  softplus is torch's (x above 20, else log1p(exp(x)); derivative 1 above 20, else z / (z + 1),
 * z = exp(x)).  With m = real - fake per clip:
 *   TTV_DISC_HEAD_GENERATOR (groups 2):          g_loss = softplus(m);  total = mean g_loss
 *   TTV_DISC_HEAD_DISCRIMINATOR (groups 2 or 4): d_loss = softplus(-m), logits_relative = m, with 4 groups r1 = (real - noisy real)^2
 *     and r2 = (fake - noisy fake)^2, with centering_weight > 0 centering = 0.5 (real + fake)^2;
 *     total = mean d_loss + gp_scale (mean r1 + mean r2) + centering_weight mean centering   (gp_scale = gp_weight / gp_noise^2)
 * terms fp32 [8]: total, d_loss | g_loss, logits_relative, r1, r2, centering (means over clips; zero where a term is off), 0, 0.
 * grad fp32 [groups n_clips tokens_per_clip]: d total / d per_token.  Any n_clips >= 1; sums in a fixed order, no atomics. */
#define TTV_DISC_HEAD_GENERATOR 0
#define TTV_DISC_HEAD_DISCRIMINATOR 1
int ttv_disc_head(const void* per_token_a, const void* per_token_b, int mode, int groups, int n_clips, int tokens_per_clip, int dtype,
                  float gp_scale, float centering_weight, float* terms, float* grad, void* stream);

/* Single operations (tests).  ttv_lpips_conv3x3: x [N][H][W][Cin] -> y [N][H][W][Cout], 3x3, stride 1, zero pad 1 per image, with
 * the weight image the dtype / shape rule above selects.  mode 0: y = relu(conv + bias); 1: y = conv * (h > 0), h [N][H][W][Cout];
 * 2: y = conv.  Workspace: ttv_lpips_conv_workspace_bytes (split-K partials; 0 when none).  ttv_lpips_maxpool: 2x2 / 2 max-pool of
 * NHWC x.  ttv_lpips_maxpool_backward: dx = (route(dy) + add) * (h > 0) over h [N][H][W][C], dy [N][H/2][W/2][C] (or NULL), add fp32
 * (or NULL); route sends each dy element to the first maximum of its window of h in row-major order. */
int64_t ttv_lpips_conv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype);
int ttv_lpips_conv3x3(const void* x, int N, int H, int W, int Cin, int Cout, const void* w, const float* bias, int mode, const void* h,
                      void* y, int dtype, void* workspace, int64_t workspace_bytes, void* stream);
int ttv_lpips_maxpool(const void* x, int N, int H, int W, int C, void* y, int dtype, void* stream);
int ttv_lpips_maxpool_backward(const void* dy, const float* add, const void* h, int N, int H, int W, int C, void* dx, int dtype,
                               void* stream);

/* ---- FVD: clip preprocessing and the I3D feature extractor (model/metrics/fvd.py FVDCalculator.update) ----------------------
 * I3D (Inception-v1 inflated, Kinetics-400 RGB) up to the 400 logits before the softmax, averaged over time, in fp32 with
 * activations channels-last.  58 convolutions in this order: 0 Conv3d_1a_7x7, 1 Conv3d_2b_1x1, 2 Conv3d_2c_3x3, then for the
 * Inception blocks Mixed_3b, 3c, 4b, 4c, 4d, 4e, 4f, 5b, 5c (b = 0 .. 8) 3 + 6 b + (b0, b1a, b1b, b2a, b2b, b3b), and 57 the logits.
 * w[i]: fp32 weight image [K][Cout], K = ((dt kH + dh) kW + dw) Cin + ci, i.e. W[co][ci][dt][dh][dw] -> [dt][dh][dw][ci][co].
 * scale[i], shift[i]: fp32 [Cout], the folded eval BatchNorm (y = conv * scale + shift, then ReLU).  The logits take shift[57] as
 * their bias and no scale (scale[57] may be NULL).  Every output is a fixed-order fp32 chain: a clip's features are
 * bit-identical whatever other clips share the launch. */
#define TTV_I3D_CONVS 58
#define TTV_I3D_FEATURES 400
typedef struct {
  const float* w[TTV_I3D_CONVS];
  const float* scale[TTV_I3D_CONVS];
  const float* shift[TTV_I3D_CONVS];
} ttv_i3d_weights;

/* Workspace of ttv_i3d_features for n clips (1 .. TTV_MAX_CLIPS_PER_LAUNCH), -1 on a bad n. */
int64_t ttv_i3d_workspace_bytes(int n);

/* Up to TTV_MAX_CLIPS_PER_LAUNCH contiguous clips [3][T][H][W] (host array of device pointers, `dtype`; dims = n_clips x
 * (C, T, H, W), host) -> out [n_clips][10][224][224][3] fp32: the clip clamped to [-1, 1] when `clamp` is set (the reference clamps
 * the reconstruction only), resampled trilinearly to 3 x 224 x 224 (torch align_corners=False; the reference's F.interpolate
 * asks for size (C, 224, 224), so the time axis always goes to C = 3 frames), frame 2 repeated into frames 3 .. 9. */
int ttv_fvd_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, int clamp, float* out, void* stream);

/* x: [n][10][224][224][3] fp32 (ttv_fvd_preprocess), feats: [n][400] fp32.  x and the workspace are 256-byte aligned. */
int ttv_i3d_features(const ttv_i3d_weights* w, const float* x, int n, float* feats, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* Single operations (tests).  ttv_i3d_conv3d: x [N][T][H][W][Cin] -> channels [c_off, c_off + Cout) of y [N][To][Ho][Wo][ldc],
 * a k x k x k convolution (k = 1, 3, 7) with stride 1 or 2 in every dimension and TF-SAME padding, y = conv * scale + shift
 * (scale / shift NULL: 1 / 0), ReLU when `relu`; w is the weight image above.  ttv_i3d_maxpool3d: kt x kh x kw max-pool with
 * strides st x sh x sw and TF-SAME padding (padded cells never win) of x [N][T][H][W][C] -> y [N][To][Ho][Wo][C]. */
int ttv_i3d_conv3d(const float* x, int N, int T, int H, int W, int Cin, int k, int stride, const float* w, const float* scale,
                   const float* shift, int Cout, int relu, float* y, int ldc, int c_off, void* stream);
int ttv_i3d_maxpool3d(const float* x, int N, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw, float* y,
                      void* stream);

/* ---- JEDi: clip preprocessing and the V-JEPA ViT-L/16 feature extractor (model/metrics/jedi.py JEDiMetric.get_feats) ------------
 * V-JEPA ViT-L/16 (patch 16, tubelet 2, 16 frames at 224^2 = 1568 tokens in (t, h, w) order, width 1024, 16 heads of 64, MLP 4096,
 * LayerNorm eps 1e-6) and the SSv2 probe's AttentivePooler (one query, one CrossAttentionBlock, LayerNorm eps 1e-5), with the
 * precision of bf16 autocast: linear / attention operands bf16, fp32 accumulation, softmax and LayerNorm statistics, an fp32
 * residual stream.  Every Linear's output is rounded to bf16 before its bias-free consumers (GELU, the residual add, pos_embed).
 * Linear weights are bf16 images [out][in] (patch_w: the Conv3d weight [1024][3][2][16][16] flattened to [1024][1536]); their biases
 * bf16 (autocast casts them too); LayerNorm weights / biases, pos_embed [1568][1024] and query_tokens [1024] fp32.
 * pool_q: bf16 [1024], xattn.q(query_tokens) as autocast computes it (the query is a constant: formed once per weight load). */
#define TTV_VJEPA_WIDTH 1024
#define TTV_VJEPA_TOKENS 1568
#define TTV_VJEPA_PATCH_K 1536
typedef struct ttv_vjepa_layer {
  const float* norm1_w; const float* norm1_b;
  const void* qkv_w; const void* qkv_b;       /* [3072][1024], [3072]: q | k | v (attn.qkv) */
  const void* proj_w; const void* proj_b;     /* [1024][1024] */
  const float* norm2_w; const float* norm2_b;
  const void* fc1_w; const void* fc1_b;       /* [4096][1024] */
  const void* fc2_w; const void* fc2_b;       /* [1024][4096] */
} ttv_vjepa_layer;
typedef struct ttv_vjepa_weights {
  int32_t width, heads, depth;                /* 1024, 16 (ViT-L only), blocks to run (24 for the checkpoint; fewer for tests) */
  const void* patch_w; const void* patch_b; const float* pos_embed;
  const ttv_vjepa_layer* layers;              /* HOST array [depth] */
  const float* norm_w; const float* norm_b;   /* the encoder's final norm */
  /* the pooler (classifier.pooler.*), needed for finetuned features only */
  const float* query_tokens; const void* pool_q;
  const float* pool_norm1_w; const float* pool_norm1_b;
  const void* pool_kv_w; const void* pool_kv_b;       /* [2048][1024]: k | v */
  const void* pool_proj_w; const void* pool_proj_b;
  const float* pool_norm2_w; const float* pool_norm2_b;
  const void* pool_fc1_w; const void* pool_fc1_b;
  const void* pool_fc2_w; const void* pool_fc2_b;
} ttv_vjepa_weights;

/* Up to TTV_MAX_CLIPS_PER_LAUNCH clips [3][T][S][S] (host array of device pointers, `dtype`; dims = n_clips x (C, T, H, W), host;
 * H == W, 1 <= T <= 16) -> out bf16 [n_clips * 1568][1536], the tubelet patch rows of the Conv3d in (c, kt, kh, kw) order: clamp to
 * [-1, 1], (v + 1) / 2, bicubic to 224 x 224 (F.interpolate, align_corners=False, antialias=False), (v - mean) / std with ImageNet's
 * mean / std, the last frame repeated up to 16 frames; fp32 arithmetic, one rounding.  16-byte aligned out. */
int ttv_jedi_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, void* out, void* stream);
/* Workspace of ttv_vjepa_features for n clips (1 .. TTV_MAX_CLIPS_PER_LAUNCH), -1 on a bad n. */
int64_t ttv_vjepa_workspace_bytes(int n);
/* x: ttv_jedi_preprocess's rows for n clips -> feats fp32 [n][1024]: the pooler's output (finetuned != 0) or the mean of the final
 * norm's output over the 1568 tokens.  Nothing sums across clips: a clip's features do not depend on the others.  Workspace 256-byte
 * aligned. */
int ttv_vjepa_features(const ttv_vjepa_weights* w, const void* x, int n, float* feats, int finetuned, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* Single operations (tests).  ttv_vjepa_layernorm: y = LN2(LN1(x)) or LN1(x) (w2 NULL) of fp32 rows of width 1024; y32 (optional) the
 * first norm's fp32 output (may alias x), y16 (optional) the last norm's bf16 output.  ttv_vjepa_linear: y = x w^T + bias on bf16
 * operands with epilogue TTV_VJEPA_EPI_STORE (bf16 y), _GELU (bf16 y = gelu_erf(bf16(acc + bias))) or _RESID (fp32 y = resid[r] +
 * bf16(acc + bias), r = row % resid_rows or row when resid_rows == 0; y may alias resid); N % 128 == 0, K % 64 == 0.
 * ttv_vjepa_pool_attention: out bf16 [n][1024] = per head softmax(q k^T / 8) v with q bf16 [1024] and kv bf16 [n * rows][2048] (k | v). */
#define TTV_VJEPA_EPI_STORE 0
#define TTV_VJEPA_EPI_GELU 1
#define TTV_VJEPA_EPI_RESID 2
int ttv_vjepa_layernorm(const float* x, int ldx, int rows, int width, const float* w1, const float* b1, float eps1, const float* w2,
                        const float* b2, float eps2, float* y32, int ld32, void* y16, int ld16, void* stream);
int ttv_vjepa_linear(const void* x, int ldx, const void* w, int ldw, const void* bias, int M, int N, int K, int epilogue,
                     const float* resid, int ldr, int resid_rows, void* y, int ldy, void* stream);
int ttv_vjepa_pool_attention(const void* q, const void* kv, int n, int rows, void* out, void* stream);

/* ---- FID / IS / MMD: frame preprocessing and the Inception-v3 feature extractor (model/metrics/metrics.py MetricCalculator) ------
 * torchvision's Inception-v3 trunk (no transform_input, no AuxLogits) up to the 2048 activations after the 8 x 8 average pool, the fc
 * logits and their softmax, in fp32 with activations channels-last.  94 units (bias-free convolution, eval BatchNorm eps 1e-3, ReLU)
 * in torchvision's module order: 0 .. 4 the stem (Conv2d_1a_3x3, 2a_3x3, 2b_3x3, 3b_1x1, 4a_3x3); 5 .. 25 Mixed_5b, 5c, 5d, 7 each
 * (branch1x1, branch5x5_1, _2, branch3x3dbl_1, _2, _3, branch_pool); 26 .. 29 Mixed_6a (branch3x3, branch3x3dbl_1, _2, _3);
 * 30 .. 69 Mixed_6b .. 6e, 10 each (branch1x1, branch7x7_1, _2, _3, branch7x7dbl_1 .. _5, branch_pool); 70 .. 75 Mixed_7a
 * (branch3x3_1, _2, branch7x7x3_1 .. _4); 76 .. 93 Mixed_7b, 7c, 9 each (branch1x1, branch3x3_1, _2a, _2b, branch3x3dbl_1, _2, _3a,
 * _3b, branch_pool).
 * unit[i].w: fp32 weight image [K][Cout], K = (dh kW + dw) Cin + ci, i.e. W[co][ci][dh][dw] -> [dh][dw][ci][co], 16-byte aligned.
 * unit[i].scale, .shift: fp32 [Cout], the folded BatchNorm (y = conv * scale + shift, then ReLU).  fc_w: fp32 [2048][1000] (the
 * transpose of fc.weight), fc_b: fp32 [1000].  Every output is a fixed-order fp32 chain: an image's features are bit-identical
 * whatever other images share the launch. */
#define TTV_INCEPTION_UNITS 94
#define TTV_INCEPTION_FEATURES 2048
#define TTV_INCEPTION_CLASSES 1000
#define TTV_INCEPTION_INPUT 299
#define TTV_INCEPTION_POOL_AVG3 0
#define TTV_INCEPTION_POOL_MAX3S2 1
typedef struct ttv_inception_unit {
  const float* w;
  const float* scale;
  const float* shift;
} ttv_inception_unit;
typedef struct ttv_inception_weights {
  ttv_inception_unit unit[TTV_INCEPTION_UNITS];
  const float* fc_w;
  const float* fc_b;
} ttv_inception_weights;

/* Workspace of ttv_inception_features for n images (1 .. TTV_MAX_CLIPS_PER_LAUNCH), -1 on a bad n. */
int64_t ttv_inception_workspace_bytes(int n);

/* Up to TTV_MAX_CLIPS_PER_LAUNCH images [3][H][W] (host array of device pointers, `dtype`; dims = n x (H, W, channel stride in
 * elements), host: rows are contiguous, and a frame t of a contiguous clip [3][T][H][W] is the image at clip + t H W with channel
 * stride T H W) -> out [n][299][299][3] fp32: clamped to [-1, 1] when `clamp` is set, resized bilinearly with torch's
 * align_corners=True rule (nn.Upsample(size=(299, 299), mode='bilinear', align_corners=True)). */
int ttv_inception_preprocess(void* const* images, const int64_t* dims, int n, int dtype, int clamp, float* out, void* stream);

/* x: [n][299][299][3] fp32 (ttv_inception_preprocess) -> acts [n][2048] fp32 and, unless probs is NULL, probs [n][1000] fp32 (the
 * softmax of fc(acts)).  x and the workspace are 256-byte aligned. */
int ttv_inception_features(const ttv_inception_weights* w, const float* x, int n, float* acts, float* probs, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* Single operations (tests).  ttv_inception_conv2d: x [N][H][W][Cin] -> channels [c_off, c_off + Cout) of y [N][Ho][Wo][ldc], a
 * kh x kw convolution (1 .. 7 each) with strides sh x sw (1 or 2) and zero padding ph x pw (Ho = (H + 2 ph - kh) / sh + 1),
 * y = conv * scale + shift (scale / shift NULL: 1 / 0), ReLU when `relu`; w is a weight image as above, Cout % 4 == 0.
 * ttv_inception_pool2d: TTV_INCEPTION_POOL_AVG3 (3 x 3, stride 1, padding 1, always divided by 9) or TTV_INCEPTION_POOL_MAX3S2
 * (3 x 3, stride 2, no padding) of x [N][H][W][C] -> channels [c_off, c_off + C) of y [N][Ho][Wo][ldc]. */
int ttv_inception_conv2d(const float* x, int N, int H, int W, int Cin, int kh, int kw, int sh, int sw, int ph, int pw, const float* w,
                         const float* scale, const float* shift, int Cout, int relu, float* y, int ldc, int c_off, void* stream);
int ttv_inception_pool2d(const float* x, int N, int H, int W, int C, int mode, float* y, int ldc, int c_off, void* stream);

/* ---- measurement hook (bench.py roofline leg) ---------------------------------------------------------- */
/* Kernel classes whose launches can be bracketed by HIP events on the stream they are launched on. */
#define TTV_KC_ATTENTION 1
#define TTV_KC_GEMM_QKV 2
#define TTV_KC_GEMM_GEGLU 3
#define TTV_KC_GEMM_RESID 4
#define TTV_KC_GEMM_STORE 5
#define TTV_KC_RMSNORM 6
#define TTV_KC_PATCH 7
#define TTV_KC_ROWS 8
/* Start recording launches of `kernel_class` (up to max_records; events are created here, outside any launch path).
 * This is the only process-global state in the library and it is off by default. */
int ttv_prof_begin(int kernel_class, int max_records);
/* Diagnostics for kernel ablation timing / tests (never set in product use): an OR of the TTV_DBG_* bits below.
 * The flags belong to the CALLING HOST THREAD (thread-local): launches made by other threads are unaffected.
 * The values are cited by number in tools/, profiles/ and DESIGN.md and never change.  Where a value is read by two kernels' worth of
 * code with two meanings it has two names (marked "same value as"); tools/README.md lists every bit beside the environment switches,
 * titok_video_amd/_lib.py mirrors the table as DBG_* (tests/test_cabi_cpu.py holds the two equal). */
enum {
  TTV_DBG_NO_STORES = 1,               /* GEMM, k_qkv256(ws) and k_mlp256 epilogues store nothing; k_gemm_k256 also skips the rotary (ttv_gemm.hip, ttv_qkv256*.inc, ttv_mlp.hip) */
  TTV_DBG_K256_NO_PANEL_DMA = 2,       /* k_gemm_k256: no weight-panel DMA after the first (ttv_gemm.hip) */
  TTV_DBG_MLP_NO_WEIGHT_DMA = 2,       /* k_mlp256: no w12 / w3 panel DMA after the first; same value as K256_NO_PANEL_DMA (ttv_mlp.hip) */
  TTV_DBG_K256_NO_TILE_RELOAD = 4,     /* k_gemm_k256: token rows are not reloaded when a block's range enters the next tile (ttv_gemm.hip) */
  TTV_DBG_MLP_NO_GEGLU = 4,            /* k_mlp256: no GEGLU arithmetic, garbage results; same value as K256_NO_TILE_RELOAD (ttv_mlp.hip) */
  TTV_DBG_K256_NO_EPILOGUE_MATH = 8,   /* k_gemm_k256: no folded pre-norm / rotary arithmetic in the epilogue, garbage results (ttv_gemm.hip) */
  TTV_DBG_MLP_TILES8 = 8,              /* ttvk_mlp_fused: force the 2-tile pair variant; same value as K256_NO_EPILOGUE_MATH (ttv_mlp.hip) */
  TTV_DBG_MLP_NO_P2 = 16,              /* k_mlp256: no w3 (P2) MFMAs, garbage results (ttv_mlp.hip) */
  TTV_DBG_MLP_PAIRS_ONLY = 32,         /* ttvk_mlp_fused: never choose the 9-tile deal (ttv_mlp.hip) */
  TTV_DBG_MLP_TILES4 = 64,             /* ttvk_mlp_fused: force the 1-tile pair variant (ttv_mlp.hip) */
  TTV_DBG_GEMM_TILE160 = 128,          /* general-K bf16 / fp32 / gather GEMM: force the 160-token tile (ttv_gemm.hip) */
  TTV_DBG_GEMM_TILE128 = 256,          /* general-K bf16 / fp32 / gather GEMM: force the 128-token tile; TILE160 wins when both are set (ttv_gemm.hip) */
  TTV_DBG_GEMM_T256 = 512,             /* bf16 GEMM: force k_gemm_bf16_t256 (256 x 256 tiles) wherever it applies (ttv_gemm.hip) */
  TTV_DBG_MLP_TILES9 = 512,            /* ttvk_mlp_fused: force the 9-tile eight-wave deal; same value as GEMM_T256 (ttv_mlp.hip) */
  TTV_DBG_GEMM_NO_T256 = 1024,         /* bf16 GEMM: never k_gemm_bf16_t256 (ttv_gemm.hip) */
  TTV_DBG_MX_UNFUSED_QUANT = 2048,     /* block-scaled fp8 layers: every operand quantised by a pass of its own, as TTV_MX_FUSED_QUANT=0 (ttv_api.hip) */
  TTV_DBG_SPLIT3_NO_IMAGES = 4096,     /* split-bf16 towers: fp32 activations, split inside the GEMMs, as TTV_SPLIT3_IMAGES=0 (ttv_api.hip) */
  TTV_DBG_SPLIT3_NO_DMA = 8192,        /* fp32 GEMM: the register-staged kernel instead of k_gemm_split_dma, as TTV_SPLIT3_DMA=0 (ttv_gemm.hip) */
  TTV_DBG_K256_GENERAL = 16384,        /* bf16 K = 256 GEMM without folded pre-norm or patch scatter: through the general-K kernels (ttv_gemm.hip) */
  TTV_DBG_QKV256_OFF = 32768,          /* to_qkv at K = 256: k_gemm_k256<EPI_QKV_ROPE> instead of k_qkv256, as TTV_QKV256=0 (ttv_gemm.hip) */
  TTV_DBG_QKV256_WS = 131072,          /* to_qkv at K = 256: the weight-stationary k_qkv256ws, as TTV_QKV256=2 (ttv_gemm.hip) */
  TTV_DBG_ENC_ALL_ROWS = 524288,       /* encoder's last layer on every row, as TTV_ENC_LATENT_LAST=0 (ttv_api.hip, ttv_train.hip) */
  TTV_DBG_ATTN_NO_SWP = 1048576,       /* ttvk_attention keeps k_attn_bf16 where it would take k_attn_swp, as TTV_ATTN_SWP=0 (ttv_attn.hip) */
  TTV_DBG_DEC_ALL_BLOCKS = 2097152,    /* decoder's last attention on every query block, as TTV_DEC_PATCH_LAST=0 (ttv_api.hip) */
  TTV_DBG_DEC_L0_NO_CONST = 4194304,   /* decoder's layer 0 ignores the constant block, as TTV_DEC_L0_CONST=0 (ttv_api.hip) */
  TTV_DBG_ENC_LAST_QKV_ALL = 8388608,  /* encoder's last to_qkv computes every panel of every row, as TTV_ENC_LAST_QKV_SKIP=0 (ttv_api.hip) */
  TTV_DBG_PATCH_EMBED_UNFUSED = 16777216 /* encoder's front as the gathering GEMM and the row kernel, as TTV_PATCH_EMBED_FUSED=0 (ttv_api.hip) */
};
int ttv_debug_set(int flags);
/* Diagnostics: device buffer (>= 256 int64) that instrumented kernels fill with s_memtime stamps of block 0; NULL = off. */
int ttv_debug_stamps(void* device_buffer);
/* Synchronise the recorded events, return their summed duration (ms) and count, and release them. */
int ttv_prof_end(double* total_ms, int* count);

#ifdef __cplusplus
}
#endif
#endif /* TITOK_HIP_H */
