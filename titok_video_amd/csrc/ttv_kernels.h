// Internal launch functions (host side).  The C-ABI in include/titok_hip.h is layered on these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/titok_hip.h"

// ---- ttv_elem.hip ----
int ttvk_rmsnorm(const void* in, int in_dtype, int ld_in, const int* src_rows, void* out, int out_dtype, int ld_out,
                 const int* dst_rows, const float* gain, int rows, int d, float eps, hipStream_t s, float* next_rstd = nullptr,
                 void* mx_q = nullptr, void* mx_s = nullptr,    // mx_q / mx_s: the stored row also as block-scaled e4m3 [rows, d] + its E8M0 scales
                 int split_image = 0);                          // fp32 output written as the split-bf16 image (hi0..3 | lo0..3 per four elements)
int ttvk_row_rstd(const void* in, int dtype, int ld_in, float* rstd, int rows, int d, float eps, hipStream_t s);
// dst[dst_rows ? dst_rows[r] : r] = src[src_rows ? src_rows[r] : r] for r < rows; row_bytes a multiple of 16, rows 16-byte aligned
int ttvk_copy_rows(const void* src, int64_t ld_src_bytes, const int* src_rows, void* dst, int64_t ld_dst_bytes, const int* dst_rows, int rows,
                   int row_bytes, hipStream_t s);
int ttvk_fill_const_rows(void* x, int dtype, int ld, const int* rows_map, int rows, int d, const float* mask_token,
                         const float* gain, float eps, hipStream_t s);
int ttvk_dec_embed(const void* codes, int C, const void* w, const void* bias, const float* mask_token, const float* gain,
                   void* x, int dtype, int ld, const int* rows_map, int rows, int d, float eps, hipStream_t s);
int ttvk_fsq_forward(const ttv_fsq_params* p, const void* z, int z_dtype, int rows, void* codes, int codes_dtype, int* indices,
                     float* bounded, hipStream_t s);
int ttvk_fsq_indices_to_codes(const ttv_fsq_params* p, const int* indices, int rows, void* codes, int codes_dtype, hipStream_t s);
int ttvk_enc_tail(const void* x, int dtype, int ld, const int* rows_map, int rows, int d, const float* gain, float eps,
                  const void* w, const void* bias, int C, const ttv_fsq_params* fsq, float* z_out, void* codes, int* indices,
                  float* bounded, hipStream_t s);
int ttvk_patch_copy(bool scatter, void* const* clips, const int* clip_desc, int clip0, int n_clips, int pt, int ph, int pw,
                    int C, void* patches, int ld, int dtype, int max_patches, hipStream_t s);
int ttvk_rope_apply(void* x, int dtype, int ld, int rows, int heads, const float* cs, hipStream_t s);
int ttvk_histogram(const int* idx, int n, int64_t* counts, int size, hipStream_t s);
int ttvk_quant_rows_fp8(const void* in, int in_dtype, int ld_in, const float* gain, float eps, void* out, int ld_out, float* scales, int rows,
                        int d, hipStream_t s);

int ttvk_split3_pack(const float* w, int ldw, void* out, int ldo, int rows, int K, hipStream_t s);
int64_t ttvk_mx_scale_ld(int d);     // bytes of E8M0 scales per row of width d
int ttvk_quant_mx_fp8(const void* in, int in_dtype, int ld_in, void* out, int ld_out, void* mx, float* row_scales, int rows, int d, hipStream_t s);

int ttvk_clip_from_u8(const void* frames, long long n_pix, void* clip, int dtype, hipStream_t s);

// ---- ttv_resample.hip ----
// geom: n_clips x (T, Hs, Ws, Hr, Wr, oy, ox, Ho, Wo, flip), host
int ttvk_clip_resample_u8(void* const* src, void* const* dst, const int32_t* geom, int n_clips, int dtype, hipStream_t s);

// ---- ttv_gemm.hip ----
// out^T-oriented GEMM: the MFMA "row" side is the output feature (W rows), the "column" side the token (X rows),
// so every lane owns 4 consecutive output features of one token and the epilogues below are lane-local.
enum GemmEpilogue {
  EPI_STORE = 0,   // y = acc (+bias) (+*add_scalar), stored in dtype
  EPI_QKV_ROPE,    // y = acc with rotary applied to the q and k column ranges (transformer.py:87,97-98)
  EPI_GEGLU,       // y[:, f] = gelu(acc[:, I+f]) * acc[:, f]           (transformer.py:51-52)
  EPI_RESID_T,     // y = alpha*resid + acc, stored in dtype            (layer 0 residual, transformer.py:129-130)
  EPI_RESID_F32,   // y = alpha*resid + acc, stored fp32                (KEEL pre-post-norm sum, transformer.py:141,144)
  EPI_RESID_NORM,  // y = RMSNorm(alpha*resid + acc) * norm_gain, stored in dtype (whole KEEL step, transformer.py:141-145);
                   // needs a kernel whose waves own full rows: bf16, K == 256, N == 256 (ttvk_gemm_supports_resid_norm)
  EPI_STORE_PATCH, // y = acc + bias written straight into the clips as patches (blocks.py:173-176 + utils.py:37-51; bf16, K = 256)
  // V-JEPA linears under bf16 autocast (model/metrics/jedi.py; ttv_vjepa.hip).  bias is dtype; the Linear's output is rounded to dtype
  // before anything else is applied to it, as autocast's bf16 F.linear output is
  EPI_BIAS_PLAIN,  // y = acc + bias, stored in dtype (EPI_STORE's arithmetic on the fixed kernel below)   (attn.qkv, pooler kv)
  EPI_BIAS_GELU,   // y = gelu_erf(round(acc + bias)), stored in dtype                                         (mlp.fc1 + GELU)
  EPI_BIAS_RESID_F32R,  // y = resid[r] + round(acc + bias), fp32 resid / y, r = row % resid_rows (0: row); y may alias resid
};

struct GemmArgs {
  const void* x; int ldx;          // tokens  [M,K]
  const void* w; int ldw;          // weights [N,K]  (EPI_GEGLU: [2I,K], N = I)
  int M, N, K;
  void* y; int ldy;
  const void* bias;                // [N] dtype or null
  const float* add_scalar;         // device scalar or null
  const void* resid; int ldr;      // [M,N] dtype
  float alpha;
  const float* rope_cs;            // [M,64]
  const int* rope_ids; const float* rope_base;   // optional (ttv_batch.rope_ids / rope_base): the K == 256 bf16 kernel gathers its factors through them
  int rope_q_end, rope_k_begin, rope_k_end;  // column ranges [0,q_end) and [k_begin,k_end) get rotary
  int dtype;
  const float* norm_gain;          // EPI_RESID_NORM: post-norm gain [N]
  // EPI_RESID_NORM, optional (training tape): the pre-norm sum alpha * resid + acc in fp32, and RMSNorm(y) * norm_gain2 of the stored
  // (rounded) row = the next pre-norm's output, so that neither needs a launch of its own
  float* sum_f32; int ld_sum;
  void* y2; int ldy2; const float* norm_gain2;
  void* yq; void* yq_mx;           // ttvk_gemm_fp8 with block scales, EPI_GEGLU: the output leaves as block-scaled e4m3 [M, N] (ld N) + E8M0 scales
                                   // (k_quant_mx_fp8's layout for width N) instead of bf16 y - the next linear's operand, no pass of its own
  int split3;                      // fp32 only: w is the split-bf16 image of the weight (ttv_split3_pack) and the products run as three bf16
                                   // MFMA passes (k_gemm_f32<.., SPLIT>)
  int x_image, y_image;            // split3: x is already a split image (written by its producer: no split in the staging) / y is written as one
                                   // (1: per four features hi0..3 | lo0..3, STORE / GEGLU; 2: to_qkv - q, k, v per eight features hi0..7 | lo0..7,
                                   // the attention kernel's operand format, gate columns fp32)
  int prenorm;                     // 1: w has the RMSNorm gain folded in, x is the un-normalised row (bf16, K == 256 only)
  const float* row_scale;          // optional [M]: output row t is multiplied by row_scale[t] before the epilogue (the rstd of a pre-norm
                                   // whose gain is folded into w: any K; bf16 kernels)
  const int* x_rows;               // optional (bf16, K == 256): GEMM row t reads x row x_rows[t]
  float eps;
  // EPI_STORE_PATCH (output side) / gather (EPI_STORE, input side): row t of the GEMM is patch t (clip-major); its clip is
  // row_seq[patch_rows[t]]; x (gather) resp. y (scatter) is then unused
  int gather;
  void* const* clips;              // HOST array of device pointers to the [C,T,H,W] outputs of clips clip0 .. clip0+n_clips-1
  int n_clips;
  const int* clip_desc;            // device [*,8], see ttv_patch_gather
  const int* patch_rows;           // device [M]
  const int* row_seq;              // device [L]
  int patch_t, patch_h, patch_w;   // powers of two; patch_w * sizeof(bf16) == 16
  int resid_rows;                  // EPI_BIAS_RESID_F32R: the residual row of GEMM row t is t % resid_rows (0: t)
  // optional (EPI_QKV_ROPE on k_qkv256 only): of every tile_period consecutive 128-row token tiles only the first tile_run are computed
  // and stored, rows and outputs in place; the other rows of y are not touched.  0 / 0: every tile.  M % (128 * tile_period) == 0.
  int tile_run, tile_period;
  // optional, with a tile list: panel_lo > 0 computes the other tiles of a period as well, but only their 64-feature panels panel_lo ..
  // N / 64 - 1 (columns [64 * panel_lo, N)); the columns in front of those rows of y are not touched.  0: today's tile list.
  int panel_lo;
};
struct ClipPtrs { void* p[TTV_MAX_CLIPS_PER_LAUNCH]; };
int ttvk_gemm(GemmEpilogue epi, const GemmArgs& a, hipStream_t s);
// x_mx / w_mx: E8M0 block scales (ttvk_quant_mx_fp8's layout) - both or neither; with them the fp32 row factors are optional
int ttvk_gemm_fp8(GemmEpilogue epi, const GemmArgs& a, const float* x_scale, const float* w_scale, hipStream_t s, const void* x_mx = nullptr,
                  const void* w_mx = nullptr);
bool ttvk_gemm_supports_resid_norm(int dtype, int N, int K);
bool ttvk_gemm_qkv_tiles_supported(int d_model, int gqa_dim, int ldw);

// ---- ttv_patch_embed.hip: the encoder's front in one kernel (gather + proj_in + mask token + ln_pre_p), width 256 bf16 ----
bool ttvk_patch_embed_norm_supported(int dtype, int width, int patch_dim, int patch_w);
int ttvk_patch_embed_norm(void* const* clips, int clip0, int n_clips, const int* clip_desc, const int* patch_rows, const int* row_seq,
                          int patch_t, int patch_h, int patch_w, int patch_dim, const void* w, int ldw, const void* bias,
                          const float* mask_token, const float* gain, float eps, void* x, int ldx, int M, hipStream_t s);
   // GemmArgs.tile_run / tile_period: will this to_qkv take them?

// ---- ttv_attn.hip ----
int ttvk_attention(const void* qkvg, int ld, void* out, int ldo, const int* cu_seqlens, const int* qblocks, int n_qblocks,
                   int q_heads, int kv_heads, int head_dim, int flags, int dtype, hipStream_t s, float* lse_out = nullptr,
                   void* out_raw = nullptr);

// bf16 tables of full items, pre-scaled q, no tape outputs: the software-pipelined kernel (ttv_attn_swp.hip); ttvk_attention dispatches
bool ttvk_attention_takes_swp(int flags);
// rows2 / kwin (optional): rows [kwin, S) of every sequence are read from rows2 [S - kwin, ld] instead of from qkvg; state (optional, with
// rows2): what ttvk_attention_swp_dump wrote for rows2 - query blocks behind kwin loop over the keys [0, kwin) and add it (see k_attn_swp)
int ttvk_attention_swp(const void* qkvg, int ld, void* out, int ldo, const int* cu_seqlens, const int* qblocks, int n_qblocks,
                       int q_heads, int kv_heads, int gate_mul, hipStream_t s, const void* rows2 = nullptr, int kwin = 0,
                       const float* state = nullptr);
int64_t ttvk_attention_swp_state_floats(int n_rows, int q_heads);
int ttvk_attention_swp_dump(const void* rows, int ld, int n_rows, int q_heads, int kv_heads, float* state, hipStream_t s);
int ttvk_attention_mxout(const void* qkvg, int ld, void* out_q, void* out_mx, int ld_mx, const int* cu_seqlens, const int* qblocks,
                         int n_qblocks, int q_heads, int kv_heads, hipStream_t s);

// ---- ttv_attn_pv8.hip: opt-in inference attention with an e4m3 P.V product (see the file's header) ----
int64_t ttvk_attention_pv8_bytes(int total_rows, int n_seqs, int kv_heads);
int ttvk_quant_v_pv8(const void* qkvg, int ld, const int* cu_seqlens, int n_seqs, int total_rows, int q_heads, int kv_heads, void* image,
                     hipStream_t s);
int ttvk_attention_pv8(const void* qkvg, int ld, void* out, int ldo, const int* cu_seqlens, const int* qblocks, int n_qblocks, int q_heads,
                       int kv_heads, int head_dim, int flags, const void* image, hipStream_t s);

// ---- ttv_attn64.hip ----
int ttvk_attention64(const void* qkvg, int ld, void* out, int ldo, const int* cu_seqlens, const int* items, int n_items, int q_heads,
                     int kv_heads, int flags, hipStream_t s);

// ---- ttv_vq.hip (nearest-codebook-entry quantiser) ----
int ttvk_vq_norms(const void* cb, int dtype, int ld, int N, int C, float* cnorm, hipStream_t s);
int64_t ttvk_vq_workspace_bytes(int rows);
int ttvk_vq_l2_argmin(const void* z, int dtype, int ldz, const void* cb, int ldc, const float* cnorm, int rows, int N, int C, int* indices,
                      float* best_dist, void* workspace, int64_t workspace_bytes, hipStream_t s);
int ttvk_vq_lookup(const void* cb, int dtype, int ldc, const int* indices, int rows, int C, void* codes, int ldo, hipStream_t s);
int ttvk_vq_lookup_bwd(const void* dcodes, int dtype, int ld, const int* indices, int rows, int C, float* dcb, int ldc, hipStream_t s);
// deterministic form: an owner per codebook entry adds its rows in ascending row order (no partials, no scratch); N = codebook entries
int ttvk_vq_lookup_bwd_det(const void* dcodes, int dtype, int ld, const int* indices, int rows, int N, int C, float* dcb, int ldc, hipStream_t s);

// ---- ttv_vq_train.hip (commitment term, EMA codebook update, dead-entry restart) ----
int64_t ttvk_vq_train_workspace_bytes(int rows, int N);
int ttvk_vq_commit_forward(const void* z, int dtype, int ldz, const void* cb, int ldc, const int* idx, int rows, int N, int C, float* loss,
                           void* workspace, int64_t workspace_bytes, hipStream_t s);
int ttvk_vq_commit_backward(const void* g, int ldg, const void* z, int ldz, const void* e, int lde, int dtype, int rows, int C, double scale,
                            void* dz, int ldd, hipStream_t s);
int ttvk_vq_ema_stats(const void* z, int dtype, int ldz, const int* idx, int rows, int N, int C, const float* cluster_size, float dead_threshold,
                      uint64_t seed, const int64_t* ema_step, int rank, int world_size, float* stats, void* workspace, int64_t workspace_bytes,
                      hipStream_t s);
int ttvk_vq_ema_update(const float* stats, float* cluster_size, float* embed_avg, float* codebook, void* copy, int copy_dtype, float* cnorm,
                       int64_t* ema_step, int N, int C, float decay, float one_minus_decay, float eps, float dead_threshold, void* workspace,
                       int64_t workspace_bytes, hipStream_t s);

// ---- ttv_mlp.hip ----
bool ttvk_mlp_fused_supported(int dtype, int width, int inner);
struct MlpNextQkv {     // optional fused back of the layer-tail kernel: the next layer's qkv projection + rotary
  void* qkv; int ld;    // [M, ld] output, (q | gate | k | v)
  const float* rope_cs; // [M, 64] (cos | sin)
  int rows;             // rows of the folded to_qkv packed behind the feed-forward images (% 64 == 0)
  int rope_q_end, rope_k_begin, rope_k_end;
};
int64_t ttvk_mlp_pack_bytes(int inner, int next_qkv_rows);
int ttvk_mlp_pack(const void* w12_folded, const void* w3, const void* wo, const void* next_qkv_folded, int next_qkv_rows, int inner,
                  void* packed, hipStream_t s);
int ttvk_mlp_fused(const void* ao, int ldao, const float* front_gain, float front_alpha, const void* x, int ldx, const void* packed,
                   int inner, void* y, int ldy, const float* post_gain, float alpha, float eps, int M, const MlpNextQkv* nq, hipStream_t s);

// ---- ttv_bwd.hip (backward kernels) ----
// Deterministic mode (ttv_det()): the reductions below that add block partials onto shared addresses write them to `det` instead, as
// [block][element] (the layouts: include/titok_hip.h beside the ttv_*_det_scratch_bytes functions), and k_det_fold adds the partials of
// an element in ascending block index and the total onto the destination.  One scratch serves every launch of one stream in turn (the
// fold of a launch is ordered in front of the next launch's partials); with the mode on a launch that needs partials and has no
// scratch, or too little, is TTV_ERR_INVALID before anything runs.  Mode off: `det` is not looked at.
// The argument is not optional: a call site says where its partials go (NULL only behind a public entry point that has refused the mode).
struct DetScratch { void* p; int64_t bytes; };
int64_t ttvk_det_rms_bytes(int rows, int d);                 // one gain: [blocks][d] fp32; the chain kernel takes two of these side by side
int64_t ttvk_det_colsum_bytes(int rows, int n);              // [row blocks][n] fp32
int64_t ttvk_det_sumall_bytes(long total);                   // [blocks] fp32
int64_t ttvk_det_outer_small_bytes(int rows, int C, int d);  // [row blocks][min(C, TTV_MAX_FSQ)][d] fp32 (one column chunk at a time)
int64_t ttvk_det_clips_bytes(const int* sizes, int n_clips, bool l1);   // l1_loss: [clip][block] fp32; sq_err: [clip][block][2] double; any n_clips: the largest launch group
int ttvk_l1_loss(void* const* recon, void* const* target, void* const* grad, const int* sizes, int n_clips, int total_clips, int dtype,
                 float* loss, hipStream_t s, const DetScratch* det);
int ttvk_sq_err(void* const* recon, void* const* target, const int* sizes, int n_clips, int dtype, int clamp, double* acc2, hipStream_t s,
                const DetScratch* det);
// dx (fp32, in/out) = out_scale * B(A), cast_out = (T) B(A) with A = dx + rmsnorm_bwd(x, gain1, dy), B = rmsnorm_bwd(y, gain2, .) or
// identity when y == NULL; gain gradients accumulated (dgain1 / dgain2 may be NULL): one atomicAdd per block and column, or - deterministic
// mode - block partials in `det` (gain 1's array, gain 2's behind it) and two folds; cast_out may be NULL
int ttvk_rmsnorm_bwd_chain(const void* x, int ldx, const void* dy, int lddy, const float* gain1, float* dgain1, float* dx, int lddx,
                           const void* y, int y_dt, int ldy, const float* gain2, float* dgain2, float out_scale, void* cast_out, int ldc, int rows,
                           int d, float eps, int dt, hipStream_t s, const DetScratch* det);
int ttvk_rmsnorm_bwd(const void* x, int x_dt, int ldx, const int* xr, const void* dy, int dy_dt, int lddy, const int* dyr,
                     const float* gain, void* dx, int dx_dt, int lddx, const int* dxr, int acc, float* dgain, int rows, int d, float eps,
                     hipStream_t s, const DetScratch* det);
int ttvk_colsum(const void* a, int dt, int lda, const int* rows_map, int rows, int n, float* out, hipStream_t s, const DetScratch* det);
int ttvk_sumall(const void* a, int dt, int lda, const int* rows_map, int rows, int n, const float* colw, float scale, float* out, hipStream_t s,
                const DetScratch* det);
int ttvk_gate_fwd(const void* a, int lda, const void* gate, int ldg, void* ag, int ldo, int rows, int d, int dt, hipStream_t s);
int ttvk_gate_bwd(const void* dag, int ldd, const void* a, int lda, const void* gate, int ldg, void* da, int ldda, void* dgate, int lddg,
                  int rows, int d, int dt, float* delta, hipStream_t s);
int ttvk_geglu_fwd(const void* u, int ldu, void* h, int ldh, int rows, int I, int dt, hipStream_t s);
int ttvk_geglu_bwd(const void* u, int ldu, const void* dh, int lddh, void* du, int lddu, int rows, int I, int dt, hipStream_t s);
int ttvk_scale_cast(const float* a, float alpha, float* b, void* c, int dt, long n, hipStream_t s);
int ttvk_to_f32(const void* a, int dt, float* b, long n, int accumulate, hipStream_t s);
int ttvk_fsq_bwd(const ttv_fsq_params* fp, const float* z, const void* dcodes, int dt, float* dz, int rows, hipStream_t s);
// part / part_bytes: optional scratch for the split partial tiles (ttvk_wgrad_ws_bytes); without it the bf16 path uses fp32 atomics
// (deterministic mode: the paths that use atomics - no or too little scratch, an unaligned operand, TTV_WGRAD_TILE64, fp32 - run with
// ONE token range per output tile instead, so that every address has a single writer)
// `batch` (optional): the split partial tiles of several weight gradients are summed by ONE launch (ttvk_wgrad_flush) instead of one
// k_wgrad_reduce per weight: the call takes its partial tiles from part + batch->used_bytes, records what to sum and returns; the
// gradients are complete only behind the flush.  A call that does not fit (more than TTV_WGRAD_BATCH entries, scratch exhausted,
// or a shape that takes another path) flushes what is pending and proceeds on its own.
#define TTV_WGRAD_BATCH 6
struct WgradBatch {
  int n = 0;
  int64_t used_bytes = 0;
  struct Entry { const float* part; float* dw; int splits, lddw, N, K, tiles_n, tiles; } e[TTV_WGRAD_BATCH];
};
int ttvk_wgrad(const void* dy, int lddy, const void* x, int ldx, float* dw, int lddw, int L, int N, int K, int dt, float* part,
               int64_t part_bytes, hipStream_t s, WgradBatch* batch = nullptr);
int ttvk_wgrad_flush(WgradBatch* batch, hipStream_t s);
int64_t ttvk_wgrad_ws_bytes(int L, int N, int K);
int ttvk_outer_small(const void* a, int a_dt, int lda, int C, const void* b, int b_dt, int ldb, const int* b_rows, float* dw, int lddw,
                     int transpose_out, int rows, int d, hipStream_t s, const DetScratch* det);
int ttvk_expand_small(const void* a, int a_dt, int lda, int C, const void* w, int w_dt, int ldw, int w_cf, void* out, int o_dt, int ldo,
                      int rows, int d, hipStream_t s);
int ttvk_reduce_small(const void* a, int a_dt, int lda, const int* a_rows, const void* w, int w_dt, int ldw, int C, float* out, int ldo,
                      int rows, int d, hipStream_t s);
// o / ldo and delta_ready apply to bf16 only (delta = rowsum(dO * O), or the caller's gate backward filled it): the fp32 checking path
// writes `delta` itself, from its own P and dP (k_attn_delta_f32_consistent), whatever the buffer held.
int ttvk_attention_bwd(const void* qkvg, int ld, const void* o, int ldo, const void* dout, int ldd, const float* lse, float* delta,
                       const int* cu, const int* blocks64, int n_blocks64, const int* row_seq, void* dqkvg, int ldg, float* dkv_scratch,
                       int total_rows, int hq, int hkv, int dt, const float* rope_cs, hipStream_t s, int delta_ready = 0, const int* qlim_desc = nullptr);
int ttvk_rope_apply_dir(void* x, int dtype, int ld, int rows, int heads, const float* cs, int conj, hipStream_t s);
int ttvk_dec_embed_ex(const void* codes, int C, const void* w, const void* bias, const float* mask_token, const float* gain, void* x,
                      int dtype, int ld, const int* rows_map, int rows, int d, float eps, void* hpre, hipStream_t s);
int ttvk_const_rows_bwd(const float* colsum, const float* mask_token, const float* gain, int dt, float eps, float* dgain, float* dmask,
                        int d, hipStream_t s);
int ttvk_rope_build(const float* base_cos, const float* base_sin, int n_ids, int F, const int* clip_desc, const int* cu, const int* row_seq,
                    float* out, int total_rows, hipStream_t s);

// ---- ttv_metrics.hip ----
// dims: n_clips x (C, T, H, W); -1 (error set) on a bad shape
int64_t ttvk_ssim_workspace_bytes(const int32_t* dims, int n_clips);
int ttvk_ssim(void* const* recon, void* const* target, const int32_t* dims, int n_clips, int dtype, int clamp, double* acc2, void* workspace,
              int64_t workspace_bytes, hipStream_t s);

// ---- ttv_crops.hip ----
int ttvk_lpips_crops_forward(void* const* recon, void* const* target, const int32_t* clip_dims, int n_clips, const int32_t* crops, int n_crops,
                             int size, void* recon_crops, void* target_crops, int dtype, hipStream_t s);
int ttvk_lpips_crops_backward(void* const* recon, void* const* grad, const int32_t* clip_dims, int n_clips, const int32_t* crops, int n_crops,
                              int size, const void* g, int dtype, hipStream_t s);

// ---- ttv_lpips.hip ----
int64_t ttvk_lpips_tape_bytes(int n, int H, int W, int dtype);
int64_t ttvk_lpips_workspace_bytes(int n, int H, int W, int dtype);
int ttvk_lpips_forward(const ttv_lpips_weights* w, const void* recon, const void* target, int n, int H, int W, int dtype, float* lpips,
                       float* gram, void* tape, void* ws, int64_t ws_bytes, hipStream_t s);
int ttvk_lpips_backward(const ttv_lpips_weights* w, const void* tape, int n, int H, int W, int dtype, const float* glpips, const float* ggram,
                        void* drecon, void* ws, int64_t ws_bytes, hipStream_t s);
int64_t ttvk_lpips_eval_workspace_bytes(int frames, int H, int W, int dtype);
int ttvk_lpips_eval_accumulate(const ttv_lpips_weights* w, void* const* recon, void* const* target, const int32_t* frames, int n_clips, int H,
                               int W, int dtype, int clamp_recon, float* per_frame, double* acc, void* ws, int64_t ws_bytes, hipStream_t s);
int64_t ttvk_lpips_conv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype);
int ttvk_lpips_conv3x3(const void* x, int N, int H, int W, int Cin, int Cout, const void* w, const float* bias, int mode, const void* h,
                       void* y, int dtype, void* ws, int64_t ws_bytes, hipStream_t s);
int ttvk_lpips_maxpool(const void* x, int N, int H, int W, int C, void* y, int dtype, hipStream_t s);
int ttvk_lpips_maxpool_backward(const void* dy, const float* add, const void* h, int N, int H, int W, int C, void* dx, int dtype, hipStream_t s);

// ---- ttv_i3d.hip ----
int64_t ttvk_i3d_workspace_bytes(int n);
int ttvk_fvd_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, int clamp, float* out, hipStream_t s);
int ttvk_i3d_features(const ttv_i3d_weights* w, const float* x, int n, float* feats, void* ws, int64_t ws_bytes, hipStream_t s);
int ttvk_i3d_conv3d(const float* x, int N, int T, int H, int W, int Cin, int k, int stride, const float* w, const float* scale,
                    const float* shift, int Cout, int relu, float* y, int ldc, int c_off, hipStream_t s);
int ttvk_i3d_maxpool3d(const float* x, int N, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw, float* y,
                       hipStream_t s);

// ---- ttv_vjepa.hip ----
int ttvk_jedi_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, void* out, hipStream_t s);
int64_t ttvk_vjepa_workspace_bytes(int n);
int ttvk_vjepa_features(const ttv_vjepa_weights* w, const void* x, int n, float* feats, int finetuned, void* ws, int64_t ws_bytes,
                        hipStream_t s);
int ttvk_vjepa_layernorm(const float* x, int ldx, int rows, int width, const float* w1, const float* b1, float eps1, const float* w2,
                         const float* b2, float eps2, float* y32, int ld32, void* y16, int ld16, hipStream_t s);
int ttvk_vjepa_linear(const void* x, int ldx, const void* w, int ldw, const void* bias, int M, int N, int K, int epilogue,
                      const float* resid, int ldr, int resid_rows, void* y, int ldy, hipStream_t s);
int ttvk_vjepa_pool_attention(const void* q, const void* kv, int n, int rows, void* out, hipStream_t s);

// ---- ttv_inception.hip ----
int64_t ttvk_inception_workspace_bytes(int n);
int ttvk_inception_preprocess(void* const* images, const int64_t* dims, int n, int dtype, int clamp, float* out, hipStream_t s);
int ttvk_inception_features(const ttv_inception_weights* w, const float* x, int n, float* acts, float* probs, void* ws, int64_t ws_bytes,
                            hipStream_t s);
int ttvk_inception_conv2d(const float* x, int N, int H, int W, int Cin, int kh, int kw, int sh, int sw, int ph, int pw, const float* w,
                          const float* scale, const float* shift, int Cout, int relu, float* y, int ldc, int c_off, hipStream_t s);
int ttvk_inception_pool2d(const float* x, int N, int H, int W, int C, int mode, float* y, int ldc, int c_off, hipStream_t s);

// ---- host helpers of the launch sequences (ttv_api.hip, ttv_train.hip, the feature extractors) ----
#define TTV_TRY(expr)                \
  do {                               \
    const int rc__ = (expr);         \
    if (rc__ != TTV_OK) return rc__; \
  } while (0)

static inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
static inline int dtype_bytes(int dt) { return dt == TTV_BF16 ? 2 : 4; }
static inline int patch_dim(const ttv_tower_dims* d) { return d->pix_channels * d->patch_t * d->patch_h * d->patch_w; }   // pixels of a patch = K of proj_in
static inline float keel_alpha(const ttv_tower_dims* d, int layer) { return layer == 0 ? 1.f : d->alpha; }             // layer 0: plain residual, no post-norm

// y[M, N] (ldy) = x[M, K] (ldx) @ w[N, K]^T (ldw); every other field zero
static inline GemmArgs gemm_args(int dtype, const void* x, int ldx, const void* w, int ldw, int M, int N, int K, void* y, int ldy) {
  GemmArgs a = {};
  a.dtype = dtype; a.x = x; a.ldx = ldx; a.w = w; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.y = y; a.ldy = ldy;
  return a;
}
// EPI_QKV_ROPE: rotary on the q columns [0, d_model) and the k columns [2 d_model, 2 d_model + gqa_dim) of (q | gate | k | v)
static inline GemmArgs gemm_rope_qk(GemmArgs a, const float* rope_cs, int d_model, int gqa_dim) {
  a.rope_cs = rope_cs; a.rope_q_end = d_model; a.rope_k_begin = 2 * d_model; a.rope_k_end = 2 * d_model + gqa_dim;
  return a;
}
// EPI_RESID_*: alpha * resid + acc
static inline GemmArgs gemm_resid(GemmArgs a, const void* resid, int ldr, float alpha) {
  a.resid = resid; a.ldr = ldr; a.alpha = alpha;
  return a;
}

// compact rows: dst[r] = src[index[r]] / dst[index[r]] = src[r], r < n_rows, both sides row_bytes apart
static inline int gather_rows(const void* src, void* dst, const int* index, int n_rows, int64_t row_bytes, hipStream_t s) {
  return ttvk_copy_rows(src, row_bytes, index, dst, row_bytes, nullptr, n_rows, (int)row_bytes, s);
}
static inline int scatter_rows(const void* src, void* dst, const int* index, int n_rows, int64_t row_bytes, hipStream_t s) {
  return ttvk_copy_rows(src, row_bytes, nullptr, dst, row_bytes, index, n_rows, (int)row_bytes, s);
}

// f(first clip, count) for every group of at most TTV_MAX_CLIPS_PER_LAUNCH clips
template <typename F> static inline int for_clip_groups(int n_clips, F f) {
  for (int c0 = 0; c0 < n_clips; c0 += TTV_MAX_CLIPS_PER_LAUNCH) {
    const int n = n_clips - c0 < TTV_MAX_CLIPS_PER_LAUNCH ? n_clips - c0 : TTV_MAX_CLIPS_PER_LAUNCH;
    TTV_TRY(f(c0, n));
  }
  return TTV_OK;
}
// patchify (scatter = false: clips -> buf [sum_patches, patch_dim]) / unpatchify (true: buf -> clips) of a tower's whole batch
static inline int patch_copy_all(bool scatter, void* const* clips, const ttv_tower_dims* d, const ttv_batch* b, void* buf, int dtype, hipStream_t s) {
  return for_clip_groups(b->n_clips, [&](int c0, int n) {
    return ttvk_patch_copy(scatter, clips + c0, b->clip_desc, c0, n, d->patch_t, d->patch_h, d->patch_w, d->pix_channels, buf, patch_dim(d), dtype,
                           b->max_patches_per_clip, s);
  });
}
