// C-ABI of libtitok_hip.so (include/titok_hip.h): argument checks, workspace carving and the launch
// sequences of the encoder / decoder towers.  Everything here only enqueues on the caller's stream.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ttv_common.h"
#include "ttv_kernels.h"

static thread_local char g_err[512] = "";

void ttv_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- measurement hook ----
int g_ttv_prof_class = 0;
// The switches that more than one site reads (declared in ttv_common.h): name and default live here, the sites cache the value.
bool ttv_sw_enc_latent_last() { static const bool v = ttv_env_flag("TTV_ENC_LATENT_LAST", true); return v; }
bool ttv_enc_latent_rows_only(const ttv_tower_dims* d, const ttv_batch* b) {
  return ttv_sw_enc_latent_last() && !(g_ttv_debug & TTV_DBG_ENC_ALL_ROWS) && d->kind == TTV_ENCODER && b->latent_rows && b->sum_tokens > 0 &&
         b->sum_tokens < b->total_rows;
}
bool ttv_sw_keel_f32sum() { static const bool v = ttv_env_flag("TTV_KEEL_F32SUM", false); return v; }
bool ttv_sw_fused_patch() { static const bool v = ttv_env_flag("TTV_FUSED_PATCH", true); return v; }
bool ttv_sw_attn_pipe() { static const bool v = ttv_env_flag("TTV_ATTN_PIPE", false); return v; }
static bool sw_dec_l0_const() { static const bool v = ttv_env_flag("TTV_DEC_L0_CONST", true); return v; }
static bool sw_enc_last_qkv_skip() { static const bool v = ttv_env_flag("TTV_ENC_LAST_QKV_SKIP", true); return v; }
float ttv_sw_attn_thr() { static const float v = ttv_env_float("TTV_ATTN_THR", 8.0f); return v; }   // log2 units; 0 = exact running maximum
// deterministic mode: process-wide (not per thread: a training step's launches come from whichever thread runs it), read at launch time
static int g_ttv_det = 0;
bool ttv_det() { return __atomic_load_n(&g_ttv_det, __ATOMIC_RELAXED) != 0; }
thread_local int g_ttv_debug = 0;     // per host thread: a thread that forces a kernel variant (tests, A/B tools) does not change what another thread launches
long long* g_ttv_stamps = nullptr;   // diagnostics: device buffer for in-kernel clock stamps (ttv_debug_stamps)
static hipEvent_t* g_prof_start = nullptr;
static hipEvent_t* g_prof_stop = nullptr;
static int g_prof_cap = 0, g_prof_n = 0;

TtvProfScope::TtvProfScope(int cls, hipStream_t stream) : slot(-1), s(stream) {
  if (g_ttv_prof_class != 0 && cls == g_ttv_prof_class && g_prof_n < g_prof_cap) {
    slot = g_prof_n++;
    (void)hipEventRecord(g_prof_start[slot], s);
  }
}
TtvProfScope::~TtvProfScope() {
  if (slot >= 0) (void)hipEventRecord(g_prof_stop[slot], s);
}

struct TowerWs {
  char *x, *xn, *qkv, *ao, *h, *pa, *pb;
  char *xl, *aol;    // [sum_tokens, width]: the latent rows of x and of the attention output, compact (encoder, last layer)
  char *f8, *f8mx;   // block-scaled fp8 image of the running linear's input [L, max(width, inner)] and its E8M0 scales
  float* y32;
  float* rstd;     // [L] row statistic of a folded pre-norm (generic-width bf16 towers)
  int64_t total;
};

static TowerWs carve(const ttv_tower_dims* d, const ttv_batch* b, char* base) {
  const int64_t e = dtype_bytes(d->dtype);
  const int64_t L = b->total_rows, P = b->sum_patches;
  const int64_t g = (int64_t)d->kv_heads * d->head_dim;
  const int64_t pd = patch_dim(d);
  int64_t off = 0;
  TowerWs w;
  auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  w.x = take(L * d->width * e);
  w.xn = take(L * d->width * e);
  w.qkv = take(L * (2 * d->width + 2 * g) * e);
  w.ao = take(L * d->width * e);
  w.y32 = (float*)take(L * d->width * 4);
  w.h = take(L * d->inner * e);
  w.pa = take(P * pd * e);        // encoder: gathered patches; decoder: proj_out output
  w.pb = take(P * d->width * e);  // encoder: proj_in output;   decoder: ln_post output
  w.rstd = (float*)take(L * 4);
  w.xl = take((int64_t)b->sum_tokens * d->width * e);
  w.aol = take((int64_t)b->sum_tokens * d->width * e);
  w.f8 = w.f8mx = nullptr;
  if (d->dtype == TTV_BF16 && d->width != 256 && d->width % 128 == 0) {      // the towers that can run the block-scaled fp8 linears
    const int64_t wide = d->width > d->inner ? d->width : d->inner;
    w.f8 = take(L * wide);
    w.f8mx = take(L * (wide / 128 + 4) * 4);
  }
  w.total = off;
  return w;
}

static int check_dims(const ttv_tower_dims* d, const ttv_batch* b) {
  TTV_CHECK_ARG(d && b, "null dims/batch");
  TTV_CHECK_ARG(d->dtype == TTV_BF16 || d->dtype == TTV_F32, "bad dtype %d", d->dtype);
  TTV_CHECK_ARG(d->head_dim == 64 && d->width == d->q_heads * 64, "width must be q_heads*64");
  TTV_CHECK_ARG(d->width % 64 == 0 && d->width <= 1024, "width %d unsupported", d->width);
  TTV_CHECK_ARG(d->inner % 32 == 0, "GEGLU inner dim must be a multiple of 32");
  TTV_CHECK_ARG(d->token_size >= 1 && d->token_size <= TTV_MAX_TOKEN, "token_size out of range");
  TTV_CHECK_ARG(((int64_t)d->pix_channels * d->patch_t * d->patch_h * d->patch_w) % 8 == 0, "patch vector length must be a multiple of 8");
  TTV_CHECK_ARG(b->n_clips > 0 && b->total_rows == b->sum_tokens + b->sum_patches, "inconsistent batch");
  return TTV_OK;
}

// What run_layers decides once per call and the helpers below read.
struct LayerCtx {
  const ttv_tower_dims* d; const ttv_batch* b; const TowerWs& ws; hipStream_t s;
  int split3, s3img;   // fp32 tower on the three-pass bf16 kernels / its activations travel as split images
  bool gen_ok;         // a folded pre-norm may take its row statistic as the GEMM's row scale (wide bf16 towers, split-bf16 towers)
  int pair, all_full, pipe;   // TTV_ATTN_PAIRED / _ALLFULL / _PIPE where the batch's own table (pair, all_full) or the switch (pipe) says so, else 0
  bool pv8;            // ttv_tower_weights.attn_pv8: every attention of the tower is ttvk_quant_v_pv8 + ttvk_attention_pv8
};

// The towers' attention: ws.qkv -> ws.ao over one work table.  The gate, the q pre-scale and the split-bf16 formats are the same at
// every site; `site` holds the TTV_ATTN_PAIRED / _ALLFULL / _PIPE bits that this table and this site may take (see the callers).
static int tower_attention(const LayerCtx& c, bool q_scaled, const int32_t* table, int n_table, int site) {
  const ttv_tower_dims* d = c.d;
  if (c.pv8) {
    // e4m3 P.V (opt-in): the image of this layer's v columns goes into the GEGLU buffer, which nobody reads before the w12 GEMM writes
    // it again; the table is walked entry by entry whatever `site` says about it
    const ttv_batch* b = c.b;
    const int nq = 2 * d->width + 2 * d->kv_heads * d->head_dim;
    TTV_CHECK_ARG(q_scaled, "attn_pv8: a layer's q is not pre-scaled (pack the towers with qkv_q_prescaled / to_qkv_qs)");
    TTV_CHECK_ARG(ttvk_attention_pv8_bytes(b->total_rows, b->n_clips, d->kv_heads) <= (int64_t)b->total_rows * d->inner * dtype_bytes(d->dtype),
                  "attn_pv8: the V image (%lld bytes) does not fit the workspace's GEGLU buffer", (long long)ttvk_attention_pv8_bytes(b->total_rows, b->n_clips, d->kv_heads));
    TTV_TRY(ttvk_quant_v_pv8(c.ws.qkv, nq, b->cu_seqlens, b->n_clips, b->total_rows, d->q_heads, d->kv_heads, c.ws.h, c.s));
    return ttvk_attention_pv8(c.ws.qkv, nq, c.ws.ao, d->width, b->cu_seqlens, table, n_table, d->q_heads, d->kv_heads, d->head_dim,
                              TTV_ATTN_GATE | TTV_ATTN_QSCALED, c.ws.h, c.s);
  }
  const int flags = TTV_ATTN_GATE | (q_scaled ? TTV_ATTN_QSCALED : 0) | (c.split3 ? TTV_ATTN_SPLIT3 : 0) |
                    (c.s3img ? (TTV_ATTN_SPLIT_OUT | TTV_ATTN_SPLIT_IN) : 0) | site;
  return ttvk_attention(c.ws.qkv, 2 * d->width + 2 * d->kv_heads * d->head_dim, c.ws.ao, d->width, c.b->cu_seqlens, table, n_table, d->q_heads,
                        d->kv_heads, d->head_dim, flags, d->dtype, c.s);
}

// One layer with all four linears on the block-scaled fp8 MFMA (BASELINE config #5; ttv_layer_weights.to_qkv_mx ...): every linear's
// input is quantised by k_quant_mx_fp8, the pre-norm gains live in the weight images and the rstd of the pre-norm is the activation's
// per-row factor in the GEMM epilogue; attention, the KEEL sums and norms stay bf16 / fp32 as in the bf16 tower.
static int run_layer_mx(const LayerCtx& c, const ttv_layer_weights& lw, int i, bool& rstd_valid, bool& xq_valid) {
  const ttv_tower_dims* d = c.d;
  const ttv_batch* b = c.b;
  const TowerWs& ws = c.ws;
  hipStream_t s = c.s;
  const int L = b->total_rows, dm = d->width, g = d->kv_heads * d->head_dim, dt = d->dtype, nq = 2 * dm + 2 * g, I = d->inner;
  const float alpha = keel_alpha(d, i);
  // Quantisation is fused into the producers where the producer owns whole 32-element blocks (TTV_MX_FUSED_QUANT=0: every operand by a
  // pass of its own, A/B): the KEEL post-norm kernel writes x also as its block-scaled image (ws.f8 / ws.f8mx), the w12 GEMM's GEGLU
  // epilogue writes h only as its image (into the bf16 h buffer and the xn buffer, both unused in this mode).  Left as passes: the
  // attention output (its kernel is untouched) and layer 0's two inputs (no norm kernel in front of them).
  static const bool fused_env = ttv_env_flag("TTV_MX_FUSED_QUANT", true);
  const bool fused_q = fused_env && !(g_ttv_debug & TTV_DBG_MX_UNFUSED_QUANT);      // ttv_debug_set bit 11: the unfused sequence (tests: both must agree bit for bit)
  if (!rstd_valid) TTV_TRY(ttvk_row_rstd(ws.x, dt, dm, ws.rstd, L, dm, d->eps, s));
  if (!xq_valid) TTV_TRY(ttvk_quant_mx_fp8(ws.x, dt, dm, ws.f8, dm, ws.f8mx, nullptr, L, dm, s));
  xq_valid = false;
  const GemmArgs a = gemm_rope_qk(gemm_args(dt, ws.f8, dm, lw.to_qkv_f8, dm, L, nq, dm, ws.qkv, nq), b->rope_cs, dm, g);
  TTV_TRY(ttvk_gemm_fp8(EPI_QKV_ROPE, a, ws.rstd, lw.to_qkv_f8_scale, s, ws.f8mx, lw.to_qkv_mx));
  const bool q_scaled = lw.qkv_q_prescaled != 0;
  if (fused_q && q_scaled && !c.pair && !c.pipe && d->head_dim == 64 && !c.pv8) {
    // the attention epilogue writes out_proj's operand itself (no bf16 output, no pass over it); ws.f8 is free: the qkv GEMM has read it
    TTV_TRY(ttvk_attention_mxout(ws.qkv, nq, ws.f8, ws.f8mx, (int)ttvk_mx_scale_ld(dm), b->cu_seqlens, b->qblocks, b->n_qblocks, d->q_heads,
                                 d->kv_heads, s));
  } else {
    // (no TTV_ATTN_ALLFULL unless the pipelined kernel is asked for: this is the A/B twin of the attention kernel with the fused MX
    // epilogue above, which is k_attn_bf16 - the two must produce the same bits, tested)
    TTV_TRY(tower_attention(c, q_scaled, b->qblocks, b->n_qblocks, c.pair | (c.pipe ? c.all_full | c.pipe : 0)));
    TTV_TRY(ttvk_quant_mx_fp8(ws.ao, dt, dm, ws.f8, dm, ws.f8mx, nullptr, L, dm, s));
  }
  const GemmArgs o = gemm_resid(gemm_args(dt, ws.f8, dm, lw.out_proj_f8, dm, L, dm, dm, ws.x, dm), ws.x, dm, alpha);
  TTV_TRY(ttvk_gemm_fp8(EPI_RESID_T, o, nullptr, lw.out_proj_f8_scale, s, ws.f8mx, lw.out_proj_mx));
  if (i > 0) {
    TTV_TRY(ttvk_rmsnorm(ws.x, dt, dm, nullptr, ws.x, dt, dm, nullptr, lw.attn_post_ln, L, dm, d->eps, s, ws.rstd, fused_q ? ws.f8 : nullptr,
                         fused_q ? ws.f8mx : nullptr));
    if (!fused_q) TTV_TRY(ttvk_quant_mx_fp8(ws.x, dt, dm, ws.f8, dm, ws.f8mx, nullptr, L, dm, s));
  } else {
    TTV_TRY(ttvk_row_rstd(ws.x, dt, dm, ws.rstd, L, dm, d->eps, s));
    TTV_TRY(ttvk_quant_mx_fp8(ws.x, dt, dm, ws.f8, dm, ws.f8mx, nullptr, L, dm, s));
  }
  GemmArgs f = gemm_args(dt, ws.f8, dm, lw.w12_f8, dm, L, I, dm, ws.h, I);
  char* const hq = ws.h;          // fp8 image of h [L, I] in the bf16 h buffer; its scales in the xn buffer (L * dm * 2 bytes >= L * 4 * nkp(I))
  char* const hq_mx = ws.xn;
  const bool h_fused = fused_q && (int64_t)ttvk_mx_scale_ld(I) <= (int64_t)dm * 2;
  if (h_fused) { f.yq = hq; f.yq_mx = hq_mx; }
  TTV_TRY(ttvk_gemm_fp8(EPI_GEGLU, f, ws.rstd, lw.w12_f8_scale, s, ws.f8mx, lw.w12_mx));
  if (!h_fused) TTV_TRY(ttvk_quant_mx_fp8(ws.h, dt, I, ws.f8, I, ws.f8mx, nullptr, L, I, s));
  const GemmArgs f3 = gemm_resid(gemm_args(dt, h_fused ? hq : ws.f8, I, lw.w3_f8, I, L, dm, I, ws.x, dm), ws.x, dm, alpha);
  TTV_TRY(ttvk_gemm_fp8(EPI_RESID_T, f3, nullptr, lw.w3_f8_scale, s, h_fused ? hq_mx : ws.f8mx, lw.w3_mx));
  rstd_valid = false;
  if (i > 0) {
    // the next layer's to_qkv operand rides along (the caller only uses it when the next layer runs this path too)
    TTV_TRY(ttvk_rmsnorm(ws.x, dt, dm, nullptr, ws.x, dt, dm, nullptr, lw.ffd_post_ln, L, dm, d->eps, s, ws.rstd, fused_q ? ws.f8 : nullptr,
                         fused_q ? ws.f8mx : nullptr));
    rstd_valid = true;
    xq_valid = fused_q;
  }
  return TTV_OK;
}

// Does a linear of the generic layer path run on the row-scaled e4m3 image (round 2's mixed bf16 / fp8 mode)?  Only when the image IS
// row-scaled: `mx` set means the pointers hold the block-scaled image of W * gain, which the row-scaled GEMM would mis-read (gain applied
// twice, block scales dropped).
static bool rows_f8(int dt, int dm, const void* img, const void* row_scale, const void* mx, const void* folded) {
  return dt == TTV_BF16 && img && row_scale && !mx && dm % 128 == 0 && !(dm == 256 && folded);
}

// A pre-normed projection's weight in every form a tower may carry: plain, with the pre-norm gain folded in (NULL: not packed),
// and the row-scaled e4m3 image (f8: use it, see rows_f8).
struct PreNormW { const float* gain; const void *w, *w_pn, *w_f8; const float* w_f8_scale; bool f8; };

// y[rows, N] = epilogue(RMSNorm(x) * gain @ W^T): to_qkv (EPI_QKV_ROPE) and w12 (EPI_GEGLU).  Routes: the row-scaled fp8 image (mixed
// bf16 / fp8, config #5: the pre-norm output is quantised to e4m3 per token into the xn buffer - L x dm bytes of values, then L fp32
// scales - and the projection runs on the fp8 MFMA); the width-256 kernel's folded pre-norm; other widths with the gain folded into
// the weight as well (w_pn) and the row statistic - from the kernel that produced x (rstd_valid) or from one light pass - multiplying
// the GEMM's output rows, so no stand-alone RMSNorm launch and no normalised copy of x; else RMSNorm into xn, then the plain weight.
// Split-bf16 towers: the normalised row is written as the projection's split image (its producer splits it once, the GEMM's staging
// threads copy bytes); TTV_SPLIT3_IMAGES=0 keeps fp32 activations and the split in the GEMM (A/B).
static int prenorm_proj(const LayerCtx& c, GemmEpilogue epi, const char* x, int rows, const PreNormW& p, int N, char* y, int y_image,
                        bool rstd_valid, int tile_run = 0, int tile_period = 0, int panel_lo = 0) {
  const ttv_tower_dims* d = c.d;
  const TowerWs& ws = c.ws;
  const int dm = d->width, dt = d->dtype;
  GemmArgs a = gemm_args(dt, nullptr, dm, nullptr, dm, rows, N, dm, y, N);       // operand and weight: by route
  if (epi == EPI_QKV_ROPE) a = gemm_rope_qk(a, c.b->rope_cs, dm, d->kv_heads * d->head_dim);
  if (p.f8) {
    float* const f8_scales = reinterpret_cast<float*>(ws.xn + align256((int64_t)c.b->total_rows * dm));
    TTV_TRY(ttvk_quant_rows_fp8(x, dt, dm, p.gain, d->eps, ws.xn, dm, f8_scales, rows, dm, c.s));
    a.x = ws.xn; a.w = p.w_f8;
    return ttvk_gemm_fp8(epi, a, f8_scales, p.w_f8_scale, c.s);
  }
  const bool fold256 = dt == TTV_BF16 && dm == 256 && p.w_pn;
  const bool fold_gen = c.gen_ok && p.w_pn;
  const bool fold = fold256 || fold_gen;
  if (fold_gen && !rstd_valid) TTV_TRY(ttvk_row_rstd(x, dt, dm, ws.rstd, rows, dm, d->eps, c.s));
  if (!fold) TTV_TRY(ttvk_rmsnorm(x, dt, dm, nullptr, ws.xn, dt, dm, nullptr, p.gain, rows, dm, d->eps, c.s, nullptr, nullptr, nullptr, c.s3img));
  a.split3 = c.split3; a.x_image = c.s3img && !fold; a.y_image = y_image;
  a.prenorm = fold256; a.eps = d->eps;
  a.row_scale = fold_gen ? ws.rstd : nullptr;
  a.x = fold ? x : ws.xn; a.w = fold ? p.w_pn : p.w;
  if (epi == EPI_QKV_ROPE) { a.rope_ids = c.b->rope_ids; a.rope_base = c.b->rope_ids ? c.b->rope_base : nullptr; }
  a.tile_run = tile_run; a.tile_period = tile_period; a.panel_lo = panel_lo;      // (the caller has asked ttvk_gemm_qkv_tiles_supported)
  return ttvk_gemm(epi, a, c.s);
}

// The tail of a KEEL sub-layer (out_proj and w3): x <- RMSNorm(alpha * x + in @ W^T) * gain, in place on the rows of cx = o.y; layer 0
// has no norm and alpha = 1.  `o` arrives with operand, weight, shapes and the output cx; the residual (cx again) and alpha are set
// here.  Width 256 does it in one kernel (EPI_RESID_NORM; in place is safe: a token row is read as residual and written by the same
// wave only).  Wide towers: the sum leaves the GEMM through HBM and a row kernel normalises it.  bf16 towers store it in the compute dtype, in place on x (a token row element
// is read as residual and written by the same lane) - the reference's autocast rounds that sum to bf16 as well (transformer.py:141:
// bf16 * alpha + bf16) -: half the bytes of the fp32 buffer on both kernels.  fp32 towers, and TTV_KEEL_F32SUM=1 (A/B), keep the fp32
// buffer.  want_rstd: the row kernel also leaves the statistic of the row it wrote in ws.rstd, for a folded pre-norm behind it;
// rstd_valid is set to it on that route and left alone on the others.
static int keel_tail(const LayerCtx& c, GemmArgs o, int layer, const float* post_gain, bool want_rstd, bool& rstd_valid) {
  const ttv_tower_dims* d = c.d;
  const int dm = d->width, dt = d->dtype;
  char* const cx = (char*)o.y;
  o = gemm_resid(o, cx, dm, keel_alpha(d, layer));
  o.split3 = c.split3; o.x_image = c.s3img;
  if (layer == 0) return ttvk_gemm(EPI_RESID_T, o, c.s);
  if (ttvk_gemm_supports_resid_norm(dt, dm, o.K)) {
    o.norm_gain = post_gain; o.eps = d->eps;
    return ttvk_gemm(EPI_RESID_NORM, o, c.s);
  }
  float* const next_rstd = want_rstd ? c.ws.rstd : nullptr;
  if (dt == TTV_BF16 && !ttv_sw_keel_f32sum()) {
    TTV_TRY(ttvk_gemm(EPI_RESID_T, o, c.s));
    TTV_TRY(ttvk_rmsnorm(cx, dt, dm, nullptr, cx, dt, dm, nullptr, post_gain, o.M, dm, d->eps, c.s, next_rstd));
  } else {
    o.y = c.ws.y32;
    TTV_TRY(ttvk_gemm(EPI_RESID_F32, o, c.s));
    TTV_TRY(ttvk_rmsnorm(c.ws.y32, TTV_F32, dm, nullptr, cx, dt, dm, nullptr, post_gain, o.M, dm, d->eps, c.s, next_rstd));
  }
  rstd_valid = want_rstd;
  return TTV_OK;
}

// Can a to_qkv of this tower run k_qkv256 over a tile list that tells latent token tiles from patch token tiles?  Every clip K latent rows
// and P patch rows (the caller's promise; the sums are checked), both multiples of the kernel's 128-row tiles, and the layer on the
// width-256 bf16 kernel with the folded pre-norm and pre-scaled q.
static bool qkv_tile_list_ok(const LayerCtx& c, const ttv_layer_weights& lw, int K, int P) {
  const ttv_tower_dims* d = c.d;
  const ttv_batch* b = c.b;
  if (d->dtype != TTV_BF16 || d->width != 256 || d->head_dim != 64 || c.split3) return false;
  if (K <= 0 || P <= 0 || K % 128 || P % 128 || (int64_t)b->n_clips * K != b->sum_tokens || (int64_t)b->n_clips * P != b->sum_patches) return false;
  if (!lw.to_qkv_pn || !lw.qkv_q_prescaled) return false;
  return ttvk_gemm_qkv_tiles_supported(d->width, d->kv_heads * d->head_dim, d->width);
}

// One ResidualAttentionBlock stack (reference transformer.py:126-146) on ws.x in place.
// Can the decoder's layer 0 take its patch rows' q | gate | k | v from the constant block (ttv_dec_l0_const)?  The block's geometry must
// be every clip's (the caller's promise; the sums are checked), rows and keys split at a multiple of the 128-row tiles of both kernels,
// and layer 0 must run the two kernels that know about it: k_qkv256 with the folded pre-norm and k_attn_swp over the batch's own table.
static bool dec_l0_const_ok(const LayerCtx& c, const ttv_tower_weights* w, const ttv_dec_l0_const* l0) {
  const ttv_tower_dims* d = c.d;
  const ttv_batch* b = c.b;
  if (!l0 || !l0->rows || !sw_dec_l0_const() || (g_ttv_debug & TTV_DBG_DEC_L0_NO_CONST)) return false;
  if (d->kind != TTV_DECODER || !qkv_tile_list_ok(c, w->layers[0], l0->latent_rows, l0->patch_rows)) return false;
  if (c.pair || c.pipe || c.pv8 || !c.all_full || (b->items64 && b->n_items64 > 0)) return false;
  return ttvk_attention_takes_swp(TTV_ATTN_GATE | TTV_ATTN_QSCALED | TTV_ATTN_ALLFULL);
}

// The encoder's last layer under lat_last queries its latent rows only: may its to_qkv skip the q | gate panels of the patch token tiles
// (GemmArgs.panel_lo)?  The batch must promise one geometry for every clip (ttv_batch.tokens_per_clip; max_patches_per_clip then IS every
// clip's P once the sums agree).  TTV_ENC_LAST_QKV_SKIP=0 / debug bit 23: every panel of every row (A/B, tests).
static bool enc_last_qkv_skip_ok(const LayerCtx& c, const ttv_layer_weights& lw) {
  const ttv_batch* b = c.b;
  if (!sw_enc_last_qkv_skip() || (g_ttv_debug & TTV_DBG_ENC_LAST_QKV_ALL) || c.d->kind != TTV_ENCODER) return false;
  return qkv_tile_list_ok(c, lw, b->tokens_per_clip, b->max_patches_per_clip);
}

static int run_layers(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const TowerWs& ws, hipStream_t s,
                      const ttv_dec_l0_const* l0 = nullptr) {
  const int L = b->total_rows, dm = d->width, g = d->kv_heads * d->head_dim, dt = d->dtype;
  const int split3 = (dt == TTV_F32 && w->f32_split3) ? 1 : 0;       // fp32 towers on the three-pass bf16 kernels (ttv_tower_weights.f32_split3)
  // pre-norm gains folded into the weight (to_qkv_pn / w12_pn) with the row statistic applied to the GEMM's output rows: the wide bf16
  // towers, and the split-bf16 towers of any width (their weights are repacked anyway; the exact-fp32 towers keep the reference's order)
  const bool gen_ok = (dt == TTV_BF16 && dm != 256) || split3;
  static const bool s3img_env = ttv_env_flag("TTV_SPLIT3_IMAGES", true);
  const int s3img = (split3 && s3img_env && !(g_ttv_debug & TTV_DBG_SPLIT3_NO_IMAGES)) ? 1 : 0;     // ttv_debug_set bit 12: fp32 activations, split inside the GEMMs (tests)
  const int nq = 2 * dm + 2 * g;
  const int64_t row_bytes = (int64_t)dm * dtype_bytes(dt);       // a split image (hi0..3 | lo0..3 per 16 bytes) has the bytes of the fp32 row
  bool qkv_ready = false;   // the previous layer's tail kernel already produced this layer's rotated qkv
  bool rstd_valid = false;  // ws.rstd holds rsqrt(mean(x^2) + eps) of the current ws.x (written by the kernel that produced x)
  bool xq_valid = false;    // ws.f8 / ws.f8mx hold the block-scaled e4m3 image of the current ws.x (run_layer_mx)
  // The encoder's output is its latent rows (blocks.py:101-103): with the batch's latent-query table the LAST layer runs its attention for
  // those query rows only and everything behind the attention on the sum K_b latent rows, gathered into compact buffers (ws.xl, ws.aol) and
  // scattered back into ws.x at the end.  Row-wise kernels on other rows: the values of the rows that are read are the same bits.
  // TTV_ENC_LATENT_LAST=0: every row, as the reference computes it (A/B, tests).  Not for the block-scaled fp8 layers (run_layer_mx).
  const bool lat_last = ttv_enc_latent_rows_only(d, b) && b->qblocks_latent && b->n_qblocks_latent > 0;
  // The decoder's output is its patch rows (blocks.py:171): with the batch's patch-query table the LAST layer's attention skips the query
  // blocks that hold latent rows only.  Their rows of ws.ao keep the previous layer's values (finite), everything behind the attention
  // is row-wise, the tail gathers patch rows: no patch row changes a bit.  TTV_DEC_PATCH_LAST=0 / debug bit 21: every block (A/B, tests).
  static const bool pat_env = ttv_env_flag("TTV_DEC_PATCH_LAST", true);
  const bool pat_last = pat_env && !(g_ttv_debug & TTV_DBG_DEC_ALL_BLOCKS) && d->kind == TTV_DECODER && d->layers >= 2 && b->qblocks_patch &&
                        b->n_qblocks_patch > 0 && !split3 && !b->qblocks_paired;
  bool compacted = false;
  const bool pv8 = w->attn_pv8 != 0;       // opt-in e4m3 P.V (ttv_tower_weights.attn_pv8)
  TTV_CHECK_ARG(!pv8 || (dt == TTV_BF16 && !split3), "attn_pv8 is a bf16 inference option (not for fp32 or split-bf16 towers)");
  const LayerCtx ctx = {d, b, ws, s, split3, s3img, gen_ok, b->qblocks_paired ? TTV_ATTN_PAIRED : 0, b->qblocks_all_full ? TTV_ATTN_ALLFULL : 0,
                        ttv_sw_attn_pipe() ? TTV_ATTN_PIPE : 0, pv8};       // (pipe: the opt-in pipelined attention kernel)
  // The decoder's patch rows enter layer 0 as one constant vector (blocks.py:165-167), so their q | gate | k | v depend on the weights
  // and the rows' positions only: with the block built for this (weight pack, clip geometry) layer 0's to_qkv computes the token tiles
  // that hold latent rows and its attention reads the patch rows from the block - one copy for every clip, L2-resident - instead of
  // from ws.qkv; with the block's state a patch query block loops over the latent keys only and adds the cached sums over the patch keys
  // (latent query rows keep their bits, patch query rows differ by one fp32 re-association).  TTV_DEC_L0_CONST=0 / debug bit
  // 22: every row and key recomputed (A/B, tests).
  const bool l0_const = dec_l0_const_ok(ctx, w, l0);
  for (int i = 0; i < d->layers; ++i) {
    const ttv_layer_weights& lw = w->layers[i];
    const bool last = i == d->layers - 1;
    const bool l0c = l0_const && i == 0;
    if (dt == TTV_BF16 && dm != 256 && dm % 128 == 0 && d->inner % 128 == 0 && !ttv_sw_keel_f32sum() && lw.to_qkv_f8 && lw.to_qkv_mx && lw.w12_f8 &&
        lw.w12_mx && lw.out_proj_f8 && lw.out_proj_mx && lw.w3_f8 && lw.w3_mx &&
        !(lat_last && last)) {    // the encoder's last layer: its latent rows on the bf16 kernels instead (a ninth of the rows)
      TTV_TRY(run_layer_mx(ctx, lw, i, rstd_valid, xq_valid));
      qkv_ready = false;
      continue;
    }
    xq_valid = false;
    // ---- attention sub-layer (transformer.py:85-104) ----
    // mixed bf16 / fp8 (config #5): to_qkv and w12 run on the row-scaled fp8 image (prenorm_proj); everything downstream is unchanged.
    // NOT when the images are the block-scaled ones (to_qkv_mx / w12_mx set: e4m3 of W * gain divided by the row factor AND the per-32
    // E8M0 scales, which only run_layer_mx's GEMMs undo): a layer of an MX tower that lands here - the encoder's latent-only last layer,
    // every layer under TTV_KEEL_F32SUM=1 - runs its projections on the bf16 kernels from the folded weights
    const bool f8_qkv = rows_f8(dt, dm, lw.to_qkv_f8, lw.to_qkv_f8_scale, lw.to_qkv_mx, lw.to_qkv_pn);
    const bool f8_w12 = rows_f8(dt, dm, lw.w12_f8, lw.w12_f8_scale, lw.w12_mx, lw.w12_pn);
    if (!qkv_ready) {
      const void* w_plain = (dt == TTV_BF16 && lw.to_qkv_qs) ? lw.to_qkv_qs : lw.to_qkv;   // inference copy with scaled q rows, if packed
      const PreNormW qw = {lw.pre_ln, w_plain, lw.to_qkv_pn, lw.to_qkv_f8, lw.to_qkv_f8_scale, f8_qkv};
      if (l0c) TTV_TRY(prenorm_proj(ctx, EPI_QKV_ROPE, ws.x, L, qw, nq, ws.qkv, 0, rstd_valid, l0->latent_rows / 128, (l0->latent_rows + l0->patch_rows) / 128));
      else if (lat_last && last && !f8_qkv && enc_last_qkv_skip_ok(ctx, lw))
        // q | gate (the first 2 dm columns) for the latent token tiles only: the attention below reads those rows' queries and nothing else
        TTV_TRY(prenorm_proj(ctx, EPI_QKV_ROPE, ws.x, L, qw, nq, ws.qkv, 0, rstd_valid, b->tokens_per_clip / 128,
                             (b->tokens_per_clip + b->max_patches_per_clip) / 128, 2 * dm / 64));
      else TTV_TRY(prenorm_proj(ctx, EPI_QKV_ROPE, ws.x, L, qw, nq, ws.qkv, s3img ? 2 : 0, rstd_valid));
    }
    // q arrives pre-scaled when the projection used the folded weight whose q rows carry scale * log2(e)
    const bool q_scaled = dt == TTV_BF16 && (lw.to_qkv_pn ? lw.qkv_q_prescaled != 0 : lw.to_qkv_qs != nullptr);
    rstd_valid = false;
    qkv_ready = false;
    const bool lat_now = lat_last && last;
    if (lat_now)
      // never paired, never pipelined.  The latent table holds full items only; it is declared so only when the batch's own table is too:
      // ttvk_attention picks its kernel by that flag, and the latent-rows forward must run the kernel the all-rows forward runs - same
      // bits, tested
      TTV_TRY(tower_attention(ctx, q_scaled, b->qblocks_latent, b->n_qblocks_latent, ctx.all_full));
    else if (l0c) {
      TtvProfScope prof(TTV_KC_ATTENTION, s);
      // (the block's own table, when given: the latent query blocks - every key - in front of the patch blocks, which now loop over the
      // latent keys only)
      const bool own = l0->qblocks && l0->n_qblocks > 0;
      TTV_TRY(ttvk_attention_swp(ws.qkv, nq, ws.ao, dm, b->cu_seqlens, own ? l0->qblocks : b->qblocks, own ? l0->n_qblocks : b->n_qblocks, d->q_heads,
                                 d->kv_heads, 1, s, l0->rows, l0->latent_rows, l0->state));
    } else if (pat_last && last && dt == TTV_BF16 && !ctx.pipe)     // (pat_last: the batch's table is unpaired)
      TTV_TRY(tower_attention(ctx, q_scaled, b->qblocks_patch, b->n_qblocks_patch, ctx.all_full));
    else if (q_scaled && b->items64 && b->n_items64 > 0 && d->head_dim == 64 && !pv8)
      TTV_TRY(ttvk_attention64(ws.qkv, nq, ws.ao, dm, b->cu_seqlens, b->items64, b->n_items64, d->q_heads, d->kv_heads,
                               TTV_ATTN_GATE | TTV_ATTN_QSCALED, s));
    else
      TTV_TRY(tower_attention(ctx, q_scaled, b->qblocks, b->n_qblocks, ctx.pair | ctx.all_full | ctx.pipe));
    // from here on the layer works on (cx, cao, Lc): the whole packed batch, or - last encoder layer - its latent rows, compact
    char* cx = ws.x;
    char* cao = ws.ao;
    int Lc = L;
    if (lat_now) {
      TTV_TRY(gather_rows(ws.x, ws.xl, b->latent_rows, b->sum_tokens, row_bytes, s));
      TTV_TRY(gather_rows(ws.ao, ws.aol, b->latent_rows, b->sum_tokens, row_bytes, s));
      cx = ws.xl; cao = ws.aol; Lc = b->sum_tokens;
      compacted = true;
    }
    // TTV_FUSED_MLP=0 selects the unfused kernel sequence (A/B measurements; same results up to bf16 rounding of h).
    // TTV_FUSED_QKV=1 additionally folds the NEXT layer's QKV projection + rotary into the tail kernel: correct and tested,
    // but measured 3 % slower end to end than the stand-alone QKV kernel (the phase runs on the 192 CUs / uneven wave pairs
    // of the tail kernel: 31 us against 35 us stand-alone in isolation, worse in the pipeline), so it is opt-in.
    static const bool use_fused_mlp = ttv_env_flag("TTV_FUSED_MLP", true);
    static const bool use_fused_qkv = ttv_env_flag("TTV_FUSED_QKV", false);
    const float alpha = keel_alpha(d, i);
    if (use_fused_mlp && ttvk_mlp_fused_supported(dt, dm, d->inner) && lw.mlp_pack) {
      // one kernel for the rest of the layer: out_proj + residual/KEEL norm, then pre-norm + w12 + GEGLU + w3 +
      // residual/KEEL norm, in place on x, and (when the pack carries it) the NEXT layer's pre_ln + to_qkv + rotary
      MlpNextQkv nx = {};
      const bool back = use_fused_qkv && !last && lw.mlp_pack_qkv_rows == nq && nq % 64 == 0 && dm % 64 == 0 && g % 64 == 0;
      if (back) { nx.qkv = ws.qkv; nx.ld = nq; nx.rope_cs = b->rope_cs; nx.rows = nq; nx.rope_q_end = dm; nx.rope_k_begin = 2 * dm; nx.rope_k_end = 2 * dm + g; }
      TTV_TRY(ttvk_mlp_fused(cao, dm, i == 0 ? nullptr : lw.attn_post_ln, alpha, cx, dm, lw.mlp_pack, d->inner, cx, dm, i == 0 ? nullptr : lw.ffd_post_ln,
                             alpha, d->eps, Lc, back ? &nx : nullptr, s));
      qkv_ready = back;
      continue;
    }
    TTV_TRY(keel_tail(ctx, gemm_args(dt, cao, dm, lw.out_proj, dm, Lc, dm, dm, cx, dm), i, lw.attn_post_ln, gen_ok && lw.w12_pn && !f8_w12, rstd_valid));
    // ---- GEGLU sub-layer (transformer.py:47-56) ----
    const PreNormW fw = {lw.ffd_norm, lw.w12, lw.w12_pn, lw.w12_f8, lw.w12_f8_scale, f8_w12};
    TTV_TRY(prenorm_proj(ctx, EPI_GEGLU, cx, Lc, fw, d->inner, ws.h, s3img, rstd_valid));
    rstd_valid = false;
    // the next layer's to_qkv takes the row statistic when it runs with the folded weight on the bf16 kernels
    const ttv_layer_weights* nl = last ? nullptr : &w->layers[i + 1];
    const bool next_rstd = gen_ok && nl && nl->to_qkv_pn && !rows_f8(dt, dm, nl->to_qkv_f8, nl->to_qkv_f8_scale, nl->to_qkv_mx, nl->to_qkv_pn);
    TTV_TRY(keel_tail(ctx, gemm_args(dt, ws.h, d->inner, lw.w3, d->inner, Lc, dm, d->inner, cx, dm), i, lw.ffd_post_ln, next_rstd, rstd_valid));
  }
  if (compacted)     // the latent rows back where the encoder's tail (and anybody else) reads them
    TTV_TRY(scatter_rows(ws.xl, ws.x, b->latent_rows, b->sum_tokens, row_bytes, s));
  return TTV_OK;
}

// What the encoder's gathering proj_in and the decoder's scattering proj_out (GemmArgs.gather / EPI_STORE_PATCH) both need: bf16, a patch
// whose pixel rows are 16 bytes and whose other extents are powers of two, one launch's worth of clips, the row -> sequence map.
// TTV_FUSED_PATCH=0: the copy kernels (A/B).  Each caller adds its own width condition.
static bool fused_patch_ok(const ttv_tower_dims* d, const ttv_batch* b, int dt) {
  auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
  return ttv_sw_fused_patch() && dt == TTV_BF16 && d->patch_w == 8 && pow2(d->patch_t) && pow2(d->patch_h) &&
         b->n_clips <= TTV_MAX_CLIPS_PER_LAUNCH && b->row_seq && patch_dim(d) % 64 == 0;
}

extern "C" {

const char* ttv_error_string(void) { return g_err; }
int ttv_version(void) { return 100; }

int ttv_fsq_forward(const ttv_fsq_params* p, const void* z, int z_dtype, int rows, void* codes, int codes_dtype, int32_t* indices,
                    float* bounded, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && (rows == 0 || (z && codes && indices)), "fsq_forward: null buffer");
  return ttvk_fsq_forward(p, z, z_dtype, rows, codes, codes_dtype, indices, bounded, (hipStream_t)stream);
}

int ttv_fsq_indices_to_codes(const ttv_fsq_params* p, const int32_t* indices, int rows, void* codes, int codes_dtype, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && (rows == 0 || (indices && codes)), "fsq_indices_to_codes: null buffer");
  return ttvk_fsq_indices_to_codes(p, indices, rows, codes, codes_dtype, (hipStream_t)stream);
}

int ttv_vq_codebook_norms(const void* codebook, int dtype, int ld, int N, int C, float* cnorm, void* stream) {
  TTV_CHECK_ARG(N == 0 || (codebook && cnorm), "vq_codebook_norms: null buffer");
  return ttvk_vq_norms(codebook, dtype, ld, N, C, cnorm, (hipStream_t)stream);
}

int64_t ttv_vq_workspace_bytes(int rows) { return ttvk_vq_workspace_bytes(rows); }

int ttv_vq_l2_argmin(const void* z, int dtype, int ldz, const void* codebook, int ldc, const float* cnorm, int rows, int N, int C,
                     int32_t* indices, float* best_dist, void* workspace, int64_t workspace_bytes, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (z && codebook && cnorm && indices), "vq_l2_argmin: null buffer");
  TTV_CHECK_ARG(ldz >= C && ldc >= C, "vq_l2_argmin: leading dims smaller than the codebook dim");
  return ttvk_vq_l2_argmin(z, dtype, ldz, codebook, ldc, cnorm, rows, N, C, indices, best_dist, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_vq_lookup(const void* codebook, int dtype, int ldc, const int32_t* indices, int rows, int C, void* codes, int ldo, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (codebook && indices && codes), "vq_lookup: null buffer");
  return ttvk_vq_lookup(codebook, dtype, ldc, indices, rows, C, codes, ldo, (hipStream_t)stream);
}

int ttv_vq_lookup_backward(const void* dcodes, int dtype, int ld, const int32_t* indices, int rows, int C, float* dcodebook, int ldc, void* stream) {
  TTV_CHECK_ARG(!ttv_det(), "vq_lookup_backward: deterministic mode is on and this entry point adds with atomics: call ttv_vq_lookup_backward_det");
  TTV_CHECK_ARG(rows == 0 || (dcodes && indices && dcodebook), "vq_lookup_backward: null buffer");
  TTV_CHECK_ARG(ld >= C && ldc >= C, "vq_lookup_backward: leading dims smaller than the codebook dim");
  return ttvk_vq_lookup_bwd(dcodes, dtype, ld, indices, rows, C, dcodebook, ldc, (hipStream_t)stream);
}

int64_t ttv_vq_lookup_backward_det_scratch_bytes(int rows, int N, int C) {
  if (rows < 0 || N < 1 || C < 1 || C > 256) { ttv_set_error("vq_lookup_backward_det_scratch_bytes: %d rows, %d entries of dim %d", rows, N, C); return -1; }
  return 0;      // an owner per codebook entry: no partials
}

int ttv_vq_lookup_backward_det(const void* dcodes, int dtype, int ld, const int32_t* indices, int rows, int N, int C, float* dcodebook, int ldc,
                               void* scratch, int64_t scratch_bytes, void* stream) {
  (void)scratch;
  TTV_CHECK_ARG(scratch_bytes >= 0, "vq_lookup_backward_det: negative scratch size");
  TTV_CHECK_ARG(rows == 0 || (dcodes && indices && dcodebook), "vq_lookup_backward_det: null buffer");
  TTV_CHECK_ARG(ld >= C && ldc >= C, "vq_lookup_backward_det: leading dims smaller than the codebook dim");
  if (!ttv_det()) return ttvk_vq_lookup_bwd(dcodes, dtype, ld, indices, rows, C, dcodebook, ldc, (hipStream_t)stream);
  return ttvk_vq_lookup_bwd_det(dcodes, dtype, ld, indices, rows, N, C, dcodebook, ldc, (hipStream_t)stream);
}

int64_t ttv_vq_train_workspace_bytes(int rows, int N) {
  if (rows < 1 || N < 1) { ttv_set_error("vq_train_workspace_bytes: %d rows, %d entries", rows, N); return -1; }
  return ttvk_vq_train_workspace_bytes(rows, N);
}

int ttv_vq_commit_forward(const void* z, int dtype, int ldz, const void* codebook, int ldc, const int32_t* indices, int rows, int N, int C,
                          float* loss, void* workspace, int64_t workspace_bytes, void* stream) {
  TTV_CHECK_ARG(z && codebook && indices && loss && workspace, "vq_commit_forward: null buffer");
  return ttvk_vq_commit_forward(z, dtype, ldz, codebook, ldc, indices, rows, N, C, loss, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_vq_commit_backward(const void* grad, int ldg, const void* z, int ldz, const void* e, int lde, int dtype, int rows, int C, double scale,
                           void* dz, int ldd, void* stream) {
  TTV_CHECK_ARG(grad && z && e && dz, "vq_commit_backward: null buffer");
  return ttvk_vq_commit_backward(grad, ldg, z, ldz, e, lde, dtype, rows, C, scale, dz, ldd, (hipStream_t)stream);
}

int ttv_vq_ema_stats(const void* z, int dtype, int ldz, const int32_t* indices, int rows, int N, int C, const float* cluster_size,
                     float dead_threshold, uint64_t seed, const int64_t* ema_step, int rank, int world_size, float* stats, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  TTV_CHECK_ARG(z && indices && stats && workspace, "vq_ema_stats: null buffer");
  return ttvk_vq_ema_stats(z, dtype, ldz, indices, rows, N, C, cluster_size, dead_threshold, seed, ema_step, rank, world_size, stats, workspace,
                           workspace_bytes, (hipStream_t)stream);
}

int ttv_vq_ema_update(const float* stats, float* cluster_size, float* embed_avg, float* codebook, void* codebook_copy, int copy_dtype,
                      float* cnorm, int64_t* ema_step, int N, int C, float decay, float one_minus_decay, float eps, float dead_threshold,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  TTV_CHECK_ARG(stats && cluster_size && embed_avg && codebook && codebook_copy && cnorm && ema_step && workspace, "vq_ema_update: null buffer");
  return ttvk_vq_ema_update(stats, cluster_size, embed_avg, codebook, codebook_copy, copy_dtype, cnorm, ema_step, N, C, decay, one_minus_decay, eps,
                            dead_threshold, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_quant_rows_fp8(const void* in, int dtype, int ld_in, const float* gain, float eps, void* out, int ld_out, float* scales, int rows,
                       int width, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (in && out && scales), "quant_rows_fp8: null buffer");
  return ttvk_quant_rows_fp8(in, dtype, ld_in, gain, eps, out, ld_out, scales, rows, width, (hipStream_t)stream);
}

int ttv_split3_pack(const float* w, int ldw, void* out, int ldo, int rows, int K, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (w && out), "split3_pack: null buffer");
  return ttvk_split3_pack(w, ldw, out, ldo, rows, K, (hipStream_t)stream);
}

int ttv_linear_split3(const float* x, int ldx, const void* w_image, int ldw, const float* bias, float* y, int ldy, int M, int N, int K, void* stream) {
  TTV_CHECK_ARG(M == 0 || (x && w_image && y), "linear_split3: null buffer");
  GemmArgs a = gemm_args(TTV_F32, x, ldx, w_image, ldw, M, N, K, y, ldy);
  a.split3 = 1; a.bias = bias;
  return ttvk_gemm(EPI_STORE, a, (hipStream_t)stream);
}

int64_t ttv_mx_scale_bytes_per_row(int width) { return ttvk_mx_scale_ld(width); }

int ttv_quant_mx_fp8(const void* in, int dtype, int ld_in, void* out, int ld_out, void* mx, float* row_scales, int rows, int width, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (in && out && mx), "quant_mx_fp8: null buffer");
  TTV_CHECK_ARG(ld_in >= width && ld_out >= width, "quant_mx_fp8: leading dims smaller than the width");
  return ttvk_quant_mx_fp8(in, dtype, ld_in, out, ld_out, mx, row_scales, rows, width, (hipStream_t)stream);
}

int ttv_linear_fp8_mx(const void* xq, int ldx, const void* x_mx, const float* x_row_scale, const void* wq, int ldw, const void* w_mx,
                      const float* w_row_scale, void* y, int ldy, int M, int N, int K, int epilogue, const float* rope_cs, int d_model,
                      int gqa_dim, const void* resid, int ldr, float alpha, void* stream) {
  TTV_CHECK_ARG(M == 0 || (xq && wq && y && x_mx && w_mx), "linear_fp8_mx: null buffer");
  TTV_CHECK_ARG(epilogue >= 0 && epilogue <= 3, "linear_fp8_mx: epilogue 0 (store), 1 (qkv + rotary), 2 (GEGLU) or 3 (alpha * resid + acc)");
  GemmArgs a = gemm_args(TTV_BF16, xq, ldx, wq, ldw, M, N, K, y, ldy);
  if (epilogue == 1) {
    TTV_CHECK_ARG(rope_cs && N == 2 * d_model + 2 * gqa_dim, "linear_fp8_mx: qkv epilogue needs rope_cs and N = 2 d_model + 2 gqa_dim");
    a = gemm_rope_qk(a, rope_cs, d_model, gqa_dim);
  }
  if (epilogue == 3) a = gemm_resid(a, resid, ldr, alpha);
  return ttvk_gemm_fp8(epilogue == 0 ? EPI_STORE : epilogue == 1 ? EPI_QKV_ROPE : epilogue == 2 ? EPI_GEGLU : EPI_RESID_T, a, x_row_scale,
                       w_row_scale, (hipStream_t)stream, x_mx, w_mx);
}

int ttv_linear_fp8(const void* xq, int ldx, const float* x_scale, const void* wq, int ldw, const float* w_scale, void* y, int ldy, int M, int N,
                   int K, int epilogue, const float* rope_cs, int d_model, int gqa_dim, void* stream) {
  TTV_CHECK_ARG(M == 0 || (xq && wq && y), "linear_fp8: null buffer");
  TTV_CHECK_ARG(epilogue >= 0 && epilogue <= 2, "linear_fp8: epilogue 0 (store), 1 (qkv + rotary) or 2 (GEGLU)");
  GemmArgs a = gemm_args(TTV_BF16, xq, ldx, wq, ldw, M, N, K, y, ldy);
  if (epilogue == 1) {
    TTV_CHECK_ARG(rope_cs && N == 2 * d_model + 2 * gqa_dim, "linear_fp8: qkv epilogue needs rope_cs and N = 2 d_model + 2 gqa_dim");
    a = gemm_rope_qk(a, rope_cs, d_model, gqa_dim);
  }
  return ttvk_gemm_fp8(epilogue == 0 ? EPI_STORE : epilogue == 1 ? EPI_QKV_ROPE : EPI_GEGLU, a, x_scale, w_scale, (hipStream_t)stream);
}

int ttv_rmsnorm(const void* in, int in_dtype, int ld_in, const int32_t* src_rows, void* out, int out_dtype, int ld_out,
                const int32_t* dst_rows, const float* gain, int rows, int width, float eps, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && (rows == 0 || (in && out && gain)), "rmsnorm: null buffer");
  return ttvk_rmsnorm(in, in_dtype, ld_in, src_rows, out, out_dtype, ld_out, dst_rows, gain, rows, width, eps, (hipStream_t)stream);
}

int ttv_rope_apply(void* x, int dtype, int ld, int rows, int heads, const float* rope_cs, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (x && rope_cs), "rope_apply: null buffer");
  TTV_CHECK_ARG(ld % 4 == 0 && ld >= heads * 64, "rope_apply: bad leading dim");
  return ttvk_rope_apply(x, dtype, ld, rows, heads, rope_cs, (hipStream_t)stream);
}

int ttv_rope_apply_conj(void* x, int dtype, int ld, int rows, int heads, const float* rope_cs, void* stream) {
  TTV_CHECK_ARG(rows >= 0, "rope_apply_conj: %d rows", rows);
  return ttvk_rope_apply_dir(x, dtype, ld, rows, heads, rope_cs, 1, (hipStream_t)stream);
}

int ttv_linear(const void* x, int ldx, const void* w, int ldw, const void* bias, const float* add_scalar, void* y, int ldy, int M,
               int N, int K, int dtype, void* stream) {
  TTV_CHECK_ARG(M == 0 || (x && w && y), "linear: null buffer");
  GemmArgs a = gemm_args(dtype, x, ldx, w, ldw, M, N, K, y, ldy);
  a.bias = bias; a.add_scalar = add_scalar;
  return ttvk_gemm(EPI_STORE, a, (hipStream_t)stream);
}

int ttv_linear_qkv_rope(const void* x, int ldx, const void* w, int ldw, void* y, int ldy, int M, int d_model, int gqa_dim,
                        const float* rope_cs, int dtype, void* stream) {
  TTV_CHECK_ARG(M == 0 || (x && w && y && rope_cs), "linear_qkv_rope: null buffer");
  const GemmArgs a = gemm_args(dtype, x, ldx, w, ldw, M, 2 * d_model + 2 * gqa_dim, d_model, y, ldy);
  return ttvk_gemm(EPI_QKV_ROPE, gemm_rope_qk(a, rope_cs, d_model, gqa_dim), (hipStream_t)stream);
}

int ttv_linear_geglu(const void* x, int ldx, const void* w, int ldw, void* y, int ldy, int M, int I, int K, int dtype, void* stream) {
  TTV_CHECK_ARG(M == 0 || (x && w && y), "linear_geglu: null buffer");
  return ttvk_gemm(EPI_GEGLU, gemm_args(dtype, x, ldx, w, ldw, M, I, K, y, ldy), (hipStream_t)stream);
}

int ttv_linear_residual(const void* x, int ldx, const void* w, int ldw, const void* resid, int ldr, float alpha, void* y, int ldy,
                        int y_f32, int M, int N, int K, int dtype, void* stream) {
  TTV_CHECK_ARG(M == 0 || (x && w && y && resid), "linear_residual: null buffer");
  const GemmArgs a = gemm_resid(gemm_args(dtype, x, ldx, w, ldw, M, N, K, y, ldy), resid, ldr, alpha);
  return ttvk_gemm(y_f32 ? EPI_RESID_F32 : EPI_RESID_T, a, (hipStream_t)stream);
}

int ttv_linear_residual_norm(const void* x, int ldx, const void* w, int ldw, const void* resid, int ldr, float alpha,
                             const float* gain, float eps, void* y, int ldy, int M, int N, int K, int dtype, void* stream) {
  TTV_CHECK_ARG(M == 0 || (x && w && y && resid && gain), "linear_residual_norm: null buffer");
  GemmArgs a = gemm_resid(gemm_args(dtype, x, ldx, w, ldw, M, N, K, y, ldy), resid, ldr, alpha);
  a.norm_gain = gain; a.eps = eps;
  if (!ttvk_gemm_supports_resid_norm(dtype, N, K)) {
    ttv_set_error("linear_residual_norm: only bf16 with N == 256 has a fused kernel");
    return TTV_ERR_UNSUPPORTED;
  }
  return ttvk_gemm(EPI_RESID_NORM, a, (hipStream_t)stream);
}

int64_t ttv_mlp_pack_bytes(int inner, int next_qkv_rows) { return ttvk_mlp_pack_bytes(inner, next_qkv_rows); }

int ttv_mlp_pack(const void* w12_folded, const void* w3, const void* out_proj, const void* next_qkv_folded, int next_qkv_rows, int inner,
                 int width, int dtype, void* packed, void* stream) {
  if (!ttvk_mlp_fused_supported(dtype, width, inner)) {
    ttv_set_error("mlp_pack: only bf16, width 256, inner %% 32 == 0");
    return TTV_ERR_UNSUPPORTED;
  }
  return ttvk_mlp_pack(w12_folded, w3, out_proj, next_qkv_folded, next_qkv_rows, inner, packed, (hipStream_t)stream);
}

int ttv_mlp_fused(const void* x, int ldx, const void* mlp_packed, int inner, void* y, int ldy, const float* post_gain, float alpha,
                  float eps, int M, int width, int dtype, void* stream) {
  if (!ttvk_mlp_fused_supported(dtype, width, inner)) {
    ttv_set_error("mlp_fused: only bf16, width 256, inner %% 32 == 0");
    return TTV_ERR_UNSUPPORTED;
  }
  return ttvk_mlp_fused(nullptr, 0, nullptr, 1.f, x, ldx, mlp_packed, inner, y, ldy, post_gain, alpha, eps, M, nullptr, (hipStream_t)stream);
}

int ttv_layer_tail_fused(const void* ao, int ldao, const float* attn_post_gain, float attn_alpha, const void* x, int ldx,
                         const void* mlp_packed, int inner, void* y, int ldy, const float* ffd_post_gain, float ffd_alpha, float eps,
                         int M, int width, int dtype, const ttv_next_qkv* next, void* stream) {
  if (!ttvk_mlp_fused_supported(dtype, width, inner)) {
    ttv_set_error("layer_tail_fused: only bf16, width 256, inner %% 32 == 0");
    return TTV_ERR_UNSUPPORTED;
  }
  TTV_CHECK_ARG(ao, "layer_tail_fused: null attention output");
  MlpNextQkv nx = {};
  if (next) { nx.qkv = next->qkv; nx.ld = next->ld; nx.rope_cs = next->rope_cs; nx.rows = next->rows; nx.rope_q_end = next->rope_q_end;
              nx.rope_k_begin = next->rope_k_begin; nx.rope_k_end = next->rope_k_end; }
  return ttvk_mlp_fused(ao, ldao, attn_post_gain, attn_alpha, x, ldx, mlp_packed, inner, y, ldy, ffd_post_gain, ffd_alpha, eps, M,
                        next ? &nx : nullptr, (hipStream_t)stream);
}

int ttv_fill_const_rows(void* x, int dtype, int ld, const int32_t* rows_map, int rows, int width, const float* mask_token,
                        const float* gain, float eps, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (x && rows_map && mask_token && gain), "fill_const_rows: null buffer");
  return ttvk_fill_const_rows(x, dtype, ld, rows_map, rows, width, mask_token, gain, eps, (hipStream_t)stream);
}

int ttv_decoder_embed(const void* codes, int token_size, const void* w, const void* bias, const float* mask_token, const float* gain,
                      void* x, int dtype, int ld, const int32_t* rows_map, int rows, int width, float eps, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (codes && w && bias && mask_token && gain && x && rows_map), "decoder_embed: null buffer");
  return ttvk_dec_embed(codes, token_size, w, bias, mask_token, gain, x, dtype, ld, rows_map, rows, width, eps, (hipStream_t)stream);
}

int ttv_decoder_embed_tape(const void* codes, int token_size, const void* w, const void* bias, const float* mask_token, const float* gain,
                           void* x, int dtype, int ld, const int32_t* rows_map, int rows, int width, float eps, void* hpre, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && (rows == 0 || (codes && w && bias && mask_token && gain && x && rows_map)), "decoder_embed_tape: null buffer");
  return ttvk_dec_embed_ex(codes, token_size, w, bias, mask_token, gain, x, dtype, ld, rows_map, rows, width, eps, hpre, (hipStream_t)stream);
}

int ttv_attention(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* qblocks, int n_qblocks,
                  int q_heads, int kv_heads, int head_dim, int flags, int dtype, void* stream) {
  TTV_CHECK_ARG(n_qblocks == 0 || (qkvg && out && cu_seqlens && qblocks), "attention: null buffer");
  return ttvk_attention(qkvg, ld, out, ldo, cu_seqlens, qblocks, n_qblocks, q_heads, kv_heads, head_dim, flags, dtype, (hipStream_t)stream);
}
int ttv_attention64(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* items, int n_items, int q_heads,
                    int kv_heads, int head_dim, int flags, int dtype, void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 && head_dim == 64, "attention64: bf16, head_dim 64 only");
  return ttvk_attention64(qkvg, ld, out, ldo, cu_seqlens, items, n_items, q_heads, kv_heads, flags, (hipStream_t)stream);
}

int64_t ttv_attention_pv8_bytes(int total_rows, int n_seqs, int kv_heads) { return ttvk_attention_pv8_bytes(total_rows, n_seqs, kv_heads); }
int ttv_quant_v_pv8(const void* qkvg, int ld, const int32_t* cu_seqlens, int n_seqs, int total_rows, int q_heads, int kv_heads, void* image,
                    void* stream) {
  return ttvk_quant_v_pv8(qkvg, ld, cu_seqlens, n_seqs, total_rows, q_heads, kv_heads, image, (hipStream_t)stream);
}
int ttv_attention_pv8(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* qblocks, int n_qblocks,
                      int q_heads, int kv_heads, int head_dim, int flags, const void* image, void* stream) {
  return ttvk_attention_pv8(qkvg, ld, out, ldo, cu_seqlens, qblocks, n_qblocks, q_heads, kv_heads, head_dim, flags, image, (hipStream_t)stream);
}

// The three fused MX producers of run_layer_mx, one by one (tests only: tests/test_hip_fp8_blocks.py)
int ttv_rmsnorm_mx(const void* in, int in_dtype, int ld_in, void* out, int out_dtype, int ld_out, const float* gain, int rows, int width,
                   float eps, float* next_rstd, void* mx_q, void* mx_s, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && (rows == 0 || (in && out && gain)), "rmsnorm_mx: null buffer");
  TTV_CHECK_ARG(!mx_q == !mx_s, "rmsnorm_mx: the image needs both its element and its scale buffer");
  return ttvk_rmsnorm(in, in_dtype, ld_in, nullptr, out, out_dtype, ld_out, nullptr, gain, rows, width, eps, (hipStream_t)stream, next_rstd, mx_q, mx_s);
}

int ttv_attention_mxout(const void* qkvg, int ld, void* out_q, void* out_mx, int ld_mx, const int32_t* cu_seqlens, const int32_t* qblocks,
                        int n_qblocks, int q_heads, int kv_heads, void* stream) {
  TTV_CHECK_ARG(n_qblocks >= 0 && (n_qblocks == 0 || (qkvg && out_q && out_mx && cu_seqlens && qblocks)), "attention_mxout: null buffer");
  return ttvk_attention_mxout(qkvg, ld, out_q, out_mx, ld_mx, cu_seqlens, qblocks, n_qblocks, q_heads, kv_heads, (hipStream_t)stream);
}

int ttv_linear_fp8_mx_geglu_q(const void* xq, int ldx, const void* x_mx, const float* x_row_scale, const void* wq, int ldw, const void* w_mx,
                              const float* w_row_scale, void* hq, void* hq_mx, int M, int N, int K, void* stream) {
  TTV_CHECK_ARG(M == 0 || (xq && wq && x_mx && w_mx && hq && hq_mx), "linear_fp8_mx_geglu_q: null buffer");
  GemmArgs a = gemm_args(TTV_BF16, xq, ldx, wq, ldw, M, N, K, hq, N);      // no bf16 output: y is the image buffer, as in run_layer_mx
  a.yq = hq; a.yq_mx = hq_mx;
  return ttvk_gemm_fp8(EPI_GEGLU, a, x_row_scale, w_row_scale, (hipStream_t)stream, x_mx, w_mx);
}

// The folded pre-norm of the wide bf16 layer (prenorm_proj's fold_gen route), one launch at a time (tests only:
// tests/test_hip_wide_layer.py): the light statistic pass, and a to_qkv / w12 / plain GEMM whose output rows take a row scale
int ttv_row_rstd(const void* x, int dtype, int ldx, float* rstd, int rows, int width, float eps, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && (rows == 0 || (x && rstd)), "row_rstd: null buffer");
  TTV_CHECK_ARG(ldx >= width, "row_rstd: leading dim smaller than the width");
  return ttvk_row_rstd(x, dtype, ldx, rstd, rows, width, eps, (hipStream_t)stream);
}

int ttv_linear_rowscale(const void* x, int ldx, const void* w, int ldw, const float* row_scale, int epilogue, const float* rope_cs, int d_model,
                        int gqa_dim, void* y, int ldy, int M, int N, int K, int dtype, void* stream) {
  TTV_CHECK_ARG(M == 0 || (x && w && y), "linear_rowscale: null buffer");
  TTV_CHECK_ARG(epilogue >= 0 && epilogue <= 2, "linear_rowscale: epilogue 0 (store), 1 (qkv + rotary) or 2 (GEGLU)");
  GemmArgs a = gemm_args(dtype, x, ldx, w, ldw, M, N, K, y, ldy);
  if (epilogue == 1) {
    TTV_CHECK_ARG(rope_cs && N == 2 * d_model + 2 * gqa_dim && K == d_model, "linear_rowscale: qkv epilogue needs rope_cs, N = 2 d_model + 2 gqa_dim and K = d_model");
    a = gemm_rope_qk(a, rope_cs, d_model, gqa_dim);
  }
  a.row_scale = row_scale;
  return ttvk_gemm(epilogue == 0 ? EPI_STORE : epilogue == 1 ? EPI_QKV_ROPE : EPI_GEGLU, a, (hipStream_t)stream);
}

int ttv_patch_gather(const void* const* clips, const int32_t* clip_desc, int clip0, int n_clips, int patch_t, int patch_h, int patch_w,
                     int channels, void* patches, int ld, int dtype, int max_patches_per_clip, void* stream) {
  TTV_CHECK_ARG(n_clips == 0 || (clips && clip_desc && patches), "patch_gather: null buffer");
  return ttvk_patch_copy(false, (void* const*)clips, clip_desc, clip0, n_clips, patch_t, patch_h, patch_w, channels, patches, ld, dtype, max_patches_per_clip, (hipStream_t)stream);
}

int ttv_patch_embed_norm(const void* const* clips, const int32_t* clip_desc, const int32_t* patch_rows, const int32_t* row_seq, int n_clips,
                         int patch_t, int patch_h, int patch_w, int channels, const void* w, int ldw, const void* bias, const float* mask_token,
                         const float* gain, float eps, void* x, int ldx, int rows, int width, int dtype, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (clips && clip_desc && patch_rows && row_seq && w && bias && mask_token && gain && x), "patch_embed_norm: null buffer");
  const int pd = channels * patch_t * patch_h * patch_w;
  if (!ttvk_patch_embed_norm_supported(dtype, width, pd, patch_w)) {
    ttv_set_error("patch_embed_norm: only bf16, width 256, patch_w 8 and a patch vector that is a multiple of 64");
    return TTV_ERR_UNSUPPORTED;
  }
  return ttvk_patch_embed_norm((void* const*)clips, 0, n_clips, clip_desc, patch_rows, row_seq, patch_t, patch_h, patch_w, pd, w, ldw, bias,
                               mask_token, gain, eps, x, ldx, rows, (hipStream_t)stream);
}

int ttv_patch_scatter(const void* patches, int ld, const int32_t* clip_desc, int clip0, int n_clips, int patch_t, int patch_h, int patch_w,
                      int channels, void* const* clips, int dtype, int max_patches_per_clip, void* stream) {
  TTV_CHECK_ARG(n_clips == 0 || (clips && clip_desc && patches), "patch_scatter: null buffer");
  return ttvk_patch_copy(true, clips, clip_desc, clip0, n_clips, patch_t, patch_h, patch_w, channels, (void*)patches, ld, dtype, max_patches_per_clip, (hipStream_t)stream);
}

int64_t ttv_tower_workspace_bytes(const ttv_tower_dims* dims, const ttv_batch* batch) {
  if (check_dims(dims, batch) != TTV_OK) return -1;
  return carve(dims, batch, nullptr).total;
}

int ttv_encoder_forward(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const void* const* clips,
                        const ttv_fsq_params* fsq, float* z, void* codes, int32_t* indices, float* bounded, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  TTV_TRY(check_dims(d, b));
  TTV_CHECK_ARG(d->kind == TTV_ENCODER, "encoder_forward: dims.kind is not TTV_ENCODER");
  TTV_CHECK_ARG(w && w->layers && clips && workspace, "encoder_forward: null argument");
  TTV_CHECK_ARG(fsq || z, "encoder_forward: neither fsq nor z requested");
  TTV_CHECK_ARG(!fsq || (codes && indices), "encoder_forward: fsq needs codes and indices buffers");
  hipStream_t s = (hipStream_t)stream;
  TowerWs ws = carve(d, b, (char*)workspace);
  TTV_CHECK_ARG(ws.total <= workspace_bytes, "encoder_forward: workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)ws.total);
  const int dm = d->width, dt = d->dtype, P = b->sum_patches, pd = patch_dim(d);

  // patchify (utils.py:26-34) + proj_in (blocks.py:91-93) + ln_pre_p of the patch rows (blocks.py:95-97).  Width 256 bf16: one kernel
  // that keeps a patch's whole row in a block, so neither a gathered copy nor the sums pass through memory (k_patch_embed256).
  // TTV_PATCH_EMBED_FUSED=0 / debug bit 24: the GEMM and the row kernel below (A/B, tests)
  static const bool embed_env = ttv_env_flag("TTV_PATCH_EMBED_FUSED", true);
  if (embed_env && !(g_ttv_debug & TTV_DBG_PATCH_EMBED_UNFUSED) && fused_patch_ok(d, b, dt) && w->proj_in_b && w->mask_token &&
      ttvk_patch_embed_norm_supported(dt, dm, pd, d->patch_w)) {
    TTV_TRY(ttvk_patch_embed_norm((void* const*)clips, 0, b->n_clips, b->clip_desc, b->patch_rows, b->row_seq, d->patch_t, d->patch_h, d->patch_w,
                                  pd, w->proj_in_w, pd, w->proj_in_b, w->mask_token, w->ln_pre_p, d->eps, ws.x, dm, P, s));
  } else {
    // when the shapes allow it the GEMM reads its K = (c, pt, ph, pw) operand straight from the clips (16-byte pixel-row segments)
    // instead of from a gathered [P, pd] copy
    const bool gather = fused_patch_ok(d, b, dt) && pd != 256;
    if (!gather) TTV_TRY(patch_copy_all(false, (void* const*)clips, d, b, ws.pa, dt, s));
    GemmArgs a = gemm_args(dt, ws.pa, pd, w->proj_in_w, pd, P, dm, pd, ws.pb, dm);
    a.bias = w->proj_in_b; a.add_scalar = w->mask_token;
    a.split3 = (dt == TTV_F32 && w->f32_split3) ? 1 : 0;
    if (gather) {
      a.gather = 1; a.clips = (void* const*)clips; a.n_clips = b->n_clips; a.clip_desc = b->clip_desc; a.patch_rows = b->patch_rows;
      a.row_seq = b->row_seq; a.patch_t = d->patch_t; a.patch_h = d->patch_h; a.patch_w = d->patch_w;
    }
    TTV_TRY(ttvk_gemm(EPI_STORE, a, s));
    TTV_TRY(ttvk_rmsnorm(ws.pb, dt, dm, nullptr, ws.x, dt, dm, b->patch_rows, w->ln_pre_p, P, dm, d->eps, s));
  }
  // x[latent rows] = ln_pre_t(mask_token * 1) (blocks.py:95-97)
  TTV_TRY(ttvk_fill_const_rows(ws.x, dt, dm, b->latent_rows, b->sum_tokens, dm, w->mask_token, w->ln_pre_t, d->eps, s));

  TTV_TRY(run_layers(d, w, b, ws, s));

  // tokens = proj_out(ln_post(x[latent rows])) -> FSQ (blocks.py:101-103, fsq.py:123-135)
  TTV_TRY(ttvk_enc_tail(ws.x, dt, dm, b->latent_rows, b->sum_tokens, dm, w->ln_post, d->eps, w->proj_out_w, w->proj_out_b, d->token_size, fsq, z, codes, indices, bounded, s));
  return TTV_OK;
}

int64_t ttv_dec_l0_const_bytes(const ttv_tower_dims* d, int patch_rows) {
  if (!d || patch_rows <= 0 || d->dtype != TTV_BF16 || d->width != 256 || d->head_dim != 64 || d->kv_heads <= 0) {
    ttv_set_error("dec_l0_const_bytes: bf16 decoders of width 256 and head_dim 64 only");
    return -1;
  }
  if (patch_rows % 128) {
    ttv_set_error("dec_l0_const_bytes: patch_rows must be a multiple of 128");
    return -1;
  }
  const int64_t nq = 2 * (int64_t)d->width + 2 * (int64_t)d->kv_heads * d->head_dim;
  // rows | attention state of every (patch query block, q-head) + the flag word | the builder's scratch x
  return align256(patch_rows * nq * 2) + align256(ttvk_attention_swp_state_floats(patch_rows, d->q_heads) * 4 + 4) + align256((int64_t)patch_rows * d->width * 2);
}

int ttv_dec_l0_const_build(const ttv_tower_dims* d, const ttv_tower_weights* w, const int32_t* iota, const float* rope_cs, const int32_t* rope_ids,
                           const float* rope_base, int patch_rows, void* block, int64_t block_bytes, int64_t* state_offset, int64_t* flag_offset,
                           void* stream) {
  TTV_CHECK_ARG(d && w && w->layers && iota && rope_cs && block && patch_rows > 0, "dec_l0_const_build: null argument");
  const int64_t need = ttv_dec_l0_const_bytes(d, patch_rows);
  if (need < 0) return TTV_ERR_UNSUPPORTED;
  TTV_CHECK_ARG(d->kind == TTV_DECODER && need <= block_bytes && (uintptr_t)block % 256 == 0, "dec_l0_const_build: not a decoder, or block too small / unaligned");
  const ttv_layer_weights& lw = w->layers[0];
  if (!lw.to_qkv_pn || !lw.qkv_q_prescaled) {
    ttv_set_error("dec_l0_const_build: layer 0 needs the folded, q-pre-scaled to_qkv weight");
    return TTV_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  const int dm = d->width, g = d->kv_heads * d->head_dim, nq = 2 * dm + 2 * g, dt = d->dtype;
  char* const rows = (char*)block;
  const int64_t state_floats = ttvk_attention_swp_state_floats(patch_rows, d->q_heads);
  float* const state = (float*)(rows + align256((int64_t)patch_rows * nq * 2));
  char* const x = (char*)state + align256(state_floats * 4 + 4);
  if (state_offset) *state_offset = (char*)state - rows;
  if (flag_offset) *flag_offset = (char*)(state + state_floats) - rows;
  // the forward's own two kernels on patch_rows rows of a scratch x: ln_pre_p(mask_token), then layer 0's to_qkv with the folded pre-norm
  TTV_TRY(ttvk_fill_const_rows(x, dt, dm, iota, patch_rows, dm, w->mask_token, w->ln_pre_p, d->eps, s));
  GemmArgs a = gemm_rope_qk(gemm_args(dt, x, dm, lw.to_qkv_pn, dm, patch_rows, nq, dm, rows, nq), rope_cs, dm, g);
  a.prenorm = 1; a.eps = d->eps;
  a.rope_ids = rope_ids; a.rope_base = rope_ids ? rope_base : nullptr;
  TTV_TRY(ttvk_gemm(EPI_QKV_ROPE, a, s));
  // what k_attn_swp accumulates for every patch query block over the patch keys, raw; the flag says whether a row sum left its window
  if (hipMemsetAsync(state + state_floats, 0, 4, s) != hipSuccess) {
    ttv_set_error("dec_l0_const_build: hipMemsetAsync failed");
    return TTV_ERR_LAUNCH;
  }
  return ttvk_attention_swp_dump(rows, nq, patch_rows, d->q_heads, d->kv_heads, state, s);
}

int ttv_decoder_forward(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const void* codes,
                        void* const* clips_out, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttv_decoder_forward_const(d, w, b, codes, clips_out, workspace, workspace_bytes, nullptr, stream);
}

int ttv_decoder_forward_const(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const void* codes,
                              void* const* clips_out, void* workspace, int64_t workspace_bytes, const ttv_dec_l0_const* l0, void* stream) {
  TTV_TRY(check_dims(d, b));
  TTV_CHECK_ARG(d->kind == TTV_DECODER, "decoder_forward: dims.kind is not TTV_DECODER");
  TTV_CHECK_ARG(w && w->layers && codes && clips_out && workspace, "decoder_forward: null argument");
  hipStream_t s = (hipStream_t)stream;
  TowerWs ws = carve(d, b, (char*)workspace);
  TTV_CHECK_ARG(ws.total <= workspace_bytes, "decoder_forward: workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)ws.total);
  const int dm = d->width, dt = d->dtype, P = b->sum_patches, pd = patch_dim(d);

  // x[latent rows] = ln_pre_t(proj_in(codes) + mask_token); x[patch rows] = ln_pre_p(mask_token * 1) (blocks.py:165-167)
  TTV_TRY(ttvk_dec_embed(codes, d->token_size, w->proj_in_w, w->proj_in_b, w->mask_token, w->ln_pre_t, ws.x, dt, dm, b->latent_rows, b->sum_tokens, dm, d->eps, s));
  TTV_TRY(ttvk_fill_const_rows(ws.x, dt, dm, b->patch_rows, P, dm, w->mask_token, w->ln_pre_p, d->eps, s));      // (the residual stream needs them with or without l0)

  TTV_TRY(run_layers(d, w, b, ws, s, l0));

  // patches = proj_out(ln_post(x[patch rows])) -> unpatchify (blocks.py:171-176)
  GemmArgs a = gemm_args(dt, nullptr, dm, w->proj_out_w, dm, P, pd, dm, ws.pa, pd);      // operand: ws.x in place or its normed patch rows, below
  a.split3 = (dt == TTV_F32 && w->f32_split3) ? 1 : 0;
  a.bias = w->proj_out_b;
  if (dt == TTV_BF16 && dm == 256 && w->proj_out_pn && pd % 8 == 0) {
    // ln_post folded into the GEMM: gain in the weight columns, rstd from the register-resident row, rows gathered in place
    a.x = ws.x; a.x_rows = b->patch_rows; a.w = w->proj_out_pn; a.prenorm = 1; a.eps = d->eps;
  } else {
    TTV_TRY(ttvk_rmsnorm(ws.x, dt, dm, b->patch_rows, ws.pb, dt, dm, nullptr, w->ln_post, P, dm, d->eps, s));
    a.x = ws.pb;
  }
  // unpatchify inside the GEMM epilogue (8 consecutive output features = one 16-byte pixel row segment of a patch) when the
  // shapes allow it: saves the [P, pd] round trip and the copy kernel.  TTV_FUSED_PATCH=0 keeps the two-kernel sequence.
  if (fused_patch_ok(d, b, dt) && dm == 256) {
    a.clips = clips_out; a.n_clips = b->n_clips; a.clip_desc = b->clip_desc; a.patch_rows = b->patch_rows; a.row_seq = b->row_seq;
    a.patch_t = d->patch_t; a.patch_h = d->patch_h; a.patch_w = d->patch_w;
    return ttvk_gemm(EPI_STORE_PATCH, a, s);
  }
  TTV_TRY(ttvk_gemm(EPI_STORE, a, s));
  return patch_copy_all(true, clips_out, d, b, ws.pa, dt, s);
}

int ttv_rope_table_build(const float* base_cos, const float* base_sin, int n_ids, int n_freqs, const int32_t* clip_desc, const int32_t* cu_seqlens,
                         const int32_t* row_seq, float* rope_cs, int total_rows, void* stream) {
  TTV_CHECK_ARG(total_rows == 0 || (base_cos && base_sin && clip_desc && cu_seqlens && row_seq && rope_cs), "rope_table_build: null buffer");
  TTV_CHECK_ARG(n_freqs >= 1 && 3 * n_freqs <= 32 && n_ids >= 1, "rope_table_build: bad table shape");
  return ttvk_rope_build(base_cos, base_sin, n_ids, n_freqs, clip_desc, cu_seqlens, row_seq, rope_cs, total_rows, (hipStream_t)stream);
}

int ttv_l1_loss(void* const* recon, void* const* target, void* const* grad, const int32_t* sizes, int n_clips, int dtype, float* loss,
                void* stream) {
  // loss must be zeroed by the caller; clips are processed in groups of TTV_MAX_CLIPS_PER_LAUNCH
  TTV_CHECK_ARG(!ttv_det(), "l1_loss: deterministic mode is on and this entry point has no scratch for the block partials: call ttv_l1_loss_det");
  return for_clip_groups(n_clips, [&](int c0, int n) {
    return ttvk_l1_loss(recon + c0, target + c0, grad ? grad + c0 : nullptr, sizes + c0, n, n_clips, dtype, loss, (hipStream_t)stream, nullptr);
  });
}

static int64_t clips_det_bytes(const int32_t* sizes, int n_clips, bool l1, const char* what) {
  if (n_clips < 0 || (n_clips > 0 && !sizes)) { ttv_set_error("%s: bad argument", what); return -1; }
  for (int i = 0; i < n_clips; ++i)
    if (sizes[i] <= 0) { ttv_set_error("%s: empty clip", what); return -1; }
  return ttvk_det_clips_bytes(sizes, n_clips, l1);
}
int64_t ttv_l1_loss_det_scratch_bytes(const int32_t* sizes, int n_clips) { return clips_det_bytes(sizes, n_clips, true, "l1_loss_det_scratch_bytes"); }
int64_t ttv_sq_err_accumulate_det_scratch_bytes(const int32_t* sizes, int n_clips) { return clips_det_bytes(sizes, n_clips, false, "sq_err_accumulate_det_scratch_bytes"); }

int ttv_l1_loss_det(void* const* recon, void* const* target, void* const* grad, const int32_t* sizes, int n_clips, int dtype, float* loss,
                    void* scratch, int64_t scratch_bytes, void* stream) {
  const DetScratch det = {scratch, scratch_bytes};
  return for_clip_groups(n_clips, [&](int c0, int n) {
    return ttvk_l1_loss(recon + c0, target + c0, grad ? grad + c0 : nullptr, sizes + c0, n, n_clips, dtype, loss, (hipStream_t)stream, &det);
  });
}

int ttv_sq_err_accumulate_det(void* const* recon, void* const* target, const int32_t* sizes, int n_clips, int dtype, int clamp, double* acc,
                              void* scratch, int64_t scratch_bytes, void* stream) {
  const DetScratch det = {scratch, scratch_bytes};
  return for_clip_groups(n_clips, [&](int c0, int n) {
    return ttvk_sq_err(recon + c0, target + c0, sizes + c0, n, dtype, clamp, acc, (hipStream_t)stream, &det);
  });
}

// The tower backward's three small reductions on their own (tests: both modes; the scratch is looked at in deterministic mode only)
int64_t ttv_colsum_det_scratch_bytes(int rows, int n) {
  if (rows < 0 || n < 1) { ttv_set_error("colsum_det_scratch_bytes: %d rows, %d columns", rows, n); return -1; }
  return ttvk_det_colsum_bytes(rows, n);
}
int64_t ttv_sumall_det_scratch_bytes(int rows, int n) {
  if (rows < 0 || n < 1) { ttv_set_error("sumall_det_scratch_bytes: %d rows, %d columns", rows, n); return -1; }
  return ttvk_det_sumall_bytes((long)rows * n);
}
int64_t ttv_outer_small_det_scratch_bytes(int rows, int C, int d) {
  if (rows < 0 || C < 1 || C > TTV_MAX_TOKEN || d < 1) { ttv_set_error("outer_small_det_scratch_bytes: %d rows, C %d, d %d", rows, C, d); return -1; }
  return ttvk_det_outer_small_bytes(rows, C, d);
}
int ttv_colsum_accumulate(const void* a, int dtype, int lda, const int32_t* rows_map, int rows, int n, float* out, void* scratch,
                          int64_t scratch_bytes, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && n >= 1 && lda >= n && (rows == 0 || (a && out)), "colsum_accumulate: bad argument");
  const DetScratch det = {scratch, scratch_bytes};
  return ttvk_colsum(a, dtype, lda, rows_map, rows, n, out, (hipStream_t)stream, &det);
}
int ttv_sumall_accumulate(const void* a, int dtype, int lda, int rows, int n, float scale, float* out, void* scratch, int64_t scratch_bytes,
                          void* stream) {
  TTV_CHECK_ARG(rows >= 0 && n >= 1 && lda >= n && (rows == 0 || (a && out)), "sumall_accumulate: bad argument");
  const DetScratch det = {scratch, scratch_bytes};
  return ttvk_sumall(a, dtype, lda, nullptr, rows, n, nullptr, scale, out, (hipStream_t)stream, &det);
}
int ttv_outer_small_accumulate(const void* a, int a_dtype, int lda, int C, const void* b, int b_dtype, int ldb, float* dw, int lddw,
                               int transpose_out, int rows, int d, void* scratch, int64_t scratch_bytes, void* stream) {
  TTV_CHECK_ARG(rows >= 0 && d >= 1 && d <= 1024 && lda >= C && ldb >= d && (rows == 0 || (a && b && dw)), "outer_small_accumulate: bad argument");
  TTV_CHECK_ARG(lddw >= (transpose_out ? C : d), "outer_small_accumulate: leading dim of dw");
  const DetScratch det = {scratch, scratch_bytes};
  return ttvk_outer_small(a, a_dtype, lda, C, b, b_dtype, ldb, nullptr, dw, lddw, transpose_out, rows, d, (hipStream_t)stream, &det);
}

int ttv_clip_from_u8(const void* frames_thwc, int T, int H, int W, void* clip_cthw, int dtype, void* stream) {
  TTV_CHECK_ARG(frames_thwc && clip_cthw && T > 0 && H > 0 && W > 0, "clip_from_u8: bad argument");
  return ttvk_clip_from_u8(frames_thwc, (long long)T * H * W, clip_cthw, dtype, (hipStream_t)stream);
}

int ttv_clip_resample_u8(void* const* frames_thwc, void* const* clips_cthw, const int32_t* geom, int n_clips, int dtype, void* stream) {
  return ttvk_clip_resample_u8(frames_thwc, clips_cthw, geom, n_clips, dtype, (hipStream_t)stream);
}

int ttv_sq_err_accumulate(void* const* recon, void* const* target, const int32_t* sizes, int n_clips, int dtype, int clamp, double* acc,
                          void* stream) {
  TTV_CHECK_ARG(!ttv_det(), "sq_err_accumulate: deterministic mode is on and this entry point has no scratch for the block partials: call ttv_sq_err_accumulate_det");
  return for_clip_groups(n_clips, [&](int c0, int n) { return ttvk_sq_err(recon + c0, target + c0, sizes + c0, n, dtype, clamp, acc, (hipStream_t)stream, nullptr); });
}

int64_t ttv_ssim_workspace_bytes(const int32_t* dims, int n_clips) { return ttvk_ssim_workspace_bytes(dims, n_clips); }

int ttv_ssim_accumulate(void* const* recon, void* const* target, const int32_t* dims, int n_clips, int dtype, int clamp, double* acc,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  return ttvk_ssim(recon, target, dims, n_clips, dtype, clamp, acc, workspace, workspace_bytes, (hipStream_t)stream);
}

int64_t ttv_lpips_tape_bytes(int n, int H, int W, int dtype) { return ttvk_lpips_tape_bytes(n, H, W, dtype); }

int64_t ttv_lpips_workspace_bytes(int n, int H, int W, int dtype) { return ttvk_lpips_workspace_bytes(n, H, W, dtype); }

int ttv_lpips_forward(const ttv_lpips_weights* w, const void* recon, const void* target, int n, int H, int W, int dtype, float* lpips,
                      float* gram, void* tape, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttvk_lpips_forward(w, recon, target, n, H, W, dtype, lpips, gram, tape, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_lpips_backward(const ttv_lpips_weights* w, const void* tape, int n, int H, int W, int dtype, const float* glpips,
                       const float* ggram, void* drecon, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttvk_lpips_backward(w, tape, n, H, W, dtype, glpips, ggram, drecon, workspace, workspace_bytes, (hipStream_t)stream);
}

int64_t ttv_lpips_eval_workspace_bytes(int frames, int H, int W, int dtype) { return ttvk_lpips_eval_workspace_bytes(frames, H, W, dtype); }

int ttv_lpips_eval_accumulate(const ttv_lpips_weights* w, void* const* recon_clips, void* const* target_clips, const int32_t* frames,
                              int n_clips, int H, int W, int dtype, int clamp_recon, float* per_frame, double* acc, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  return ttvk_lpips_eval_accumulate(w, recon_clips, target_clips, frames, n_clips, H, W, dtype, clamp_recon, per_frame, acc, workspace,
                                    workspace_bytes, (hipStream_t)stream);
}

int ttv_lpips_crops_forward(void* const* recon_clips, void* const* target_clips, const int32_t* clip_dims, int n_clips, const int32_t* crops,
                            int n_crops, int size, void* recon_crops, void* target_crops, int dtype, void* stream) {
  return ttvk_lpips_crops_forward(recon_clips, target_clips, clip_dims, n_clips, crops, n_crops, size, recon_crops, target_crops, dtype,
                                  (hipStream_t)stream);
}

int ttv_lpips_crops_backward(void* const* recon_clips, void* const* grad_clips, const int32_t* clip_dims, int n_clips, const int32_t* crops,
                             int n_crops, int size, const void* g, int dtype, void* stream) {
  return ttvk_lpips_crops_backward(recon_clips, grad_clips, clip_dims, n_clips, crops, n_crops, size, g, dtype, (hipStream_t)stream);
}

int64_t ttv_lpips_conv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype) {
  return ttvk_lpips_conv_workspace_bytes(N, H, W, Cin, Cout, dtype);
}

int ttv_lpips_conv3x3(const void* x, int N, int H, int W, int Cin, int Cout, const void* w, const float* bias, int mode, const void* h,
                      void* y, int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttvk_lpips_conv3x3(x, N, H, W, Cin, Cout, w, bias, mode, h, y, dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_lpips_maxpool(const void* x, int N, int H, int W, int C, void* y, int dtype, void* stream) {
  return ttvk_lpips_maxpool(x, N, H, W, C, y, dtype, (hipStream_t)stream);
}

int ttv_lpips_maxpool_backward(const void* dy, const float* add, const void* h, int N, int H, int W, int C, void* dx, int dtype,
                               void* stream) {
  return ttvk_lpips_maxpool_backward(dy, add, h, N, H, W, C, dx, dtype, (hipStream_t)stream);
}

int64_t ttv_i3d_workspace_bytes(int n) { return ttvk_i3d_workspace_bytes(n); }

int ttv_fvd_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, int clamp, float* out, void* stream) {
  return ttvk_fvd_preprocess(clips, dims, n_clips, dtype, clamp, out, (hipStream_t)stream);
}

int ttv_i3d_features(const ttv_i3d_weights* w, const float* x, int n, float* feats, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  return ttvk_i3d_features(w, x, n, feats, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_i3d_conv3d(const float* x, int N, int T, int H, int W, int Cin, int k, int stride, const float* w, const float* scale,
                   const float* shift, int Cout, int relu, float* y, int ldc, int c_off, void* stream) {
  return ttvk_i3d_conv3d(x, N, T, H, W, Cin, k, stride, w, scale, shift, Cout, relu, y, ldc, c_off, (hipStream_t)stream);
}

int ttv_i3d_maxpool3d(const float* x, int N, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw, float* y,
                      void* stream) {
  return ttvk_i3d_maxpool3d(x, N, T, H, W, C, kt, kh, kw, st, sh, sw, y, (hipStream_t)stream);
}

int64_t ttv_inception_workspace_bytes(int n) { return ttvk_inception_workspace_bytes(n); }

int ttv_inception_preprocess(void* const* images, const int64_t* dims, int n, int dtype, int clamp, float* out, void* stream) {
  return ttvk_inception_preprocess(images, dims, n, dtype, clamp, out, (hipStream_t)stream);
}

int ttv_inception_features(const ttv_inception_weights* w, const float* x, int n, float* acts, float* probs, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return ttvk_inception_features(w, x, n, acts, probs, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_inception_conv2d(const float* x, int N, int H, int W, int Cin, int kh, int kw, int sh, int sw, int ph, int pw, const float* w,
                         const float* scale, const float* shift, int Cout, int relu, float* y, int ldc, int c_off, void* stream) {
  return ttvk_inception_conv2d(x, N, H, W, Cin, kh, kw, sh, sw, ph, pw, w, scale, shift, Cout, relu, y, ldc, c_off, (hipStream_t)stream);
}

int ttv_inception_pool2d(const float* x, int N, int H, int W, int C, int mode, float* y, int ldc, int c_off, void* stream) {
  return ttvk_inception_pool2d(x, N, H, W, C, mode, y, ldc, c_off, (hipStream_t)stream);
}

int ttv_jedi_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, void* out, void* stream) {
  return ttvk_jedi_preprocess(clips, dims, n_clips, dtype, out, (hipStream_t)stream);
}

int64_t ttv_vjepa_workspace_bytes(int n) { return ttvk_vjepa_workspace_bytes(n); }

int ttv_vjepa_features(const ttv_vjepa_weights* w, const void* x, int n, float* feats, int finetuned, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return ttvk_vjepa_features(w, x, n, feats, finetuned, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_vjepa_layernorm(const float* x, int ldx, int rows, int width, const float* w1, const float* b1, float eps1, const float* w2,
                        const float* b2, float eps2, float* y32, int ld32, void* y16, int ld16, void* stream) {
  return ttvk_vjepa_layernorm(x, ldx, rows, width, w1, b1, eps1, w2, b2, eps2, y32, ld32, y16, ld16, (hipStream_t)stream);
}

int ttv_vjepa_linear(const void* x, int ldx, const void* w, int ldw, const void* bias, int M, int N, int K, int epilogue,
                     const float* resid, int ldr, int resid_rows, void* y, int ldy, void* stream) {
  return ttvk_vjepa_linear(x, ldx, w, ldw, bias, M, N, K, epilogue, resid, ldr, resid_rows, y, ldy, (hipStream_t)stream);
}

int ttv_vjepa_pool_attention(const void* q, const void* kv, int n, int rows, void* out, void* stream) {
  return ttvk_vjepa_pool_attention(q, kv, n, rows, out, (hipStream_t)stream);
}

int ttv_debug_set(int flags) {
  g_ttv_debug = flags;
  return TTV_OK;
}

int ttv_set_deterministic(int on) { return __atomic_exchange_n(&g_ttv_det, on ? 1 : 0, __ATOMIC_RELAXED); }
int ttv_get_deterministic(void) { return ttv_det() ? 1 : 0; }

int ttv_debug_stamps(void* device_buffer) {
  g_ttv_stamps = (long long*)device_buffer;
  return TTV_OK;
}

int ttv_prof_begin(int kernel_class, int max_records) {
  TTV_CHECK_ARG(g_ttv_prof_class == 0, "prof_begin: already recording");
  TTV_CHECK_ARG(kernel_class > 0 && max_records > 0 && max_records <= (1 << 20), "prof_begin: bad arguments");
  g_prof_start = new hipEvent_t[max_records];
  g_prof_stop = new hipEvent_t[max_records];
  for (int i = 0; i < max_records; ++i) {
    if (hipEventCreate(&g_prof_start[i]) != hipSuccess || hipEventCreate(&g_prof_stop[i]) != hipSuccess) {
      ttv_set_error("prof_begin: hipEventCreate failed");
      return TTV_ERR_LAUNCH;
    }
  }
  g_prof_cap = max_records;
  g_prof_n = 0;
  g_ttv_prof_class = kernel_class;
  return TTV_OK;
}

int ttv_prof_end(double* total_ms, int* count) {
  TTV_CHECK_ARG(g_ttv_prof_class != 0 && total_ms && count, "prof_end: not recording");
  g_ttv_prof_class = 0;
  double tot = 0.0;
  for (int i = 0; i < g_prof_n; ++i) {
    float ms = 0.f;
    (void)hipEventSynchronize(g_prof_stop[i]);
    (void)hipEventElapsedTime(&ms, g_prof_start[i], g_prof_stop[i]);
    tot += ms;
  }
  *total_ms = tot;
  *count = g_prof_n;
  for (int i = 0; i < g_prof_cap; ++i) {
    (void)hipEventDestroy(g_prof_start[i]);
    (void)hipEventDestroy(g_prof_stop[i]);
  }
  delete[] g_prof_start;
  delete[] g_prof_stop;
  g_prof_start = g_prof_stop = nullptr;
  g_prof_cap = g_prof_n = 0;
  return TTV_OK;
}

int ttv_codebook_histogram(const int32_t* indices, int n, int64_t* counts, int codebook_size, void* stream) {
  TTV_CHECK_ARG(n == 0 || (indices && counts), "codebook_histogram: null buffer");
  return ttvk_histogram(indices, n, counts, codebook_size, (hipStream_t)stream);
}

}  // extern "C"
