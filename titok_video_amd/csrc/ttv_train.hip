// Training step of a tower (reference train.py:65-83 = autograd through blocks.py / transformer.py / fsq.py):
// a tape-recording forward (unfused kernel sequence, every tensor backward needs is written into the caller's tape)
// and the hand-written backward launch sequence.  Gradients of parameters are ACCUMULATED into caller-zeroed fp32
// buffers (atomics in the reduction kernels); activation gradients travel in the compute dtype, the residual-stream
// gradient in fp32.
#include <stdio.h>
#include <stdlib.h>

#include "ttv_common.h"
#include "ttv_kernels.h"

struct Tape {
  char* base;
  int64_t total;
  // per tower
  char *patches, *pe, *hpre, *pn;     // encoder: gathered patches, proj_in output (pre-norm); decoder: pre-norm latent rows, ln_post out
  char* X[65];                        // residual stream at every layer boundary (X[0] = tower input rows, X[layers] = output)
  struct L { char *xn1, *qkvg, *a, *ag, *x1, *xn2, *u, *h, *y1, *y2; float* lse; } l[64];   // y1 / y2: the KEEL sums, dtype tape_y_dtype()
  char *agc, *xc;                     // encoder, last layer: its latent rows of ag and of X[layers - 1], compact (see latent_tail)
};

// The KEEL sums y = alpha * x + f(x) the post-norms read (forward) and differentiate (backward) are kept in the tower's dtype: a bf16
// tower rounds them to bf16 as the reference's autocast does (transformer.py:141: bf16 * alpha + bf16) and as the inference path does -
// half the bytes on the GEMM that writes them, the norm that reads them and the backward chain (round 5; fp32 before).  The opt-in
// fused-norm tape forward (TTV_TRAIN_FUSED_NORMS=1) writes fp32 sums from its GEMM kernel and keeps fp32.
static bool tape_fuse_norms() {
  static const bool v = ttv_env_flag("TTV_TRAIN_FUSED_NORMS", false);
  return v;
}
static int tape_y_dtype(int dt) {
  static const bool f32 = ttv_env_flag("TTV_TAPE_Y_F32", false);      // A/B: fp32 sums as before round 5
  return (dt == TTV_F32 || tape_fuse_norms() || f32) ? TTV_F32 : TTV_BF16;
}
// tape_mode TTV_TAPE_STORED: one region per layer (layer 0 has no y1 / y2).  TTV_TAPE_RECOMPUTE: min(2, layers) layer SLOTS of the size
// of a layer > 0 instead; t.l[i] is slot i & 1 for every i, so the forward and the backward address a layer's tape the same way in both
// modes and only WHEN a slot holds which layer differs (layers_forward_train, layers_backward).
static bool tape_mode_ok(int tape_mode) { return tape_mode == TTV_TAPE_STORED || tape_mode == TTV_TAPE_RECOMPUTE; }
static Tape carve_tape(const ttv_tower_dims* d, const ttv_batch* b, char* base, int tape_mode) {
  Tape t;
  const int64_t ye = dtype_bytes(tape_y_dtype(d->dtype));
  const int64_t e = dtype_bytes(d->dtype), L = b->total_rows, P = b->sum_patches, K = b->sum_tokens, dm = d->width;
  const int64_t g = (int64_t)d->kv_heads * d->head_dim, nq = 2 * dm + 2 * g;
  const int64_t pd = patch_dim(d);
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  t.base = base;
  t.patches = t.pe = t.hpre = t.pn = nullptr;
  t.agc = t.xc = nullptr;
  if (d->kind == TTV_ENCODER) { t.patches = take(P * pd * e); t.pe = take(P * dm * e); t.agc = take(K * dm * e); t.xc = take(K * dm * e); }
  else { t.hpre = take(K * dm * e); t.pn = take(P * dm * e); }
  for (int i = 0; i <= d->layers; ++i) t.X[i] = take(L * dm * e);
  const bool slots = tape_mode == TTV_TAPE_RECOMPUTE;
  const int regions = slots ? (d->layers < 2 ? d->layers : 2) : d->layers;
  for (int i = 0; i < regions; ++i) {
    Tape::L& l = t.l[i];
    const bool y = slots || i > 0;          // a slot takes any layer
    l.xn1 = take(L * dm * e); l.qkvg = take(L * nq * e); l.lse = (float*)take(L * d->q_heads * 4);
    l.a = take(L * dm * e); l.ag = take(L * dm * e);
    l.y1 = take(y ? L * dm * ye : 0); l.x1 = take(L * dm * e); l.xn2 = take(L * dm * e);
    l.u = take(L * 2 * d->inner * e); l.h = take(L * d->inner * e); l.y2 = take(y ? L * dm * ye : 0);
  }
  for (int i = regions; i < d->layers; ++i) t.l[i] = t.l[i & 1];
  t.total = off;
  return t;
}

struct BwdWs {
  float *dxa, *dxb, *delta, *dkv, *colsum, *small_f32;
  float* dxc;       // [sum_tokens, width] fp32: the latent rows of the residual-stream gradient, compact (encoder, last layer)
  char *g_d, *g_d2, *g_i, *g_2i, *g_nq, *g_pd;
  char *g_df2, *g_do;   // [L, width]: the second df buffer (layers alternate) and do - operands the weight-gradient stream may still read
  float* wg_part;
  int64_t wg_part_bytes;
  DetScratch det;   // deterministic mode only: the block partials of the row reductions (every launch of the caller's stream in turn)
  int64_t total;
};
static BwdWs carve_bwd(const ttv_tower_dims* d, const ttv_batch* b, char* base) {
  BwdWs w;
  const int64_t e = dtype_bytes(d->dtype), L = b->total_rows, P = b->sum_patches, dm = d->width;
  const int64_t g = (int64_t)d->kv_heads * d->head_dim, nq = 2 * dm + 2 * g;
  const int64_t pd = patch_dim(d);
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  w.dxa = (float*)take(L * dm * 4); w.dxb = (float*)take(L * dm * 4);
  w.delta = (float*)take(L * d->q_heads * 4);
  w.dkv = (float*)take(d->dtype == TTV_F32 ? L * 2 * g * 4 : 0);
  w.colsum = (float*)take(dm * 4);
  w.small_f32 = (float*)take(L * dm * 4);          // fp32 [rows, d] scratch for the d <-> token_size projections
  w.dxc = (float*)take((int64_t)b->sum_tokens * dm * 4);
  w.g_d = take(L * dm * e); w.g_d2 = take(L * dm * e); w.g_i = take(L * d->inner * e); w.g_2i = take(L * 2 * d->inner * e);
  w.g_nq = take(L * nq * e); w.g_pd = take(P * pd * e);
  w.g_df2 = take(L * dm * e); w.g_do = take(L * dm * e);
  // split partial tiles of the weight-gradient GEMMs (largest of the shapes the tower uses)
  int64_t wgb = 0;
  if (d->dtype == TTV_BF16) {
    // the four weight gradients of a layer keep their partial tiles side by side and are summed by one launch (WgradBatch): room for
    // their SUM; the head / tail projections run on their own (largest single shape)
    const int64_t shapes[6][3] = {{L, dm, d->inner}, {L, 2 * d->inner, dm}, {L, dm, dm}, {L, nq, dm}, {P, dm, pd}, {P, pd, dm}};
    int64_t layer_sum = 0;
    for (int i = 0; i < 6; ++i) {
      const int64_t v = ttvk_wgrad_ws_bytes((int)shapes[i][0], (int)shapes[i][1], (int)shapes[i][2]);
      if (i < 4) layer_sum += v;
      wgb = v > wgb ? v : wgb;
    }
    wgb = layer_sum > wgb ? layer_sum : wgb;
  }
  w.wg_part = (float*)take(wgb); w.wg_part_bytes = wgb;
  // Deterministic mode: room for the largest partial array among the backward's reductions.  They all run on the caller's stream (the
  // weight-gradient stream adds into the four weight matrices of a layer and nothing else), one after the other, and each launch's fold
  // is ordered in front of the next launch's partials.  Mode off: no bytes, the size is what it was.
  int64_t db = 0;
  if (ttv_det()) {
    const int C = d->token_size, K = b->sum_tokens;
    const int rows3[3] = {(int)L, (int)P, K};
    for (int i = 0; i < 3; ++i) {
      const int64_t v = 2 * ttvk_det_rms_bytes(rows3[i], (int)dm);      // the chain kernel: two gains
      db = v > db ? v : db;
    }
    const int64_t nmax = pd > dm ? pd : dm;
    const int64_t cand[3] = {ttvk_det_colsum_bytes((int)L, (int)(nmax > C ? nmax : C)), ttvk_det_sumall_bytes((long)L * dm),
                             ttvk_det_outer_small_bytes(K, C, (int)dm)};
    for (int i = 0; i < 3; ++i) db = cand[i] > db ? cand[i] : db;
  }
  w.det.p = take(db); w.det.bytes = db;
  w.total = off;
  return w;
}

static int check(const ttv_tower_dims* d, const ttv_batch* b, int tape_mode) {
  TTV_CHECK_ARG(tape_mode_ok(tape_mode), "tape mode %d is neither TTV_TAPE_STORED nor TTV_TAPE_RECOMPUTE", tape_mode);
  // the fused-norm forward writes a layer's xn1 from the GEMM of the layer below; a rebuilt layer would form its own, other bits
  TTV_CHECK_ARG(tape_mode != TTV_TAPE_RECOMPUTE || !tape_fuse_norms(), "TTV_TAPE_RECOMPUTE does not combine with TTV_TRAIN_FUSED_NORMS=1");
  TTV_CHECK_ARG(d && b, "null dims/batch");
  TTV_CHECK_ARG(d->dtype == TTV_BF16 || d->dtype == TTV_F32, "bad dtype");
  TTV_CHECK_ARG(d->layers >= 1 && d->layers <= 64, "layers out of range");
  TTV_CHECK_ARG(d->head_dim == 64 && d->width == d->q_heads * 64 && d->width <= 1024, "width must be q_heads*64 <= 1024");
  TTV_CHECK_ARG(b->blocks64 && b->row_seq, "training needs batch.blocks64 and batch.row_seq");
  TTV_CHECK_ARG(d->token_size >= 1 && d->token_size <= TTV_MAX_TOKEN, "training towers take token_size <= %d", TTV_MAX_TOKEN);
  return TTV_OK;
}

// The encoder's output is read from its latent rows only (blocks.py:101-103): in its LAST layer everything behind the attention - out_proj,
// the KEEL norms, the feed-forward - runs on the sum K_b latent rows, gathered into compact buffers; the tape entries of that sub-layer
// (x1, xn2, u, h, y1, y2) then hold those rows in their first sum K_b rows, and the backward gathers / scatters accordingly.  The gradient
// of the loss with respect to the last layer's patch-row outputs is zero, so nothing is lost; attention (forward and backward) still runs
// on every row - a query row with dO = 0 contributes nothing.  TTV_ENC_LATENT_LAST=0 / ttv_debug_set bit 19: every row (A/B, tests).
static bool latent_tail(const ttv_tower_dims* d, const ttv_batch* b, int layer) {
  return ttv_enc_latent_rows_only(d, b) && layer == d->layers - 1 && d->inner >= d->width;
}

// ... and the attention itself for the latent QUERY rows only (keys / values: every row), forward and backward, when the batch carries the
// latent work table and the clip descriptors (the backward derives K_b from them)
static bool latent_attn(const ttv_tower_dims* d, const ttv_batch* b, int layer) {
  return latent_tail(d, b, layer) && b->qblocks_latent && b->n_qblocks_latent > 0 && b->clip_desc;
}

// ------------------------------------------------------------------------------------------------ forward (tape)
// One layer: reads X[i], writes layer i's tape entries into `l` and X[i + 1] (encoder, last layer: its latent rows, through t.agc / t.xc).
// The stored tape calls it with t.l[i] once; the recompute tape calls it with the layer's slot in the forward (the slot is scratch there)
// and again from the backward - the same kernels with the same launch arguments on the same inputs, hence the same bits.
// xn1_ready (fused norms only): in, this layer's xn1 was written by the layer below; out, the next layer's was written by this one.
static int layer_forward_train(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, Tape& t, int i, Tape::L& l,
                               bool& xn1_ready, hipStream_t s) {
  const int L = b->total_rows, dm = d->width, g = d->kv_heads * d->head_dim, dt = d->dtype, nq = 2 * dm + 2 * g, I = d->inner;
  // Round 4, OPT-IN (TTV_TRAIN_FUSED_NORMS=1): where the fused residual + KEEL-norm GEMM applies (bf16, width 256) the post-norm, the fp32
  // pre-norm sum the backward needs AND the following pre-norm come out of the GEMM kernel (GemmArgs.sum_f32 / y2): 5 launches per layer
  // instead of 9, same tape.  Measured neutral (same box, tools/bench_train.py: 8.234 vs 8.236 ms at 32 clips, 3.47 vs 3.44 ms at 5): the
  // row-owning GEMM kernels lose against the tiled GEMM + 160-token tiles what the four row kernels cost, and the step is GPU-bound, not
  // launch-bound - so the proven sequence stays the default.  (It writes the NEXT layer's xn1, which a slot tape has no room for: the
  // recompute entry points refuse it.)
  const bool fuse_norms = tape_fuse_norms();
  const int ydt = tape_y_dtype(dt);
  const int64_t row_bytes = (int64_t)dm * dtype_bytes(dt);
  const ttv_layer_weights& lw = w->layers[i];
  const float alpha = keel_alpha(d, i);
  if (!xn1_ready) TTV_TRY(ttvk_rmsnorm(t.X[i], dt, dm, nullptr, l.xn1, dt, dm, nullptr, lw.pre_ln, L, dm, d->eps, s));
  xn1_ready = false;
  GemmArgs a = gemm_rope_qk(gemm_args(dt, l.xn1, dm, lw.to_qkv, dm, L, nq, dm, l.qkvg, nq), b->rope_cs, dm, g);
  a.rope_ids = b->rope_ids; a.rope_base = b->rope_ids ? b->rope_base : nullptr;
  TTV_TRY(ttvk_gemm(EPI_QKV_ROPE, a, s));
  // encoder, last layer: attention outputs are needed for the latent query rows only (latent_attn); the raw output of the other rows is
  // zeroed (the gate backward reads it for every row, times a zero gradient) and the backward skips those query rows too
  const bool lat_q = latent_attn(d, b, i);
  const int32_t* qb = lat_q ? b->qblocks_latent : b->qblocks;
  const int nqb = lat_q ? b->n_qblocks_latent : b->n_qblocks;
  const int pair = (!lat_q && b->qblocks_paired) ? TTV_ATTN_PAIRED : 0;
  if (lat_q) (void)hipMemsetAsync(l.a, 0, (size_t)L * dm * dtype_bytes(dt), s);
  if (dt == TTV_BF16) {
    // one launch writes the raw output a (tape) and the gated one ag = a * sigmoid(gate) (gate applied to the stored, rounded a)
    TTV_TRY(ttvk_attention(l.qkvg, nq, l.ag, dm, b->cu_seqlens, qb, nqb, d->q_heads, d->kv_heads, d->head_dim, TTV_ATTN_GATE | pair, dt, s, l.lse, l.a));
  } else {
    TTV_TRY(ttvk_attention(l.qkvg, nq, l.a, dm, b->cu_seqlens, qb, nqb, d->q_heads, d->kv_heads, d->head_dim, pair, dt, s, l.lse));
    TTV_TRY(ttvk_gate_fwd(l.a, dm, (const char*)l.qkvg + (size_t)dm * dtype_bytes(dt), nq, l.ag, dm, L, dm, dt, s));
  }
  // the rest of the layer on (Lc rows: ag_in, x_in): every row, or - encoder, last layer - the latent rows, compact
  const bool lat = latent_tail(d, b, i);
  const int Lc = lat ? b->sum_tokens : L;
  char* ag_in = l.ag;
  char* x_in = t.X[i];
  char* x_out = t.X[i + 1];
  if (lat) {
    TTV_TRY(gather_rows(l.ag, t.agc, b->latent_rows, Lc, row_bytes, s));
    TTV_TRY(gather_rows(t.X[i], t.xc, b->latent_rows, Lc, row_bytes, s));
    ag_in = t.agc; x_in = t.xc; x_out = t.xc;          // the layer's output: compact in place of its input rows, scattered below
  }
  // out_proj + residual: the sum into x1 (layer 0, and the fused route which norms it in the kernel) or into the tape's y1
  const bool o_fused = i > 0 && fuse_norms && ttvk_gemm_supports_resid_norm(dt, dm, dm);
  GemmArgs o = gemm_resid(gemm_args(dt, ag_in, dm, lw.out_proj, dm, Lc, dm, dm, (i == 0 || o_fused) ? l.x1 : l.y1, dm), x_in, dm, alpha);
  if (i == 0) {
    TTV_TRY(ttvk_gemm(EPI_RESID_T, o, s));
  } else if (o_fused) {
    o.norm_gain = lw.attn_post_ln; o.eps = d->eps;
    o.sum_f32 = (float*)l.y1; o.ld_sum = dm; o.y2 = l.xn2; o.ldy2 = dm; o.norm_gain2 = lw.ffd_norm;
    TTV_TRY(ttvk_gemm(EPI_RESID_NORM, o, s));
  } else {
    TTV_TRY(ttvk_gemm(ydt == TTV_F32 ? EPI_RESID_F32 : EPI_RESID_T, o, s));
    TTV_TRY(ttvk_rmsnorm(l.y1, ydt, dm, nullptr, l.x1, dt, dm, nullptr, lw.attn_post_ln, Lc, dm, d->eps, s));
  }
  if (!o_fused)
    TTV_TRY(ttvk_rmsnorm(l.x1, dt, dm, nullptr, l.xn2, dt, dm, nullptr, lw.ffd_norm, Lc, dm, d->eps, s));
  if (dt == TTV_BF16) {
    // one launch: u = xn2 W12^T kept for the backward (through `resid`, no alpha) and h = gelu(gate) * x from the stored values
    GemmArgs f = gemm_args(dt, l.xn2, dm, lw.w12, dm, Lc, I, dm, l.h, I);
    f.resid = l.u; f.ldr = 2 * I;
    TTV_TRY(ttvk_gemm(EPI_GEGLU, f, s));
  } else {
    TTV_TRY(ttvk_gemm(EPI_STORE, gemm_args(dt, l.xn2, dm, lw.w12, dm, Lc, 2 * I, dm, l.u, 2 * I), s));
    TTV_TRY(ttvk_geglu_fwd(l.u, 2 * I, l.h, I, Lc, I, dt, s));
  }
  // w3 + residual: as out_proj above, into the layer's output rows or the tape's y2
  const bool f3_fused = i > 0 && fuse_norms && ttvk_gemm_supports_resid_norm(dt, dm, I);
  GemmArgs f3 = gemm_resid(gemm_args(dt, l.h, I, lw.w3, I, Lc, dm, I, (i == 0 || f3_fused) ? x_out : l.y2, dm), l.x1, dm, alpha);
  if (i == 0) {
    TTV_TRY(ttvk_gemm(EPI_RESID_T, f3, s));
  } else if (f3_fused) {
    f3.norm_gain = lw.ffd_post_ln; f3.eps = d->eps;
    f3.sum_f32 = (float*)l.y2; f3.ld_sum = dm;
    if (i + 1 < d->layers) {          // the next layer's pre-norm rides along
      f3.y2 = t.l[i + 1].xn1; f3.ldy2 = dm; f3.norm_gain2 = w->layers[i + 1].pre_ln;
      xn1_ready = true;
    }
    TTV_TRY(ttvk_gemm(EPI_RESID_NORM, f3, s));
  } else {
    TTV_TRY(ttvk_gemm(ydt == TTV_F32 ? EPI_RESID_F32 : EPI_RESID_T, f3, s));
    TTV_TRY(ttvk_rmsnorm(l.y2, ydt, dm, nullptr, x_out, dt, dm, nullptr, lw.ffd_post_ln, Lc, dm, d->eps, s));
  }
  if (lat)     // the latent rows of the tower's output where the tail (and the backward) read them; its patch rows are never read
    TTV_TRY(scatter_rows(t.xc, t.X[i + 1], b->latent_rows, Lc, row_bytes, s));
  return TTV_OK;
}
static int layers_forward_train(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, Tape& t, hipStream_t s) {
  bool xn1_ready = false;
  for (int i = 0; i < d->layers; ++i) TTV_TRY(layer_forward_train(d, w, b, t, i, t.l[i], xn1_ready, s));
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------ weight-gradient stream
// The weight-gradient GEMMs of a layer (dW = dY^T X, four per layer, plus the launch that sums their split partial tiles) are off the
// backward's critical path: nothing of the layer reads them.  They run on a second HIP stream, forked from the caller's stream by an event
// behind the producer of each dY and joined at the end of the layer, so that their launch tails and partly filled rounds overlap the
// dX chain (and, at the reference's 5-clip batches, their launch latencies).  The caller's stream stays the only one the caller sees:
// every fork is an event recorded on it, the join makes it wait - legal inside a HIP-graph capture of the step as well.
// Operands the second stream reads are not overwritten before the join (df alternates between two buffers, do / da have their own).
// TTV_WGRAD_SIDE=0: everything on the caller's stream (A/B).
struct WgradSide {
  hipStream_t w = nullptr;
  hipEvent_t fork[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t join = nullptr;
  int state = 0;   // 0 not tried, 1 ready, -1 unavailable
};
static WgradSide* wgrad_side(bool dp) {
  // 1 (default): on, also with the DP path's per-layer events attached; 0: never; 3: single-process steps only.  (For a while the DP
  // path kept the one-stream backward after a red run of the two-rank test; that run turned out to be the test's own tolerance - an
  // AdamW update of a near-zero gradient element is rounding noise - and showed up again with this stream off: DESIGN 5b.)
  static const int mode = ttv_env_int("TTV_WGRAD_SIDE", 1);
  if (mode <= 0 || (dp && mode == 3)) return nullptr;
  static thread_local WgradSide tab[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  WgradSide& sd = tab[dev];
  if (sd.state == 0) {
    sd.state = -1;
    if (hipStreamCreateWithFlags(&sd.w, hipStreamNonBlocking) != hipSuccess) return nullptr;
    for (int i = 0; i < 4; ++i)
      if (hipEventCreateWithFlags(&sd.fork[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&sd.join, hipEventDisableTiming) != hipSuccess) return nullptr;
    sd.state = 1;
  }
  return sd.state == 1 ? &sd : nullptr;
}
// the second stream takes up the caller's stream at this point
static int side_fork(WgradSide* sd, int k, hipStream_t s) {
  if (!sd) return TTV_OK;
  if (hipEventRecord(sd->fork[k], s) != hipSuccess || hipStreamWaitEvent(sd->w, sd->fork[k], 0) != hipSuccess) {
    ttv_set_error("backward: fork of the weight-gradient stream failed");
    return TTV_ERR_LAUNCH;
  }
  return TTV_OK;
}
static int side_join(WgradSide* sd, hipStream_t s) {
  if (!sd) return TTV_OK;
  if (hipEventRecord(sd->join, sd->w) != hipSuccess || hipStreamWaitEvent(s, sd->join, 0) != hipSuccess) {
    ttv_set_error("backward: join of the weight-gradient stream failed");
    return TTV_ERR_LAUNCH;
  }
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------ backward (layers)
// On entry ws.dxa holds dL/dX[layers] (fp32); on exit ws.dxa holds dL/dX[0].
// TTV_TAPE_RECOMPUTE: t.l[i] is slot i & 1, and a layer's tape is rebuilt from X[i] by layer_forward_train before it is read.  The forward
// left its two top layers in the slots (it used the same alternation), so the first layer rebuilt is layers - 3.
static int layers_backward(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* b, Tape& t,
                           const ttv_tower_grads* gr, BwdWs& ws, int tape_mode, hipStream_t s) {
  const int L = b->total_rows, dm = d->width, g = d->kv_heads * d->head_dim, dt = d->dtype, nq = 2 * dm + 2 * g, I = d->inner;
  const int ydt = tape_y_dtype(dt);
  float* dx = ws.dxa;     // gradient of the layer output
  float* tmp = ws.dxb;
  WgradBatch wgb;
  char* g_df[2] = {ws.g_d, ws.g_df2};   // df of this layer / da of this layer, then df of the layer below
  int cur = 0;
  for (int i = d->layers - 1; i >= 0; --i) {
    const ttv_layer_weights& lw = w->layers[i];
    const ttv_layer_weights_t& lt = wt->layers[i];
    const ttv_layer_grads& lg = gr->layers[i];
    Tape::L& l = t.l[i];
    // the layer's weight-gradient GEMMs and their summing launch: on the second stream (wgrad_side) when any is wanted
    WgradSide* sd = (lg.w3 || lg.w12 || lg.out_proj || lg.to_qkv) ? wgrad_side(gr->layer_done_events != nullptr) : nullptr;
    const hipStream_t sw = sd ? sd->w : s;
    char* const df = g_df[cur];
    char* const da = g_df[cur ^ 1];
    // ---------------- feed-forward sub-layer: X[i+1] = post_ln(alpha*x1 + w3 h)  (layer 0: x1 + w3 h) ----------------
    // The top layer undoes its feed-forward post-norm here; for the layers below it was chained onto the pre_ln backward of the
    // layer above (end of the previous iteration).
    // encoder, last layer: the sub-layers behind the attention ran on the latent rows only (latent_tail): their backward does too, on the
    // gathered latent rows of dL/dX[layers] (every other row of it is zero)
    const bool lat = latent_tail(d, b, i);
    const int Lc = lat ? b->sum_tokens : L;
    const long nLc = (long)Lc * dm;
    float* const dxf = dx;                 // the full-size gradient buffer
    if (lat) {
      TTV_TRY(gather_rows(dxf, ws.dxc, b->latent_rows, Lc, (int64_t)dm * 4, s));
      dx = ws.dxc;
    }
    float* dx1;
    if (i == d->layers - 1) {
      if (i > 0) {
        TTV_TRY(ttvk_rmsnorm_bwd(l.y2, ydt, dm, nullptr, dx, TTV_F32, dm, nullptr, lw.ffd_post_ln, tmp, TTV_F32, dm, nullptr, 0, lg.ffd_post_ln, Lc, dm, d->eps, s, &ws.det));
        // tmp = dy2 ; df (T) = dy2 ; dx1 = alpha * dy2 (into dx)
        TTV_TRY(ttvk_scale_cast(tmp, d->alpha, dx, df, dt, nLc, s));
      } else {
        TTV_TRY(ttvk_scale_cast(dx, 1.f, nullptr, df, dt, nLc, s));   // df = (T) dx ; dx1 = dx
      }
    }
    dx1 = dx;
    // dh = df W3 ; dW3 += df^T h
    TTV_TRY(side_fork(sd, 0, s));          // df is complete
    TTV_TRY(ttvk_gemm(EPI_STORE, gemm_args(dt, df, dm, lt.w3_t, dm, Lc, I, dm, ws.g_i, I), s));
    TTV_TRY(ttvk_wgrad(df, dm, l.h, I, lg.w3, I, Lc, dm, I, dt, ws.wg_part, ws.wg_part_bytes, sw, &wgb));
    TTV_TRY(ttvk_geglu_bwd(l.u, 2 * I, ws.g_i, I, ws.g_2i, 2 * I, Lc, I, dt, s));
    TTV_TRY(side_fork(sd, 1, s));          // du is complete
    // dxn2 = du W12 ; dW12 += du^T xn2
    TTV_TRY(ttvk_gemm(EPI_STORE, gemm_args(dt, ws.g_2i, 2 * I, lt.w12_t, 2 * I, Lc, dm, 2 * I, ws.g_d2, dm), s));
    TTV_TRY(ttvk_wgrad(ws.g_2i, 2 * I, l.xn2, dm, lg.w12, dm, Lc, 2 * I, dm, dt, ws.wg_part, ws.wg_part_bytes, sw, &wgb));
    // dx1 += rmsnorm_bwd(x1, ffd_norm, dxn2), then straight through the attention sub-layer's post-norm:
    // ---------------- attention sub-layer: x1 = post_ln(alpha*x + out_proj ag) ----------------
    // i > 0: dy1 = rmsnorm_bwd(y1, attn_post_ln, dx1) ; do = (T) dy1 ; dx = alpha * dy1      i == 0: do = (T) dx1 ; dx = dx1
    TTV_TRY(ttvk_rmsnorm_bwd_chain(l.x1, dm, ws.g_d2, dm, lw.ffd_norm, lg.ffd_norm, dx1, dm, i > 0 ? l.y1 : nullptr, ydt, dm,
                                   i > 0 ? lw.attn_post_ln : nullptr, i > 0 ? lg.attn_post_ln : nullptr, i > 0 ? d->alpha : 1.f, ws.g_do, dm, Lc,
                                   dm, d->eps, dt, s, &ws.det));
    TTV_TRY(side_fork(sd, 2, s));          // do is complete
    // dag = do Wo ; dWo += do^T ag
    TTV_TRY(ttvk_gemm(EPI_STORE, gemm_args(dt, ws.g_do, dm, lt.out_proj_t, dm, Lc, dm, dm, ws.g_d2, dm), s));
    TTV_TRY(ttvk_wgrad(ws.g_do, dm, lat ? t.agc : l.ag, dm, lg.out_proj, dm, Lc, dm, dm, dt, ws.wg_part, ws.wg_part_bytes, sw, &wgb));
    // back to every row: the gradient of the attention output and of the residual stream are zero outside the latent rows
    char* dag = ws.g_d2;
    const size_t es = dtype_bytes(dt);
    if (lat) {
      (void)hipMemsetAsync(ws.g_i, 0, (size_t)L * dm * es, s);
      TTV_TRY(scatter_rows(ws.g_d2, ws.g_i, b->latent_rows, Lc, (int64_t)dm * es, s));
      dag = ws.g_i;
      (void)hipMemsetAsync(dxf, 0, (size_t)L * dm * sizeof(float), s);
      TTV_TRY(scatter_rows(ws.dxc, dxf, b->latent_rows, Lc, (int64_t)dm * 4, s));
      dx = dxf;
    }
    // da = dag*sigmoid(gate) (into the df buffer this layer does not use) ; dgate -> dqkvg[:, d:2d]
    char* dqkvg = ws.g_nq;
    TTV_TRY(ttvk_gate_bwd(dag, dm, l.a, dm, (const char*)l.qkvg + (size_t)dm * es, nq, da, dm, dqkvg + (size_t)dm * es, nq, L, dm, dt,
                          ws.delta, s));   // also fills delta = sum_d da * a per (row, head) for the attention backward
    // attention backward -> dq, dk, dv columns of dqkvg
    TTV_TRY(ttvk_attention_bwd(l.qkvg, nq, l.a, dm, da, dm, l.lse, ws.delta, b->cu_seqlens, b->blocks64, b->n_blocks64, b->row_seq, dqkvg, nq,
                               ws.dkv, L, d->q_heads, d->kv_heads, dt, b->rope_cs, s, 1, latent_attn(d, b, i) ? b->clip_desc : nullptr));   // dq, dk come back un-rotated; delta from the gate backward
    // dxn1 = dqkvg Wqkv ; dWqkv += dqkvg^T xn1
    TTV_TRY(side_fork(sd, 3, s));          // dqkvg is complete
    TTV_TRY(ttvk_gemm(EPI_STORE, gemm_args(dt, dqkvg, nq, lt.to_qkv_t, nq, L, dm, nq, ws.g_d2, dm), s));
    TTV_TRY(ttvk_wgrad(dqkvg, nq, l.xn1, dm, lg.to_qkv, dm, L, nq, dm, dt, ws.wg_part, ws.wg_part_bytes, sw, &wgb));
    TTV_TRY(ttvk_wgrad_flush(&wgb, sw));     // the layer's four weight gradients: one summing launch
    // Recompute tape: the chain below reads y2 of layer i - 1, and the next iteration the rest of that layer's tape: rebuild it now, on
    // the caller's stream, into the OTHER slot.  That slot held layer i + 1, whose weight-gradient GEMMs - the only readers outside this
    // stream (h, xn2, ag, xn1) - were joined at the end of the previous iteration; this layer's own slot, which the second stream is
    // still reading, is not touched.  X[i] is rewritten with the bits it holds.
    if (tape_mode == TTV_TAPE_RECOMPUTE && i > 0 && i < d->layers - 1) {
      bool xn1_ready = false;
      TTV_TRY(layer_forward_train(d, w, b, t, i - 1, t.l[i - 1], xn1_ready, s));
    }
    // dx += rmsnorm_bwd(X[i], pre_ln, dxn1) = dL/dX[i]; chained with the head of the layer below: through its feed-forward
    // post-norm (layers >= 1) and the bf16 copy df that its w3 products read
    if (i == 0) {
      TTV_TRY(ttvk_rmsnorm_bwd(t.X[i], dt, dm, nullptr, ws.g_d2, dt, dm, nullptr, lw.pre_ln, dx, TTV_F32, dm, nullptr, 1, lg.pre_ln, L, dm, d->eps, s, &ws.det));
    } else {
      const bool post = i - 1 > 0;
      TTV_TRY(ttvk_rmsnorm_bwd_chain(t.X[i], dm, ws.g_d2, dm, lw.pre_ln, lg.pre_ln, dx, dm, post ? t.l[i - 1].y2 : nullptr, ydt, dm,
                                     post ? w->layers[i - 1].ffd_post_ln : nullptr, post ? gr->layers[i - 1].ffd_post_ln : nullptr,
                                     post ? d->alpha : 1.f, g_df[cur ^ 1], dm, L, dm, d->eps, dt, s, &ws.det));   // df of the layer below (da is consumed)
    }
    cur ^= 1;
    TTV_TRY(side_join(sd, s));             // the caller's stream takes the weight gradients back in; dY operands may be overwritten from here
    // every gradient of layer i is final here (its ffd_post_ln gain received its contribution in the iteration above)
    if (gr->layer_done_events && gr->layer_done_events[i]) {
      if (hipEventRecord((hipEvent_t)gr->layer_done_events[i], s) != hipSuccess) {
        ttv_set_error("backward: hipEventRecord(layer_done_events[%d]) failed", i);
        return TTV_ERR_LAUNCH;
      }
    }
  }
  return TTV_OK;
}

extern "C" {

int64_t ttv_tower_tape_bytes_ex(const ttv_tower_dims* dims, const ttv_batch* batch, int tape_mode) {
  if (!dims || !batch || !tape_mode_ok(tape_mode)) return -1;
  return carve_tape(dims, batch, nullptr, tape_mode).total;
}
int64_t ttv_tower_bwd_workspace_bytes_ex(const ttv_tower_dims* dims, const ttv_batch* batch, int tape_mode) {
  if (!dims || !batch || !tape_mode_ok(tape_mode)) return -1;
  return carve_bwd(dims, batch, nullptr).total;          // the recompute writes the tape only: one workspace for both modes
}
int64_t ttv_tower_tape_bytes(const ttv_tower_dims* dims, const ttv_batch* batch) {
  return ttv_tower_tape_bytes_ex(dims, batch, TTV_TAPE_STORED);
}
int64_t ttv_tower_bwd_workspace_bytes(const ttv_tower_dims* dims, const ttv_batch* batch) {
  return ttv_tower_bwd_workspace_bytes_ex(dims, batch, TTV_TAPE_STORED);
}

int ttv_fsq_backward(const ttv_fsq_params* p, const float* z, const void* dcodes, int dcodes_dtype, float* dz, int rows, void* stream) {
  TTV_CHECK_ARG(p && (rows == 0 || (z && dcodes && dz)), "fsq_backward: null buffer");
  return ttvk_fsq_bwd(p, z, dcodes, dcodes_dtype, dz, rows, (hipStream_t)stream);
}

// The tape's elementwise and small-projection ops one by one (tests): each is the launcher the towers call, argument checks included.
int ttv_gate_forward(const void* a, int lda, const void* gate, int ldg, void* ag, int ldo, int rows, int width, int dtype, void* stream) {
  TTV_CHECK_ARG(rows >= 0, "gate_forward: %d rows", rows);
  return ttvk_gate_fwd(a, lda, gate, ldg, ag, ldo, rows, width, dtype, (hipStream_t)stream);
}
int ttv_gate_backward(const void* dag, int lddag, const void* a, int lda, const void* gate, int ldg, void* da, int ldda, void* dgate,
                      int lddg, int rows, int width, int dtype, float* delta, void* stream) {
  TTV_CHECK_ARG(rows >= 0, "gate_backward: %d rows", rows);
  return ttvk_gate_bwd(dag, lddag, a, lda, gate, ldg, da, ldda, dgate, lddg, rows, width, dtype, delta, (hipStream_t)stream);
}
int ttv_geglu_forward(const void* u, int ldu, void* h, int ldh, int rows, int inner, int dtype, void* stream) {
  TTV_CHECK_ARG(rows >= 0, "geglu_forward: %d rows", rows);
  return ttvk_geglu_fwd(u, ldu, h, ldh, rows, inner, dtype, (hipStream_t)stream);
}
int ttv_geglu_backward(const void* u, int ldu, const void* dh, int lddh, void* du, int lddu, int rows, int inner, int dtype, void* stream) {
  TTV_CHECK_ARG(rows >= 0, "geglu_backward: %d rows", rows);
  return ttvk_geglu_bwd(u, ldu, dh, lddh, du, lddu, rows, inner, dtype, (hipStream_t)stream);
}
int ttv_scale_cast(const float* a, float alpha, float* b, void* c, int dtype, int64_t n, void* stream) {
  TTV_CHECK_ARG(n >= 0, "scale_cast: %lld elements", (long long)n);
  return ttvk_scale_cast(a, alpha, b, c, dtype, (long)n, (hipStream_t)stream);
}
int ttv_cast_to_f32(const void* a, int dtype, float* b, int64_t n, int accumulate, void* stream) {
  TTV_CHECK_ARG(n >= 0, "cast_to_f32: %lld elements", (long long)n);
  return ttvk_to_f32(a, dtype, b, (long)n, accumulate, (hipStream_t)stream);
}
int ttv_expand_small(const void* a, int a_dtype, int lda, int C, const void* w, int w_dtype, int ldw, int w_cf, void* out, int out_dtype,
                     int ldo, int rows, int width, void* stream) {
  TTV_CHECK_ARG(rows >= 0, "expand_small: %d rows", rows);
  return ttvk_expand_small(a, a_dtype, lda, C, w, w_dtype, ldw, w_cf, out, out_dtype, ldo, rows, width, (hipStream_t)stream);
}
int ttv_reduce_small(const void* a, int a_dtype, int lda, const int32_t* a_rows, const void* w, int w_dtype, int ldw, int C, float* out,
                     int ldo, int rows, int width, void* stream) {
  TTV_CHECK_ARG(rows >= 0, "reduce_small: %d rows", rows);
  return ttvk_reduce_small(a, a_dtype, lda, a_rows, w, w_dtype, ldw, C, out, ldo, rows, width, (hipStream_t)stream);
}
int ttv_const_rows_backward(const float* colsum, const float* mask_token, const float* gain, int dtype, float eps, float* dgain,
                            float* dmask, int width, void* stream) {
  return ttvk_const_rows_bwd(colsum, mask_token, gain, dtype, eps, dgain, dmask, width, (hipStream_t)stream);
}

int ttv_encoder_forward_train_ex(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const void* const* clips, float* z,
                                 void* tape, int64_t tape_bytes, void* stream, int tape_mode) {
  TTV_TRY(check(d, b, tape_mode));
  TTV_CHECK_ARG(d->kind == TTV_ENCODER && w && w->layers && clips && z && tape, "encoder_forward_train: bad argument");
  hipStream_t s = (hipStream_t)stream;
  Tape t = carve_tape(d, b, (char*)tape, tape_mode);
  TTV_CHECK_ARG(t.total <= tape_bytes, "encoder_forward_train: tape too small");
  const int dm = d->width, dt = d->dtype, P = b->sum_patches, pd = patch_dim(d);
  TTV_TRY(patch_copy_all(false, (void* const*)clips, d, b, t.patches, dt, s));
  GemmArgs a = gemm_args(dt, t.patches, pd, w->proj_in_w, pd, P, dm, pd, t.pe, dm);
  a.bias = w->proj_in_b; a.add_scalar = w->mask_token;
  TTV_TRY(ttvk_gemm(EPI_STORE, a, s));
  TTV_TRY(ttvk_rmsnorm(t.pe, dt, dm, nullptr, t.X[0], dt, dm, b->patch_rows, w->ln_pre_p, P, dm, d->eps, s));
  TTV_TRY(ttvk_fill_const_rows(t.X[0], dt, dm, b->latent_rows, b->sum_tokens, dm, w->mask_token, w->ln_pre_t, d->eps, s));
  TTV_TRY(layers_forward_train(d, w, b, t, s));
  TTV_TRY(ttvk_enc_tail(t.X[d->layers], dt, dm, b->latent_rows, b->sum_tokens, dm, w->ln_post, d->eps, w->proj_out_w, w->proj_out_b, d->token_size, nullptr, z, nullptr, nullptr, nullptr, s));
  return TTV_OK;
}

int ttv_encoder_forward_train(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const void* const* clips, float* z,
                              void* tape, int64_t tape_bytes, void* stream) {
  return ttv_encoder_forward_train_ex(d, w, b, clips, z, tape, tape_bytes, stream, TTV_TAPE_STORED);
}

int ttv_encoder_backward_ex(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* b, const float* dz,
                            void* tape, const ttv_tower_grads* gr, void* const* dclips, void* workspace, int64_t workspace_bytes, void* stream,
                            int tape_mode) {
  TTV_TRY(check(d, b, tape_mode));
  TTV_CHECK_ARG(d->kind == TTV_ENCODER && w && wt && wt->layers && (!gr || gr->layers) && dz && tape && workspace, "encoder_backward: bad argument");
  // grads == NULL: every parameter is frozen (generator step through the discriminator, loss_module.py:144-151) - only the
  // input-clip gradient is produced; all weight-gradient GEMMs, gain / bias reductions are skipped
  static const ttv_layer_grads no_layer_grads[64] = {};
  static const ttv_tower_grads no_grads = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, no_layer_grads};
  if (!gr) {
    TTV_CHECK_ARG(dclips, "encoder_backward: nothing to compute (no parameter and no input gradients requested)");
    gr = &no_grads;
  }
  hipStream_t s = (hipStream_t)stream;
  Tape t = carve_tape(d, b, (char*)tape, tape_mode);
  BwdWs ws = carve_bwd(d, b, (char*)workspace);
  TTV_CHECK_ARG(ws.total <= workspace_bytes, "encoder_backward: workspace too small");
  const int L = b->total_rows, dm = d->width, dt = d->dtype, P = b->sum_patches, K = b->sum_tokens, C = d->token_size, pd = patch_dim(d);
  // ---- tail: z = proj_out(n) + b, n = ln_post(X_last[latent rows]) ----
  TTV_TRY(ttvk_rmsnorm(t.X[d->layers], dt, dm, b->latent_rows, ws.g_d, dt, dm, nullptr, w->ln_post, K, dm, d->eps, s));   // n
  TTV_TRY(ttvk_outer_small(dz, TTV_F32, C, C, ws.g_d, dt, dm, nullptr, gr->proj_out_w, dm, 0, K, dm, s, &ws.det));
  TTV_TRY(ttvk_colsum(dz, TTV_F32, C, nullptr, K, C, gr->proj_out_b, s, &ws.det));
  TTV_TRY(ttvk_expand_small(dz, TTV_F32, C, C, w->proj_out_w, dt, dm, 1, ws.g_d2, dt, dm, K, dm, s));                      // dn
  (void)hipMemsetAsync(ws.dxa, 0, (size_t)L * dm * sizeof(float), s);
  TTV_TRY(ttvk_rmsnorm_bwd(t.X[d->layers], dt, dm, b->latent_rows, ws.g_d2, dt, dm, nullptr, w->ln_post, ws.dxa, TTV_F32, dm, b->latent_rows, 0, gr->ln_post, K, dm, d->eps, s, &ws.det));
  TTV_TRY(layers_backward(d, w, wt, b, t, gr, ws, tape_mode, s));
  // ---- head ----
  // latent rows are the constant vector ln_pre_t(mask_token * 1)
  (void)hipMemsetAsync(ws.colsum, 0, dm * sizeof(float), s);
  TTV_TRY(ttvk_colsum(ws.dxa, TTV_F32, dm, b->latent_rows, K, dm, ws.colsum, s, &ws.det));
  TTV_TRY(ttvk_const_rows_bwd(ws.colsum, w->mask_token, w->ln_pre_t, dt, d->eps, gr->ln_pre_t, gr->mask_token, dm, s));
  // patch rows: X0[patch] = ln_pre_p(pe), pe = proj_in(patches) + bias + mask_token
  TTV_TRY(ttvk_rmsnorm_bwd(t.pe, dt, dm, nullptr, ws.dxa, TTV_F32, dm, b->patch_rows, w->ln_pre_p, ws.g_d, dt, dm, nullptr, 0, gr->ln_pre_p, P, dm, d->eps, s, &ws.det));  // dpe
  TTV_TRY(ttvk_sumall(ws.g_d, dt, dm, nullptr, P, dm, nullptr, 1.f, gr->mask_token, s, &ws.det));
  TTV_TRY(ttvk_colsum(ws.g_d, dt, dm, nullptr, P, dm, gr->proj_in_b, s, &ws.det));
  TTV_TRY(ttvk_wgrad(ws.g_d, dm, t.patches, pd, gr->proj_in_w, pd, P, dm, pd, dt, ws.wg_part, ws.wg_part_bytes, s));
  if (dclips) {
    TTV_TRY(ttvk_gemm(EPI_STORE, gemm_args(dt, ws.g_d, dm, wt->proj_in_t, dm, P, pd, dm, ws.g_pd, pd), s));
    TTV_TRY(patch_copy_all(true, dclips, d, b, ws.g_pd, dt, s));
  }
  return TTV_OK;
}

int ttv_encoder_backward(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* b, const float* dz,
                         void* tape, const ttv_tower_grads* gr, void* const* dclips, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttv_encoder_backward_ex(d, w, wt, b, dz, tape, gr, dclips, workspace, workspace_bytes, stream, TTV_TAPE_STORED);
}

int ttv_decoder_forward_train_ex(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const void* codes, void* const* clips_out,
                                 void* tape, int64_t tape_bytes, void* workspace, int64_t workspace_bytes, void* stream, int tape_mode) {
  TTV_TRY(check(d, b, tape_mode));
  TTV_CHECK_ARG(d->kind == TTV_DECODER && w && w->layers && codes && clips_out && tape && workspace, "decoder_forward_train: bad argument");
  hipStream_t s = (hipStream_t)stream;
  Tape t = carve_tape(d, b, (char*)tape, tape_mode);
  TTV_CHECK_ARG(t.total <= tape_bytes, "decoder_forward_train: tape too small");
  const int dm = d->width, dt = d->dtype, P = b->sum_patches, pd = patch_dim(d);
  TTV_CHECK_ARG((int64_t)P * pd * dtype_bytes(dt) <= workspace_bytes, "decoder_forward_train: workspace too small");
  TTV_TRY(ttvk_dec_embed_ex(codes, d->token_size, w->proj_in_w, w->proj_in_b, w->mask_token, w->ln_pre_t, t.X[0], dt, dm, b->latent_rows, b->sum_tokens, dm, d->eps, t.hpre, s));
  TTV_TRY(ttvk_fill_const_rows(t.X[0], dt, dm, b->patch_rows, P, dm, w->mask_token, w->ln_pre_p, d->eps, s));
  TTV_TRY(layers_forward_train(d, w, b, t, s));
  TTV_TRY(ttvk_rmsnorm(t.X[d->layers], dt, dm, b->patch_rows, t.pn, dt, dm, nullptr, w->ln_post, P, dm, d->eps, s));
  GemmArgs a = gemm_args(dt, t.pn, dm, w->proj_out_w, dm, P, pd, dm, workspace, pd);
  a.bias = w->proj_out_b;
  TTV_TRY(ttvk_gemm(EPI_STORE, a, s));
  return patch_copy_all(true, clips_out, d, b, workspace, dt, s);
}

int ttv_decoder_forward_train(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_batch* b, const void* codes, void* const* clips_out,
                              void* tape, int64_t tape_bytes, void* workspace, int64_t workspace_bytes, void* stream) {
  return ttv_decoder_forward_train_ex(d, w, b, codes, clips_out, tape, tape_bytes, workspace, workspace_bytes, stream, TTV_TAPE_STORED);
}

int ttv_decoder_backward_ex(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* b, const void* codes,
                            const void* const* dclips_out, void* tape, const ttv_tower_grads* gr, float* dcodes, void* workspace,
                            int64_t workspace_bytes, void* stream, int tape_mode) {
  TTV_TRY(check(d, b, tape_mode));
  TTV_CHECK_ARG(d->kind == TTV_DECODER && w && wt && wt->layers && gr && gr->layers && codes && dclips_out && tape && workspace, "decoder_backward: bad argument");
  hipStream_t s = (hipStream_t)stream;
  Tape t = carve_tape(d, b, (char*)tape, tape_mode);
  BwdWs ws = carve_bwd(d, b, (char*)workspace);
  TTV_CHECK_ARG(ws.total <= workspace_bytes, "decoder_backward: workspace too small");
  const int L = b->total_rows, dm = d->width, dt = d->dtype, P = b->sum_patches, K = b->sum_tokens, C = d->token_size, pd = patch_dim(d);
  // ---- tail: clips = unpatch(proj_out(pn) + bias), pn = ln_post(X_last[patch rows]) ----
  TTV_TRY(patch_copy_all(false, (void* const*)dclips_out, d, b, ws.g_pd, dt, s));
  TTV_TRY(ttvk_colsum(ws.g_pd, dt, pd, nullptr, P, pd, gr->proj_out_b, s, &ws.det));
  TTV_TRY(ttvk_wgrad(ws.g_pd, pd, t.pn, dm, gr->proj_out_w, dm, P, pd, dm, dt, ws.wg_part, ws.wg_part_bytes, s));
  TTV_TRY(ttvk_gemm(EPI_STORE, gemm_args(dt, ws.g_pd, pd, wt->proj_out_t, pd, P, dm, pd, ws.g_d2, dm), s));   // dpn
  (void)hipMemsetAsync(ws.dxa, 0, (size_t)L * dm * sizeof(float), s);
  TTV_TRY(ttvk_rmsnorm_bwd(t.X[d->layers], dt, dm, b->patch_rows, ws.g_d2, dt, dm, nullptr, w->ln_post, ws.dxa, TTV_F32, dm, b->patch_rows, 0, gr->ln_post, P, dm, d->eps, s, &ws.det));
  TTV_TRY(layers_backward(d, w, wt, b, t, gr, ws, tape_mode, s));
  // ---- head ----
  (void)hipMemsetAsync(ws.colsum, 0, dm * sizeof(float), s);
  TTV_TRY(ttvk_colsum(ws.dxa, TTV_F32, dm, b->patch_rows, P, dm, ws.colsum, s, &ws.det));
  TTV_TRY(ttvk_const_rows_bwd(ws.colsum, w->mask_token, w->ln_pre_p, dt, d->eps, gr->ln_pre_p, gr->mask_token, dm, s));
  // latent rows: X0[latent] = ln_pre_t(hpre), hpre = proj_in(codes) + bias + mask_token
  TTV_TRY(ttvk_rmsnorm_bwd(t.hpre, dt, dm, nullptr, ws.dxa, TTV_F32, dm, b->latent_rows, w->ln_pre_t, ws.small_f32, TTV_F32, dm, nullptr, 0, gr->ln_pre_t, K, dm, d->eps, s, &ws.det));  // dh
  TTV_TRY(ttvk_sumall(ws.small_f32, TTV_F32, dm, nullptr, K, dm, nullptr, 1.f, gr->mask_token, s, &ws.det));
  TTV_TRY(ttvk_colsum(ws.small_f32, TTV_F32, dm, nullptr, K, dm, gr->proj_in_b, s, &ws.det));
  TTV_TRY(ttvk_outer_small(codes, dt, C, C, ws.small_f32, TTV_F32, dm, nullptr, gr->proj_in_w, C, 1, K, dm, s, &ws.det));
  if (dcodes) TTV_TRY(ttvk_reduce_small(ws.small_f32, TTV_F32, dm, nullptr, w->proj_in_w, dt, C, C, dcodes, C, K, dm, s));
  return TTV_OK;
}

int ttv_decoder_backward(const ttv_tower_dims* d, const ttv_tower_weights* w, const ttv_tower_weights_t* wt, const ttv_batch* b, const void* codes,
                         const void* const* dclips_out, void* tape, const ttv_tower_grads* gr, float* dcodes, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  return ttv_decoder_backward_ex(d, w, wt, b, codes, dclips_out, tape, gr, dcodes, workspace, workspace_bytes, stream, TTV_TAPE_STORED);
}

int64_t ttv_linear_wgrad_workspace_bytes(int L, int N, int K) { return ttvk_wgrad_ws_bytes(L, N, K); }

int ttv_linear_wgrad(const void* dy, int lddy, const void* x, int ldx, float* dw, int lddw, int L, int N, int K, int dtype, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  TTV_CHECK_ARG(L == 0 || (dy && x && dw), "linear_wgrad: null buffer");
  TTV_CHECK_ARG(workspace_bytes >= 0 && (workspace || workspace_bytes == 0), "linear_wgrad: bad workspace");
  return ttvk_wgrad(dy, lddy, x, ldx, dw, lddw, L, N, K, dtype, (float*)workspace, workspace_bytes, (hipStream_t)stream);
}

int ttv_rmsnorm_backward_chain(const void* x, int ldx, const void* dy, int lddy, const float* gain1, float* dgain1, float* dx, int lddx,
                               const float* y, int ldy, const float* gain2, float* dgain2, float out_scale, void* cast_out, int ldc, int rows,
                               int width, float eps, int dtype, void* stream) {
  TTV_CHECK_ARG(!ttv_det(), "rmsnorm_backward_chain: deterministic mode is on and this entry point has no scratch for the block partials: call ttv_rmsnorm_backward_chain_det");
  TTV_CHECK_ARG(rows == 0 || (x && dy && gain1 && dx), "rmsnorm_backward_chain: null buffer");
  return ttvk_rmsnorm_bwd_chain(x, ldx, dy, lddy, gain1, dgain1, dx, lddx, y, TTV_F32, ldy, gain2, dgain2, out_scale, cast_out, ldc, rows, width, eps,
                                dtype, (hipStream_t)stream, nullptr);      // mode off (checked above): no partials
}

int ttv_rmsnorm_backward(const void* x, int ldx, const void* dy, int lddy, const float* gain, void* dx, int lddx, float* dgain, int rows,
                         int width, float eps, int dtype, void* stream) {
  TTV_CHECK_ARG(!ttv_det(), "rmsnorm_backward: deterministic mode is on and this entry point has no scratch for the block partials: call ttv_rmsnorm_backward_det");
  TTV_CHECK_ARG(rows == 0 || (x && dy && gain && dx), "rmsnorm_backward: null buffer");
  return ttvk_rmsnorm_bwd(x, dtype, ldx, nullptr, dy, dtype, lddy, nullptr, gain, dx, dtype, lddx, nullptr, 0, dgain, rows, width, eps, (hipStream_t)stream,
                          nullptr);      // mode off (checked above): no partials
}

int64_t ttv_rmsnorm_backward_det_scratch_bytes(int rows, int width) {
  if (rows < 0 || width < 4 || width % 4 != 0 || width > 1024) { ttv_set_error("rmsnorm_backward_det_scratch_bytes: %d rows of width %d", rows, width); return -1; }
  return ttvk_det_rms_bytes(rows, width);
}
int64_t ttv_rmsnorm_backward_chain_det_scratch_bytes(int rows, int width) {
  const int64_t one = ttv_rmsnorm_backward_det_scratch_bytes(rows, width);
  return one < 0 ? one : 2 * one;
}

int ttv_rmsnorm_backward_chain_det(const void* x, int ldx, const void* dy, int lddy, const float* gain1, float* dgain1, float* dx, int lddx,
                                   const float* y, int ldy, const float* gain2, float* dgain2, float out_scale, void* cast_out, int ldc, int rows,
                                   int width, float eps, int dtype, void* scratch, int64_t scratch_bytes, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (x && dy && gain1 && dx), "rmsnorm_backward_chain_det: null buffer");
  const DetScratch det = {scratch, scratch_bytes};
  return ttvk_rmsnorm_bwd_chain(x, ldx, dy, lddy, gain1, dgain1, dx, lddx, y, TTV_F32, ldy, gain2, dgain2, out_scale, cast_out, ldc, rows, width, eps,
                                dtype, (hipStream_t)stream, &det);
}

int ttv_rmsnorm_backward_det(const void* x, int ldx, const void* dy, int lddy, const float* gain, void* dx, int lddx, float* dgain, int rows,
                             int width, float eps, int dtype, const int32_t* x_rows, const int32_t* dy_rows, const int32_t* dx_rows, void* scratch,
                             int64_t scratch_bytes, void* stream) {
  TTV_CHECK_ARG(rows == 0 || (x && dy && gain && dx), "rmsnorm_backward_det: null buffer");
  const DetScratch det = {scratch, scratch_bytes};
  return ttvk_rmsnorm_bwd(x, dtype, ldx, x_rows, dy, dtype, lddy, dy_rows, gain, dx, dtype, lddx, dx_rows, 0, dgain, rows, width, eps, (hipStream_t)stream,
                          &det);
}

int ttv_attention_backward(const void* qkvg, int ld, const void* o, int ldo, const void* dout, int ldd, const float* lse, float* delta,
                           const int32_t* cu_seqlens, const int32_t* blocks64, int n_blocks64, const int32_t* row_seq, void* dqkvg,
                           int ldg, float* dkv_scratch, int total_rows, int q_heads, int kv_heads, int dtype, const float* rope_cs,
                           void* stream) {
  TTV_CHECK_ARG(total_rows == 0 || (qkvg && o && dout && lse && delta && cu_seqlens && blocks64 && dqkvg), "attention_backward: null buffer");
  return ttvk_attention_bwd(qkvg, ld, o, ldo, dout, ldd, lse, delta, cu_seqlens, blocks64, n_blocks64, row_seq, dqkvg, ldg, dkv_scratch,
                            total_rows, q_heads, kv_heads, dtype, rope_cs, (hipStream_t)stream);
}

int ttv_attention_backward_qlim(const void* qkvg, int ld, const void* o, int ldo, const void* dout, int ldd, const float* lse, float* delta,
                                const int32_t* cu_seqlens, const int32_t* blocks64, int n_blocks64, const int32_t* row_seq, void* dqkvg,
                                int ldg, float* dkv_scratch, int total_rows, int q_heads, int kv_heads, int dtype, const float* rope_cs,
                                const int32_t* clip_desc, void* stream) {
  TTV_CHECK_ARG(total_rows == 0 || (qkvg && o && dout && lse && delta && cu_seqlens && blocks64 && dqkvg), "attention_backward_qlim: null buffer");
  return ttvk_attention_bwd(qkvg, ld, o, ldo, dout, ldd, lse, delta, cu_seqlens, blocks64, n_blocks64, row_seq, dqkvg, ldg, dkv_scratch,
                            total_rows, q_heads, kv_heads, dtype, rope_cs, (hipStream_t)stream, 0, clip_desc);
}

int ttv_attention_lse(const void* qkvg, int ld, void* out, int ldo, const int32_t* cu_seqlens, const int32_t* qblocks, int n_qblocks,
                      int q_heads, int kv_heads, int head_dim, int flags, int dtype, float* lse, void* stream) {
  TTV_CHECK_ARG(n_qblocks == 0 || (qkvg && out && cu_seqlens && qblocks), "attention_lse: null buffer");
  return ttvk_attention(qkvg, ld, out, ldo, cu_seqlens, qblocks, n_qblocks, q_heads, kv_heads, head_dim, flags, dtype, (hipStream_t)stream, lse);
}

}  // extern "C"
