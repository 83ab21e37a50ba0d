// ================================================================================================
// to_qkv of a width-256 tower, round 4 (included by ttv_gemm.hip behind k_gemm_k256, whose QKV instantiation it replaces):
// pre_ln + to_qkv + rotary, reference model/base/transformer.py:86-98.
//
// Same decomposition as k_gemm_k256 - 4 waves, a wave keeps its 32 tokens x 256 k in registers, 64-row weight panels stream
// L2 -> LDS by LDS-DMA into two 32 KiB stages (the SAME swizzled image), blocks walk contiguous (token tile, panel) items - but
// everything a wave does besides its MFMAs is cut into slices that ride BETWEEN the MFMAs of an item, one k-step (two MFMAs) per
// scheduling region.  In-kernel stamps of the phase-structured loop (tools/qkv256_stamps.sh, profiles/r04_qkv256_stamps.txt): of
// ~4 000 cycles per item and wave only ~1 900 were the MFMA phase (two waves share a SIMD's matrix pipe: 2 x 1 024); the eight DMA
// instructions of the next panel took ~780 cycles to be accepted, the four stores ~500, the wait for the DMA and the barrier ~700, and a
// token-tile change cost a wave 9 000 - 17 000 cycles (all blocks fetch their rows at once and compute nothing meanwhile).  Hence:
//   * MFMA shape 32x32x16 (feature rows x 32 tokens): 32 MFMAs of 32 cycles per item instead of 64 of 16 - the same matrix-pipe
//     time, half the issue-port hold - and a lane owns 32 outputs of ONE token;
//   * double-buffered accumulators: the epilogue arithmetic of item i-1 (rotary with rstd folded into the factors, or the row scale;
//     bf16 pack; exchange with lane ^ 32) rides under item i's MFMAs, group by group, and each 16-byte chunk is stored as soon as
//     it is complete (k-steps 3, 7, 11, 15);
//   * the next panel's eight DMA instructions are issued one per k-step in the first half of the item, so they are accepted while
//     MFMAs run and have landed when the item ends; the wait for them is COUNTED (three stores are younger than the last DMA
//     instruction: vmcnt(3)), so stores stay in flight across the barrier;
//   * after a token-tile change the first item's MFMA of k-step ks waits only for the row fragment ks (the compiler's counted
//     vmcnt), the row's sum of squares (v_dot2c_f32_bf16 on the packed fragments) rides under that item's MFMAs, the rotary-factor
//     gathers are issued in its middle, and rstd / the folded factors are finished behind it - they are first needed by the epilogue
//     of that item, which rides under the NEXT one.
// Output layout per store instruction: lane (r, h) writes features 32t + 16gp + 8h .. + 7 of token r: lanes r and r + 32 exchange one
// packed 4-feature group per pair with v_permlane32_swap (C layout of the 32x32 MFMA: rows 8(j>>2) + 4h + (j&3)).
// Results are bit-identical to k_gemm_k256<EPI_QKV_ROPE> without the folded pre-norm (same products, same k order, same rotary
// arithmetic; tools/qkv256_bench.py); with it, rstd comes from another summation order and multiplies the factors instead of the sums.
// ================================================================================================
// Diagnostic build -DQKV_STAMPS (tools/qkv256_stamps.sh): s_memtime at the segment boundaries of a step, summed per wave over its items;
// every 16th block writes stamps[((block / 16) * 4 + wave) * 8 + segment]: 0 token-tile change (row loads issued, owed epilogue),
// 1 first-panel wait, 2 the item body (32 MFMAs + everything riding), 3 the body of a tile's first item + finishing rstd / factors,
// 4 counted wait, 5 barrier, 6 the block's last epilogue, 7 = items.
#ifdef QKV_STAMPS
#define QK_STAMP_DECL unsigned long long qst_prev__ = 0, qst_acc__[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define QK_STAMP_START()                                                                                     \
  do {                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(qst_prev__)::"memory");                       \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
  } while (0)
#define QK_STAMP(seg_)                                                                                       \
  do {                                                                                                       \
    unsigned long long t__;                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");                              \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    qst_acc__[seg_] += t__ - qst_prev__;                                                                     \
    qst_prev__ = t__;                                                                                        \
  } while (0)
#else
#define QK_STAMP_DECL
#define QK_STAMP_START()
#define QK_STAMP(seg_)
#endif
typedef unsigned qk_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned qk_u32x2 __attribute__((ext_vector_type(2)));
// FLOOR (GemmDev.panel_lo > 0, with a tile list): EVERY token tile is an item tile, and the tiles behind the first tile_run of a period
// get the panels panel_lo .. n_panels - 1 only - the k | v columns of rows whose q | gate nobody reads (the encoder's last layer: queries
// are the latent rows).  Only the item -> (token tile, panel) map differs: it is stepped, not divided, from the block's first item on.
template <bool PRENORM, bool FLOOR>
__global__ __launch_bounds__(256, 2) void k_qkv256(GemmDev p, int n_panels, int total_items) {
  __shared__ uint4 wl[2][K256_ROWS * 32];  // [stage][row * 32 + swizzled 16-byte chunk]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int it0 = (int)((long)total_items * lb / gridDim.x);
  const int it1 = (int)((long)total_items * (lb + 1) / gridDim.x);
  if (it0 >= it1) return;
  const bf16_t* X = (const bf16_t*)p.x;

  // ---- panel staging (k_gemm_k256's image: wave w stages rows 16w .. 16w+15, two 512-byte rows per instruction) ----
  const uint32_t wl_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&wl[0][0];
  // Instruction i of a wave covers panel rows 16w + 2i + h (h = lane >> 5), lane & 31 = LDS chunk; the DMA writes lanes linearly, so the
  // swizzle is applied on the source: LDS chunk c holds global chunk (c & 16) | ((c & 15) ^ (row & 15)), and row & 15 = 2i + h, i.e.
  // ((c & 15) ^ h) ^ 2i: one lane constant (chunk bytes of i = 0), the 2i by XOR (bits 5-7 of the byte offset), the row by the scalar base.
  const uint32_t dchunk0 = (uint32_t)(((lane & 16) | ((lane & 15) ^ h)) * 16);
  const uint32_t drow0 = (uint32_t)h * (uint32_t)p.ldw * 2u;
  const uint32_t dstride = (uint32_t)p.ldw * 4u;          // two panel rows
  // one DMA instruction (1 KiB of the wave's 8 KiB share): src_ = scalar base of the wave's share of the panel, dst_ = its LDS byte address
#define QK_DMA_PIECE(dc_, i_, src_, dst_)                                                                       \
  do {                                                                                                       \
    unsigned keep__;                                                                                         \
    const uint32_t voff__ = ((dc_) ^ (uint32_t)((i_) << 5)) + drow0;                                            \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep__) : "v"(voff__), "s"((src_) + (size_t)(i_) * dstride), "s"((dst_) + (i_) * 1024) : "memory"); \
  } while (0)
#define QK_PANEL_SRC(panel_) (reinterpret_cast<const char*>(p.w) + ((size_t)(panel_) * 64 + wave * 16) * (size_t)p.ldw * 2)
#define QK_PANEL_DST(buf_) (wl_lds + (buf_) * (K256_ROWS * 512) + wave * (16 * 512))

  // ---- A fragment (weights) read addresses: row 32t + r, logical chunk 2ks + h; eight lane constants, the rest immediates ----
  const int r15 = r & 15;
  const char* const wl_base = reinterpret_cast<const char*>(&wl[0][0]);
  const uint32_t aoff0 = (uint32_t)(r * 32 + (h ^ r15)) * 16u;     // chunk (2k + h) ^ r15 = (h ^ r15) ^ 2k: bits 5-7 of the byte offset
#define QK_AFRAG(buf_, t_, ks_) \
  (*reinterpret_cast<const bf16x8*>(wl_base + (a0__ ^ (uint32_t)(((ks_) & 7) << 5)) + (buf_) * (K256_ROWS * 512) + (t_) * (32 * 512) + (((ks_) >> 3) & 1) * 256))

  bf16x8 bfr[16];          // the wave's 32 tokens x 256 k as B fragments: token r, k = 16 ks + 8 h .. + 7
  float rstd = 1.f;
  float2 rcs[2][4][2];     // (cos, sin) * rstd of pairs 16t + 4g + 2h + e2 of a 64-wide head, for token r
  char* ytok = nullptr;    // &y[token][8 h]
  uint2 idp = make_uint2(0u, 0u);   // the token's position ids (rotary factors by id)
  int tk = 0;              // the lane's (clamped) token row
  bool tok_ok = true, wave_full = true;
  int cur_tile = -1;
  int pend = 0;            // epilogue owed for the previous item: 0 none, 1 plain panel, 2 rotary panel
  int pend_panel = 0;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // ---- epilogue arithmetic of one item, cut into the slices that ride between the MFMAs of the next one ----
  // group G = 4t + g (t: 32-feature half of the panel, g: the lane's g-th run of four consecutive features, 8g + 4h .. + 3):
  //   QK_ROT(G)  : rotary (or row scale) of the group's four values            8 (4) vector instructions
  //   QK_PACK(G) : bf16 pack; for odd g the exchange with lane ^ 32             2 + 2
  // o_, pk_, out_ are temporaries of the enclosing body (literal indices after unrolling).
#define QK_ROT(acc_, ROT_, G_)                                                                               \
  do {                                                                                                       \
    const int t__ = (G_) >> 2, g__ = (G_) & 3;                                                               \
    const float a0__ = acc_[t__][4 * g__], a1__ = acc_[t__][4 * g__ + 1], a2__ = acc_[t__][4 * g__ + 2], a3__ = acc_[t__][4 * g__ + 3]; \
    if (ROT_) {                                                                                              \
      const float2 k0__ = rcs[t__][g__][0], k1__ = rcs[t__][g__][1];                                         \
      o_[0] = a0__ * k0__.x - a1__ * k0__.y; o_[1] = a0__ * k0__.y + a1__ * k0__.x;                          \
      o_[2] = a2__ * k1__.x - a3__ * k1__.y; o_[3] = a2__ * k1__.y + a3__ * k1__.x;                          \
    } else {                                                                                                 \
      o_[0] = a0__ * rstd; o_[1] = a1__ * rstd; o_[2] = a2__ * rstd; o_[3] = a3__ * rstd;                    \
    }                                                                                                        \
    asm volatile("" : "+v"(o_[0]), "+v"(o_[1]), "+v"(o_[2]), "+v"(o_[3]));                                   \
  } while (0)
#define QK_PACK(G_)                                                                                          \
  do {                                                                                                       \
    const int g__ = (G_) & 3;                                                                                \
    const bf16x4 b__ = {(bf16_t)o_[0], (bf16_t)o_[1], (bf16_t)o_[2], (bf16_t)o_[3]};                         \
    pk_[g__ & 1] = __builtin_bit_cast(qk_u32x2, b__);                                                        \
    if (g__ & 1) {                                                                                           \
      const auto sx__ = __builtin_amdgcn_permlane32_swap(pk_[0].x, pk_[1].x, false, false);                  \
      const auto sy__ = __builtin_amdgcn_permlane32_swap(pk_[0].y, pk_[1].y, false, false);                  \
      out_ = (qk_u32x4){sx__[0], sy__[0], sx__[1], sy__[1]};                                                 \
      asm volatile("" : "+v"(out_));                                                                         \
    } else {                                                                                                 \
      asm volatile("" : "+v"(pk_[0]));                                                                       \
    }                                                                                                        \
  } while (0)
  // chunk c = 2t + gp of the item on panel panel_: features 32t + 16gp + 8h .. + 7
#define QK_STORE_CHUNK(c_, panel_)                                                                           \
  do {                                                                                                       \
    if (tok_ok && !(p.debug & TTV_DBG_NO_STORES)) *reinterpret_cast<qk_u32x4*>(ytok + (size_t)(panel_) * 128 + (c_) * 32) = out_; \
  } while (0)
  // the whole epilogue of an item at once (pipeline drain: token tile change, last item)
#define QK_EPILOGUE(acc_, ROT_, panel_)                                                                      \
  do {                                                                                                       \
    float o_[4]; qk_u32x2 pk_[2]; qk_u32x4 out_;                                                             \
    _Pragma("unroll") for (int G__ = 0; G__ < 8; ++G__) {                                                    \
      QK_ROT(acc_, ROT_, G__);                                                                               \
      QK_PACK(G__);                                                                                          \
      if (G__ & 1) QK_STORE_CHUNK(G__ >> 1, panel_);                                                         \
    }                                                                                                        \
  } while (0)

  // One item: 32 MFMAs (k-step ks: the two 32-feature halves against the wave's token fragment ks), every k-step its own scheduling
  // region with the order inside pinned by sched_group_barrier.  Riding along: the A fragments of k-step ks + 1 (top of k-step ks);
  // k-steps 0-7 one DMA instruction of the next panel each; MODE_ 1 (plain) / 2 (rotary): the epilogue of item i - 1 - even k-steps
  // the rotation of group ks / 2, odd k-steps its pack / exchange, a finished chunk stored behind k-steps 3, 7, 11, 15; MODE_ 0 (first
  // item after a token-tile change): the row's sum of squares on the fragments as they arrive, the rotary-factor loads at k-step 8.
#define QK_BODY(cur_, prev_, buf_, MODE_)                                                                    \
  do {                                                                                                       \
    bf16x8 af__[2][2];                                                                                       \
    float o_[4]; qk_u32x2 pk_[2]; qk_u32x4 out_;                                                             \
    float ss0__ = 0.f, ss1__ = 0.f;                                                                          \
    uint32_t a0__ = aoff0, dc0__ = dchunk0;                                                                  \
    asm volatile("" : "+v"(a0__), "+v"(dc0__));   /* the per-k-step XORs stay in their k-steps (not hoisted out of the item loop) */ \
    af__[0][0] = QK_AFRAG(buf_, 0, 0);                                                                       \
    af__[0][1] = QK_AFRAG(buf_, 1, 0);                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    _Pragma("unroll") for (int ks__ = 0; ks__ < 16; ++ks__) {                                                \
      if (ks__ < 8 && has_next__) {                                                                          \
        if (ks__ == 0) QK_DMA_PIECE(dc0__, 0, nsrc__, ndst__); else if (ks__ == 1) QK_DMA_PIECE(dc0__, 1, nsrc__, ndst__);  \
        else if (ks__ == 2) QK_DMA_PIECE(dc0__, 2, nsrc__, ndst__); else if (ks__ == 3) QK_DMA_PIECE(dc0__, 3, nsrc__, ndst__); \
        else if (ks__ == 4) QK_DMA_PIECE(dc0__, 4, nsrc__, ndst__); else if (ks__ == 5) QK_DMA_PIECE(dc0__, 5, nsrc__, ndst__); \
        else if (ks__ == 6) QK_DMA_PIECE(dc0__, 6, nsrc__, ndst__); else QK_DMA_PIECE(dc0__, 7, nsrc__, ndst__);            \
      }                                                                                                      \
      if (MODE_ == 0 && ks__ == 8) {                                                                         \
        int hq__ = h;                                                                                        \
        asm volatile("" : "+v"(hq__));      /* keeps the sixteen (frequency, axis) pairs of a lane out of loop-invariant registers */ \
        if (p.rope_ids) {                                                                                    \
          _Pragma("unroll") for (int t__ = 0; t__ < 2; ++t__)                                                \
            _Pragma("unroll") for (int g__ = 0; g__ < 4; ++g__)                                              \
              _Pragma("unroll") for (int e__ = 0; e__ < 2; ++e__) {                                          \
                const int pp__ = 16 * t__ + 4 * g__ + 2 * hq__ + e__;                                        \
                const int f__ = pp__ < 30 ? pp__ / 3 : 0, ax__ = pp__ < 30 ? pp__ - 3 * (pp__ / 3) : 3;      \
                const uint32_t wd__ = (ax__ & 2) ? idp.y : idp.x;                                            \
                const uint32_t id__ = (ax__ & 1) ? (wd__ >> 16) : (wd__ & 0xffffu);                          \
                rcs[t__][g__][e__] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(p.rope_base) + id__ * 80u + (uint32_t)f__ * 8u); \
              }                                                                                              \
        } else {                                                                                             \
          const float* c__ = p.rope_cs + (size_t)tk * 64 + 2 * hq__;                                         \
          _Pragma("unroll") for (int t__ = 0; t__ < 2; ++t__)                                                \
            _Pragma("unroll") for (int g__ = 0; g__ < 4; ++g__) {                                            \
              const float2 cc__ = *reinterpret_cast<const float2*>(c__ + 16 * t__ + 4 * g__);                \
              const float2 sn__ = *reinterpret_cast<const float2*>(c__ + 32 + 16 * t__ + 4 * g__);           \
              rcs[t__][g__][0] = make_float2(cc__.x, sn__.x);                                                \
              rcs[t__][g__][1] = make_float2(cc__.y, sn__.y);                                                \
            }                                                                                                \
        }                                                                                                    \
      }                                                                                                      \
      __builtin_amdgcn_sched_barrier(0);                                                                     \
      if (ks__ + 1 < 16) {                                                                                   \
        af__[(ks__ + 1) & 1][0] = QK_AFRAG(buf_, 0, ks__ + 1);                                               \
        af__[(ks__ + 1) & 1][1] = QK_AFRAG(buf_, 1, ks__ + 1);                                               \
      }                                                                                                      \
      cur_[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af__[ks__ & 1][0], bfr[ks__], ks__ ? cur_[0] : zero16, 0, 0, 0); \
      cur_[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af__[ks__ & 1][1], bfr[ks__], ks__ ? cur_[1] : zero16, 0, 0, 0); \
      if (MODE_) {                                                                                           \
        if ((ks__ & 1) == 0) QK_ROT(prev_, MODE_ == 2, ks__ >> 1); else QK_PACK(ks__ >> 1);                  \
      } else if (PRENORM) {                                                                                  \
        const bf16x8 v__ = bfr[ks__];                                                                        \
        ss0__ = __builtin_amdgcn_fdot2_f32_bf16((bf16x2){v__[0], v__[1]}, (bf16x2){v__[0], v__[1]}, ss0__, false); \
        ss1__ = __builtin_amdgcn_fdot2_f32_bf16((bf16x2){v__[2], v__[3]}, (bf16x2){v__[2], v__[3]}, ss1__, false); \
        ss0__ = __builtin_amdgcn_fdot2_f32_bf16((bf16x2){v__[4], v__[5]}, (bf16x2){v__[4], v__[5]}, ss0__, false); \
        ss1__ = __builtin_amdgcn_fdot2_f32_bf16((bf16x2){v__[6], v__[7]}, (bf16x2){v__[6], v__[7]}, ss1__, false); \
        asm volatile("" : "+v"(ss0__), "+v"(ss1__));                                                         \
      }                                                                                                      \
      if (ks__ + 1 < 16) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                  \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                     \
      if (MODE_) { if ((ks__ & 1) || MODE_ != 2) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0); else __builtin_amdgcn_sched_group_barrier(0x002, 4, 0); } \
      else if (PRENORM) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                                   \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                     \
      if (MODE_) { if ((ks__ & 1) || MODE_ != 2) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0); else __builtin_amdgcn_sched_group_barrier(0x002, 4, 0); } \
      else if (PRENORM) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                                   \
      __builtin_amdgcn_sched_barrier(0);                                                                     \
      if (MODE_ && (ks__ & 3) == 3) {                                                                        \
        QK_STORE_CHUNK(ks__ >> 2, pend_panel);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
      }                                                                                                      \
    }                                                                                                        \
    if (MODE_ == 0) {                                                                                        \
      if (PRENORM) {                                                                                         \
        float ss__ = ss0__ + ss1__;                                                                          \
        ss__ = pair32_sum(ss__);                                                                    \
        rstd = 1.0f / sqrtf(ss__ * (1.0f / 256.0f) + p.eps);                                                 \
      }                                                                                                      \
      _Pragma("unroll") for (int t__ = 0; t__ < 2; ++t__)                                                    \
        _Pragma("unroll") for (int g__ = 0; g__ < 4; ++g__)                                                  \
          _Pragma("unroll") for (int e__ = 0; e__ < 2; ++e__)                                                \
            rcs[t__][g__][e__] = make_float2(rcs[t__][g__][e__].x * rstd, rcs[t__][g__][e__].y * rstd);      \
    }                                                                                                        \
  } while (0)

#define QK_STEP(cur_, prev_, it_)                                                                            \
  do {                                                                                                       \
    const int it__ = (it_);                                                                                  \
    const int buf__ = (it__ - it0) & 1;                                                                      \
    int tile__, panel__;                                                                                     \
    if (FLOOR) {                                                                                             \
      /* this item is (fl_tile, fl_panel); step to the next one: its panel is what the body stages */        \
      tile__ = fl_tile; panel__ = fl_panel;                                                                  \
      if (++fl_panel == n_panels) {                                                                          \
        ++fl_tile;                                                                                           \
        if (++fl_pos == p.tile_period) fl_pos = 0;                                                           \
        fl_panel = fl_pos < p.tile_run ? 0 : p.panel_lo;                                                     \
      }                                                                                                      \
    } else {                                                                                                 \
      tile__ = it__ / n_panels; panel__ = it__ - tile__ * n_panels;                                          \
    }                                                                                                        \
    if (tile__ != cur_tile) {                                                                                \
      cur_tile = tile__;                                                                                     \
      /* the new rows are requested first: the epilogue owed to the previous tile (it needs that tile's factors and addresses) */ \
      /* runs under their latency */                                                                         \
      /* a tile list (GemmDev.tile_run / tile_period): item tile -> token tile, rows and outputs in place */  \
      const int ttile__ = FLOOR ? tile__ : p.tile_period ? (tile__ / p.tile_run) * p.tile_period + tile__ % p.tile_run : tile__; \
      const int t0__ = ttile__ * K256_TT + wave * 32;                                                        \
      int ntk__ = t0__ + r;                                                                                  \
      const bool nok__ = ntk__ < p.M;                                                                        \
      ntk__ = nok__ ? ntk__ : p.M - 1;                                                                       \
      const bf16_t* xr__ = X + (size_t)(p.x_rows ? p.x_rows[ntk__] : ntk__) * p.ldx + h * 8;                 \
      _Pragma("unroll") for (int ks__ = 0; ks__ < 16; ++ks__) bfr[ks__] = *reinterpret_cast<const bf16x8*>(xr__ + ks__ * 16); \
      uint2 nidp__ = make_uint2(0u, 0u);                                                                     \
      if (p.rope_ids) nidp__ = *reinterpret_cast<const uint2*>(p.rope_ids + 2 * (size_t)ntk__);              \
      if (pend == 2) QK_EPILOGUE(prev_, true, pend_panel); else if (pend == 1) QK_EPILOGUE(prev_, false, pend_panel); \
      pend = 0;                                                                                              \
      /* the rows have landed before any body runs: a use the compiler must wait for HERE.  Left pending, its wait-count pass puts    */ \
      /* counted vmcnt waits for the sixteen row loads into EVERY body (it cannot know that a tile change implies pend == 0), down to */ \
      /* vmcnt(0): each plain / rotary item then drains its own stores and the next panel's DMA (tools/qkv256_stamps.sh)              */ \
      _Pragma("unroll") for (int ks__ = 0; ks__ < 16; ++ks__) asm volatile("" : "+v"(bfr[ks__]));            \
      tk = ntk__; tok_ok = nok__; idp = nidp__;                                                              \
      wave_full = t0__ + 32 <= p.M;                                                                          \
      ytok = reinterpret_cast<char*>((bf16_t*)p.y + (size_t)tk * p.ldy) + h * 16;                            \
      rstd = 1.f;                                                                                            \
    }                                                                                                        \
    QK_STAMP(0);                                                                                             \
    if (it__ == it0) {                                                                                       \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                       \
      __syncthreads();                                                                                       \
    }                                                                                                        \
    QK_STAMP(1);                                                                                             \
    const bool has_next__ = it__ + 1 < it1;                                                                  \
    const char* nsrc__ = QK_PANEL_SRC(FLOOR ? fl_panel : (it__ + 1) % n_panels);                             \
    const uint32_t ndst__ = QK_PANEL_DST(buf__ ^ 1);                                                         \
    const int f_first__ = panel__ * 64;                                                                      \
    const int rot__ = (f_first__ < p.rope_q_end || (f_first__ >= p.rope_k_begin && f_first__ < p.rope_k_end)) ? 2 : 1; \
    bool counted__ = false;                                                                                  \
    if (pend == 2) {                                                                                         \
      if (buf__) QK_BODY(cur_, prev_, 1, 2); else QK_BODY(cur_, prev_, 0, 2);                                \
      counted__ = wave_full && !(p.debug & TTV_DBG_NO_STORES);                                                               \
      QK_STAMP(2);                                                                                           \
    } else if (pend == 1) {                                                                                  \
      if (buf__) QK_BODY(cur_, prev_, 1, 1); else QK_BODY(cur_, prev_, 0, 1);                                \
      counted__ = wave_full && !(p.debug & TTV_DBG_NO_STORES);                                                               \
      QK_STAMP(2);                                                                                           \
    } else {                                                                                                 \
      if (buf__) QK_BODY(cur_, prev_, 1, 0); else QK_BODY(cur_, prev_, 0, 0);                                \
      QK_STAMP(3);                                                                                           \
    }                                                                                                        \
    /* the next panel has landed (this wave's share): the stores behind k-steps 7, 11, 15 are younger than the last DMA instruction */ \
    if (counted__) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");                                          \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                    \
    QK_STAMP(4);                                                                                             \
    __builtin_amdgcn_s_barrier();                                                                            \
    QK_STAMP(5);                                                                                             \
    pend = rot__;                                                                                            \
    pend_panel = panel__;                                                                                    \
  } while (0)

  f32x16 accA[2], accB[2];
  QK_STAMP_DECL;
  // FLOOR: the block's first item.  A period of tile_period token tiles holds tile_run * n_panels + (tile_period - tile_run) * (n_panels -
  // panel_lo) items: the full tiles first, panel-major inside a tile.  fl_pos = the tile's place in its period.
  int fl_tile = 0, fl_panel = 0, fl_pos = 0;
  if (FLOOR) {
    const int full = p.tile_run * n_panels, wide = n_panels - p.panel_lo;
    const int per = full + (p.tile_period - p.tile_run) * wide;
    const int q = it0 / per;
    int rem = it0 - q * per;
    if (rem < full) { fl_pos = rem / n_panels; fl_panel = rem - fl_pos * n_panels; }
    else { rem -= full; fl_pos = p.tile_run + rem / wide; fl_panel = p.panel_lo + rem % wide; }
    fl_tile = q * p.tile_period + fl_pos;
  }
  {
    const char* src0 = QK_PANEL_SRC(FLOOR ? fl_panel : it0 % n_panels);
    const uint32_t dst0 = QK_PANEL_DST(0);
    QK_DMA_PIECE(dchunk0, 0, src0, dst0); QK_DMA_PIECE(dchunk0, 1, src0, dst0); QK_DMA_PIECE(dchunk0, 2, src0, dst0); QK_DMA_PIECE(dchunk0, 3, src0, dst0);
    QK_DMA_PIECE(dchunk0, 4, src0, dst0); QK_DMA_PIECE(dchunk0, 5, src0, dst0); QK_DMA_PIECE(dchunk0, 6, src0, dst0); QK_DMA_PIECE(dchunk0, 7, src0, dst0);
  }
  QK_STAMP_START();
  int it = it0;
  for (; it + 1 < it1; it += 2) {
    QK_STEP(accA, accB, it);
    QK_STEP(accB, accA, it + 1);
  }
  if (it < it1) {
    QK_STEP(accA, accB, it);
    if (pend == 2) QK_EPILOGUE(accA, true, pend_panel); else QK_EPILOGUE(accA, false, pend_panel);
  } else {
    if (pend == 2) QK_EPILOGUE(accB, true, pend_panel); else QK_EPILOGUE(accB, false, pend_panel);
  }
  QK_STAMP(6);
#ifdef QKV_STAMPS
  if (p.stamps && lb % 16 == 0 && lane == 0) {
    long long* dst = p.stamps + ((size_t)(lb / 16) * 4 + wave) * 8;
    for (int i = 0; i < 7; ++i) dst[i] = (long long)qst_acc__[i];
    dst[7] = it1 - it0;
  }
#endif
#undef QK_DMA_PIECE
#undef QK_PANEL_SRC
#undef QK_PANEL_DST
#undef QK_AFRAG
#undef QK_ROT
#undef QK_PACK
#undef QK_STORE_CHUNK
#undef QK_EPILOGUE
#undef QK_BODY
#undef QK_STEP
}
