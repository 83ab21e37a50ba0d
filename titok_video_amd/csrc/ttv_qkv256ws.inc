// ================================================================================================
// to_qkv of a width-256 tower with the WEIGHTS stationary in LDS (round 4; included by ttv_gemm.hip behind ttv_qkv256.inc):
// pre_ln + to_qkv + rotary, reference model/base/transformer.py:86-98.
//
// Why: in the streaming kernels (k_gemm_k256, k_qkv256) a CU moves, per pair of items, 64 KiB of weight panels L2 -> LDS through its one
// vector-memory address path, writes them into LDS, reads 256 KiB of A fragments back out of LDS and issues 2 048 cycles of MFMAs: the
// three pipes are loaded about equally and at two waves per SIMD they do not overlap - an item pair takes ~6 000 cycles whichever way
// the instructions are interleaved (profiles/r04_qkv256_stamps_*.txt; the total is conserved when DMA issue, stores and the epilogue are
// moved under the MFMAs).  Here the panel traffic is gone:
//   * one block of 8 waves per CU owns a GROUP of up to four 64-row panels (128 KiB of LDS, loaded once, k_gemm_k256's swizzled image);
//     a 768-feature projection is three groups, and the blocks of one XCD (block % 8) split its eighth of the token groups between the
//     panel groups, so a token row is fetched from HBM once per XCD and served to the other two groups by that XCD's L2;
//   * a wave's unit of work is 32 tokens x the group's panels: token fragments in registers (global loads, no LDS), per panel 32 MFMAs
//     (32x32x16) against A fragments read from the resident panels; waves never synchronise after the weight load (no barrier, no DMA, no
//     counted waits in the loop);
//   * as in k_qkv256 the epilogue of item i-1 (rotary with rstd folded into the factors / row scale, bf16 pack, exchange with lane ^ 32,
//     16-byte stores) rides between the MFMAs of item i, the row's sum of squares and the rotary-factor gathers ride under the first item of
//     a unit, whose MFMA of k-step ks waits only for the token fragment ks.
// Per item pair a CU now issues 2 048 cycles of MFMAs beside 1 024 cycles of LDS reads and ~750 cycles of vector-memory traffic.
// Results: the arithmetic of k_qkv256 (bit-identical to k_gemm_k256<EPI_QKV_ROPE> without the folded pre-norm).
// ================================================================================================
// knock-out switches of diagnostic builds (tools/qkv256_knockout.sh; garbage results, timing only): -DQW_KO_LDS no A-fragment reads in the
// loop, -DQW_KO_EPI no riding epilogue (arithmetic, exchange, stores), -DQW_KO_MFMA no MFMAs, -DQW_KO_X token rows loaded for the first unit only
#ifndef QW_KO_LDS
#define QW_KO_LDS 0
#endif
#ifndef QW_KO_EPI
#define QW_KO_EPI 0
#endif
#ifndef QW_KO_MFMA
#define QW_KO_MFMA 0
#endif
#ifndef QW_KO_X
#define QW_KO_X 0
#endif
#ifndef QW_KO_ROWS      // stores go out as whole 128-byte row segments (8 adjacent lanes per token; WRONG placement of the values: timing only)
#define QW_KO_ROWS 0
#endif
template <bool PRENORM>
__global__ __launch_bounds__(512, 1) void k_qkv256ws(GemmDev p, int n_panels, int n_groups) {
  __shared__ uint4 wl[4][K256_ROWS * 32];  // [panel of the group][row * 32 + swizzled 16-byte chunk], 128 KiB

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 0 .. 7
  const int r = lane & 31, h = lane >> 5;
  // block -> (XCD, panel group, index within both); units of XCD x: token groups [TG x / 8, TG (x + 1) / 8)
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int grp = q % n_groups, j = q / n_groups;
  const int q_x = ((int)gridDim.x - xcd + 7) >> 3;                 // blocks of this XCD
  const int nblk = (q_x - grp + n_groups - 1) / n_groups;          // ... that work on this panel group
  const int tgs = (p.M + 31) >> 5;
  const int tg0 = (int)((long)tgs * xcd / 8), n_u = (int)((long)tgs * (xcd + 1) / 8) - tg0;
  const int nw = nblk * 8, wv = j * 8 + wave;
  if (j * 8 >= n_u) return;                                        // no wave of this block has a unit (block-uniform)
  const int pg0 = grp * 4, npg = n_panels - pg0 < 4 ? n_panels - pg0 : 4;
  const bf16_t* X = (const bf16_t*)p.x;

  // ---- the group's panels -> LDS, once: wave w stages rows 8w .. 8w+7 of every panel (two 512-byte rows per DMA instruction) ----
  {
    const uint32_t wl_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&wl[0][0];
    const int gc = lane & 31;
    for (int pi = 0; pi < npg; ++pi) {
      const char* src = reinterpret_cast<const char*>(p.w) + (size_t)(pg0 + pi) * 64 * (size_t)p.ldw * 2;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wave * 8 + 2 * i + h;
        const int ch = (gc & 16) | ((gc & 15) ^ (row & 15));
        const uint32_t voff = ((uint32_t)row * (uint32_t)p.ldw + ch * 8) * 2u;
        const uint32_t dst = wl_lds + pi * (K256_ROWS * 512) + (wave * 8 + 2 * i) * 512;
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(src), "s"(dst) : "memory");
      }
    }
  }

  // ---- A fragment (weights) read address: row 32t + r, logical chunk 2ks + h -> chunk (h ^ r15) ^ 2k (bits 5-7 of the byte offset) ----
  const int r15 = r & 15;
  const char* const wl_base = reinterpret_cast<const char*>(&wl[0][0]);
  const uint32_t aoff0 = (uint32_t)(r * 32 + (h ^ r15)) * 16u;
#define QW_AFRAG(t_, ks_) (QW_KO_LDS ? bfr[((ks_) + (t_)) & 15] : \
  *reinterpret_cast<const bf16x8*>(wl_base + (a0__ ^ (uint32_t)(((ks_) & 7) << 5)) + (t_) * (32 * 512) + (((ks_) >> 3) & 1) * 256))

  bf16x8 bfr[16];          // the wave's 32 tokens x 256 k as B fragments: token r, k = 16 ks + 8 h .. + 7
  float rstd = 1.f;
  float2 rcs[2][4][2];     // (cos, sin) * rstd of pairs 16t + 4g + 2h + e2 of a 64-wide head, for token r
  char* ytok = nullptr;    // &y[token][8 h]
  char* yrow__ = nullptr;  // QW_KO_ROWS only
  uint2 idp = make_uint2(0u, 0u);
  int tk = 0;
  bool tok_ok = true;
  int pend = 0;            // epilogue owed for the previous item: 0 none, 1 plain panel, 2 rotary panel
  int pend_panel = 0;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // ---- epilogue slices (k_qkv256's): group G = 4t + g, features 32t + 8g + 4h .. + 3 of token r ----
#define QW_ROT(acc_, ROT_, G_)                                                                               \
  do {                                                                                                       \
    const int t__ = (G_) >> 2, g__ = (G_) & 3;                                                               \
    const float a0v__ = acc_[t__][4 * g__], a1v__ = acc_[t__][4 * g__ + 1], a2v__ = acc_[t__][4 * g__ + 2], a3v__ = acc_[t__][4 * g__ + 3]; \
    if (ROT_) {                                                                                              \
      const float2 k0__ = rcs[t__][g__][0], k1__ = rcs[t__][g__][1];                                         \
      o_[0] = a0v__ * k0__.x - a1v__ * k0__.y; o_[1] = a0v__ * k0__.y + a1v__ * k0__.x;                      \
      o_[2] = a2v__ * k1__.x - a3v__ * k1__.y; o_[3] = a2v__ * k1__.y + a3v__ * k1__.x;                      \
    } else {                                                                                                 \
      o_[0] = a0v__ * rstd; o_[1] = a1v__ * rstd; o_[2] = a2v__ * rstd; o_[3] = a3v__ * rstd;                \
    }                                                                                                        \
    asm volatile("" : "+v"(o_[0]), "+v"(o_[1]), "+v"(o_[2]), "+v"(o_[3]));                                   \
  } while (0)
#define QW_PACK(G_)                                                                                          \
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
#define QW_STORE_CHUNK(c_, panel_)                                                                           \
  do {                                                                                                       \
    if (QW_KO_ROWS) {                                                                                        \
      if (tok_ok && !(p.debug & TTV_DBG_NO_STORES)) *reinterpret_cast<qk_u32x4*>(yrow__ + (size_t)(c_) * 8 * p.ldy * 2 + (size_t)(panel_) * 128) = out_; \
    } else                                                                                                   \
    if (tok_ok && !(p.debug & TTV_DBG_NO_STORES)) *reinterpret_cast<qk_u32x4*>(ytok + (size_t)(panel_) * 128 + (c_) * 32) = out_; \
  } while (0)
#define QW_EPILOGUE(acc_, ROT_, panel_)                                                                      \
  do {                                                                                                       \
    float o_[4]; qk_u32x2 pk_[2]; qk_u32x4 out_;                                                             \
    _Pragma("unroll") for (int G__ = 0; G__ < 8; ++G__) {                                                    \
      QW_ROT(acc_, ROT_, G__);                                                                               \
      QW_PACK(G__);                                                                                          \
      if (G__ & 1) QW_STORE_CHUNK(G__ >> 1, panel_);                                                         \
    }                                                                                                        \
  } while (0)

  // One item = one resident panel (LDS byte offset poff_) against the wave's tokens: 32 MFMAs, every k-step (two MFMAs) its own
  // scheduling region.  Riding along: the A fragments of k-step ks + 1; MODE_ 1 (plain) / 2 (rotary): the epilogue of the previous
  // item, a finished chunk stored behind k-steps 3, 7, 11, 15; MODE_ 0 (first item of a unit): the row's sum of squares on the token
  // fragments as they arrive, the rotary-factor loads at k-step 8, rstd and the folded factors behind the last MFMA.
#define QW_BODY(cur_, prev_, poff_, MODE_)                                                                   \
  do {                                                                                                       \
    bf16x8 af__[2][2];                                                                                       \
    float o_[4]; qk_u32x2 pk_[2]; qk_u32x4 out_;                                                             \
    float ss0__ = 0.f, ss1__ = 0.f;                                                                          \
    uint32_t a0__ = aoff0 + (poff_);                                                                         \
    asm volatile("" : "+v"(a0__));          /* the per-k-step XORs stay in their k-steps (not hoisted out of the item loop) */ \
    af__[0][0] = QW_AFRAG(0, 0);                                                                             \
    af__[0][1] = QW_AFRAG(1, 0);                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    _Pragma("unroll") for (int ks__ = 0; ks__ < 16; ++ks__) {                                                \
      if (MODE_ == 0 && ks__ == 8 && want_rope__) {                                                          \
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
        af__[(ks__ + 1) & 1][0] = QW_AFRAG(0, ks__ + 1);                                                     \
        af__[(ks__ + 1) & 1][1] = QW_AFRAG(1, ks__ + 1);                                                     \
      }                                                                                                      \
      if (!QW_KO_MFMA) {                                                                                     \
        cur_[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af__[ks__ & 1][0], bfr[ks__], ks__ ? cur_[0] : zero16, 0, 0, 0); \
        cur_[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af__[ks__ & 1][1], bfr[ks__], ks__ ? cur_[1] : zero16, 0, 0, 0); \
      } else {                                                                                               \
        asm volatile("" :: "v"(af__[ks__ & 1][0]), "v"(af__[ks__ & 1][1]));                                  \
        if (ks__ == 0) { cur_[0] = zero16; cur_[1] = zero16; }                                               \
      }                                                                                                      \
      if (MODE_ && !QW_KO_EPI) {                                                                             \
        if ((ks__ & 1) == 0) QW_ROT(prev_, MODE_ == 2, ks__ >> 1); else QW_PACK(ks__ >> 1);                  \
      } else if (PRENORM && !MODE_) {                                                                                  \
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
      if (MODE_ && !QW_KO_EPI && (ks__ & 3) == 3) {                                                          \
        QW_STORE_CHUNK(ks__ >> 2, pend_panel);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
      }                                                                                                      \
    }                                                                                                        \
    if (MODE_ == 0) {                                                                                        \
      if (PRENORM) {                                                                                         \
        float ss__ = ss0__ + ss1__;                                                                          \
        ss__ = pair32_sum(ss__);                                                                    \
        rstd = 1.0f / sqrtf(ss__ * (1.0f / 256.0f) + p.eps);                                                 \
      }                                                                                                      \
      if (want_rope__) {                                                                                     \
        _Pragma("unroll") for (int t__ = 0; t__ < 2; ++t__)                                                  \
          _Pragma("unroll") for (int g__ = 0; g__ < 4; ++g__)                                                \
            _Pragma("unroll") for (int e__ = 0; e__ < 2; ++e__)                                              \
              rcs[t__][g__][e__] = make_float2(rcs[t__][g__][e__].x * rstd, rcs[t__][g__][e__].y * rstd);    \
      }                                                                                                      \
    }                                                                                                        \
  } while (0)

  // item pi_ of the current unit: cur_ / prev_ are the two accumulator sets (literal names: no register copies)
#define QW_STEP(cur_, prev_, pi_)                                                                            \
  do {                                                                                                       \
    const int panel__ = pg0 + (pi_);                                                                         \
    const uint32_t poff__ = (uint32_t)(pi_) * (K256_ROWS * 512);                                             \
    const int f_first__ = panel__ * 64;                                                                      \
    const int rot__ = (f_first__ < p.rope_q_end || (f_first__ >= p.rope_k_begin && f_first__ < p.rope_k_end)) ? 2 : 1; \
    if (pend == 2) QW_BODY(cur_, prev_, poff__, 2);                                                          \
    else if (pend == 1) QW_BODY(cur_, prev_, poff__, 1);                                                     \
    else QW_BODY(cur_, prev_, poff__, 0);                                                                    \
    pend = rot__;                                                                                            \
    pend_panel = panel__;                                                                                    \
  } while (0)

  // does any panel of the group rotate?  (the gate / v groups need no factors)
  bool want_rope__ = false;
  for (int pi = 0; pi < npg; ++pi) {
    const int f = (pg0 + pi) * 64;
    want_rope__ = want_rope__ || f < p.rope_q_end || (f >= p.rope_k_begin && f < p.rope_k_end);
  }

  f32x16 accA[2], accB[2];
#ifdef QKV_STAMPS
  unsigned long long qw_c0 = 0, qw_r0 = 0, qw_c1 = 0, qw_r1 = 0, qw_c2 = 0, qw_r2 = 0;
  int qw_items = 0;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(qw_c0), "=s"(qw_r0)::"memory");
#endif
  int par = 0;             // which accumulator set the next item writes
  bool first = true;
  for (int u = wv; u < n_u; u += nw) {
    // the unit's token rows are requested first; the epilogue owed to the previous unit runs under their latency
    const int t0 = (tg0 + u) * 32;
    int ntk = t0 + r;
    const bool nok = ntk < p.M;
    ntk = nok ? ntk : p.M - 1;
    const bf16_t* xr = X + (size_t)(p.x_rows ? p.x_rows[ntk] : ntk) * p.ldx + h * 8;
    if (!QW_KO_X || first) {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) bfr[ks] = *reinterpret_cast<const bf16x8*>(xr + ks * 16);
    }
    uint2 nidp = make_uint2(0u, 0u);
    if (p.rope_ids && want_rope__) nidp = *reinterpret_cast<const uint2*>(p.rope_ids + 2 * (size_t)ntk);
    if (pend) {
      if (par) { if (pend == 2) QW_EPILOGUE(accA, true, pend_panel); else QW_EPILOGUE(accA, false, pend_panel); }
      else { if (pend == 2) QW_EPILOGUE(accB, true, pend_panel); else QW_EPILOGUE(accB, false, pend_panel); }
      pend = 0;
    }
    tk = ntk; tok_ok = nok; idp = nidp;
    ytok = reinterpret_cast<char*>((bf16_t*)p.y + (size_t)tk * p.ldy) + h * 16;
    yrow__ = reinterpret_cast<char*>((bf16_t*)p.y + (size_t)(t0 + (lane >> 3) < p.M ? t0 + (lane >> 3) : p.M - 1) * p.ldy) + (lane & 7) * 16;
    rstd = 1.f;
    if (first) {           // the group's panels have landed (this wave's share), for every wave of the block
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      first = false;
#ifdef QKV_STAMPS
      asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(qw_c1), "=s"(qw_r1)::"memory");
#endif
    }
    for (int pi = 0; pi < npg; ++pi) {
      if (par) QW_STEP(accB, accA, pi); else QW_STEP(accA, accB, pi);
      par ^= 1;
#ifdef QKV_STAMPS
      ++qw_items;
#endif
    }
  }
  if (first) {             // a wave without units still takes part in the block's one barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (pend) {
    if (par) { if (pend == 2) QW_EPILOGUE(accA, true, pend_panel); else QW_EPILOGUE(accA, false, pend_panel); }
    else { if (pend == 2) QW_EPILOGUE(accB, true, pend_panel); else QW_EPILOGUE(accB, false, pend_panel); }
  }
#ifdef QKV_STAMPS
  // per wave of every 8th block: cycles and 100 MHz ticks from kernel entry to the end of the weight load, and over the unit loop; items
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(qw_c2), "=s"(qw_r2)::"memory");
  if (p.stamps && (blockIdx.x >> 3) % 4 == 0 && lane == 0 && qw_items) {
    long long* dst = p.stamps + ((size_t)((blockIdx.x >> 5) * 8 + (blockIdx.x & 7)) * 8 + wave) * 8;
    dst[0] = (long long)(qw_c1 - qw_c0); dst[1] = (long long)(qw_r1 - qw_r0);
    dst[2] = (long long)(qw_c2 - qw_c1); dst[3] = (long long)(qw_r2 - qw_r1);
    dst[7] = qw_items;
  }
#endif
#undef QW_AFRAG
#undef QW_ROT
#undef QW_PACK
#undef QW_STORE_CHUNK
#undef QW_EPILOGUE
#undef QW_BODY
#undef QW_STEP
}
