// Opt-in inference attention whose second product runs in 8 bits: O^T += V8^T P8^T on v_mfma_scale_f32_32x32x64_f8f6f4 (block-scaled
// OCP e4m3, fp32 accumulation), one instruction per 32 head dims and 64-key tile where k_attn_bf16 issues four bf16 MFMAs.
// S = Q K^T stays bf16 x bf16 -> fp32 exactly as in k_attn_bf16 (q pre-scaled: a score is the exponent), the softmax stays fp32.
// Two kernels: k_quant_v_pv8 writes the MX image of the v columns (one pass per layer), k_attn_pv8<GATE> reads it.  DESIGN.md 4z.
//
// The instruction, measured (tools/ubench/mx_probe_32x32x64.hip, profiles/pv8_mx_probe.txt; exact integers, asymmetric one-hot data):
//   * A (32 rows x 64 k) and B (64 k x 32 columns): lane = 32 h + row (A) / 32 h + column (B) holds 32 operand bytes in 8 registers;
//     A element (h, byte b) pairs with B element (h, byte b) - the instruction's k index of (h, b) is 16 h + b for b < 16 and
//     32 + 16 h + (b - 16) for b >= 16, the same on both sides, so ANY assignment of keys to (h, b) is right once A and B share it;
//   * D[i][j] sits in lane 32 h + j, register e with i = 8 (e >> 2) + 4 h + (e & 3): the layout of the 32x32x16 bf16 MFMA;
//   * scale operands: one byte per lane (op_sel 0..3 picks the byte of the register), value 2^(byte - 127); the byte of lane
//     (row, hs) multiplies the bytes 16 hs .. 16 hs + 15 of BOTH lanes (row, 0), (row, 1) - the instruction's k block 32 hs .. 32 hs + 31 -
//     NOT the 32 bytes that lane holds.  The same holds for B with columns.
// The kernel's choice.  The score accumulator of tile half t (keys 32 t .. 32 t + 31 of a 64-key tile) has, in lane (query r, h) and
// register e, the key 32 t + 8 (e >> 2) + 4 h + (e & 3).  Its 32 values per lane, packed with v_cvt_pk_fp8_f32 in register order, ARE
// the B operand: byte b = 16 t + e.  The A operand of lane (d, h) therefore holds V[key(h, b)][d] at byte b, and an MX block - bytes
// 16 t .. 16 t + 15 of both lane halves - is the NATURAL half t of the tile: keys 32 t .. 32 t + 31 of one head-dim column; lane (d, hs)
// supplies the scale of half hs.
//
// Image (k_quant_v_pv8), per (sequence, key tile, kv-head) 4 224 bytes, tiles counted from the sequence's first row; the tiles of
// sequence i start at slot (cu[i] >> 6) + i (no prefix sum: floor(a / 64) + ceil(b / 64) <= floor((a + b) / 64) + 1), slots between
// sequences stay unused; tile address = ((slot * kv_heads) + kv-head) * 4224:
//   bytes [0, 4096)     [dt = d >> 5][lane = 32 h + (d & 31)][b = 16 t + e]: e4m3_rne(V[key][d] * 2^-E), key = 32 t + 8 (e >> 2) + 4 h + (e & 3):
//                       a lane of the attention kernel reads its 32 bytes of a d-tile with two 16-byte loads, no transpose, no LDS;
//   bytes [4096, 4224)  [dt][32 t + (d & 31)]: the E8M0 byte of block (t, d) - lane 32 hs + (d & 31) reads the byte it must supply.
// E = ceil(log2(amax / 448)) from the fp32 product amax * (1 / 448) (k_quant_mx_fp8's rule, oracle/fp8_oracle.py), byte clamped to
// 1 .. 254, 127 for an all-zero block; keys past the sequence end are zero bytes.
//
// Softmax with a P that cannot saturate.  p = exp2(s - m_ref) against a running reference m_ref that is never above the running row
// maximum; P enters the product as e4m3_rne(p * 2^PV8_K), PV8_K = 6.  The factor is folded into the exponent - the score accumulators
// start from -(m_ref - 6), k_attn_bf16's PRE device, so a score leaves the matrix pipe as the exponent of p * 2^6 - and is carried by
// the row sum too (l adds the fp32 values BEFORE their rounding to e4m3), so O / l undoes it exactly.  The reference moves by this
// kernel's own rule: a tile whose row maximum exceeds m_ref by more than PV8_LAG = 2 log2 units moves m_ref to that maximum (see the
// loop).  So m_ref lags the running maximum by at most D = 2 units, p <= 4 and p * 2^6 <= 2^8 = 256 <= 448: P is never saturated by
// construction.  (k_attn_bf16's defer_thr = 8 and its LAZY bound 2^30 are fine for bf16 P and would saturate here.)
//
// Block = 4 waves = 128 query rows of one (sequence, q-head), as k_attn_bf16 and over the same [n, 4] work tables; K tiles of 64 keys
// bf16 by LDS-DMA, double-buffered (16 KB LDS); V fragments and scales straight from the image (L2: the four waves and the q-heads of a
// kv-head read the same 4 KB).  Mode-1 entries (64 query rows) run without the key split: waves 2, 3 stage their share of K and meet
// the barriers, nothing else.  A plain loop: no software pipelining.
#include "ttv_common.h"
#include "ttv_kernels.h"

#define PV8_KB 64
#define PV8_TILE_BYTES 4224          // 4096 element bytes + 128 scale bytes
#define PV8_K 6.0f                   // P is quantised as p * 2^6
#define PV8_LAG 2.0f                 // the reference lags the running maximum by at most 2 log2 units: p * 2^6 <= 2^8 <= 448
typedef int v8i32 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------
// v columns of the packed q | gate | k | v rows -> MX e4m3 image in the attention kernel's fragment order.
// One block per (tile slot, kv-head); thread (t = tid >> 6, d = tid & 63) owns block (t, d): 32 keys of one column.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_quant_v_pv8(const bf16_t* __restrict__ qkvg, int ld, const int* __restrict__ cu, int n_seqs,
                                                     int v_col0, int kv_heads, uint8_t* __restrict__ image) {
  const int slot = blockIdx.x, kvh = blockIdx.y;
  // the sequence whose tiles hold this slot: the largest i with (cu[i] >> 6) + i <= slot (strictly increasing in i)
  int lo = 0, hi = n_seqs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((cu[mid] >> 6) + mid <= slot) lo = mid; else hi = mid - 1;
  }
  const int s0 = cu[lo], S = cu[lo + 1] - s0;
  const int kt = slot - ((s0 >> 6) + lo);
  if (kt * PV8_KB >= S) return;                    // a slot between two sequences
  const int d = threadIdx.x & 63, t = threadIdx.x >> 6;
  const bf16_t* col = qkvg + (size_t)s0 * ld + v_col0 + kvh * 64 + d;
  const int key0 = kt * PV8_KB + t * 32;
  float v[32];
  float amax = 0.f;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    v[k] = key0 + k < S ? (float)col[(size_t)(key0 + k) * ld] : 0.f;
    amax = fmaxf(amax, fabsf(v[k]));
  }
  // E8M0 byte = biased exponent of the smallest power of two >= amax / 448 (k_quant_mx_fp8)
  const uint32_t tb = __float_as_uint(amax * (1.0f / 448.0f));
  int byte = (int)((tb >> 23) & 0xFF) + ((tb & 0x7FFFFF) ? 1 : 0);
  byte = amax > 0.f ? (byte < 1 ? 1 : (byte > 254 ? 254 : byte)) : 127;
  const float inv = __uint_as_float((uint32_t)(254 - byte) << 23);      // 2^-(byte - 127)
  uint8_t* tile = image + ((size_t)slot * kv_heads + kvh) * PV8_TILE_BYTES;
  const int dt = d >> 5, dr = d & 31;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {               // bytes e = 4 j .. 4 j + 3 of lane half h: keys 8 j + 4 h + 0 .. 3 of the block
      const int k = 8 * j + 4 * h;
      int x = 0;
      x = __builtin_amdgcn_cvt_pk_fp8_f32(v[k] * inv, v[k + 1] * inv, x, false);
      x = __builtin_amdgcn_cvt_pk_fp8_f32(v[k + 2] * inv, v[k + 3] * inv, x, true);
      w[j] = x;
    }
    *reinterpret_cast<uint4*>(tile + dt * 2048 + (32 * h + dr) * 32 + 16 * t) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  tile[4096 + dt * 64 + 32 * t + dr] = (uint8_t)byte;
}

// ------------------------------------------------------------------------------------------------
template <bool GATE>
__global__ __launch_bounds__(256, 3) void k_attn_pv8(const bf16_t* __restrict__ qkvg, int ld, bf16_t* __restrict__ out, int ldo,
                                                     const int* __restrict__ cu, const int* __restrict__ qblocks, int d_model, int gqa, int rep,
                                                     const uint8_t* __restrict__ image) {
  __shared__ __attribute__((aligned(16))) uint4 kl[2][PV8_KB * 8];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int tix = blockIdx.x;
  // work table entry (sequence, first query row, q-head, mode): ttv_attention's tables; sequence < 0 = padding
  const int seq = qblocks[4 * tix], q0 = qblocks[4 * tix + 1], head = qblocks[4 * tix + 2], mode = qblocks[4 * tix + 3];
  if (seq < 0) return;
  const int s0 = cu[seq], S = cu[seq + 1] - s0;
  const int kv_heads = gqa >> 6, kvh = head / rep;
  const bf16_t* qbase = qkvg + (size_t)s0 * ld + head * 64;
  const bf16_t* gbase = qkvg + (size_t)s0 * ld + d_model + head * 64;
  const bf16_t* kbase = qkvg + (size_t)s0 * ld + 2 * d_model + kvh * 64;
  const uint8_t* img = image + ((size_t)((s0 >> 6) + seq) * kv_heads + kvh) * PV8_TILE_BYTES;     // tile 0 of this (sequence, kv-head)
  const size_t img_step = (size_t)kv_heads * PV8_TILE_BYTES;
  const bool active = mode == 0 || wave < 2;        // wave-uniform: a 64-row entry has work for two waves

  // Q fragments (B operand of S^T = K Q^T): lane holds Q[query r][16 ks + 8 h + 0..7]
  const int qrow = q0 + wave * 32 + r;
  const int qrc = qrow < S ? qrow : S - 1;
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qbase + (size_t)qrc * ld + ks * 16 + h * 8);

  // K tiles by LDS-DMA, k_attn_bf16's scheme: instruction i of wave w covers tile rows 8 (2 w + i) .. + 7, lane >> 3 picks the row,
  // lane & 7 the 16-byte LDS chunk; the XOR swizzle is applied on the global side (chunk c holds global chunk c ^ ((row >> 1) & 7)).
  // Rows past the sequence end re-fetch its last row (masked in the scores).
  const uint32_t kl_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&kl[0][0];
  const int drow0 = (wave * 2) * 8 + (lane >> 3), drow1 = drow0 + 8;
  const int kc0 = ((lane & 7) ^ ((drow0 >> 1) & 7)) * 8, kc1 = ((lane & 7) ^ ((drow1 >> 1) & 7)) * 8;
#define DMA16(voff_, base_, dst_)                                                                                \
  do {                                                                                                           \
    unsigned keep__;                                                                                             \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep__) : "v"(voff_), "s"(base_), "s"(dst_) : "memory");                                 \
  } while (0)
#define DMA_K(kt_, buf_)                                                                                         \
  do {                                                                                                           \
    const int key0__ = (kt_) * PV8_KB;                                                                           \
    const bf16_t* kb__ = kbase + (size_t)key0__ * ld;                                                            \
    const uint32_t dk__ = kl_lds + (buf_) * (PV8_KB * 128) + wave * 2048;                                        \
    const int lim__ = S - 1 - key0__;                                                                            \
    const int g0__ = drow0 < lim__ ? drow0 : lim__, g1__ = drow1 < lim__ ? drow1 : lim__;                        \
    DMA16((uint32_t)(g0__ * ld + kc0) * 2u, kb__, dk__);                                                         \
    DMA16((uint32_t)(g1__ * ld + kc1) * 2u, kb__, dk__ + 1024);                                                  \
  } while (0)

  f32x16 o_acc[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o_acc[dt][e] = 0.f;
  float m_ref = 0.f, l_run = 0.f;                   // m_ref: placeholder until the first tile sets it
  f32x16 negoff;                                    // start vector of the score accumulators: -(m_ref - 6) in every register
#pragma unroll
  for (int e = 0; e < 16; ++e) negoff[e] = PV8_K;

  // K fragment (A operand of S^T): key row 32 t + r, 16-byte chunk (2 ks + h) ^ ((row >> 1) & 7)
  const int ksw = (r >> 1) & 7;
  const char* const kbase_lds = reinterpret_cast<const char*>(&kl[0][0]) + r * 128;

  const int nkt = (S + PV8_KB - 1) / PV8_KB;
  DMA_K(0, 0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int buf = kt & 1;
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's share of tile kt has landed
    __syncthreads();                      // tile complete; every wave is done with the other stage
    if (kt + 1 < nkt) DMA_K(kt + 1, buf ^ 1);
    if (!active) continue;

    // V8 fragments and block scales of the tile: requested now, used behind the softmax
    const uint8_t* tile = img + (size_t)kt * img_step;
    const uint4 va0 = *reinterpret_cast<const uint4*>(tile + lane * 32), va1 = *reinterpret_cast<const uint4*>(tile + lane * 32 + 16);
    const uint4 vb0 = *reinterpret_cast<const uint4*>(tile + 2048 + lane * 32), vb1 = *reinterpret_cast<const uint4*>(tile + 2048 + lane * 32 + 16);
    const int vs0 = tile[4096 + lane], vs1 = tile[4096 + 64 + lane];

    // ---- S^T = K Q^T (64 keys x 32 queries per wave): s_acc[t][e] = score of key 32 t + 8 (e >> 2) + 4 h + (e & 3), MINUS off ----
    // As k_attn_bf16's PRE form: the two score chains start from the vector -off (off = m_ref - 6), so a score leaves the matrix pipe
    // as the exponent of p * 2^6 and needs no subtraction; asm with early-clobber outputs, so that neither chain copies the start vector.
    const char* kt_lds = kbase_lds + buf * (PV8_KB * 128);
    f32x16 s_acc[2];
    auto scores = [&]() {
      bf16x8 kf[2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[t][ks] = *reinterpret_cast<const bf16x8*>(kt_lds + t * 4096 + (((2 * ks + h) ^ ksw) << 4));
      asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(s_acc[0]) : "v"(kf[0][0]), "v"(qf[0]), "v"(negoff));
      asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(s_acc[1]) : "v"(kf[1][0]), "v"(qf[0]), "v"(negoff));
#pragma unroll
      for (int ks = 1; ks < 4; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t) s_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[t][ks], qf[ks], s_acc[t], 0, 0, 0);
      // keys past the end of the sequence (last tile only): p = 0 whatever the image holds there
      if (kt * PV8_KB + PV8_KB > S) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = kt * PV8_KB + t * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (key >= S) s_acc[t][e] = -INFINITY;
          }
      }
    };
    // row maximum of the tile's (relative) scores: four chains, then the two lane halves of a query exchange
    auto row_max = [&]() -> float {
      float c4[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int t = c >> 1, e0 = (c & 1) * 8;
        float a = fmaxf(fmaxf(s_acc[t][e0], s_acc[t][e0 + 1]), s_acc[t][e0 + 2]);
        a = fmaxf(fmaxf(a, s_acc[t][e0 + 3]), s_acc[t][e0 + 4]);
        a = fmaxf(fmaxf(a, s_acc[t][e0 + 5]), s_acc[t][e0 + 6]);
        c4[c] = fmaxf(a, s_acc[t][e0 + 7]);
      }
      const float m2 = fmaxf(fmaxf(c4[0], c4[1]), fmaxf(c4[2], c4[3]));
      const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, m2), __builtin_bit_cast(unsigned, m2), false, false);
      const unsigned u0 = sw[0], u1 = sw[1];      // (through named unsigneds: see k_attn_bf16's row_max)
      return fmaxf(__uint_as_float(u0), __uint_as_float(u1));
    };
    // p * 2^6 = exp2(relative score) in place; returns the lane's sum over its 32 keys (two packed chains, fp32)
    auto exp_and_sum = [&]() -> float {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) s_acc[t][e] = __builtin_amdgcn_exp2f(s_acc[t][e]);
      f32x2 ps0 = {0.f, 0.f}, ps1 = {0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
          ps0 += (f32x2){s_acc[t][e], s_acc[t][e + 1]};
          ps1 += (f32x2){s_acc[t][e + 2], s_acc[t][e + 3]};
        }
      ps0 += ps1;
      return ps0[0] + ps0[1];
    };
    scores();
    // ---- the reference ----
    // The tile's row maximum (relative to the reference) decides: a row whose maximum lies more than PV8_LAG above its reference - and
    // every row on an entry's first tile - moves the reference to that maximum, which is then the running maximum; l and O are rescaled
    // by exp2(old - new) (0 after a jump of more than ~150 units, never inf), the tile's scores and the start vector shift with it.
    // Wave-uniform branch: rare once the first tiles have been seen.  (Tried and dropped: k_attn_bf16's LAZY form - no row maximum, a
    // lane whose 32 values sum to more than 448 sends the wave through the tile again.  With P held under 448 the sums trip it in most
    // tiles of a 1 152-key sequence: 79.6 us against 64.3 at the benchmark shape.)
    const float mx = row_max() - PV8_K;
    if (kt == 0 || __builtin_amdgcn_ballot_w64(mx > PV8_LAG) != 0ull) {
      const float d = kt == 0 ? mx : (mx > PV8_LAG ? mx : 0.f);          // first tile: the reference is the placeholder 0
      const float alpha = kt == 0 ? 1.f : __builtin_amdgcn_exp2f(-d);   // nothing accumulated yet on the first tile; 1 for the rows that stay
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o_acc[dt][e] *= alpha;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) s_acc[t][e] -= d;
      m_ref += d;
#pragma unroll
      for (int e = 0; e < 16; ++e) negoff[e] = PV8_K - m_ref;
    }
    const float psum = exp_and_sum();
    l_run += psum;
    // ---- P8^T: the accumulator registers in order ARE the B operand (byte 16 t + e) ----
    v8i32 pb;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int x = 0;
        x = __builtin_amdgcn_cvt_pk_fp8_f32(s_acc[t][4 * j], s_acc[t][4 * j + 1], x, false);
        x = __builtin_amdgcn_cvt_pk_fp8_f32(s_acc[t][4 * j + 2], s_acc[t][4 * j + 3], x, true);
        pb[4 * t + j] = x;
      }
    // ---- O^T += V8^T P8^T: one instruction per d-tile; V's block scales as the A scale (byte 0), B scale 2^0 ----
    const v8i32 va = {(int)va0.x, (int)va0.y, (int)va0.z, (int)va0.w, (int)va1.x, (int)va1.y, (int)va1.z, (int)va1.w};
    const v8i32 vb = {(int)vb0.x, (int)vb0.y, (int)vb0.z, (int)vb0.w, (int)vb1.x, (int)vb1.y, (int)vb1.z, (int)vb1.w};
    o_acc[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, o_acc[0], 0 /* A e4m3 */, 0 /* B e4m3 */, 0, vs0, 0, 0x7F7F7F7F);
    o_acc[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vb, pb, o_acc[1], 0, 0, 0, vs1, 0, 0x7F7F7F7F);
  }
#undef DMA_K
#undef DMA16
  if (!active) return;

  // ---- normalise (the 2^6 of P cancels against the row sum's), gate, store: lane holds O[query r][32 dt + 8 g + 4 h + 0..3] ----
  // as k_attn_bf16: lanes (r, 0), (r, 1) exchange 8-byte groups so that every lane stores 16 consecutive bytes
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv_l = __builtin_amdgcn_rcpf(l_tot);
  bf16_t* orow = out + (size_t)(s0 + qrc) * ldo + head * 64;
  const bf16_t* grow = gbase + (size_t)qrc * ld;
  const bool store = qrow < S;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      uint2 pk[2];
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int g = 2 * gp + gg;
        const int d0 = dt * 32 + 8 * g + 4 * h;
        f32x4 v = {o_acc[dt][4 * g] * inv_l, o_acc[dt][4 * g + 1] * inv_l, o_acc[dt][4 * g + 2] * inv_l, o_acc[dt][4 * g + 3] * inv_l};
        if (GATE) {
          const f32x4 gt = Vec4<bf16_t>::load(grow + d0);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gt[e] * -1.44269504088896340736f));
        }
        const bf16x4 b4 = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
        pk[gg] = __builtin_bit_cast(uint2, b4);
      }
      const auto sx = __builtin_amdgcn_permlane32_swap(pk[0].x, pk[1].x, false, false);
      const auto sy = __builtin_amdgcn_permlane32_swap(pk[0].y, pk[1].y, false, false);
      const uint4 o16 = {sx[0], sy[0], sx[1], sy[1]};
      if (store) *reinterpret_cast<uint4*>(orow + dt * 32 + 16 * gp + 8 * h) = o16;
    }
}

// ------------------------------------------------------------------------------------------------
int64_t ttvk_attention_pv8_bytes(int total_rows, int n_seqs, int kv_heads) {
  if (total_rows < 0 || n_seqs < 0 || kv_heads <= 0) return -1;
  return ((int64_t)(total_rows >> 6) + n_seqs) * kv_heads * PV8_TILE_BYTES;
}

int ttvk_quant_v_pv8(const void* qkvg, int ld, const int* cu_seqlens, int n_seqs, int total_rows, int q_heads, int kv_heads, void* image,
                     hipStream_t s) {
  TTV_CHECK_ARG(n_seqs >= 0 && total_rows >= 0, "quant_v_pv8: negative sizes");
  if (n_seqs == 0 || total_rows == 0) return TTV_OK;
  TTV_CHECK_ARG(kv_heads > 0 && q_heads > 0 && q_heads % kv_heads == 0, "quant_v_pv8: q_heads %% kv_heads");
  const int d_model = q_heads * 64, gqa = kv_heads * 64;
  TTV_CHECK_ARG(ld >= 2 * d_model + 2 * gqa, "quant_v_pv8: ld %d is smaller than the q | gate | k | v row of 64-wide heads (%d)", ld, 2 * d_model + 2 * gqa);
  TTV_CHECK_ARG(qkvg && cu_seqlens && image && (uintptr_t)qkvg % 2 == 0 && (uintptr_t)image % 16 == 0, "quant_v_pv8: null / unaligned pointers (image: 16 bytes)");
  const int slots = (total_rows >> 6) + n_seqs;
  TTV_CHECK_ARG(kv_heads <= 65535, "quant_v_pv8: too many kv-heads");
  hipLaunchKernelGGL(k_quant_v_pv8, dim3(slots, kv_heads), dim3(128), 0, s, (const bf16_t*)qkvg, ld, cu_seqlens, n_seqs, 2 * d_model + gqa, kv_heads,
                     (uint8_t*)image);
  TTV_CHECK_LAUNCH("quant_v_pv8");
  return TTV_OK;
}

// flags: TTV_ATTN_GATE (optional) and TTV_ATTN_QSCALED (required: the caller's statement that q carries head_dim^-0.5 * log2(e))
int ttvk_attention_pv8(const void* qkvg, int ld, void* out, int ldo, const int* cu_seqlens, const int* qblocks, int n_qblocks, int q_heads,
                       int kv_heads, int head_dim, int flags, const void* image, hipStream_t s) {
  TTV_CHECK_ARG(head_dim == 64, "attention_pv8: head_dim %d unsupported (the image and the kernel are built for 64)", head_dim);
  TTV_CHECK_ARG(flags & TTV_ATTN_QSCALED, "attention_pv8: q must arrive pre-scaled by head_dim^-0.5 * log2(e) (TTV_ATTN_QSCALED; ttv_layer_weights.qkv_q_prescaled)");
  TTV_CHECK_ARG(!(flags & ~(TTV_ATTN_GATE | TTV_ATTN_QSCALED)), "attention_pv8: flags 0x%x - only TTV_ATTN_GATE beside TTV_ATTN_QSCALED", flags);
  TTV_CHECK_ARG(n_qblocks >= 0, "attention_pv8: negative table length");
  if (n_qblocks == 0) return TTV_OK;
  TTV_CHECK_ARG(kv_heads > 0 && q_heads > 0 && q_heads % kv_heads == 0, "attention_pv8: q_heads %% kv_heads");
  const int d_model = q_heads * 64, gqa = kv_heads * 64, rep = q_heads / kv_heads;
  TTV_CHECK_ARG(ld >= 2 * d_model + 2 * gqa && ld % 8 == 0 && ldo >= d_model && ldo % 8 == 0, "attention_pv8: bad leading dims");
  TTV_CHECK_ARG(qkvg && out && cu_seqlens && qblocks && image, "attention_pv8: null pointer");
  TTV_CHECK_ARG((uintptr_t)qkvg % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)image % 16 == 0, "attention_pv8: unaligned pointers (qkvg, out, image: 16 bytes)");
  TtvProfScope prof(TTV_KC_ATTENTION, s);
  if (flags & TTV_ATTN_GATE)
    hipLaunchKernelGGL((k_attn_pv8<true>), dim3(n_qblocks), dim3(256), 0, s, (const bf16_t*)qkvg, ld, (bf16_t*)out, ldo, cu_seqlens, qblocks, d_model, gqa, rep,
                       (const uint8_t*)image);
  else
    hipLaunchKernelGGL((k_attn_pv8<false>), dim3(n_qblocks), dim3(256), 0, s, (const bf16_t*)qkvg, ld, (bf16_t*)out, ldo, cu_seqlens, qblocks, d_model, gqa, rep,
                       (const uint8_t*)image);
  TTV_CHECK_LAUNCH("attention_pv8");
  return TTV_OK;
}
