// The encoder's front in one kernel (width 256, bf16): patchify + proj_in + mask token + ln_pre_p (reference blocks.py:91-97,
// utils.py:26-34), x[patch_rows[t]] = RMSNorm(bf16(bf16(clip_patch(t) . W^T + bias) + mask_token)) * gain.
//
// Before: k_gemm_bf16<EPI_STORE, GATHER> (register-staged, a barrier per k-tile, 128 of the 256 features per block, so every patch is
// gathered twice) writes the sums as bf16 [P, 256], and a row kernel reads them back to normalise them into x.  Here a block owns 128
// patches x all 256 features, so the row statistic stays inside the block and the sums never leave it:
//   * 8 waves = 2 feature halves x 4 token quarters, a wave keeps 128 x 32 outputs (8 x 2 accumulator tiles of v_mfma_f32_16x16x32_bf16);
//   * k-tiles of 64 in ascending k, one accumulator chain per output, the fragment <-> k assignment of k_gemm_bf16: the dot products
//     are the bits that kernel produces, and so is everything up to the rounded sum the norm reads;
//   * both operands arrive by LDS-DMA (global_load_lds_dwordx4) into a ring of three 48 KiB stages, two k-tiles ahead of the MFMAs.  A
//     wave-instruction fills 8 tile rows of 128 bytes lane-linearly, so the XOR swizzle of the fragment reads is applied on the source
//     (k_gemm_bf16_dma's scheme); the patch operand takes a 64-bit address per lane, which makes the gather free: a 16-byte chunk is the
//     pw = 8 pixels of one (c, ipt, iph) image row of the patch;
//   * one barrier per k-tile; the wait in front of it is counted (the six pieces of the next k-tile stay in flight);
//   * epilogue: bias, rounding, mask token, rounding (what the stored bf16 sum was), the row's sum of squares over the lane's 32
//     features summed in the row kernel's order (see the epilogue), then the norm and 8-byte stores.
// Every output is the bit the two-kernel sequence produces (tests/test_hip_encoder_edges.py).
#include "ttv_common.h"
#include "ttv_kernels.h"

#define PE_TT 128            // patches per block
#define PE_F 256             // features = the tower's width
#define PE_BK 64
#define PE_STAGES 3
#define PE_STAGE_U4 ((PE_F + PE_TT) * 8)      // uint4 per stage: 256 weight rows, then 128 patch rows, 128 bytes each

struct PatchEmbedDev {
  ClipPtrs clips;
  const int* clip_desc; const int* patch_rows; const int* row_seq;
  const bf16_t* w; const bf16_t* bias; const float* mask_token; const float* gain;
  bf16_t* x;
  int ldw, ldx, M, K, clip0, pt_shift, ph_shift;
  float eps;
};

__global__ __launch_bounds__(512, 1) void k_patch_embed256(PatchEmbedDev p) {
  __shared__ __attribute__((aligned(16))) uint4 lds[PE_STAGES][PE_STAGE_U4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wf = wave & 1, wt = wave >> 1;
  const int tbase = blockIdx.x * PE_TT;

  // ---- staging addresses: wave w stages weight rows 32 w .. + 31 (4 instructions of 8 rows) and patch rows 16 w .. + 15 (2) ----
  const int lr = lane >> 3, lp = lane & 7;
  uint32_t woff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = wave * 32 + i * 8 + lr;
    woff[i] = ((uint32_t)row * (uint32_t)p.ldw + (uint32_t)((lp ^ ((row >> 1) & 7)) * 8)) * 2u;
  }
  const bf16_t* gbase[2];
  int gthw[2], ghw[2], gw_[2], gch[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * 16 + i * 8 + lr;
    int t = tbase + row;
    t = t < p.M ? t : p.M - 1;
    const int ci = p.row_seq[p.patch_rows[t]];
    const int* ds = p.clip_desc + (size_t)ci * 8;
    const int Tn = ds[0], H = ds[1], W = ds[2], gh = ds[4], gw = ds[5], pl = t - ds[6];
    const int gwi = pl % gw, r = pl / gw, ghi = r % gh, gti = r / gh;
    gthw[i] = Tn * H * W; ghw[i] = H * W; gw_[i] = W;
    gch[i] = lp ^ ((row >> 1) & 7);
    gbase[i] = reinterpret_cast<const bf16_t*>(p.clips.p[ci - p.clip0]) + ((size_t)((gti << p.pt_shift) * H + (ghi << p.ph_shift)) * W + gwi * 8);
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&lds[0][0];
  constexpr uint32_t STAGEB = PE_STAGE_U4 * 16;
#define PE_DMA_W(voff_, base_, dst_)                                                                             \
  do {                                                                                                           \
    unsigned keep__;                                                                                             \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep__) : "v"(voff_), "s"(base_), "s"(dst_) : "memory");                                 \
  } while (0)
#define PE_DMA_X(ptr_, dst_)                                                                                     \
  do {                                                                                                           \
    unsigned keep__;                                                                                             \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep__) : "v"(ptr_), "s"(dst_) : "memory");                                              \
  } while (0)
  // the six pieces of k-tile kt_ into stage st_
#define PE_STAGE(kt_, st_)                                                                                       \
  do {                                                                                                           \
    const bf16_t* wb__ = p.w + (size_t)(kt_) * PE_BK;                                                            \
    const uint32_t dw__ = lds0 + (st_) * STAGEB + wave * 4096;                                                   \
    const uint32_t dx__ = lds0 + (st_) * STAGEB + PE_F * 128 + wave * 2048;                                      \
    _Pragma("unroll") for (int i__ = 0; i__ < 4; ++i__) PE_DMA_W(woff[i__], wb__, dw__ + i__ * 1024);            \
    _Pragma("unroll") for (int i__ = 0; i__ < 2; ++i__) {                                                        \
      const int sg__ = (kt_) * 8 + gch[i__];                                                                     \
      const int c__ = sg__ >> (p.pt_shift + p.ph_shift), ipt__ = (sg__ >> p.ph_shift) & ((1 << p.pt_shift) - 1); \
      const int iph__ = sg__ & ((1 << p.ph_shift) - 1);                                                          \
      const bf16_t* src__ = gbase[i__] + ((size_t)c__ * gthw[i__] + (size_t)ipt__ * ghw[i__] + (size_t)iph__ * gw_[i__]); \
      PE_DMA_X(src__, dx__ + i__ * 1024);                                                                        \
    }                                                                                                            \
  } while (0)

  f32x4 acc[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int l15 = lane & 15, kq = lane >> 4;
  const int nk = p.K / PE_BK;
  // fragment byte offsets inside a stage: row 16 i + l15 (+ a multiple of 32), chunk (4 ks + kq) ^ ((row >> 1) & 7) = ^ ((l15 >> 1) & 7)
  const char* const ldsb = reinterpret_cast<const char*>(&lds[0][0]);
  const uint32_t fo0 = (uint32_t)(l15 * 128 + (((0 + kq) ^ ((l15 >> 1) & 7)) << 4));
  const uint32_t fo1 = (uint32_t)(l15 * 128 + (((4 + kq) ^ ((l15 >> 1) & 7)) << 4));
  const uint32_t a_base = (uint32_t)(wf * 128 * 128), b_base = (uint32_t)(PE_F * 128 + wt * 32 * 128);

  // The descriptor loads above have landed before the first piece is issued: the compiler's wait-count pass does not see the LDS-DMA
  // instructions (inline assembly), so a counted wait of its own for an older load would come out too weak once pieces are in flight.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PE_STAGE(0, 0);
  if (nk > 1) PE_STAGE(1, 1);
  int st = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // this wave's pieces of k-tile kt have landed (those of kt + 1, issued behind them, may still fly), then everybody's; the barrier
    // also says that every wave has finished reading stage (kt - 1) % 3, which the pieces issued below overwrite
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 2 < nk) {
      const int st2 = st + 2 >= PE_STAGES ? st + 2 - PE_STAGES : st + 2;
      PE_STAGE(kt + 2, st2);
    }
    const char* const sb = ldsb + (size_t)st * STAGEB;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint32_t fo = ks ? fo1 : fo0;
      bf16x8 a[8], b[2];
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = *reinterpret_cast<const bf16x8*>(sb + a_base + fo + i * 2048);
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const bf16x8*>(sb + b_base + fo + j * 2048);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    st = st + 1 == PE_STAGES ? 0 : st + 1;
  }
#undef PE_STAGE
#undef PE_DMA_W
#undef PE_DMA_X

  // ---- epilogue: lane (l15, kq) holds features wf * 128 + 16 i + 4 kq .. + 3 of tokens wt * 32 + 16 j + l15 ----
  const float sc = round_to<bf16_t>(p.mask_token[0]);
  // The row statistic in k_rmsnorm's own order, so that rstd - and with it every output - is the bit the row kernel produces: there lane
  // L = f / 4 of a wave squares features 4 L .. 4 L + 3 (e1^2, then e0, e2, e3 by fma) and the wave adds partners L ^ 32, 16, 8, 4, 2, 1.
  // Here L = 32 wf + 4 i + kq: the feature halves meet first, per group of four (through LDS: stage `st` is idle - last read three k-tiles
  // ago, no piece in flight), then the lane's own i ^ 4, i ^ 2, i ^ 1, then kq ^ 2 and kq ^ 1 (lanes ^ 32, ^ 16).  Rows of 33 words: no bank conflicts.
  float* const gx = reinterpret_cast<float*>(&lds[st][0]);
  float grp[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int f = wf * 128 + i * 16 + kq * 4;
    const f32x4 bv = Vec4<bf16_t>::load(p.bias + f);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      acc[i][j] += bv;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        // the Linear output is rounded to bf16 before the scalar is added (blocks.py:97), and the sum was stored as bf16
        acc[i][j][e] = round_to<bf16_t>(round_to<bf16_t>(acc[i][j][e]) + sc);
      const f32x4 y = acc[i][j];
      grp[i][j] = fmaf(y[3], y[3], fmaf(y[2], y[2], fmaf(y[0], y[0], y[1] * y[1])));
      gx[(wf * PE_TT + wt * 32 + j * 16 + l15) * 33 + i * 4 + kq] = grp[i][j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tl = wt * 32 + j * 16 + l15;
    const int t = tbase + tl;
    float s1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s1[i] = grp[i][j] + gx[((wf ^ 1) * PE_TT + tl) * 33 + i * 4 + kq];
    const float t0 = s1[0] + s1[4], t1 = s1[1] + s1[5], t2 = s1[2] + s1[6], t3 = s1[3] + s1[7];
    float tot = (t0 + t2) + (t1 + t3);
    tot = pair32_sum(tot);
    {
      const unsigned u = __float_as_uint(tot);
      const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
      const unsigned a0 = a[0], a1 = a[1];
      tot = __uint_as_float(a0) + __uint_as_float(a1);
    }
    const float rstd = 1.0f / sqrtf(tot / 256.0f + p.eps);
    if (t < p.M) {
      bf16_t* const q = p.x + (size_t)p.patch_rows[t] * p.ldx;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int f = wf * 128 + i * 16 + kq * 4;
        const f32x4 g = *reinterpret_cast<const f32x4*>(p.gain + f);
        const f32x4 o = {acc[i][j][0] * rstd * g[0], acc[i][j][1] * rstd * g[1], acc[i][j][2] * rstd * g[2], acc[i][j][3] * rstd * g[3]};
        Vec4<bf16_t>::store(q + f, o);
      }
    }
  }
}

bool ttvk_patch_embed_norm_supported(int dtype, int width, int patch_dim, int patch_w) {
  return dtype == TTV_BF16 && width == PE_F && patch_dim % PE_BK == 0 && patch_dim >= PE_BK && patch_w == 8;
}

int ttvk_patch_embed_norm(void* const* clips, int clip0, int n_clips, const int* clip_desc, const int* patch_rows, const int* row_seq,
                          int patch_t, int patch_h, int patch_w, int patch_dim, const void* w, int ldw, const void* bias,
                          const float* mask_token, const float* gain, float eps, void* x, int ldx, int M, hipStream_t s) {
  if (M == 0) return TTV_OK;
  auto lg2 = [](int v) { int sh = 0; while ((1 << sh) < v) ++sh; return (1 << sh) == v ? sh : -1; };
  TTV_CHECK_ARG(patch_w == 8 && lg2(patch_t) >= 0 && lg2(patch_h) >= 0 && patch_dim % PE_BK == 0 && patch_dim >= PE_BK &&
                    patch_dim % (patch_t * patch_h * patch_w) == 0,
                "patch_embed_norm: patch_w == 8, power-of-two patch_t / patch_h and a patch vector that is a multiple of 64");
  TTV_CHECK_ARG(n_clips > 0 && n_clips <= TTV_MAX_CLIPS_PER_LAUNCH, "patch_embed_norm: 1 .. %d clips per call", TTV_MAX_CLIPS_PER_LAUNCH);
  TTV_CHECK_ARG(ldw >= patch_dim && ldw % 8 == 0 && ldx >= PE_F && ldx % 4 == 0 && (uint64_t)PE_F * (uint64_t)ldw * 2u < (1ull << 32),
                "patch_embed_norm: leading dims must hold a row and keep its alignment");
  TTV_CHECK_ARG((uintptr_t)w % 16 == 0 && (uintptr_t)x % 8 == 0 && (uintptr_t)bias % 8 == 0 && (uintptr_t)gain % 16 == 0,
                "patch_embed_norm: pointers must keep their vector alignment");
  PatchEmbedDev d;
  for (int i = 0; i < n_clips; ++i) {
    TTV_CHECK_ARG(clips[i] && (uintptr_t)clips[i] % 16 == 0, "patch_embed_norm: clip %d is null or not 16-byte aligned", i);
    d.clips.p[i] = clips[i];
  }
  for (int i = n_clips; i < TTV_MAX_CLIPS_PER_LAUNCH; ++i) d.clips.p[i] = nullptr;
  d.clip_desc = clip_desc; d.patch_rows = patch_rows; d.row_seq = row_seq;
  d.w = (const bf16_t*)w; d.bias = (const bf16_t*)bias; d.mask_token = mask_token; d.gain = gain; d.x = (bf16_t*)x;
  d.ldw = ldw; d.ldx = ldx; d.M = M; d.K = patch_dim; d.clip0 = clip0; d.pt_shift = lg2(patch_t); d.ph_shift = lg2(patch_h);
  d.eps = eps;
  TtvProfScope prof(TTV_KC_GEMM_STORE, s);
  hipLaunchKernelGGL(k_patch_embed256, dim3(ttv_cdiv(M, PE_TT)), dim3(512), 0, s, d);
  TTV_CHECK_LAUNCH("patch_embed256");
  return TTV_OK;
}
