// LPIPS + Gram perceptual terms of the generator loss (reference model/metrics/lpips_gram.py, LPIPS.forward; used by
// model/losses/loss_module.py:121-138).  Forward of the VGG16 features[0:30] trunk on a stack of 2n images (n reconstruction
// crops, then n target crops), the LPIPS head on the five taps relu1_2 .. relu5_3, the optional Gram term, and the input-gradient
// backward into the n reconstruction crops (weights are frozen: no weight gradients).
//
// Layout: activations NHWC, the images of a call stacked into one tall image of N*H rows ("tall rows"), so a tile may span two
// images at the small stages; a tap whose source row leaves its own image reads zero (the per-image zero padding).
//
// Kernels
//   k_conv_mfma  : bf16 3x3 / stride 1 / pad 1 convolution as an implicit GEMM on v_mfma_f32_16x16x32_bf16.  One workgroup
//                  (4 waves) owns 128 output pixels (a TH x TW block of tall rows x columns, TW = 16 or the power of two >= W,
//                  at least 4) x 64 output channels.  Per 32-channel input chunk the block plus its one-pixel halo and the 9 x 64 x 32
//                  weight slice are staged in LDS once and all 9 taps read shifted windows of it (no im2col); the next chunk's
//                  global loads are issued into registers before the current chunk's MFMAs.  MFMA A = weights (rows = output
//                  channels), B = pixels, so a lane owns 4 consecutive output channels of one pixel: 8-byte NHWC stores.
//                  Layers whose tile count leaves the chip under-filled split the input chunks over S workgroups (S <= 8, a
//                  power of two): fp32 partials to the workspace, summed in the fixed order s = 0 .. S-1 by k_conv_splitk.
//                  Epilogues: forward (bias, ReLU), dgrad masked by (h > 0) where h is the forward activation below, dgrad raw.
//   k_conv_direct: plain fp32-FMA convolution, one thread per output element: every layer but conv1_1 of the fp32 path (exact
//                  fp32, the correctness anchor, not timed), and the single-op entry point's shapes the MFMA tile does not take.
//   k_conv_first / k_conv_last : conv1_1 forward (Cin = 3, read from the NCHW crops; the scaled input is rounded to T as autocast
//                  feeds the reference's first conv) and its dgrad (Cout = 3, written NCHW and divided by scale), one thread per pixel
//                  with fp32 FMAs, both dtypes.  Deliberate choice: these two layers hold 0.6 % of the network's FLOPs and do not
//                  take the MFMA path.
//   k_pool       : 2 x 2 / 2 max-pool forward.
//   k_route      : max-pool backward + head gradient + ReLU mask: the gradient of a pooled output goes to the FIRST maximum of
//                  its window in row-major order (torch max_pool2d), then += head gradient (fp32), then * (h > 0).
//   k_head_fwd / k_head_bwd : LPIPS head per tap, one 16-lane row per pixel: normalise both features (eps in the sqrt and added again,
//                  the second normalize_tensor of lpips_gram.py), sum_c lin_c (u_c - v_c)^2, all fp32.  Per-(image, 64-pixel
//                  block) partials (double) reduced in a fixed order by k_head_finish.  No float atomics on this path: identical
//                  inputs give identical bits for the loss and the gradient.
//   k_gram_diff / k_gram_bwd : Gram term, plain fp32 loops (correctness before speed; off in the reference's configs):
//                  D = (F0^T F0 - F1^T F1) / hw per image and tap, sum D^2 per block -> partials; backward
//                  dF0 += g * 4 / (5 C^2 hw) * F0 D.  One launch per tap.
//
//   k_conv_first_clip / k_eval_finish : the evaluation path (per-frame LPIPS of whole frames of any size 16 .. 2048, no tape): conv1_1
//                  read in place from frame t of a [3][T][H][W] clip with the reconstruction's clamp fused, and the finish step that
//                  is given each tap's true pixel count (H >> k)(W >> k) and adds the per-frame values to a double [sum, count] pair
//                  in frame order.  Everything between is the kernels above: k_conv_mfma tiles partial columns and odd per-image
//                  heights as it is (columns >= W and rows >= R load zero and are not stored; the image row is (tall row) % H),
//                  k_pool floors with the input's own pitch, k_head_fwd takes any hw.
//
// The lin layers are applied with eval semantics (no dropout), the way the reference builds the module (.eval()).
#include "ttv_common.h"
#include "ttv_kernels.h"

#include <algorithm>
#include <utility>

namespace {

constexpr int LP_LAYERS = 13;
constexpr int LP_CIN[LP_LAYERS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_LAYERS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_STAGE[LP_LAYERS] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};   // spatial stage (H >> stage)
constexpr int LP_TAP_LAYER[5] = {1, 3, 6, 9, 12};                              // relu1_2 .. relu5_3; the first four feed a pool
constexpr int LP_TAP_C[5] = {64, 128, 256, 512, 512};
__constant__ float c_shift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float c_scale[3] = {0.458f, 0.448f, 0.450f};

constexpr int CM_TP = 128;       // output pixels per tile
constexpr int CM_TN = 64;        // output channels per tile
constexpr int CM_K = 32;         // input channels per chunk
constexpr int CM_P = 40;         // LDS pitch in bf16 of a 32-channel record (80 B: 16-byte aligned, rows spread over banks)
constexpr int CM_SPMAX = 204;    // staged pixels at most: (TH + 2)(TW + 2) for TW in {4, 8, 16} -> 204, 180, 180
constexpr int CM_IN_IT = (CM_SPMAX * 4 + 255) / 256;   // 16-byte input loads per thread per chunk

enum { MODE_FWD = 0, MODE_MASK = 1, MODE_RAW = 2 };

int cm_tw(int W) {
  int tw = 4;
  while (tw < W && tw < 16) tw *= 2;
  return tw;
}

template <typename T>
__device__ __forceinline__ float epi(float v, int mode, float bias, const T* h, size_t idx) {
  if (mode == MODE_FWD) return fmaxf(v + bias, 0.0f);
  if (mode == MODE_MASK) return Cvt<T>::to_f(h[idx]) > 0.0f ? v : 0.0f;
  return v;
}

// ---- bf16 implicit-GEMM convolution ------------------------------------------------------------------------------------
// x: [R = N*H][W][Cin] bf16; wm: [Cin/32][9][Cout][32] bf16; y: [R][W][Cout] (or fp32 partials [S][R][W][Cout] when part).
__global__ __launch_bounds__(256) void k_conv_mfma(const bf16_t* __restrict__ x, int H, int R, int W, int Cin, int Cout,
                                                   const bf16_t* __restrict__ wm, const float* __restrict__ bias, int mode,
                                                   const bf16_t* __restrict__ h, bf16_t* __restrict__ y, float* __restrict__ part,
                                                   int TWl) {
  __shared__ __attribute__((aligned(16))) bf16_t s_in[CM_SPMAX * CM_P];
  __shared__ __attribute__((aligned(16))) bf16_t s_w[9 * CM_TN * CM_P];
  const int TW = 1 << TWl, TH = CM_TP >> TWl, SW = TW + 2, SP = (TH + 2) * SW;
  const int tiles_x = (W + TW - 1) >> TWl;
  const int gy0 = (blockIdx.x / tiles_x) * TH, x0 = (blockIdx.x % tiles_x) * TW;
  const int n0 = blockIdx.y * CM_TN;
  const int nk = Cin / CM_K, S = gridDim.z, s = blockIdx.z;
  const int kc0 = s * nk / S, kc1 = (s + 1) * nk / S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // per-lane pixel of each B fragment, and whether its rows above / below lie in the same image
  int poff[2];
  bool ok_top[2], ok_bot[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = wave * 32 + j * 16 + (lane & 15);
    const int ty = p >> TWl, tx = p & (TW - 1);
    poff[j] = ty * SW + tx;
    const int yl = (gy0 + ty) % H;
    ok_top[j] = yl > 0;
    ok_bot[j] = yl < H - 1;
  }

  // the weight registers are nine named values: as an array they are kept in scratch
  uint4 rin[CM_IN_IT], rw0, rw1, rw2, rw3, rw4, rw5, rw6, rw7, rw8;
#define CM_FETCH(kc_)                                                                                                          \
  do {                                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < CM_IN_IT; ++i) {                                                                     \
      const int u = tid + 256 * i, sp = u >> 2, q = u & 3;                                                                     \
      const int g = gy0 - 1 + sp / SW, xx = x0 - 1 + sp % SW;                                                                 \
      const bool in = sp < SP && g >= 0 && g < R && xx >= 0 && xx < W;                                                         \
      rin[i] = in ? *reinterpret_cast<const uint4*>(x + ((size_t)g * W + xx) * Cin + (kc_) * CM_K + q * 8) : make_uint4(0, 0, 0, 0); \
    }                                                                                                                          \
    const bf16_t* wsrc_ = wm + ((size_t)(kc_) * 9 * Cout + n0 + (tid >> 2)) * CM_K + (tid & 3) * 8;                        \
    const size_t wt_ = (size_t)Cout * CM_K;                                                                                    \
    rw0 = *reinterpret_cast<const uint4*>(wsrc_);                                                                              \
    rw1 = *reinterpret_cast<const uint4*>(wsrc_ + wt_);                                                                        \
    rw2 = *reinterpret_cast<const uint4*>(wsrc_ + 2 * wt_);                                                                    \
    rw3 = *reinterpret_cast<const uint4*>(wsrc_ + 3 * wt_);                                                                    \
    rw4 = *reinterpret_cast<const uint4*>(wsrc_ + 4 * wt_);                                                                    \
    rw5 = *reinterpret_cast<const uint4*>(wsrc_ + 5 * wt_);                                                                    \
    rw6 = *reinterpret_cast<const uint4*>(wsrc_ + 6 * wt_);                                                                    \
    rw7 = *reinterpret_cast<const uint4*>(wsrc_ + 7 * wt_);                                                                    \
    rw8 = *reinterpret_cast<const uint4*>(wsrc_ + 8 * wt_);                                                                    \
  } while (0)

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  CM_FETCH(kc0);   // kc0 < kc1: S <= Cin / 32
  for (int kc = kc0; kc < kc1; ++kc) {
    __syncthreads();   // the previous chunk's MFMAs have read the LDS
#pragma unroll
    for (int i = 0; i < CM_IN_IT; ++i) {
      const int u = tid + 256 * i, sp = u >> 2, q = u & 3;
      if (sp < SP) *reinterpret_cast<uint4*>(s_in + sp * CM_P + q * 8) = rin[i];
    }
    {
      bf16_t* dst = s_w + (tid >> 2) * CM_P + (tid & 3) * 8;
      constexpr int ts = CM_TN * CM_P;
      *reinterpret_cast<uint4*>(dst) = rw0;
      *reinterpret_cast<uint4*>(dst + ts) = rw1;
      *reinterpret_cast<uint4*>(dst + 2 * ts) = rw2;
      *reinterpret_cast<uint4*>(dst + 3 * ts) = rw3;
      *reinterpret_cast<uint4*>(dst + 4 * ts) = rw4;
      *reinterpret_cast<uint4*>(dst + 5 * ts) = rw5;
      *reinterpret_cast<uint4*>(dst + 6 * ts) = rw6;
      *reinterpret_cast<uint4*>(dst + 7 * ts) = rw7;
      *reinterpret_cast<uint4*>(dst + 8 * ts) = rw8;
    }
    __syncthreads();
    CM_FETCH(min(kc + 1, kc1 - 1));   // unconditional (the last one reloads the current chunk): keeps the registers out of scratch
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int kh = t / 3, kw = t % 3;
      bf16x8 a[4], b[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8*>(s_w + (t * CM_TN + i * 16 + (lane & 15)) * CM_P + 8 * (lane >> 4));
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool ok = kh == 1 || (kh == 0 ? ok_top[j] : ok_bot[j]);
        const uint4 v = *reinterpret_cast<const uint4*>(s_in + (poff[j] + kh * SW + kw) * CM_P + 8 * (lane >> 4));
        b[j] = __builtin_bit_cast(bf16x8, ok ? v : make_uint4(0, 0, 0, 0));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: lane owns output channels n0 + 16 i + 4 (lane >> 4) + r of pixel wave * 32 + 16 j + (lane & 15)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = wave * 32 + j * 16 + (lane & 15);
    const int go = gy0 + (p >> TWl), xx = x0 + (p & (TW - 1));
    const bool valid = go < R && xx < W;
    const size_t pix = (size_t)go * W + xx;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!valid) break;
      const int c = n0 + i * 16 + 4 * (lane >> 4);
      const size_t idx = pix * Cout + c;
      if (part) {
        *reinterpret_cast<f32x4*>(part + (size_t)s * R * W * Cout + idx) = acc[i][j];
      } else {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = epi<bf16_t>(acc[i][j][r], mode, mode == MODE_FWD ? bias[c + r] : 0.f, h, idx + r);
        Vec4<bf16_t>::store(y + idx, v);
      }
    }
  }
}

#undef CM_FETCH

// fixed-order sum of the S split-K partials + epilogue; 4 consecutive channels per thread
template <typename T>
__global__ __launch_bounds__(256) void k_conv_splitk(const float* __restrict__ part, int S, size_t total, int Cout,
                                                     const float* __restrict__ bias, int mode, const T* __restrict__ h, T* __restrict__ y) {
  const size_t q = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (q >= total) return;
  f32x4 v = *reinterpret_cast<const f32x4*>(part + q);
  for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(part + (size_t)s * total + q);
  const int c = (int)(q % Cout);
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = epi<T>(v[r], mode, mode == MODE_FWD ? bias[c + r] : 0.f, h, q + r);
  Vec4<T>::store(y + q, v);
}

// ---- direct convolution (fp32 path) ---------------------------------------------------------------------------------------
// x: NHWC [N][H][W][Cin]; wg: [9][Cin][Cout] (T); y: NHWC [N][H][W][Cout] with the mode's epilogue.  Taps in order, channels inside.
template <typename T>
__global__ __launch_bounds__(256) void k_conv_direct(const T* __restrict__ x, int N, int H, int W, int Cin, int Cout, const T* __restrict__ wg,
                                                     const float* __restrict__ bias, int mode, const T* __restrict__ h, T* __restrict__ y) {
  const size_t total = (size_t)N * H * W * Cout;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int co = (int)(e % Cout);
    const size_t pix = e / Cout;
    const int xx = (int)(pix % W), yy = (int)((pix / W) % H), img = (int)(pix / ((size_t)W * H));
    float acc = 0.f;
    for (int kh = 0; kh < 3; ++kh) {
      const int sy = yy + kh - 1;
      if (sy < 0 || sy >= H) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int sx = xx + kw - 1;
        if (sx < 0 || sx >= W) continue;
        const T* wt = wg + (size_t)(kh * 3 + kw) * Cin * Cout + co;
        const T* src = x + (((size_t)img * H + sy) * W + sx) * Cin;
        for (int ci = 0; ci < Cin; ++ci) acc = fmaf(Cvt<T>::to_f(src[ci]), Cvt<T>::to_f(wt[(size_t)ci * Cout]), acc);
      }
    }
    y[e] = Cvt<T>::from_f(epi<T>(acc, mode, mode == MODE_FWD ? bias[co] : 0.f, h, e));
  }
}

// conv1_1 forward: one thread per pixel, all 64 output channels.  The 27 scaled inputs ((v - shift) / scale in fp32, rounded to T)
// are gathered once into registers; the weights ([9][3][64], wave-uniform addresses) and bias are read as scalars.  Same tap-major
// accumulation order as k_conv_direct.  Images 0 .. nsplit-1 come from x, the rest from x2 (both NCHW).
template <typename T>
__global__ __launch_bounds__(256) void k_conv_first(const T* __restrict__ x, const T* __restrict__ x2, int nsplit, int N, int H, int W,
                                                    const T* __restrict__ wg, const float* __restrict__ bias, T* __restrict__ y) {
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (size_t)N * H * W) return;
  const int xx = (int)(pix % W), yy = (int)((pix / W) % H), img = (int)(pix / ((size_t)W * H));
  const T* src = img < nsplit ? x + (size_t)img * 3 * H * W : x2 + (size_t)(img - nsplit) * 3 * H * W;
  float v[27];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int sy = yy + t / 3 - 1, sx = xx + t % 3 - 1;
    const bool in = sy >= 0 && sy < H && sx >= 0 && sx < W;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
      v[t * 3 + ci] = in ? round_to<T>((Cvt<T>::to_f(src[((size_t)ci * H + sy) * W + sx]) - c_shift[ci]) / c_scale[ci]) : 0.f;
  }
  T* out = y + pix * 64;
  for (int c0 = 0; c0 < 64; c0 += 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(v[k], Cvt<T>::to_f(wg[k * 64 + c0 + j]), acc[j]);
#pragma unroll
    for (int j = 0; j < 8; j += 4) {
      f32x4 o = {fmaxf(acc[j] + bias[c0 + j], 0.f), fmaxf(acc[j + 1] + bias[c0 + j + 1], 0.f), fmaxf(acc[j + 2] + bias[c0 + j + 2], 0.f),
                 fmaxf(acc[j + 3] + bias[c0 + j + 3], 0.f)};
      Vec4<T>::store(out + c0 + j, o);
    }
  }
}

// conv1_1 dgrad: d crops (NCHW) = conv(dy [N][H][W][64], [9][64][3]) / scale, one thread per pixel, three accumulators
template <typename T>
__global__ __launch_bounds__(256) void k_conv_last(const T* __restrict__ dy, int N, int H, int W, const T* __restrict__ wgd, T* __restrict__ y) {
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (size_t)N * H * W) return;
  const int xx = (int)(pix % W), yy = (int)((pix / W) % H), img = (int)(pix / ((size_t)W * H));
  float acc[3] = {0.f, 0.f, 0.f};
  for (int t = 0; t < 9; ++t) {
    const int sy = yy + t / 3 - 1, sx = xx + t % 3 - 1;
    if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
    const T* src = dy + (((size_t)img * H + sy) * W + sx) * 64;
    const T* wt = wgd + t * 64 * 3;
    for (int c0 = 0; c0 < 64; c0 += 4) {
      const f32x4 a = Vec4<T>::load(src + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmaf(a[j], Cvt<T>::to_f(wt[(c0 + j) * 3 + c]), acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) y[(((size_t)img * 3 + c) * H + yy) * W + xx] = Cvt<T>::from_f(acc[c] / c_scale[c]);
}

// ---- max-pool ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_pool(const T* __restrict__ x, int N, int H, int W, int C, T* __restrict__ y) {
  const int Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)N * Ho * Wo * C;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const size_t pix = e / C;
    const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho), img = (int)(pix / ((size_t)Wo * Ho));
    const T* b = x + (((size_t)img * H + 2 * yo) * W + 2 * xo) * C + c;
    const float v0 = Cvt<T>::to_f(b[0]), v1 = Cvt<T>::to_f(b[C]), v2 = Cvt<T>::to_f(b[(size_t)W * C]), v3 = Cvt<T>::to_f(b[(size_t)W * C + C]);
    y[e] = Cvt<T>::from_f(fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)));
  }
}

// dx = (route(dpool) + add) * (h > 0) over h's [N][H][W][C]; dpool [N][H/2][W/2][C] or null (no pool), add fp32 or null
template <typename T>
__global__ __launch_bounds__(256) void k_route(const T* __restrict__ dpool, const float* __restrict__ add, const T* __restrict__ h, int N,
                                               int H, int W, int C, T* __restrict__ dx) {
  const size_t total = (size_t)N * H * W * C;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const float hv = Cvt<T>::to_f(h[e]);
    float g = 0.f;
    if (dpool) {
      const int c = (int)(e % C);
      const size_t pix = e / C;
      const int xx = (int)(pix % W), yy = (int)((pix / W) % H), img = (int)(pix / ((size_t)W * H));
      const int y0 = yy & ~1, x0 = xx & ~1;
      const T* b = h + (((size_t)img * H + y0) * W + x0) * C + c;
      const float v[4] = {Cvt<T>::to_f(b[0]), Cvt<T>::to_f(b[C]), Cvt<T>::to_f(b[(size_t)W * C]), Cvt<T>::to_f(b[(size_t)W * C + C])};
      int first = 0;                                  // first maximum in row-major order (strictly greater replaces)
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (v[k] > v[first]) first = k;
      if (first == (yy - y0) * 2 + (xx - x0)) g = Cvt<T>::to_f(dpool[(((size_t)img * (H / 2) + yy / 2) * (W / 2) + xx / 2) * C + c]);
    }
    if (add) g += add[e];
    dx[e] = Cvt<T>::from_f(hv > 0.f ? g : 0.f);
  }
}

// ---- LPIPS head ----------------------------------------------------------------------------------------------------------
constexpr int HD_PIX = 64;   // pixels per head block: 4 waves x 4 iterations x 4 pixels (one 16-lane row per pixel)

__device__ __forceinline__ float row16_sum(float v) {   // sum over the 16 lanes of a row, every lane gets it (fixed butterfly)
  v += wave_xor_dpp8(v);
  v += wave_xor_dpp4(v);
  v += wave_xor_dpp2(v);
  v += wave_xor_dpp1(v);
  return v;
}

// f: the tap's [2n][hw][C] features (images 0 .. n-1 reconstruction, n .. 2n-1 target).  part[img * blocks + blk] (double).
// A 16-lane row owns one pixel, lane j of the row channels j, j + 16, ... (C / 16 of them, C in 64 .. 512).
template <typename T>
__global__ __launch_bounds__(256) void k_head_fwd(const T* __restrict__ f, int n, int hw, int C, const float* __restrict__ lin,
                                                  double* __restrict__ part) {
  __shared__ float rsum[16];
  const int img = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane >> 4, j = lane & 15;
  const T* f0 = f + (size_t)img * hw * C;
  const T* f1 = f + (size_t)(n + img) * hw * C;
  const int cpl = C >> 4;
  float acc = 0.f;
  for (int i = 0; i < HD_PIX / 16; ++i) {
    const int p = blk * HD_PIX + wave * (HD_PIX / 4) + i * 4 + row;
    const bool ok = p < hw;
    float a[32], b[32], s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      a[k] = b[k] = 0.f;
      if (k < cpl && ok) {
        a[k] = Cvt<T>::to_f(f0[(size_t)p * C + j + 16 * k]);
        b[k] = Cvt<T>::to_f(f1[(size_t)p * C + j + 16 * k]);
        s0 = fmaf(a[k], a[k], s0);
        s1 = fmaf(b[k], b[k], s1);
      }
    }
    const float n0 = sqrtf(row16_sum(s0) + 1e-10f) + 1e-10f, n1 = sqrtf(row16_sum(s1) + 1e-10f) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      if (k < cpl) {
        const float u = a[k] / n0 - b[k] / n1;
        d = fmaf(lin[j + 16 * k], u * u, d);
      }
    }
    d = row16_sum(d);
    if (ok) acc += d;
  }
  if (j == 0) rsum[wave * 4 + row] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int r = 0; r < 16; ++r) t += rsum[r];
    part[(size_t)img * gridDim.x + blk] = t;
  }
}

// hg[img][p][c] = d lpips_img / d f0 * glp[img] (fp32, overwritten)
template <typename T>
__global__ __launch_bounds__(256) void k_head_bwd(const T* __restrict__ f, int n, int hw, int C, const float* __restrict__ lin,
                                                  const float* __restrict__ glp, float* __restrict__ hg) {
  const int img = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane >> 4, j = lane & 15;
  const T* f0 = f + (size_t)img * hw * C;
  const T* f1 = f + (size_t)(n + img) * hw * C;
  const float g = glp[img] / (float)hw;
  const int cpl = C >> 4;
  for (int i = 0; i < HD_PIX / 16; ++i) {
    const int p = blk * HD_PIX + wave * (HD_PIX / 4) + i * 4 + row;
    const bool ok = p < hw;
    float a[32], b[32], s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      a[k] = b[k] = 0.f;
      if (k < cpl && ok) {
        a[k] = Cvt<T>::to_f(f0[(size_t)p * C + j + 16 * k]);
        b[k] = Cvt<T>::to_f(f1[(size_t)p * C + j + 16 * k]);
        s0 = fmaf(a[k], a[k], s0);
        s1 = fmaf(b[k], b[k], s1);
      }
    }
    const float s = sqrtf(row16_sum(s0) + 1e-10f), n0 = s + 1e-10f, n1 = sqrtf(row16_sum(s1) + 1e-10f) + 1e-10f;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      if (k < cpl) {
        b[k] = 2.0f * lin[j + 16 * k] * (a[k] / n0 - b[k] / n1) * g;    // b now holds a_c of the backward formula
        dot = fmaf(b[k], a[k], dot);
      }
    }
    const float coef = row16_sum(dot) / (n0 * n0 * s);
#pragma unroll
    for (int k = 0; k < 32; ++k)
      if (k < cpl && ok) hg[((size_t)img * hw + p) * C + j + 16 * k] = b[k] / n0 - a[k] * coef;
  }
}

// ---- Gram term -------------------------------------------------------------------------------------------------------------
// D[img][i][j] = (sum_p f0[p][i] f0[p][j] - sum_p f1[p][i] f1[p][j]) / hw; gpart[img * blocks + blk] = sum over the block's D^2
template <typename T>
__global__ __launch_bounds__(256) void k_gram_diff(const T* __restrict__ f, int n, int hw, int C, float* __restrict__ D,
                                                   double* __restrict__ gpart) {
  __shared__ double red[256];
  const int img = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x, i = e / C, j = e % C;
  const T* f0 = f + (size_t)img * hw * C;
  const T* f1 = f + (size_t)(n + img) * hw * C;
  float g0 = 0.f, g1 = 0.f;
  for (int p = 0; p < hw; ++p) {
    g0 = fmaf(Cvt<T>::to_f(f0[(size_t)p * C + i]), Cvt<T>::to_f(f0[(size_t)p * C + j]), g0);
    g1 = fmaf(Cvt<T>::to_f(f1[(size_t)p * C + i]), Cvt<T>::to_f(f1[(size_t)p * C + j]), g1);
  }
  const float d = (g0 - g1) / (float)hw;
  if (D) D[(size_t)img * C * C + e] = d;
  red[threadIdx.x] = (double)d * d;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) gpart[(size_t)img * gridDim.x + blockIdx.x] = red[0];
}

template <typename T>
__global__ __launch_bounds__(256) void k_gram_bwd(const T* __restrict__ f, int hw, int C, const float* __restrict__ D,
                                                  const float* __restrict__ ggr, float* __restrict__ hg) {
  const int img = blockIdx.y;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)hw * C) return;
  const int p = (int)(e / C), i = (int)(e % C);
  const T* f0 = f + ((size_t)img * hw + p) * C;
  const float* Di = D + ((size_t)img * C + i) * C;
  float acc = 0.f;
  for (int j = 0; j < C; ++j) acc = fmaf(Cvt<T>::to_f(f0[j]), Di[j], acc);
  hg[(size_t)img * hw * C + e] += ggr[img] * (4.0f / (5.0f * (float)C * (float)C * (float)hw)) * acc;
}

// lpips[img] = sum over taps of (sum of the tap's partials) / hw;  gram[img] = mean over taps of (sum of partials) / C^2
__global__ void k_head_finish(const double* __restrict__ part, const double* __restrict__ gpart, int n, int hw0, float* __restrict__ lpips,
                              float* __restrict__ gram) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= n) return;
  double lp = 0.0, gr = 0.0;
  size_t off = 0, goff = 0;
  for (int k = 0; k < 5; ++k) {
    const int hw = hw0 >> (2 * k), blocks = (hw + HD_PIX - 1) / HD_PIX, C = k < 4 ? 64 << k : 512, gblocks = C * C / 256;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[off + (size_t)img * blocks + b];
    lp += s / hw;
    off += (size_t)n * blocks;
    if (gram) {
      double t = 0.0;
      for (int b = 0; b < gblocks; ++b) t += gpart[goff + (size_t)img * gblocks + b];
      gr += t / ((double)C * C);
      goff += (size_t)n * gblocks;
    }
  }
  lpips[img] = (float)lp;
  if (gram) gram[img] = (float)(gr / 5.0);
}

// ---- evaluation: per-frame LPIPS of whole frames (EvalMetrics 'lpips') ----------------------------------------------------------
// conv1_1 forward read in place from a clip pair [3][T][H][W] (channel stride T*H*W): frames t0 .. t0 + cnt - 1 of the reconstruction
// go to images img0 .. of the stack y, the same frames of the target to images F + img0 ..  (F = frames of the pass).  The
// reconstruction is clamped to [-1, 1] in T before the scaling when `clamp` (a NaN stays a NaN, as torch.clamp).  Per pixel the same
// arithmetic in the same order as k_conv_first.
template <typename T>
__global__ __launch_bounds__(256) void k_conv_first_clip(const T* __restrict__ rc, const T* __restrict__ tg, int Tn, int t0, int cnt, int img0,
                                                         int F, int H, int W, int clamp, const T* __restrict__ wg,
                                                         const float* __restrict__ bias, T* __restrict__ y) {
  const size_t hw = (size_t)H * W, pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= 2 * (size_t)cnt * hw) return;
  const int xx = (int)(pix % W), yy = (int)((pix / W) % H), fi = (int)(pix / hw) % cnt, side = (int)(pix / (hw * cnt));
  const T* src = (side ? tg : rc) + (size_t)(t0 + fi) * hw;
  const size_t cs = (size_t)Tn * hw;
  const bool cl = clamp && side == 0;
  float v[27];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int sy = yy + t / 3 - 1, sx = xx + t % 3 - 1;
    const bool in = sy >= 0 && sy < H && sx >= 0 && sx < W;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
      float p = in ? Cvt<T>::to_f(src[ci * cs + (size_t)sy * W + sx]) : 0.f;
      if (cl) p = p < -1.f ? -1.f : (p > 1.f ? 1.f : p);
      v[t * 3 + ci] = in ? round_to<T>((p - c_shift[ci]) / c_scale[ci]) : 0.f;
    }
  }
  T* out = y + (((size_t)side * F + img0 + fi) * hw + (size_t)yy * W + xx) * 64;
  for (int c0 = 0; c0 < 64; c0 += 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(v[k], Cvt<T>::to_f(wg[k * 64 + c0 + j]), acc[j]);
#pragma unroll
    for (int j = 0; j < 8; j += 4) {
      f32x4 o = {fmaxf(acc[j] + bias[c0 + j], 0.f), fmaxf(acc[j + 1] + bias[c0 + j + 1], 0.f), fmaxf(acc[j + 2] + bias[c0 + j + 2], 0.f),
                 fmaxf(acc[j + 3] + bias[c0 + j + 3], 0.f)};
      Vec4<T>::store(out + c0 + j, o);
    }
  }
}

constexpr int EV_MAX_FRAMES = 2048;   // frames of one pass (a stack of 4096 images, what check_shape allows the loss path)

// Each tap's true pixel count (H >> k) * (W >> k): hw0 >> 2k is wrong once a stage is odd (24 x 40: tap 4 has 1 x 2 = 2 pixels,
// 960 >> 8 = 3).
struct EvalTaps {
  int hw[5];
};

// value[f] = sum over taps of (sum of the tap's partials, block order) / hw_k for the F frames of a pass; one block.  `out`
// (or NULL) gets the values; `acc` (or NULL) gets acc[0] += value[f] for f = 0 .. F-1 in that order by one thread, acc[1] += F.
__global__ __launch_bounds__(256) void k_eval_finish(const double* __restrict__ part, EvalTaps tp, int F, float* __restrict__ out,
                                                     double* __restrict__ acc) {
  __shared__ float s_v[EV_MAX_FRAMES];
  for (int f = threadIdx.x; f < F; f += 256) {
    double lp = 0.0;
    size_t off = 0;
    for (int k = 0; k < 5; ++k) {
      const int blocks = (tp.hw[k] + HD_PIX - 1) / HD_PIX;
      double s = 0.0;
      for (int b = 0; b < blocks; ++b) s += part[off + (size_t)f * blocks + b];
      lp += s / tp.hw[k];
      off += (size_t)F * blocks;
    }
    s_v[f] = (float)lp;
    if (out) out[f] = (float)lp;
  }
  __syncthreads();
  if (threadIdx.x == 0 && acc) {
    double s = acc[0];
    for (int f = 0; f < F; ++f) s += (double)s_v[f];
    acc[0] = s;
    acc[1] += (double)F;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
unsigned grid_for(size_t total) {
  const size_t b = (total + 255) / 256;
  return (unsigned)(b < 65536 ? (b ? b : 1) : 65536);
}

bool use_mfma(int dtype, int Cin, int Cout) { return dtype == TTV_BF16 && Cin % CM_K == 0 && Cout % CM_TN == 0; }

int split_for(int N, int H, int W, int Cin, int Cout) {
  const int TW = cm_tw(W), TH = CM_TP / TW;
  const long long tiles = (long long)ttv_cdiv(N * H, TH) * ttv_cdiv(W, TW) * (Cout / CM_TN);
  int S = 1;
  while (tiles * S < 1024 && S * 2 <= Cin / CM_K && S < 8) S *= 2;
  return S;
}

int64_t conv_ws_bytes(int dtype, int N, int H, int W, int Cin, int Cout) {
  if (!use_mfma(dtype, Cin, Cout)) return 0;
  const int S = split_for(N, H, W, Cin, Cout);
  return S > 1 ? (int64_t)S * N * H * W * Cout * 4 : 0;
}

int conv_launch(int dtype, const void* x, int N, int H, int W, int Cin, int Cout, const void* w, const float* bias, int mode, const void* h,
                void* y, void* ws, hipStream_t st) {
  if (use_mfma(dtype, Cin, Cout)) {
    const int TW = cm_tw(W), TH = CM_TP / TW, TWl = __builtin_ctz(TW);
    const int S = split_for(N, H, W, Cin, Cout);
    dim3 grid((unsigned)(ttv_cdiv(N * H, TH) * ttv_cdiv(W, TW)), (unsigned)(Cout / CM_TN), (unsigned)S);
    float* part = S > 1 ? reinterpret_cast<float*>(ws) : nullptr;
    hipLaunchKernelGGL(k_conv_mfma, grid, dim3(256), 0, st, (const bf16_t*)x, H, N * H, W, Cin, Cout, (const bf16_t*)w, bias, mode,
                       (const bf16_t*)h, (bf16_t*)y, part, TWl);
    TTV_CHECK_LAUNCH("lpips conv (mfma)");
    if (S > 1) {
      const size_t total = (size_t)N * H * W * Cout;
      hipLaunchKernelGGL(k_conv_splitk<bf16_t>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, part, S, total, Cout, bias,
                         mode, (const bf16_t*)h, (bf16_t*)y);
      TTV_CHECK_LAUNCH("lpips conv (split-k sum)");
    }
    return TTV_OK;
  }
  const size_t total = (size_t)N * H * W * Cout;
  if (dtype == TTV_BF16)
    hipLaunchKernelGGL(k_conv_direct<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)x, N, H, W, Cin, Cout, (const bf16_t*)w,
                       bias, mode, (const bf16_t*)h, (bf16_t*)y);
  else
    hipLaunchKernelGGL(k_conv_direct<float>, dim3(grid_for(total)), dim3(256), 0, st, (const float*)x, N, H, W, Cin, Cout, (const float*)w, bias,
                       mode, (const float*)h, (float*)y);
  TTV_CHECK_LAUNCH("lpips conv (direct)");
  return TTV_OK;
}

int pool_launch(int dtype, const void* x, int N, int H, int W, int C, void* y, hipStream_t st) {
  const size_t total = (size_t)N * (H / 2) * (W / 2) * C;
  if (dtype == TTV_BF16) hipLaunchKernelGGL(k_pool<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)x, N, H, W, C, (bf16_t*)y);
  else hipLaunchKernelGGL(k_pool<float>, dim3(grid_for(total)), dim3(256), 0, st, (const float*)x, N, H, W, C, (float*)y);
  TTV_CHECK_LAUNCH("lpips max-pool");
  return TTV_OK;
}

int route_launch(int dtype, const void* dpool, const float* add, const void* h, int N, int H, int W, int C, void* dx, hipStream_t st) {
  const size_t total = (size_t)N * H * W * C;
  if (dtype == TTV_BF16)
    hipLaunchKernelGGL(k_route<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)dpool, add, (const bf16_t*)h, N, H, W, C,
                       (bf16_t*)dx);
  else
    hipLaunchKernelGGL(k_route<float>, dim3(grid_for(total)), dim3(256), 0, st, (const float*)dpool, add, (const float*)h, N, H, W, C,
                       (float*)dx);
  TTV_CHECK_LAUNCH("lpips max-pool backward");
  return TTV_OK;
}

// Byte offsets of one call's buffers.  Tape: act[l] = [2n][H_l][W_l][Cout_l] for the 13 conv outputs, pool[p] after layers 1, 3, 6, 9.
// Workspace: lpips partials, gram partials, head gradients (fp32, n images), Gram D (fp32, n images, when gram), two dgrad
// ping-pong buffers of n x H x W x 64 elements, one pooled-gradient buffer, and the largest split-K partial buffer.
struct Layout {
  size_t act[LP_LAYERS], pool[4], tape;
  size_t part, gpart, hg[5], D[5], bufa, bufb, bufp, split, ws;
};

Layout layout(int n, int H, int W, int dtype) {
  Layout L{};
  const size_t es = dtype_bytes(dtype);
  size_t o = 0;
  int pi = 0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    const int s = LP_STAGE[l];
    L.act[l] = o;
    o = align256(o + (size_t)2 * n * (H >> s) * (W >> s) * LP_COUT[l] * es);
    if (l == 1 || l == 3 || l == 6 || l == 9) {
      L.pool[pi++] = o;
      o = align256(o + (size_t)2 * n * (H >> (s + 1)) * (W >> (s + 1)) * LP_COUT[l] * es);
    }
  }
  L.tape = o;
  o = 0;
  size_t np = 0, ng = 0;
  for (int k = 0; k < 5; ++k) {
    const size_t hw = (size_t)(H >> k) * (W >> k);
    np += (size_t)n * ((hw + HD_PIX - 1) / HD_PIX);
    ng += (size_t)n * LP_TAP_C[k] * LP_TAP_C[k] / 256;
  }
  L.part = o;
  o = align256(o + np * 8);
  L.gpart = o;
  o = align256(o + ng * 8);
  for (int k = 0; k < 5; ++k) {
    L.hg[k] = o;
    o = align256(o + (size_t)n * (H >> k) * (W >> k) * LP_TAP_C[k] * 4);
  }
  for (int k = 0; k < 5; ++k) {
    L.D[k] = o;
    o = align256(o + (size_t)n * LP_TAP_C[k] * LP_TAP_C[k] * 4);
  }
  const size_t big = (size_t)n * H * W * 64 * es;
  L.bufa = o;
  o = align256(o + big);
  L.bufb = o;
  o = align256(o + big);
  L.bufp = o;
  o = align256(o + big / 4);
  int64_t sp = 0;
  for (int l = 1; l < LP_LAYERS; ++l) {
    const int s = LP_STAGE[l];
    sp = std::max(sp, conv_ws_bytes(dtype, 2 * n, H >> s, W >> s, LP_CIN[l], LP_COUT[l]));
    sp = std::max(sp, conv_ws_bytes(dtype, n, H >> s, W >> s, LP_COUT[l], LP_CIN[l]));
  }
  L.split = o;
  o = align256(o + (size_t)sp);
  L.ws = o;
  return L;
}

int check_shape(int n, int H, int W, int dtype) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "lpips: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(n >= 1 && n <= 4096, "lpips: n = %d images (1 .. 4096)", n);
  TTV_CHECK_ARG(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && H <= 2048 && W <= 2048,
                "lpips: %d x %d images; H and W must be multiples of 16 in 16 .. 2048", H, W);
  return TTV_OK;
}

int check_weights(const ttv_lpips_weights* w) {
  TTV_CHECK_ARG(w, "lpips: null weights");
  for (int l = 0; l < LP_LAYERS; ++l) TTV_CHECK_ARG(w->w[l] && w->wd[l] && w->b[l], "lpips: null weight image of layer %d", l);
  for (int k = 0; k < 5; ++k) TTV_CHECK_ARG(w->lin[k], "lpips: null lin%d weight", k);
  return TTV_OK;
}

// One evaluation pass of F frame pairs: two ping-pong activation buffers sized for the largest stage (2F images x H x W x 64), the
// head partials of the five taps, the largest split-K partial buffer.  No tape.
struct EvalLayout {
  size_t bufa, bufb, part, split, ws;
};

EvalLayout eval_layout(int F, int H, int W, int dtype) {
  EvalLayout L{};
  const size_t big = (size_t)2 * F * H * W * 64 * dtype_bytes(dtype);
  size_t o = 0, np = 0;
  L.bufa = o;
  o = align256(o + big);
  L.bufb = o;
  o = align256(o + big);
  for (int k = 0; k < 5; ++k) np += (size_t)F * (((size_t)(H >> k) * (W >> k) + HD_PIX - 1) / HD_PIX);
  L.part = o;
  o = align256(o + np * 8);
  int64_t sp = 0;
  for (int l = 1; l < LP_LAYERS; ++l) sp = std::max(sp, conv_ws_bytes(dtype, 2 * F, H >> LP_STAGE[l], W >> LP_STAGE[l], LP_CIN[l], LP_COUT[l]));
  L.split = o;
  o = align256(o + (size_t)sp);
  L.ws = o;
  return L;
}

int check_eval_shape(int H, int W, int dtype) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "lpips eval: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(H >= 16 && W >= 16 && H <= 2048 && W <= 2048, "lpips eval: %d x %d frames; H and W must lie in 16 .. 2048", H, W);
  return TTV_OK;
}

template <typename T>
int eval_pass(const ttv_lpips_weights* wt, void* const* recon, void* const* target, const int32_t* frames, int clip, int t, int F, int H,
              int W, int dtype, int clamp, float* out, double* acc, char* wp, const EvalLayout& L, hipStream_t st) {
  T* cur = reinterpret_cast<T*>(wp + L.bufa);
  T* other = reinterpret_cast<T*>(wp + L.bufb);
  for (int done = 0; done < F;) {   // conv1_1 from the clips: one launch per clip that has frames in this pass
    const int cnt = std::min(F - done, frames[clip] - t);
    const unsigned blocks = (unsigned)(((size_t)2 * cnt * H * W + 255) / 256);
    hipLaunchKernelGGL(k_conv_first_clip<T>, dim3(blocks), dim3(256), 0, st, (const T*)recon[clip], (const T*)target[clip], frames[clip], t,
                       cnt, done, F, H, W, clamp, (const T*)wt->w[0], wt->b[0], cur);
    TTV_CHECK_LAUNCH("lpips eval conv1_1");
    done += cnt;
    t += cnt;
    if (t == frames[clip]) ++clip, t = 0;
  }
  EvalTaps tp;
  size_t off = 0;
  int tap = 0;
  for (int l = 1; l < LP_LAYERS; ++l) {
    const int s = LP_STAGE[l], Hs = H >> s, Ws = W >> s, C = LP_COUT[l];
    TTV_TRY(conv_launch(dtype, cur, 2 * F, Hs, Ws, LP_CIN[l], C, wt->w[l], wt->b[l], MODE_FWD, nullptr, other, wp + L.split, st));
    std::swap(cur, other);
    if (l != LP_TAP_LAYER[tap]) continue;
    const int hw = Hs * Ws, blocks = ttv_cdiv(hw, HD_PIX);   // the tap's head, before its buffer is reused
    hipLaunchKernelGGL(k_head_fwd<T>, dim3(blocks, F), dim3(256), 0, st, (const T*)cur, F, hw, C, wt->lin[tap],
                       reinterpret_cast<double*>(wp + L.part) + off);
    TTV_CHECK_LAUNCH("lpips eval head");
    off += (size_t)F * blocks;
    tp.hw[tap++] = hw;
    if (tap < 5) {   // floor pool: (Hs >> 1) x (Ws >> 1), an odd stage loses its last row or column
      TTV_TRY(pool_launch(dtype, cur, 2 * F, Hs, Ws, C, other, st));
      std::swap(cur, other);
    }
  }
  hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(256), 0, st, (const double*)(wp + L.part), tp, F, out, acc);
  TTV_CHECK_LAUNCH("lpips eval finish");
  return TTV_OK;
}

}  // namespace

int64_t ttvk_lpips_tape_bytes(int n, int H, int W, int dtype) {
  if (check_shape(n, H, W, dtype) != TTV_OK) return -1;
  return (int64_t)layout(n, H, W, dtype).tape;
}

int64_t ttvk_lpips_workspace_bytes(int n, int H, int W, int dtype) {
  if (check_shape(n, H, W, dtype) != TTV_OK) return -1;
  return (int64_t)layout(n, H, W, dtype).ws;
}

int ttvk_lpips_forward(const ttv_lpips_weights* wt, const void* recon, const void* target, int n, int H, int W, int dtype, float* lpips,
                       float* gram, void* tape, void* ws, int64_t ws_bytes, hipStream_t st) {
  TTV_TRY(check_shape(n, H, W, dtype));
  TTV_TRY(check_weights(wt));
  const Layout L = layout(n, H, W, dtype);
  TTV_CHECK_ARG(recon && target && lpips && tape && ws, "lpips forward: null argument");
  TTV_CHECK_ARG((int64_t)L.ws <= ws_bytes, "lpips forward: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.ws);
  TTV_CHECK_ARG((((uintptr_t)tape | (uintptr_t)ws) & 255) == 0, "lpips forward: tape and workspace must be 256-byte aligned");
  char* tp = reinterpret_cast<char*>(tape);
  char* wp = reinterpret_cast<char*>(ws);
  const int N = 2 * n;
  {   // layer 0: straight from the NCHW crops
    const unsigned blocks = (unsigned)(((size_t)N * H * W + 255) / 256);
    if (dtype == TTV_BF16)
      hipLaunchKernelGGL(k_conv_first<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)recon, (const bf16_t*)target, n, N, H, W,
                         (const bf16_t*)wt->w[0], wt->b[0], (bf16_t*)(tp + L.act[0]));
    else
      hipLaunchKernelGGL(k_conv_first<float>, dim3(blocks), dim3(256), 0, st, (const float*)recon, (const float*)target, n, N, H, W,
                         (const float*)wt->w[0], wt->b[0], (float*)(tp + L.act[0]));
    TTV_CHECK_LAUNCH("lpips conv1_1");
  }
  const void* in = tp + L.act[0];
  int pi = 0;
  for (int l = 1; l < LP_LAYERS; ++l) {
    const int s = LP_STAGE[l];
    TTV_TRY(conv_launch(dtype, in, N, H >> s, W >> s, LP_CIN[l], LP_COUT[l], wt->w[l], wt->b[l], MODE_FWD, nullptr, tp + L.act[l],
                        wp + L.split, st));
    in = tp + L.act[l];
    if (l == 1 || l == 3 || l == 6 || l == 9) {
      TTV_TRY(pool_launch(dtype, in, N, H >> s, W >> s, LP_COUT[l], tp + L.pool[pi], st));
      in = tp + L.pool[pi++];
    }
  }
  size_t off = 0, goff = 0;
  for (int k = 0; k < 5; ++k) {
    const int hw = (H >> k) * (W >> k), C = LP_TAP_C[k], blocks = ttv_cdiv(hw, HD_PIX), gblocks = C * C / 256;
    const void* f = tp + L.act[LP_TAP_LAYER[k]];
    double* part = reinterpret_cast<double*>(wp + L.part) + off;
    if (dtype == TTV_BF16) hipLaunchKernelGGL(k_head_fwd<bf16_t>, dim3(blocks, n), dim3(256), 0, st, (const bf16_t*)f, n, hw, C, wt->lin[k], part);
    else hipLaunchKernelGGL(k_head_fwd<float>, dim3(blocks, n), dim3(256), 0, st, (const float*)f, n, hw, C, wt->lin[k], part);
    TTV_CHECK_LAUNCH("lpips head");
    off += (size_t)n * blocks;
    if (gram) {
      double* gp = reinterpret_cast<double*>(wp + L.gpart) + goff;
      if (dtype == TTV_BF16)
        hipLaunchKernelGGL(k_gram_diff<bf16_t>, dim3(gblocks, n), dim3(256), 0, st, (const bf16_t*)f, n, hw, C, (float*)nullptr, gp);
      else hipLaunchKernelGGL(k_gram_diff<float>, dim3(gblocks, n), dim3(256), 0, st, (const float*)f, n, hw, C, (float*)nullptr, gp);
      TTV_CHECK_LAUNCH("lpips gram");
      goff += (size_t)n * gblocks;
    }
  }
  hipLaunchKernelGGL(k_head_finish, dim3(ttv_cdiv(n, 256)), dim3(256), 0, st, (const double*)(wp + L.part), (const double*)(wp + L.gpart), n,
                     H * W, lpips, gram);
  TTV_CHECK_LAUNCH("lpips finish");
  return TTV_OK;
}

int ttvk_lpips_backward(const ttv_lpips_weights* wt, const void* tape, int n, int H, int W, int dtype, const float* glp, const float* ggr,
                        void* drecon, void* ws, int64_t ws_bytes, hipStream_t st) {
  TTV_TRY(check_shape(n, H, W, dtype));
  TTV_TRY(check_weights(wt));
  const Layout L = layout(n, H, W, dtype);
  TTV_CHECK_ARG(tape && glp && drecon && ws, "lpips backward: null argument");
  TTV_CHECK_ARG((int64_t)L.ws <= ws_bytes, "lpips backward: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.ws);
  TTV_CHECK_ARG((((uintptr_t)tape | (uintptr_t)ws) & 255) == 0, "lpips backward: tape and workspace must be 256-byte aligned");
  const char* tp = reinterpret_cast<const char*>(tape);
  char* wp = reinterpret_cast<char*>(ws);
  // head (and Gram) gradients of every tap, fp32, for the n reconstruction images (the first n of the tape's stack)
  for (int k = 0; k < 5; ++k) {
    const int hw = (H >> k) * (W >> k), C = LP_TAP_C[k], blocks = ttv_cdiv(hw, HD_PIX), gblocks = C * C / 256;
    const void* f = tp + L.act[LP_TAP_LAYER[k]];
    float* hg = reinterpret_cast<float*>(wp + L.hg[k]);
    if (dtype == TTV_BF16) hipLaunchKernelGGL(k_head_bwd<bf16_t>, dim3(blocks, n), dim3(256), 0, st, (const bf16_t*)f, n, hw, C, wt->lin[k], glp, hg);
    else hipLaunchKernelGGL(k_head_bwd<float>, dim3(blocks, n), dim3(256), 0, st, (const float*)f, n, hw, C, wt->lin[k], glp, hg);
    TTV_CHECK_LAUNCH("lpips head backward");
    if (ggr) {
      float* D = reinterpret_cast<float*>(wp + L.D[k]);
      double* gp = reinterpret_cast<double*>(wp + L.gpart);
      const unsigned eb = (unsigned)(((size_t)hw * C + 255) / 256);
      if (dtype == TTV_BF16) {
        hipLaunchKernelGGL(k_gram_diff<bf16_t>, dim3(gblocks, n), dim3(256), 0, st, (const bf16_t*)f, n, hw, C, D, gp);
        hipLaunchKernelGGL(k_gram_bwd<bf16_t>, dim3(eb, n), dim3(256), 0, st, (const bf16_t*)f, hw, C, (const float*)D, ggr, hg);
      } else {
        hipLaunchKernelGGL(k_gram_diff<float>, dim3(gblocks, n), dim3(256), 0, st, (const float*)f, n, hw, C, D, gp);
        hipLaunchKernelGGL(k_gram_bwd<float>, dim3(eb, n), dim3(256), 0, st, (const float*)f, hw, C, (const float*)D, ggr, hg);
      }
      TTV_CHECK_LAUNCH("lpips gram backward");
    }
  }
  // relu5_3: d pre-activation of layer 12 = head gradient * (h > 0)
  void* cur = wp + L.bufa;
  void* other = wp + L.bufb;
  TTV_TRY(route_launch(dtype, nullptr, reinterpret_cast<const float*>(wp + L.hg[4]), tp + L.act[12], n, H >> 4, W >> 4, 512, cur, st));
  int tap = 3;
  for (int l = 12; l >= 1; --l) {
    const int s = LP_STAGE[l], below = l - 1;
    const bool pooled = below == 1 || below == 3 || below == 6 || below == 9;
    if (pooled) {   // d(pool output), then route + head gradient + mask at the pool's input resolution
      TTV_TRY(conv_launch(dtype, cur, n, H >> s, W >> s, LP_COUT[l], LP_CIN[l], wt->wd[l], nullptr, MODE_RAW, nullptr, wp + L.bufp,
                          wp + L.split, st));
      TTV_TRY(route_launch(dtype, wp + L.bufp, reinterpret_cast<const float*>(wp + L.hg[tap]), tp + L.act[below], n, H >> (s - 1),
                           W >> (s - 1), LP_CIN[l], other, st));
      --tap;
    } else {
      TTV_TRY(conv_launch(dtype, cur, n, H >> s, W >> s, LP_COUT[l], LP_CIN[l], wt->wd[l], nullptr, MODE_MASK, tp + L.act[below], other,
                          wp + L.split, st));
    }
    std::swap(cur, other);
  }
  {   // layer 0: d crops (NCHW) = conv(d pre-activation, flipped W1) / scale
    const unsigned blocks = (unsigned)(((size_t)n * H * W + 255) / 256);
    if (dtype == TTV_BF16)
      hipLaunchKernelGGL(k_conv_last<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)cur, n, H, W, (const bf16_t*)wt->wd[0],
                         (bf16_t*)drecon);
    else
      hipLaunchKernelGGL(k_conv_last<float>, dim3(blocks), dim3(256), 0, st, (const float*)cur, n, H, W, (const float*)wt->wd[0], (float*)drecon);
    TTV_CHECK_LAUNCH("lpips conv1_1 dgrad");
  }
  return TTV_OK;
}

// ---- evaluation -------------------------------------------------------------------------------------------------------------------
int64_t ttvk_lpips_eval_workspace_bytes(int frames, int H, int W, int dtype) {
  if (check_eval_shape(H, W, dtype) != TTV_OK) return -1;
  if (frames < 1 || frames > EV_MAX_FRAMES) {
    ttv_set_error("lpips eval: %d frames in a pass (1 .. %d)", frames, EV_MAX_FRAMES);
    return -1;
  }
  return (int64_t)eval_layout(frames, H, W, dtype).ws;
}

int ttvk_lpips_eval_accumulate(const ttv_lpips_weights* wt, void* const* recon, void* const* target, const int32_t* frames, int n_clips, int H,
                               int W, int dtype, int clamp_recon, float* per_frame, double* acc, void* ws, int64_t ws_bytes, hipStream_t st) {
  TTV_TRY(check_eval_shape(H, W, dtype));
  TTV_TRY(check_weights(wt));
  TTV_CHECK_ARG(recon && target && frames && ws && (per_frame || acc), "lpips eval: null argument");
  TTV_CHECK_ARG(n_clips >= 1 && n_clips <= (1 << 20), "lpips eval: %d clips", n_clips);
  int64_t total = 0;
  for (int i = 0; i < n_clips; ++i) {
    TTV_CHECK_ARG(recon[i] && target[i], "lpips eval: null pointer in clip %d", i);
    TTV_CHECK_ARG(frames[i] >= 1 && frames[i] <= (1 << 20), "lpips eval: clip %d has %d frames", i, frames[i]);
    total += frames[i];
  }
  TTV_CHECK_ARG(total <= (1 << 24), "lpips eval: %lld frames in one call", (long long)total);
  TTV_CHECK_ARG(((uintptr_t)ws & 255) == 0, "lpips eval: the workspace must be 256-byte aligned");
  // the largest pass the workspace holds (split-K partials make the size not quite monotone in F: walk down)
  const int64_t per_frame_bytes = (int64_t)eval_layout(1, H, W, dtype).bufb * 2;
  int F = (int)std::min<int64_t>(std::min<int64_t>(total, EV_MAX_FRAMES), std::max<int64_t>(ws_bytes / per_frame_bytes, 1));
  const auto fits = [&](int64_t n) { return n == 0 || (int64_t)eval_layout((int)n, H, W, dtype).ws <= ws_bytes; };
  while (F > 1 && !(fits(F) && fits(total % F))) --F;   // the last, shorter pass must fit too
  TTV_CHECK_ARG(fits(F), "lpips eval: workspace of %lld bytes, one %d x %d frame needs %lld",
                (long long)ws_bytes, H, W, (long long)eval_layout(1, H, W, dtype).ws);
  char* wp = reinterpret_cast<char*>(ws);
  int clip = 0, t = 0;
  for (int64_t f0 = 0; f0 < total;) {
    const int n = (int)std::min<int64_t>(F, total - f0);
    const EvalLayout L = eval_layout(n, H, W, dtype);
    float* out = per_frame ? per_frame + f0 : nullptr;
    if (dtype == TTV_BF16) TTV_TRY(eval_pass<bf16_t>(wt, recon, target, frames, clip, t, n, H, W, dtype, clamp_recon, out, acc, wp, L, st));
    else TTV_TRY(eval_pass<float>(wt, recon, target, frames, clip, t, n, H, W, dtype, clamp_recon, out, acc, wp, L, st));
    f0 += n;
    for (int left = n; left > 0;) {   // advance (clip, t) by n frames
      const int cnt = std::min(left, frames[clip] - t);
      left -= cnt;
      t += cnt;
      if (t == frames[clip]) ++clip, t = 0;
    }
  }
  return TTV_OK;
}

// ---- single operations (tests) -----------------------------------------------------------------------------------------------
int64_t ttvk_lpips_conv_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype) { return conv_ws_bytes(dtype, N, H, W, Cin, Cout); }

int ttvk_lpips_conv3x3(const void* x, int N, int H, int W, int Cin, int Cout, const void* w, const float* bias, int mode, const void* h,
                       void* y, int dtype, void* ws, int64_t ws_bytes, hipStream_t st) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "lpips conv3x3: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && (int64_t)N * H <= (1 << 30), "lpips conv3x3: bad shape");
  TTV_CHECK_ARG(mode >= MODE_FWD && mode <= MODE_RAW, "lpips conv3x3: mode %d", mode);
  TTV_CHECK_ARG(x && w && y && (mode != MODE_FWD || bias) && (mode != MODE_MASK || h), "lpips conv3x3: null argument");
  const int64_t need = conv_ws_bytes(dtype, N, H, W, Cin, Cout);
  TTV_CHECK_ARG(ws_bytes >= need && (need == 0 || ws), "lpips conv3x3: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)need);
  if (use_mfma(dtype, Cin, Cout))
    TTV_CHECK_ARG((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)ws) & 15) == 0, "lpips conv3x3: buffers must be 16-byte aligned");
  return conv_launch(dtype, x, N, H, W, Cin, Cout, w, bias, mode, h, y, ws, st);
}

int ttvk_lpips_maxpool(const void* x, int N, int H, int W, int C, void* y, int dtype, hipStream_t st) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "lpips maxpool: dtype %d", dtype);
  TTV_CHECK_ARG(N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C >= 1 && x && y, "lpips maxpool: bad argument");
  return pool_launch(dtype, x, N, H, W, C, y, st);
}

int ttvk_lpips_maxpool_backward(const void* dy, const float* add, const void* h, int N, int H, int W, int C, void* dx, int dtype, hipStream_t st) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "lpips maxpool backward: dtype %d", dtype);
  TTV_CHECK_ARG(N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C >= 1 && h && dx, "lpips maxpool backward: bad argument");
  return route_launch(dtype, dy, add, h, N, H, W, C, dx, st);
}
