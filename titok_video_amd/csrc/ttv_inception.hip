// Frame FID / IS / MMD feature extractor (reference model/metrics/metrics.py MetricCalculator and its InceptionV3 wrapper): the frame
// preprocessing and torchvision's Inception-v3 trunk (Szegedy et al. 2016) up to the 2048 pooled activations, the fc logits and their
// softmax.  Everything fp32, activations channels-last (NHWC: [image][h][w][c]).
//
// Kernels
//   k_inc_prep : per image [3][H][W] (bf16 or fp32, rows contiguous, a channel stride of its own so that a frame of a clip
//                [3][T][H][W] is an image in place; ragged, up to TTV_MAX_CLIPS_PER_LAUNCH per launch): optional clamp to [-1, 1],
//                bilinear resize to 299 x 299 with torch's align_corners=True source rule (scale = (in - 1) / (out - 1) in fp32,
//                src = scale * dst, upper neighbour clamped) -> [n][299][299][3].  No ImageNet normalisation: the reference's wrapper
//                calls torchvision's submodules one by one, so transform_input never runs.
//   k_inc_conv : 2-D convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain per output).
//                Rows = output positions (image, h, w), K = kh kw Cin in (tap, channel) order, columns = output channels; kernel
//                kh x kw, strides sh x sw and zero padding ph x pw are arguments (1x7, 7x1, 1x3, 3x1, 5x5, stride-2 VALID).
//                k_i3d_conv's tiling: one workgroup (4 waves) owns 128 rows x 64 channels, a wave 32 rows x 64 channels (two
//                32 x 32 accumulators); per 16-deep K chunk the 128 x 16 operand block (padded taps read as zero) and the 16 x 64
//                weight block are staged in LDS and the next chunk's global loads are issued before the current chunk's MFMAs.
//                Unlike k_i3d_conv the LDS blocks are double-buffered: the next chunk is stored into the other buffer behind the
//                MFMAs, so a chunk costs one workgroup barrier, not two (same sums in the same order).  Epilogue:
//                y = acc * scale + shift (folded BatchNorm), optional ReLU, stored to channels [c_off, c_off + Cout) of rows of
//                ldc channels, so a block's branches write their slices of the concatenation directly.  No split-K: every output
//                is one fixed-order chain, so an image's result does not depend on the other images of the launch.  Cin % 4 == 0
//                takes 16-byte operand loads; the stem (Cin = 3, K = 27) takes the scalar loader, K padded to the chunk.  The tail
//                tile of a Cout that is no multiple of 64 reads no weights and writes no channels outside the slice.
//   k_inc_pool : avg3 (3 x 3, stride 1, padding 1, padded cells counted: the sum of the cells inside in row-major tap order, divided by
//                9) and max3s2 (3 x 3, stride 2, VALID), both into a channel slice like the convolution.
//   k_inc_tail : mean over the 8 x 8 positions (fixed order) -> acts [n][2048]; fc with bias (fixed-order dot products) and the
//                softmax over the 1000 logits with max subtraction (fixed-order tree reductions) -> probs [n][1000] (optional).
#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

constexpr int PREP_S = TTV_INCEPTION_INPUT;

struct IncImages {
  const void* x[TTV_MAX_CLIPS_PER_LAUNCH];
  long long chan[TTV_MAX_CLIPS_PER_LAUNCH];   // elements between the channels of an image
  int H[TTV_MAX_CLIPS_PER_LAUNCH], W[TTV_MAX_CLIPS_PER_LAUNCH];
};

// torch upsample (align_corners=True): fp32 scale (in - 1) / (out - 1), src = scale * dst, upper neighbour clamped
__device__ __forceinline__ void lin_src_ac(int dst, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const float src = scale * (float)dst;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

// one thread per output pixel (image, y, x) with its 3 channels
template <typename T>
__global__ __launch_bounds__(256) void k_inc_prep(IncImages a, int clamp, float* __restrict__ out) {
  const int img = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= PREP_S * PREP_S) return;
  const int y = p / PREP_S, x = p - y * PREP_S;
  const int Hi = a.H[img], Wi = a.W[img];
  const T* src = reinterpret_cast<const T*>(a.x[img]);
  int y0, y1, x0, x1;
  float ly, lx;
  lin_src_ac(y, Hi, PREP_S, y0, y1, ly);
  lin_src_ac(x, Wi, PREP_S, x0, x1, lx);
  const float my = 1.f - ly, mx = 1.f - lx;
  float* q = out + ((size_t)img * PREP_S * PREP_S + p) * 3;
  for (int c = 0; c < 3; ++c) {
    const T* s = src + (size_t)c * a.chan[img];
    auto g = [&](int yy, int xx) {
      float f = Cvt<T>::to_f(s[(size_t)yy * Wi + xx]);
      if (clamp) f = fminf(fmaxf(f, -1.f), 1.f);
      return f;
    };
    q[c] = my * (mx * g(y0, x0) + lx * g(y0, x1)) + ly * (mx * g(y1, x0) + lx * g(y1, x1));
  }
}

// ---- convolution -----------------------------------------------------------------------------------------------------------
constexpr int CV_BM = 128, CV_BN = 64, CV_BK = 16, CV_AP = CV_BM + 4;

struct ConvArgs {
  const float* x;        // [N][Hi][Wi][Cin]
  const float* w;        // [K][Cout]
  const float* scale;    // [Cout]
  const float* shift;    // [Cout]
  float* y;              // [N][Ho][Wo][ldc], channels c_off ..
  int N, Hi, Wi, Cin, kh, kw, sh, sw, ph, pw, Ho, Wo, Cout, ldc, c_off, relu, K, M;
};

// row m -> (image, input corner); image -1 for m >= M
__device__ __forceinline__ void row_origin(const ConvArgs& a, int m, int& n, int& h0, int& w0) {
  if (m >= a.M) {
    n = -1;
    h0 = w0 = 0;
    return;
  }
  const int wo = m % a.Wo, r1 = m / a.Wo, ho = r1 % a.Ho;
  n = r1 / a.Ho;
  h0 = ho * a.sh - a.ph;
  w0 = wo * a.sw - a.pw;
}

__device__ __forceinline__ bool tap_of(const ConvArgs& a, int k, int& ci, int& dh, int& dw) {
  if (k >= a.K) return false;
  const int tap = k / a.Cin;
  ci = k - tap * a.Cin;
  dh = tap / a.kw;
  dw = tap - dh * a.kw;
  return true;
}

__device__ __forceinline__ const float* in_ptr(const ConvArgs& a, int n, int h, int w, int ci) {
  if (n < 0 || h < 0 || h >= a.Hi || w < 0 || w >= a.Wi) return nullptr;
  return a.x + (((size_t)n * a.Hi + h) * a.Wi + w) * a.Cin + ci;
}

// VEC = 4: thread t stages k columns 4 (t & 3) .. +3 of rows (t >> 2) + 64 j, j < 2 (Cin % 4 == 0, so the 4 share a tap).
// VEC = 1: thread t stages k column t & 15 of rows (t >> 4) + 16 j, j < 8.
template <int VEC>
struct ALoader {
  static constexpr int R = VEC == 4 ? 2 : 8;
  int n[R], h0[R], w0[R];
  float v[R * VEC];
  __device__ void init(const ConvArgs& a, int m0) {
    for (int j = 0; j < R; ++j) {
      const int m = VEC == 4 ? m0 + (int)(threadIdx.x >> 2) + 64 * j : m0 + (int)(threadIdx.x >> 4) + 16 * j;
      row_origin(a, m, n[j], h0[j], w0[j]);
    }
  }
  __device__ void load(const ConvArgs& a, int k0) {
    const int k = VEC == 4 ? k0 + 4 * (int)(threadIdx.x & 3) : k0 + (int)(threadIdx.x & 15);
    int ci = 0, dh = 0, dw = 0;
    const bool ok = tap_of(a, k, ci, dh, dw);
    for (int j = 0; j < R; ++j) {
      const float* p = ok ? in_ptr(a, n[j], h0[j] + dh, w0[j] + dw, ci) : nullptr;
      if (VEC == 4) {
        const f32x4 q = p ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int e = 0; e < 4; ++e) v[4 * j + e] = q[e];
      } else {
        v[j] = p ? *p : 0.f;
      }
    }
  }
  __device__ void store(float* As) const {
    for (int j = 0; j < R; ++j) {
      if (VEC == 4) {
        const int m = (int)(threadIdx.x >> 2) + 64 * j, kk = 4 * (int)(threadIdx.x & 3);
        for (int e = 0; e < 4; ++e) As[(kk + e) * CV_AP + m] = v[4 * j + e];
      } else {
        As[(int)(threadIdx.x & 15) * CV_AP + (int)(threadIdx.x >> 4) + 16 * j] = v[j];
      }
    }
  }
};

template <int VEC>
__global__ __launch_bounds__(256) void k_inc_conv(ConvArgs a) {
  __shared__ float As[2][CV_BK * CV_AP];
  __shared__ float Bs[2][CV_BK * CV_BN];
  const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * CV_BN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  ALoader<VEC> al;
  al.init(a, m0);
  const int bk = threadIdx.x >> 4, bn = (threadIdx.x & 15) * 4;   // weight block: one float4 per thread
  f32x4 bv;
  auto load_b = [&](int k0) {
    const int k = k0 + bk, c = n0 + bn;     // c and Cout are multiples of 4: a float4 lies wholly inside or outside the weights
    bv = (k < a.K && c < a.Cout) ? *reinterpret_cast<const f32x4*>(a.w + (size_t)k * a.Cout + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  f32x16 acc0 = {}, acc1 = {};
  al.load(a, 0);
  load_b(0);
  al.store(As[0]);
  *reinterpret_cast<f32x4*>(Bs[0] + bk * CV_BN + bn) = bv;
  const int nk = (a.K + CV_BK - 1) / CV_BK;
  for (int kc = 0; kc < nk; ++kc) {
    // chunk kc is in buffer kc & 1; everybody is done with the MFMAs of chunk kc - 1, whose buffer takes chunk kc + 1 below
    __syncthreads();
    const float* Ac = As[kc & 1];
    const float* Bc = Bs[kc & 1];
    const bool more = kc + 1 < nk;
    if (more) {
      al.load(a, (kc + 1) * CV_BK);
      load_b((kc + 1) * CV_BK);
    }
#pragma unroll
    for (int ks = 0; ks < CV_BK / 2; ++ks) {
      const int kr = 2 * ks + (lane >> 5);
      const float av = Ac[kr * CV_AP + 32 * wave + (lane & 31)];
      const float b0 = Bc[kr * CV_BN + (lane & 31)];
      const float b1 = Bc[kr * CV_BN + 32 + (lane & 31)];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
    if (more) {
      al.store(As[(kc + 1) & 1]);
      *reinterpret_cast<f32x4*>(Bs[(kc + 1) & 1] + bk * CV_BN + bn) = bv;
    }
  }
  // C/D map of the 32x32 f32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int c = n0 + 32 * half + (lane & 31);
    if (c >= a.Cout) continue;
    const float sc = a.scale ? a.scale[c] : 1.f, sh = a.shift ? a.shift[c] : 0.f;
    const f32x16& acc = half ? acc1 : acc0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m >= a.M) continue;
      float v = acc[r] * sc + sh;
      if (a.relu) v = fmaxf(v, 0.f);
      a.y[(size_t)m * a.ldc + a.c_off + c] = v;
    }
  }
}

// ---- pools / tail ----------------------------------------------------------------------------------------------------------
struct PoolArgs {
  const float* x;   // [N][Hi][Wi][C]
  float* y;         // [N][Ho][Wo][ldc], channels c_off ..
  int N, Hi, Wi, C, Ho, Wo, ldc, c_off;
};

template <int MODE>
__global__ __launch_bounds__(256) void k_inc_pool(PoolArgs a) {
  const size_t total = (size_t)a.N * a.Ho * a.Wo * a.C;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % a.C);
  size_t r = i / a.C;
  const int wo = (int)(r % a.Wo);
  r /= a.Wo;
  const int ho = (int)(r % a.Ho);
  const int n = (int)(r / a.Ho);
  const int s = MODE == TTV_INCEPTION_POOL_AVG3 ? 1 : 2, p = MODE == TTV_INCEPTION_POOL_AVG3 ? 1 : 0;
  float acc = MODE == TTV_INCEPTION_POOL_AVG3 ? 0.f : -INFINITY;
  for (int dh = 0; dh < 3; ++dh) {
    const int h = ho * s - p + dh;
    if (h < 0 || h >= a.Hi) continue;
    for (int dw = 0; dw < 3; ++dw) {
      const int w = wo * s - p + dw;
      if (w < 0 || w >= a.Wi) continue;
      const float v = a.x[(((size_t)n * a.Hi + h) * a.Wi + w) * a.C + c];
      acc = MODE == TTV_INCEPTION_POOL_AVG3 ? acc + v : fmaxf(acc, v);
    }
  }
  if (MODE == TTV_INCEPTION_POOL_AVG3) acc = acc / 9.f;   // padded cells count: always nine
  a.y[(((size_t)n * a.Ho + ho) * a.Wo + wo) * a.ldc + a.c_off + c] = acc;
}

constexpr int TAIL_C = TTV_INCEPTION_FEATURES, TAIL_P = 8 * 8, TAIL_OUT = TTV_INCEPTION_CLASSES, TAIL_T = 1024;

// fixed-order tree over the workgroup's 1024 values in LDS
template <bool MAX>
__device__ __forceinline__ float tail_reduce(float* red, float v) {
  __syncthreads();     // the previous result has been read
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = TAIL_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = MAX ? fmaxf(red[threadIdx.x], red[threadIdx.x + s]) : red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// one workgroup of 1024 threads per image: channel means over the 64 positions, one logit per thread, softmax
__global__ __launch_bounds__(TAIL_T) void k_inc_tail(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ acts, float* __restrict__ probs) {
  __shared__ float avg[TAIL_C];
  __shared__ float red[TAIL_T];
  const int n = blockIdx.x;
  const float* xn = x + (size_t)n * TAIL_P * TAIL_C;
  for (int c = threadIdx.x; c < TAIL_C; c += TAIL_T) {
    float s = 0.f;
    for (int p = 0; p < TAIL_P; ++p) s += xn[(size_t)p * TAIL_C + c];
    s = s / (float)TAIL_P;
    avg[c] = s;
    acts[(size_t)n * TAIL_C + c] = s;
  }
  if (!probs) return;
  __syncthreads();
  const int j = threadIdx.x;
  float logit = -INFINITY;
  if (j < TAIL_OUT) {
    float s = 0.f;
    for (int c = 0; c < TAIL_C; ++c) s = fmaf(avg[c], w[(size_t)c * TAIL_OUT + j], s);
    logit = s + bias[j];
  }
  const float mx = tail_reduce<true>(red, logit);
  const float e = j < TAIL_OUT ? expf(logit - mx) : 0.f;
  const float sum = tail_reduce<false>(red, e);
  if (j < TAIL_OUT) probs[(size_t)n * TAIL_OUT + j] = e / sum;
}

// ---- launches --------------------------------------------------------------------------------------------------------------
inline int conv_out(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }

int conv_launch(const float* x, int N, int Hi, int Wi, int Cin, int kh, int kw, int sh, int sw, int ph, int pw, const float* w,
                const float* scale, const float* shift, int Cout, int relu, float* y, int ldc, int c_off, hipStream_t st) {
  ConvArgs a;
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.y = y;
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw;
  a.Ho = conv_out(Hi, kh, sh, ph); a.Wo = conv_out(Wi, kw, sw, pw);
  a.Cout = Cout; a.ldc = ldc; a.c_off = c_off; a.relu = relu;
  a.K = kh * kw * Cin;
  const int64_t M = (int64_t)N * a.Ho * a.Wo;
  TTV_CHECK_ARG(M < ((int64_t)1 << 31) - CV_BM && M * ldc < ((int64_t)1 << 40), "inception conv2d: %lld output rows is too many", (long long)M);
  a.M = (int)M;
  const dim3 grid((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)((Cout + CV_BN - 1) / CV_BN));
  if (Cin % 4 == 0) hipLaunchKernelGGL(k_inc_conv<4>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_inc_conv<1>, grid, dim3(256), 0, st, a);
  TTV_CHECK_LAUNCH("inception conv2d");
  return TTV_OK;
}

int pool_launch(const float* x, int N, int Hi, int Wi, int C, int mode, float* y, int ldc, int c_off, hipStream_t st) {
  PoolArgs a;
  a.x = x; a.y = y; a.N = N; a.Hi = Hi; a.Wi = Wi; a.C = C; a.ldc = ldc; a.c_off = c_off;
  const bool avg = mode == TTV_INCEPTION_POOL_AVG3;
  a.Ho = avg ? Hi : conv_out(Hi, 3, 2, 0);
  a.Wo = avg ? Wi : conv_out(Wi, 3, 2, 0);
  const int64_t total = (int64_t)N * a.Ho * a.Wo * C;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (avg) hipLaunchKernelGGL(k_inc_pool<TTV_INCEPTION_POOL_AVG3>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_inc_pool<TTV_INCEPTION_POOL_MAX3S2>, grid, dim3(256), 0, st, a);
  TTV_CHECK_LAUNCH("inception pool2d");
  return TTV_OK;
}

int check_weights(const ttv_inception_weights* w, bool want_fc) {
  TTV_CHECK_ARG(w, "inception: null weights");
  for (int i = 0; i < TTV_INCEPTION_UNITS; ++i) {
    TTV_CHECK_ARG(w->unit[i].w && w->unit[i].scale && w->unit[i].shift, "inception: weights of unit %d missing", i);
    TTV_CHECK_ARG(((uintptr_t)w->unit[i].w & 15) == 0, "inception: weight image %d must be 16-byte aligned", i);
  }
  TTV_CHECK_ARG(!want_fc || (w->fc_w && w->fc_b), "inception: fc weights missing");
  return TTV_OK;
}

// per-image float counts of the workspace buffers (P, Q: the ping-pong activations, largest 147 x 147 x 64; T1, T2: branch
// temporaries, largest 35 x 35 x 96; T3: the pooled input of a block's pool branch, largest 35 x 35 x 288)
constexpr int64_t WS_PQ = (int64_t)147 * 147 * 64, WS_T = (int64_t)35 * 35 * 96, WS_T3 = (int64_t)35 * 35 * 288;

}  // namespace

int64_t ttvk_inception_workspace_bytes(int n) {
  if (n < 1 || n > TTV_MAX_CLIPS_PER_LAUNCH) {
    ttv_set_error("inception: n = %d images, 1 .. %d allowed", n, TTV_MAX_CLIPS_PER_LAUNCH);
    return -1;
  }
  return 2 * align256(WS_PQ * 4 * n) + 2 * align256(WS_T * 4 * n) + align256(WS_T3 * 4 * n);
}

int ttvk_inception_preprocess(void* const* images, const int64_t* dims, int n, int dtype, int clamp, float* out, hipStream_t st) {
  TTV_CHECK_ARG(n >= 1 && n <= TTV_MAX_CLIPS_PER_LAUNCH, "inception preprocess: %d images, 1 .. %d allowed", n, TTV_MAX_CLIPS_PER_LAUNCH);
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "inception preprocess: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(images && dims && out, "inception preprocess: null argument");
  IncImages a;
  for (int i = 0; i < n; ++i) {
    const int64_t H = dims[3 * i], W = dims[3 * i + 1], chan = dims[3 * i + 2];
    TTV_CHECK_ARG(H >= 1 && W >= 1 && H * W < ((int64_t)1 << 31), "inception preprocess: image %d has shape 3 x %lld x %lld", i, (long long)H,
                  (long long)W);
    TTV_CHECK_ARG(chan >= H * W, "inception preprocess: image %d has a channel stride of %lld elements, below its %lld pixels", i,
                  (long long)chan, (long long)(H * W));
    TTV_CHECK_ARG(images[i], "inception preprocess: null image %d", i);
    a.x[i] = images[i];
    a.chan[i] = chan;
    a.H[i] = (int)H;
    a.W[i] = (int)W;
  }
  const dim3 grid((unsigned)((PREP_S * PREP_S + 255) / 256), (unsigned)n);
  if (dtype == TTV_BF16) hipLaunchKernelGGL(k_inc_prep<bf16_t>, grid, dim3(256), 0, st, a, clamp, out);
  else hipLaunchKernelGGL(k_inc_prep<float>, grid, dim3(256), 0, st, a, clamp, out);
  TTV_CHECK_LAUNCH("inception preprocess");
  return TTV_OK;
}

int ttvk_inception_conv2d(const float* x, int N, int H, int W, int Cin, int kh, int kw, int sh, int sw, int ph, int pw, const float* w,
                          const float* scale, const float* shift, int Cout, int relu, float* y, int ldc, int c_off, hipStream_t st) {
  TTV_CHECK_ARG(x && w && y, "inception conv2d: null argument");
  TTV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "inception conv2d: bad shape");
  TTV_CHECK_ARG(kh >= 1 && kw >= 1 && kh <= 7 && kw <= 7, "inception conv2d: kernel %d x %d (1 .. 7 each)", kh, kw);
  TTV_CHECK_ARG((sh == 1 || sh == 2) && (sw == 1 || sw == 2), "inception conv2d: stride %d x %d (1 or 2 each)", sh, sw);
  TTV_CHECK_ARG(ph >= 0 && pw >= 0 && ph < kh && pw < kw, "inception conv2d: padding %d x %d for a %d x %d kernel", ph, pw, kh, kw);
  TTV_CHECK_ARG(H + 2 * ph >= kh && W + 2 * pw >= kw, "inception conv2d: a %d x %d kernel does not fit %d x %d with padding %d x %d", kh, kw, H,
                W, ph, pw);
  TTV_CHECK_ARG(Cout % 4 == 0, "inception conv2d: Cout = %d must be a multiple of 4", Cout);
  TTV_CHECK_ARG(c_off >= 0 && c_off + Cout <= ldc, "inception conv2d: channels %d + %d do not fit rows of %d", c_off, Cout, ldc);
  TTV_CHECK_ARG((((uintptr_t)x | (uintptr_t)w) & 15) == 0, "inception conv2d: x and w must be 16-byte aligned");
  return conv_launch(x, N, H, W, Cin, kh, kw, sh, sw, ph, pw, w, scale, shift, Cout, relu, y, ldc, c_off, st);
}

int ttvk_inception_pool2d(const float* x, int N, int H, int W, int C, int mode, float* y, int ldc, int c_off, hipStream_t st) {
  TTV_CHECK_ARG(x && y, "inception pool2d: null argument");
  TTV_CHECK_ARG(mode == TTV_INCEPTION_POOL_AVG3 || mode == TTV_INCEPTION_POOL_MAX3S2, "inception pool2d: mode %d", mode);
  TTV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1, "inception pool2d: bad shape");
  TTV_CHECK_ARG(mode == TTV_INCEPTION_POOL_AVG3 || (H >= 3 && W >= 3), "inception pool2d: a 3 x 3 VALID window does not fit %d x %d", H, W);
  TTV_CHECK_ARG(c_off >= 0 && c_off + C <= ldc, "inception pool2d: channels %d + %d do not fit rows of %d", c_off, C, ldc);
  return pool_launch(x, N, H, W, C, mode, y, ldc, c_off, st);
}

int ttvk_inception_features(const ttv_inception_weights* wt, const float* x, int n, float* acts, float* probs, void* ws, int64_t ws_bytes,
                            hipStream_t st) {
  TTV_TRY(check_weights(wt, probs != nullptr));
  const int64_t need = ttvk_inception_workspace_bytes(n);
  if (need < 0) return TTV_ERR_INVALID;
  TTV_CHECK_ARG(x && acts && ws, "inception features: null argument");
  TTV_CHECK_ARG(need <= ws_bytes, "inception features: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  TTV_CHECK_ARG((((uintptr_t)x | (uintptr_t)ws) & 255) == 0, "inception features: x and workspace must be 256-byte aligned");
  char* wp = reinterpret_cast<char*>(ws);
  const int64_t pq = align256(WS_PQ * 4 * n), tb = align256(WS_T * 4 * n);
  float* cur = reinterpret_cast<float*>(wp);
  float* nxt = reinterpret_cast<float*>(wp + pq);
  float* T1 = reinterpret_cast<float*>(wp + 2 * pq);
  float* T2 = reinterpret_cast<float*>(wp + 2 * pq + tb);
  float* T3 = reinterpret_cast<float*>(wp + 2 * pq + 2 * tb);
  int u = 0;          // the next unit of the weight table: the calls below come in the table's order
  int h = TTV_INCEPTION_INPUT, c = 3;
  // unit u: in [n][h][h][cin] -> channels [off, off + cout) of out [n][ho][ho][ldc]
  auto conv = [&](const float* in, int cin, int kh, int kw, int s, int ph, int pw, int cout, float* out, int ldc, int off) {
    const ttv_inception_unit& q = wt->unit[u++];
    return conv_launch(in, n, h, h, cin, kh, kw, s, s, ph, pw, q.w, q.scale, q.shift, cout, 1, out, ldc, off, st);
  };
  auto swap = [&]() { float* s = cur; cur = nxt; nxt = s; };
  // stem
  TTV_TRY(conv(x, 3, 3, 3, 2, 0, 0, 32, cur, 32, 0));        // Conv2d_1a_3x3 -> 149
  h = 149;
  TTV_TRY(conv(cur, 32, 3, 3, 1, 0, 0, 32, nxt, 32, 0));     // Conv2d_2a_3x3 -> 147
  h = 147;
  TTV_TRY(conv(nxt, 32, 3, 3, 1, 1, 1, 64, cur, 64, 0));     // Conv2d_2b_3x3
  TTV_TRY(pool_launch(cur, n, h, h, 64, TTV_INCEPTION_POOL_MAX3S2, nxt, 64, 0, st));   // -> 73
  h = 73;
  TTV_TRY(conv(nxt, 64, 1, 1, 1, 0, 0, 80, cur, 80, 0));     // Conv2d_3b_1x1
  TTV_TRY(conv(cur, 80, 3, 3, 1, 0, 0, 192, nxt, 192, 0));   // Conv2d_4a_3x3 -> 71
  h = 71;
  TTV_TRY(pool_launch(nxt, n, h, h, 192, TTV_INCEPTION_POOL_MAX3S2, cur, 192, 0, st));  // -> 35
  h = 35;
  c = 192;
  // InceptionA: Mixed_5b, 5c, 5d -> [1x1 64 | 5x5 64 | 3x3dbl 96 | pool pf]
  for (int pf : {32, 64, 64}) {
    const int ld = 224 + pf;
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 64, nxt, ld, 0));          // branch1x1
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 48, T1, 48, 0));           // branch5x5_1
    TTV_TRY(conv(T1, 48, 5, 5, 1, 2, 2, 64, nxt, ld, 64));         // branch5x5_2
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 64, T1, 64, 0));           // branch3x3dbl_1
    TTV_TRY(conv(T1, 64, 3, 3, 1, 1, 1, 96, T2, 96, 0));           // branch3x3dbl_2
    TTV_TRY(conv(T2, 96, 3, 3, 1, 1, 1, 96, nxt, ld, 128));        // branch3x3dbl_3
    TTV_TRY(pool_launch(cur, n, h, h, c, TTV_INCEPTION_POOL_AVG3, T3, c, 0, st));
    TTV_TRY(conv(T3, c, 1, 1, 1, 0, 0, pf, nxt, ld, 224));         // branch_pool
    c = ld;
    swap();
  }
  // InceptionB: Mixed_6a -> 17 x 17 x [3x3 384 | 3x3dbl 96 | pool 288]
  TTV_TRY(conv(cur, c, 3, 3, 2, 0, 0, 384, nxt, 768, 0));          // branch3x3
  TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 64, T1, 64, 0));             // branch3x3dbl_1
  TTV_TRY(conv(T1, 64, 3, 3, 1, 1, 1, 96, T2, 96, 0));             // branch3x3dbl_2
  TTV_TRY(conv(T2, 96, 3, 3, 2, 0, 0, 96, nxt, 768, 384));         // branch3x3dbl_3
  TTV_TRY(pool_launch(cur, n, h, h, c, TTV_INCEPTION_POOL_MAX3S2, nxt, 768, 480, st));
  h = 17;
  c = 768;
  swap();
  // InceptionC: Mixed_6b .. 6e -> [1x1 192 | 7x7 192 | 7x7dbl 192 | pool 192]
  for (int c7 : {128, 160, 160, 192}) {
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 192, nxt, 768, 0));        // branch1x1
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, c7, T1, c7, 0));           // branch7x7_1
    TTV_TRY(conv(T1, c7, 1, 7, 1, 0, 3, c7, T2, c7, 0));           // branch7x7_2 (1, 7)
    TTV_TRY(conv(T2, c7, 7, 1, 1, 3, 0, 192, nxt, 768, 192));      // branch7x7_3 (7, 1)
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, c7, T1, c7, 0));           // branch7x7dbl_1
    TTV_TRY(conv(T1, c7, 7, 1, 1, 3, 0, c7, T2, c7, 0));           // branch7x7dbl_2 (7, 1)
    TTV_TRY(conv(T2, c7, 1, 7, 1, 0, 3, c7, T1, c7, 0));           // branch7x7dbl_3 (1, 7)
    TTV_TRY(conv(T1, c7, 7, 1, 1, 3, 0, c7, T2, c7, 0));           // branch7x7dbl_4 (7, 1)
    TTV_TRY(conv(T2, c7, 1, 7, 1, 0, 3, 192, nxt, 768, 384));      // branch7x7dbl_5 (1, 7)
    TTV_TRY(pool_launch(cur, n, h, h, c, TTV_INCEPTION_POOL_AVG3, T3, c, 0, st));
    TTV_TRY(conv(T3, c, 1, 1, 1, 0, 0, 192, nxt, 768, 576));       // branch_pool
    swap();
  }
  // InceptionD: Mixed_7a -> 8 x 8 x [3x3 320 | 7x7x3 192 | pool 768]
  TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 192, T1, 192, 0));           // branch3x3_1
  TTV_TRY(conv(T1, 192, 3, 3, 2, 0, 0, 320, nxt, 1280, 0));        // branch3x3_2
  TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 192, T1, 192, 0));           // branch7x7x3_1
  TTV_TRY(conv(T1, 192, 1, 7, 1, 0, 3, 192, T2, 192, 0));          // branch7x7x3_2 (1, 7)
  TTV_TRY(conv(T2, 192, 7, 1, 1, 3, 0, 192, T1, 192, 0));          // branch7x7x3_3 (7, 1)
  TTV_TRY(conv(T1, 192, 3, 3, 2, 0, 0, 192, nxt, 1280, 320));      // branch7x7x3_4
  TTV_TRY(pool_launch(cur, n, h, h, c, TTV_INCEPTION_POOL_MAX3S2, nxt, 1280, 512, st));
  h = 8;
  c = 1280;
  swap();
  // InceptionE: Mixed_7b, 7c -> [1x1 320 | 3x3 384 + 384 | 3x3dbl 384 + 384 | pool 192]
  for (int b = 0; b < 2; ++b) {
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 320, nxt, 2048, 0));       // branch1x1
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 384, T1, 384, 0));         // branch3x3_1
    TTV_TRY(conv(T1, 384, 1, 3, 1, 0, 1, 384, nxt, 2048, 320));    // branch3x3_2a (1, 3)
    TTV_TRY(conv(T1, 384, 3, 1, 1, 1, 0, 384, nxt, 2048, 704));    // branch3x3_2b (3, 1)
    TTV_TRY(conv(cur, c, 1, 1, 1, 0, 0, 448, T1, 448, 0));         // branch3x3dbl_1
    TTV_TRY(conv(T1, 448, 3, 3, 1, 1, 1, 384, T2, 384, 0));        // branch3x3dbl_2
    TTV_TRY(conv(T2, 384, 1, 3, 1, 0, 1, 384, nxt, 2048, 1088));   // branch3x3dbl_3a (1, 3)
    TTV_TRY(conv(T2, 384, 3, 1, 1, 1, 0, 384, nxt, 2048, 1472));   // branch3x3dbl_3b (3, 1)
    TTV_TRY(pool_launch(cur, n, h, h, c, TTV_INCEPTION_POOL_AVG3, T3, c, 0, st));
    TTV_TRY(conv(T3, c, 1, 1, 1, 0, 0, 192, nxt, 2048, 1856));     // branch_pool
    c = 2048;
    swap();
  }
  // u == TTV_INCEPTION_UNITS here: 5 + 3 * 7 + 4 + 4 * 10 + 6 + 2 * 9 = 94
  hipLaunchKernelGGL(k_inc_tail, dim3((unsigned)n), dim3(TAIL_T), 0, st, cur, wt->fc_w, wt->fc_b, acts, probs);
  TTV_CHECK_LAUNCH("inception tail");
  return TTV_OK;
}
