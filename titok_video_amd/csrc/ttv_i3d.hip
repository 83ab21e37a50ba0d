// FVD feature extractor (reference model/metrics/fvd.py FVDCalculator.update and its I3D detector): the clip preprocessing and the
// Inception-v1-inflated I3D network (Carreira & Zisserman 2017, Kinetics-400 RGB) up to the 400 logits before the softmax, averaged
// over time.  Everything fp32, activations channels-last (NDHWC: [clip][t][h][w][c]).
//
// Kernels
//   k_fvd_prep   : per clip [3][T][H][W] (bf16 or fp32, ragged, up to TTV_MAX_CLIPS_PER_LAUNCH per launch): optional clamp to
//                  [-1, 1], trilinear resample to 3 x 224 x 224 with torch's align_corners=False source rule
//                  (src = max((dst + 0.5) * in / out - 0.5, 0), upper neighbour clamped), frame 2 replicated into frames 3..9
//                  -> [n][10][224][224][3].  The time axis goes to 3 frames because the reference asks F.interpolate for
//                  size (C, 224, 224): see model/metrics/fvd.py.
//   k_i3d_conv   : 3-D convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain per output).
//                  Rows = output positions (clip, t, h, w), K = kT kH kW Cin in (tap, channel) order, columns = output channels.
//                  One workgroup (4 waves) owns 128 rows x 64 channels, a wave 32 rows x 64 channels (two 32 x 32 accumulators).
//                  Per 16-deep K chunk the 128 x 16 operand block (gathered from the input with the TF-SAME halo read as zero)
//                  and the 16 x 64 weight block are staged in LDS; the next chunk's global loads are issued into registers
//                  before the current chunk's MFMAs.  Epilogue: y = acc * scale + shift (folded BatchNorm), optional ReLU,
//                  stored to channels [c_off, c_off + Cout) of rows of ldc channels, so an Inception block's branches write
//                  their slices of the concatenated output directly.  No split-K: every output is one fixed-order chain, so
//                  a clip's result does not depend on the other clips of the launch.  Cin % 4 == 0 takes 16-byte operand
//                  loads; the stem (Cin = 3, K = 1029) takes the scalar loader of the same kernel, K padded to the chunk.
//   k_i3d_pool   : 3-D max-pool with TF-SAME padding, padded cells skipped (all inputs are post-ReLU, so this equals zero padding).
//   k_i3d_tail   : AvgPool 2x7x7 (VALID) -> logits (1x1x1 conv with bias, no BN / ReLU) -> mean over time (one step) -> [n][400].
#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

constexpr int PREP_T = 3, PREP_FRAMES = 10, PREP_S = 224;

struct FvdClips {
  const void* x[TTV_MAX_CLIPS_PER_LAUNCH];
  int T[TTV_MAX_CLIPS_PER_LAUNCH], H[TTV_MAX_CLIPS_PER_LAUNCH], W[TTV_MAX_CLIPS_PER_LAUNCH];
};

// torch upsample (align_corners=False, no scale factor): fp32 scale in / out, source index clamped at 0, upper neighbour clamped
__device__ __forceinline__ void lin_src(int dst, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)out;
  float src = fmaf(scale, (float)dst + 0.5f, -0.5f);   // one rounding, as torch's CPU kernel computes it
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

// one thread per output pixel (clip, t in 0..2, y, x) with its 3 channels; frames 3..9 copy frame 2
template <typename T>
__global__ __launch_bounds__(256) void k_fvd_prep(FvdClips a, int clamp, float* __restrict__ out) {
  const int clip = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= PREP_T * PREP_S * PREP_S) return;
  const int t = p / (PREP_S * PREP_S), yx = p - t * PREP_S * PREP_S, y = yx / PREP_S, x = yx - y * PREP_S;
  const int Ti = a.T[clip], Hi = a.H[clip], Wi = a.W[clip];
  const T* src = reinterpret_cast<const T*>(a.x[clip]);
  int t0, t1, y0, y1, x0, x1;
  float lt, ly, lx;
  lin_src(t, Ti, PREP_T, t0, t1, lt);
  lin_src(y, Hi, PREP_S, y0, y1, ly);
  lin_src(x, Wi, PREP_S, x0, x1, lx);
  const float mt = 1.f - lt, my = 1.f - ly, mx = 1.f - lx;
  const size_t plane = (size_t)Hi * Wi, chan = (size_t)Ti * plane;
  float v[3];
  for (int c = 0; c < 3; ++c) {
    const T* s = src + c * chan;
    auto g = [&](int tt, int yy, int xx) {
      float f = Cvt<T>::to_f(s[tt * plane + (size_t)yy * Wi + xx]);
      if (clamp) f = fminf(fmaxf(f, -1.f), 1.f);
      return f;
    };
    const float f0 = my * (mx * g(t0, y0, x0) + lx * g(t0, y0, x1)) + ly * (mx * g(t0, y1, x0) + lx * g(t0, y1, x1));
    const float f1 = my * (mx * g(t1, y0, x0) + lx * g(t1, y0, x1)) + ly * (mx * g(t1, y1, x0) + lx * g(t1, y1, x1));
    v[c] = mt * f0 + lt * f1;
  }
  float* o = out + (size_t)clip * PREP_FRAMES * PREP_S * PREP_S * 3;
  const size_t fr = (size_t)PREP_S * PREP_S * 3;
  for (int f = t; f < PREP_FRAMES; f += (t == 2 ? 1 : PREP_FRAMES)) {
    float* q = o + f * fr + (size_t)yx * 3;
    q[0] = v[0];
    q[1] = v[1];
    q[2] = v[2];
  }
}

// ---- convolution -----------------------------------------------------------------------------------------------------------
constexpr int CV_BM = 128, CV_BN = 64, CV_BK = 16, CV_AP = CV_BM + 4;

struct ConvArgs {
  const float* x;        // [N][Ti][Hi][Wi][Cin]
  const float* w;        // [K][Cout]
  const float* scale;    // [Cout]
  const float* shift;    // [Cout]
  float* y;              // [N][To][Ho][Wo][ldc], channels c_off ..
  int N, Ti, Hi, Wi, Cin, k, s, pt, ph, pw, To, Ho, Wo, Cout, ldc, c_off, relu, K, M;
};

// row m -> (clip, input corner); valid = m < M
__device__ __forceinline__ void row_origin(const ConvArgs& a, int m, int& base_n, int& t0, int& h0, int& w0) {
  if (m >= a.M) {
    base_n = -1;
    t0 = h0 = w0 = 0;
    return;
  }
  const int wo = m % a.Wo, r1 = m / a.Wo, ho = r1 % a.Ho, r2 = r1 / a.Ho, to = r2 % a.To, n = r2 / a.To;
  base_n = n;
  t0 = to * a.s - a.pt;
  h0 = ho * a.s - a.ph;
  w0 = wo * a.s - a.pw;
}

__device__ __forceinline__ bool tap_of(const ConvArgs& a, int k, int& ci, int& dt, int& dh, int& dw) {
  if (k >= a.K) return false;
  const int tap = k / a.Cin;
  ci = k - tap * a.Cin;
  const int kk = a.k * a.k;
  dt = tap / kk;
  const int r = tap - dt * kk;
  dh = r / a.k;
  dw = r - dh * a.k;
  return true;
}

__device__ __forceinline__ const float* in_ptr(const ConvArgs& a, int n, int t, int h, int w, int ci) {
  if (n < 0 || t < 0 || t >= a.Ti || h < 0 || h >= a.Hi || w < 0 || w >= a.Wi) return nullptr;
  return a.x + ((((size_t)n * a.Ti + t) * a.Hi + h) * a.Wi + w) * a.Cin + ci;
}

// VEC = 4: thread t stages k columns 4 (t & 3) .. +3 of rows (t >> 2) + 64 j, j < 2 (Cin % 4 == 0, so the 4 share a tap).
// VEC = 1: thread t stages k column t & 15 of rows (t >> 4) + 16 j, j < 8.
template <int VEC>
struct ALoader {
  static constexpr int R = VEC == 4 ? 2 : 8;
  int n[R], t0[R], h0[R], w0[R];
  float v[R * VEC];
  __device__ void init(const ConvArgs& a, int m0) {
    for (int j = 0; j < R; ++j) {
      const int m = VEC == 4 ? m0 + (int)(threadIdx.x >> 2) + 64 * j : m0 + (int)(threadIdx.x >> 4) + 16 * j;
      row_origin(a, m, n[j], t0[j], h0[j], w0[j]);
    }
  }
  __device__ void load(const ConvArgs& a, int k0) {
    const int k = VEC == 4 ? k0 + 4 * (int)(threadIdx.x & 3) : k0 + (int)(threadIdx.x & 15);
    int ci, dt, dh, dw;
    const bool ok = tap_of(a, k, ci, dt, dh, dw);
    for (int j = 0; j < R; ++j) {
      const float* p = ok ? in_ptr(a, n[j], t0[j] + dt, h0[j] + dh, w0[j] + dw, ci) : nullptr;
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
__global__ __launch_bounds__(256) void k_i3d_conv(ConvArgs a) {
  __shared__ float As[CV_BK * CV_AP];
  __shared__ float Bs[CV_BK * CV_BN];
  const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * CV_BN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  ALoader<VEC> al;
  al.init(a, m0);
  const int bk = threadIdx.x >> 4, bn = (threadIdx.x & 15) * 4;   // weight block: one float4 per thread
  f32x4 bv;
  auto load_b = [&](int k0) {
    const int k = k0 + bk, c = n0 + bn;
    bv = (k < a.K && c < a.Cout) ? *reinterpret_cast<const f32x4*>(a.w + (size_t)k * a.Cout + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  f32x16 acc0 = {}, acc1 = {};
  al.load(a, 0);
  load_b(0);
  const int nk = (a.K + CV_BK - 1) / CV_BK;
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();    // the previous chunk's MFMAs are done with the LDS blocks
    al.store(As);
    *reinterpret_cast<f32x4*>(Bs + bk * CV_BN + bn) = bv;
    __syncthreads();
    if (kc + 1 < nk) {
      al.load(a, (kc + 1) * CV_BK);
      load_b((kc + 1) * CV_BK);
    }
#pragma unroll
    for (int ks = 0; ks < CV_BK / 2; ++ks) {
      const int kr = 2 * ks + (lane >> 5);
      const float av = As[kr * CV_AP + 32 * wave + (lane & 31)];
      const float b0 = Bs[kr * CV_BN + (lane & 31)];
      const float b1 = Bs[kr * CV_BN + 32 + (lane & 31)];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
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

// ---- max-pool / tail -------------------------------------------------------------------------------------------------------
struct PoolArgs {
  const float* x;
  float* y;
  int N, Ti, Hi, Wi, C, kt, kh, kw, st, sh, sw, pt, ph, pw, To, Ho, Wo;
};

__global__ __launch_bounds__(256) void k_i3d_pool(PoolArgs a) {
  const size_t total = (size_t)a.N * a.To * a.Ho * a.Wo * a.C;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % a.C);
  size_t r = i / a.C;
  const int wo = (int)(r % a.Wo);
  r /= a.Wo;
  const int ho = (int)(r % a.Ho);
  r /= a.Ho;
  const int to = (int)(r % a.To);
  const int n = (int)(r / a.To);
  float best = -INFINITY;
  for (int dt = 0; dt < a.kt; ++dt) {
    const int t = to * a.st - a.pt + dt;
    if (t < 0 || t >= a.Ti) continue;
    for (int dh = 0; dh < a.kh; ++dh) {
      const int h = ho * a.sh - a.ph + dh;
      if (h < 0 || h >= a.Hi) continue;
      for (int dw = 0; dw < a.kw; ++dw) {
        const int w = wo * a.sw - a.pw + dw;
        if (w < 0 || w >= a.Wi) continue;
        best = fmaxf(best, a.x[((((size_t)n * a.Ti + t) * a.Hi + h) * a.Wi + w) * a.C + c]);
      }
    }
  }
  a.y[i] = best;
}

constexpr int TAIL_C = 1024, TAIL_P = 2 * 7 * 7, TAIL_OUT = 400;

// one workgroup per clip: channel means over the 98 positions (fixed order), then the 400 logits (fixed-order dot products)
__global__ __launch_bounds__(256) void k_i3d_tail(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                  float* __restrict__ out) {
  __shared__ float avg[TAIL_C];
  const int n = blockIdx.x;
  const float* xn = x + (size_t)n * TAIL_P * TAIL_C;
  for (int c = threadIdx.x; c < TAIL_C; c += 256) {
    float s = 0.f;
    for (int p = 0; p < TAIL_P; ++p) s += xn[(size_t)p * TAIL_C + c];
    avg[c] = s / (float)TAIL_P;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < TAIL_OUT; j += 256) {
    float s = 0.f;
    for (int c = 0; c < TAIL_C; ++c) s = fmaf(avg[c], w[(size_t)c * TAIL_OUT + j], s);
    out[(size_t)n * TAIL_OUT + j] = s + bias[j];   // logits of the single time step: the mean over time is the value itself
  }
}

// ---- network table ---------------------------------------------------------------------------------------------------------
// TF "SAME": out = ceil(n / s), pad = max((out - 1) s + k - n, 0), front pad / 2
inline int same_out(int n, int s) { return (n + s - 1) / s; }
inline int same_front(int n, int k, int s) {
  const int o = same_out(n, s), p = (o - 1) * s + k - n;
  return p > 0 ? p / 2 : 0;
}

// Inception channels (b0, b1a, b1b, b2a, b2b, b3b) of Mixed_3b .. Mixed_5c
constexpr int INC[9][6] = {{64, 96, 128, 16, 32, 32},     {128, 128, 192, 32, 96, 64},  {192, 96, 208, 16, 48, 64},
                           {160, 112, 224, 24, 64, 64},   {128, 128, 256, 24, 64, 64},  {112, 144, 288, 32, 64, 64},
                           {256, 160, 320, 32, 128, 128}, {256, 160, 320, 32, 128, 128}, {384, 192, 384, 48, 128, 128}};

// per-clip float counts of the workspace buffers (P, Q: the ping-pong activations; T1, T2, T3: Inception temporaries)
constexpr int64_t WS_PQ = (int64_t)5 * 112 * 112 * 64, WS_T = (int64_t)5 * 28 * 28 * 256;

int conv_launch(const float* x, int N, int Ti, int Hi, int Wi, int Cin, int k, int s, const float* w, const float* scale,
                const float* shift, int Cout, int relu, float* y, int ldc, int c_off, hipStream_t st) {
  ConvArgs a;
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.y = y;
  a.N = N; a.Ti = Ti; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.k = k; a.s = s;
  a.pt = same_front(Ti, k, s); a.ph = same_front(Hi, k, s); a.pw = same_front(Wi, k, s);
  a.To = same_out(Ti, s); a.Ho = same_out(Hi, s); a.Wo = same_out(Wi, s);
  a.Cout = Cout; a.ldc = ldc; a.c_off = c_off; a.relu = relu;
  a.K = k * k * k * Cin;
  const int64_t M = (int64_t)N * a.To * a.Ho * a.Wo;
  TTV_CHECK_ARG(M < ((int64_t)1 << 31) - CV_BM && M * ldc < ((int64_t)1 << 40), "i3d conv3d: %lld output rows is too many", (long long)M);
  a.M = (int)M;
  const dim3 grid((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)((Cout + CV_BN - 1) / CV_BN));
  if (Cin % 4 == 0) hipLaunchKernelGGL(k_i3d_conv<4>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_i3d_conv<1>, grid, dim3(256), 0, st, a);
  TTV_CHECK_LAUNCH("i3d conv3d");
  return TTV_OK;
}

int pool_launch(const float* x, int N, int Ti, int Hi, int Wi, int C, int kt, int kh, int kw, int st_, int sh, int sw, float* y,
                hipStream_t st) {
  PoolArgs a;
  a.x = x; a.y = y; a.N = N; a.Ti = Ti; a.Hi = Hi; a.Wi = Wi; a.C = C;
  a.kt = kt; a.kh = kh; a.kw = kw; a.st = st_; a.sh = sh; a.sw = sw;
  a.pt = same_front(Ti, kt, st_); a.ph = same_front(Hi, kh, sh); a.pw = same_front(Wi, kw, sw);
  a.To = same_out(Ti, st_); a.Ho = same_out(Hi, sh); a.Wo = same_out(Wi, sw);
  const int64_t total = (int64_t)N * a.To * a.Ho * a.Wo * C;
  hipLaunchKernelGGL(k_i3d_pool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  TTV_CHECK_LAUNCH("i3d maxpool3d");
  return TTV_OK;
}

int check_weights(const ttv_i3d_weights* w) {
  TTV_CHECK_ARG(w, "i3d: null weights");
  for (int i = 0; i < TTV_I3D_CONVS; ++i) {
    const bool logits = i == TTV_I3D_CONVS - 1;
    TTV_CHECK_ARG(w->w[i] && w->shift[i] && (logits || w->scale[i]), "i3d: weights of conv %d missing", i);
    TTV_CHECK_ARG(((uintptr_t)w->w[i] & 15) == 0, "i3d: weight image %d must be 16-byte aligned", i);
  }
  return TTV_OK;
}

}  // namespace

int64_t ttvk_i3d_workspace_bytes(int n) {
  if (n < 1 || n > TTV_MAX_CLIPS_PER_LAUNCH) {
    ttv_set_error("i3d: n = %d clips, 1 .. %d allowed", n, TTV_MAX_CLIPS_PER_LAUNCH);
    return -1;
  }
  return 2 * align256(WS_PQ * 4 * n) + 3 * align256(WS_T * 4 * n);
}

int ttvk_fvd_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, int clamp, float* out, hipStream_t st) {
  TTV_CHECK_ARG(n_clips >= 1 && n_clips <= TTV_MAX_CLIPS_PER_LAUNCH, "fvd preprocess: %d clips, 1 .. %d allowed", n_clips,
                TTV_MAX_CLIPS_PER_LAUNCH);
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "fvd preprocess: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(clips && dims && out, "fvd preprocess: null argument");
  FvdClips a;
  for (int i = 0; i < n_clips; ++i) {
    const int C = dims[4 * i], T = dims[4 * i + 1], H = dims[4 * i + 2], W = dims[4 * i + 3];
    TTV_CHECK_ARG(C == 3, "fvd preprocess: clip %d has %d channels, the detector takes 3", i, C);
    TTV_CHECK_ARG(T >= 1 && H >= 1 && W >= 1 && (int64_t)T * H * W * 3 < ((int64_t)1 << 31), "fvd preprocess: clip %d has shape 3 x %d x %d x %d", i, T,
                  H, W);
    TTV_CHECK_ARG(clips[i], "fvd preprocess: null clip %d", i);
    a.x[i] = clips[i];
    a.T[i] = T;
    a.H[i] = H;
    a.W[i] = W;
  }
  const dim3 grid((unsigned)((PREP_T * PREP_S * PREP_S + 255) / 256), (unsigned)n_clips);
  if (dtype == TTV_BF16) hipLaunchKernelGGL(k_fvd_prep<bf16_t>, grid, dim3(256), 0, st, a, clamp, out);
  else hipLaunchKernelGGL(k_fvd_prep<float>, grid, dim3(256), 0, st, a, clamp, out);
  TTV_CHECK_LAUNCH("fvd preprocess");
  return TTV_OK;
}

int ttvk_i3d_conv3d(const float* x, int N, int T, int H, int W, int Cin, int k, int stride, const float* w, const float* scale,
                    const float* shift, int Cout, int relu, float* y, int ldc, int c_off, hipStream_t st) {
  TTV_CHECK_ARG(x && w && y, "i3d conv3d: null argument");
  TTV_CHECK_ARG(N >= 1 && T >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "i3d conv3d: bad shape");
  TTV_CHECK_ARG(k == 1 || k == 3 || k == 7, "i3d conv3d: kernel size %d (1, 3 or 7)", k);
  TTV_CHECK_ARG(stride == 1 || stride == 2, "i3d conv3d: stride %d (1 or 2)", stride);
  TTV_CHECK_ARG(Cout % 4 == 0, "i3d conv3d: Cout = %d must be a multiple of 4", Cout);
  TTV_CHECK_ARG(c_off >= 0 && c_off + Cout <= ldc, "i3d conv3d: channels %d + %d do not fit rows of %d", c_off, Cout, ldc);
  TTV_CHECK_ARG((((uintptr_t)x | (uintptr_t)w) & 15) == 0, "i3d conv3d: x and w must be 16-byte aligned");
  return conv_launch(x, N, T, H, W, Cin, k, stride, w, scale, shift, Cout, relu, y, ldc, c_off, st);
}

int ttvk_i3d_maxpool3d(const float* x, int N, int T, int H, int W, int C, int kt, int kh, int kw, int st_, int sh, int sw, float* y,
                       hipStream_t st) {
  TTV_CHECK_ARG(x && y, "i3d maxpool3d: null argument");
  TTV_CHECK_ARG(N >= 1 && T >= 1 && H >= 1 && W >= 1 && C >= 1, "i3d maxpool3d: bad shape");
  TTV_CHECK_ARG(kt >= 1 && kh >= 1 && kw >= 1 && kt <= 7 && kh <= 7 && kw <= 7 && st_ >= 1 && sh >= 1 && sw >= 1 && st_ <= kt &&
                    sh <= kh && sw <= kw,
                "i3d maxpool3d: window %d x %d x %d, stride %d x %d x %d", kt, kh, kw, st_, sh, sw);
  return pool_launch(x, N, T, H, W, C, kt, kh, kw, st_, sh, sw, y, st);
}

int ttvk_i3d_features(const ttv_i3d_weights* wt, const float* x, int n, float* feats, void* ws, int64_t ws_bytes, hipStream_t st) {
  TTV_TRY(check_weights(wt));
  const int64_t need = ttvk_i3d_workspace_bytes(n);
  if (need < 0) return TTV_ERR_INVALID;
  TTV_CHECK_ARG(x && feats && ws, "i3d features: null argument");
  TTV_CHECK_ARG(need <= ws_bytes, "i3d features: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  TTV_CHECK_ARG((((uintptr_t)x | (uintptr_t)ws) & 255) == 0, "i3d features: x and workspace must be 256-byte aligned");
  char* wp = reinterpret_cast<char*>(ws);
  float* P = reinterpret_cast<float*>(wp);
  float* Q = reinterpret_cast<float*>(wp + align256(WS_PQ * 4 * n));
  float* T1 = reinterpret_cast<float*>(wp + 2 * align256(WS_PQ * 4 * n));
  float* T2 = reinterpret_cast<float*>(wp + 2 * align256(WS_PQ * 4 * n) + align256(WS_T * 4 * n));
  float* T3 = reinterpret_cast<float*>(wp + 2 * align256(WS_PQ * 4 * n) + 2 * align256(WS_T * 4 * n));
  auto conv = [&](int i, const float* in, int t, int h, int w, int cin, int k, int s, int cout, float* out, int ldc, int off) {
    return conv_launch(in, n, t, h, w, cin, k, s, wt->w[i], wt->scale[i], wt->shift[i], cout, 1, out, ldc, off, st);
  };
  TTV_TRY(conv(0, x, 10, 224, 224, 3, 7, 2, 64, P, 64, 0));              // Conv3d_1a_7x7 -> 5 x 112 x 112 x 64
  TTV_TRY(pool_launch(P, n, 5, 112, 112, 64, 1, 3, 3, 1, 2, 2, Q, st));  // MaxPool3d_2a_3x3 -> 5 x 56 x 56
  TTV_TRY(conv(1, Q, 5, 56, 56, 64, 1, 1, 64, P, 64, 0));                // Conv3d_2b_1x1
  TTV_TRY(conv(2, P, 5, 56, 56, 64, 3, 1, 192, Q, 192, 0));              // Conv3d_2c_3x3
  TTV_TRY(pool_launch(Q, n, 5, 56, 56, 192, 1, 3, 3, 1, 2, 2, P, st));   // MaxPool3d_3a_3x3 -> 5 x 28 x 28
  float* cur = P;
  float* nxt = Q;
  int t = 5, h = 28, c = 192;
  for (int b = 0; b < 9; ++b) {
    if (b == 2) {   // MaxPool3d_4a_3x3 -> 3 x 14 x 14
      TTV_TRY(pool_launch(cur, n, t, h, h, c, 3, 3, 3, 2, 2, 2, nxt, st));
      t = 3; h = 14;
      float* s = cur; cur = nxt; nxt = s;
    } else if (b == 7) {   // MaxPool3d_5a_2x2 -> 2 x 7 x 7
      TTV_TRY(pool_launch(cur, n, t, h, h, c, 2, 2, 2, 2, 2, 2, nxt, st));
      t = 2; h = 7;
      float* s = cur; cur = nxt; nxt = s;
    }
    const int* ch = INC[b];
    const int cout = ch[0] + ch[2] + ch[4] + ch[5], i0 = 3 + 6 * b;
    TTV_TRY(conv(i0 + 0, cur, t, h, h, c, 1, 1, ch[0], nxt, cout, 0));                         // b0
    TTV_TRY(conv(i0 + 1, cur, t, h, h, c, 1, 1, ch[1], T1, ch[1], 0));                         // b1a
    TTV_TRY(conv(i0 + 2, T1, t, h, h, ch[1], 3, 1, ch[2], nxt, cout, ch[0]));                  // b1b
    TTV_TRY(conv(i0 + 3, cur, t, h, h, c, 1, 1, ch[3], T2, ch[3], 0));                         // b2a
    TTV_TRY(conv(i0 + 4, T2, t, h, h, ch[3], 3, 1, ch[4], nxt, cout, ch[0] + ch[2]));          // b2b
    TTV_TRY(pool_launch(cur, n, t, h, h, c, 3, 3, 3, 1, 1, 1, T3, st));                        // b3a
    TTV_TRY(conv(i0 + 5, T3, t, h, h, c, 1, 1, ch[5], nxt, cout, ch[0] + ch[2] + ch[4]));      // b3b
    c = cout;
    float* s = cur; cur = nxt; nxt = s;
  }
  hipLaunchKernelGGL(k_i3d_tail, dim3((unsigned)n), dim3(256), 0, st, cur, wt->w[TTV_I3D_CONVS - 1], wt->shift[TTV_I3D_CONVS - 1], feats);
  TTV_CHECK_LAUNCH("i3d tail");
  return TTV_OK;
}
