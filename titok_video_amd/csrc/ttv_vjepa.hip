// JEDi feature extractor (reference model/metrics/jedi.py JEDiMetric.get_feats): the clip preprocessing and the V-JEPA ViT-L/16
// encoder (24 pre-norm blocks, width 1024, 16 heads of 64, patch 16, tubelet 2, 16 frames at 224^2 = 1568 tokens) with the SSv2
// attentive probe's pooler on top.  Precision is that of the reference's validation step under bf16 autocast: linear and attention
// operands bf16, fp32 accumulation, softmax and LayerNorm statistics, an fp32 residual stream, fp32 features.
//
// Kernels
//   k_jedi_prep    : ragged square clips [3][T][S][S] (bf16 / fp32, T <= 16) -> tubelet patch rows [n * 1568][1536] bf16 in the
//                    (c, kt, kh, kw) order of the flattened Conv3d weight: clamp to [-1, 1], (v + 1) / 2, bicubic to 224^2 (torch's
//                    F.interpolate, align_corners=False, A = -0.75, border-clamped taps, no clamp of the result), ImageNet
//                    normalisation, the last frame repeated up to frame 16.  One thread per 8 consecutive kw of one patch row; all
//                    fp32, one rounding to bf16 at the end (what autocast does to the conv's input).
//   k_ln           : LayerNorm of fp32 rows of width 1024 (one wave per row, two-pass statistics in registers), optionally followed
//                    by a second LayerNorm of the fp32 result (the encoder's final norm + the pooler's norm1: one read, two norms).
//                    bf16 and / or fp32 output.
//   k_attn_table   : the work table of ttvk_attention for n sequences of 1568 rows x 16 heads (full 128-row items, the eight XCD
//                    lists each holding whole (sequence, head) groups).
//   k_pool_attn    : the pooler's cross-attention: one query row per (clip, head) against the clip's 1568 keys; one workgroup per
//                    (head, clip), fixed-order reductions.
//   k_mean_rows    : finetuned=False: the mean of the final norm's fp32 output over a clip's 1568 tokens, a fixed-order sum.
// The linears run on the general bf16 GEMM (ttv_gemm.hip) with the epilogues EPI_BIAS_PLAIN / EPI_BIAS_GELU / EPI_BIAS_RESID_F32R,
// the encoder's attention on ttvk_attention (no gate, q_heads == kv_heads, the qkv projection written as q | unused | k | v).  Nothing
// sums across clips: a clip's features are bit-identical whatever else is in its launch.
#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

constexpr int VJ_S = 224, VJ_P = 16, VJ_G = VJ_S / VJ_P, VJ_FRAMES = 16, VJ_TOK = (VJ_FRAMES / 2) * VJ_G * VJ_G;   // 1568 tokens
constexpr int VJ_D = TTV_VJEPA_WIDTH, VJ_H = 16, VJ_HD = 64, VJ_KIN = 3 * 2 * VJ_P * VJ_P, VJ_MLP = 4 * VJ_D;
constexpr int VJ_QB = (VJ_TOK + 127) / 128;   // 13 query blocks of 128 rows per (sequence, head)

struct JediClips {
  const void* x[TTV_MAX_CLIPS_PER_LAUNCH];
  int T[TTV_MAX_CLIPS_PER_LAUNCH], S[TTV_MAX_CLIPS_PER_LAUNCH];
};

template <typename T>
__device__ __forceinline__ float rescaled(const T* p) {
  float v = Cvt<T>::to_f(*p);
  v = fminf(fmaxf(v, -1.f), 1.f);
  return (v + 1.f) / 2.f;
}

// thread = (clip, token, c, kt, kh, half): 8 outputs kw = 8 half .. 8 half + 7 of one patch row
template <typename T>
__global__ __launch_bounds__(256) void k_jedi_prep(JediClips a, bf16_t* __restrict__ out) {
  const int clip = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= VJ_TOK * (VJ_KIN / 8)) return;
  const int tok = g / (VJ_KIN / 8), chunk = g - tok * (VJ_KIN / 8);   // chunk = ((c * 2 + kt) * 16 + kh) * 2 + half
  const int half = chunk & 1, kh = (chunk >> 1) & 15, kt = (chunk >> 5) & 1, c = chunk >> 6;
  const int tp = tok / (VJ_G * VJ_G), hp = (tok / VJ_G) % VJ_G, wp = tok % VJ_G;
  const int Tn = a.T[clip], S = a.S[clip];
  int f = 2 * tp + kt;
  f = f < Tn ? f : Tn - 1;                                            // pad_frames: the last frame repeated
  const T* frame = reinterpret_cast<const T*>(a.x[clip]) + ((size_t)c * Tn + f) * S * S;
  int iy[4];
  float wy[4];
  cubic_taps(hp * VJ_P + kh, S, VJ_S, iy, wy);   // torch's bicubic taps, shared with ttv_crops.hip (ttv_common.h)
  const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f;
  const float stdv = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int ix[4];
    float wx[4];
    cubic_taps(wp * VJ_P + half * 8 + e, S, VJ_S, ix, wx);
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // rows outer, columns inner, products and sums rounded one by one (torch's CPU order)
      const T* row = frame + (size_t)iy[r] * S;
      float h = __fmul_rn(rescaled(row + ix[0]), wx[0]);
      h = __fadd_rn(h, __fmul_rn(rescaled(row + ix[1]), wx[1]));
      h = __fadd_rn(h, __fmul_rn(rescaled(row + ix[2]), wx[2]));
      h = __fadd_rn(h, __fmul_rn(rescaled(row + ix[3]), wx[3]));
      acc = r == 0 ? __fmul_rn(h, wy[0]) : __fadd_rn(acc, __fmul_rn(h, wy[r]));
    }
    o[e] = (bf16_t)((acc - mean) / stdv);
  }
  *reinterpret_cast<bf16x8*>(out + ((size_t)clip * VJ_TOK + tok) * VJ_KIN + chunk * 8) = o;
}

__device__ __forceinline__ float xor_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// LayerNorm of one register-resident row (16 values per lane: four float4 at columns 4 lane + 256 i), weight / bias fp32
__device__ __forceinline__ void ln_row(f32x4 (&v)[4], const float* w, const float* b, float eps, int lane) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = xor_sum(s) * (1.f / VJ_D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[i][e] -= mean;
      q = fmaf(v[i][e], v[i][e], q);
    }
  const float rstd = 1.f / sqrtf(xor_sum(q) * (1.f / VJ_D) + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int col = 4 * lane + 256 * i;
    const f32x4 g = *reinterpret_cast<const f32x4*>(w + col), bb = *reinterpret_cast<const f32x4*>(b + col);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[i][e] = fmaf(v[i][e] * rstd, g[e], bb[e]);
  }
}

struct LnArgs {
  const float* x; int ldx; int rows;
  const float* w1; const float* b1; float eps1;
  const float* w2; const float* b2; float eps2;   // w2 == nullptr: one norm
  float* y32; int ld32;                           // optional: the first norm's output, fp32 (may alias x)
  bf16_t* y16; int ld16;                          // optional: the last norm's output, bf16
};

__global__ __launch_bounds__(256) void k_ln(LnArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const float* xr = a.x + (size_t)row * a.ldx;
  f32x4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * lane + 256 * i);
  ln_row(v, a.w1, a.b1, a.eps1, lane);
  if (a.y32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(a.y32 + (size_t)row * a.ld32 + 4 * lane + 256 * i) = v[i];
  }
  if (a.w2) ln_row(v, a.w2, a.b2, a.eps2, lane);
  if (a.y16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x4 o = {(bf16_t)v[i][0], (bf16_t)v[i][1], (bf16_t)v[i][2], (bf16_t)v[i][3]};
      *reinterpret_cast<bf16x4*>(a.y16 + (size_t)row * a.ld16 + 4 * lane + 256 * i) = o;
    }
  }
}

// entry b of the table: XCD list L = b % 8 holds the (sequence, head) groups g = L + 8 m (n * 16 groups, a multiple of 8)
__global__ __launch_bounds__(256) void k_attn_table(int n, int* __restrict__ tab, int* __restrict__ cu) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b <= n) cu[b] = b * VJ_TOK;
  if (b >= n * VJ_H * VJ_QB) return;
  const int L = b & 7, pos = b >> 3, m = pos / VJ_QB, qb = pos - m * VJ_QB;
  const int g = L + 8 * m;
  tab[4 * b + 0] = g / VJ_H;
  tab[4 * b + 1] = qb * 128;
  tab[4 * b + 2] = g % VJ_H;
  tab[4 * b + 3] = 0;
}

// softmax(q k^T / 8) v of one query row per (head, clip); kv rows [rows][2 * 1024] bf16 (k | v, head h at columns 64 h), q bf16 [1024]
__global__ __launch_bounds__(256) void k_pool_attn(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, int rows,
                                                   bf16_t* __restrict__ out) {
  extern __shared__ float sc[];                  // [rows] scores, then 4 x 64 partial outputs
  __shared__ float qs[VJ_HD], red[8];
  const int h = blockIdx.x, clip = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* base = kv + (size_t)clip * rows * (2 * VJ_D);
  if (tid < VJ_HD) qs[tid] = (float)q[h * VJ_HD + tid];
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < rows; j += 256) {
    const bf16_t* k = base + (size_t)j * (2 * VJ_D) + h * VJ_HD;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < VJ_HD; c += 8) {
      const bf16x8 kk = *reinterpret_cast<const bf16x8*>(k + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(qs[c + e], (float)kk[e], s);
    }
    s *= 0.125f;
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int j = tid; j < rows; j += 256) {
    const float p = __expf(sc[j] - mx);
    sc[j] = p;
    sum += p;
  }
  sum = xor_sum(sum);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();   // all p written, all partial sums in
  sum = (red[4] + red[5]) + (red[6] + red[7]);
  // output feature d = lane, key range quarter = wave
  const int q4 = (rows + 3) / 4, j0 = wave * q4, j1 = min(rows, j0 + q4);
  float o = 0.f;
  for (int j = j0; j < j1; ++j) o = fmaf(sc[j], (float)base[(size_t)j * (2 * VJ_D) + VJ_D + h * VJ_HD + lane], o);
  float* part = sc + ((rows + 3) & ~3);
  part[wave * VJ_HD + lane] = o;
  __syncthreads();
  if (wave == 0) {
    const float t = (part[lane] + part[VJ_HD + lane]) + (part[2 * VJ_HD + lane] + part[3 * VJ_HD + lane]);
    out[(size_t)clip * VJ_D + h * VJ_HD + lane] = (bf16_t)(t / sum);
  }
}

// feats[clip][col] = mean over the clip's 1568 rows of x (fp32), summed in row order
__global__ __launch_bounds__(256) void k_mean_rows(const float* __restrict__ x, int rows, float* __restrict__ feats) {
  const int clip = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
  const float* p = x + (size_t)clip * rows * VJ_D + col;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += p[(size_t)r * VJ_D];
  feats[(size_t)clip * VJ_D + col] = s / (float)rows;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int ln_launch(const LnArgs& a, hipStream_t s) {
  if (a.rows == 0) return TTV_OK;
  hipLaunchKernelGGL(k_ln, dim3(ttv_cdiv(a.rows, 4)), dim3(256), 0, s, a);
  TTV_CHECK_LAUNCH("vjepa layernorm");
  return TTV_OK;
}

int linear(int epi, const void* x, int ldx, const void* w, int ldw, const void* bias, int M, int N, int K, const float* resid, int ldr,
           int resid_rows, void* y, int ldy, hipStream_t s) {
  GemmArgs g = {};
  g.x = x; g.ldx = ldx; g.w = w; g.ldw = ldw; g.M = M; g.N = N; g.K = K; g.y = y; g.ldy = ldy; g.bias = bias;
  g.resid = resid; g.ldr = ldr; g.resid_rows = resid_rows; g.alpha = 1.f; g.dtype = TTV_BF16;
  const GemmEpilogue e = epi == TTV_VJEPA_EPI_STORE ? EPI_BIAS_PLAIN : epi == TTV_VJEPA_EPI_GELU ? EPI_BIAS_GELU : EPI_BIAS_RESID_F32R;
  return ttvk_gemm(e, g, s);
}

int pool_attn_launch(const void* q, const void* kv, int n, int rows, void* out, hipStream_t s) {
  const size_t lds = (size_t)(((rows + 3) & ~3) + 4 * VJ_HD) * sizeof(float);
  hipLaunchKernelGGL(k_pool_attn, dim3(VJ_H, n), dim3(256), lds, s, (const bf16_t*)q, (const bf16_t*)kv, rows, (bf16_t*)out);
  TTV_CHECK_LAUNCH("vjepa pooler attention");
  return TTV_OK;
}

struct Ws {
  int* tab; int* cu; float* xres; bf16_t* h; bf16_t* ao; bf16_t* big; bf16_t* pa; bf16_t* pb; bf16_t* pf;
  int64_t bytes;
};

Ws carve(char* base, int n) {
  Ws w;
  int64_t off = 0;
  auto take = [&](int64_t b) { char* p = base ? base + off : nullptr; off += align256(b); return p; };
  const int64_t M = (int64_t)n * VJ_TOK;
  w.tab = (int*)take((int64_t)n * VJ_H * VJ_QB * 4 * 4);
  w.cu = (int*)take((int64_t)(n + 1) * 4);
  w.xres = (float*)take(M * VJ_D * 4);
  w.h = (bf16_t*)take(M * VJ_D * 2);
  w.ao = (bf16_t*)take(M * VJ_D * 2);
  w.big = (bf16_t*)take(M * VJ_MLP * 2);
  w.pa = (bf16_t*)take((int64_t)n * VJ_D * 2);
  w.pb = (bf16_t*)take((int64_t)n * VJ_D * 2);
  w.pf = (bf16_t*)take((int64_t)n * VJ_MLP * 2);
  w.bytes = off;
  return w;
}

}  // namespace

int ttvk_jedi_preprocess(void* const* clips, const int32_t* dims, int n_clips, int dtype, void* out, hipStream_t st) {
  TTV_CHECK_ARG(n_clips >= 1 && n_clips <= TTV_MAX_CLIPS_PER_LAUNCH, "jedi preprocess: %d clips, 1 .. %d allowed", n_clips,
                TTV_MAX_CLIPS_PER_LAUNCH);
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "jedi preprocess: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(clips && dims && out, "jedi preprocess: null argument");
  TTV_CHECK_ARG(al16(out), "jedi preprocess: out must be 16-byte aligned");
  JediClips a;
  for (int i = 0; i < n_clips; ++i) {
    const int C = dims[4 * i], T = dims[4 * i + 1], H = dims[4 * i + 2], W = dims[4 * i + 3];
    TTV_CHECK_ARG(C == 3, "jedi preprocess: clip %d has %d channels, V-JEPA takes 3", i, C);
    TTV_CHECK_ARG(H == W, "jedi preprocess: clip %d is %d x %d; the reference resizes the shorter edge to 224 and then cannot "
                  "interpolate its position embedding for a non-square frame", i, H, W);
    TTV_CHECK_ARG(T >= 1 && T <= VJ_FRAMES, "jedi preprocess: clip %d has %d frames, 1 .. %d allowed (the reference cannot "
                  "interpolate its position embedding beyond 16)", i, T, VJ_FRAMES);
    TTV_CHECK_ARG(H >= 1 && (int64_t)T * H * W * 3 < ((int64_t)1 << 31), "jedi preprocess: clip %d has shape 3 x %d x %d x %d", i, T, H, W);
    TTV_CHECK_ARG(clips[i], "jedi preprocess: null clip %d", i);
    a.x[i] = clips[i];
    a.T[i] = T;
    a.S[i] = H;
  }
  const dim3 grid((unsigned)ttv_cdiv(VJ_TOK * (VJ_KIN / 8), 256), (unsigned)n_clips);
  if (dtype == TTV_BF16) hipLaunchKernelGGL(k_jedi_prep<bf16_t>, grid, dim3(256), 0, st, a, (bf16_t*)out);
  else hipLaunchKernelGGL(k_jedi_prep<float>, grid, dim3(256), 0, st, a, (bf16_t*)out);
  TTV_CHECK_LAUNCH("jedi preprocess");
  return TTV_OK;
}

int64_t ttvk_vjepa_workspace_bytes(int n) {
  if (n < 1 || n > TTV_MAX_CLIPS_PER_LAUNCH) {
    ttv_set_error("vjepa workspace: %d clips, 1 .. %d allowed", n, TTV_MAX_CLIPS_PER_LAUNCH);
    return -1;
  }
  return carve(nullptr, n).bytes;
}

int ttvk_vjepa_layernorm(const float* x, int ldx, int rows, int width, const float* w1, const float* b1, float eps1, const float* w2,
                         const float* b2, float eps2, float* y32, int ld32, void* y16, int ld16, hipStream_t s) {
  TTV_CHECK_ARG(width == VJ_D, "vjepa layernorm: width %d, only %d is built", width, VJ_D);
  TTV_CHECK_ARG(rows >= 0 && x && w1 && b1 && (y32 || y16), "vjepa layernorm: null argument");
  TTV_CHECK_ARG(!w2 || b2, "vjepa layernorm: the second norm needs its bias");
  TTV_CHECK_ARG(eps1 > 0.f && (!w2 || eps2 > 0.f), "vjepa layernorm: eps must be positive");
  TTV_CHECK_ARG(ldx >= width && ldx % 4 == 0 && (!y32 || (ld32 >= width && ld32 % 4 == 0)) && (!y16 || (ld16 >= width && ld16 % 4 == 0)),
                "vjepa layernorm: bad leading dimensions");
  TTV_CHECK_ARG(al16(x) && al16(w1) && al16(b1) && (!w2 || (al16(w2) && al16(b2))) && al16(y32) && ((uintptr_t)y16 & 7) == 0,
                "vjepa layernorm: unaligned pointers");
  LnArgs a = {x, ldx, rows, w1, b1, eps1, w2, b2, eps2, y32, ld32, (bf16_t*)y16, ld16};
  return ln_launch(a, s);
}

int ttvk_vjepa_linear(const void* x, int ldx, const void* w, int ldw, const void* bias, int M, int N, int K, int epilogue,
                      const float* resid, int ldr, int resid_rows, void* y, int ldy, hipStream_t s) {
  TTV_CHECK_ARG(epilogue == TTV_VJEPA_EPI_STORE || epilogue == TTV_VJEPA_EPI_GELU || epilogue == TTV_VJEPA_EPI_RESID,
                "vjepa linear: unknown epilogue %d", epilogue);
  TTV_CHECK_ARG(x && w && bias && y && M >= 0 && N > 0 && K > 0, "vjepa linear: null argument or bad shape");
  TTV_CHECK_ARG(N % 128 == 0 && K % 64 == 0, "vjepa linear: N = %d must be a multiple of 128 and K = %d of 64", N, K);
  TTV_CHECK_ARG(ldx >= K && ldw >= K && ldy >= N, "vjepa linear: leading dimensions smaller than the rows");
  TTV_CHECK_ARG(epilogue != TTV_VJEPA_EPI_RESID || (resid && ldr >= N && resid_rows >= 0), "vjepa linear: the residual epilogue needs resid");
  return linear(epilogue, x, ldx, w, ldw, bias, M, N, K, resid, ldr, resid_rows, y, ldy, s);
}

int ttvk_vjepa_pool_attention(const void* q, const void* kv, int n, int rows, void* out, hipStream_t s) {
  TTV_CHECK_ARG(q && kv && out, "vjepa pooler attention: null argument");
  TTV_CHECK_ARG(n >= 1 && n <= 65535 && rows >= 1 && rows <= 8192, "vjepa pooler attention: %d clips of %d rows", n, rows);
  TTV_CHECK_ARG(al16(kv), "vjepa pooler attention: kv must be 16-byte aligned");
  return pool_attn_launch(q, kv, n, rows, out, s);
}

int ttvk_vjepa_features(const ttv_vjepa_weights* w, const void* x, int n, float* feats, int finetuned, void* workspace,
                        int64_t workspace_bytes, hipStream_t s) {
  TTV_CHECK_ARG(w && x && feats && workspace, "vjepa features: null argument");
  TTV_CHECK_ARG(n >= 1 && n <= TTV_MAX_CLIPS_PER_LAUNCH, "vjepa features: %d clips, 1 .. %d allowed", n, TTV_MAX_CLIPS_PER_LAUNCH);
  TTV_CHECK_ARG(w->width == VJ_D && w->heads == VJ_H, "vjepa features: width %d / %d heads; only ViT-L (1024 / 16, head_dim 64) is built "
                "(vit_huge's head_dim 80 is not)", w->width, w->heads);
  TTV_CHECK_ARG(w->depth >= 1 && w->depth <= 64 && w->layers, "vjepa features: depth %d", w->depth);
  TTV_CHECK_ARG(w->patch_w && w->patch_b && w->pos_embed && w->norm_w && w->norm_b, "vjepa features: missing encoder weights");
  TTV_CHECK_ARG(!finetuned || (w->query_tokens && w->pool_q && w->pool_norm1_w && w->pool_norm1_b && w->pool_kv_w && w->pool_kv_b &&
                               w->pool_proj_w && w->pool_proj_b && w->pool_norm2_w && w->pool_norm2_b && w->pool_fc1_w && w->pool_fc1_b &&
                               w->pool_fc2_w && w->pool_fc2_b),
                "vjepa features: finetuned features need the pooler's weights");
  for (int l = 0; l < w->depth; ++l) {
    const ttv_vjepa_layer& L = w->layers[l];
    TTV_CHECK_ARG(L.norm1_w && L.norm1_b && L.qkv_w && L.qkv_b && L.proj_w && L.proj_b && L.norm2_w && L.norm2_b && L.fc1_w && L.fc1_b &&
                  L.fc2_w && L.fc2_b, "vjepa features: block %d has a null weight", l);
  }
  TTV_CHECK_ARG(al16(x) && al16(feats) && ((uintptr_t)workspace & 255) == 0, "vjepa features: x / feats 16-byte, workspace 256-byte aligned");
  const Ws ws = carve((char*)workspace, n);
  TTV_CHECK_ARG(workspace_bytes >= ws.bytes, "vjepa features: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)ws.bytes);
  const int M = n * VJ_TOK, E = n * VJ_H * VJ_QB;
  hipLaunchKernelGGL(k_attn_table, dim3(ttv_cdiv(E + 1, 256)), dim3(256), 0, s, n, ws.tab, ws.cu);
  TTV_CHECK_LAUNCH("vjepa attention table");
  // patch_embed.proj (Conv3d as a GEMM over tubelet rows), rounded to bf16, + pos_embed (fp32)
  TTV_TRY(linear(TTV_VJEPA_EPI_RESID, x, VJ_KIN, w->patch_w, VJ_KIN, w->patch_b, M, VJ_D, VJ_KIN, w->pos_embed, VJ_D, VJ_TOK, ws.xres, VJ_D, s));
  for (int l = 0; l < w->depth; ++l) {
    const ttv_vjepa_layer& L = w->layers[l];
    TTV_TRY(ln_launch({ws.xres, VJ_D, M, L.norm1_w, L.norm1_b, 1e-6f, nullptr, nullptr, 0.f, nullptr, 0, ws.h, VJ_D}, s));
    // qkv as q | (unused gate columns) | k | v, the layout of ttvk_attention
    TTV_TRY(linear(TTV_VJEPA_EPI_STORE, ws.h, VJ_D, L.qkv_w, VJ_D, L.qkv_b, M, VJ_D, VJ_D, nullptr, 0, 0, ws.big, 4 * VJ_D, s));
    TTV_TRY(linear(TTV_VJEPA_EPI_STORE, ws.h, VJ_D, (const bf16_t*)L.qkv_w + (size_t)VJ_D * VJ_D, VJ_D, (const bf16_t*)L.qkv_b + VJ_D, M,
                   2 * VJ_D, VJ_D, nullptr, 0, 0, ws.big + 2 * VJ_D, 4 * VJ_D, s));
    TTV_TRY(ttvk_attention(ws.big, 4 * VJ_D, ws.ao, VJ_D, ws.cu, ws.tab, E, VJ_H, VJ_H, VJ_HD, 0, TTV_BF16, s));
    TTV_TRY(linear(TTV_VJEPA_EPI_RESID, ws.ao, VJ_D, L.proj_w, VJ_D, L.proj_b, M, VJ_D, VJ_D, ws.xres, VJ_D, 0, ws.xres, VJ_D, s));
    TTV_TRY(ln_launch({ws.xres, VJ_D, M, L.norm2_w, L.norm2_b, 1e-6f, nullptr, nullptr, 0.f, nullptr, 0, ws.h, VJ_D}, s));
    TTV_TRY(linear(TTV_VJEPA_EPI_GELU, ws.h, VJ_D, L.fc1_w, VJ_D, L.fc1_b, M, VJ_MLP, VJ_D, nullptr, 0, 0, ws.big, VJ_MLP, s));
    TTV_TRY(linear(TTV_VJEPA_EPI_RESID, ws.big, VJ_MLP, L.fc2_w, VJ_MLP, L.fc2_b, M, VJ_D, VJ_MLP, ws.xres, VJ_D, 0, ws.xres, VJ_D, s));
  }
  if (!finetuned) {
    TTV_TRY(ln_launch({ws.xres, VJ_D, M, w->norm_w, w->norm_b, 1e-6f, nullptr, nullptr, 0.f, ws.xres, VJ_D, nullptr, 0}, s));
    hipLaunchKernelGGL(k_mean_rows, dim3(VJ_D / 256, n), dim3(256), 0, s, ws.xres, VJ_TOK, feats);
    TTV_CHECK_LAUNCH("vjepa token mean");
    return TTV_OK;
  }
  // the final norm (fp32 out, as autocast keeps layer_norm) and the pooler's norm1 in one pass, then AttentivePooler's CrossAttentionBlock
  TTV_TRY(ln_launch({ws.xres, VJ_D, M, w->norm_w, w->norm_b, 1e-6f, w->pool_norm1_w, w->pool_norm1_b, 1e-5f, nullptr, 0, ws.h, VJ_D}, s));
  TTV_TRY(linear(TTV_VJEPA_EPI_STORE, ws.h, VJ_D, w->pool_kv_w, VJ_D, w->pool_kv_b, M, 2 * VJ_D, VJ_D, nullptr, 0, 0, ws.big, 2 * VJ_D, s));
  TTV_TRY(pool_attn_launch(w->pool_q, ws.big, n, VJ_TOK, ws.pa, s));
  TTV_TRY(linear(TTV_VJEPA_EPI_RESID, ws.pa, VJ_D, w->pool_proj_w, VJ_D, w->pool_proj_b, n, VJ_D, VJ_D, w->query_tokens, VJ_D, 1, feats, VJ_D, s));
  TTV_TRY(ln_launch({feats, VJ_D, n, w->pool_norm2_w, w->pool_norm2_b, 1e-5f, nullptr, nullptr, 0.f, nullptr, 0, ws.pb, VJ_D}, s));
  TTV_TRY(linear(TTV_VJEPA_EPI_GELU, ws.pb, VJ_D, w->pool_fc1_w, VJ_D, w->pool_fc1_b, n, VJ_MLP, VJ_D, nullptr, 0, 0, ws.pf, VJ_MLP, s));
  TTV_TRY(linear(TTV_VJEPA_EPI_RESID, ws.pf, VJ_MLP, w->pool_fc2_w, VJ_MLP, w->pool_fc2_b, n, VJ_D, VJ_MLP, feats, VJ_D, 0, feats, VJ_D, s));
  return TTV_OK;
}
