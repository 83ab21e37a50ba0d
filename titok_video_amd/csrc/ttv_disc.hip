// The two stretches of the discriminator step that lie between the towers (reference model/losses/loss_module.py:165-213): the R1 / R2
// noise with both additions, and the logit head with its gradient.  include/titok_hip.h states the values in full.
//
// Kernels
//   k_gp_noise_add : out_real = real + s, out_fake = fake + s for every element of every clip, the same s for both (:189-191).  A
//                    multi-tensor kernel: a device table of (real, fake, out_real, out_fake, noise, numel, element offset) per clip and
//                    a flat list of (clip, first element) chunks of GP_CHUNK elements; blocks stride over the chunk list.  A thread owns
//                    16 bytes of each operand (8 bf16 / 4 fp32): two 16-byte loads, two 16-byte stores (three loads when s is given).
//                    No LDS.  Generate mode draws s in registers - Philox4x32-10 on the counter (element block, draw) under the key
//                    (seed), two Box-Muller pairs per block of four elements - and never writes it.  Clips whose pointers are not
//                    16-byte aligned, and the last numel % V elements of a clip, go element by element.
//   k_disc_head    : one block.  Per clip the mean of its R per-token outputs (fp32, rounded once to the input dtype: the logit the
//                    eager .mean(-1) returns), then in fp32 the relativistic loss, the finite-difference R1 / R2, the centering term,
//                    their means over clips and d total / d per-token output.  Threads stride over clips, a wave sums with DPP moves,
//                    the four waves meet in LDS: a fixed order, no atomics.
#include <math.h>

#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

constexpr int GP_CHUNK = 8192;           // elements per chunk; a multiple of 256 threads x 8 elements
constexpr int GP_MAX_BLOCKS = 4096;

struct GpEntry {                         // 56 bytes, the layout include/titok_hip.h gives
  const void* real;
  const void* fake;
  void* out_real;
  void* out_fake;
  const void* noise;
  int64_t numel;
  int64_t offset;
};

// a 32-bit word -> a uniform strictly inside (0, 1), exact in fp32
__device__ __forceinline__ float unit_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 0x1p-23f; }

// the four standard normals of one block: words (0, 1) and (2, 3) are one Box-Muller pair each, lanes cos, sin, cos, sin
__device__ __forceinline__ void normal4(uint64_t block, uint32_t k0, uint32_t k1, uint32_t d0, uint32_t d1, float (&n)[4]) {
  uint32_t c[4] = {(uint32_t)block, (uint32_t)(block >> 32), d0, d1};
  philox4x32_10(c, k0, k1);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float r = sqrtf(-2.0f * logf(unit_open(c[2 * p])));
    float sn, cs;
    sincospif(2.0f * unit_open(c[2 * p + 1]), &sn, &cs);
    n[2 * p] = r * cs;
    n[2 * p + 1] = r * sn;
  }
}

template <typename T, bool GEN>
__global__ __launch_bounds__(256) void k_gp_noise_add(const GpEntry* __restrict__ table, const int2* __restrict__ chunks, int n_chunks,
                                                      uint32_t k0, uint32_t k1, uint32_t d0, uint32_t d1, float gp_noise) {
  constexpr int V = 16 / (int)sizeof(T);
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const int2 c = chunks[ch];
    const GpEntry e = table[c.x];
    const int n = (int)e.numel;
    const int end = min(c.y + GP_CHUNK, n);
    const T* real = reinterpret_cast<const T*>(e.real);
    const T* fake = reinterpret_cast<const T*>(e.fake);
    const T* noise = reinterpret_cast<const T*>(e.noise);
    T* out_real = reinterpret_cast<T*>(e.out_real);
    T* out_fake = reinterpret_cast<T*>(e.out_fake);
    const bool vec_ok = (((uintptr_t)real | (uintptr_t)fake | (uintptr_t)out_real | (uintptr_t)out_fake | (GEN ? 0 : (uintptr_t)noise)) & 15) == 0;
    for (int i = c.y + (int)threadIdx.x * V; i < end; i += 256 * V) {      // i % V == 0: chunks start at multiples of GP_CHUNK
      const bool whole = vec_ok && i + V <= n;
      T rv[V], fv[V], sv[V], orv[V], ofv[V];
      if (whole) {
        *reinterpret_cast<uint4*>(rv) = *reinterpret_cast<const uint4*>(real + i);
        *reinterpret_cast<uint4*>(fv) = *reinterpret_cast<const uint4*>(fake + i);
        if (!GEN) *reinterpret_cast<uint4*>(sv) = *reinterpret_cast<const uint4*>(noise + i);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const bool in = i + k < n;
          rv[k] = in ? real[i + k] : Cvt<T>::from_f(0.f);
          fv[k] = in ? fake[i + k] : Cvt<T>::from_f(0.f);
          if (!GEN) sv[k] = in ? noise[i + k] : Cvt<T>::from_f(0.f);
        }
      }
      float s[V];
      if (GEN) {
        const uint64_t block = (uint64_t)(e.offset + i) >> 2;               // offset % 4 == 0 and i % 4 == 0
#pragma unroll
        for (int b = 0; b < V / 4; ++b) {
          float nn[4];
          normal4(block + b, k0, k1, d0, d1, nn);
#pragma unroll
          for (int k = 0; k < 4; ++k) s[4 * b + k] = round_to<T>(round_to<T>(nn[k]) * gp_noise);      // randn_like, then * gp_noise
        }
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] = Cvt<T>::to_f(sv[k]);
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        orv[k] = Cvt<T>::from_f(Cvt<T>::to_f(rv[k]) + s[k]);
        ofv[k] = Cvt<T>::from_f(Cvt<T>::to_f(fv[k]) + s[k]);
      }
      if (whole) {
        *reinterpret_cast<uint4*>(out_real + i) = *reinterpret_cast<const uint4*>(orv);
        *reinterpret_cast<uint4*>(out_fake + i) = *reinterpret_cast<const uint4*>(ofv);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (i + k < n) {
            out_real[i + k] = orv[k];
            out_fake[i + k] = ofv[k];
          }
      }
    }
  }
}

// ---- the logit head --------------------------------------------------------------------------------------------------------------
struct HeadArgs {
  const void* a;         // groups 0 .. G/2 - 1 (or all G when b is null)
  const void* b;         // groups G/2 .. G - 1, or null
  int32_t mode, G, n, R;
  float w_gp, w_center;  // gp_weight / gp_noise^2 and centering_weight; zero = term off
  float* terms;          // [8]
  float* grad;           // [G n R]
};

// torch's softplus (beta 1, threshold 20) and its derivative form
__device__ __forceinline__ float softplus20(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float softplus20_grad(float x) {
  const float z = expf(x);
  return x > 20.f ? 1.f : z / (z + 1.f);
}

template <typename T>
__global__ __launch_bounds__(256) void k_disc_head(const HeadArgs h) {
  __shared__ float red[4][5];
  const int n = h.n, R = h.R, G = h.G;
  const int half = (G / 2) * n * R;
  const T* a = reinterpret_cast<const T*>(h.a);
  const T* b = reinterpret_cast<const T*>(h.b);
  auto logit = [&](int g, int c) {
    const int t = (g * n + c) * R;
    const T* p = (b && t >= half) ? b + (t - half) : a + t;
    float sum = 0.f;
    for (int r = 0; r < R; ++r) sum += Cvt<T>::to_f(p[r]);
    return round_to<T>(sum / (float)R);
  };
  auto put = [&](int g, int c, float v) {
    float* q = h.grad + (size_t)(g * n + c) * R;
    for (int r = 0; r < R; ++r) q[r] = v;
  };
  const float per_token = 1.f / ((float)n * (float)R);
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};      // d_loss | g_loss, logits_relative, r1, r2, centering
  for (int c = threadIdx.x; c < n; c += 256) {
    const float sr = logit(0, c), sf = logit(1, c);
    const float m = sr - sf;
    if (h.mode == TTV_DISC_HEAD_GENERATOR) {     // g_loss = softplus(real - fake)
      acc[0] += softplus20(m);
      const float d = softplus20_grad(m) * per_token;
      put(0, c, d);
      put(1, c, -d);
      continue;
    }
    acc[0] += softplus20(-m);                     // d_loss = softplus(-(real - fake))
    acc[1] += m;
    const float d = softplus20_grad(-m);
    float gr = -d, gf = d;
    if (G == 4) {
      const float dr = sr - logit(2, c), df = sf - logit(3, c);
      acc[2] += dr * dr;
      acc[3] += df * df;
      const float pr = h.w_gp * (2.f * dr), pf = h.w_gp * (2.f * df);
      gr += pr;
      gf += pf;
      put(2, c, -pr * per_token);
      put(3, c, -pf * per_token);
    }
    if (h.w_center > 0.f) {
      const float sc = sr + sf;
      acc[4] += 0.5f * (sc * sc);
      gr += h.w_center * sc;
      gf += h.w_center * sc;
    }
    put(0, c, gr * per_token);
    put(1, c, gf * per_token);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float v = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mean[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) mean[k] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) / (float)n;
    float total = mean[0];
    if (h.mode == TTV_DISC_HEAD_DISCRIMINATOR) {
      if (G == 4) total += h.w_gp * (mean[2] + mean[3]);
      if (h.w_center > 0.f) total += h.w_center * mean[4];
    }
    h.terms[0] = total;
#pragma unroll
    for (int k = 0; k < 5; ++k) h.terms[1 + k] = mean[k];
    h.terms[6] = 0.f;
    h.terms[7] = 0.f;
  }
}

}  // namespace

extern "C" {

int ttv_gp_noise_add(const void* table, int n_clips, const int32_t* chunks, int n_chunks, int generate, uint64_t seed, uint64_t draw,
                     float gp_noise, int dtype, void* stream) {
  if (n_chunks == 0) return TTV_OK;
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "gp_noise_add: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(n_clips >= 1 && n_chunks >= 1 && table && chunks, "gp_noise_add: %d clips, %d chunks, or a null table", n_clips, n_chunks);
  TTV_CHECK_ARG((uintptr_t)table % 8 == 0 && (uintptr_t)chunks % 8 == 0, "gp_noise_add: a table is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)(n_chunks < GP_MAX_BLOCKS ? n_chunks : GP_MAX_BLOCKS);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), d0 = (uint32_t)draw, d1 = (uint32_t)(draw >> 32);
  const GpEntry* t = (const GpEntry*)table;
  const int2* c = (const int2*)chunks;
  if (dtype == TTV_BF16) {
    if (generate) hipLaunchKernelGGL((k_gp_noise_add<bf16_t, true>), dim3(blocks), dim3(256), 0, s, t, c, n_chunks, k0, k1, d0, d1, gp_noise);
    else hipLaunchKernelGGL((k_gp_noise_add<bf16_t, false>), dim3(blocks), dim3(256), 0, s, t, c, n_chunks, k0, k1, d0, d1, gp_noise);
  } else {
    if (generate) hipLaunchKernelGGL((k_gp_noise_add<float, true>), dim3(blocks), dim3(256), 0, s, t, c, n_chunks, k0, k1, d0, d1, gp_noise);
    else hipLaunchKernelGGL((k_gp_noise_add<float, false>), dim3(blocks), dim3(256), 0, s, t, c, n_chunks, k0, k1, d0, d1, gp_noise);
  }
  TTV_CHECK_LAUNCH("gp_noise_add");
  return TTV_OK;
}

int ttv_disc_head(const void* per_token_a, const void* per_token_b, int mode, int groups, int n_clips, int tokens_per_clip, int dtype,
                  float gp_scale, float centering_weight, float* terms, float* grad, void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "disc_head: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(mode == TTV_DISC_HEAD_GENERATOR || mode == TTV_DISC_HEAD_DISCRIMINATOR, "disc_head: mode %d", mode);
  TTV_CHECK_ARG(groups == 2 || (groups == 4 && mode == TTV_DISC_HEAD_DISCRIMINATOR), "disc_head: %d groups (2, or 4 in discriminator mode)", groups);
  TTV_CHECK_ARG(n_clips >= 1 && tokens_per_clip >= 1 && (int64_t)groups * n_clips * tokens_per_clip < ((int64_t)1 << 31),
                "disc_head: %d clips of %d tokens", n_clips, tokens_per_clip);
  TTV_CHECK_ARG(per_token_a && terms && grad, "disc_head: null argument");
  TTV_CHECK_ARG(gp_scale >= 0.f && centering_weight >= 0.f, "disc_head: negative weight");
  HeadArgs h = {per_token_a, per_token_b, mode, groups, n_clips, tokens_per_clip, groups == 4 ? gp_scale : 0.f,
                mode == TTV_DISC_HEAD_DISCRIMINATOR ? centering_weight : 0.f, terms, grad};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TTV_BF16) hipLaunchKernelGGL(k_disc_head<bf16_t>, dim3(1), dim3(256), 0, s, h);
  else hipLaunchKernelGGL(k_disc_head<float>, dim3(1), dim3(256), 0, s, h);
  TTV_CHECK_LAUNCH("disc_head");
  return TTV_OK;
}

}  // extern "C"
