// The logged side-by-side video of the validation step (reference train.py:141-142): per selected clip
//   torch.cat((y, x.clamp(-1, 1)), dim=-1).permute(1, 0, 2, 3).cpu().float().numpy(), then ((v + 1) / 2 * 255).astype(np.uint8)
// as ONE launch that writes the uint8 panel [T][3][H][2W] of every clip it is given: columns 0 .. W-1 the target y, columns W .. 2W-1
// the reconstruction x clamped to [-1, 1].  include/titok_hip.h states the value in full; it is numpy's fp32 arithmetic step by step
// (add, divide, multiply, each rounded to fp32; truncation), so the bytes are defined bit for bit.
//
// Kernel
//   k_recon_panels<T, VEC> : grid (tiles, clips of the launch), no LDS.  Lanes run along W of the output.
//     VEC  : W % 8 == 0 and 16-byte aligned sources, 8-byte aligned panel (the trainer's case: patch width 8, torch allocations).  A
//            thread owns 8 consecutive columns of one half of one output row: one 16-byte load (bf16) or two (fp32), one 8-byte store
//            of the eight packed levels.  A wave covers 512 consecutive output bytes.
//     !VEC : any W, any alignment.  A thread owns one 4-byte-aligned word of the panel's byte range (its first and last words may be
//            partial: those bytes go singly), reads its four sources element by element - they may sit in two rows, or in both
//            halves - and stores the word once.
//   Every input element is read once and every output byte written once.
// Traffic at the trainer's shape, 16 clips of 16 x 128 x 128 bf16: 2 x 16 x 786 432 x 2 B = 50.3 MB read, 16 x 1 572 864 B = 25.2 MB
// written, 75.5 MB in all: 12 us at the 6.3 TB/s a streaming kernel reaches on MI355X (9.4 us at the 8 TB/s of the data sheet).
// Measured (tools/val_bench.py, profiles/val_bench.txt): 19.3 us per launch = 3.9 TB/s, 0.62 of that floor, when the launches
// rotate over eight working sets (576 MiB, more than twice the Infinity Cache, so every byte comes from and goes to HBM); 16.8 us
// on one working set, which the cache holds between launches.  With the copy and the host side 0.55 ms per call, against 14 - 17 ms
// for the eager expression on the same box.
// The eager expression moves the target and the reconstruction through four kernels (clamp, cat, the fp32 copy of the permuted
// view) and sends 4 bytes per element over the host link, where this sends 1.
#include <algorithm>

#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

struct PanelArgs {
  const void* target[TTV_MAX_CLIPS_PER_LAUNCH];
  const void* recon[TTV_MAX_CLIPS_PER_LAUNCH];
  uint8_t* out[TTV_MAX_CLIPS_PER_LAUNCH];
  int32_t T[TTV_MAX_CLIPS_PER_LAUNCH], H[TTV_MAX_CLIPS_PER_LAUNCH], W[TTV_MAX_CLIPS_PER_LAUNCH];
};

// ((v + 1) / 2 * 255) in fp32, every step rounded on its own (no contraction: the sum is not folded into the product), truncated
// toward zero.  Where numpy leaves astype(uint8) to the platform: below 0 -> 0, 255 and above -> 255, NaN -> 0.
__device__ __forceinline__ uint32_t panel_level(float v) {
#pragma clang fp contract(off)
  float t = v + 1.0f;
  t = t / 2.0f;
  t = t * 255.0f;
  if (!(t > 0.0f)) return 0u;          // negatives, -0, NaN
  if (t >= 255.0f) return 255u;
  return (uint32_t)t;
}
// torch's clamp(-1, 1): a NaN stays a NaN (and becomes level 0)
__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }

template <typename T> __device__ __forceinline__ void load8(const T* p, float (&o)[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&o)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float (&o)[8]) {
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (float)a[e];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_recon_panels(const PanelArgs a) {
  const int clip = blockIdx.y;
  const int Tn = a.T[clip], H = a.H[clip], W = a.W[clip];
  const T* trg = reinterpret_cast<const T*>(a.target[clip]);
  const T* rec = reinterpret_cast<const T*>(a.recon[clip]);
  uint8_t* out = a.out[clip];
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;          // a panel is below 2^31 bytes: 32-bit index arithmetic throughout
  const uint32_t rows = (uint32_t)Tn * 3u * (uint32_t)H;        // output rows (t, c, h), 2W bytes each
  if (VEC) {
    const uint32_t per_row = (uint32_t)W / 4u;                  // groups of 8 columns in an output row of 2W
    if (g >= rows * per_row) return;
    const uint32_t row = g / per_row, seg = g - row * per_row;
    const uint32_t tc = row / (uint32_t)H, h = row - tc * (uint32_t)H, t = tc / 3u, c = tc - 3u * t;
    const bool second = seg >= per_row / 2u;                    // wave-uniform wherever W >= 512; both sides are a load and a pack
    const uint32_t col = (second ? seg - per_row / 2u : seg) * 8u;
    const size_t src = (((size_t)c * Tn + t) * H + h) * W + col;
    float v[8];
    load8<T>((second ? rec : trg) + src, v);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo |= panel_level(second ? clamp1(v[e]) : v[e]) << (8 * e);
      hi |= panel_level(second ? clamp1(v[4 + e]) : v[4 + e]) << (8 * e);
    }
    *reinterpret_cast<uint2*>(out + (size_t)row * 2 * W + (size_t)seg * 8) = make_uint2(lo, hi);
  } else {
    const long long total = (long long)rows * 2 * W;
    const int mis = (int)((uintptr_t)out & 3);           // the words are those of the address space, not of the panel
    const long long j0 = (long long)g * 4 - mis;         // first byte of this thread's word, relative to the panel
    if (j0 >= total) return;
    const long long jb = j0 < 0 ? 0 : j0, je = j0 + 4 < total ? j0 + 4 : total;
    uint32_t row = (uint32_t)jb / (2u * (uint32_t)W), col = (uint32_t)jb - row * 2u * (uint32_t)W;
    uint32_t word = 0;
    for (long long j = jb; j < je; ++j) {
      const uint32_t tc = row / (uint32_t)H, h = row - tc * (uint32_t)H, t = tc / 3u, c = tc - 3u * t;
      const size_t base = (((size_t)c * Tn + t) * H + h) * W;
      const float v = col < (uint32_t)W ? Cvt<T>::to_f(trg[base + col]) : clamp1(Cvt<T>::to_f(rec[base + col - W]));
      word |= panel_level(v) << (8 * (int)(j - j0));
      if (++col == 2u * (uint32_t)W) { col = 0; ++row; }
    }
    if (je - jb == 4) {
      *reinterpret_cast<uint32_t*>(out + j0) = word;
    } else {
      for (long long j = jb; j < je; ++j) out[j] = (uint8_t)(word >> (8 * (int)(j - j0)));
    }
  }
}

template <typename T>
void launch(const PanelArgs& a, int n, bool vec, long long items, hipStream_t s) {
  const dim3 grid((unsigned)((items + 255) / 256), (unsigned)n);
  if (vec) hipLaunchKernelGGL((k_recon_panels<T, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_recon_panels<T, false>), grid, dim3(256), 0, s, a);
}

}  // namespace

extern "C" {

int ttv_recon_panels_u8(void* const* target, void* const* recon, const int32_t* dims, int n_clips, int dtype, void* const* panels,
                        void* stream) {
  if (n_clips == 0) return TTV_OK;
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "recon_panels_u8: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(n_clips > 0 && target && recon && dims && panels, "recon_panels_u8: %d clips, or a null table", n_clips);
  const size_t esz = dtype_bytes(dtype);
  for (int i = 0; i < n_clips; ++i) {
    const int T = dims[3 * i], H = dims[3 * i + 1], W = dims[3 * i + 2];
    TTV_CHECK_ARG(T >= 1 && H >= 1 && W >= 1 && T <= 65536 && H <= 65536 && W <= 65536 && (int64_t)3 * T * H * 2 * W < ((int64_t)1 << 31),
                  "recon_panels_u8: clip %d is %d x %d x %d (each 1 .. 65536, a panel below 2^31 bytes)", i, T, H, W);
    TTV_CHECK_ARG(target[i] && recon[i] && panels[i], "recon_panels_u8: null pointer in clip %d", i);
    TTV_CHECK_ARG((uintptr_t)target[i] % esz == 0 && (uintptr_t)recon[i] % esz == 0, "recon_panels_u8: clip %d is not aligned to its element size", i);
  }
  hipStream_t s = (hipStream_t)stream;
  // A launch takes up to TTV_MAX_CLIPS_PER_LAUNCH clips of one path: clips that can go 16 bytes at a time, and the others.
  for (int pass = 0; pass < 2; ++pass) {
    const bool vec = pass == 0;
    PanelArgs a = {};
    int n = 0;
    long long items = 0;
    auto flush = [&]() -> int {
      if (n == 0) return TTV_OK;
      if (dtype == TTV_BF16) launch<bf16_t>(a, n, vec, items, s);
      else launch<float>(a, n, vec, items, s);
      TTV_CHECK_LAUNCH("recon_panels_u8");
      n = 0;
      items = 0;
      return TTV_OK;
    };
    for (int i = 0; i < n_clips; ++i) {
      const int T = dims[3 * i], H = dims[3 * i + 1], W = dims[3 * i + 2];
      const bool can = W % 8 == 0 && (uintptr_t)target[i] % 16 == 0 && (uintptr_t)recon[i] % 16 == 0 && (uintptr_t)panels[i] % 8 == 0;
      if (can != vec) continue;
      a.target[n] = target[i]; a.recon[n] = recon[i]; a.out[n] = (uint8_t*)panels[i];
      a.T[n] = T; a.H[n] = H; a.W[n] = W;
      const long long bytes = (long long)3 * T * H * 2 * W;
      items = std::max(items, vec ? bytes / 8 : bytes / 4 + 2);      // + 2: a misaligned panel touches one word more, and the remainder
      if (++n == TTV_MAX_CLIPS_PER_LAUNCH) {
        const int rc = flush();
        if (rc != TTV_OK) return rc;
      }
    }
    const int rc = flush();
    if (rc != TTV_OK) return rc;
  }
  return TTV_OK;
}

}  // extern "C"
