// Loader front on the device: crop + antialiased bicubic resize + flip + normalisation of decoded uint8 frames, one launch per batch
// (reference dataset/video_dataset.py:38-127: v2.RandomResizedCrop / v2.Resize + CenterCrop with BICUBIC, antialias=True, then
// RandomHorizontalFlip, ToDtype and [-1, 1]).
//
// Value (aten's _upsample_bicubic2d_aa on the float path, include/titok_hip.h states it in full): separable, width pass then height
// pass, fp32 weights normalised by their sum, fp32 accumulation in ascending tap order, no rounding between the passes; then
// level = clamp(rint(v), 0, 255) and level / 127.5 - 1 formed exactly as k_clip_from_u8 forms it, one rounding to the clip's dtype.
//
// A block owns an output tile of RS_TH x RS_TW pixels of one frame, all three channels:
//   1. prologue: the tile's column and row taps (first source index, count, normalised weights) into LDS.  The tap centre
//      c = n_in * (2 i + 1) / (2 n_out) is split into an integer and a fraction in [0, 1) so that the weight argument (j - c + 0.5)
//      is formed from small numbers: the fp32 position error of scale * (i + 0.5) (6e-5 at column 640) never reaches the weights.
//   2. the source footprint is walked in chunks of RS_R rows.  A chunk's interleaved bytes come in with 16-byte loads from 16-byte
//      aligned addresses (the in-row shift 0 .. 15 is kept per row; a vector that is not wholly inside the source array is loaded
//      byte by byte, so nothing before or behind the array is touched), the width pass writes [row][channel][RS_TW] fp32 to LDS -
//      once per source row, whatever the number of output rows that use it - and the height pass adds the chunk's rows to the 12
//      accumulators of each thread (4 consecutive output columns x 3 channels of one output row), in ascending row order, so the sum
//      does not depend on where the chunks fall.
//   3. epilogue: round to a level, normalise, 4 elements per store along W (16 bytes fp32, 8 bytes bf16) when Wo % 4 == 0.
// `flip` only changes which resampled column an output column takes its taps from; loads and stores are the same.
#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

constexpr int RS_TW = 64;            // output tile width
constexpr int RS_TH = 16;            // output tile height
constexpr int RS_R = 16;             // source rows per chunk
constexpr int RS_MAX_SCALE = 8;      // n_in / n_out above this is refused on the host
constexpr int RS_MAXT = 36;          // taps per output index: at most 2 * support + 1 = 4 * RS_MAX_SCALE + 1 = 33 (+ fp32 slack), padded
constexpr int RS_MAX_COLS = (RS_TW - 1) * RS_MAX_SCALE + RS_MAXT + 2;      // source columns under one tile
constexpr int RS_ROW_BYTES = (RS_MAX_COLS * 3 + 15 + 15) / 16 * 16;        // + the alignment shift, in whole 16-byte vectors
constexpr int RS_MAX_DIM = 16384;
static_assert(4 * RS_MAX_SCALE + 1 <= RS_MAXT, "tap table too small for the scale cap");
static_assert(RS_TW * RS_TH * 3 == 256 * 12, "12 accumulators per thread");

struct ResampleClips {
  const uint8_t* src[TTV_MAX_CLIPS_PER_LAUNCH];
  void* dst[TTV_MAX_CLIPS_PER_LAUNCH];
  // two sizes per word, low | high << 16 (each <= RS_MAX_DIM).  Words on purpose: 16-bit arrays indexed by the clip make hipcc fold
  // clip * 2 into the 64-bit base of the scalar loads of the neighbouring 32-bit arrays, and a scalar load ignores the low two
  // bits of its base - odd clips then read the entry of the clip before them.
  uint32_t HsWs[TTV_MAX_CLIPS_PER_LAUNCH], HrWr[TTV_MAX_CLIPS_PER_LAUNCH], oyox[TTV_MAX_CLIPS_PER_LAUNCH], HoWo[TTV_MAX_CLIPS_PER_LAUNCH];
  int32_t T_flip[TTV_MAX_CLIPS_PER_LAUNCH];            // T | flip << 30
  int32_t block0[TTV_MAX_CLIPS_PER_LAUNCH + 1];        // first block of each clip; block0[n] = blocks of the call
  int32_t n;
};

// Keys cubic convolution kernel, a = -0.5 (aten's bicubic antialias filter)
__device__ __forceinline__ float cubic_aa(float x) {
  x = fabsf(x);
  if (x < 1.0f) return ((1.5f * x - 2.5f) * x) * x + 1.0f;
  if (x < 2.0f) return -0.5f * (((x - 5.0f) * x + 8.0f) * x - 4.0f);
  return 0.0f;
}

// One axis, output index i of n_out over n_in samples: first tap, tap count and what the weights need (centre = q + frac).
struct Taps {
  int lo, cnt, q;
  float frac, inv;
};
__device__ __forceinline__ Taps taps_of(int i, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out;
  const float support = scale >= 1.0f ? 2.0f * scale : 2.0f;
  const int num = n_in * (2 * i + 1), den = 2 * n_out;         // < 2^31: both sizes <= RS_MAX_DIM
  Taps t;
  t.q = num / den;
  t.frac = (float)(num - t.q * den) / (float)den;
  t.inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
  const float c = (float)t.q + t.frac;
  t.lo = max(0, (int)(c - support + 0.5f));
  const int hi = min(min((int)(c + support + 0.5f), n_in), t.lo + RS_MAXT);
  t.cnt = max(hi - t.lo, 0);
  return t;
}

template <typename T>
__global__ __launch_bounds__(256) void k_clip_resample_u8(const ResampleClips a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[RS_R * RS_ROW_BYTES];
  __shared__ __attribute__((aligned(16))) float s_mid[RS_R * 3 * RS_TW];
  __shared__ float s_wx[RS_MAXT * RS_TW];            // [tap][column]: lanes of the width pass read consecutive words
  __shared__ float s_wy[RS_TH * RS_MAXT];            // [row][tap]
  __shared__ int s_xlo[RS_TW], s_xcnt[RS_TW], s_ylo[RS_TH], s_ycnt[RS_TH];

  const int tid = threadIdx.x;
  int clip = 0;
  for (int step = TTV_MAX_CLIPS_PER_LAUNCH / 2; step > 0; step >>= 1)
    if (clip + step < a.n && a.block0[clip + step] <= (int)blockIdx.x) clip += step;
  const int Hs = a.HsWs[clip] & 0xFFFF, Ws = a.HsWs[clip] >> 16, Hr = a.HrWr[clip] & 0xFFFF, Wr = a.HrWr[clip] >> 16;
  const int oy = a.oyox[clip] & 0xFFFF, ox = a.oyox[clip] >> 16, Ho = a.HoWo[clip] & 0xFFFF, Wo = a.HoWo[clip] >> 16;
  const int T_ = a.T_flip[clip] & 0x3FFFFFFF, flip = a.T_flip[clip] >> 30;
  const int tiles_x = (Wo + RS_TW - 1) / RS_TW, tiles_y = (Ho + RS_TH - 1) / RS_TH;
  int b = (int)blockIdx.x - a.block0[clip];
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, t = b / tiles_y;
  const int x0 = tx * RS_TW, y0 = ty * RS_TH;
  const int nx = min(RS_TW, Wo - x0), ny = min(RS_TH, Ho - y0);      // valid columns / rows of this tile

  // ---- 1. taps -------------------------------------------------------------------------------
  if (tid < RS_TW + RS_TH) {
    const bool is_x = tid < RS_TW;
    const int e = is_x ? tid : tid - RS_TW;
    const bool valid = e < (is_x ? nx : ny);
    const int i = is_x ? ox + (flip ? Wo - 1 - (x0 + e) : x0 + e) : oy + y0 + e;
    Taps tp = taps_of(valid ? i : 0, is_x ? Ws : Hs, is_x ? Wr : Hr);
    if (!valid) tp.cnt = 0;
    float total = 0.0f;
    for (int k = 0; k < tp.cnt; ++k) {
      const float w = cubic_aa(((float)(tp.lo + k - tp.q) + (0.5f - tp.frac)) * tp.inv);
      total += w;
      if (is_x) s_wx[k * RS_TW + e] = w;
      else s_wy[e * RS_MAXT + k] = w;
    }
    for (int k = 0; k < tp.cnt; ++k) {
      if (is_x) s_wx[k * RS_TW + e] = __fdiv_rn(s_wx[k * RS_TW + e], total);
      else s_wy[e * RS_MAXT + k] = __fdiv_rn(s_wy[e * RS_MAXT + k], total);
    }
    if (is_x) { s_xlo[e] = tp.lo; s_xcnt[e] = tp.cnt; }
    else { s_ylo[e] = tp.lo; s_ycnt[e] = tp.cnt; }
  }
  __syncthreads();

  // footprint of the tile: taps are monotonic in the resampled index, a flipped tile runs right to left
  const int xa = flip ? nx - 1 : 0, xb = flip ? 0 : nx - 1;
  const int fx0 = s_xlo[xa];
  const int ncols = min(s_xlo[xb] + s_xcnt[xb] - fx0, RS_MAX_COLS);
  const int fy0 = s_ylo[0], fy1 = s_ylo[ny - 1] + s_ycnt[ny - 1];

  const uint8_t* const src_begin = a.src[clip];
  const uint8_t* const src_end = src_begin + (size_t)T_ * Hs * Ws * 3;
  const uint8_t* const frame = src_begin + (size_t)t * Hs * Ws * 3;

  // width pass: thread = one output column, rows wr, wr + 4, wr + 8, wr + 12 of the chunk
  const int wx = tid & (RS_TW - 1), wr = tid >> 6;
  const int my_xcnt = s_xcnt[wx];
  const int my_xoff = min(max(s_xlo[wx] - fx0, 0), RS_MAX_COLS - RS_MAXT) * 3;
  // height pass: thread = output row hy, columns 4 hx .. 4 hx + 3
  const int hy = tid >> 4, hx = tid & 15;
  const int my_ylo = s_ylo[hy], my_yhi = my_ylo + s_ycnt[hy];
  f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  for (int r0 = fy0; r0 < fy1; r0 += RS_R) {
    const int nr = min(RS_R, fy1 - r0);
    // ---- 2a. source bytes of rows r0 .. r0 + nr, columns fx0 .. fx0 + ncols ---------------------------------
    {
      const int nvec = (ncols * 3 + 15 + 15) / 16;            // covers any shift; <= RS_ROW_BYTES / 16
      for (int idx = tid; idx < nr * nvec; idx += 256) {
        const int rr = idx / nvec, v = idx - rr * nvec;
        const uint8_t* g = frame + ((size_t)(r0 + rr) * Ws + fx0) * 3;
        const uint8_t* ga = g - ((uintptr_t)g & 15) + (size_t)v * 16;
        uint4 val;
        if (ga >= src_begin && ga + 16 <= src_end) {
          val = *reinterpret_cast<const uint4*>(ga);
        } else {
          uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (ga + k >= src_begin && ga + k < src_end) w[k >> 2] |= (uint32_t)ga[k] << (8 * (k & 3));
          val = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(s_src + rr * RS_ROW_BYTES + v * 16) = val;
      }
    }
    __syncthreads();
    // ---- 2b. width pass -> s_mid[row][channel][column] ----------------------------------------------------
    {
      float m[4][3];
      const uint8_t* p[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rr = wr + 4 * i;
        const uint8_t* g = frame + ((size_t)(r0 + rr) * Ws + fx0) * 3;
        p[i] = s_src + rr * RS_ROW_BYTES + (int)((uintptr_t)g & 15) + my_xoff;
        m[i][0] = m[i][1] = m[i][2] = 0.0f;
      }
      for (int k = 0; k < my_xcnt; ++k) {
        const float w = s_wx[k * RS_TW + wx];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (wr + 4 * i < nr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) m[i][c] = fmaf(w, (float)p[i][3 * k + c], m[i][c]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) s_mid[((wr + 4 * i) * 3 + c) * RS_TW + wx] = m[i][c];
    }
    __syncthreads();
    // ---- 2c. height pass over the rows of this chunk ---------------------------------------------------------
    {
      const int ja = max(my_ylo, r0), jb = min(my_yhi, r0 + nr);
      for (int j = ja; j < jb; ++j) {
        const float w = s_wy[hy * RS_MAXT + (j - my_ylo)];
        const float* mrow = s_mid + (j - r0) * 3 * RS_TW + hx * 4;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(mrow + c * RS_TW);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[c][e] = fmaf(w, v[e], acc[c][e]);
        }
      }
    }
    // the next chunk's loads overwrite s_src, which 2b has finished reading (barrier above); its 2b overwrites s_mid only after
    // the barrier that follows those loads, which every thread reaches after its 2c
  }

  // ---- 3. level, normalisation, store -------------------------------------------------------------
  const int y = y0 + hy, x = x0 + hx * 4;
  if (hy >= ny || x >= Wo) return;
  T* const dst = reinterpret_cast<T*>(a.dst[clip]);
  const size_t plane = (size_t)Ho * Wo;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float level = fminf(fmaxf(rintf(acc[c][e]), 0.0f), 255.0f);
      o[e] = __fsub_rn(__fdiv_rn(level, 127.5f), 1.0f);
    }
    T* row = dst + ((size_t)c * T_ + t) * plane + (size_t)y * Wo + x;
    if ((Wo & 3) == 0) {            // x % 4 == 0 and the clip is 16-byte aligned: whole vectors, never past the row
      Vec4<T>::store(row, o);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < Wo) row[e] = Cvt<T>::from_f(o[e]);
    }
  }
}

}  // namespace

int ttvk_clip_resample_u8(void* const* src, void* const* dst, const int32_t* geom, int n_clips, int dtype, hipStream_t s) {
  TTV_CHECK_ARG(n_clips >= 0 && n_clips <= TTV_MAX_CLIPS_PER_LAUNCH, "clip_resample_u8: %d clips, at most %d per call", n_clips,
                TTV_MAX_CLIPS_PER_LAUNCH);
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "clip_resample_u8: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  if (n_clips == 0) return TTV_OK;
  TTV_CHECK_ARG(src && dst && geom, "clip_resample_u8: null argument");
  ResampleClips a = {};
  int64_t blocks = 0;
  for (int i = 0; i < n_clips; ++i) {
    const int32_t* g = geom + 10 * i;
    const int T = g[0], Hs = g[1], Ws = g[2], Hr = g[3], Wr = g[4], oy = g[5], ox = g[6], Ho = g[7], Wo = g[8], flip = g[9];
    TTV_CHECK_ARG(src[i] && dst[i], "clip_resample_u8: null pointer in clip %d", i);
    TTV_CHECK_ARG(T >= 1 && Hs >= 1 && Ws >= 1 && Hr >= 1 && Wr >= 1 && Ho >= 1 && Wo >= 1 && Hs <= RS_MAX_DIM && Ws <= RS_MAX_DIM &&
                      Hr <= RS_MAX_DIM && Wr <= RS_MAX_DIM && T <= RS_MAX_DIM,
                  "clip_resample_u8: clip %d: T %d, source %d x %d, resized %d x %d, output %d x %d (each 1 .. %d)", i, T, Hs, Ws, Hr, Wr, Ho,
                  Wo, RS_MAX_DIM);
    TTV_CHECK_ARG((int64_t)T * Hs * Ws * 3 < ((int64_t)1 << 31) && (int64_t)T * Ho * Wo * 3 < ((int64_t)1 << 31),
                  "clip_resample_u8: clip %d is too large (2^31 bytes / elements)", i);
    TTV_CHECK_ARG(Hs <= RS_MAX_SCALE * Hr && Ws <= RS_MAX_SCALE * Wr,
                  "clip_resample_u8: clip %d: scale %d x %d -> %d x %d is above the cap of %d per axis", i, Hs, Ws, Hr, Wr, RS_MAX_SCALE);
    TTV_CHECK_ARG(oy >= 0 && ox >= 0 && oy + Ho <= Hr && ox + Wo <= Wr,
                  "clip_resample_u8: clip %d: window %d x %d at (%d, %d) lies outside the resized frame %d x %d", i, Ho, Wo, oy, ox, Hr, Wr);
    TTV_CHECK_ARG(flip == 0 || flip == 1, "clip_resample_u8: clip %d: flip = %d (0 or 1)", i, flip);
    TTV_CHECK_ARG((uintptr_t)dst[i] % 16 == 0, "clip_resample_u8: destination of clip %d is not 16-byte aligned", i);
    a.src[i] = (const uint8_t*)src[i];
    a.dst[i] = dst[i];
    a.HsWs[i] = (uint32_t)Hs | (uint32_t)Ws << 16;
    a.HrWr[i] = (uint32_t)Hr | (uint32_t)Wr << 16;
    a.oyox[i] = (uint32_t)oy | (uint32_t)ox << 16;
    a.HoWo[i] = (uint32_t)Ho | (uint32_t)Wo << 16;
    a.T_flip[i] = T | (flip << 30);
    a.block0[i] = (int32_t)blocks;
    blocks += (int64_t)T * ttv_cdiv(Ho, RS_TH) * ttv_cdiv(Wo, RS_TW);
    TTV_CHECK_ARG(blocks < ((int64_t)1 << 31), "clip_resample_u8: too many output tiles in one call");
  }
  for (int i = n_clips; i <= TTV_MAX_CLIPS_PER_LAUNCH; ++i) a.block0[i] = (int32_t)blocks;
  a.n = n_clips;
  if (dtype == TTV_BF16) hipLaunchKernelGGL(k_clip_resample_u8<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_clip_resample_u8<float>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  TTV_CHECK_LAUNCH("clip_resample_u8");
  return TTV_OK;
}
