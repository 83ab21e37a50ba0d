// How good the video is that comes back (titok_video_amd/video.py: frame_sse, frame_ssim, VideoQuality): per frame and per component
// (R, G, B of packed uint8 frames, or Y, U, V of 4:2:0 planes) the exact sum of squared level differences and the SSIM between the
// pictures under test `a` (frame j) and the yardstick `b` (frame j * b_stride).  include/titok_hip.h states every value.
//
// Kernels
//   k_frame_sse_rgb      : a frame pair is two runs of L = 3 H W bytes whose byte k belongs to component k % 3.  A thread takes 12 bytes
//                          (4 pixels, so the component of every byte is a constant) of both: the 4 aligned words that hold them,
//                          shifted into place (v_alignbyte_b32; the two sides may sit differently on the word grid), byte by byte
//                          where a word would leave the array and in the last, shorter group of a frame.  TTV_QSSE_ITERS groups per
//                          thread, 256 groups apart; three 32-bit partials, summed over the wave by lane exchanges, over the block
//                          through 48 bytes of LDS, and added to the frame's three 64-bit sums by one vector atomic each.
//   k_frame_sse_planes   : the same for three planes with pitches; a block works on one component of one frame, a thread takes 8
//                          samples of a row from each side: 8 bytes out of 3 aligned words (planar), or the even bytes of 16 out of
//                          5 aligned words (interleaved chroma: the other component's bytes are loaded and dropped).  Rows off the
//                          word grid go through the same shift; the end of a row that is no multiple of 8 samples and words that
//                          would leave the plane's extent go byte by byte.  Pitch padding is never read into a sum.
//   k_frame_ssim         : k_ssim_tiles (ttv_metrics.hip) on levels: one workgroup per (frame, component, 32 x 32 tile of the valid
//                          region); the tile and its 5-sample halo (42 x 42) of both planes staged in LDS as fp32 pairs after
//                          subtracting the sample at the centre of the tile's first window from each plane (integers up to 255 in
//                          magnitude, squares up to 65025: exact in fp32), byte loads with the component's sample step (3 for packed
//                          RGB, 1 or 2 for planes); horizontal pass to five maps of 42 x 32, vertical pass with 4 outputs per thread;
//                          the tile's sum as a double into workspace slot = block index.  43.4 KB of LDS, three workgroups per CU.
//   k_frame_ssim_finish  : a thread per (frame, component) adds its tiles in tile order and divides by (h - 10)(w - 10).
// Traffic: the SSE kernels read every compared byte once (2 x 3 bytes per RGB pixel, 2 x 1.5 per 4:2:0 pixel; an interleaved chroma
// plane twice, the second time from the cache); the SSIM kernel reads (42 / 32)^2 = 1.72 times that for whole tiles.
#include <algorithm>
#include <cmath>

#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

// One component of one side: sample (frame j, row y, column x) is the byte base[j * frame + y * pitch + x * step]; [base, end) is
// what the caller vouches for (from the first sample of the first frame to the last sample of the last frame).
struct QPlane {
  const uint8_t* base;
  const uint8_t* end;
  int64_t frame, pitch;
  int32_t step;
};
struct QPair {
  QPlane a[3], b[3];
  int32_t h[3], w[3];
  int32_t b_stride;
};

// ---- sums of squared differences ------------------------------------------------------------------------------------------------------
// Items of a block: 256 * TTV_QSSE_ITERS groups of at most 8 samples of one component, so a block's partial stays in 32 bits.
#ifndef TTV_QSSE_ITERS
#define TTV_QSSE_ITERS 4
#endif
static_assert(TTV_QSSE_ITERS >= 1 && 256ull * TTV_QSSE_ITERS * 8 * 65025 < (1ull << 32), "a block's partial sum must fit 32 bits");

// nb (<= 4 * N) bytes from p, in place in d; the rest of d is zero.  N + 1 aligned words shifted into place where all 4 * N bytes are
// wanted and the words lie inside [lo, hi); byte by byte elsewhere.
template <int N>
__device__ __forceinline__ void load_bytes(const uint8_t* p, const uint8_t* lo, const uint8_t* hi, int nb, uint32_t (&d)[N]) {
  const uintptr_t at = (uintptr_t)p, w0 = at & ~(uintptr_t)3;
  if (nb == 4 * N && w0 >= (uintptr_t)lo && w0 + 4 * (N + 1) <= (uintptr_t)hi) {
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(w0);
    uint32_t w[N + 1];
#pragma unroll
    for (int k = 0; k <= N; ++k) w[k] = wp[k];
    const uint32_t sh = (uint32_t)(at & 3);
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = 0;
#pragma unroll
    for (int i = 0; i < 4 * N; ++i)
      if (i < nb) d[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
  }
}
// ns (<= 8) samples from p, `step` (1 or 2) bytes apart, packed into d; the rest of d is zero.
__device__ __forceinline__ void load_samples8(const uint8_t* p, int step, const uint8_t* lo, const uint8_t* hi, int ns, uint32_t (&d)[2]) {
  if (step == 1) {
    load_bytes<2>(p, lo, hi, ns, d);
  } else {
    // 15 bytes hold the 8 samples; the 16th (the other component's) is asked for and dropped, so the word path needs it inside
    uint32_t t[4];
    load_bytes<4>(p, lo, hi, ns == 8 && p + 16 <= hi ? 16 : 2 * ns - 1, t);
    d[0] = (t[0] & 0xFFu) | ((t[0] >> 8) & 0xFF00u) | ((t[1] & 0xFFu) << 16) | ((t[1] << 8) & 0xFF000000u);
    d[1] = (t[2] & 0xFFu) | ((t[2] >> 8) & 0xFF00u) | ((t[3] & 0xFFu) << 16) | ((t[3] << 8) & 0xFF000000u);
  }
}
__device__ __forceinline__ uint32_t sq_diff_u8(uint32_t wa, uint32_t wb, int byte) {
  const int d = (int)((wa >> (8 * byte)) & 0xFFu) - (int)((wb >> (8 * byte)) & 0xFFu);
  return (uint32_t)__mul24(d, d);
}

// The block's sums of N partials per thread (all 256 threads arrive), each below 2^32, added to dst[0 .. N) by one 64-bit atomic each.
template <int N>
__device__ __forceinline__ void block_add_u64(const uint32_t (&part)[N], unsigned long long* dst) {
  __shared__ uint32_t wave_part[4][N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const uint32_t s = wave_sum_u32(part[c]);
    if ((threadIdx.x & 63u) == 0) wave_part[threadIdx.x >> 6][c] = s;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int c = threadIdx.x;
    const uint32_t total = wave_part[0][c] + wave_part[1][c] + wave_part[2][c] + wave_part[3][c];
    if (total) atomicAdd(dst + c, (unsigned long long)total);
  }
}

__global__ __launch_bounds__(256) void k_frame_sse_rgb(const uint8_t* __restrict__ a, const uint8_t* a_end,
                                                       const uint8_t* __restrict__ b, const uint8_t* b_end, long long L,
                                                       int b_stride, long long groups, uint32_t blocks_per_frame,
                                                       unsigned long long* __restrict__ sse) {
  const uint32_t j = blockIdx.x / blocks_per_frame;
  const long long first = (long long)(blockIdx.x - j * blocks_per_frame) * (256 * TTV_QSSE_ITERS) + threadIdx.x;
  const uint8_t* fa = a + (size_t)j * L;
  const uint8_t* fb = b + (size_t)j * b_stride * L;
  uint32_t part[3] = {0, 0, 0};
#pragma unroll
  for (int it = 0; it < TTV_QSSE_ITERS; ++it) {
    const long long g = first + it * 256;                          // group of 12 bytes = 4 pixels of the frame
    if (g >= groups) break;
    const long long k0 = g * 12;
    const int nb = (int)min(12ll, L - k0);
    uint32_t da[3], db[3];
    load_bytes<3>(fa + k0, a, a_end, nb, da);
    load_bytes<3>(fb + k0, b, b_end, nb, db);
#pragma unroll
    for (int i = 0; i < 12; ++i) part[i % 3] += sq_diff_u8(da[i >> 2], db[i >> 2], i & 3);      // bytes beyond nb are 0 on both sides
  }
  block_add_u64<3>(part, sse + (size_t)j * 3);
}

__global__ __launch_bounds__(256) void k_frame_sse_planes(const QPair q, uint32_t bpc0, uint32_t bpc1, unsigned long long* __restrict__ sse) {
  const uint32_t blocks_per_frame = bpc0 + 2 * bpc1;
  const uint32_t j = blockIdx.x / blocks_per_frame, r = blockIdx.x - j * blocks_per_frame;
  const int c = r < bpc0 ? 0 : (r < bpc0 + bpc1 ? 1 : 2);
  const uint32_t chunk = r - (c == 0 ? 0 : (c == 1 ? bpc0 : bpc0 + bpc1));
  const QPlane A = q.a[c], B = q.b[c];
  const int h = q.h[c], w = q.w[c];
  const uint32_t per_row = ((uint32_t)w + 7u) / 8u, groups = per_row * (uint32_t)h;      // below 2^31 (the entry point's check)
  const uint32_t first = chunk * (256u * TTV_QSSE_ITERS) + threadIdx.x;
  const uint8_t* fa = A.base + (size_t)j * A.frame;
  const uint8_t* fb = B.base + (size_t)j * q.b_stride * B.frame;
  uint32_t part[1] = {0};
#pragma unroll
  for (int it = 0; it < TTV_QSSE_ITERS; ++it) {
    const uint32_t g = first + (uint32_t)it * 256u;                // group of 8 samples of a row
    if (g >= groups) break;
    const uint32_t y = g / per_row;
    const int x0 = (int)(g - y * per_row) * 8, ns = min(8, w - x0);
    uint32_t da[2], db[2];
    load_samples8(fa + (size_t)y * A.pitch + (size_t)x0 * A.step, A.step, A.base, A.end, ns, da);
    load_samples8(fb + (size_t)y * B.pitch + (size_t)x0 * B.step, B.step, B.base, B.end, ns, db);
#pragma unroll
    for (int i = 0; i < 8; ++i) part[0] += sq_diff_u8(da[i >> 2], db[i >> 2], i & 3);          // samples beyond ns are 0 on both sides
  }
  block_add_u64<1>(part, sse + (size_t)j * 3 + c);
}

// ---- SSIM -----------------------------------------------------------------------------------------------------------------------------
#define QS_R 5                       // window radius
#define QS_TH 32                     // output tile rows
#define QS_TW 32                     // output tile columns
#define QS_SH (QS_TH + 2 * QS_R)     // staged rows (42)
#define QS_SW (QS_TW + 2 * QS_R)     // staged columns (42)
#define QS_SP (QS_SW + 1)            // staged row pitch in (x, y) pairs: odd, so the horizontal pass's 8-byte reads are conflict-free

struct QTaps {
  float g[2 * QS_R + 1];
};
// first workspace slot of each component inside a frame; t0[3] = slots per frame
struct QTiles {
  int32_t t0[4];
};
__host__ __device__ __forceinline__ int qs_tiles_x(int w) { return (w - 2 * QS_R + QS_TW - 1) / QS_TW; }
__host__ __device__ __forceinline__ int qs_tiles_y(int h) { return (h - 2 * QS_R + QS_TH - 1) / QS_TH; }

__global__ __launch_bounds__(256) void k_frame_ssim(const QPair q, const QTiles tl, const QTaps taps, double* __restrict__ part) {
  __shared__ f32x2 sxy[QS_SH * QS_SP];   // staged (x - kx, y - ky)
  __shared__ f32x2 hm[QS_SH * QS_TW];    // horizontal pass: (x, y)
  __shared__ f32x2 hq[QS_SH * QS_TW];    //                  (x^2, y^2)
  __shared__ float hp[QS_SH * QS_TW];    //                  xy
  __shared__ double red[256];
  constexpr float C1 = 6.5025f, C2 = 58.5225f;    // (0.01 * 255)^2, (0.03 * 255)^2
  constexpr int NIT = (QS_SH * QS_SW + 255) / 256;

  const uint32_t per_frame = (uint32_t)tl.t0[3];
  const uint32_t j = blockIdx.x / per_frame, r = blockIdx.x - j * per_frame;
  const int c = (int)r < tl.t0[1] ? 0 : ((int)r < tl.t0[2] ? 1 : 2);
  const int tile = (int)r - tl.t0[c];
  const QPlane A = q.a[c], B = q.b[c];
  const int h = q.h[c], w = q.w[c];
  const int tx = qs_tiles_x(w);
  const int y0 = (tile / tx) * QS_TH, x0 = (tile % tx) * QS_TW;
  const int vh = min(QS_TH, h - 2 * QS_R - y0), vw = min(QS_TW, w - 2 * QS_R - x0);   // valid outputs of this tile
  const uint8_t* fa = A.base + (size_t)j * A.frame;
  const uint8_t* fb = B.base + (size_t)j * q.b_stride * B.frame;
  const int tid = threadIdx.x;

  // ---- stage: rows y0 .. y0 + 41, columns x0 .. x0 + 41; cells outside the plane (read by no kept window) hold 0
  const float kx = (float)fa[(size_t)(y0 + QS_R) * A.pitch + (size_t)(x0 + QS_R) * A.step];
  const float ky = (float)fb[(size_t)(y0 + QS_R) * B.pitch + (size_t)(x0 + QS_R) * B.step];
  float xs[NIT], ys[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + it * 256, rr = i / QS_SW, cc = i - rr * QS_SW;
    const int gy = y0 + rr, gx = x0 + cc;
    const bool in = i < QS_SH * QS_SW && gy < h && gx < w;
    xs[it] = in ? (float)fa[(size_t)gy * A.pitch + (size_t)gx * A.step] : kx;
    ys[it] = in ? (float)fb[(size_t)gy * B.pitch + (size_t)gx * B.step] : ky;
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + it * 256, rr = i / QS_SW, cc = i - rr * QS_SW;
    if (i < QS_SH * QS_SW) sxy[rr * QS_SP + cc] = (f32x2){xs[it] - kx, ys[it] - ky};
  }
  __syncthreads();

  // ---- horizontal pass: 42 rows x 8 groups of 4 output columns (taps in ascending order for every output)
  for (int i = tid; i < QS_SH * (QS_TW / 4); i += 256) {
    const int rr = i / (QS_TW / 4), c0 = (i % (QS_TW / 4)) * 4;
    float sx[4] = {}, sy[4] = {}, sxx[4] = {}, syy[4] = {}, sxy_[4] = {};
#pragma unroll
    for (int k = 0; k < 2 * QS_R + 4; ++k) {
      const f32x2 v = sxy[rr * QS_SP + c0 + k];
      const float xx = v.x * v.x, yy = v.y * v.y, xy = v.x * v.y;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int t = k - o;
        if (t >= 0 && t <= 2 * QS_R) {
          sx[o] = fmaf(taps.g[t], v.x, sx[o]);
          sy[o] = fmaf(taps.g[t], v.y, sy[o]);
          sxx[o] = fmaf(taps.g[t], xx, sxx[o]);
          syy[o] = fmaf(taps.g[t], yy, syy[o]);
          sxy_[o] = fmaf(taps.g[t], xy, sxy_[o]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      hm[rr * QS_TW + c0 + o] = (f32x2){sx[o], sy[o]};
      hq[rr * QS_TW + c0 + o] = (f32x2){sxx[o], syy[o]};
      hp[rr * QS_TW + c0 + o] = sxy_[o];
    }
  }
  __syncthreads();

  // ---- vertical pass + index: 4 consecutive output rows of one column per thread
  const int vc = tid & (QS_TW - 1), vr0 = (tid / QS_TW) * 4;
  double acc = 0.0;
  {
    float mx[4] = {}, my[4] = {}, exx[4] = {}, eyy[4] = {}, exy[4] = {};
#pragma unroll
    for (int i = 0; i < 2 * QS_R + 4; ++i) {
      const int row = (vr0 + i) * QS_TW + vc;
      const f32x2 m = hm[row], s = hq[row];
      const float p = hp[row];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int t = i - o;
        if (t >= 0 && t <= 2 * QS_R) {
          mx[o] = fmaf(taps.g[t], m.x, mx[o]);
          my[o] = fmaf(taps.g[t], m.y, my[o]);
          exx[o] = fmaf(taps.g[t], s.x, exx[o]);
          eyy[o] = fmaf(taps.g[t], s.y, eyy[o]);
          exy[o] = fmaf(taps.g[t], p, exy[o]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (vr0 + o < vh && vc < vw) {
        const float sx2 = fmaxf(fmaf(-mx[o], mx[o], exx[o]), 0.0f);    // shift-free second moments
        const float sy2 = fmaxf(fmaf(-my[o], my[o], eyy[o]), 0.0f);
        const float sxy2 = fmaf(-mx[o], my[o], exy[o]);
        const float ux = kx + mx[o], uy = ky + my[o];                  // means of the unshifted planes
        const float num = (2.0f * (ux * uy) + C1) * (2.0f * sxy2 + C2);
        const float den = ((ux * ux + uy * uy) + C1) * ((sx2 + sy2) + C2);
        acc += (double)(num / den);
      }
    }
  }
  // fixed-order sum over the 256 threads
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_frame_ssim_finish(const QPair q, const QTiles tl, long long entries, const double* __restrict__ part,
                                                           double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const long long j = e / 3;
  const int c = (int)(e - j * 3);
  const double* p = part + (size_t)j * tl.t0[3] + tl.t0[c];
  const int tiles = tl.t0[c + 1] - tl.t0[c];
  double v = 0.0;
  for (int k = 0; k < tiles; ++k) v += p[k];
  out[e] = v / ((double)(q.h[c] - 2 * QS_R) * (double)(q.w[c] - 2 * QS_R));
}

// ---- host: the checks and the kernels' view ---------------------------------------------------------------------------------------------
// The frames a side holds: n for `a`, (n - 1) * b_stride + 1 for `b` (one for an empty call, so the description is still checked).
int64_t side_frames(int n, int stride) { return n > 0 ? (int64_t)(n - 1) * stride + 1 : 1; }

int common_checks(const char* what, int n, int b_stride, int H, int W, int min_hw) {
  TTV_CHECK_ARG(n >= 0 && b_stride >= 1, "%s: n = %d frames at b_stride %d (n >= 0, b_stride >= 1)", what, n, b_stride);
  TTV_CHECK_ARG(H >= min_hw && W >= min_hw, "%s: frames of %d x %d; H and W must be at least %d", what, H, W, min_hw);
  return TTV_OK;
}

int rgb_pair(const char* what, const void* a, const void* b, int n, int b_stride, int H, int W, int min_hw, QPair* q) {
  const int rc = common_checks(what, n, b_stride, H, W, min_hw);
  if (rc != TTV_OK) return rc;
  TTV_CHECK_ARG(a && b, "%s: null frames", what);
  const int64_t L = (int64_t)3 * H * W;
  for (int c = 0; c < 3; ++c) {
    q->a[c] = {(const uint8_t*)a + c, (const uint8_t*)a + side_frames(n, 1) * L, L, (int64_t)3 * W, 3};
    q->b[c] = {(const uint8_t*)b + c, (const uint8_t*)b + side_frames(n, b_stride) * L, L, (int64_t)3 * W, 3};
    q->h[c] = H;
    q->w[c] = W;
  }
  q->b_stride = b_stride;
  return TTV_OK;
}

// The checks include/titok_hip.h lists for a ttv_yuv420 that holds `frames` frames of H x W (matrix, range and siting are not read).
int yuv_side(const char* what, const char* side, const ttv_yuv420* f, int H, int W, int64_t frames, QPlane (&p)[3]) {
  TTV_CHECK_ARG(f != nullptr, "%s: null frame description (%s)", what, side);
  TTV_CHECK_ARG(f->y && f->u && f->v, "%s: a null plane (%s)", what, side);
  TTV_CHECK_ARG(f->c_step == 1 || f->c_step == 2, "%s: c_step %d is neither 1 (planar) nor 2 (interleaved) (%s)", what, f->c_step, side);
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int64_t c_row = (int64_t)f->c_step * (Wc - 1) + 1;
  TTV_CHECK_ARG(f->y_pitch >= W && f->c_pitch >= (int64_t)f->c_step * Wc, "%s: pitches %d and %d for rows of %d and %lld bytes (%s)", what,
                f->y_pitch, f->c_pitch, W, (long long)f->c_step * Wc, side);
  const int64_t y_min = (int64_t)(H - 1) * f->y_pitch + W, c_min = (int64_t)(Hc - 1) * f->c_pitch + c_row;
  TTV_CHECK_ARG(f->y_frame >= y_min && f->c_frame >= c_min, "%s: frame strides %lld and %lld for frames of %lld and %lld bytes (%s)", what,
                (long long)f->y_frame, (long long)f->c_frame, (long long)y_min, (long long)c_min, side);
  const uint8_t *y = (const uint8_t*)f->y, *u = (const uint8_t*)f->u, *v = (const uint8_t*)f->v;
  p[0] = {y, y + (frames - 1) * f->y_frame + y_min, f->y_frame, f->y_pitch, 1};
  p[1] = {u, u + (frames - 1) * f->c_frame + c_min, f->c_frame, f->c_pitch, f->c_step};
  p[2] = {v, v + (frames - 1) * f->c_frame + c_min, f->c_frame, f->c_pitch, f->c_step};
  return TTV_OK;
}

int yuv_pair(const char* what, const ttv_yuv420* a, const ttv_yuv420* b, int n, int b_stride, int H, int W, int min_hw, QPair* q) {
  int rc = common_checks(what, n, b_stride, H, W, min_hw);
  if (rc != TTV_OK) return rc;
  if ((rc = yuv_side(what, "a", a, H, W, side_frames(n, 1), q->a)) != TTV_OK) return rc;
  if ((rc = yuv_side(what, "b", b, H, W, side_frames(n, b_stride), q->b)) != TTV_OK) return rc;
  q->h[0] = H;
  q->w[0] = W;
  q->h[1] = q->h[2] = (H + 1) / 2;
  q->w[1] = q->w[2] = (W + 1) / 2;
  q->b_stride = b_stride;
  return TTV_OK;
}

int clear_sums(const char* what, uint64_t* sse, int n, hipStream_t s) {
  // the blocks of a frame add into its sums, so they start at zero: written, not accumulated
  const hipError_t e = hipMemsetAsync(sse, 0, (size_t)n * 3 * sizeof(uint64_t), s);
  if (e != hipSuccess) {
    ttv_set_error("%s: clearing the sums: %s", what, hipGetErrorString(e));
    return TTV_ERR_LAUNCH;
  }
  return TTV_OK;
}

QTiles ssim_tiles(const QPair& q) {
  QTiles t;
  t.t0[0] = 0;
  for (int c = 0; c < 3; ++c) t.t0[c + 1] = t.t0[c] + qs_tiles_x(q.w[c]) * qs_tiles_y(q.h[c]);
  return t;
}
// workspace slots of a call, or -1 (error set) when they do not fit one launch
int64_t ssim_slots(const char* what, const QPair& q, int n) {
  int64_t per_frame = 0;
  for (int c = 0; c < 3; ++c) per_frame += (int64_t)qs_tiles_x(q.w[c]) * qs_tiles_y(q.h[c]);
  if (per_frame * std::max(n, 1) >= ((int64_t)1 << 31)) {
    ttv_set_error("%s: %lld tiles in one call (below 2^31: take fewer frames)", what, (long long)(per_frame * n));
    return -1;
  }
  return per_frame * n;
}

int launch_ssim(const char* what, const QPair& q, int n, double* ssim, void* workspace, int64_t workspace_bytes, void* stream) {
  const int64_t slots = ssim_slots(what, q, n);
  if (slots < 0) return TTV_ERR_INVALID;
  TTV_CHECK_ARG(ssim && workspace, "%s: null output or workspace", what);
  TTV_CHECK_ARG(((uintptr_t)ssim & 7) == 0 && ((uintptr_t)workspace & 7) == 0, "%s: output and workspace must be 8-byte aligned", what);
  TTV_CHECK_ARG(workspace_bytes >= slots * (int64_t)sizeof(double), "%s: workspace of %lld bytes, %lld needed", what, (long long)workspace_bytes,
                (long long)(slots * (int64_t)sizeof(double)));
  if (n == 0) return TTV_OK;
  QTaps taps;
  double g[2 * QS_R + 1], sum = 0.0;
  for (int i = 0; i <= 2 * QS_R; ++i) sum += g[i] = std::exp(-((i - QS_R) / 1.5) * ((i - QS_R) / 1.5) / 2.0);
  for (int i = 0; i <= 2 * QS_R; ++i) taps.g[i] = (float)(g[i] / sum);
  const QTiles tl = ssim_tiles(q);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(k_frame_ssim, dim3((unsigned)slots), dim3(256), 0, s, q, tl, taps, part);
  TTV_CHECK_LAUNCH(what);
  const long long entries = (long long)n * 3;
  hipLaunchKernelGGL(k_frame_ssim_finish, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, q, tl, entries, part, ssim);
  TTV_CHECK_LAUNCH(what);
  return TTV_OK;
}

}  // namespace

extern "C" {

int ttv_video_frame_sse_u8(const void* a_thwc, const void* b_thwc, int n, int b_stride, int H, int W, uint64_t* sse, void* stream) {
  QPair q;
  const int rc = rgb_pair("video_frame_sse_u8", a_thwc, b_thwc, n, b_stride, H, W, 1, &q);
  if (rc != TTV_OK) return rc;
  TTV_CHECK_ARG(sse && (uintptr_t)sse % 8 == 0, "video_frame_sse_u8: the sums are %s", sse ? "not 8-byte aligned" : "null");
  if (n == 0) return TTV_OK;
  const int64_t L = (int64_t)3 * H * W, groups = (L + 11) / 12, span = 256 * TTV_QSSE_ITERS;
  const int64_t per_frame = (groups + span - 1) / span, blocks = per_frame * n;
  TTV_CHECK_ARG(blocks < ((int64_t)1 << 31), "video_frame_sse_u8: %lld blocks in one launch (below 2^31: take fewer frames)", (long long)blocks);
  hipStream_t s = (hipStream_t)stream;
  const int rz = clear_sums("video_frame_sse_u8", sse, n, s);
  if (rz != TTV_OK) return rz;
  const uint8_t *a = (const uint8_t*)a_thwc, *b = (const uint8_t*)b_thwc;
  hipLaunchKernelGGL(k_frame_sse_rgb, dim3((unsigned)blocks), dim3(256), 0, s, a, a + (int64_t)n * L, b, b + side_frames(n, b_stride) * L,
                     (long long)L, b_stride, (long long)groups, (uint32_t)per_frame, reinterpret_cast<unsigned long long*>(sse));
  TTV_CHECK_LAUNCH("video_frame_sse_u8");
  return TTV_OK;
}

int ttv_video_frame_sse_yuv420(const ttv_yuv420* a, const ttv_yuv420* b, int n, int b_stride, int H, int W, uint64_t* sse, void* stream) {
  QPair q;
  const int rc = yuv_pair("video_frame_sse_yuv420", a, b, n, b_stride, H, W, 1, &q);
  if (rc != TTV_OK) return rc;
  TTV_CHECK_ARG(sse && (uintptr_t)sse % 8 == 0, "video_frame_sse_yuv420: the sums are %s", sse ? "not 8-byte aligned" : "null");
  if (n == 0) return TTV_OK;
  const int64_t span = 256 * TTV_QSSE_ITERS;
  const int64_t gy = (int64_t)((q.w[0] + 7) / 8) * q.h[0], gc = (int64_t)((q.w[1] + 7) / 8) * q.h[1];
  const int64_t by = (gy + span - 1) / span, bc = (gc + span - 1) / span, blocks = (by + 2 * bc) * n;
  TTV_CHECK_ARG(gy < ((int64_t)1 << 31), "video_frame_sse_yuv420: a luma plane of %d x %d is %lld groups of 8 samples (below 2^31)", H, W, (long long)gy);
  TTV_CHECK_ARG(blocks < ((int64_t)1 << 31), "video_frame_sse_yuv420: %lld blocks in one launch (below 2^31: take fewer frames)", (long long)blocks);
  hipStream_t s = (hipStream_t)stream;
  const int rz = clear_sums("video_frame_sse_yuv420", sse, n, s);
  if (rz != TTV_OK) return rz;
  hipLaunchKernelGGL(k_frame_sse_planes, dim3((unsigned)blocks), dim3(256), 0, s, q, (uint32_t)by, (uint32_t)bc,
                     reinterpret_cast<unsigned long long*>(sse));
  TTV_CHECK_LAUNCH("video_frame_sse_yuv420");
  return TTV_OK;
}

int64_t ttv_video_frame_ssim_workspace_bytes(int n, int H, int W, int yuv420) {
  const char* what = "video_frame_ssim_workspace_bytes";
  const int min_hw = yuv420 ? 4 * QS_R + 1 : 2 * QS_R + 1;
  if (common_checks(what, n, 1, H, W, min_hw) != TTV_OK) return -1;
  QPair q;
  for (int c = 0; c < 3; ++c) {
    q.h[c] = yuv420 && c ? (H + 1) / 2 : H;
    q.w[c] = yuv420 && c ? (W + 1) / 2 : W;
  }
  const int64_t slots = ssim_slots(what, q, n);
  return slots < 0 ? -1 : slots * (int64_t)sizeof(double);
}

int ttv_video_frame_ssim_u8(const void* a_thwc, const void* b_thwc, int n, int b_stride, int H, int W, double* ssim, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  QPair q;
  const int rc = rgb_pair("video_frame_ssim_u8", a_thwc, b_thwc, n, b_stride, H, W, 2 * QS_R + 1, &q);
  if (rc != TTV_OK) return rc;
  return launch_ssim("video_frame_ssim_u8", q, n, ssim, workspace, workspace_bytes, stream);
}

int ttv_video_frame_ssim_yuv420(const ttv_yuv420* a, const ttv_yuv420* b, int n, int b_stride, int H, int W, double* ssim, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  QPair q;
  const int rc = yuv_pair("video_frame_ssim_yuv420", a, b, n, b_stride, H, W, 4 * QS_R + 1, &q);
  if (rc != TTV_OK) return rc;
  return launch_ssim("video_frame_ssim_yuv420", q, n, ssim, workspace, workspace_bytes, stream);
}

}  // extern "C"
