// Whole videos in and out (titok_video_amd/video.py): a decoded video uint8 [T][H][W][3] is cut into equal, overlapping 3-D tiles the
// towers can take, and the reconstructed tiles are blended back into uint8 frames.  include/titok_hip.h states the plan (origins,
// tile order, weights) and the value of every output element; both kernels are streaming kernels with no atomics.  A third one
// measures what a reconstruction costs: per tile the exact integer sum of squared level differences against the source
// (ttv_video_tile_sse_u8; video.py builds the per-tile token allocation on it).
// The same three with Y'CbCr 4:2:0 planes in place of packed RGB (ttv_video_*_yuv420) follow the RGB kernels below.
//
// Kernels
//   k_video_tiles<T>     : grid (blocks per tile x tiles of the range), 1 KiB of LDS (the 256 normalised levels).  Wt % 8 == 0.  A
//                          thread owns 8 consecutive pixels of one tile row: their 24 source bytes start at any byte offset (rows
//                          are 3W bytes), so it loads the 7 aligned words that hold them, shifts them into place (v_alignbyte_b32)
//                          and stores one 16-byte (bf16) or two 16-byte (fp32) vectors into each of the three channel planes.  A
//                          thread whose words would leave the array, or whose columns are clamped (W shorter than the tile), reads
//                          its bytes one by one.
//   k_video_tiles_any<T> : any Wt, a thread per pixel of a tile: 3 byte loads, 3 element stores.
//   k_video_blend<T>     : a thread owns 4 consecutive pixels of an output row (12 bytes).  It walks the tiles that hold any of them
//                          in ascending index - up to 3 per axis for a pixel - and reads from each one vector per channel (the four
//                          pixels inside the tile on a vector boundary) or up to 12 single elements; the 12 bytes go out as three
//                          words when they lie on the 4-byte grid (always, when 3W % 4 == 0 and the output is aligned; one row in
//                          four otherwise) and byte by byte elsewhere.
//   k_video_tile_sse<T>  : k_video_tiles with the tile read, not written: the same thread geometry and source load, one 16-byte
//                          (bf16) or two 16-byte (fp32) loads per channel plane; a thread takes 8 such groups of 8 pixels, 256
//                          groups apart, and keeps a 32-bit partial, summed over the wave by lane exchanges, over the block through
//                          16 bytes of LDS, and added to the tile's 64-bit sum by one vector atomic per block.
//                          k_video_tile_sse_any<T>: any Wt, a pixel at a time.  Reads what the gather reads and writes, stores
//                          8 bytes per tile.
// Traffic per pixel of the timeline, tile t with overlap o per axis (r = prod t / (t - o), the cover ratio: 1.75 at 16 x 128 x 128
// with 4 x 16 x 16): the gather reads 3 r bytes and writes 3 r elements; the blend reads 3 r elements and writes 3 bytes.  DESIGN.md
// has the measured rates beside a device-to-device copy of the same byte count.
#include <algorithm>

#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

struct VideoAxis {
  int32_t n;          // length on the timeline
  int32_t tile, stride, count, overlap;
};
struct VideoGeo {
  VideoAxis a[3];
  int32_t H, W, frame_stride;      // of the source frames
};

__host__ __device__ __forceinline__ int axis_origin(const VideoAxis& a, int k) {
  if (k < a.count - 1) return k * a.stride;
  return a.n > a.tile ? a.n - a.tile : 0;
}
__host__ __device__ __forceinline__ int axis_weight(const VideoAxis& a, int u) {
  int w = u + 1;
  if (a.tile - u < w) w = a.tile - u;
  if (a.overlap + 1 < w) w = a.overlap + 1;
  return w;
}

// The tiles of an axis that hold any of the points p0 .. p1 (p0 == p1: one point): `regular` consecutive ones from k0 among the
// tiles 0 .. count - 2 - from the first that holds p0 to the last that holds p1 - then the last tile (index count - 1) when p1
// reaches it.  Ascending, and however many there are (three at most for one point under the plan's rules).  Whether a tile of a
// span holds one given point is its local coordinate's business.
struct Cover {
  int k0, regular, n;
};
__device__ __forceinline__ Cover axis_cover(const VideoAxis& a, int p0, int p1) {
  Cover c = {0, 0, 0};
  if (a.count > 1) {
    const int lo = p0 - a.tile + 1;
    c.k0 = lo <= 0 ? 0 : (lo + a.stride - 1) / a.stride;
    const int hi = min(p1 / a.stride, a.count - 2);
    c.regular = hi >= c.k0 ? hi - c.k0 + 1 : 0;
  }
  c.n = c.regular + (p1 >= a.n - a.tile ? 1 : 0);
  return c;
}
__device__ __forceinline__ int cover_tile(const VideoAxis& a, const Cover& c, int j) { return j < c.regular ? c.k0 + j : a.count - 1; }

template <typename T> __device__ __forceinline__ void store8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&v)[8]) {
  *reinterpret_cast<f32x4*>(p) = (f32x4){v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = (f32x4){v[4], v[5], v[6], v[7]};
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float (&v)[8]) {
  bf16x8 b;
#pragma unroll
  for (int e = 0; e < 8; ++e) b[e] = (bf16_t)v[e];
  *reinterpret_cast<bf16x8*>(p) = b;
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
struct TileAt {
  int t0, h0, w0;
};
__device__ __forceinline__ TileAt tile_origin(const VideoGeo& g, int tile) {
  const int kw = tile % g.a[2].count, r = tile / g.a[2].count;
  return {axis_origin(g.a[0], r / g.a[1].count), axis_origin(g.a[1], r % g.a[1].count), axis_origin(g.a[2], kw)};
}
// byte offset of the source row of tile row (i, y): frame frame_stride * min(t0 + i, T' - 1), row min(h0 + y, H - 1)
__device__ __forceinline__ size_t source_row(const VideoGeo& g, const TileAt& o, int i, int y) {
  const int ts = g.frame_stride * min(o.t0 + i, g.a[0].n - 1), ys = min(o.h0 + y, g.H - 1);
  return ((size_t)ts * g.H + ys) * (size_t)g.W * 3;
}

// The 24 bytes of pixels x0 .. x0 + 7 of the source row `src`, in place in d (channel c of pixel e is byte 3 e + c): k_video_tiles'
// source load as a function, for k_video_tile_sse.  The 7 aligned words that hold the bytes, shifted into place; byte by byte, with
// the columns clamped to W - 1, where the pixels are not all inside the row or a word would leave the array.  (k_video_tiles keeps
// its own copy of these lines: called from there, the compiler orders the byte-wise path differently, and that kernel's code is
// held as it was measured.)
__device__ __forceinline__ void source_px8(const uint8_t* frames, size_t frame_bytes, const uint8_t* src, int x0, int W, uint32_t (&d)[6]) {
  const uintptr_t at = (uintptr_t)(src + (size_t)x0 * 3), lo = at & ~(uintptr_t)3;
  if (x0 + 8 <= W && lo >= (uintptr_t)frames && lo + 28 <= (uintptr_t)frames + frame_bytes) {
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(lo);
    uint32_t w[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[k] = wp[k];
    const uint32_t sh = (uint32_t)(at & 3);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint8_t* px = src + (size_t)min(x0 + e, W - 1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) d[(3 * e + c) >> 2] |= (uint32_t)px[c] << (8 * ((3 * e + c) & 3));
    }
  }
}
__device__ __forceinline__ uint32_t px8_byte(const uint32_t (&d)[6], int e, int c) { return (d[(3 * e + c) >> 2] >> (8 * ((3 * e + c) & 3))) & 0xFFu; }

template <typename T>
__global__ __launch_bounds__(256) void k_video_tiles(const uint8_t* __restrict__ frames, size_t frame_bytes, T* __restrict__ out,
                                                     const VideoGeo g, int tile_begin, uint32_t groups_per_tile, uint32_t blocks_per_tile) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t gi = (blockIdx.x - local * blocks_per_tile) * 256u + threadIdx.x;      // group of 8 pixels inside the tile
  // The 256 values a byte can take, each formed by the shared expression (the same bits), then looked up: a correctly rounded
  // division is some 15 instructions, and 24 of them per thread would make this kernel compute-bound.
  __shared__ float unit[256];
  unit[threadIdx.x] = ttv_unit_from_u8(threadIdx.x);
  __syncthreads();
  if (gi >= groups_per_tile) return;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const uint32_t per_row = (uint32_t)Wt / 8u;
  const uint32_t row = gi / per_row, xg = gi - row * per_row;
  const int i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  const int x0 = o.w0 + (int)xg * 8;
  const uint8_t* src = frames + source_row(g, o, i, y);
  uint32_t d[6];                                                  // the 24 bytes of pixels x0 .. x0 + 7, in place
  const uintptr_t at = (uintptr_t)(src + (size_t)x0 * 3), lo = at & ~(uintptr_t)3;
  if (x0 + 8 <= g.W && lo >= (uintptr_t)frames && lo + 28 <= (uintptr_t)frames + frame_bytes) {
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(lo);
    uint32_t w[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[k] = wp[k];
    const uint32_t sh = (uint32_t)(at & 3);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint8_t* px = src + (size_t)min(x0 + e, g.W - 1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) d[(3 * e + c) >> 2] |= (uint32_t)px[c] << (8 * ((3 * e + c) & 3));
    }
  }
  const size_t plane = (size_t)g.a[0].tile * Ht * Wt;
  T* dst = out + (size_t)local * 3 * plane + (size_t)row * Wt + (size_t)xg * 8;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = unit[(d[(3 * e + c) >> 2] >> (8 * ((3 * e + c) & 3))) & 0xFFu];
    store8<T>(dst + (size_t)c * plane, v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_video_tiles_any(const uint8_t* __restrict__ frames, T* __restrict__ out, const VideoGeo g,
                                                         int tile_begin, uint32_t pixels_per_tile, uint32_t blocks_per_tile) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t pi = (blockIdx.x - local * blocks_per_tile) * 256u + threadIdx.x;
  if (pi >= pixels_per_tile) return;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const uint32_t row = pi / (uint32_t)Wt;
  const int x = (int)(pi - row * (uint32_t)Wt), i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  const uint8_t* px = frames + source_row(g, o, i, y) + (size_t)min(o.w0 + x, g.W - 1) * 3;
  T* dst = out + (size_t)local * 3 * pixels_per_tile + pi;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[(size_t)c * pixels_per_tile] = Cvt<T>::from_f(ttv_unit_from_u8(px[c]));
}

// ---- blend ----------------------------------------------------------------------------------------------------------------
// torch's clamp(-1, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp_unit(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }
// (q + 1) * 127.5 with each step rounded on its own, then round-half-even; t < 0 -> 0, t >= 255 -> 255, NaN -> 0
__device__ __forceinline__ uint32_t frame_level(float q) {
#pragma clang fp contract(off)
  const float t = __fmul_rn(__fadd_rn(q, 1.0f), 127.5f);
  if (!(t >= 0.0f)) return 0u;
  if (t >= 255.0f) return 255u;
  return (uint32_t)rintf(t);
}

template <typename T>
__global__ __launch_bounds__(256) void k_video_blend(const T* const* __restrict__ tiles, uint8_t* __restrict__ out, const VideoGeo g,
                                                     int t_begin, uint32_t groups_per_row, long long total_groups) {
#pragma clang fp contract(off)
  const long long gidx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gidx >= total_groups) return;
  const long long row = gidx / groups_per_row;                    // (frame of the range, y)
  const int x0 = (int)(gidx - row * groups_per_row) * 4;
  const int tl = (int)(row / g.H), y = (int)(row - (long long)tl * g.H);
  const int npx = min(4, g.W - x0);
  const VideoAxis &at = g.a[0], &ah = g.a[1], &aw = g.a[2];
  const int Ht = ah.tile, Wt = aw.tile;
  const size_t plane = (size_t)at.tile * Ht * Wt;
  const int t = t_begin + tl;
  const Cover ct = axis_cover(at, t, t), ch = axis_cover(ah, y, y), cw = axis_cover(aw, x0, x0 + npx - 1);
  // The thread's four pixels share their t and y tiles and nearly always their x tiles, so a tile is visited once for all four and
  // its up to 12 elements are loaded together (one vector per channel where the four lie in the tile on a vector boundary): the
  // loads of a visit are in flight at the same time, and a visit is the unit of the dependent chain pointer -> elements.
  float num[4][3], only[4][3];
  int den[4], cnt[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    den[e] = cnt[e] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) num[e][c] = only[e][c] = 0.0f;
  }
  for (int jt = 0; jt < ct.n; ++jt) {
    const int kt = cover_tile(at, ct, jt), ut = t - axis_origin(at, kt), wt = axis_weight(at, ut);
    for (int jh = 0; jh < ch.n; ++jh) {
      const int kh = cover_tile(ah, ch, jh), uh = y - axis_origin(ah, kh), wth = wt * axis_weight(ah, uh);
      const size_t line = ((size_t)ut * Ht + uh) * Wt;
      for (int jw = 0; jw < cw.n; ++jw) {
        const int kw = cover_tile(aw, cw, jw), uw = x0 - axis_origin(aw, kw);       // local x of the first pixel, may be negative
        const T* p = tiles[((size_t)kt * ah.count + kh) * aw.count + kw];
        float v[3][4];
        bool in[4];
        if (npx == 4 && uw >= 0 && uw + 4 <= Wt && ((uw | Wt) & 3) == 0 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const f32x4 q = Vec4<T>::load(p + (size_t)c * plane + line + uw);
            v[c][0] = q[0]; v[c][1] = q[1]; v[c][2] = q[2]; v[c][3] = q[3];
          }
          in[0] = in[1] = in[2] = in[3] = true;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            in[e] = e < npx && uw + e >= 0 && uw + e < Wt;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][e] = in[e] ? Cvt<T>::to_f(p[(size_t)c * plane + line + (uw + e)]) : 0.0f;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!in[e]) continue;
          const int w = wth * axis_weight(aw, uw + e);
          den[e] += w;
          cnt[e] += 1;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            only[e][c] = clamp_unit(v[c][e]);
            num[e][c] = __fadd_rn(num[e][c], __fmul_rn((float)w, only[e][c]));
          }
        }
      }
    }
  }
  uint32_t level[12];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool one = ct.n * ch.n * cnt[e] == 1;
    const float fden = (float)den[e];
#pragma unroll
    for (int c = 0; c < 3; ++c) level[3 * e + c] = e < npx ? frame_level(one ? only[e][c] : __fdiv_rn(num[e][c], fden)) : 0u;
  }
  uint8_t* dst = out + ((size_t)row * g.W + x0) * 3;
  if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int k = 0; k < 3; ++k) dw[k] = level[4 * k] | (level[4 * k + 1] << 8) | (level[4 * k + 2] << 16) | (level[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int b = 0; b < 12; ++b)
      if (b < 3 * npx) dst[b] = (uint8_t)level[b];
  }
}

// ---- per-tile squared error against the source ------------------------------------------------------------------------------
// 8 consecutive elements of a reconstructed tile: one (bf16) or two (fp32) 16-byte vectors where the tile lies on the 16-byte grid
// (rows and planes are multiples of 8 elements), single elements under any other pointer.
template <typename T> __device__ __forceinline__ void load8(const T* __restrict__ p, bool vec, float (&v)[8]);
template <> __device__ __forceinline__ void load8<float>(const float* __restrict__ p, bool vec, float (&v)[8]) {
  if (vec) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = p[e];
  }
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* __restrict__ p, bool vec, float (&v)[8]) {
  if (vec) {
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)b[e];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)p[e];
  }
}

// frame_level(clamp_unit(v)) as a float, without a branch: a NaN of any kind is replaced by -1, whose level is 0 (a select, not the
// NaN rule of min / max: a widened bf16 may be a signalling NaN, which those return as a NaN); everything else is clamped to [-1, 1] as
// clamp_unit does, and then t lies in [0, 255], where frame_level is round-half-even(t).  (frame_level's three exits are divergent
// branches per element in a kernel that forms 24 levels per thread.)
__device__ __forceinline__ float tile_level(float v) {
#pragma clang fp contract(off)
  const float w = v != v ? -1.0f : v;
  const float q = fminf(fmaxf(w, -1.0f), 1.0f);
  return rintf(__fmul_rn(__fadd_rn(q, 1.0f), 127.5f));
}
// acc + (level(recon) - level)^2 in fp32: integers below 2^24 all the way (a thread adds at most 24 x 65025), so exact.
__device__ __forceinline__ float add_sq_diff(float acc, float recon, uint32_t level) {
#pragma clang fp contract(off)
  const float d = __fsub_rn(tile_level(recon), (float)level);
  return __fmaf_rn(d, d, acc);
}

// A thread takes TTV_SSE_ITERS items of its block's span (8 pixels each in k_video_tile_sse, one in the _any kernel), 256 items apart,
// so a block covers 256 * TTV_SSE_ITERS items of one tile and ends in ONE atomic: all the sums of a call lie in a few cache lines, and
// atomics on one line are served one after the other (the 64 x 256 x 256 video in bf16 takes 49 us with one
// item per thread = 5760 atomics, 27 us with four or eight).  8 keeps the block's partial in 32 bits: 256 * 8 * 24 * 65025 < 2^32.
#ifndef TTV_SSE_ITERS
#define TTV_SSE_ITERS 8
#endif
static_assert(TTV_SSE_ITERS >= 1 && 256ull * TTV_SSE_ITERS * 24 * 65025 < (1ull << 32), "a block's partial sum must fit 32 bits");

// A block's threads (all 256 of them, none may have left) each bring a partial of at most TTV_SSE_ITERS * 24 * 65025; their sum,
// below 2^32, is added to *dst by one 64-bit atomic of thread 0.  Integer addition: the order of the blocks changes no bit.
__device__ __forceinline__ void block_add_u64(uint32_t part, unsigned long long* dst) {
  __shared__ uint32_t wave_part[4];
  part = wave_sum_u32(part);
  if ((threadIdx.x & 63u) == 0) wave_part[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = wave_part[0] + wave_part[1] + wave_part[2] + wave_part[3];
    if (total) atomicAdd(dst, (unsigned long long)total);
  }
}

// k_video_tile_sse<T>     : k_video_tiles' geometry (Wt % 8 == 0, a thread owns 8 pixels of a tile row at a time, the same source
//                           load) with the tile read in place of written; rows and columns the tile holds beyond a short axis are
//                           not counted.
// k_video_tile_sse_any<T> : any Wt, a pixel of a tile at a time.
template <typename T>
__global__ __launch_bounds__(256) void k_video_tile_sse(const uint8_t* __restrict__ frames, size_t frame_bytes, const T* const* __restrict__ recon,
                                                        const VideoGeo g, int tile_begin, uint32_t groups_per_tile, uint32_t blocks_per_tile,
                                                        unsigned long long* __restrict__ sse) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t first = (blockIdx.x - local * blocks_per_tile) * (256u * TTV_SSE_ITERS) + threadIdx.x;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const uint32_t per_row = (uint32_t)Wt / 8u;
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  const T* p = recon[local];
  const bool vec = ((uintptr_t)p & 15) == 0;
  const size_t plane = (size_t)g.a[0].tile * Ht * Wt;
  uint32_t part = 0;
#pragma unroll 2
  for (int it = 0; it < TTV_SSE_ITERS; ++it) {
    const uint32_t gi = first + (uint32_t)it * 256u;                // group of 8 pixels inside the tile
    if (gi >= groups_per_tile) break;
    const uint32_t row = gi / per_row, xg = gi - row * per_row;
    const int i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
    const int x0 = o.w0 + (int)xg * 8;
    if (o.t0 + i >= g.a[0].n || o.h0 + y >= g.H || x0 >= g.W) continue;
    const T* q = p + (size_t)row * Wt + (size_t)xg * 8;
    float v[3][8];
#pragma unroll
    for (int c = 0; c < 3; ++c) load8<T>(q + (size_t)c * plane, vec, v[c]);
    uint32_t d[6];
    source_px8(frames, frame_bytes, frames + source_row(g, o, i, y), x0, g.W, d);
    const int npx = g.W - x0;                                     // pixels of the eight that the video holds, when below 8
    float acc = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) s = add_sq_diff(s, v[c][e], px8_byte(d, e, c));
      acc += e < npx ? s : 0.0f;
    }
    part += (uint32_t)acc;
  }
  block_add_u64(part, sse + local);
}

template <typename T>
__global__ __launch_bounds__(256) void k_video_tile_sse_any(const uint8_t* __restrict__ frames, const T* const* __restrict__ recon, const VideoGeo g,
                                                            int tile_begin, uint32_t pixels_per_tile, uint32_t blocks_per_tile,
                                                            unsigned long long* __restrict__ sse) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t first = (blockIdx.x - local * blocks_per_tile) * (256u * TTV_SSE_ITERS) + threadIdx.x;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  const T* p = recon[local];
  uint32_t part = 0;
  for (int it = 0; it < TTV_SSE_ITERS; ++it) {
    const uint32_t pi = first + (uint32_t)it * 256u;
    if (pi >= pixels_per_tile) break;
    const uint32_t row = pi / (uint32_t)Wt;
    const int x = (int)(pi - row * (uint32_t)Wt), i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
    if (o.t0 + i >= g.a[0].n || o.h0 + y >= g.H || o.w0 + x >= g.W) continue;
    const uint8_t* px = frames + source_row(g, o, i, y) + (size_t)(o.w0 + x) * 3;
    const T* q = p + pi;
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc = add_sq_diff(acc, Cvt<T>::to_f(q[(size_t)c * pixels_per_tile]), px[c]);
    part += (uint32_t)acc;
  }
  block_add_u64(part, sse + local);
}

// ---- Y'CbCr 4:2:0 frames in and out (ttv_yuv420) ----------------------------------------------------------------------------------
// include/titok_hip.h defines every value on integers; the kernels below restate it.  Kernels
//   k_video_tiles_yuv<T>      : k_video_tiles' geometry (Wt % 8 == 0, a thread owns 8 pixels of a tile row).  The 8 luma bytes come
//                               from the 3 aligned words that hold them; the chroma the 8 pixels need lies in 6 consecutive chroma
//                               columns of 2 rows, which the thread loads once per plane (24 byte loads), combines along y, and then
//                               along x with weights that depend on the column's parity only - uniform over a block, so the parity of
//                               the tile's origin is a template argument and every index is a constant.  The division by 255 * 2^15 is
//                               a multiplication by the reciprocal and one fused correction (unit_from_n).  Clamped columns (W shorter
//                               than the tile) and words that would leave the plane go pixel by pixel (yuv_pixel).
//   k_video_tiles_yuv_any<T>  : any Wt, a thread per pixel.
//   k_video_tile_sse_yuv<T>, k_video_tile_sse_yuv_any<T> : k_video_tile_sse with the source level (N + 32768) >> 16.
//   k_video_blend_yuv<T, XT>  : a thread owns 4 pixels of one output row, as in k_video_blend, and blends them the same way (one
//                               tile visit for the four); it stores 4 luma bytes.  A block holds both rows of a row pair: through LDS
//                               a thread gets the last column of the thread to its left (TTV_YUV_LEFT reads column 2i - 1) and the
//                               other row's share of the chroma sums; the thread of the upper row finishes the group's first
//                               chroma sample, the thread of the lower row the second.  3 KiB of LDS, two barriers.
struct YuvCoef {
  int32_t y0, ky16, rv, gu, gv, bu;                        // to RGB: ky16 = 16 ky
  int32_t yr, yg, yb, ur, ug, ub, vr, vg, vb;              // from RGB
  int32_t y_lo, y_hi, c_lo, c_hi;                          // the legal levels of the range
};
struct YuvFrames {
  uint8_t *y, *u, *v;
  int64_t y_frame, c_frame;
  int32_t y_pitch, c_pitch, c_step, c_shift, Hc, Wc, center;      // c_step = 1 << c_shift
  size_t y_bytes;                                          // from y to one past the last luma sample of the last frame
  YuvCoef k;
};

constexpr int32_t kNMax = 255 * 65536;

// The two chroma samples of an axis that luma position p reads, clamped to the plane, and their weights (sum 4).
__device__ __forceinline__ void chroma_taps(int p, int n, bool center, int& a, int& b, int& wa, int& wb) {
  const int j = p >> 1;
  if (p & 1) { a = j; b = j + 1; wa = center ? 3 : 2; wb = center ? 1 : 2; }
  else       { a = j - 1; b = j; wa = center ? 1 : 0; wb = center ? 3 : 4; }
  a = max(a, 0);
  b = min(b, n - 1);
}
__device__ __forceinline__ void yuv_to_n(const YuvCoef& k, int Y, int U16, int V16, int (&N)[3]) {
  // every factor fits 24 bits (16 ky < 2^17, the coefficients < 2^14, |u|, |v| <= 2048): full-rate multiplies, the same integers
  const int yc = __mul24(k.ky16, Y - k.y0), u = U16 - 2048, v = V16 - 2048;
  N[0] = min(max(yc + __mul24(k.rv, v), 0), kNMax);
  N[1] = min(max(yc + __mul24(k.gu, u) + __mul24(k.gv, v), 0), kNMax);
  N[2] = min(max(yc + __mul24(k.bu, u), 0), kNMax);
}
// N of the pixel (frame ts, row ys, column xs), all inside the picture
__device__ __forceinline__ void yuv_pixel(const YuvFrames& s, int ts, int ys, int xs, int (&N)[3]) {
  int ra, rb, wra, wrb, ca, cb, wca, wcb;
  chroma_taps(ys, s.Hc, true, ra, rb, wra, wrb);
  chroma_taps(xs, s.Wc, s.center != 0, ca, cb, wca, wcb);
  const size_t f = (size_t)ts * s.c_frame, oa = f + (size_t)ra * s.c_pitch, ob = f + (size_t)rb * s.c_pitch;
  const int xa = ca << s.c_shift, xb = cb << s.c_shift;
  const int U16 = __mul24(wra, __mul24(wca, s.u[oa + xa]) + __mul24(wcb, s.u[oa + xb])) + __mul24(wrb, __mul24(wca, s.u[ob + xa]) + __mul24(wcb, s.u[ob + xb]));
  const int V16 = __mul24(wra, __mul24(wca, s.v[oa + xa]) + __mul24(wcb, s.v[oa + xb])) + __mul24(wrb, __mul24(wca, s.v[ob + xa]) + __mul24(wcb, s.v[ob + xb]));
  yuv_to_n(s.k, s.y[(size_t)ts * s.y_frame + (size_t)ys * s.y_pitch + xs], U16, V16, N);
}

// Pixels x0 .. x0 + 7 (all inside the row) of frame ts, row ys, with P = x0 & 1.  Relative to chroma column (x0 >> 1) - 1, pixel e
// reads columns a and a + 1 with a = ((P + e) >> 1) + ((P + e) & 1): an even column its own sample and the one before, an odd one its
// own and the one after; six columns hold them all.
template <int P>
__device__ __forceinline__ void yuv_px8(const YuvFrames& s, int ts, int ys, int x0, const uint32_t (&yw)[2], int (&N)[8][3]) {
  int ra, rb, wra, wrb;
  chroma_taps(ys, s.Hc, true, ra, rb, wra, wrb);
  const size_t f = (size_t)ts * s.c_frame, oa = f + (size_t)ra * s.c_pitch, ob = f + (size_t)rb * s.c_pitch;
  const int c_lo = (x0 >> 1) - 1;
  int U6[6], V6[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int off = min(max(c_lo + k, 0), s.Wc - 1) << s.c_shift;
    U6[k] = __mul24(wra, s.u[oa + off]) + __mul24(wrb, s.u[ob + off]);
    V6[k] = __mul24(wra, s.v[oa + off]) + __mul24(wrb, s.v[ob + off]);
  }
  const int e_a = s.center ? 1 : 0, e_b = 4 - e_a, o_a = s.center ? 3 : 2, o_b = 4 - o_a;      // weights of an even and an odd column
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int q = (P + e) & 1, a = ((P + e) >> 1) + q;
    const int wa = q ? o_a : e_a, wb = q ? o_b : e_b;
    const int Y = (int)((yw[e >> 2] >> (8 * (e & 3))) & 0xFFu);
    yuv_to_n(s.k, Y, __mul24(wa, U6[a]) + __mul24(wb, U6[a + 1]), __mul24(wa, V6[a]) + __mul24(wb, V6[a + 1]), N[e]);
  }
}
// N of the 8 pixels min(x0 + e, W - 1) of tile row (frame ts, row ys): the word path where the eight are inside the row and the
// three aligned words that hold their luma are inside the planes' extent, pixel by pixel elsewhere.
__device__ __forceinline__ void yuv_row8(const YuvFrames& s, int ts, int ys, int x0, int W, int (&N)[8][3]) {
  const uint8_t* yp = s.y + (size_t)ts * s.y_frame + (size_t)ys * s.y_pitch + x0;
  const uintptr_t at = (uintptr_t)yp, lo = at & ~(uintptr_t)3;
  if (x0 + 8 <= W && lo >= (uintptr_t)s.y && lo + 12 <= (uintptr_t)s.y + s.y_bytes) {
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(lo);
    const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2], sh = (uint32_t)(at & 3);
    const uint32_t yw[2] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh)};
    if (x0 & 1) yuv_px8<1>(s, ts, ys, x0, yw, N);
    else yuv_px8<0>(s, ts, ys, x0, yw, N);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) yuv_pixel(s, ts, ys, min(x0 + e, W - 1), N[e]);
  }
}

// float(N) / 8355840.0f - 1.0f with the division correctly rounded: q0 = N * rc, r = N - q0 * d exactly (one fused operation),
// q = q0 + r * rc.  With rc the correctly rounded reciprocal of d = 255 * 2^15 and N an integer of at most 24 bits this is the
// correctly rounded quotient for every N in 0 .. 255 * 2^16 (all 16 711 681 of them were compared with the division on the host).
__device__ __forceinline__ float unit_from_n(int n) {
  const float d = 8355840.0f, rc = 1.0f / 8355840.0f, a = (float)n;
  const float q0 = __fmul_rn(a, rc);
  const float q = __fmaf_rn(__fmaf_rn(-q0, d, a), rc, q0);
  return __fsub_rn(q, 1.0f);
}
__device__ __forceinline__ uint32_t level_from_n(int n) { return (uint32_t)(n + 32768) >> 16; }

template <typename T>
__global__ __launch_bounds__(256) void k_video_tiles_yuv(const YuvFrames s, T* __restrict__ out, const VideoGeo g, int tile_begin,
                                                         uint32_t groups_per_tile, uint32_t blocks_per_tile) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t gi = (blockIdx.x - local * blocks_per_tile) * 256u + threadIdx.x;
  if (gi >= groups_per_tile) return;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const uint32_t per_row = (uint32_t)Wt / 8u;
  const uint32_t row = gi / per_row, xg = gi - row * per_row;
  const int i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  int N[8][3];
  yuv_row8(s, g.frame_stride * min(o.t0 + i, g.a[0].n - 1), min(o.h0 + y, g.H - 1), o.w0 + (int)xg * 8, g.W, N);
  const size_t plane = (size_t)g.a[0].tile * Ht * Wt;
  T* dst = out + (size_t)local * 3 * plane + (size_t)row * Wt + (size_t)xg * 8;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = unit_from_n(N[e][c]);
    store8<T>(dst + (size_t)c * plane, v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_video_tiles_yuv_any(const YuvFrames s, T* __restrict__ out, const VideoGeo g, int tile_begin,
                                                             uint32_t pixels_per_tile, uint32_t blocks_per_tile) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t pi = (blockIdx.x - local * blocks_per_tile) * 256u + threadIdx.x;
  if (pi >= pixels_per_tile) return;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const uint32_t row = pi / (uint32_t)Wt;
  const int x = (int)(pi - row * (uint32_t)Wt), i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  int N[3];
  yuv_pixel(s, g.frame_stride * min(o.t0 + i, g.a[0].n - 1), min(o.h0 + y, g.H - 1), min(o.w0 + x, g.W - 1), N);
  T* dst = out + (size_t)local * 3 * pixels_per_tile + pi;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[(size_t)c * pixels_per_tile] = Cvt<T>::from_f(unit_from_n(N[c]));
}

template <typename T>
__global__ __launch_bounds__(256) void k_video_tile_sse_yuv(const YuvFrames s, const T* const* __restrict__ recon, const VideoGeo g, int tile_begin,
                                                            uint32_t groups_per_tile, uint32_t blocks_per_tile, unsigned long long* __restrict__ sse) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t first = (blockIdx.x - local * blocks_per_tile) * (256u * TTV_SSE_ITERS) + threadIdx.x;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const uint32_t per_row = (uint32_t)Wt / 8u;
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  const T* p = recon[local];
  const bool vec = ((uintptr_t)p & 15) == 0;
  const size_t plane = (size_t)g.a[0].tile * Ht * Wt;
  uint32_t part = 0;
  for (int it = 0; it < TTV_SSE_ITERS; ++it) {
    const uint32_t gi = first + (uint32_t)it * 256u;
    if (gi >= groups_per_tile) break;
    const uint32_t row = gi / per_row, xg = gi - row * per_row;
    const int i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
    const int x0 = o.w0 + (int)xg * 8;
    if (o.t0 + i >= g.a[0].n || o.h0 + y >= g.H || x0 >= g.W) continue;
    const T* q = p + (size_t)row * Wt + (size_t)xg * 8;
    float v[3][8];
#pragma unroll
    for (int c = 0; c < 3; ++c) load8<T>(q + (size_t)c * plane, vec, v[c]);
    int N[8][3];
    yuv_row8(s, g.frame_stride * (o.t0 + i), o.h0 + y, x0, g.W, N);
    const int npx = g.W - x0;
    float acc = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float sq = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) sq = add_sq_diff(sq, v[c][e], level_from_n(N[e][c]));
      acc += e < npx ? sq : 0.0f;
    }
    part += (uint32_t)acc;
  }
  block_add_u64(part, sse + local);
}

template <typename T>
__global__ __launch_bounds__(256) void k_video_tile_sse_yuv_any(const YuvFrames s, const T* const* __restrict__ recon, const VideoGeo g,
                                                                int tile_begin, uint32_t pixels_per_tile, uint32_t blocks_per_tile,
                                                                unsigned long long* __restrict__ sse) {
  const uint32_t local = blockIdx.x / blocks_per_tile;
  const uint32_t first = (blockIdx.x - local * blocks_per_tile) * (256u * TTV_SSE_ITERS) + threadIdx.x;
  const int Ht = g.a[1].tile, Wt = g.a[2].tile;
  const TileAt o = tile_origin(g, tile_begin + (int)local);
  const T* p = recon[local];
  uint32_t part = 0;
  for (int it = 0; it < TTV_SSE_ITERS; ++it) {
    const uint32_t pi = first + (uint32_t)it * 256u;
    if (pi >= pixels_per_tile) break;
    const uint32_t row = pi / (uint32_t)Wt;
    const int x = (int)(pi - row * (uint32_t)Wt), i = (int)(row / (uint32_t)Ht), y = (int)(row - (uint32_t)i * (uint32_t)Ht);
    if (o.t0 + i >= g.a[0].n || o.h0 + y >= g.H || o.w0 + x >= g.W) continue;
    int N[3];
    yuv_pixel(s, g.frame_stride * (o.t0 + i), o.h0 + y, o.w0 + x, N);
    const T* q = p + pi;
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc = add_sq_diff(acc, Cvt<T>::to_f(q[(size_t)c * pixels_per_tile]), level_from_n(N[c]));
    part += (uint32_t)acc;
  }
  block_add_u64(part, sse + local);
}

// The levels ttv_video_blend_u8 defines for pixels x0 .. x0 + npx - 1 (npx <= 4) of row y of timeline frame t: k_video_blend's walk -
// one visit per covering tile for all four pixels, sums in ascending tile index - as a function (that kernel keeps its own lines: its
// code is held as it was measured).  level[e][c]; entries at e >= npx are 0.
template <typename T>
__device__ __forceinline__ void blend_levels4(const T* const* __restrict__ tiles, const VideoGeo& g, int t, int y, int x0, int npx,
                                              uint32_t (&level)[4][3]) {
#pragma clang fp contract(off)
  const VideoAxis &at = g.a[0], &ah = g.a[1], &aw = g.a[2];
  const int Ht = ah.tile, Wt = aw.tile;
  const size_t plane = (size_t)at.tile * Ht * Wt;
  const Cover ct = axis_cover(at, t, t), ch = axis_cover(ah, y, y), cw = axis_cover(aw, x0, x0 + npx - 1);
  float num[4][3], only[4][3];
  int den[4], cnt[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    den[e] = cnt[e] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) num[e][c] = only[e][c] = 0.0f;
  }
  for (int jt = 0; jt < ct.n; ++jt) {
    const int kt = cover_tile(at, ct, jt), ut = t - axis_origin(at, kt), wt = axis_weight(at, ut);
    for (int jh = 0; jh < ch.n; ++jh) {
      const int kh = cover_tile(ah, ch, jh), uh = y - axis_origin(ah, kh), wth = wt * axis_weight(ah, uh);
      const size_t line = ((size_t)ut * Ht + uh) * Wt;
      for (int jw = 0; jw < cw.n; ++jw) {
        const int kw = cover_tile(aw, cw, jw), uw = x0 - axis_origin(aw, kw);
        const T* p = tiles[((size_t)kt * ah.count + kh) * aw.count + kw];
        float v[3][4];
        bool in[4];
        if (npx == 4 && uw >= 0 && uw + 4 <= Wt && ((uw | Wt) & 3) == 0 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const f32x4 q = Vec4<T>::load(p + (size_t)c * plane + line + uw);
            v[c][0] = q[0]; v[c][1] = q[1]; v[c][2] = q[2]; v[c][3] = q[3];
          }
          in[0] = in[1] = in[2] = in[3] = true;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            in[e] = e < npx && uw + e >= 0 && uw + e < Wt;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][e] = in[e] ? Cvt<T>::to_f(p[(size_t)c * plane + line + (uw + e)]) : 0.0f;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!in[e]) continue;
          const int w = wth * axis_weight(aw, uw + e);
          den[e] += w;
          cnt[e] += 1;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            only[e][c] = clamp_unit(v[c][e]);
            num[e][c] = __fadd_rn(num[e][c], __fmul_rn((float)w, only[e][c]));
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool one = ct.n * ch.n * cnt[e] == 1;
    const float fden = (float)den[e];
#pragma unroll
    for (int c = 0; c < 3; ++c) level[e][c] = e < npx ? frame_level(one ? only[e][c] : __fdiv_rn(num[e][c], fden)) : 0u;
  }
}

// A block is XT threads along x times 256 / XT rows (XT = 64: two row pairs, XT = 128: one); a thread owns 4 pixels of one row.
// Where a row needs several blocks (ovl = 1) a block's first thread is a helper: it blends the group left of the block's own for
// the sake of its last column and stores nothing, so no thread blends a pixel on its own.
template <typename T, int XT>
__global__ __launch_bounds__(256) void k_video_blend_yuv(const T* const* __restrict__ tiles, const YuvFrames s, const VideoGeo g, int t_begin,
                                                         uint32_t x_blocks, uint32_t row_pairs, int ovl) {
  constexpr int PAIRS = 128 / XT;                                 // row pairs of a block
  __shared__ uint32_t last[256], part[2][256];
  const int tid = (int)threadIdx.x, tx = tid % XT, ry = tid / XT, r = ry & 1;
  const uint32_t bx = blockIdx.x % x_blocks, rp = (blockIdx.x / x_blocks) * PAIRS + (uint32_t)(ry >> 1);   // rp: (frame of the range, chroma row)
  const int group = (int)bx * (XT - ovl) + tx - ovl, x0 = group * 4;
  const int tl = (int)(rp / (uint32_t)s.Hc), j = (int)(rp - (uint32_t)tl * (uint32_t)s.Hc);
  const int y = 2 * j + r, npx = min(4, g.W - x0);
  const bool active = rp < row_pairs && y < g.H && group >= 0 && x0 < g.W;
  const bool owner = active && !(ovl && tx == 0);                 // stores what it blends
  const YuvCoef& k = s.k;
  const bool left = !s.center;
  uint32_t L[4][3] = {};
  if (active) {
    blend_levels4<T>(tiles, g, t_begin + tl, y, x0, npx, L);
    last[tid] = L[3][0] | (L[3][1] << 8) | (L[3][2] << 16);
  }
  if (owner) {
    uint32_t Y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = k.y0 + (int)((uint32_t)(__mul24(k.yr, (int)L[e][0]) + __mul24(k.yg, (int)L[e][1]) + __mul24(k.yb, (int)L[e][2]) + 32768) >> 16);
      Y[e] = (uint32_t)min(max(v, k.y_lo), k.y_hi);
    }
    uint8_t* dst = s.y + (size_t)tl * s.y_frame + (size_t)y * s.y_pitch + x0;
    if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
      *reinterpret_cast<uint32_t*>(dst) = Y[0] | (Y[1] << 8) | (Y[2] << 16) | (Y[3] << 24);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < npx) dst[e] = (uint8_t)Y[e];
    }
  }
  __syncthreads();
  // this row's share of the two chroma sums of the group, samples x0 / 2 and x0 / 2 + 1: at most 4 x 255 each, 10 bits
  int P0[3], P1[3];
  if (owner) {
    const uint32_t before = x0 == 0 ? (L[0][0] | (L[0][1] << 8) | (L[0][2] << 16)) : last[tid - 1];      // column -1 is clamped to column 0
    const int e1 = min(1, npx - 1), e3 = min(3, npx - 1);         // columns beyond W - 1 are clamped
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int l0 = (int)L[0][c], l1 = (int)(e1 == 1 ? L[1][c] : L[0][c]), l2 = (int)L[2][c];
      const int l3 = (int)(e3 == 3 ? L[3][c] : L[2][c]);
      P0[c] = left ? (int)((before >> (8 * c)) & 0xFFu) + 2 * l0 + l1 : l0 + l1;
      P1[c] = left ? l1 + 2 * l2 + l3 : l2 + l3;
    }
    part[0][tid] = (uint32_t)(P0[0] | (P0[1] << 10) | (P0[2] << 20));
    part[1][tid] = (uint32_t)(P1[0] | (P1[1] << 10) | (P1[2] << 20));
  }
  __syncthreads();
  if (!owner) return;
  // The two rows of a pair share the work: row 0 finishes sample x0 / 2, row 1 sample x0 / 2 + 1.  A last single row of an odd H
  // stands for both rows of its pair and finishes both samples.
  const bool alone = 2 * j + 1 >= g.H;
  const int sh = left ? 19 : 18, half = left ? (8 << 15) : (4 << 15);
  const size_t co = (size_t)tl * s.c_frame + (size_t)j * s.c_pitch + (size_t)(x0 >> 1) * s.c_step;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if ((!alone && q != r) || (q == 1 && npx < 3)) continue;
    int S[3];
    const uint32_t other = alone ? 0u : part[q][tid ^ XT];
#pragma unroll
    for (int c = 0; c < 3; ++c) S[c] = alone ? 2 * (q ? P1[c] : P0[c]) : (q ? P1[c] : P0[c]) + (int)((other >> (10 * c)) & 0x3FFu);
    const int U = 128 + ((__mul24(k.ur, S[0]) + __mul24(k.ug, S[1]) + __mul24(k.ub, S[2]) + half) >> sh);        // factors below 2^17 and 2^11
    const int V = 128 + ((__mul24(k.vr, S[0]) + __mul24(k.vg, S[1]) + __mul24(k.vb, S[2]) + half) >> sh);
    s.u[co + (size_t)q * s.c_step] = (uint8_t)min(max(U, k.c_lo), k.c_hi);
    s.v[co + (size_t)q * s.c_step] = (uint8_t)min(max(V, k.c_lo), k.c_hi);
  }
}

// ---- host: the plan's rules ---------------------------------------------------------------------------------------------------
int plan_geometry(const char* what, const ttv_video_plan* p, VideoGeo* g) {
  TTV_CHECK_ARG(p != nullptr, "%s: null plan", what);
  TTV_CHECK_ARG(p->T >= 1 && p->H >= 1 && p->W >= 1 && p->frame_stride >= 1, "%s: video %d x %d x %d with frame stride %d (each at least 1)", what,
                p->T, p->H, p->W, p->frame_stride);
  const int n[3] = {(int)(((int64_t)p->T + p->frame_stride - 1) / p->frame_stride), p->H, p->W};
  int64_t elements = 1, tiles = 1, weight = 1;
  for (int k = 0; k < 3; ++k) {
    const int tile = p->tile[k], o = p->overlap[k], count = p->count[k];
    TTV_CHECK_ARG(tile >= 1 && o >= 0 && count >= 1, "%s: axis %d has tile %d, overlap %d, %d tiles", what, k, tile, o, count);
    int64_t want = 1;
    if (n[k] > tile) {
      TTV_CHECK_ARG(2 * (int64_t)o <= tile, "%s: axis %d: overlap %d is more than half the tile %d", what, k, o, tile);
      const int64_t stride = tile - o;
      want = ((int64_t)n[k] - tile + stride - 1) / stride + 1;
    }
    TTV_CHECK_ARG(count == want, "%s: axis %d of length %d with tile %d and overlap %d has %lld tiles, not %d: an origin would lie outside the timeline",
                  what, k, n[k], tile, o, (long long)want, count);
    g->a[k] = {n[k], tile, tile - o, count, o};
    elements = std::min<int64_t>(elements * tile, (int64_t)1 << 40);
    tiles = std::min<int64_t>(tiles * count, (int64_t)1 << 40);
    weight = std::min<int64_t>(weight * ((int64_t)o + 1), (int64_t)1 << 40);
  }
  TTV_CHECK_ARG(elements < ((int64_t)1 << 31) && tiles < ((int64_t)1 << 31), "%s: a tile of %lld elements or %lld tiles (each below 2^31)", what,
                (long long)elements, (long long)tiles);
  TTV_CHECK_ARG(weight < ((int64_t)1 << 24), "%s: the largest weight (overlap + 1 over the axes) is %lld, not below 2^24", what, (long long)weight);
  g->H = p->H; g->W = p->W; g->frame_stride = p->frame_stride;
  return TTV_OK;
}

// round-half-up of num / den, both positive
int64_t round_half_up(int64_t num, int64_t den) { return (2 * num + den) / (2 * den); }

// The integer coefficients include/titok_hip.h defines, from Kr and Kb in 1/10000 and the range's scales as fractions.
YuvCoef yuv_coefficients(int matrix, int range) {
  const int64_t kr = matrix == TTV_YUV_BT601 ? 2990 : 2126, kb = matrix == TTV_YUV_BT601 ? 1140 : 722, kg = 10000 - kr - kb;
  const bool lim = range == TTV_YUV_LIMITED;
  const int64_t syn = lim ? 255 : 1, syd = lim ? 219 : 1, scn = lim ? 255 : 1, scd = lim ? 224 : 1;      // sy, sc; ys = 1 / sy, cs = 1 / sc
  YuvCoef k;
  k.y0 = lim ? 16 : 0;
  k.ky16 = 16 * (int32_t)round_half_up(syn * 4096, syd);
  k.rv = (int32_t)round_half_up(2 * (10000 - kr) * scn * 4096, 10000 * scd);
  k.bu = (int32_t)round_half_up(2 * (10000 - kb) * scn * 4096, 10000 * scd);
  k.gu = -(int32_t)round_half_up(2 * (10000 - kb) * kb * scn * 4096, 10000 * kg * scd);
  k.gv = -(int32_t)round_half_up(2 * (10000 - kr) * kr * scn * 4096, 10000 * kg * scd);
  const int32_t ytot = (int32_t)round_half_up(syd * 65536, syn);
  k.yr = (int32_t)round_half_up(kr * syd * 65536, 10000 * syn);
  k.yb = (int32_t)round_half_up(kb * syd * 65536, 10000 * syn);
  k.yg = ytot - k.yr - k.yb;
  k.ub = k.vr = (int32_t)round_half_up(scd * 32768, scn);
  k.ur = -(int32_t)round_half_up(kr * scd * 65536, 2 * (10000 - kb) * scn);
  k.ug = -(k.ur + k.ub);
  k.vb = -(int32_t)round_half_up(kb * scd * 65536, 2 * (10000 - kr) * scn);
  k.vg = -(k.vr + k.vb);
  k.y_lo = k.c_lo = lim ? 16 : 0;
  k.y_hi = lim ? 235 : 255;
  k.c_hi = lim ? 240 : 255;
  return k;
}

// The checks of a frame description that holds `frames` frames of H x W, and the kernels' view of it.
int yuv_frames(const char* what, const ttv_yuv420* f, int H, int W, int64_t frames, YuvFrames* s) {
  TTV_CHECK_ARG(f != nullptr, "%s: null frame description", what);
  TTV_CHECK_ARG(f->y && f->u && f->v, "%s: a null plane", what);
  TTV_CHECK_ARG(f->c_step == 1 || f->c_step == 2, "%s: c_step %d is neither 1 (planar) nor 2 (interleaved)", what, f->c_step);
  TTV_CHECK_ARG(f->matrix == TTV_YUV_BT601 || f->matrix == TTV_YUV_BT709, "%s: matrix %d is neither TTV_YUV_BT601 nor TTV_YUV_BT709", what, f->matrix);
  TTV_CHECK_ARG(f->range == TTV_YUV_LIMITED || f->range == TTV_YUV_FULL, "%s: range %d is neither TTV_YUV_LIMITED nor TTV_YUV_FULL", what, f->range);
  TTV_CHECK_ARG(f->siting == TTV_YUV_LEFT || f->siting == TTV_YUV_CENTER, "%s: siting %d is neither TTV_YUV_LEFT nor TTV_YUV_CENTER", what, f->siting);
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int64_t c_row = (int64_t)f->c_step * (Wc - 1) + 1;          // bytes from a chroma row's first sample to its last
  TTV_CHECK_ARG(f->y_pitch >= W && f->c_pitch >= (int64_t)f->c_step * Wc, "%s: pitches %d and %d for rows of %d and %lld bytes", what, f->y_pitch,
                f->c_pitch, W, (long long)f->c_step * Wc);
  const int64_t y_min = (int64_t)(H - 1) * f->y_pitch + W, c_min = (int64_t)(Hc - 1) * f->c_pitch + c_row;
  TTV_CHECK_ARG(f->y_frame >= y_min && f->c_frame >= c_min, "%s: frame strides %lld and %lld for frames of %lld and %lld bytes", what,
                (long long)f->y_frame, (long long)f->c_frame, (long long)y_min, (long long)c_min);
  s->y = (uint8_t*)f->y; s->u = (uint8_t*)f->u; s->v = (uint8_t*)f->v;
  s->y_frame = f->y_frame; s->c_frame = f->c_frame;
  s->y_pitch = f->y_pitch; s->c_pitch = f->c_pitch; s->c_step = f->c_step; s->c_shift = f->c_step - 1;
  s->Hc = Hc; s->Wc = Wc; s->center = f->siting == TTV_YUV_CENTER;
  s->y_bytes = (size_t)((frames - 1) * f->y_frame + y_min);
  s->k = yuv_coefficients(f->matrix, f->range);
  return TTV_OK;
}

}  // namespace

extern "C" {

int ttv_video_tiles_u8(const void* frames_thwc, const ttv_video_plan* plan, int tile_begin, int tile_end, void* tiles, int dtype,
                       void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "video_tiles_u8: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  VideoGeo g;
  const int rc = plan_geometry("video_tiles_u8", plan, &g);
  if (rc != TTV_OK) return rc;
  const int64_t n_tiles = (int64_t)g.a[0].count * g.a[1].count * g.a[2].count;
  TTV_CHECK_ARG(0 <= tile_begin && tile_begin <= tile_end && tile_end <= n_tiles, "video_tiles_u8: tiles [%d, %d) of %lld", tile_begin, tile_end,
                (long long)n_tiles);
  if (tile_begin == tile_end) return TTV_OK;
  TTV_CHECK_ARG(frames_thwc && tiles, "video_tiles_u8: null pointer");
  TTV_CHECK_ARG((uintptr_t)tiles % 16 == 0, "video_tiles_u8: the tile buffer is not 16-byte aligned");
  const int64_t pixels = (int64_t)g.a[0].tile * g.a[1].tile * g.a[2].tile;
  const bool vec = g.a[2].tile % 8 == 0;
  const int64_t items = vec ? pixels / 8 : pixels;
  const int64_t per_tile = (items + 255) / 256, blocks = per_tile * (tile_end - tile_begin);
  TTV_CHECK_ARG(blocks < ((int64_t)1 << 31), "video_tiles_u8: %lld blocks in one launch (below 2^31: take a shorter tile range)", (long long)blocks);
  const size_t frame_bytes = (size_t)plan->T * plan->H * plan->W * 3;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  const uint8_t* f = (const uint8_t*)frames_thwc;
  if (dtype == TTV_BF16) {
    if (vec) hipLaunchKernelGGL((k_video_tiles<bf16_t>), grid, block, 0, s, f, frame_bytes, (bf16_t*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
    else hipLaunchKernelGGL((k_video_tiles_any<bf16_t>), grid, block, 0, s, f, (bf16_t*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
  } else {
    if (vec) hipLaunchKernelGGL((k_video_tiles<float>), grid, block, 0, s, f, frame_bytes, (float*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
    else hipLaunchKernelGGL((k_video_tiles_any<float>), grid, block, 0, s, f, (float*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
  }
  TTV_CHECK_LAUNCH("video_tiles_u8");
  return TTV_OK;
}

int ttv_video_blend_u8(void* const* tiles, void* const* tiles_dev, const ttv_video_plan* plan, int t0, int t1, int dtype, void* frames_out,
                       void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "video_blend_u8: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  VideoGeo g;
  const int rc = plan_geometry("video_blend_u8", plan, &g);
  if (rc != TTV_OK) return rc;
  TTV_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= g.a[0].n, "video_blend_u8: frames [%d, %d) of a timeline of %d", t0, t1, g.a[0].n);
  if (t0 == t1) return TTV_OK;
  TTV_CHECK_ARG(tiles && tiles_dev && frames_out, "video_blend_u8: null table or output");
  const size_t esz = dtype_bytes(dtype);
  const int64_t per_layer = (int64_t)g.a[1].count * g.a[2].count;
  for (int kt = 0; kt < g.a[0].count; ++kt) {
    const int o = axis_origin(g.a[0], kt);
    if (o >= t1 || o + g.a[0].tile <= t0) continue;              // the layer holds no frame of the range
    for (int64_t k = kt * per_layer; k < (kt + 1) * per_layer; ++k)
      TTV_CHECK_ARG(tiles[k] && (uintptr_t)tiles[k] % esz == 0, "video_blend_u8: tile %lld covers frames [%d, %d) and is %s", (long long)k, t0, t1,
                    tiles[k] ? "not aligned to its element size" : "NULL");
  }
  const uint32_t per_row = ((uint32_t)g.W + 3u) / 4u;
  const long long groups = (long long)(t1 - t0) * g.H * per_row;
  const long long blocks = (groups + 255) / 256;
  TTV_CHECK_ARG(blocks < ((long long)1 << 31), "video_blend_u8: %lld blocks in one launch (below 2^31: take a shorter frame range)", blocks);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TTV_BF16)
    hipLaunchKernelGGL((k_video_blend<bf16_t>), dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t* const*)tiles_dev, (uint8_t*)frames_out, g, t0, per_row, groups);
  else
    hipLaunchKernelGGL((k_video_blend<float>), dim3((unsigned)blocks), dim3(256), 0, s, (const float* const*)tiles_dev, (uint8_t*)frames_out, g, t0, per_row, groups);
  TTV_CHECK_LAUNCH("video_blend_u8");
  return TTV_OK;
}

int ttv_video_tile_sse_u8(const void* frames_thwc, const ttv_video_plan* plan, int tile_begin, int tile_end, void* const* recon,
                          void* const* recon_dev, int dtype, uint64_t* sse, void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "video_tile_sse_u8: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  VideoGeo g;
  const int rc = plan_geometry("video_tile_sse_u8", plan, &g);
  if (rc != TTV_OK) return rc;
  const int64_t n_tiles = (int64_t)g.a[0].count * g.a[1].count * g.a[2].count;
  TTV_CHECK_ARG(0 <= tile_begin && tile_begin <= tile_end && tile_end <= n_tiles, "video_tile_sse_u8: tiles [%d, %d) of %lld", tile_begin, tile_end,
                (long long)n_tiles);
  if (tile_begin == tile_end) return TTV_OK;
  TTV_CHECK_ARG(frames_thwc && recon && recon_dev && sse, "video_tile_sse_u8: null frames, table or sums");
  TTV_CHECK_ARG((uintptr_t)sse % 8 == 0, "video_tile_sse_u8: the sums are not 8-byte aligned");
  const size_t esz = dtype_bytes(dtype);
  const int n = tile_end - tile_begin;
  for (int j = 0; j < n; ++j)
    TTV_CHECK_ARG(recon[j] && (uintptr_t)recon[j] % esz == 0, "video_tile_sse_u8: the reconstruction of tile %d is %s", tile_begin + j,
                  recon[j] ? "not aligned to its element size" : "NULL");
  const int64_t pixels = (int64_t)g.a[0].tile * g.a[1].tile * g.a[2].tile;
  const bool vec = g.a[2].tile % 8 == 0;
  const int64_t items = vec ? pixels / 8 : pixels;
  const int64_t span = 256 * TTV_SSE_ITERS;                       // items of a tile per block
  const int64_t per_tile = (items + span - 1) / span, blocks = per_tile * n;
  TTV_CHECK_ARG(blocks < ((int64_t)1 << 31), "video_tile_sse_u8: %lld blocks in one launch (below 2^31: take a shorter tile range)", (long long)blocks);
  const size_t frame_bytes = (size_t)plan->T * plan->H * plan->W * 3;
  hipStream_t s = (hipStream_t)stream;
  // the blocks of a tile add into its sum, so it starts at zero: written, not accumulated
  const hipError_t e = hipMemsetAsync(sse, 0, (size_t)n * sizeof(uint64_t), s);
  if (e != hipSuccess) {
    ttv_set_error("video_tile_sse_u8: clearing the sums: %s", hipGetErrorString(e));
    return TTV_ERR_LAUNCH;
  }
  const dim3 grid((unsigned)blocks), block(256);
  const uint8_t* f = (const uint8_t*)frames_thwc;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(sse);
  if (dtype == TTV_BF16) {
    const bf16_t* const* r = (const bf16_t* const*)recon_dev;
    if (vec) hipLaunchKernelGGL((k_video_tile_sse<bf16_t>), grid, block, 0, s, f, frame_bytes, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
    else hipLaunchKernelGGL((k_video_tile_sse_any<bf16_t>), grid, block, 0, s, f, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
  } else {
    const float* const* r = (const float* const*)recon_dev;
    if (vec) hipLaunchKernelGGL((k_video_tile_sse<float>), grid, block, 0, s, f, frame_bytes, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
    else hipLaunchKernelGGL((k_video_tile_sse_any<float>), grid, block, 0, s, f, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
  }
  TTV_CHECK_LAUNCH("video_tile_sse_u8");
  return TTV_OK;
}

int ttv_video_tiles_yuv420(const ttv_yuv420* frames, const ttv_video_plan* plan, int tile_begin, int tile_end, void* tiles, int dtype,
                           void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "video_tiles_yuv420: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  VideoGeo g;
  const int rc = plan_geometry("video_tiles_yuv420", plan, &g);
  if (rc != TTV_OK) return rc;
  const int64_t n_tiles = (int64_t)g.a[0].count * g.a[1].count * g.a[2].count;
  TTV_CHECK_ARG(0 <= tile_begin && tile_begin <= tile_end && tile_end <= n_tiles, "video_tiles_yuv420: tiles [%d, %d) of %lld", tile_begin,
                tile_end, (long long)n_tiles);
  YuvFrames s;
  const int rf = yuv_frames("video_tiles_yuv420", frames, plan->H, plan->W, plan->T, &s);
  if (rf != TTV_OK) return rf;
  if (tile_begin == tile_end) return TTV_OK;
  TTV_CHECK_ARG(tiles, "video_tiles_yuv420: null pointer");
  TTV_CHECK_ARG((uintptr_t)tiles % 16 == 0, "video_tiles_yuv420: the tile buffer is not 16-byte aligned");
  const int64_t pixels = (int64_t)g.a[0].tile * g.a[1].tile * g.a[2].tile;
  const bool vec = g.a[2].tile % 8 == 0;
  const int64_t items = vec ? pixels / 8 : pixels;
  const int64_t per_tile = (items + 255) / 256, blocks = per_tile * (tile_end - tile_begin);
  TTV_CHECK_ARG(blocks < ((int64_t)1 << 31), "video_tiles_yuv420: %lld blocks in one launch (below 2^31: take a shorter tile range)", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  if (dtype == TTV_BF16) {
    if (vec) hipLaunchKernelGGL((k_video_tiles_yuv<bf16_t>), grid, block, 0, st, s, (bf16_t*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
    else hipLaunchKernelGGL((k_video_tiles_yuv_any<bf16_t>), grid, block, 0, st, s, (bf16_t*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
  } else {
    if (vec) hipLaunchKernelGGL((k_video_tiles_yuv<float>), grid, block, 0, st, s, (float*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
    else hipLaunchKernelGGL((k_video_tiles_yuv_any<float>), grid, block, 0, st, s, (float*)tiles, g, tile_begin, (uint32_t)items, (uint32_t)per_tile);
  }
  TTV_CHECK_LAUNCH("video_tiles_yuv420");
  return TTV_OK;
}

int ttv_video_blend_yuv420(void* const* tiles, void* const* tiles_dev, const ttv_video_plan* plan, int t0, int t1, int dtype,
                           const ttv_yuv420* frames_out, void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "video_blend_yuv420: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  VideoGeo g;
  const int rc = plan_geometry("video_blend_yuv420", plan, &g);
  if (rc != TTV_OK) return rc;
  TTV_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= g.a[0].n, "video_blend_yuv420: frames [%d, %d) of a timeline of %d", t0, t1, g.a[0].n);
  YuvFrames s;
  const int rf = yuv_frames("video_blend_yuv420", frames_out, plan->H, plan->W, std::max(t1 - t0, 1), &s);
  if (rf != TTV_OK) return rf;
  if (t0 == t1) return TTV_OK;
  TTV_CHECK_ARG(tiles && tiles_dev, "video_blend_yuv420: null table");
  const size_t esz = dtype_bytes(dtype);
  const int64_t per_layer = (int64_t)g.a[1].count * g.a[2].count;
  for (int kt = 0; kt < g.a[0].count; ++kt) {
    const int o = axis_origin(g.a[0], kt);
    if (o >= t1 || o + g.a[0].tile <= t0) continue;              // the layer holds no frame of the range
    for (int64_t k = kt * per_layer; k < (kt + 1) * per_layer; ++k)
      TTV_CHECK_ARG(tiles[k] && (uintptr_t)tiles[k] % esz == 0, "video_blend_yuv420: tile %lld covers frames [%d, %d) and is %s", (long long)k, t0,
                    t1, tiles[k] ? "not aligned to its element size" : "NULL");
  }
  // a row of at most 64 groups of 4 pixels: blocks of 64 x 4 threads, two row pairs each; wider rows: 128 x 2, and where a row takes
  // several blocks each spends its first thread on the group left of its own (k_video_blend_yuv)
  const int64_t groups = ((int64_t)g.W + 3) / 4, row_pairs = (int64_t)(t1 - t0) * s.Hc;
  const bool narrow = groups <= 64;
  const int ovl = groups > 128 ? 1 : 0;
  const int64_t x_blocks = narrow ? 1 : (groups + (128 - ovl) - 1) / (128 - ovl);
  const int64_t blocks = x_blocks * (narrow ? (row_pairs + 1) / 2 : row_pairs);
  TTV_CHECK_ARG(blocks < ((int64_t)1 << 31) && row_pairs < ((int64_t)1 << 31),
                "video_blend_yuv420: %lld blocks in one launch (below 2^31: take a shorter frame range)", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  if (dtype == TTV_BF16) {
    const bf16_t* const* td = (const bf16_t* const*)tiles_dev;
    if (narrow) hipLaunchKernelGGL((k_video_blend_yuv<bf16_t, 64>), grid, block, 0, st, td, s, g, t0, (uint32_t)x_blocks, (uint32_t)row_pairs, ovl);
    else hipLaunchKernelGGL((k_video_blend_yuv<bf16_t, 128>), grid, block, 0, st, td, s, g, t0, (uint32_t)x_blocks, (uint32_t)row_pairs, ovl);
  } else {
    const float* const* td = (const float* const*)tiles_dev;
    if (narrow) hipLaunchKernelGGL((k_video_blend_yuv<float, 64>), grid, block, 0, st, td, s, g, t0, (uint32_t)x_blocks, (uint32_t)row_pairs, ovl);
    else hipLaunchKernelGGL((k_video_blend_yuv<float, 128>), grid, block, 0, st, td, s, g, t0, (uint32_t)x_blocks, (uint32_t)row_pairs, ovl);
  }
  TTV_CHECK_LAUNCH("video_blend_yuv420");
  return TTV_OK;
}

int ttv_video_tile_sse_yuv420(const ttv_yuv420* frames, const ttv_video_plan* plan, int tile_begin, int tile_end, void* const* recon,
                              void* const* recon_dev, int dtype, uint64_t* sse, void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "video_tile_sse_yuv420: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  VideoGeo g;
  const int rc = plan_geometry("video_tile_sse_yuv420", plan, &g);
  if (rc != TTV_OK) return rc;
  const int64_t n_tiles = (int64_t)g.a[0].count * g.a[1].count * g.a[2].count;
  TTV_CHECK_ARG(0 <= tile_begin && tile_begin <= tile_end && tile_end <= n_tiles, "video_tile_sse_yuv420: tiles [%d, %d) of %lld", tile_begin,
                tile_end, (long long)n_tiles);
  YuvFrames s;
  const int rf = yuv_frames("video_tile_sse_yuv420", frames, plan->H, plan->W, plan->T, &s);
  if (rf != TTV_OK) return rf;
  if (tile_begin == tile_end) return TTV_OK;
  TTV_CHECK_ARG(recon && recon_dev && sse, "video_tile_sse_yuv420: null table or sums");
  TTV_CHECK_ARG((uintptr_t)sse % 8 == 0, "video_tile_sse_yuv420: the sums are not 8-byte aligned");
  const size_t esz = dtype_bytes(dtype);
  const int n = tile_end - tile_begin;
  for (int j = 0; j < n; ++j)
    TTV_CHECK_ARG(recon[j] && (uintptr_t)recon[j] % esz == 0, "video_tile_sse_yuv420: the reconstruction of tile %d is %s", tile_begin + j,
                  recon[j] ? "not aligned to its element size" : "NULL");
  const int64_t pixels = (int64_t)g.a[0].tile * g.a[1].tile * g.a[2].tile;
  const bool vec = g.a[2].tile % 8 == 0;
  const int64_t items = vec ? pixels / 8 : pixels;
  const int64_t span = 256 * TTV_SSE_ITERS;
  const int64_t per_tile = (items + span - 1) / span, blocks = per_tile * n;
  TTV_CHECK_ARG(blocks < ((int64_t)1 << 31), "video_tile_sse_yuv420: %lld blocks in one launch (below 2^31: take a shorter tile range)", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(sse, 0, (size_t)n * sizeof(uint64_t), st);     // written, not accumulated
  if (e != hipSuccess) {
    ttv_set_error("video_tile_sse_yuv420: clearing the sums: %s", hipGetErrorString(e));
    return TTV_ERR_LAUNCH;
  }
  const dim3 grid((unsigned)blocks), block(256);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(sse);
  if (dtype == TTV_BF16) {
    const bf16_t* const* r = (const bf16_t* const*)recon_dev;
    if (vec) hipLaunchKernelGGL((k_video_tile_sse_yuv<bf16_t>), grid, block, 0, st, s, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
    else hipLaunchKernelGGL((k_video_tile_sse_yuv_any<bf16_t>), grid, block, 0, st, s, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
  } else {
    const float* const* r = (const float* const*)recon_dev;
    if (vec) hipLaunchKernelGGL((k_video_tile_sse_yuv<float>), grid, block, 0, st, s, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
    else hipLaunchKernelGGL((k_video_tile_sse_yuv_any<float>), grid, block, 0, st, s, r, g, tile_begin, (uint32_t)items, (uint32_t)per_tile, out);
  }
  TTV_CHECK_LAUNCH("video_tile_sse_yuv420");
  return TTV_OK;
}

}  // extern "C"
