// Perceptual crop sampling of the generator step (reference model/losses/loss_module.py:59-93) and its backward: the stretch between
// the towers and the LPIPS kernels.  Per crop: one frame of a clip [3][T][H][W], the reconstruction clamped to [-1, 1], optionally
// resized (torch's upsample_bicubic2d, align_corners=False, no antialiasing: cubic_taps of ttv_common.h) to the virtual size Hr x Wr,
// and the s x s window at (oy, ox) of it.  include/titok_hip.h states the value in full.
//
// Kernels
//   k_crops_fwd : grid (tiles, crops of the launch).  A thread owns 16 bytes of one output row (8 bf16 / 4 fp32 columns) of one
//                 channel and writes them, one 16-byte store each, for the reconstruction and for the target (the taps are shared).
//                 Not resized: a copy.  Resized: rows outer, columns inner, two fmaf chains of four, fp32, one rounding to the clip
//                 dtype.  The source is read element by element (2 or 4 bytes): the window origin ox is any integer, so a source
//                 row is not 16-byte aligned in general, and the taps of neighbouring outputs overlap - the reads of a wave fall
//                 into a few cache lines it shares.  Measured at 25 crops of 128 x 128 bf16 (9.8 MB read + written): 4.9 us.
//   k_crops_bwd : one launch writes the whole gradient of every clip it is given.  A block owns BW_PIX consecutive pixels (row-major
//                 in the frame) of one frame, all three channels; its frame's crop - if any - is found in the launch's table:
//                   no crop     : zeros
//                   not resized : mask * g at (y - oy, x - ox) inside the window, zeros outside it
//                   resized     : the gather form of the transpose.  The output rows i whose clamped taps touch input row y are a
//                                 contiguous range (the tap origin floor(src) is monotonic in i; ttv_cubic_floor is the forward's own
//                                 arithmetic, so the two can not disagree), likewise columns; the thread walks rows ascending, in a
//                                 row columns ascending, taps ascending, and adds with fmaf: a fixed order, no atomics.
//                 A thread recomputes the taps of the output rows and columns it walks (2 - 6 per axis at the config's grids)
//                 rather than staging them in LDS: at 5 clips of 16 x 128 x 128 bf16 with 25 crops (7.9 MB of gradients written,
//                 4.9 MB read) the launch takes 10.4 us, against the 100 fills, 25 clamp masks and the stack / unbind copies
//                 (0.6 ms of kernel time in all) it replaces.  bf16 rows go out as 8-byte stores (4 pixels per thread).
//                 mask = 1[-1 <= x <= 1] of the reconstruction pixel (torch's clamp backward, inclusive).
// A frame is sampled at most once (the reference shuffles without replacement); the entry point refuses a table that is not so.
// The tables are kernel arguments: more crops (or clips) than one launch's table holds are split into launches here.
#include <algorithm>
#include <vector>

#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

constexpr int CR_FWD_CROPS = 48;        // crops per forward launch
constexpr int CR_BWD_SEGS = 32;         // (clip, frame range) segments per backward launch
constexpr int CR_BWD_CROPS = 48;        // crops per backward launch
constexpr int CR_MAX_DIM = 16384;
constexpr int CR_MAX_SIZE = 2048;       // what LPIPS accepts

struct FwdArgs {
  const void* recon[CR_FWD_CROPS];      // the crop's frame: channel 0 of frame f, i.e. clip + f * H * W
  const void* target[CR_FWD_CROPS];
  int32_t plane[CR_FWD_CROPS];          // T * H * W: channel stride
  int32_t H[CR_FWD_CROPS], W[CR_FWD_CROPS], Hr[CR_FWD_CROPS], Wr[CR_FWD_CROPS], oy[CR_FWD_CROPS], ox[CR_FWD_CROPS];
  void* out_recon;                      // first crop of the launch
  void* out_target;
  int32_t s;
};

// clamp to [-1, 1] as torch does it: a NaN stays a NaN
__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }

// 16 bytes of one row, one store: 4 fp32 or 8 bf16 (p is 16-byte aligned: the crops are, and size % 16 == 0)
__device__ __forceinline__ void store16(float* p, const float (&v)[4]) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void store16(bf16_t* p, const float (&v)[8]) {
  bf16x8 b;
#pragma unroll
  for (int e = 0; e < 8; ++e) b[e] = (bf16_t)v[e];
  *reinterpret_cast<bf16x8*>(p) = b;
}

template <typename T>
__global__ __launch_bounds__(256) void k_crops_fwd(const FwdArgs a) {
  constexpr int V = 16 / (int)sizeof(T);
  const int crop = blockIdx.y, s = a.s;
  const int per_row = s / V;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= 3 * s * per_row) return;
  const int c = g / (s * per_row), rem = g - c * s * per_row;
  const int i = rem / per_row, j0 = (rem - i * per_row) * V;
  const int H = a.H[crop], W = a.W[crop], Hr = a.Hr[crop], Wr = a.Wr[crop], oy = a.oy[crop], ox = a.ox[crop];
  const T* rec = reinterpret_cast<const T*>(a.recon[crop]) + (size_t)c * a.plane[crop];
  const T* trg = reinterpret_cast<const T*>(a.target[crop]) + (size_t)c * a.plane[crop];
  float vr[V], vt[V];
  if (Hr == H && Wr == W) {             // block-uniform: a crop is either resized or not
    const size_t at = (size_t)(oy + i) * W + ox + j0;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      vr[e] = clamp1(Cvt<T>::to_f(rec[at + e]));
      vt[e] = Cvt<T>::to_f(trg[at + e]);
    }
  } else {
    int iy[4];
    float wy[4];
    cubic_taps(oy + i, H, Hr, iy, wy);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      int ix[4];
      float wx[4];
      cubic_taps(ox + j0 + e, W, Wr, ix, wx);
      float ar = 0.f, at = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {     // rows outer, columns inner
        const T* rr = rec + (size_t)iy[r] * W;
        const T* tr = trg + (size_t)iy[r] * W;
        float hr = 0.f, ht = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          hr = fmaf(wx[k], clamp1(Cvt<T>::to_f(rr[ix[k]])), hr);
          ht = fmaf(wx[k], Cvt<T>::to_f(tr[ix[k]]), ht);
        }
        ar = fmaf(wy[r], hr, ar);
        at = fmaf(wy[r], ht, at);
      }
      vr[e] = ar;
      vt[e] = at;
    }
  }
  const size_t o = (((size_t)crop * 3 + c) * s + i) * s + j0;
  T* orec = reinterpret_cast<T*>(a.out_recon) + o;
  T* otrg = reinterpret_cast<T*>(a.out_target) + o;
  store16(orec, vr);
  store16(otrg, vt);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
constexpr int BW_NP = 4;                 // consecutive pixels per thread
constexpr int BW_PIX = 256 * BW_NP;      // pixels per block

struct BwdArgs {
  const void* x[CR_BWD_SEGS];            // the reconstruction clip (for the clamp mask)
  void* dx[CR_BWD_SEGS];                 // its gradient
  int32_t T[CR_BWD_SEGS], H[CR_BWD_SEGS], W[CR_BWD_SEGS];
  int32_t f0[CR_BWD_SEGS];               // first frame of the segment
  int32_t block0[CR_BWD_SEGS + 1];       // first block of each segment; block0[n_seg] = blocks of the launch
  int32_t n_seg, n_crops;
  int32_t c_seg[CR_BWD_CROPS], c_frame[CR_BWD_CROPS], c_index[CR_BWD_CROPS];      // c_index: the crop's position in g
  int32_t c_Hr[CR_BWD_CROPS], c_Wr[CR_BWD_CROPS], c_oy[CR_BWD_CROPS], c_ox[CR_BWD_CROPS];
  const void* g;                         // [n][3][s][s]
  int32_t s;
};

// The outputs lo .. hi of an axis n_in -> n_out whose clamped taps can touch input x: floor(src) in [x - 2, x + 1], and everything
// below at x == 0, everything above at x == n_in - 1 (the border clamps).  floor(src) is monotonic in the output index, so an
// estimate from the inverse map is walked to the exact ends with the forward's own arithmetic.
__device__ __forceinline__ int touch_lo(int x, int n_in, int n_out, float scale) {
  if (x <= 0) return 0;
  int lo = (int)floorf(((float)x - 1.5f) / scale - 0.5f);
  lo = min(max(lo, 0), n_out - 1);
  while (lo > 0 && ttv_cubic_floor(lo - 1, scale) >= x - 2) --lo;
  while (lo < n_out && ttv_cubic_floor(lo, scale) < x - 2) ++lo;
  return lo;
}
__device__ __forceinline__ int touch_hi(int x, int n_in, int n_out, float scale) {
  if (x >= n_in - 1) return n_out - 1;
  int hi = (int)floorf(((float)x + 2.5f) / scale - 0.5f);
  hi = min(max(hi, 0), n_out - 1);
  while (hi < n_out - 1 && ttv_cubic_floor(hi + 1, scale) <= x + 1) ++hi;
  while (hi >= 0 && ttv_cubic_floor(hi, scale) > x + 1) --hi;
  return hi;
}

// R^T g at the NP pixels (y, x) .. (y, x + NP - 1) of a resized frame, all three channels
template <typename T, int NP>
__device__ __forceinline__ void gather(const T* __restrict__ g, int s, int H, int W, int Hr, int Wr, int oy, int ox, int y, int x,
                                       float (&acc)[NP][3]) {
  const float sy = (float)H / (float)Hr, sx = (float)W / (float)Wr;
  const int ilo = max(touch_lo(y, H, Hr, sy), oy), ihi = min(touch_hi(y, H, Hr, sy), oy + s - 1);
  const int jlo = max(touch_lo(x, W, Wr, sx), ox), jhi = min(touch_hi(x + NP - 1, W, Wr, sx), ox + s - 1);
  const size_t plane = (size_t)s * s;
  for (int i = ilo; i <= ihi; ++i) {
    int iy[4];
    float wy[4];
    cubic_taps(i, H, Hr, iy, wy);
    float row[NP][3];
#pragma unroll
    for (int e = 0; e < NP; ++e) row[e][0] = row[e][1] = row[e][2] = 0.f;
    const T* grow = g + (size_t)(i - oy) * s;
    for (int j = jlo; j <= jhi; ++j) {
      int ix[4];
      float wx[4];
      cubic_taps(j, W, Wr, ix, wx);
      const int jj = j - ox;
      const float g0 = Cvt<T>::to_f(grow[jj]), g1 = Cvt<T>::to_f(grow[plane + jj]), g2 = Cvt<T>::to_f(grow[2 * plane + jj]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < NP; ++e)
          if (ix[k] == x + e) {
            row[e][0] = fmaf(wx[k], g0, row[e][0]);
            row[e][1] = fmaf(wx[k], g1, row[e][1]);
            row[e][2] = fmaf(wx[k], g2, row[e][2]);
          }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (iy[k] == y) {
#pragma unroll
        for (int e = 0; e < NP; ++e)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[e][c] = fmaf(wy[k], row[e][c], acc[e][c]);
      }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_crops_bwd(const BwdArgs a) {
  int seg = 0;
  for (int k = 1; k < a.n_seg; ++k)
    if (a.block0[k] <= (int)blockIdx.x) seg = k;
  const int Tn = a.T[seg], H = a.H[seg], W = a.W[seg];
  const int hw = H * W;
  const int tiles = (hw + BW_PIX - 1) / BW_PIX;
  const int b = (int)blockIdx.x - a.block0[seg];
  const int frame = a.f0[seg] + b / tiles;
  const int p = (b % tiles) * BW_PIX + threadIdx.x * BW_NP;      // first pixel of this thread, row-major in the frame
  int ci = -1;
  for (int k = 0; k < a.n_crops; ++k)
    if (a.c_seg[k] == seg && a.c_frame[k] == frame) ci = k;
  if (p >= hw) return;
  const size_t plane = (size_t)Tn * hw;
  const size_t at = (size_t)frame * hw + p;
  T* dx = reinterpret_cast<T*>(a.dx[seg]) + at;
  const bool vec = (hw & 3) == 0;        // p % 4 == 0 and the clip is 16-byte aligned: whole vectors inside the frame
  float acc[BW_NP][3];
#pragma unroll
  for (int e = 0; e < BW_NP; ++e) acc[e][0] = acc[e][1] = acc[e][2] = 0.f;
  if (ci >= 0) {
    const int s = a.s, Hr = a.c_Hr[ci], Wr = a.c_Wr[ci], oy = a.c_oy[ci], ox = a.c_ox[ci];
    const T* g = reinterpret_cast<const T*>(a.g) + (size_t)a.c_index[ci] * 3 * s * s;
    const T* x = reinterpret_cast<const T*>(a.x[seg]) + at;
    const int y0 = p / W, x0 = p - y0 * W;
    if (Hr == H && Wr == W) {
#pragma unroll
      for (int e = 0; e < BW_NP; ++e) {
        int yy = y0, xx = x0 + e;
        if (xx >= W) { yy += xx / W; xx %= W; }
        if (p + e < hw && yy >= oy && yy < oy + s && xx >= ox && xx < ox + s) {
          const T* ge = g + (size_t)(yy - oy) * s + (xx - ox);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[e][c] = Cvt<T>::to_f(ge[(size_t)c * s * s]);
        }
      }
    } else if (x0 + BW_NP <= W) {
      gather<T, BW_NP>(g, s, H, W, Hr, Wr, oy, ox, y0, x0, acc);
    } else {                             // the thread's pixels straddle a row end (W % 4 != 0 only)
#pragma unroll
      for (int e = 0; e < BW_NP; ++e) {
        if (p + e >= hw) break;
        int yy = y0, xx = x0 + e;
        if (xx >= W) { yy += xx / W; xx %= W; }
        float one[1][3] = {{0.f, 0.f, 0.f}};
        gather<T, 1>(g, s, H, W, Hr, Wr, oy, ox, yy, xx, one);
        acc[e][0] = one[0][0]; acc[e][1] = one[0][1]; acc[e][2] = one[0][2];
      }
    }
#pragma unroll
    for (int e = 0; e < BW_NP; ++e) {
      if (p + e >= hw) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = Cvt<T>::to_f(x[(size_t)c * plane + e]);
        if (!(v >= -1.f && v <= 1.f)) acc[e][c] = 0.f;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    T* d = dx + (size_t)c * plane;
    if (vec) {
      Vec4<T>::store(d, f32x4{acc[0][c], acc[1][c], acc[2][c], acc[3][c]});
    } else {
#pragma unroll
      for (int e = 0; e < BW_NP; ++e)
        if (p + e < hw) d[e] = Cvt<T>::from_f(acc[e][c]);
    }
  }
}

struct Crop {
  int clip, frame, Hr, Wr, oy, ox, index;
};

// The checks both entry points share; fills `out` (in table order) and leaves nothing launched on a refusal.
int parse_table(const char* what, const int32_t* clip_dims, int n_clips, const int32_t* crops, int n_crops, int size, int dtype,
                std::vector<Crop>& out) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "%s: dtype %d is neither TTV_BF16 nor TTV_F32", what, dtype);
  TTV_CHECK_ARG(n_clips >= 1 && n_crops >= 1, "%s: %d clips, %d crops (at least one of each)", what, n_clips, n_crops);
  TTV_CHECK_ARG(clip_dims && crops, "%s: null argument", what);
  TTV_CHECK_ARG(size >= 16 && size <= CR_MAX_SIZE && size % 16 == 0, "%s: crop size %d (a multiple of 16, 16 .. %d)", what, size, CR_MAX_SIZE);
  TTV_CHECK_ARG((int64_t)n_crops * 3 * size * size < ((int64_t)1 << 31), "%s: %d crops of %d x %d are too many (2^31 elements)", what,
                n_crops, size, size);
  for (int i = 0; i < n_clips; ++i) {
    const int T = clip_dims[3 * i], H = clip_dims[3 * i + 1], W = clip_dims[3 * i + 2];
    TTV_CHECK_ARG(T >= 1 && H >= 1 && W >= 1 && T <= CR_MAX_DIM && H <= CR_MAX_DIM && W <= CR_MAX_DIM && (int64_t)3 * T * H * W < ((int64_t)1 << 31),
                  "%s: clip %d is %d x %d x %d (each 1 .. %d, below 2^31 elements)", what, i, T, H, W, CR_MAX_DIM);
  }
  out.resize(n_crops);
  std::vector<int64_t> keys(n_crops);
  for (int k = 0; k < n_crops; ++k) {
    const int32_t* d = crops + 8 * k;
    const int clip = d[0], frame = d[1], H = d[2], W = d[3], Hr = d[4], Wr = d[5], oy = d[6], ox = d[7];
    TTV_CHECK_ARG(clip >= 0 && clip < n_clips, "%s: crop %d names clip %d of %d", what, k, clip, n_clips);
    TTV_CHECK_ARG(frame >= 0 && frame < clip_dims[3 * clip], "%s: crop %d names frame %d of %d", what, k, frame, clip_dims[3 * clip]);
    TTV_CHECK_ARG(H == clip_dims[3 * clip + 1] && W == clip_dims[3 * clip + 2], "%s: crop %d says its frame is %d x %d, clip %d is %d x %d", what,
                  k, H, W, clip, clip_dims[3 * clip + 1], clip_dims[3 * clip + 2]);
    if (Hr != H || Wr != W) {            // resized: the short edge becomes `size`, the long edge int(size * long / short)
      const int64_t sh = std::min(H, W), lg = std::max(H, W);
      const int nl = (int)((int64_t)size * lg / sh);
      const int eh = W <= H ? nl : size, ew = W <= H ? size : nl;
      TTV_CHECK_ARG(Hr == eh && Wr == ew, "%s: crop %d: resized frame %d x %d, but the short edge of %d x %d at size %d gives %d x %d", what, k,
                    Hr, Wr, H, W, size, eh, ew);
      TTV_CHECK_ARG(Hr <= CR_MAX_DIM * 8 && Wr <= CR_MAX_DIM * 8, "%s: crop %d: resized frame %d x %d is too large", what, k, Hr, Wr);
    }
    TTV_CHECK_ARG(oy >= 0 && ox >= 0 && oy <= Hr - size && ox <= Wr - size, "%s: crop %d: window %d x %d at (%d, %d) lies outside the frame %d x %d",
                  what, k, size, size, oy, ox, Hr, Wr);
    out[k] = Crop{clip, frame, Hr, Wr, oy, ox, k};
    keys[k] = (int64_t)clip * (CR_MAX_DIM + 1) + frame;
  }
  std::sort(keys.begin(), keys.end());
  for (int k = 1; k < n_crops; ++k)
    TTV_CHECK_ARG(keys[k] != keys[k - 1], "%s: frame %d of clip %d is sampled twice (a frame is sampled at most once)", what,
                  (int)(keys[k] % (CR_MAX_DIM + 1)), (int)(keys[k] / (CR_MAX_DIM + 1)));
  return TTV_OK;
}

}  // namespace

int ttvk_lpips_crops_forward(void* const* recon, void* const* target, const int32_t* clip_dims, int n_clips, const int32_t* crops, int n_crops,
                             int size, void* recon_crops, void* target_crops, int dtype, hipStream_t s) {
  std::vector<Crop> table;
  const int rc = parse_table("lpips_crops_forward", clip_dims, n_clips, crops, n_crops, size, dtype, table);
  if (rc != TTV_OK) return rc;
  TTV_CHECK_ARG(recon && target && recon_crops && target_crops, "lpips_crops_forward: null argument");
  for (int i = 0; i < n_clips; ++i) TTV_CHECK_ARG(recon[i] && target[i], "lpips_crops_forward: null pointer in clip %d", i);
  TTV_CHECK_ARG((uintptr_t)recon_crops % 16 == 0 && (uintptr_t)target_crops % 16 == 0, "lpips_crops_forward: a destination is not 16-byte aligned");
  const size_t esz = dtype_bytes(dtype);
  const int V = 16 / (int)esz;
  const unsigned tiles = (unsigned)ttv_cdiv(3 * size * (size / V), 256);
  for (int c0 = 0; c0 < n_crops; c0 += CR_FWD_CROPS) {
    const int n = std::min(CR_FWD_CROPS, n_crops - c0);
    FwdArgs a = {};
    for (int k = 0; k < n; ++k) {
      const Crop& c = table[c0 + k];
      const int T = clip_dims[3 * c.clip], H = clip_dims[3 * c.clip + 1], W = clip_dims[3 * c.clip + 2];
      const size_t off = (size_t)c.frame * H * W * esz;
      a.recon[k] = (const char*)recon[c.clip] + off;
      a.target[k] = (const char*)target[c.clip] + off;
      a.plane[k] = T * H * W;
      a.H[k] = H; a.W[k] = W; a.Hr[k] = c.Hr; a.Wr[k] = c.Wr; a.oy[k] = c.oy; a.ox[k] = c.ox;
    }
    a.out_recon = (char*)recon_crops + (size_t)c0 * 3 * size * size * esz;
    a.out_target = (char*)target_crops + (size_t)c0 * 3 * size * size * esz;
    a.s = size;
    if (dtype == TTV_BF16) hipLaunchKernelGGL(k_crops_fwd<bf16_t>, dim3(tiles, (unsigned)n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_crops_fwd<float>, dim3(tiles, (unsigned)n), dim3(256), 0, s, a);
    TTV_CHECK_LAUNCH("lpips_crops_forward");
  }
  return TTV_OK;
}

int ttvk_lpips_crops_backward(void* const* recon, void* const* grad, const int32_t* clip_dims, int n_clips, const int32_t* crops, int n_crops,
                              int size, const void* g, int dtype, hipStream_t s) {
  std::vector<Crop> table;
  const int rc = parse_table("lpips_crops_backward", clip_dims, n_clips, crops, n_crops, size, dtype, table);
  if (rc != TTV_OK) return rc;
  TTV_CHECK_ARG(recon && grad && g, "lpips_crops_backward: null argument");
  for (int i = 0; i < n_clips; ++i) {
    TTV_CHECK_ARG(recon[i] && grad[i], "lpips_crops_backward: null pointer in clip %d", i);
    TTV_CHECK_ARG((uintptr_t)grad[i] % 16 == 0, "lpips_crops_backward: the gradient of clip %d is not 16-byte aligned", i);
  }
  std::sort(table.begin(), table.end(), [](const Crop& l, const Crop& r) { return l.clip != r.clip ? l.clip < r.clip : l.frame < r.frame; });
  // Launches of whole frames in (clip, frame) order: a segment is a frame range of one clip; a launch closes when its segment or
  // crop table is full.  Every frame of every clip lands in exactly one segment.
  BwdArgs a = {};
  int64_t blocks = 0;
  size_t next = 0;                       // first crop of `table` not yet placed
  auto flush = [&]() -> int {
    if (a.n_seg == 0) return TTV_OK;
    for (int k = a.n_seg; k <= CR_BWD_SEGS; ++k) a.block0[k] = (int32_t)blocks;
    a.g = g;
    a.s = size;
    if (dtype == TTV_BF16) hipLaunchKernelGGL(k_crops_bwd<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_crops_bwd<float>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    TTV_CHECK_LAUNCH("lpips_crops_backward");
    a = BwdArgs{};
    blocks = 0;
    return TTV_OK;
  };
  for (int clip = 0; clip < n_clips; ++clip) {
    const int T = clip_dims[3 * clip], H = clip_dims[3 * clip + 1], W = clip_dims[3 * clip + 2];
    const int tiles = ttv_cdiv(H * W, BW_PIX);
    int f = 0;
    while (f < T) {
      if (a.n_seg == CR_BWD_SEGS || a.n_crops == CR_BWD_CROPS) {
        const int rcf = flush();
        if (rcf != TTV_OK) return rcf;
      }
      // frames f .. f1 - 1: up to the frame whose crop would overflow the table, and within 2^31 blocks
      const int seg = a.n_seg;
      int f1 = f;
      size_t k = next;
      while (f1 < T && blocks + (int64_t)(f1 - f + 1) * tiles < ((int64_t)1 << 30)) {
        if (k < table.size() && table[k].clip == clip && table[k].frame == f1) {
          if (a.n_crops == CR_BWD_CROPS) break;
          const Crop& c = table[k];
          const int q = a.n_crops++;
          a.c_seg[q] = seg; a.c_frame[q] = c.frame; a.c_index[q] = c.index;
          a.c_Hr[q] = c.Hr; a.c_Wr[q] = c.Wr; a.c_oy[q] = c.oy; a.c_ox[q] = c.ox;
          ++k;
        }
        ++f1;
      }
      if (f1 == f) {                     // nothing fitted: the launch is full
        const int rcf = flush();
        if (rcf != TTV_OK) return rcf;
        continue;
      }
      next = k;
      a.x[seg] = recon[clip];
      a.dx[seg] = grad[clip];
      a.T[seg] = T; a.H[seg] = H; a.W[seg] = W; a.f0[seg] = f;
      a.block0[seg] = (int32_t)blocks;
      blocks += (int64_t)(f1 - f) * tiles;
      a.n_seg = seg + 1;
      f = f1;
    }
  }
  return flush();
}
