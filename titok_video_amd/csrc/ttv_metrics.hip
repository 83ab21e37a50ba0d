// SSIM statistic of the evaluation loop (reference model/metrics/eval_metrics.py:20-21,32-37: each clip x.clamp(-1, 1), CTHW ->
// TCHW, into torchmetrics StructuralSimilarityIndexMeasure(data_range=2) with its defaults).  That metric, per frame (= image):
//   11-tap Gaussian, sigma 1.5, g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum, 2-D window g^T g per channel;
//   C1 = (0.01 * 2)^2, C2 = (0.03 * 2)^2;  five filtered maps x, y, x^2, y^2, xy;
//   ssim = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)),  sx^2 = max(E[x^2] - mx^2, 0), sxy = E[xy] - mx my;
//   torchmetrics reflect-pads by 5, convolves 'valid' and crops 5 from every side: what it keeps are exactly the windows wholly
//   inside the frame, so the map is the valid (H - 10) x (W - 10) region of every channel and the padding never reaches it;
//   frame value = mean over C x (H - 10) x (W - 10); state = sum of frame values + frame count; compute() = sum / count
//   (a mean of per-frame means, not a pixel-weighted mean).
// Deliberate deviations: all arithmetic is fp32 for bf16 and fp32 inputs (torchmetrics under bf16 autocast convolves in bf16);
// frames with H < 11 or W < 11 are refused (torchmetrics gives NaN for 6..10 and raises for <= 5); no cross-rank sum.
//
// Launch 1, k_ssim_tiles: one workgroup per (clip, frame, 32 x 32 output tile) of the valid region, all C channels in the item.
//   Per channel the tile plus its 5-pixel halo (42 x 42) of both images is staged in LDS as fp32 (x, y) pairs, the reconstruction
//   clamped on load, 16-byte loads where the clip pointers are 16-byte aligned and W is a multiple of the vector; the horizontal
//   pass writes the five maps of 42 rows x 32 columns to LDS, the vertical pass forms the index of 4 outputs per thread.
//   Both images are filtered after subtracting one of their own pixels (the centre of the tile's first window): variance and
//   covariance do not change under a shift, and E[x^2] - mx^2 then cancels on the local spread instead of on the value (exact
//   for constant frames, where fp32 would otherwise leave sxy at a few 1e-7 against C2 = 3.6e-3).  The tile's sum (double) goes
//   to workspace slot = item.  The next channel's tile is loaded into registers while the current one is filtered.  LDS 43.4 KB:
//   three workgroups per CU.
// Launch 2, k_ssim_finish: one workgroup, a thread per frame (frames of all clips dealt round the 256 threads), sums each frame's
//   tiles in tile order, divides by C (H - 10)(W - 10), and the frame values are summed in a fixed order: acc[0] += sum,
//   acc[1] += frames.  No atomics: identical inputs give identical bits.
#include "ttv_common.h"
#include "ttv_kernels.h"

#define SS_R 5                       // window radius
#define SS_TH 32                     // output tile rows
#define SS_TW 32                     // output tile columns
#define SS_SH (SS_TH + 2 * SS_R)     // staged rows (42)
#define SS_SW (SS_TW + 2 * SS_R)     // staged columns (42)
#define SS_SP (SS_SW + 1)            // staged row pitch in (x, y) pairs: odd, so the horizontal pass's 8-byte reads are conflict-free

struct SsimClips {
  const void* recon[TTV_MAX_CLIPS_PER_LAUNCH];
  const void* target[TTV_MAX_CLIPS_PER_LAUNCH];
  int C[TTV_MAX_CLIPS_PER_LAUNCH], T[TTV_MAX_CLIPS_PER_LAUNCH], H[TTV_MAX_CLIPS_PER_LAUNCH], W[TTV_MAX_CLIPS_PER_LAUNCH];
  int item0[TTV_MAX_CLIPS_PER_LAUNCH + 1];   // first item (= workspace slot) of each clip; item0[n] = items of the call
  int frame0[TTV_MAX_CLIPS_PER_LAUNCH + 1];  // first frame of each clip; frame0[n] = frames of the call
  float g[2 * SS_R + 1];                     // Gaussian taps, fp32
};

__device__ __forceinline__ int ss_tiles_x(int W) { return (W - 2 * SS_R + SS_TW - 1) / SS_TW; }
__device__ __forceinline__ int ss_tiles_y(int H) { return (H - 2 * SS_R + SS_TH - 1) / SS_TH; }

// fixed-order sum of one double per thread over the 256 threads of the block (result in red[0], visible to every thread)
__device__ __forceinline__ double ss_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

template <typename T>
__global__ __launch_bounds__(256) void k_ssim_tiles(SsimClips a, int n_clips, int clamp, double* __restrict__ part) {
  __shared__ f32x2 sxy[SS_SH * SS_SP];   // staged (x - kx, y - ky)
  __shared__ f32x2 hm[SS_SH * SS_TW];    // horizontal pass: (x, y)
  __shared__ f32x2 hq[SS_SH * SS_TW];    //                  (x^2, y^2)
  __shared__ float hp[SS_SH * SS_TW];    //                  xy
  __shared__ double red[256];
  constexpr float C1 = 0.0004f, C2 = 0.0036f;    // (0.01 * 2)^2, (0.03 * 2)^2
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int NCH = (SS_SW + V - 1) / V;       // vector chunks per staged row

  const int item = blockIdx.x;
  int c = 0;                                      // last clip whose first item <= item (item0 strictly increasing)
  for (int step = TTV_MAX_CLIPS_PER_LAUNCH / 2; step > 0; step >>= 1)
    if (c + step < n_clips && a.item0[c + step] <= item) c += step;
  const int C = a.C[c], Tn = a.T[c], H = a.H[c], W = a.W[c];
  const int tx = ss_tiles_x(W), tiles = tx * ss_tiles_y(H);
  const int local = item - a.item0[c], t = local / tiles, tile = local - t * tiles;
  const int y0 = (tile / tx) * SS_TH, x0 = (tile % tx) * SS_TW;
  const int vh = min(SS_TH, H - 2 * SS_R - y0), vw = min(SS_TW, W - 2 * SS_R - x0);   // valid outputs of this tile
  const T* rb = reinterpret_cast<const T*>(a.recon[c]);
  const T* tb = reinterpret_cast<const T*>(a.target[c]);
  const bool vec_ok = ((((uintptr_t)rb | (uintptr_t)tb) & 15) == 0) && W % V == 0;    // then every chunk start is 16-byte aligned
  const size_t plane = (size_t)H * W;
  const int tid = threadIdx.x;
  const int vc = tid & (SS_TW - 1), vr0 = (tid / SS_TW) * 4;   // vertical pass: column vc, output rows vr0 .. vr0 + 3
  double acc = 0.0;

  // staging of one channel: the loads of channel ch + 1 are issued into registers before the filters of channel ch run
  constexpr int NIT = (SS_SH * NCH + 255) / 256;   // staging chunks per thread
  T xr[NIT][V], yr[NIT][V];
  T kxr, kyr;                                      // the shift pixels of the fetched channel
  auto fetch = [&](int ch) {
    const T* rp = rb + ((size_t)ch * Tn + t) * plane;
    const T* tp = tb + ((size_t)ch * Tn + t) * plane;
    const size_t kofs = (size_t)(y0 + SS_R) * W + x0 + SS_R;
    kxr = rp[kofs];
    kyr = tp[kofs];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256, r = i / NCH, q = (i - r * NCH) * V;
      const int gy = y0 + r, gx = x0 + q;
      if (i >= SS_SH * NCH || gy >= H) continue;
      if (vec_ok && gx < W) {
        *reinterpret_cast<uint4*>(xr[it]) = *reinterpret_cast<const uint4*>(rp + (size_t)gy * W + gx);
        *reinterpret_cast<uint4*>(yr[it]) = *reinterpret_cast<const uint4*>(tp + (size_t)gy * W + gx);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if (gx + e < W) {
            xr[it][e] = rp[(size_t)gy * W + gx + e];
            yr[it][e] = tp[(size_t)gy * W + gx + e];
          }
        }
      }
    }
  };
  fetch(0);

  for (int ch = 0; ch < C; ++ch) {
    // ---- stage: rows y0 .. y0 + 41, columns x0 .. x0 + 41; cells outside the frame (read by no kept window) hold 0
    float kx = (float)kxr;
    if (clamp) kx = __builtin_amdgcn_fmed3f(kx, -1.0f, 1.0f);
    const float ky = (float)kyr;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256, r = i / NCH, q = (i - r * NCH) * V;
      if (i >= SS_SH * NCH) continue;
      const int gy = y0 + r, gx = x0 + q;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (q + e < SS_SW) {
          const bool in = gy < H && gx + e < W;
          float x = in ? (float)xr[it][e] : kx;
          if (clamp) x = __builtin_amdgcn_fmed3f(x, -1.0f, 1.0f);
          const float y = in ? (float)yr[it][e] : ky;
          sxy[r * SS_SP + q + e] = (f32x2){x - kx, y - ky};
        }
      }
    }
    __syncthreads();
    if (ch + 1 < C) fetch(ch + 1);

    // ---- horizontal pass: 42 rows x 8 groups of 4 output columns (taps in ascending order for every output)
    for (int i = tid; i < SS_SH * (SS_TW / 4); i += 256) {
      const int r = i / (SS_TW / 4), c0 = (i % (SS_TW / 4)) * 4;
      float sx[4] = {}, sy[4] = {}, sxx[4] = {}, syy[4] = {}, sxy_[4] = {};
#pragma unroll
      for (int j = 0; j < 2 * SS_R + 4; ++j) {
        const f32x2 v = sxy[r * SS_SP + c0 + j];
        const float xx = v.x * v.x, yy = v.y * v.y, xy = v.x * v.y;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int k = j - o;
          if (k >= 0 && k <= 2 * SS_R) {
            sx[o] = fmaf(a.g[k], v.x, sx[o]);
            sy[o] = fmaf(a.g[k], v.y, sy[o]);
            sxx[o] = fmaf(a.g[k], xx, sxx[o]);
            syy[o] = fmaf(a.g[k], yy, syy[o]);
            sxy_[o] = fmaf(a.g[k], xy, sxy_[o]);
          }
        }
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        hm[r * SS_TW + c0 + o] = (f32x2){sx[o], sy[o]};
        hq[r * SS_TW + c0 + o] = (f32x2){sxx[o], syy[o]};
        hp[r * SS_TW + c0 + o] = sxy_[o];
      }
    }
    __syncthreads();

    // ---- vertical pass + index: 4 consecutive output rows of one column per thread
    {
      float mx[4] = {}, my[4] = {}, exx[4] = {}, eyy[4] = {}, exy[4] = {};
#pragma unroll
      for (int i = 0; i < 2 * SS_R + 4; ++i) {
        const int row = (vr0 + i) * SS_TW + vc;
        const f32x2 m = hm[row], q = hq[row];
        const float p = hp[row];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int k = i - o;
          if (k >= 0 && k <= 2 * SS_R) {
            mx[o] = fmaf(a.g[k], m.x, mx[o]);
            my[o] = fmaf(a.g[k], m.y, my[o]);
            exx[o] = fmaf(a.g[k], q.x, exx[o]);
            eyy[o] = fmaf(a.g[k], q.y, eyy[o]);
            exy[o] = fmaf(a.g[k], p, exy[o]);
          }
        }
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (vr0 + o < vh && vc < vw) {
          const float sx2 = fmaxf(fmaf(-mx[o], mx[o], exx[o]), 0.0f);    // shift-free second moments
          const float sy2 = fmaxf(fmaf(-my[o], my[o], eyy[o]), 0.0f);
          const float sxy2 = fmaf(-mx[o], my[o], exy[o]);
          const float ux = kx + mx[o], uy = ky + my[o];                  // means of the unshifted images
          const float num = (2.0f * (ux * uy) + C1) * (2.0f * sxy2 + C2);
          const float den = ((ux * ux + uy * uy) + C1) * ((sx2 + sy2) + C2);
          acc += (double)(num / den);
        }
      }
    }
    // the next channel's staging writes only sxy, which no thread reads after the barrier behind the horizontal pass
  }
  const double s = ss_block_sum(acc, red);
  if (tid == 0) part[item] = s;
}

__global__ __launch_bounds__(256) void k_ssim_finish(SsimClips a, int n_clips, const double* __restrict__ part, double* __restrict__ acc2) {
  __shared__ double red[256];
  const int frames = a.frame0[n_clips];
  double s = 0.0;
  for (int f = threadIdx.x; f < frames; f += 256) {
    int c = 0;                                    // last clip whose first frame <= f
    for (int step = TTV_MAX_CLIPS_PER_LAUNCH / 2; step > 0; step >>= 1)
      if (c + step < n_clips && a.frame0[c + step] <= f) c += step;
    const int tiles = ss_tiles_x(a.W[c]) * ss_tiles_y(a.H[c]);
    const double* p = part + a.item0[c] + (size_t)(f - a.frame0[c]) * tiles;
    double v = 0.0;
    int k = 0;
    for (; k + 8 <= tiles; k += 8) {             // eight loads in flight, added in tile order
      double w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = p[k + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += w[u];
    }
    for (; k < tiles; ++k) v += p[k];
    s += v / ((double)a.C[c] * (a.H[c] - 2 * SS_R) * (a.W[c] - 2 * SS_R));
  }
  s = ss_block_sum(s, red);
  if (threadIdx.x == 0) {
    acc2[0] += s;
    acc2[1] += (double)frames;
  }
}

// shapes -> per-clip item offsets; -1 (error set) on a bad shape
static int64_t ssim_layout(const int32_t* dims, int n_clips, SsimClips* a) {
  if (!(n_clips >= 0 && n_clips <= TTV_MAX_CLIPS_PER_LAUNCH)) {
    ttv_set_error("ssim: at most %d clips per call, got %d", TTV_MAX_CLIPS_PER_LAUNCH, n_clips);
    return -1;
  }
  if (n_clips > 0 && !dims) {
    ttv_set_error("ssim: null dims");
    return -1;
  }
  int64_t items = 0, frames = 0;
  for (int i = 0; i < n_clips; ++i) {
    const int C = dims[4 * i], T = dims[4 * i + 1], H = dims[4 * i + 2], W = dims[4 * i + 3];
    if (C < 1 || T < 1) {
      ttv_set_error("ssim: clip %d has C = %d, T = %d (both must be >= 1)", i, C, T);
      return -1;
    }
    if (H < 2 * SS_R + 1 || W < 2 * SS_R + 1) {
      ttv_set_error("ssim: clip %d has %d x %d frames; the 11 x 11 window needs H >= 11 and W >= 11", i, H, W);
      return -1;
    }
    a->C[i] = C; a->T[i] = T; a->H[i] = H; a->W[i] = W;
    a->item0[i] = (int)items;
    a->frame0[i] = (int)frames;
    frames += T;
    items += (int64_t)T * ttv_cdiv(W - 2 * SS_R, SS_TW) * ttv_cdiv(H - 2 * SS_R, SS_TH);
    if (items > 0x7fffffff || frames > 0x7fffffff) {
      ttv_set_error("ssim: more than 2^31 - 1 tiles in one call");
      return -1;
    }
  }
  a->item0[n_clips] = (int)items;
  a->frame0[n_clips] = (int)frames;
  return items;
}

int64_t ttvk_ssim_workspace_bytes(const int32_t* dims, int n_clips) {
  SsimClips a;
  const int64_t items = ssim_layout(dims, n_clips, &a);
  return items < 0 ? -1 : items * (int64_t)sizeof(double);
}

int ttvk_ssim(void* const* recon, void* const* target, const int32_t* dims, int n_clips, int dtype, int clamp, double* acc2, void* workspace,
              int64_t workspace_bytes, hipStream_t s) {
  SsimClips a;
  const int64_t items = ssim_layout(dims, n_clips, &a);
  if (items < 0) return TTV_ERR_INVALID;
  if (n_clips == 0) return TTV_OK;
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "ssim: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(recon && target && acc2 && workspace, "ssim: null argument");
  TTV_CHECK_ARG(workspace_bytes >= items * (int64_t)sizeof(double), "ssim: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)(items * (int64_t)sizeof(double)));
  TTV_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)acc2 & 7) == 0, "ssim: workspace and acc must be 8-byte aligned");
  for (int i = 0; i < n_clips; ++i) {
    TTV_CHECK_ARG(recon[i] && target[i], "ssim: null clip %d", i);
    a.recon[i] = recon[i];
    a.target[i] = target[i];
  }
  double g[2 * SS_R + 1], sum = 0.0;
  for (int i = 0; i <= 2 * SS_R; ++i) {
    const double d = (i - SS_R) / 1.5;
    g[i] = exp(-0.5 * d * d);
    sum += g[i];
  }
  for (int i = 0; i <= 2 * SS_R; ++i) a.g[i] = (float)(g[i] / sum);
  double* part = reinterpret_cast<double*>(workspace);
  if (dtype == TTV_BF16) hipLaunchKernelGGL((k_ssim_tiles<bf16_t>), dim3((unsigned)items), dim3(256), 0, s, a, n_clips, clamp, part);
  else hipLaunchKernelGGL((k_ssim_tiles<float>), dim3((unsigned)items), dim3(256), 0, s, a, n_clips, clamp, part);
  TTV_CHECK_LAUNCH("ssim tiles");
  hipLaunchKernelGGL(k_ssim_finish, dim3(1), dim3(256), 0, s, a, n_clips, part, acc2);
  TTV_CHECK_LAUNCH("ssim finish");
  return TTV_OK;
}
