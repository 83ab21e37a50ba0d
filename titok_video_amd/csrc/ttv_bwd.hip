// Backward kernels of the TiTok-Video towers (training step, reference train.py:65-83 runs autograd through
// model/base/blocks.py + transformer.py + fsq.py; these kernels are that backward written by hand).
//
//   k_rmsnorm_bwd      dx, dgain of y = x * rsqrt(mean(x^2)+eps) * gain, with row gather/scatter maps
//   k_colsum           bias gradients (sum over rows)
//   k_gate_fwd/_bwd    a * sigmoid(gate)                                       (transformer.py:103)
//   k_geglu_fwd/_bwd   gelu_erf(u_g) * u_x                                     (transformer.py:51-52)
//   k_fsq_bwd          straight-through round: dz = dcodes * half_l/half_width * (1 - tanh^2(z+shift))   (fsq.py:48-51,78-90)
//   k_scale_cast       b = alpha * a (fp32), c = (T) a
//   k_wgrad_bf16       dW[N,K] += dY[L,N]^T X[L,K]: contraction over TOKENS, so both MFMA operands are fetched with
//                      ds_read_b64_tr_b16 (hardware transpose read) from row-major LDS tiles; split over token ranges,
//                      fp32 atomic accumulation into dW (one 256-byte row segment per wave instruction)
//   k_attn_delta       delta[t,h] = sum_d dO*O
//   k_attn_delta_f32_consistent   the fp32 checking path's delta = sum_j p_j dP_j / sum_j p_j, from its own P and dP
//   k_attn_bwd_dq / k_attn_bwd_dkv   flash-style recompute (P from Q,K and the forward's LSE): no atomics - one kernel
//                      owns query blocks (dQ), the other key blocks (dK, dV); GQA heads of a group are summed in-kernel
//   *_f32 variants     naive VALU kernels, used only to check gradients tightly in fp32
#include "ttv_common.h"
#include "ttv_kernels.h"

#define BW_MAX_ITERS 4

// ------------------------------------------------------------------------------------------------ deterministic mode: the fold
// Second stage of every fixed-order row reduction: part is [nblocks][n] (T = float, double for the PSNR sums), written by the
// DET form of the reducing kernel with plain stores.  One thread per element adds its partials in ascending block index, starting from
// block 0's, and then the total onto the destination with a plain load / add / store (the destination is accumulated into).
// Element e lives at dst[(e / inner) * stride_outer + (e % inner) * stride_inner].
template <typename T>
__global__ __launch_bounds__(256) void k_det_fold(const T* __restrict__ part, int nblocks, int n, int inner, long stride_outer,
                                                  long stride_inner, T* __restrict__ dst) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  T sum = part[e];
  int b = 1;
  for (; b + 8 <= nblocks; b += 8) {      // eight loads in flight, added one after the other
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(b + u) * n + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  for (; b < nblocks; ++b) sum += part[(size_t)b * n + e];
  T* p = dst + (long)(e / inner) * stride_outer + (long)(e % inner) * stride_inner;
  *p = *p + sum;
}
template <typename T>
static int det_fold(const void* part, int nblocks, int n, int inner, long stride_outer, long stride_inner, T* dst, hipStream_t s) {
  hipLaunchKernelGGL((k_det_fold<T>), dim3(ttv_cdiv(n, 256)), dim3(256), 0, s, (const T*)part, nblocks, n, inner, stride_outer, stride_inner, dst);
  TTV_CHECK_LAUNCH("det_fold");
  return TTV_OK;
}
// the scratch a deterministic launch needs: present, 16-byte aligned, large enough - checked before anything is launched
#define TTV_CHECK_DET(det_, need_, what_)                                                                                         \
  TTV_CHECK_ARG((det_) && (det_)->p && ((uintptr_t)(det_)->p % 16 == 0) && (det_)->bytes >= (int64_t)(need_),                      \
                what_ ": deterministic mode needs %lld bytes of 16-byte aligned scratch for its block partials, the caller handed over %lld", \
                (long long)(need_), (long long)((det_) ? (det_)->bytes : 0))

// ------------------------------------------------------------------------------------------------ rmsnorm backward
// DET: the block's gain partial goes to dgain[block][d] (the caller passes the scratch) instead of one atomicAdd per column
template <typename TX, typename TG, typename TO, bool DET>
__global__ __launch_bounds__(256) void k_rmsnorm_bwd(const TX* __restrict__ x, int ldx, const int* __restrict__ x_rows,
                                                     const TG* __restrict__ dy, int lddy, const int* __restrict__ dy_rows,
                                                     const float* __restrict__ gain, TO* __restrict__ dx, int lddx,
                                                     const int* __restrict__ dx_rows, int accumulate, float* __restrict__ dgain,
                                                     int rows, int d, float eps, int rows_per_wave) {
  __shared__ float red[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float dg[BW_MAX_ITERS][4];
#pragma unroll
  for (int it = 0; it < BW_MAX_ITERS; ++it)
#pragma unroll
    for (int e = 0; e < 4; ++e) dg[it][e] = 0.f;
  // RB rows in flight per wave: a single row is a chain of dependent steps (loads -> wave reduction -> second reduction ->
  // store, ~2 us); with the block count held at ~256 for the gain atomics there is one wave per SIMD, so the overlap has to
  // come from independent rows inside the wave
  constexpr int RB = 4;
  const int r0 = (blockIdx.x * 4 + wave) * rows_per_wave;
  const int r_end = r0 + rows_per_wave < rows ? r0 + rows_per_wave : rows;
  for (int rb = r0; rb < r_end; rb += RB) {
    f32x4 xv[RB][BW_MAX_ITERS], gv[RB][BW_MAX_ITERS];
    float ss[RB], dot[RB], rstd[RB];
    bool live[RB];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const int r = rb + q;
      live[q] = r < r_end;
      const int rc = live[q] ? r : r_end - 1;
      const TX* px = x + (size_t)(x_rows ? x_rows[rc] : rc) * ldx;
      const TG* pg = dy + (size_t)(dy_rows ? dy_rows[rc] : rc) * lddy;
      ss[q] = 0.f;
#pragma unroll
      for (int it = 0; it < BW_MAX_ITERS; ++it) {
        const int c = (it * 64 + lane) * 4;
        if (c < d) {
          xv[q][it] = Vec4<TX>::load(px + c);
          gv[q][it] = Vec4<TG>::load(pg + c);
          ss[q] += xv[q][it][0] * xv[q][it][0] + xv[q][it][1] * xv[q][it][1] + xv[q][it][2] * xv[q][it][2] + xv[q][it][3] * xv[q][it][3];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) ss[q] = wave_sum(ss[q]);
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      rstd[q] = 1.0f / sqrtf(ss[q] / (float)d + eps);
      dot[q] = 0.f;   // sum_f (dy*gain) * xhat
#pragma unroll
      for (int it = 0; it < BW_MAX_ITERS; ++it) {
        const int c = (it * 64 + lane) * 4;
        if (c < d) {
          const f32x4 g = *reinterpret_cast<const f32x4*>(gain + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float xh = xv[q][it][e] * rstd[q];
            if (live[q]) dg[it][e] += gv[q][it][e] * xh;
            gv[q][it][e] *= g[e];
            dot[q] += gv[q][it][e] * xh;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) dot[q] = wave_sum(dot[q]) / (float)d;
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      if (!live[q]) continue;
      const int r = rb + q;
      TO* pd = dx + (size_t)(dx_rows ? dx_rows[r] : r) * lddx;
#pragma unroll
      for (int it = 0; it < BW_MAX_ITERS; ++it) {
        const int c = (it * 64 + lane) * 4;
        if (c < d) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = rstd[q] * (gv[q][it][e] - xv[q][it][e] * rstd[q] * dot[q]);
          if (accumulate) o += Vec4<TO>::load(pd + c);
          Vec4<TO>::store(pd + c, o);
        }
      }
    }
  }
  if (dgain) {
#pragma unroll
    for (int it = 0; it < BW_MAX_ITERS; ++it) {
      const int c = (it * 64 + lane) * 4;
      if (c < d) *reinterpret_cast<f32x4*>(&red[wave][c]) = (f32x4){dg[it][0], dg[it][1], dg[it][2], dg[it][3]};
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256) {
      const float v = red[0][c] + red[1][c] + red[2][c] + red[3][c];
      if (DET) dgain[(size_t)blockIdx.x * d + c] = v; else atomicAdd(dgain + c, v);
    }
  }
}

// rows per wave and blocks of the two norm-backward kernels (one geometry for both modes)
static inline int rms_bwd_rpw(int rows) {
  const int rpw = ttv_cdiv(rows, 4 * 512);   // ~2 blocks per CU: the row loop is latency-bound, two waves per SIMD overlap it
  return rpw < 1 ? 1 : rpw;
}
static inline int rms_bwd_blocks(int rows) { return ttv_cdiv(rows, 4 * rms_bwd_rpw(rows)); }
int64_t ttvk_det_rms_bytes(int rows, int d) { return rows > 0 && d > 0 ? (int64_t)rms_bwd_blocks(rows) * d * 4 : 0; }

template <typename TX, typename TG, typename TO>
static int launch_rms_bwd(const void* x, int ldx, const int* xr, const void* dy, int lddy, const int* dyr, const float* gain, void* dx,
                          int lddx, const int* dxr, int acc, float* dgain, int rows, int d, float eps, hipStream_t s, const DetScratch* det) {
  // few, fat blocks: the gain gradient is one atomicAdd per column per BLOCK onto the same `d` addresses, so the block count
  // (not the row count) sets the contention; ~256 blocks keep every CU busy
  const int rpw = rms_bwd_rpw(rows), nb = rms_bwd_blocks(rows);
  if (dgain && ttv_det()) {
    TTV_CHECK_DET(det, ttvk_det_rms_bytes(rows, d), "rmsnorm_bwd");
    hipLaunchKernelGGL((k_rmsnorm_bwd<TX, TG, TO, true>), dim3(nb), dim3(256), 0, s, (const TX*)x, ldx, xr, (const TG*)dy,
                       lddy, dyr, gain, (TO*)dx, lddx, dxr, acc, (float*)det->p, rows, d, eps, rpw);
    TTV_CHECK_LAUNCH("rmsnorm_bwd");
    return det_fold<float>(det->p, nb, d, d, 0, 1, dgain, s);
  }
  hipLaunchKernelGGL((k_rmsnorm_bwd<TX, TG, TO, false>), dim3(nb), dim3(256), 0, s, (const TX*)x, ldx, xr, (const TG*)dy,
                     lddy, dyr, gain, (TO*)dx, lddx, dxr, acc, dgain, rows, d, eps, rpw);
  TTV_CHECK_LAUNCH("rmsnorm_bwd");
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------ chained norm backward
// The backward of a layer boundary is row-local end to end:
//   h   = acc + rmsnorm_bwd(x, gain1, dy)          (pre-norm of a sub-layer: its gradient joins the residual gradient `acc`)
//   out = rmsnorm_bwd(y, gain2, h)                 (KEEL post-norm of the sub-layer below; skipped when y == NULL: out = h)
//   dx  = out_scale * out  (fp32, in place of acc) ; cast_out = (T) out      (alpha * dy and the GEMM operand copy)
// One kernel instead of rmsnorm_bwd(accumulate) + rmsnorm_bwd + scale_cast: the row is read once (x, dy, acc, y) and written
// once (dx, cast_out); the three launches moved 9.7 KB per row at width 256, this one moves 4.6 KB.
__device__ __forceinline__ float dpp_f(float v, const int ctrl_tag) {
  const int i = __builtin_bit_cast(int, v);
  int r;
  switch (ctrl_tag) {
    case 0: r = __builtin_amdgcn_update_dpp(0, i, 0xB1, 0xF, 0xF, true); break;    // quad_perm [1,0,3,2]
    case 1: r = __builtin_amdgcn_update_dpp(0, i, 0x4E, 0xF, 0xF, true); break;    // quad_perm [2,3,0,1]
    case 2: r = __builtin_amdgcn_update_dpp(0, i, 0x141, 0xF, 0xF, true); break;   // row_half_mirror
    default: r = __builtin_amdgcn_update_dpp(0, i, 0x140, 0xF, 0xF, true); break;  // row_mirror
  }
  return __builtin_bit_cast(float, r);
}
// 64-lane sum: four DPP steps inside the 16-lane rows, two cross-row exchanges
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_f(v, 0);
  v += dpp_f(v, 1);
  v += dpp_f(v, 2);
  v += dpp_f(v, 3);
  return quad16_sum(v);        // lanes ^ 16, then ^ 32, on v_permlane16_swap / v_permlane32_swap (same association as the two ds_bpermute steps it replaces)
}

// DET: dgain1 / dgain2 are the [block][d] partial arrays of the two gains
template <typename T, typename YT, int ITERS, bool DET>
__global__ __launch_bounds__(256) void k_rmsnorm_bwd_chain(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int lddy,
                                                           const float* __restrict__ gain1, float* __restrict__ dgain1, float* dx, int lddx,
                                                           const YT* __restrict__ y, int ldy, const float* __restrict__ gain2,
                                                           float* __restrict__ dgain2, float out_scale, T* __restrict__ cast_out, int ldc,
                                                           int rows, int d, float eps, int rows_per_wave) {
  __shared__ float red[4][ITERS * 256];
  constexpr int RB = ITERS == 1 ? 4 : 2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool second = y != nullptr;
  const float inv_d = 1.0f / (float)d;
  f32x4 g1[ITERS], g2[ITERS], dg1[ITERS], dg2[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int c = (it * 64 + lane) * 4;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    g1[it] = c < d ? *reinterpret_cast<const f32x4*>(gain1 + c) : z;
    g2[it] = (second && c < d) ? *reinterpret_cast<const f32x4*>(gain2 + c) : z;
    dg1[it] = z;
    dg2[it] = z;
  }
  const int r0 = (blockIdx.x * 4 + wave) * rows_per_wave;
  const int r_end = r0 + rows_per_wave < rows ? r0 + rows_per_wave : rows;
  for (int rb = r0; rb < r_end; rb += RB) {
    f32x4 xv[RB][ITERS], gv[RB][ITERS], hv[RB][ITERS], yv[RB][ITERS];
    float ss1[RB], ss2[RB], dot[RB], rstd1[RB], rstd2[RB];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const int r = rb + q < r_end ? rb + q : r_end - 1;
      ss1[q] = 0.f;
      ss2[q] = 0.f;
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int c = (it * 64 + lane) * 4;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        xv[q][it] = z; gv[q][it] = z; hv[q][it] = z; yv[q][it] = z;
        if (c < d) {
          xv[q][it] = Vec4<T>::load(x + (size_t)r * ldx + c);
          gv[q][it] = Vec4<T>::load(dy + (size_t)r * lddy + c);
          hv[q][it] = *reinterpret_cast<const f32x4*>(dx + (size_t)r * lddx + c);
          if (second) yv[q][it] = Vec4<YT>::load(y + (size_t)r * ldy + c);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ss1[q] = fmaf(xv[q][it][e], xv[q][it][e], ss1[q]);
          ss2[q] = fmaf(yv[q][it][e], yv[q][it][e], ss2[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) ss1[q] = wave_sum_dpp(ss1[q]);
    if (second) {
#pragma unroll
      for (int q = 0; q < RB; ++q) ss2[q] = wave_sum_dpp(ss2[q]);
    }
    // stage 1: h = acc + rstd1 * (g1*dy - xhat * mean(g1*dy*xhat)) ; dgain1 += dy * xhat
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      const bool live = rb + q < r_end;
      rstd1[q] = 1.0f / sqrtf(ss1[q] * inv_d + eps);
      rstd2[q] = 1.0f / sqrtf(ss2[q] * inv_d + eps);
      dot[q] = 0.f;
#pragma unroll
      for (int it = 0; it < ITERS; ++it)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = xv[q][it][e] * rstd1[q];
          if (live) dg1[it][e] = fmaf(gv[q][it][e], xh, dg1[it][e]);
          gv[q][it][e] *= g1[it][e];
          dot[q] = fmaf(gv[q][it][e], xh, dot[q]);
          xv[q][it][e] = xh;
        }
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) dot[q] = wave_sum_dpp(dot[q]) * inv_d;
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int it = 0; it < ITERS; ++it)
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[q][it][e] += rstd1[q] * (gv[q][it][e] - xv[q][it][e] * dot[q]);
    // stage 2: out = rstd2 * (g2*h - yhat * mean(g2*h*yhat)) ; dgain2 += h * yhat
    if (second) {
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const bool live = rb + q < r_end;
        dot[q] = 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float yh = yv[q][it][e] * rstd2[q];
            if (live) dg2[it][e] = fmaf(hv[q][it][e], yh, dg2[it][e]);
            hv[q][it][e] *= g2[it][e];
            dot[q] = fmaf(hv[q][it][e], yh, dot[q]);
            yv[q][it][e] = yh;
          }
      }
#pragma unroll
      for (int q = 0; q < RB; ++q) dot[q] = wave_sum_dpp(dot[q]) * inv_d;
#pragma unroll
      for (int q = 0; q < RB; ++q)
#pragma unroll
        for (int it = 0; it < ITERS; ++it)
#pragma unroll
          for (int e = 0; e < 4; ++e) hv[q][it][e] = rstd2[q] * (hv[q][it][e] - yv[q][it][e] * dot[q]);
    }
#pragma unroll
    for (int q = 0; q < RB; ++q) {
      if (rb + q >= r_end) continue;
      const int r = rb + q;
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int c = (it * 64 + lane) * 4;
        if (c < d) {
          if (cast_out) Vec4<T>::store(cast_out + (size_t)r * ldc + c, hv[q][it]);
          *reinterpret_cast<f32x4*>(dx + (size_t)r * lddx + c) = hv[q][it] * out_scale;
        }
      }
    }
  }
  // gain gradients: block-level sum through LDS, one atomicAdd per column per block
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    float* dgain = pass ? dgain2 : dgain1;
    if (pass && !second) break;
    if (!dgain) continue;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = (it * 64 + lane) * 4;
      if (c < d) *reinterpret_cast<f32x4*>(&red[wave][c]) = pass ? dg2[it] : dg1[it];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256) {
      const float v = red[0][c] + red[1][c] + red[2][c] + red[3][c];
      if (DET) dgain[(size_t)blockIdx.x * d + c] = v; else atomicAdd(dgain + c, v);
    }
  }
}

template <typename T, typename YT, int ITERS>
static void launch_rms_chain(const void* x, int ldx, const void* dy, int lddy, const float* gain1, float* dgain1, float* dx, int lddx,
                             const void* y, int ldy, const float* gain2, float* dgain2, float out_scale, void* cast_out, int ldc, int rows,
                             int d, float eps, hipStream_t s, bool det) {
  const int rpw = rms_bwd_rpw(rows);
  if (det)
    hipLaunchKernelGGL((k_rmsnorm_bwd_chain<T, YT, ITERS, true>), dim3(rms_bwd_blocks(rows)), dim3(256), 0, s, (const T*)x, ldx, (const T*)dy, lddy,
                       gain1, dgain1, dx, lddx, (const YT*)y, ldy, gain2, dgain2, out_scale, (T*)cast_out, ldc, rows, d, eps, rpw);
  else
    hipLaunchKernelGGL((k_rmsnorm_bwd_chain<T, YT, ITERS, false>), dim3(rms_bwd_blocks(rows)), dim3(256), 0, s, (const T*)x, ldx, (const T*)dy, lddy,
                       gain1, dgain1, dx, lddx, (const YT*)y, ldy, gain2, dgain2, out_scale, (T*)cast_out, ldc, rows, d, eps, rpw);
}

// y_dt: dtype of the second norm's input y (TTV_F32, or TTV_BF16 with dt == TTV_BF16: the bf16 towers' tape keeps the KEEL sums in bf16)
int ttvk_rmsnorm_bwd_chain(const void* x, int ldx, const void* dy, int lddy, const float* gain1, float* dgain1_dst, float* dx, int lddx,
                           const void* y, int y_dt, int ldy, const float* gain2, float* dgain2_dst, float out_scale, void* cast_out, int ldc, int rows,
                           int d, float eps, int dt, hipStream_t s, const DetScratch* scratch) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(d % 4 == 0 && d <= 1024, "rmsnorm_bwd_chain: width");
  TTV_CHECK_ARG(dt == TTV_BF16 || dt == TTV_F32, "rmsnorm_bwd_chain: dtype");
  TTV_CHECK_ARG(!y || gain2, "rmsnorm_bwd_chain: second norm needs its gain");
  TTV_CHECK_ARG(!y || y_dt == TTV_F32 || (y_dt == TTV_BF16 && dt == TTV_BF16), "rmsnorm_bwd_chain: y is fp32, or bf16 beside bf16 rows");
  const int iters = ttv_cdiv(d, 256);
  // deterministic mode: the kernel writes the block partials of gain 1 to the scratch's first ttvk_det_rms_bytes(), those of gain 2
  // behind them; two folds add them onto the gain gradients
  const bool want2 = y && dgain2_dst;
  const bool det = (dgain1_dst || want2) && ttv_det();
  float *dgain1 = dgain1_dst, *dgain2 = dgain2_dst;
  const int64_t one = ttvk_det_rms_bytes(rows, d);
  if (det) {
    TTV_CHECK_DET(scratch, 2 * one, "rmsnorm_bwd_chain");
    dgain1 = dgain1_dst ? (float*)scratch->p : nullptr;
    dgain2 = want2 ? (float*)((char*)scratch->p + one) : nullptr;
  }
#define RC(T, YT, I) launch_rms_chain<T, YT, I>(x, ldx, dy, lddy, gain1, dgain1, dx, lddx, y, ldy, gain2, dgain2, out_scale, cast_out, ldc, rows, d, eps, s, det)
  if (dt == TTV_BF16 && y && y_dt == TTV_BF16) {
    if (iters == 1) RC(bf16_t, bf16_t, 1); else if (iters == 2) RC(bf16_t, bf16_t, 2); else RC(bf16_t, bf16_t, 4);
  } else if (dt == TTV_BF16) {
    if (iters == 1) RC(bf16_t, float, 1); else if (iters == 2) RC(bf16_t, float, 2); else RC(bf16_t, float, 4);
  } else {
    if (iters == 1) RC(float, float, 1); else if (iters == 2) RC(float, float, 2); else RC(float, float, 4);
  }
#undef RC
  TTV_CHECK_LAUNCH("rmsnorm_bwd_chain");
  if (det) {
    const int nb = rms_bwd_blocks(rows);
    if (dgain1) TTV_TRY(det_fold<float>(dgain1, nb, d, d, 0, 1, dgain1_dst, s));
    if (dgain2) TTV_TRY(det_fold<float>(dgain2, nb, d, d, 0, 1, dgain2_dst, s));
  }
  return TTV_OK;
}

// x dtype, dy dtype, dx dtype codes: TTV_BF16 / TTV_F32
int ttvk_rmsnorm_bwd(const void* x, int x_dt, int ldx, const int* xr, const void* dy, int dy_dt, int lddy, const int* dyr,
                     const float* gain, void* dx, int dx_dt, int lddx, const int* dxr, int acc, float* dgain, int rows, int d, float eps,
                     hipStream_t s, const DetScratch* det) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(d % 4 == 0 && d <= 1024, "rmsnorm_bwd: width");
#define RB(TX, TG, TO) return launch_rms_bwd<TX, TG, TO>(x, ldx, xr, dy, lddy, dyr, gain, dx, lddx, dxr, acc, dgain, rows, d, eps, s, det)
  const int key = x_dt * 4 + dy_dt * 2 + dx_dt;
  switch (key) {
    case 0: RB(bf16_t, bf16_t, bf16_t);
    case 1: RB(bf16_t, bf16_t, float);
    case 2: RB(bf16_t, float, bf16_t);
    case 3: RB(bf16_t, float, float);
    case 4: RB(float, bf16_t, bf16_t);
    case 5: RB(float, bf16_t, float);
    case 6: RB(float, float, bf16_t);
    case 7: RB(float, float, float);
  }
#undef RB
  return TTV_ERR_INVALID;
}

// ------------------------------------------------------------------------------------------------ column sums (bias grads)
// thread -> column (grid.y tiles of 256 columns), block -> row range.  Eight rows in flight per thread (independent partial sums):
// with one running sum the 128 rows of a block were 128 dependent load -> add steps and the launch took ~30 us whatever the batch
// (latency, not bytes: 6 launches per training step); the partial sums are combined in a fixed order, rows past the end add zero.
// DET: out is the [row block][n] partial array
template <typename T, bool DET>
__global__ __launch_bounds__(256) void k_colsum(const T* __restrict__ a, int lda, const int* __restrict__ rows_map, int rows, int n,
                                                float* __restrict__ out, int rows_per_block) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= n) return;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = r0; r < r1; r += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int rr = r + u < r1 ? r + u : r1 - 1;
      v[u] = Cvt<T>::to_f(a[(size_t)(rows_map ? rows_map[rr] : rr) * lda + c]);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] += r + u < r1 ? v[u] : 0.f;
  }
  const float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  if (DET) out[(size_t)blockIdx.x * n + c] = v; else atomicAdd(out + c, v);
}

#define COLSUM_RPB 64
int64_t ttvk_det_colsum_bytes(int rows, int n) { return rows > 0 && n > 0 ? (int64_t)ttv_cdiv(rows, COLSUM_RPB) * n * 4 : 0; }

int ttvk_colsum(const void* a, int dt, int lda, const int* rows_map, int rows, int n, float* out, hipStream_t s, const DetScratch* det) {
  if (rows == 0 || n == 0 || !out) return TTV_OK;   // out == NULL: this parameter's gradient is not wanted
  // narrow matrices (n <= 256: one column tile) are latency-bound per block: shorter row ranges, more blocks
  const int rpb = COLSUM_RPB;
  dim3 grid(ttv_cdiv(rows, rpb), ttv_cdiv(n, 256));
  if (ttv_det()) {
    TTV_CHECK_DET(det, ttvk_det_colsum_bytes(rows, n), "colsum");
    float* part = (float*)det->p;
    if (dt == TTV_BF16) hipLaunchKernelGGL((k_colsum<bf16_t, true>), grid, dim3(256), 0, s, (const bf16_t*)a, lda, rows_map, rows, n, part, rpb);
    else hipLaunchKernelGGL((k_colsum<float, true>), grid, dim3(256), 0, s, (const float*)a, lda, rows_map, rows, n, part, rpb);
    TTV_CHECK_LAUNCH("colsum");
    return det_fold<float>(part, (int)grid.x, n, n, 0, 1, out, s);
  }
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_colsum<bf16_t, false>), grid, dim3(256), 0, s, (const bf16_t*)a, lda, rows_map, rows, n, out, rpb);
  else hipLaunchKernelGGL((k_colsum<float, false>), grid, dim3(256), 0, s, (const float*)a, lda, rows_map, rows, n, out, rpb);
  TTV_CHECK_LAUNCH("colsum");
  return TTV_OK;
}

// sum of ALL elements (mask_token gradient pieces): out[0] += scale * sum(a[rows, 0:n])
// DET: out is the [block] partial array
template <typename T, bool DET>
__global__ __launch_bounds__(256) void k_sumall(const T* __restrict__ a, int lda, const int* __restrict__ rows_map, int rows, int n,
                                                const float* __restrict__ colw, float scale, float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  const long total = (long)rows * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int r = (int)(i / n), c = (int)(i % n);
    const float v = Cvt<T>::to_f(a[(size_t)(rows_map ? rows_map[r] : r) * lda + c]);
    acc += colw ? v * colw[c] : v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = scale * (red[0] + red[1] + red[2] + red[3]);
    if (DET) out[blockIdx.x] = v; else atomicAdd(out, v);
  }
}

static inline int sumall_blocks(long total) {
  const long b = (total + 255) / 256;
  return (int)(b > 1024 ? 1024 : b);
}
int64_t ttvk_det_sumall_bytes(long total) { return total > 0 ? (int64_t)sumall_blocks(total) * 4 : 0; }

int ttvk_sumall(const void* a, int dt, int lda, const int* rows_map, int rows, int n, const float* colw, float scale, float* out,
                hipStream_t s, const DetScratch* det) {
  if (rows == 0 || n == 0 || !out) return TTV_OK;
  const long total = (long)rows * n;
  const int blocks = sumall_blocks(total);
  if (ttv_det()) {
    TTV_CHECK_DET(det, ttvk_det_sumall_bytes(total), "sumall");
    float* part = (float*)det->p;
    if (dt == TTV_BF16) hipLaunchKernelGGL((k_sumall<bf16_t, true>), dim3(blocks), dim3(256), 0, s, (const bf16_t*)a, lda, rows_map, rows, n, colw, scale, part);
    else hipLaunchKernelGGL((k_sumall<float, true>), dim3(blocks), dim3(256), 0, s, (const float*)a, lda, rows_map, rows, n, colw, scale, part);
    TTV_CHECK_LAUNCH("sumall");
    return det_fold<float>(part, blocks, 1, 1, 0, 0, out, s);
  }
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_sumall<bf16_t, false>), dim3(blocks), dim3(256), 0, s, (const bf16_t*)a, lda, rows_map, rows, n, colw, scale, out);
  else hipLaunchKernelGGL((k_sumall<float, false>), dim3(blocks), dim3(256), 0, s, (const float*)a, lda, rows_map, rows, n, colw, scale, out);
  TTV_CHECK_LAUNCH("sumall");
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------ elementwise
__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + __expf(-v)); }

// ag = a * sigmoid(gate).  ag may be a itself (no __restrict__ on the two): every vector is loaded and stored by one thread, once.
template <typename T>
__global__ __launch_bounds__(256) void k_gate_fwd(const T* a, int lda, const T* __restrict__ gate, int ldg, T* ag, int ldo, int rows, int d) {
  const long total = (long)rows * (d / 4);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / (d / 4);
    const int c = (int)(i % (d / 4)) * 4;
    const f32x4 av = Vec4<T>::load(a + r * lda + c), gv = Vec4<T>::load(gate + r * ldg + c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = av[e] * sigmoidf_(gv[e]);
    Vec4<T>::store(ag + r * ldo + c, o);
  }
}
// da = dag * sigmoid(gate);  dgate = dag * a * sigmoid(gate) * (1 - sigmoid(gate))
// delta (optional, fp32 [rows, d/64]): the attention backward's delta[t, h] = sum over the head's 64 dims of da * a, taken from
// the values this kernel holds anyway (da as it is stored, i.e. rounded to T) - 16 consecutive threads cover one (row, head).
template <typename T>
__global__ __launch_bounds__(256) void k_gate_bwd(const T* __restrict__ dag, int ldd, const T* __restrict__ a, int lda,
                                                  const T* __restrict__ gate, int ldg, T* __restrict__ da, int ldda, T* __restrict__ dgate,
                                                  int lddg, int rows, int d, float* __restrict__ delta) {
  const long total = (long)rows * (d / 4);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / (d / 4);
    const int c = (int)(i % (d / 4)) * 4;
    const f32x4 dv = Vec4<T>::load(dag + r * ldd + c), av = Vec4<T>::load(a + r * lda + c), gv = Vec4<T>::load(gate + r * ldg + c);
    f32x4 o1, o2;
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float sg = sigmoidf_(gv[e]);
      o1[e] = dv[e] * sg;
      o2[e] = dv[e] * av[e] * sg * (1.0f - sg);
      part = fmaf(round_to<T>(o1[e]), av[e], part);
    }
    Vec4<T>::store(da + r * ldda + c, o1);
    Vec4<T>::store(dgate + r * lddg + c, o2);
    if (delta) {   // d % 64 == 0 (checked on the host): whole 16-lane groups are inside or outside the loop together
      part += dpp_f(part, 0);
      part += dpp_f(part, 1);
      part += dpp_f(part, 2);
      part += dpp_f(part, 3);
      if ((threadIdx.x & 15) == 0) delta[r * (d >> 6) + (c >> 6)] = part;
    }
  }
}
__device__ __forceinline__ float gelu_f(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad_f(float v) {
  const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * __expf(-0.5f * v * v);
  return cdf + v * pdf;
}
// h = gelu(u[:, I:]) * u[:, :I]
template <typename T>
__global__ __launch_bounds__(256) void k_geglu_fwd(const T* __restrict__ u, int ldu, T* __restrict__ h, int ldh, int rows, int I) {
  const long total = (long)rows * (I / 4);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / (I / 4);
    const int c = (int)(i % (I / 4)) * 4;
    const f32x4 xv = Vec4<T>::load(u + r * ldu + c), gv = Vec4<T>::load(u + r * ldu + I + c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = gelu_f(gv[e]) * xv[e];
    Vec4<T>::store(h + r * ldh + c, o);
  }
}
// du[:, :I] = dh * gelu(u_g);  du[:, I:] = dh * u_x * gelu'(u_g)
template <typename T>
__global__ __launch_bounds__(256) void k_geglu_bwd(const T* __restrict__ u, int ldu, const T* __restrict__ dh, int lddh,
                                                   T* __restrict__ du, int lddu, int rows, int I) {
  const long total = (long)rows * (I / 4);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / (I / 4);
    const int c = (int)(i % (I / 4)) * 4;
    const f32x4 xv = Vec4<T>::load(u + r * ldu + c), gv = Vec4<T>::load(u + r * ldu + I + c), dv = Vec4<T>::load(dh + r * lddh + c);
    f32x4 o1, o2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o1[e] = dv[e] * gelu_f(gv[e]);
      o2[e] = dv[e] * xv[e] * gelu_grad_f(gv[e]);
    }
    Vec4<T>::store(du + r * lddu + c, o1);
    Vec4<T>::store(du + r * lddu + I + c, o2);
  }
}
// bf16 form: 16-byte accesses (8 features per thread) and Phi(g) = sigmoid(p(g)) of the forward's geglu_fast() (ttv_common.h: |g Phi - gelu| <= 2.6e-5,
// a tenth of a bf16 half-ulp) instead of erff() - with erff() and expf() per element the kernel was bound by its ~60 VALU instructions per
// element, not by its 260 MB (round 5: 44.7 -> see profiles/r05_train_geglu_bwd.txt).  gelu'(g) = Phi(g) + g phi(g), phi by one v_exp_f32.
__global__ __launch_bounds__(256) void k_geglu_bwd_bf16(const bf16_t* __restrict__ u, int ldu, const bf16_t* __restrict__ dh, int lddh,
                                                        bf16_t* __restrict__ du, int lddu, int rows, int I) {
  const int i8 = I / 8;
  const long total = (long)rows * i8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / i8;
    const int c = (int)(i - r * i8) * 8;
    const bf16x8 xv = *reinterpret_cast<const bf16x8*>(u + r * ldu + c), gv = *reinterpret_cast<const bf16x8*>(u + r * ldu + I + c);
    const bf16x8 dv = *reinterpret_cast<const bf16x8*>(dh + r * lddh + c);
    bf16x8 o1, o2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float g = (float)gv[e], d = (float)dv[e], x = (float)xv[e];
      const float gc = __builtin_amdgcn_fmed3f(g, -8.0f, 8.0f);
      const float g2 = gc * gc;
      float q = fmaf(g2, 1.014262858e-03f, -1.067757308e-01f);
      q = fmaf(q, g2, -2.301121361e+00f);
      const float cdf = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(q * gc));
      const float pdf = 0.39894228040143267794f * __builtin_amdgcn_exp2f(-0.72134752044448170368f * (g * g));
      o1[e] = (bf16_t)(d * (g * cdf));
      o2[e] = (bf16_t)(d * x * fmaf(g, pdf, cdf));
    }
    *reinterpret_cast<bf16x8*>(du + r * lddu + c) = o1;
    *reinterpret_cast<bf16x8*>(du + r * lddu + I + c) = o2;
  }
}
// b = alpha * a (fp32 -> fp32, may alias), c = (T) a
template <typename T>
__global__ __launch_bounds__(256) void k_scale_cast(const float* __restrict__ a, float alpha, float* __restrict__ b, T* __restrict__ c, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(a + i * 4);
    if (c) Vec4<T>::store(c + i * 4, v);
    if (b) *reinterpret_cast<f32x4*>(b + i * 4) = alpha * v;
  }
}
// out (fp32) = (float) in  [T -> f32 copy, e.g. cast grads]
template <typename T>
__global__ __launch_bounds__(256) void k_to_f32(const T* __restrict__ a, float* __restrict__ b, long n4, int accumulate) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 v = Vec4<T>::load(a + i * 4);
    if (accumulate) v += *reinterpret_cast<const f32x4*>(b + i * 4);
    *reinterpret_cast<f32x4*>(b + i * 4) = v;
  }
}

static inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}
// The kernels above move whole 4-element vectors of T: the width, every leading dimension and every pointer in units of 4 elements
// (16 bytes in fp32, 8 in bf16).  Checked here so the tower paths and the stand-alone entry points are refused alike, before any launch.
static inline bool ew_dtype_ok(int dt) { return dt == TTV_BF16 || dt == TTV_F32; }
static inline bool ew_ptr_ok(const void* p, int dt) { return p && (uintptr_t)p % (dt == TTV_BF16 ? 8 : 16) == 0; }
static inline bool ew_ld_ok(int ld, int width) { return ld >= width && ld % 4 == 0; }

int ttvk_gate_fwd(const void* a, int lda, const void* gate, int ldg, void* ag, int ldo, int rows, int d, int dt, hipStream_t s) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(ew_dtype_ok(dt) && rows > 0 && d > 0 && d % 4 == 0, "gate_fwd: dtype %d, %d rows, width %d (a positive multiple of 4)", dt, rows, d);
  TTV_CHECK_ARG(ew_ld_ok(lda, d) && ew_ld_ok(ldg, d) && ew_ld_ok(ldo, d), "gate_fwd: leading dimensions %d %d %d (>= %d, multiples of 4)", lda, ldg, ldo, d);
  TTV_CHECK_ARG(ew_ptr_ok(a, dt) && ew_ptr_ok(gate, dt) && ew_ptr_ok(ag, dt), "gate_fwd: null or not 4-element aligned pointer");
  const int nb = ew_blocks((long)rows * d / 4);
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_gate_fwd<bf16_t>), dim3(nb), dim3(256), 0, s, (const bf16_t*)a, lda, (const bf16_t*)gate, ldg, (bf16_t*)ag, ldo, rows, d);
  else hipLaunchKernelGGL((k_gate_fwd<float>), dim3(nb), dim3(256), 0, s, (const float*)a, lda, (const float*)gate, ldg, (float*)ag, ldo, rows, d);
  TTV_CHECK_LAUNCH("gate_fwd");
  return TTV_OK;
}
int ttvk_gate_bwd(const void* dag, int ldd, const void* a, int lda, const void* gate, int ldg, void* da, int ldda, void* dgate, int lddg,
                  int rows, int d, int dt, float* delta, hipStream_t s) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(ew_dtype_ok(dt) && rows > 0 && d > 0 && d % 4 == 0, "gate_bwd: dtype %d, %d rows, width %d (a positive multiple of 4)", dt, rows, d);
  TTV_CHECK_ARG(!delta || d % 64 == 0, "gate_bwd: delta needs whole 64-wide heads");
  TTV_CHECK_ARG(ew_ld_ok(ldd, d) && ew_ld_ok(lda, d) && ew_ld_ok(ldg, d) && ew_ld_ok(ldda, d) && ew_ld_ok(lddg, d),
                "gate_bwd: leading dimensions %d %d %d %d %d (>= %d, multiples of 4)", ldd, lda, ldg, ldda, lddg, d);
  TTV_CHECK_ARG(ew_ptr_ok(dag, dt) && ew_ptr_ok(a, dt) && ew_ptr_ok(gate, dt) && ew_ptr_ok(da, dt) && ew_ptr_ok(dgate, dt),
                "gate_bwd: null or not 4-element aligned pointer");
  const int nb = ew_blocks((long)rows * d / 4);
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_gate_bwd<bf16_t>), dim3(nb), dim3(256), 0, s, (const bf16_t*)dag, ldd, (const bf16_t*)a, lda, (const bf16_t*)gate, ldg, (bf16_t*)da, ldda, (bf16_t*)dgate, lddg, rows, d, delta);
  else hipLaunchKernelGGL((k_gate_bwd<float>), dim3(nb), dim3(256), 0, s, (const float*)dag, ldd, (const float*)a, lda, (const float*)gate, ldg, (float*)da, ldda, (float*)dgate, lddg, rows, d, delta);
  TTV_CHECK_LAUNCH("gate_bwd");
  return TTV_OK;
}
int ttvk_geglu_fwd(const void* u, int ldu, void* h, int ldh, int rows, int I, int dt, hipStream_t s) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(ew_dtype_ok(dt) && rows > 0 && I > 0 && I % 4 == 0, "geglu_fwd: dtype %d, %d rows, inner %d (a positive multiple of 4)", dt, rows, I);
  TTV_CHECK_ARG(ew_ld_ok(ldu, 2 * I) && ew_ld_ok(ldh, I), "geglu_fwd: leading dimensions %d (>= %d) %d (>= %d), multiples of 4", ldu, 2 * I, ldh, I);
  TTV_CHECK_ARG(ew_ptr_ok(u, dt) && ew_ptr_ok(h, dt), "geglu_fwd: null or not 4-element aligned pointer");
  const int nb = ew_blocks((long)rows * I / 4);
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_geglu_fwd<bf16_t>), dim3(nb), dim3(256), 0, s, (const bf16_t*)u, ldu, (bf16_t*)h, ldh, rows, I);
  else hipLaunchKernelGGL((k_geglu_fwd<float>), dim3(nb), dim3(256), 0, s, (const float*)u, ldu, (float*)h, ldh, rows, I);
  TTV_CHECK_LAUNCH("geglu_fwd");
  return TTV_OK;
}
int ttvk_geglu_bwd(const void* u, int ldu, const void* dh, int lddh, void* du, int lddu, int rows, int I, int dt, hipStream_t s) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(ew_dtype_ok(dt) && rows > 0 && I > 0 && I % 4 == 0, "geglu_bwd: dtype %d, %d rows, inner %d (a positive multiple of 4)", dt, rows, I);
  TTV_CHECK_ARG(ew_ld_ok(ldu, 2 * I) && ew_ld_ok(lddh, I) && ew_ld_ok(lddu, 2 * I),
                "geglu_bwd: leading dimensions %d %d %d (u, du >= %d, dh >= %d, multiples of 4)", ldu, lddh, lddu, 2 * I, I);
  TTV_CHECK_ARG(ew_ptr_ok(u, dt) && ew_ptr_ok(dh, dt) && ew_ptr_ok(du, dt), "geglu_bwd: null or not 4-element aligned pointer");
  const int nb = ew_blocks((long)rows * I / 4);
  static const bool exact = ttv_env_flag("TTV_GEGLU_BWD_ERF", false);      // A/B: the erff() form
  const bool v8 = !exact && I % 8 == 0 && ldu % 8 == 0 && lddh % 8 == 0 && lddu % 8 == 0 && ((uintptr_t)u % 16 == 0) && ((uintptr_t)dh % 16 == 0) && ((uintptr_t)du % 16 == 0);
  if (dt == TTV_BF16 && v8) hipLaunchKernelGGL(k_geglu_bwd_bf16, dim3(ew_blocks((long)rows * I / 8)), dim3(256), 0, s, (const bf16_t*)u, ldu, (const bf16_t*)dh, lddh, (bf16_t*)du, lddu, rows, I);
  else if (dt == TTV_BF16) hipLaunchKernelGGL((k_geglu_bwd<bf16_t>), dim3(nb), dim3(256), 0, s, (const bf16_t*)u, ldu, (const bf16_t*)dh, lddh, (bf16_t*)du, lddu, rows, I);
  else hipLaunchKernelGGL((k_geglu_bwd<float>), dim3(nb), dim3(256), 0, s, (const float*)u, ldu, (const float*)dh, lddh, (float*)du, lddu, rows, I);
  TTV_CHECK_LAUNCH("geglu_bwd");
  return TTV_OK;
}
int ttvk_scale_cast(const float* a, float alpha, float* b, void* c, int dt, long n, hipStream_t s) {
  if (n == 0) return TTV_OK;
  // the kernel walks n / 4 vectors: a tail of n % 4 elements would be left unwritten without a word
  TTV_CHECK_ARG(ew_dtype_ok(dt) && n > 0 && n % 4 == 0, "scale_cast: dtype %d, %ld elements (a positive multiple of 4)", dt, n);
  TTV_CHECK_ARG(ew_ptr_ok(a, TTV_F32) && (!b || ew_ptr_ok(b, TTV_F32)) && (!c || ew_ptr_ok(c, dt)), "scale_cast: null or not 4-element aligned pointer");
  const int nb = ew_blocks(n / 4);
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_scale_cast<bf16_t>), dim3(nb), dim3(256), 0, s, a, alpha, b, (bf16_t*)c, n / 4);
  else hipLaunchKernelGGL((k_scale_cast<float>), dim3(nb), dim3(256), 0, s, a, alpha, b, (float*)c, n / 4);
  TTV_CHECK_LAUNCH("scale_cast");
  return TTV_OK;
}
int ttvk_to_f32(const void* a, int dt, float* b, long n, int accumulate, hipStream_t s) {
  if (n == 0) return TTV_OK;
  TTV_CHECK_ARG(ew_dtype_ok(dt) && n > 0 && n % 4 == 0, "to_f32: dtype %d, %ld elements (a positive multiple of 4)", dt, n);
  TTV_CHECK_ARG(ew_ptr_ok(a, dt) && ew_ptr_ok(b, TTV_F32), "to_f32: null or not 4-element aligned pointer");
  const int nb = ew_blocks(n / 4);
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_to_f32<bf16_t>), dim3(nb), dim3(256), 0, s, (const bf16_t*)a, b, n / 4, accumulate);
  else hipLaunchKernelGGL((k_to_f32<float>), dim3(nb), dim3(256), 0, s, (const float*)a, b, n / 4, accumulate);
  TTV_CHECK_LAUNCH("to_f32");
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------ FSQ straight-through backward
struct FsqBwdDev { int n; float k[TTV_MAX_FSQ], shift[TTV_MAX_FSQ]; };
template <typename TG>
__global__ __launch_bounds__(256) void k_fsq_bwd(FsqBwdDev p, const float* __restrict__ z, const TG* __restrict__ dcodes,
                                                 float* __restrict__ dz, int rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * p.n) return;
  const int c = i % p.n;
  const float t = tanhf(z[i] + p.shift[c]);
  dz[i] = Cvt<TG>::to_f(dcodes[i]) * p.k[c] * (1.0f - t * t);
}
int ttvk_fsq_bwd(const ttv_fsq_params* fp, const float* z, const void* dcodes, int dt, float* dz, int rows, hipStream_t s) {
  if (rows == 0) return TTV_OK;
  FsqBwdDev p;
  p.n = fp->n;
  for (int i = 0; i < TTV_MAX_FSQ; ++i) {
    p.k[i] = i < fp->n ? fp->half_l[i] / fp->half_width[i] : 0.f;
    p.shift[i] = fp->shift[i];
  }
  const int nb = ttv_cdiv(rows * fp->n, 256);
  if (dt == TTV_BF16) hipLaunchKernelGGL((k_fsq_bwd<bf16_t>), dim3(nb), dim3(256), 0, s, p, z, (const bf16_t*)dcodes, dz, rows);
  else hipLaunchKernelGGL((k_fsq_bwd<float>), dim3(nb), dim3(256), 0, s, p, z, (const float*)dcodes, dz, rows);
  TTV_CHECK_LAUNCH("fsq_bwd");
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------ weight gradient GEMM
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_b;
__device__ __forceinline__ bf16x4 tr16(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_b*)p); }

// dW[N,K] (fp32, accumulated with atomics) += dY[L,N]^T X[L,K].  Block: 64 x 64 outputs, one token range (blockIdx.z).
// LDS tiles are row-major [64 tokens][64 cols] bf16 (128-byte rows); a fragment of 8 consecutive TOKENS for one column is
// two transposed reads of 4 tokens (lane 4q+p of a 16-lane group addresses token row q, columns 4p..4p+3).
__global__ __launch_bounds__(256) void k_wgrad_bf16(const bf16_t* __restrict__ dy, int lddy, const bf16_t* __restrict__ x, int ldx,
                                                    float* __restrict__ dw, int lddw, int L, int N, int K, int tokens_per_block) {
  __shared__ __attribute__((aligned(16))) uint4 ay[64 * 8];
  __shared__ __attribute__((aligned(16))) uint4 ax[64 * 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wk = wave >> 1;
  const int l15 = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
  const int t_begin = blockIdx.z * tokens_per_block;
  const int t_end = min(L, t_begin + tokens_per_block);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // staging: 512 chunks per tile, 2 per thread: token = (tid>>3) + 32*i, 16-byte chunk = tid & 7
  const int srow = tid >> 3, sc = tid & 7;
  const uint4 zero4 = {0u, 0u, 0u, 0u};
  const int gi = l15, tq = gi >> 2, tp = gi & 3;
  for (int t0 = t_begin; t0 < t_end; t0 += 64) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = t0 + srow + 32 * i;
      const bool ok = t < t_end;
      const int cn = n0 + sc * 8, ck = k0 + sc * 8;
      ay[(srow + 32 * i) * 8 + sc] = (ok && cn < N) ? *reinterpret_cast<const uint4*>(dy + (size_t)t * lddy + cn) : zero4;
      ax[(srow + 32 * i) * 8 + sc] = (ok && ck < K) ? *reinterpret_cast<const uint4*>(x + (size_t)t * ldx + ck) : zero4;
    }
    __syncthreads();
    const char* by = reinterpret_cast<const char*>(ay);
    const char* bx = reinterpret_cast<const char*>(ax);
#pragma unroll
    for (int st = 0; st < 2; ++st) {   // 32 tokens per MFMA k-step
      const int trow = st * 32 + kq * 8 + tq;
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int col = wn * 32 + i * 16 + tp * 4;
        const bf16x4 lo = tr16(by + trow * 128 + col * 2), hi = tr16(by + (trow + 4) * 128 + col * 2);
        a[i] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = wk * 32 + j * 16 + tp * 4;
        const bf16x4 lo = tr16(bx + trow * 128 + col * 2), hi = tr16(bx + (trow + 4) * 128 + col * 2);
        b[j] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // C layout: col = lane&15 -> B column = k index; row = 4*kq + reg -> A row = n index
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = k0 + wk * 32 + j * 16 + l15;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int nn = n0 + wn * 32 + i * 16 + kq * 4 + e;
        if (nn < N && kk < K) atomicAdd(dw + (size_t)nn * lddw + kk, acc[i][j][e]);
      }
    }
}

// 128 x 128 outputs per block (64 x 64 per wave: every transposed fragment read feeds four MFMAs), 64 tokens per step.
// Tiles are staged by LDS-DMA into two stages of [64 tokens][128 cols] bf16 (256-byte rows = one bank row).  A transposed
// read addresses, per 32-lane half, 8 token rows x 32 bytes in the same columns: the 32-byte column pair of row r is stored
// at pair index ^ g(r), g(r) = (r & 3) | ((r >> 3) & 1) << 2, so the 8 rows of a half land on 8 different pairs (conflict-free).
// The DMA writes LDS linearly per lane, so the swizzle is applied on the global side (lane fetches the chunk that belongs at
// its LDS position).  Columns past N / K fetch a valid chunk instead (they only feed outputs that are never written); token
// rows past the range are re-fetched from the last valid row and zeroed in LDS before the barrier.
#define WG_STAGE_BYTES 32768
#define WG_OP_BYTES 16384
//
// PARTIAL: instead of fp32 atomics (which retire ~1 element per clock per L2 channel and dominate short token ranges) every
// block stores its 128 x 128 fp32 tile in fragment order (each wave instruction writes 1 KB contiguous) to
// part[(tile * splits + split)][wave][i][j][lane][4]; k_wgrad_reduce sums the splits in a fixed order and adds into dW, so
// the result is also bit-reproducible from run to run.
// Round 5: loader waves.  A wave can issue one 1 KB global_load_lds_dwordx4 per ~105 - 140 cycles at best (tools/ubench/dma_rates.hip),
// and the round-4 loop had every compute wave issue eight of them per 64-token stage in front of its 32 MFMAs (512 cycles): ~2 200
// cycles per stage and block, two blocks per CU (a deeper ring alone changed nothing: profiles/r05_negative_results.txt).  Now a block
// has 4 + WG_NL waves: waves 0-3 compute as before (64 x 64 outputs each; per 32-token sub-step 16 MFMAs with the 16 transposed
// fragment reads of the NEXT sub-step under the first eight of them), the others only stage - loader w issues the instructions of
// its 64 / WG_NL token rows of the stage WG_RING - 1 ahead, waits for the stage one ahead (counted: the younger stages stay in flight),
// zeroes its rows past the token range and joins the block's one barrier per stage.  One block per CU (128 KB of ring), ~800 cycles
// per stage on every CU instead of ~1 085 (2 170 / 2 blocks), and a lone block per CU - grids of fewer blocks than 2 per CU, which is
// what the split plan produces - no longer runs at half speed: w12 57 -> 39 us, the others 30 - 34 -> 25 - 26 us, training step
// 7.10 -> 6.97 ms (profiles/r05_wgrad_loader_waves.txt).  Measured on the way: 4 and 8 loader waves are equal (the ring is not what the
// compute waves wait for); a 3-slot ring (one stage of lead) exposes the load latency (w12 58 us); operands re-read from L2 only are
// no faster, so the remaining ~290 cycles per stage above the MFMAs are the block-wide barrier and its drain (tools/wgrad_stamps.py).
// Same MFMA sequence per accumulator as before (a partial tile over the same token range has the round-4 kernel's bits; the split plan
// - and with it the order of the fp32 sum over ranges - changed with the one-block-per-CU grid).
#ifndef WG_RING
#define WG_RING 4           // ring slots (3 or 4): the loaders run WG_RING - 2 stages ahead of the stage the compute waves prefetch from
#endif
#ifndef WG_NL
#define WG_NL 4            // loader waves per block (4 or 8: equal speed)
#endif
#ifdef WG_L2TEST               // diagnostic build: every stage re-reads the block's first four (cache-resident operands; results wrong)
#define WG_SRC_STAGE(s_) ((s_) & 3)
#else
#define WG_SRC_STAGE(s_) (s_)
#endif
#ifndef WG_KO
#define WG_KO 0           // diagnostic knock-outs (results wrong): 1 no MFMAs, 2 no fragment reads, 4 no DMA
#endif
#define WG_NI (16 / WG_NL)
#ifdef WG_STAMPS              // diagnostic build (tools/wgrad_stamps.sh): s_memtime sums per segment and wave of every 37th block
__device__ long long* g_wg_stamps_dev;
#define WG_STAMP_DECL unsigned long long st_prev__ = 0, st_acc__[4] = {0, 0, 0, 0}
#define WG_STAMP_START()                                                                               \
  do {                                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_prev__)::"memory");                  \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  } while (0)
#define WG_STAMP(seg_)                                                                                 \
  do {                                                                                                 \
    unsigned long long t__;                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");                        \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
    st_acc__[seg_] += t__ - st_prev__;                                                                 \
    st_prev__ = t__;                                                                                   \
  } while (0)
#define WG_STAMP_OUT()                                                                                 \
  do {                                                                                                 \
    if (g_wg_stamps_dev && blockIdx.x % 37 == 0 && lane == 0) {                                        \
      unsigned long long rt1__;                                                                        \
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt1__)::"memory");               \
      long long* o__ = g_wg_stamps_dev + ((size_t)(blockIdx.x / 37) * (4 + WG_NL) + wave8) * 8;        \
      for (int i__ = 0; i__ < 4; ++i__) o__[i__] = (long long)st_acc__[i__];                           \
      o__[4] = (long long)(rt1__ - rt0__);                                                             \
      o__[5] = n_stages;                                                                               \
    }                                                                                                  \
  } while (0)
#else
#define WG_STAMP_DECL
#define WG_STAMP_START()
#define WG_STAMP(seg_)
#define WG_STAMP_OUT()
#endif   // DMA instructions per operand, loader and stage (4 token rows each)
template <bool PARTIAL>
__global__ __launch_bounds__(256 + 64 * WG_NL, 1) void k_wgrad128_bf16(const bf16_t* __restrict__ dy, int lddy, const bf16_t* __restrict__ x, int ldx,
                                                          float* __restrict__ dw, int lddw, int L, int N, int K, int tokens_per_block,
                                                          float* __restrict__ part, int tiles_n, int tiles_k, int splits) {
  extern __shared__ __attribute__((aligned(16))) char wg[];      // WG_RING stages of WG_STAGE_BYTES
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wave8 >= 4;
  const int wave = loader ? wave8 - 4 : wave8;   // loader index / compute wave
  const int wn = wave & 1, wk = wave >> 1;
  const int l15 = lane & 15, kq = lane >> 4, tq = l15 >> 2, tp = l15 & 3;
  // XCD-aware work mapping: consecutive block ids go round-robin over the 8 XCDs (each with its own L2), so the token range
  // (split) is taken from id % 8 and the tile from id / 8: all tiles of one split run on ONE XCD at about the same time and the
  // dY / X rows they share are fetched from HBM / MALL once and re-read from that L2 (splits is a multiple of 8 when > 8).
  const int tiles = tiles_n * tiles_k;
  int split, tile;
  if (splits >= 8) {
    const int slot = blockIdx.x >> 3;
    split = (blockIdx.x & 7) + 8 * (slot / tiles);
    tile = slot % tiles;
  } else {
    split = blockIdx.x / tiles;
    tile = blockIdx.x % tiles;
  }
  if (split >= splits) return;
  const int n0 = (tile % tiles_n) * 128, k0 = (tile / tiles_n) * 128;
  const int t_begin = split * tokens_per_block;
  const int t_end = min(L, t_begin + tokens_per_block);
  if (!PARTIAL && t_begin >= t_end) return;
  const uint32_t wg_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&wg[0];
  const int n_stages = t_begin < t_end ? (t_end - t_begin + 63) / 64 : 0;

  if (loader) {
    // ================= loader waves: stage s -> ring slot s % WG_RING =================
    // DMA lane mapping: instruction i of loader w covers tile rows 4*(4w+i) .. +3 (lane>>4 picks the row), LDS chunk = lane&15
    uint32_t voy[WG_NI], vox[WG_NI];
    int cy[WG_NI], cx[WG_NI];
#pragma unroll
    for (int i = 0; i < WG_NI; ++i) {
      const int g = kq | ((((wave * WG_NI + i) >> 1) & 1) << 2);
      const int ch = l15 ^ (g << 1);
      cy[i] = (n0 + ch * 8 < N) ? ch * 8 : 0;
      cx[i] = (k0 + ch * 8 < K) ? ch * 8 : 0;
      const int r = (wave * WG_NI + i) * 4 + kq;
      voy[i] = (uint32_t)(r * lddy + cy[i]) * 2u;
      vox[i] = (uint32_t)(r * ldx + cx[i]) * 2u;
    }
#define WG_DMA(voff_, base_, dst_)                                                                              \
  do {                                                                                                          \
    unsigned keep__;                                                                                            \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep__) : "v"(voff_), "s"(base_), "s"(dst_) : "memory");                                \
  } while (0)
    // the loader's eight instructions of stage s_ (first token t_begin + 64 s_); stages past the range are not issued
#define WG_ISSUE(s_)                                                                                            \
  do {                                                                                                          \
    if ((s_) < n_stages) {                                                                                      \
      const int t0__ = t_begin + 64 * WG_SRC_STAGE(s_);                                                         \
      const bf16_t* by__ = dy + (size_t)t0__ * lddy + n0;                                                       \
      const bf16_t* bx__ = x + (size_t)t0__ * ldx + k0;                                                         \
      const int last__ = t_end - 1 - t0__;                                                                      \
      _Pragma("unroll") for (int i__ = 0; i__ < WG_NI; ++i__) {                                                     \
        const uint32_t dst__ = wg_lds + ((s_) % WG_RING) * WG_STAGE_BYTES + (wave * WG_NI + i__) * 1024;      \
        uint32_t vy__ = voy[i__], vx__ = vox[i__];                                                              \
        if (last__ < 63) {                                                                                      \
          const int r__ = min((wave * WG_NI + i__) * 4 + kq, last__);                                               \
          vy__ = (uint32_t)(r__ * lddy + cy[i__]) * 2u;                                                         \
          vx__ = (uint32_t)(r__ * ldx + cx[i__]) * 2u;                                                          \
        }                                                                                                       \
        if (!(WG_KO & 4)) {                                                                                     \
          WG_DMA(vy__, by__, dst__);                                                                            \
          WG_DMA(vx__, bx__, dst__ + WG_OP_BYTES);                                                              \
        }                                                                                                       \
      }                                                                                                         \
    }                                                                                                           \
  } while (0)
    // rows of stage s_ past the token range (both operands; the loader zeroes the rows it fetched, after its own wait for them)
#define WG_ZERO_TAIL(s_)                                                                                        \
  do {                                                                                                          \
    if ((s_) < n_stages && t_end - (t_begin + 64 * (s_)) < 64) {                                                \
      _Pragma("unroll") for (int i__ = 0; i__ < WG_NI; ++i__) {                                                     \
        const int r__ = (wave * WG_NI + i__) * 4 + kq;                                                              \
        if (t_begin + 64 * (s_) + r__ >= t_end) {                                                               \
          char* d__ = wg + ((s_) % WG_RING) * WG_STAGE_BYTES + r__ * 256 + l15 * 16;                      \
          *reinterpret_cast<uint4*>(d__) = make_uint4(0u, 0u, 0u, 0u);                                          \
          *reinterpret_cast<uint4*>(d__ + WG_OP_BYTES) = make_uint4(0u, 0u, 0u, 0u);                            \
        }                                                                                                       \
      }                                                                                                         \
    }                                                                                                           \
  } while (0)
    WG_ISSUE(0);
    WG_ISSUE(1);
    if (WG_RING == 4) WG_ISSUE(2);
    WG_STAMP_DECL;
#ifdef WG_STAMPS
    unsigned long long rt0__;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt0__)::"memory");
#endif
    if (n_stages > 0) {
      // stages 0 and 1 complete for this loader (stage 2's eight instructions, if issued, stay in flight)
      if (WG_RING == 4 && n_stages > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * WG_NI) : "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      WG_ZERO_TAIL(0);
      WG_ZERO_TAIL(1);
      __syncthreads();                        // barrier P: stages 0, 1 complete
    }
    WG_STAMP_START();
    for (int st = 0; st < n_stages; ++st) {
      if (st > 0) {
        // stage st+1 complete (issued two stages ago); stage st+2's instructions - if that stage exists - stay in flight
        if (WG_RING == 4 && st + 2 < n_stages) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * WG_NI) : "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        WG_STAMP(0);
        WG_ZERO_TAIL(st + 1);
        __syncthreads();                      // barrier st: stages <= st+1 complete; the compute waves have left stage st-1
        WG_STAMP(1);
      }
      WG_ISSUE(st + WG_RING - 1);             // into the slot of stage st-1
      WG_STAMP(2);
    }
    WG_STAMP_OUT();
#undef WG_ZERO_TAIL
#undef WG_ISSUE
#undef WG_DMA
    return;
  }

  // ================= compute waves =================
  // fragment read offsets: token row = 32*st + 8*kq + tq (+4 for the upper half of the 8 tokens), g is the same for all of them
  const int g2 = tq | ((kq & 1) << 2);
  const int rowoff = (kq * 8 + tq) * 256 + (tp & 1) * 8;
  int offa[4], offb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    offa[i] = rowoff + (((wn * 8 + i * 2 + (tp >> 1)) ^ (g2 << 1)) << 4);
    offb[i] = rowoff + (((wk * 8 + i * 2 + (tp >> 1)) ^ (g2 << 1)) << 4) + WG_OP_BYTES;
  }
  // the 16 transposed reads of one sub-step (st_ = 0 / 1) of the stage at sb_ -> a_[4], b_[4]
#define WG_FRAGS(sb_, st_, a_, b_)                                                                              \
  do {                                                                                                          \
    _Pragma("unroll") for (int j__ = 0; j__ < 4; ++j__) {                                                       \
      const bf16x4 lo__ = tr16((sb_) + (st_) * 8192 + offb[j__]), hi__ = tr16((sb_) + (st_) * 8192 + 1024 + offb[j__]); \
      b_[j__] = (bf16x8){lo__[0], lo__[1], lo__[2], lo__[3], hi__[0], hi__[1], hi__[2], hi__[3]};               \
    }                                                                                                           \
    _Pragma("unroll") for (int i__ = 0; i__ < 4; ++i__) {                                                       \
      const bf16x4 lo__ = tr16((sb_) + (st_) * 8192 + offa[i__]), hi__ = tr16((sb_) + (st_) * 8192 + 1024 + offa[i__]); \
      a_[i__] = (bf16x8){lo__[0], lo__[1], lo__[2], lo__[3], hi__[0], hi__[1], hi__[2], hi__[3]};               \
    }                                                                                                           \
  } while (0)
  // one sub-step's 16 MFMAs with the 16 reads of the next one under the first eight of them (two per gap, the B fragments - which
  // the next sub-step's first four MFMAs need - first): every read has a full LDS latency of matrix work behind it
#define WG_GAPS()                                                                                               \
  do {                                                                                                          \
    _Pragma("unroll") for (int g__ = 0; g__ < 8; ++g__) {                                                       \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                        \
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                        \
    }                                                                                                           \
    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                                          \
  } while (0)

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  bf16x8 a0[4], b0[4], a1[4], b1[4];
  if (n_stages > 0) {
    __syncthreads();                          // barrier P
    WG_FRAGS(wg, 0, a0, b0);
  }
  WG_STAMP_DECL;
#ifdef WG_STAMPS
  unsigned long long rt0__;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt0__)::"memory");
#endif
  WG_STAMP_START();
  for (int st = 0; st < n_stages; ++st) {
    const char* sb = wg + (st % WG_RING) * WG_STAGE_BYTES;
    const char* sn = wg + ((st + 1) % WG_RING) * WG_STAGE_BYTES;
    if (st > 0) __syncthreads();              // barrier st (sub-step 0's fragments of this stage are already in a0 / b0)
    WG_STAMP(0);
    // sub-step 0 | reads of sub-step 1
    if (!(WG_KO & 2)) WG_FRAGS(sb, 1, a1, b1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (!(WG_KO & 1)) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0[j], acc[i][j], 0, 0, 0);
    }
    WG_GAPS();
    WG_STAMP(1);
    // sub-step 1 | reads of the next stage's sub-step 0 (that stage was complete at this stage's barrier)
    // (behind the last stage this reads a ring slot nobody filled: the values are not used)
    if (!(WG_KO & 2)) WG_FRAGS(sn, 0, a0, b0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (!(WG_KO & 1)) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
    }
    WG_GAPS();
    WG_STAMP(2);
  }
  WG_STAMP_OUT();
#undef WG_GAPS
#undef WG_FRAGS
  if (PARTIAL) {
    const size_t blk = (size_t)tile * splits + split;
    f32x4* dst = reinterpret_cast<f32x4*>(part) + blk * 4096 + wave * 1024 + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[(i * 4 + j) * 64] = acc[i][j];
    return;
  }
  // C layout: col = lane&15 -> B column = k index; row = 4*kq + reg -> A row = n index
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = k0 + wk * 64 + j * 16 + l15;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int nn = n0 + wn * 64 + i * 16 + kq * 4 + e;
        if (nn < N && kk < K) atomicAdd(dw + (size_t)nn * lddw + kk, acc[i][j][e]);
      }
    }
}

// dW += sum over splits of the partial tiles of k_wgrad128_bf16<true>.  A block owns 64 float4 of a tile (one fragment: 4
// consecutive n at one k per lane); its four waves each sum a quarter of the splits (8 independent loads in flight), the
// quarters are combined through LDS in a fixed order.  64 blocks per tile.
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ part, int splits, float* __restrict__ dw, int lddw, int N,
                                                      int K, int tiles_n) {
  __shared__ f32x4 red[3][64];
  const int tile = blockIdx.x >> 6, frag = blockIdx.x & 63, lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int wave = frag >> 4, i = (frag >> 2) & 3, j = frag & 3, l15 = lane & 15, kq = lane >> 4;
  const int per = (splits + 3) >> 2;
  const int s0 = grp * per, s1 = min(splits, s0 + per);
  const f32x4* src = reinterpret_cast<const f32x4*>(part) + (size_t)tile * splits * 4096 + frag * 64 + lane;
  f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
  int sp = s0;
  for (; sp + 8 <= s1; sp += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(sp + u) * 4096];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  for (; sp < s1; ++sp) sum += src[(size_t)sp * 4096];
  if (grp) red[grp - 1][lane] = sum;
  __syncthreads();
  if (grp) return;
  sum += red[0][lane];
  sum += red[1][lane];
  sum += red[2][lane];
  const int n0 = (tile % tiles_n) * 128, k0 = (tile / tiles_n) * 128;
  const int kk = k0 + (wave >> 1) * 64 + j * 16 + l15;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int nn = n0 + (wave & 1) * 64 + i * 16 + kq * 4 + e;
    if (nn < N && kk < K) dw[(size_t)nn * lddw + kk] += sum[e];
  }
}

// The same sum for up to TTV_WGRAD_BATCH weight gradients in one launch (ttvk_wgrad_flush): block -> (entry, tile, fragment) through the
// entries' block prefix; arithmetic and order per element are k_wgrad_reduce's (bit-identical gradients).  At the reference's batch
// sizes a reduce launch is ~7.5 us of latency for microseconds of work and a training step had 34 of them.
struct WgradBatchDev {
  int n;
  int first_block[TTV_WGRAD_BATCH + 1];
  WgradBatch::Entry e[TTV_WGRAD_BATCH];
};
__global__ __launch_bounds__(256) void k_wgrad_reduce_multi(WgradBatchDev b) {
  __shared__ f32x4 red[3][64];
  int ei = 0;
#pragma unroll
  for (int i = 1; i < TTV_WGRAD_BATCH; ++i)
    if (i < b.n && (int)blockIdx.x >= b.first_block[i]) ei = i;
  const WgradBatch::Entry en = b.e[ei];
  const int blk = blockIdx.x - b.first_block[ei];
  const int tile = blk >> 6, frag = blk & 63, lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int wave = frag >> 4, i = (frag >> 2) & 3, j = frag & 3, l15 = lane & 15, kq = lane >> 4;
  const int splits = en.splits;
  const int per = (splits + 3) >> 2;
  const int s0 = grp * per, s1 = min(splits, s0 + per);
  const f32x4* src = reinterpret_cast<const f32x4*>(en.part) + (size_t)tile * splits * 4096 + frag * 64 + lane;
  f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
  int sp = s0;
  for (; sp + 8 <= s1; sp += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(sp + u) * 4096];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  for (; sp < s1; ++sp) sum += src[(size_t)sp * 4096];
  if (grp) red[grp - 1][lane] = sum;
  __syncthreads();
  if (grp) return;
  sum += red[0][lane];
  sum += red[1][lane];
  sum += red[2][lane];
  const int n0 = (tile % en.tiles_n) * 128, k0 = (tile / en.tiles_n) * 128;
  const int kk = k0 + (wave >> 1) * 64 + j * 16 + l15;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int nn = n0 + (wave & 1) * 64 + i * 16 + kq * 4 + e;
    if (nn < en.N && kk < en.K) en.dw[(size_t)nn * en.lddw + kk] += sum[e];
  }
}

int ttvk_wgrad_flush(WgradBatch* batch, hipStream_t s) {
  if (!batch || batch->n == 0) return TTV_OK;
  WgradBatchDev d = {};
  d.n = batch->n;
  int blocks = 0;
  for (int i = 0; i < batch->n; ++i) {
    d.first_block[i] = blocks;
    d.e[i] = batch->e[i];
    blocks += batch->e[i].tiles * 64;
  }
  d.first_block[batch->n] = blocks;
  hipLaunchKernelGGL(k_wgrad_reduce_multi, dim3(blocks), dim3(256), 0, s, d);
  batch->n = 0;
  batch->used_bytes = 0;
  TTV_CHECK_LAUNCH("wgrad_reduce_multi");
  return TTV_OK;
}

// naive fp32 variant (gradient checks): thread per output element, block 16 x 16, token range per blockIdx.z
__global__ __launch_bounds__(256) void k_wgrad_f32(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                                   float* __restrict__ dw, int lddw, int L, int N, int K, int tokens_per_block) {
  __shared__ float sy[32][17], sx[32][17];
  const int tn = threadIdx.x & 15, tk = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + tn, k = blockIdx.y * 16 + tk;
  const int t_begin = blockIdx.z * tokens_per_block, t_end = min(L, t_begin + tokens_per_block);
  float acc = 0.f;
  for (int t0 = t_begin; t0 < t_end; t0 += 32) {
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256) {
      const int r = i >> 4, c = i & 15, t = t0 + r;
      sy[r][c] = (t < t_end && blockIdx.x * 16 + c < N) ? dy[(size_t)t * lddy + blockIdx.x * 16 + c] : 0.f;
      sx[r][c] = (t < t_end && blockIdx.y * 16 + c < K) ? x[(size_t)t * ldx + blockIdx.y * 16 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) acc = fmaf(sy[r][tn], sx[r][tk], acc);
  }
  if (n < N && k < K) atomicAdd(dw + (size_t)n * lddw + k, acc);
}

static int wgrad_target_blocks() {
  static const int v = ttv_env_int("TTV_WGRAD_BLOCKS", 200);
  return v < 1 ? 1 : v;
}
static int wgrad_min_steps() {
  static const int v = ttv_env_int("TTV_WGRAD_MIN_STEPS", 16);
  return v < 1 ? 1 : v;
}
static void wgrad_plan(int L, int N, int K, int* splits, int* tpb) {
  const int nb = ttv_cdiv(N, 128) * ttv_cdiv(K, 128);
  // token ranges: a multiple of 8 (one per XCD and round), about wgrad_target_blocks() blocks in all - the per-block tile
  // write-out is the fixed cost, and the kernel runs ONE block per CU (its ring is 128 KB of LDS): the rounding below must stay
  // under 256 blocks or a second, nearly empty round follows (200: 176 - 192 blocks at the tiny tower's shapes; 256 and two blocks per
  // CU before round 5, tools/wgrad_plan_sweep.sh)
  int sp = 8 * ((wgrad_target_blocks() + 4 * nb) / (8 * nb));
  // ... and a block should have wgrad_min_steps() 64-token steps to amortise its 64 KB partial tile (written here, read again by the sum)
  const int cap = 8 * (L / (64 * wgrad_min_steps() * 8));
  if (sp > cap) sp = cap;
  if (sp < 8) sp = 8;
  if (sp > ttv_cdiv(L, 64)) sp = ttv_cdiv(L, 64);
  if (sp < 1) sp = 1;
  *tpb = ttv_cdiv(ttv_cdiv(L, sp), 64) * 64;
  *splits = ttv_cdiv(L, *tpb);
}
int64_t ttvk_wgrad_ws_bytes(int L, int N, int K) {
  if (L <= 0 || N <= 0 || K <= 0) return 0;
  int splits, tpb;
  wgrad_plan(L, N, K, &splits, &tpb);
  return (int64_t)ttv_cdiv(N, 128) * ttv_cdiv(K, 128) * splits * 65536;
}

int ttvk_wgrad(const void* dy, int lddy, const void* x, int ldx, float* dw, int lddw, int L, int N, int K, int dt, float* part,
               int64_t part_bytes, hipStream_t s, WgradBatch* batch) {
  if (L == 0 || N == 0 || K == 0 || !dw) return TTV_OK;   // dw == NULL: frozen weight
  static const bool batch_env = ttv_env_flag("TTV_WGRAD_BATCHED", true);   // A/B
  if (!batch_env && batch) { TTV_TRY(ttvk_wgrad_flush(batch, s)); batch = nullptr; }
  const bool det = ttv_det();
  if (dt == TTV_BF16 && N % 8 == 0 && K % 8 == 0 && lddy % 8 == 0 && ldx % 8 == 0) {
    // TTV_WGRAD_TILE64 is on when merely present, whatever its value: only a set variable reads the same under two defaults
    static const int wg_tile64 = ttv_env_int("TTV_WGRAD_TILE64", 0) == ttv_env_int("TTV_WGRAD_TILE64", 1) ? 1 : 0;
    if (!wg_tile64 && ((uintptr_t)dy % 16 == 0) && ((uintptr_t)x % 16 == 0)) {
      int splits, tpb;
      wgrad_plan(L, N, K, &splits, &tpb);
      const int tn = ttv_cdiv(N, 128), tk = ttv_cdiv(K, 128);
      // 128 KB of dynamic LDS (the 4-slot ring): above the 64 KB a launch gets without asking - once per device of this process
      static bool ring_attr[16] = {};
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16 || !ring_attr[dev]) {
        if (hipFuncSetAttribute((const void*)k_wgrad128_bf16<true>, hipFuncAttributeMaxDynamicSharedMemorySize, WG_RING * WG_STAGE_BYTES) != hipSuccess ||
            hipFuncSetAttribute((const void*)k_wgrad128_bf16<false>, hipFuncAttributeMaxDynamicSharedMemorySize, WG_RING * WG_STAGE_BYTES) != hipSuccess) {
          ttv_set_error("wgrad: %d bytes of dynamic LDS refused", WG_RING * WG_STAGE_BYTES);
          return TTV_ERR_LAUNCH;
        }
        if (dev >= 0 && dev < 16) ring_attr[dev] = true;
      }
#ifdef WG_STAMPS
      { extern long long* g_ttv_stamps; long long* p__ = g_ttv_stamps; (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_wg_stamps_dev), &p__, sizeof(p__), 0, hipMemcpyHostToDevice, s); }
#endif
      dim3 grid(tn * tk * (splits >= 8 ? 8 * ttv_cdiv(splits, 8) : splits));
      const int64_t need = (int64_t)tn * tk * splits * 65536;
      if (batch && part && ((uintptr_t)part % 16 == 0) && (batch->n == TTV_WGRAD_BATCH || batch->used_bytes + need > part_bytes))
        TTV_TRY(ttvk_wgrad_flush(batch, s));        // does not fit behind what is pending: sum that first, start over at the scratch's base
      if (batch && part && ((uintptr_t)part % 16 == 0) && batch->used_bytes + need <= part_bytes) {
        float* mine = reinterpret_cast<float*>(reinterpret_cast<char*>(part) + batch->used_bytes);
        hipLaunchKernelGGL(k_wgrad128_bf16<true>, grid, dim3(256 + 64 * WG_NL), WG_RING * WG_STAGE_BYTES, s, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, dw, lddw, L, N, K,
                           tpb, mine, tn, tk, splits);
        WgradBatch::Entry& en = batch->e[batch->n++];
        en.part = mine; en.dw = dw; en.splits = splits; en.lddw = lddw; en.N = N; en.K = K; en.tiles_n = tn; en.tiles = tn * tk;
        batch->used_bytes += need;
      } else if (part && part_bytes >= need && ((uintptr_t)part % 16 == 0)) {
        if (batch) TTV_TRY(ttvk_wgrad_flush(batch, s));
        hipLaunchKernelGGL(k_wgrad128_bf16<true>, grid, dim3(256 + 64 * WG_NL), WG_RING * WG_STAGE_BYTES, s, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, dw, lddw, L, N, K,
                           tpb, part, tn, tk, splits);
        hipLaunchKernelGGL(k_wgrad_reduce, dim3(tn * tk * 64), dim3(256), 0, s, part, splits, dw, lddw, N, K, tn);
      } else if (det) {
        // no room for partial tiles: one token range per output tile, so that the kernel's atomicAdd is the address's only writer
        hipLaunchKernelGGL(k_wgrad128_bf16<false>, dim3(tn * tk),dim3(256 + 64 * WG_NL), WG_RING * WG_STAGE_BYTES, s, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, dw, lddw, L, N, K,
                           ttv_cdiv(L, 64) * 64, nullptr, tn, tk, 1);
      } else {
        hipLaunchKernelGGL(k_wgrad128_bf16<false>, grid, dim3(256 + 64 * WG_NL), WG_RING * WG_STAGE_BYTES, s, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, dw, lddw, L, N, K,
                           tpb, nullptr, tn, tk, splits);
      }
    } else {
      const int nb = ttv_cdiv(N, 64) * ttv_cdiv(K, 64);
      int splits = ttv_cdiv(2048, nb);   // aim at >= 2048 blocks
      if (splits > ttv_cdiv(L, 64)) splits = ttv_cdiv(L, 64);
      if (splits < 1 || det) splits = 1;   // deterministic mode: a single writer per address
      const int tpb = ttv_cdiv(ttv_cdiv(L, splits), 64) * 64;
      dim3 grid(ttv_cdiv(N, 64), ttv_cdiv(K, 64), ttv_cdiv(L, tpb));
      hipLaunchKernelGGL(k_wgrad_bf16, grid, dim3(256), 0, s, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, dw, lddw, L, N, K, tpb);
    }
  } else if (dt == TTV_F32) {
    const int tpb = det ? L : 1024;      // deterministic mode: grid.z = 1, a single writer per address
    dim3 grid(ttv_cdiv(N, 16), ttv_cdiv(K, 16), ttv_cdiv(L, tpb));
    hipLaunchKernelGGL(k_wgrad_f32, grid, dim3(256), 0, s, (const float*)dy, lddy, (const float*)x, ldx, dw, lddw, L, N, K, tpb);
  } else {
    ttv_set_error("wgrad: bf16 needs N, K and leading dims multiples of 8");
    return TTV_ERR_INVALID;
  }
  TTV_CHECK_LAUNCH("wgrad");
  return TTV_OK;
}

// small-N / small-K linear backward helpers for the d <-> token_size projections (encoder proj_out [C,d], decoder proj_in [d,C])
// dW[c, f] += sum_r a[r, c] * b[r, f]  (a: [rows, C] fp32 or T with C <= 8;  b: [rows, d]) ; one wave per row chunk
// DET: dw is the [row block][C][d] partial array (lddw and transpose_out are the fold's business)
template <typename TA, typename TB, bool DET>
__global__ __launch_bounds__(256) void k_outer_small(const TA* __restrict__ a, int lda, int C, const TB* __restrict__ b, int ldb,
                                                     const int* __restrict__ b_rows, float* __restrict__ dw, int lddw, int transpose_out,
                                                     int rows, int d, int rows_per_block) {
  // thread -> feature f (d <= 1024: loop), accumulates C partial sums over the block's rows; four rows in flight (the row loop was one
  // dependent load -> fma chain per row: ~36 us per launch at any batch size)
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  for (int f = threadIdx.x; f < d; f += 256) {
    float acc[TTV_MAX_FSQ];
#pragma unroll
    for (int c = 0; c < TTV_MAX_FSQ; ++c) acc[c] = 0.f;
    for (int r = r0; r < r1; r += 4) {
      float bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + u < r1 ? r + u : r1 - 1;
        bv[u] = r + u < r1 ? Cvt<TB>::to_f(b[(size_t)(b_rows ? b_rows[rr] : rr) * ldb + f]) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + u < r1 ? r + u : r1 - 1;
#pragma unroll
        for (int c = 0; c < TTV_MAX_FSQ; ++c)
          if (c < C) acc[c] += Cvt<TA>::to_f(a[(size_t)rr * lda + c]) * bv[u];
      }
    }
#pragma unroll
    for (int c = 0; c < TTV_MAX_FSQ; ++c)
      if (c < C) {
        if (DET) dw[((size_t)blockIdx.x * C + c) * d + f] = acc[c];
        else atomicAdd(transpose_out ? dw + (size_t)f * lddw + c : dw + (size_t)c * lddw + f, acc[c]);
      }
  }
}

#define OUTER_SMALL_RPB 32
int64_t ttvk_det_outer_small_bytes(int rows, int C, int d) {
  if (rows <= 0 || C <= 0 || d <= 0) return 0;
  return (int64_t)ttv_cdiv(rows, OUTER_SMALL_RPB) * (C < TTV_MAX_FSQ ? C : TTV_MAX_FSQ) * d * 4;
}

int ttvk_outer_small(const void* a, int a_dt, int lda, int C, const void* b, int b_dt, int ldb, const int* b_rows, float* dw, int lddw,
                     int transpose_out, int rows, int d, hipStream_t s, const DetScratch* scratch) {
  if (rows == 0 || !dw) return TTV_OK;
  TTV_CHECK_ARG(C >= 1 && C <= TTV_MAX_TOKEN, "outer_small: C");
  const int rpb = OUTER_SMALL_RPB;
  dim3 grid(ttv_cdiv(rows, rpb));
  const bool det = ttv_det();
  if (det) TTV_CHECK_DET(scratch, ttvk_det_outer_small_bytes(rows, C, d), "outer_small");
  // the kernel keeps TTV_MAX_FSQ partial sums per thread: wider tokens (the L2 quantiser's, up to TTV_MAX_TOKEN) go in column chunks
  // (deterministic mode: each chunk's partials through the same scratch, its fold in front of the next chunk's launch)
  for (int c0 = 0; c0 < C; c0 += TTV_MAX_FSQ) {
    const int cn = C - c0 < TTV_MAX_FSQ ? C - c0 : TTV_MAX_FSQ;
    float* dwc = transpose_out ? dw + c0 : dw + (size_t)c0 * lddw;
#define OS_(TA, TB, DET_, dst_) hipLaunchKernelGGL((k_outer_small<TA, TB, DET_>), grid, dim3(256), 0, s, (const TA*)a + c0, lda, cn, (const TB*)b, ldb, b_rows, dst_, lddw, transpose_out, rows, d, rpb)
#define OS(TA, TB) do { if (det) OS_(TA, TB, true, (float*)scratch->p); else OS_(TA, TB, false, dwc); } while (0)
    if (a_dt == TTV_F32 && b_dt == TTV_F32) OS(float, float);
    else if (a_dt == TTV_F32 && b_dt == TTV_BF16) OS(float, bf16_t);
    else if (a_dt == TTV_BF16 && b_dt == TTV_F32) OS(bf16_t, float);
    else OS(bf16_t, bf16_t);
#undef OS
#undef OS_
    if (det) {
      TTV_CHECK_LAUNCH("outer_small");
      // element (c, f) of the chunk: dw[c][f], or dw[f][c] when the output is transposed
      TTV_TRY(det_fold<float>(scratch->p, (int)grid.x, cn * d, d, transpose_out ? 1 : lddw, transpose_out ? lddw : 1, dwc, s));
    }
  }
  TTV_CHECK_LAUNCH("outer_small");
  return TTV_OK;
}

// out[r, f] = sum_c a[r, c] * w[c, f] (w_cf = 1) or w[f, c] (w_cf = 0): the d-side gradient of a d <-> C projection
template <typename TA, typename TW, typename TO>
__global__ __launch_bounds__(256) void k_expand_small(const TA* __restrict__ a, int lda, int C, const TW* __restrict__ w, int ldw, int w_cf,
                                                      TO* __restrict__ out, int ldo, int rows, int d) {
  const long total = (long)rows * d;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int r = (int)(i / d), f = (int)(i % d);
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc += Cvt<TA>::to_f(a[(size_t)r * lda + c]) * Cvt<TW>::to_f(w_cf ? w[(size_t)c * ldw + f] : w[(size_t)f * ldw + c]);
    out[(size_t)r * ldo + f] = Cvt<TO>::from_f(acc);
  }
}
// out[r, c] = sum_f a[r, f] * w[f, c]   (d -> C contraction, e.g. dcodes = dh W_in)
template <typename TA, typename TW>
__global__ __launch_bounds__(256) void k_reduce_small(const TA* __restrict__ a, int lda, const int* __restrict__ a_rows, const TW* __restrict__ w,
                                                      int ldw, int C, float* __restrict__ out, int ldo, int rows, int d) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  if (r >= rows) return;
  const TA* pa = a + (size_t)(a_rows ? a_rows[r] : r) * lda;
  for (int c = 0; c < C; ++c) {
    float acc = 0.f;
    for (int f = lane; f < d; f += 64) acc += Cvt<TA>::to_f(pa[f]) * Cvt<TW>::to_f(w[(size_t)f * ldw + c]);
    acc = wave_sum(acc);
    if (lane == 0) out[(size_t)r * ldo + c] = acc;
  }
}

int ttvk_expand_small(const void* a, int a_dt, int lda, int C, const void* w, int w_dt, int ldw, int w_cf, void* out, int o_dt, int ldo,
                      int rows, int d, hipStream_t s) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(rows > 0 && C >= 1 && d >= 1 && lda >= C && ldo >= d && ldw >= (w_cf ? d : C) && a && w && out,
                "expand_small: %d rows, C %d, d %d, leading dimensions %d %d %d", rows, C, d, lda, ldw, ldo);
  const int nb = ew_blocks((long)rows * d);
#define ES(TA, TW, TO) hipLaunchKernelGGL((k_expand_small<TA, TW, TO>), dim3(nb), dim3(256), 0, s, (const TA*)a, lda, C, (const TW*)w, ldw, w_cf, (TO*)out, ldo, rows, d)
  if (a_dt == TTV_F32 && w_dt == TTV_BF16 && o_dt == TTV_BF16) ES(float, bf16_t, bf16_t);
  else if (a_dt == TTV_F32 && w_dt == TTV_F32 && o_dt == TTV_F32) ES(float, float, float);
  else if (a_dt == TTV_F32 && w_dt == TTV_BF16 && o_dt == TTV_F32) ES(float, bf16_t, float);
  else { ttv_set_error("expand_small: dtype combination"); return TTV_ERR_INVALID; }
#undef ES
  TTV_CHECK_LAUNCH("expand_small");
  return TTV_OK;
}
int ttvk_reduce_small(const void* a, int a_dt, int lda, const int* a_rows, const void* w, int w_dt, int ldw, int C, float* out, int ldo,
                      int rows, int d, hipStream_t s) {
  if (rows == 0) return TTV_OK;
  TTV_CHECK_ARG(rows > 0 && C >= 1 && d >= 1 && ldw >= C && ldo >= C && (a_rows || lda >= d) && a && w && out,
                "reduce_small: %d rows, C %d, d %d, leading dimensions %d %d %d", rows, C, d, lda, ldw, ldo);
  dim3 grid(ttv_cdiv(rows, 4));
#define RS(TA, TW) hipLaunchKernelGGL((k_reduce_small<TA, TW>), grid, dim3(256), 0, s, (const TA*)a, lda, a_rows, (const TW*)w, ldw, C, out, ldo, rows, d)
  if (a_dt == TTV_BF16 && w_dt == TTV_BF16) RS(bf16_t, bf16_t);
  else if (a_dt == TTV_F32 && w_dt == TTV_F32) RS(float, float);
  else if (a_dt == TTV_F32 && w_dt == TTV_BF16) RS(float, bf16_t);
  else { ttv_set_error("reduce_small: dtype combination"); return TTV_ERR_INVALID; }
#undef RS
  TTV_CHECK_LAUNCH("reduce_small");
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------ attention backward
// delta[t, h] = sum_d dO[t, h, d] * O[t, h, d]
template <typename T>
__global__ __launch_bounds__(256) void k_attn_delta(const T* __restrict__ dout, int ldd, const T* __restrict__ o, int ldo,
                                                    float* __restrict__ delta, int rows, int heads) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * heads) return;
  const int t = i / heads, h = i % heads;
  float acc = 0.f;
#pragma unroll 4
  for (int c = 0; c < 64; c += 4) {
    const f32x4 a = Vec4<T>::load(dout + (size_t)t * ldd + h * 64 + c), b = Vec4<T>::load(o + (size_t)t * ldo + h * 64 + c);
    acc += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  }
  delta[i] = acc;
}

// Query rows of a sequence that take part in the attention backward.  qlim_desc = the batch's clip descriptors (entries 3-5 of a clip: its
// patch grid; the latent tokens are the K_b = S - gt * gh * gw rows in front of the patches) when the forward computed the attention of the LATENT query rows only (encoder,
// last layer: ttv_train.hip latent_tail) - whole 128-row query blocks, as the forward's work table; the rows behind have dO = 0 and no
// valid log-sum-exp, they are skipped (dQ = 0, no contribution to dK / dV).  NULL: every row.
__device__ __forceinline__ int attn_bwd_query_rows(const int* __restrict__ qlim_desc, int seq, int s0, int S) {
  if (!qlim_desc) return S;
  const int kb = S - qlim_desc[8 * seq + 3] * qlim_desc[8 * seq + 4] * qlim_desc[8 * seq + 5];     // latent tokens = rows - patches (gt * gh * gw)
  const int lim = (kb + 127) / 128 * 128;
  return lim < S ? lim : S;
}

// delta of the naive fp32 backward, formed from the very P and dP that backward subtracts it from: one wave per (query row, q-head),
//   delta[t, h] = sum_j p_j dP_j / sum_j p_j,   p_j = exp(s_j - lse), dP_j = dO . v_j   (the expressions of k_attn_bwd_f32, same order).
// rowsum(dO * O) is the same number on paper, but it comes from the forward's O, and p_j from the forward's lse: the recomputed scores
// differ from the forward's in the last bits, so sum_j p_j (dP_j - delta) is not zero but ~1e-6 |dP|.  Where the keys of a sequence
// share a large common component (decoder layer 0: every patch row is the mask token) dQ = sum_j dS_j k_j multiplies that residue
// by the common component, which the exact gradient cancels: the to_qkv gradient of that layer was 4 - 5 times as far from float64 as
// an fp32 autograd of the same model, against 2 times everywhere else.  Rows attn_bwd_query_rows leaves out are not written.
__global__ __launch_bounds__(256) void k_attn_delta_f32_consistent(const float* __restrict__ qkvg, int ld, const float* __restrict__ dout, int ldd,
                                                                   const float* __restrict__ lse, float* __restrict__ delta,
                                                                   const int* __restrict__ cu, const int* __restrict__ row_seq,
                                                                   int total_rows, int hq, int hkv, float scale, const int* __restrict__ qlim_desc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + wave;
  if (idx >= total_rows * hq) return;
  const int t = idx / hq, h = idx % hq;
  const int d_model = hq * 64, gqa = hkv * 64, kvh = h / (hq / hkv);
  const int seq = row_seq[t];
  const int s0 = cu[seq], s1 = cu[seq + 1];
  if (qlim_desc && t - s0 >= attn_bwd_query_rows(qlim_desc, seq, s0, s1 - s0)) return;
  const float q = qkvg[(size_t)t * ld + h * 64 + lane];
  const float dov = dout[(size_t)t * ldd + h * 64 + lane];
  const float l = lse[(size_t)t * hq + h];
  double sp = 0.0, spd = 0.0;       // float64 sums of the fp32 terms: delta is then the rounding of the exact ratio of what the backward adds
  for (int j = s0; j < s1; ++j) {
    const float kv = qkvg[(size_t)j * ld + 2 * d_model + kvh * 64 + lane];
    const float vv = qkvg[(size_t)j * ld + 2 * d_model + gqa + kvh * 64 + lane];
    const float sdot = wave_sum(q * kv) * scale;
    const float p = expf(sdot - l);
    const float dp = wave_sum(dov * vv);
    sp += (double)p;
    spd += (double)p * (double)dp;
  }
  if (lane == 0) delta[(size_t)t * hq + h] = (float)(spd / sp);
}

// naive fp32 backward: one wave per (query row, q-head); lane = head dim.  dk/dv accumulate with fp32 atomics into
// [L, g] scratch (zeroed by the caller), dq is written directly.  ATOMIC_DKV = false (deterministic mode): dq only, the same
// arithmetic; dk / dv then come from k_attn_bwd_f32_dkv below.
template <bool ATOMIC_DKV>
__global__ __launch_bounds__(256) void k_attn_bwd_f32(const float* __restrict__ qkvg, int ld, const float* __restrict__ dout, int ldd,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      const int* __restrict__ cu, const int* __restrict__ row_seq,
                                                      float* __restrict__ dqkvg, int ldg, float* __restrict__ dkv, int total_rows,
                                                      int hq, int hkv, float scale, const int* __restrict__ qlim_desc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + wave;
  if (idx >= total_rows * hq) return;
  const int t = idx / hq, h = idx % hq;
  const int d_model = hq * 64, gqa = hkv * 64, kvh = h / (hq / hkv);
  const int seq = row_seq[t];
  const int s0 = cu[seq], s1 = cu[seq + 1];
  if (qlim_desc && t - s0 >= attn_bwd_query_rows(qlim_desc, seq, s0, s1 - s0)) {   // a query row the forward did not compute: no gradient
    dqkvg[(size_t)t * ldg + h * 64 + lane] = 0.f;
    return;
  }
  const float q = qkvg[(size_t)t * ld + h * 64 + lane];
  const float dov = dout[(size_t)t * ldd + h * 64 + lane];
  const float l = lse[(size_t)t * hq + h], dl = delta[(size_t)t * hq + h];
  // dq in float64: sum_j ds_j is zero on paper, so where the keys share a large common component the running fp32 sum of ds_j k_j
  // carried that component times the partial sums of ds and rounded at their size, not at the size of the result
  double dq = 0.0;
  for (int j = s0; j < s1; ++j) {
    const float kv = qkvg[(size_t)j * ld + 2 * d_model + kvh * 64 + lane];
    const float vv = qkvg[(size_t)j * ld + 2 * d_model + gqa + kvh * 64 + lane];
    const float sdot = wave_sum(q * kv) * scale;
    const float p = expf(sdot - l);
    const float dp = wave_sum(dov * vv);
    const float ds = p * (dp - dl) * scale;
    dq += (double)ds * (double)kv;
    if (ATOMIC_DKV) {
      atomicAdd(dkv + (size_t)j * 2 * gqa + kvh * 64 + lane, ds * q);
      atomicAdd(dkv + (size_t)j * 2 * gqa + gqa + kvh * 64 + lane, p * dov);
    }
  }
  dqkvg[(size_t)t * ldg + h * 64 + lane] = (float)dq;
}

// Deterministic dk / dv of the naive fp32 backward: one wave OWNS a (key row, kv-head) and adds the terms of the kernel above in a fixed
// order - the sequence's query rows ascending, and for each the q-heads of the GQA group ascending (the rows attn_bwd_query_rows
// leaves out are skipped, as there).  Same inputs, lse and delta; every term is formed by the same expressions.  dkv [L, 2g] is written,
// not added to.
__global__ __launch_bounds__(256) void k_attn_bwd_f32_dkv(const float* __restrict__ qkvg, int ld, const float* __restrict__ dout, int ldd,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          const int* __restrict__ cu, const int* __restrict__ row_seq, float* __restrict__ dkv,
                                                          int total_rows, int hq, int hkv, float scale, const int* __restrict__ qlim_desc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + wave;
  if (idx >= total_rows * hkv) return;
  const int j = idx / hkv, kvh = idx % hkv;
  const int d_model = hq * 64, gqa = hkv * 64, rep = hq / hkv;
  const int seq = row_seq[j];
  const int s0 = cu[seq], S = cu[seq + 1] - s0;
  const int nq = attn_bwd_query_rows(qlim_desc, seq, s0, S);
  const float kv = qkvg[(size_t)j * ld + 2 * d_model + kvh * 64 + lane];
  const float vv = qkvg[(size_t)j * ld + 2 * d_model + gqa + kvh * 64 + lane];
  double dk = 0.0, dv = 0.0;        // as dq above: the query rows share a common component too
  for (int t = s0; t < s0 + nq; ++t)
    for (int h = kvh * rep; h < (kvh + 1) * rep; ++h) {
      const float q = qkvg[(size_t)t * ld + h * 64 + lane];
      const float dov = dout[(size_t)t * ldd + h * 64 + lane];
      const float l = lse[(size_t)t * hq + h], dl = delta[(size_t)t * hq + h];
      const float sdot = wave_sum(q * kv) * scale;
      const float p = expf(sdot - l);
      const float dp = wave_sum(dov * vv);
      const float ds = p * (dp - dl) * scale;
      dk += (double)ds * (double)q;
      dv += (double)p * (double)dov;
    }
  dkv[(size_t)j * 2 * gqa + kvh * 64 + lane] = (float)dk;
  dkv[(size_t)j * 2 * gqa + gqa + kvh * 64 + lane] = (float)dv;
}

// ---- bf16 MFMA kernels.  LDS tiles are row-major [64 rows][64 cols] bf16 with 128-byte rows; the 16-byte chunk c of row r
// is stored at chunk position c ^ ((r >> 1) & 7): the 16 rows a ds_read_b128 fragment read touches then cover all 64
// banks once (unswizzled they fall on two 4-bank groups, 8-way), and the transposed reads drop from 4-way to 2-way. ----
// chunk swizzle of the 64 x 64 tiles (128-byte rows: rows r and r + 2 share their banks), m = (row >> 1) & 7.  Plain m keeps the b128 row
// reads (16 lanes = 16 rows of one chunk) conflict-free but only swaps the two chunks of a 32-byte pair between rows r and r + 2, and the
// transposed reads (frag_colp: 16 lanes = 4 consecutive rows x 32 bytes) then run at half rate: SQ_LDS_BANK_CONFLICT was 26 % of
// k_attn_bwd's LDS-active cycles (profiles/r04_train_sq.txt).  This permutation of m puts rows r, r + 2, r + 4, r + 6 on four different pairs
// and still gives the eight rows of one parity eight different chunks; both read kinds at full rate (tools/ubench/lds_rates.hip,
// profiles/r04_lds_rates_attn_bwd.txt: 123 -> 218 bytes / cycle / CU for the transposed reads, 223 -> 225 for the row reads; the simpler
// ((m & 3) << 1) | (m >> 2) fixes the first and halves the second).  -DTTV_TSW_OLD: plain m (A/B).
#ifdef TTV_TSW_OLD
#define TSW(r_) (((r_) >> 1) & 7)
#else
#define TSW(r_) ((((((r_) >> 1) & 1) | (((((r_) >> 2) ^ ((r_) >> 3)) & 1) << 1)) << 1) | (((r_) >> 3) & 1))
#endif
// fragment with 8 consecutive COLUMNS of one row (K-contiguous operand): rows r0+l15, columns kc*8.. (b128)
__device__ __forceinline__ bf16x8 frag_row(const uint4* tile, int row, int chunk) { return __builtin_bit_cast(bf16x8, tile[row * 8 + (chunk ^ TSW(row))]); }
// fragment with 8 consecutive ROWS (row0 + 8*kq + 0..7) of one column col0 + l15: two transposed reads
__device__ __forceinline__ const char* tile_addr(const uint4* tile, int row, int col) {   // col % 4 == 0
  return reinterpret_cast<const char*>(tile) + row * 128 + ((((col >> 3) ^ TSW(row)) << 4) | ((col & 7) << 1));
}
__device__ __forceinline__ bf16x8 frag_col(const uint4* tile, int row0, int col0, int lane) {
  const int gi = lane & 15, tq = gi >> 2, tp = gi & 3, kq = lane >> 4;
  const int r = row0 + kq * 8 + tq, c = col0 + tp * 4;
  const bf16x4 lo = tr16(tile_addr(tile, r, c)), hi = tr16(tile_addr(tile, r + 4, c));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// gradient w.r.t. the un-rotated q / k: the transpose of the rotary map (rope.py:19-27) applied to 4 consecutive dims = 2 pairs;
// cs -> cos of the two pairs, cs + 32 -> sin.  In fp32, before the single rounding of the store.
__device__ __forceinline__ f32x4 rope_inverse4(f32x4 v, const float* cs) {
  const float c0 = cs[0], c1 = cs[1], s0 = cs[32], s1 = cs[33];
  return (f32x4){v[0] * c0 + v[1] * s0, v[1] * c0 - v[0] * s0, v[2] * c1 + v[3] * s1, v[3] * c1 - v[2] * s1};
}

// 64 x 64 bf16 tile -> swizzled LDS tile by LDS-DMA (no register round trip, no ds_write): wave w issues the two
// instructions covering rows 16w .. 16w+15 (8 rows = 1 KB each).  The DMA writes lane l at LDS offset 16 l, so the swizzle is
// applied on the global side: the lane fetches the chunk that belongs at its LDS position.  Rows past row_last are fetched
// from row_last (valid memory, finite values); their scores are masked by the callers.
__device__ __forceinline__ void dma_tile64(uint32_t lds_tile, const bf16_t* base, int ld, int row0, int row_last, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (wave * 2 + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ TSW(r);
    const int gr = min(row0 + r, row_last);
    const uint32_t voff = (uint32_t)(gr * ld + c * 8) * 2u;
    const uint32_t dst = lds_tile + (wave * 2 + i) * 1024;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
  }
}
// 64 floats (one per lane, byte offset voff from base) -> LDS dst .. dst + 255
__device__ __forceinline__ void dma_f32x64(uint32_t dst, const float* base, uint32_t voff) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}

// Fragment for a contraction over 32 ROWS of a row-major tile taken in the order of a C-layout accumulator pair
// (lane group kq: rows row0 + {4kq..4kq+3, 16+4kq..16+4kq+3}), for column col0 + l15: two transposed reads.
// With it, the S / dS accumulators of the first product ARE the B operand of the second one (packed to bf16):
// no LDS round trip and no barrier between the two products.
__device__ __forceinline__ bf16x8 frag_colp(const uint4* tile, int row0, int col0, int lane) {
  const int gi = lane & 15, tq = gi >> 2, tp = gi & 3, kq = lane >> 4;
  const int r = row0 + kq * 4 + tq, c = col0 + tp * 4;
  const bf16x4 lo = tr16(tile_addr(tile, r, c)), hi = tr16(tile_addr(tile, r + 16, c));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ bf16x8 pack_pair(f32x4 lo, f32x4 hi) {
  return (bf16x8){(bf16_t)lo[0], (bf16_t)lo[1], (bf16_t)lo[2], (bf16_t)lo[3], (bf16_t)hi[0], (bf16_t)hi[1], (bf16_t)hi[2], (bf16_t)hi[3]};
}

// dK, dV of one 64-key block of one (sequence, kv-head): loops over the group's q-heads and all 64-query blocks.
// Wave (wa, wb) recomputes S[q][key] / dP[q][key] for queries wa*32.. (MFMA rows) x keys wb*32.. (columns): a lane then holds
// 4 consecutive QUERIES of one key column, i.e. the B fragment of the products contracted over queries,
//   dV^T[d][key] += dO^T[d][q] P[q][key],   dK^T[d][key] += Q^T[d][q] dS[q][key],
// whose A operands are transposed reads of the dO / Q tiles.  Each wave accumulates all 64 d for its 32 keys over its 32
// queries; the two waves of a key half are summed once at the end.
// The block's K / V rows are the B operands of S and dP in every step: their fragments are loaded from global once and stay
// in registers.  The streamed Q / dO tiles (and the lse / delta rows) arrive by LDS-DMA into two stages, one step ahead: one
// barrier per step, nothing of the staging passes through VGPRs.
// tiles: 4 x 512 uint4 (Q stages 0/1, dO stages 0/1; the final cross-wave sum reuses it); ls: [stage][lse | delta][query]
__device__ __forceinline__ void attn_bwd_dkv_block(uint4* tiles, float (*ls)[2][64], const int bx, const int by,
                                                   const bf16_t* __restrict__ qkvg, int ld, const bf16_t* __restrict__ dout, int ldd,
                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                   const int* __restrict__ cu, const int* __restrict__ blocks,
                                                   bf16_t* __restrict__ dqkvg, int ldg, int hq, int hkv, float scale,
                                                   const float* __restrict__ rope_cs, const int* __restrict__ qlim_desc) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wa = wave & 1, wb = wave >> 1;
  const int l15 = lane & 15, kq = lane >> 4;
  const int seq = blocks[2 * bx], key0 = blocks[2 * bx + 1];
  const int kvh = by;
  const int s0 = cu[seq], S = cu[seq + 1] - s0;
  const int d_model = hq * 64, gqa = hkv * 64, rep = hq / hkv;
  const bf16_t* base = qkvg + (size_t)s0 * ld;
  const bf16_t* dbase = dout + (size_t)s0 * ldd;
  const uint32_t tiles_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&tiles[0];
  const uint32_t ls_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&ls[0][0][0];
  const int nqb = (attn_bwd_query_rows(qlim_desc, seq, s0, S) + 63) / 64, nsteps = rep * nqb;      // query blocks that carry a gradient
#define DKV_ISSUE(step_, buf_)                                                                              \
  do {                                                                                                      \
    const int hr__ = (step_) / nqb, q0__ = ((step_) - hr__ * nqb) * 64, h__ = kvh * rep + hr__;             \
    dma_tile64(tiles_lds + (buf_) * 8192, base + h__ * 64, ld, q0__, S - 1, wave, lane);                    \
    dma_tile64(tiles_lds + 16384 + (buf_) * 8192, dbase + h__ * 64, ldd, q0__, S - 1, wave, lane);          \
    if (wave == 0) {                                                                                        \
      const uint32_t vo__ = (uint32_t)((s0 + min(q0__ + lane, S - 1)) * hq + h__) * 4u;                     \
      dma_f32x64(ls_lds + (buf_) * 512, lse, vo__);                                                         \
      dma_f32x64(ls_lds + (buf_) * 512 + 256, delta, vo__);                                                 \
    }                                                                                                       \
  } while (0)
  if (nsteps > 0) DKV_ISSUE(0, 0);      // a clip without gradient-carrying query rows (K_b = 0 under the latent tail): dK = dV = 0, nothing staged
  bf16x8 bk[2][2], bv[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = min(key0 + wb * 32 + j * 16 + l15, S - 1);
    const bf16_t* kr = base + (size_t)key * ld + 2 * d_model + kvh * 64 + kq * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bk[ks][j] = *reinterpret_cast<const bf16x8*>(kr + ks * 32);
      bv[ks][j] = *reinterpret_cast<const bf16x8*>(kr + gqa + ks * 32);
    }
  }
  f32x4 dk[4][2], dv[4][2];   // [d tile][key tile of this wave]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) { dk[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  for (int step = 0; step < nsteps; ++step) {
    const int buf = step & 1;
    const int hr = step / nqb, q0 = (step - hr * nqb) * 64;
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's share of stage `buf` has landed
    __syncthreads();                      // stage complete; every wave is done with the other stage
    if (step + 1 < nsteps) DKV_ISSUE(step + 1, buf ^ 1);
    const uint4* qt = tiles + buf * 512;
    const uint4* dt_ = tiles + 1024 + buf * 512;
    const float* lse_s = &ls[buf][0][0];
    const float* delta_s = &ls[buf][1][0];
    // S[q][key], dP[q][key]: A = Q / dO rows (queries), B = K / V rows (keys, registers)
    f32x4 sp[2][2], dp[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) { sp[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 aq[2], ad[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        aq[i] = frag_row(qt, wa * 32 + i * 16 + l15, ks * 4 + kq);
        ad[i] = frag_row(dt_, wa * 32 + i * 16 + l15, ks * 4 + kq);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          sp[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[i], bk[ks][j], sp[i][j], 0, 0, 0);
          dp[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad[i], bv[ks][j], dp[i][j], 0, 0, 0);
        }
    }
    // the transposed dO / Q fragments of the second products do not depend on the scores: requested before the exponentials
    bf16x8 ado[4], aqt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ado[i] = frag_colp(dt_, wa * 32, i * 16, lane);   // rows = d (16 i + l15), k = this wave's 32 queries
      aqt[i] = frag_colp(qt, wa * 32, i * 16, lane);
    }
    // P = exp(S*scale - lse[q]), dS = P (dP - delta[q]) scale ; lane: queries wa*32 + i*16 + 4kq + e (rows), key column l15
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int qb = wa * 32 + i * 16 + kq * 4;
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qb), d4 = *reinterpret_cast<const f32x4*>(delta_s + qb);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool kv_ok = key0 + wb * 32 + j * 16 + l15 < S;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pv = (kv_ok && q0 + qb + e < S) ? __expf(sp[i][j][e] * scale - l4[e]) : 0.f;
          dp[i][j][e] = pv * (dp[i][j][e] - d4[e]) * scale;
          sp[i][j][e] = pv;
        }
      }
    }
    bf16x8 bp[2], bs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) { bp[j] = pack_pair(sp[0][j], sp[1][j]); bs[j] = pack_pair(dp[0][j], dp[1][j]); }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        dv[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ado[i], bp[j], dv[i][j], 0, 0, 0);
        dk[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqt[i], bs[j], dk[i][j], 0, 0, 0);
      }
  }
#undef DKV_ISSUE
  // sum the two query halves: wave wa keeps d tiles {2wa, 2wa+1} and receives them from its partner
  uint4* red = tiles;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int io = (1 - wa) * 2 + i;   // the d tiles the partner keeps
      red[(((wb * 2 + wa) * 2 + i) * 2 + j) * 128 + lane] = __builtin_bit_cast(uint4, dk[io][j]);
      red[(((wb * 2 + wa) * 2 + i) * 2 + j) * 128 + 64 + lane] = __builtin_bit_cast(uint4, dv[io][j]);
    }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ik = wa * 2 + i;
      const f32x4 pk = __builtin_bit_cast(f32x4, red[(((wb * 2 + (1 - wa)) * 2 + i) * 2 + j) * 128 + lane]);
      const f32x4 pv = __builtin_bit_cast(f32x4, red[(((wb * 2 + (1 - wa)) * 2 + i) * 2 + j) * 128 + 64 + lane]);
      const int key = key0 + wb * 32 + j * 16 + l15, d0 = ik * 16 + kq * 4;   // lane: 4 consecutive d (rows) of key (col) l15
      if (key < S) {
        bf16_t* row = dqkvg + (size_t)(s0 + key) * ldg + 2 * d_model + kvh * 64 + d0;
        f32x4 gk = dk[ik][j] + pk;
        if (rope_cs) gk = rope_inverse4(gk, rope_cs + (size_t)(s0 + key) * 64 + (d0 >> 1));
        Vec4<bf16_t>::store(row, gk);
        Vec4<bf16_t>::store(row + gqa, dv[ik][j] + pv);
      }
    }
}

// dQ of one 64-query block of one (sequence, q-head): loops over all 64-key blocks.  Wave (wa, wb) recomputes S^T / dP^T for
// keys wa*32.. (MFMA rows) x queries wb*32.. (columns): a lane holds 4 consecutive KEYS of one query column = the B fragment of
//   dQ^T[d][q] += K^T[d][key] dS^T[key][q]   (contraction over keys; A = transposed read of the K tile).
// Each wave accumulates all 64 d for its 32 queries over its 32 keys of every block; the two key halves are summed at the end.
// Mirror image of the kernel above: the block's Q / dO fragments (B operands) and its lse / delta live in registers, the K / V
// tiles stream through two LDS-DMA stages.
// tiles: 4 x 512 uint4 (K stages 0/1, V stages 0/1; the final cross-wave sum reuses it)
__device__ __forceinline__ void attn_bwd_dq_block(uint4* tiles, const int bx, const int by,
                                                  const bf16_t* __restrict__ qkvg, int ld, const bf16_t* __restrict__ dout, int ldd,
                                                  const float* __restrict__ lse, const float* __restrict__ delta,
                                                  const int* __restrict__ cu, const int* __restrict__ blocks,
                                                  bf16_t* __restrict__ dqkvg, int ldg, int hq, int hkv, float scale,
                                                  const float* __restrict__ rope_cs, const int* __restrict__ qlim_desc) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wa = wave & 1, wb = wave >> 1;
  const int l15 = lane & 15, kq = lane >> 4;
  const int seq = blocks[2 * bx], q0 = blocks[2 * bx + 1];
  const int h = by;
  const int s0 = cu[seq], S = cu[seq + 1] - s0;
  if (qlim_desc && q0 >= attn_bwd_query_rows(qlim_desc, seq, s0, S)) {     // query rows without a gradient: dQ = 0 (block-uniform)
    const int row = q0 + (tid >> 2), c0 = (tid & 3) * 16;                     // 64 rows x 64 columns, 16 columns per thread
    if (row < S) {
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      uint4* dst = reinterpret_cast<uint4*>(dqkvg + (size_t)(s0 + row) * ldg + h * 64 + c0);
      dst[0] = z;
      dst[1] = z;
    }
    return;
  }
  const int d_model = hq * 64, gqa = hkv * 64, kvh = h / (hq / hkv);
  const bf16_t* base = qkvg + (size_t)s0 * ld;
  const bf16_t* kbase = base + 2 * d_model + kvh * 64;
  const uint32_t tiles_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&tiles[0];
#define DQ_ISSUE(key0_, buf_)                                                                \
  do {                                                                                       \
    dma_tile64(tiles_lds + (buf_) * 8192, kbase, ld, (key0_), S - 1, wave, lane);            \
    dma_tile64(tiles_lds + 16384 + (buf_) * 8192, kbase + gqa, ld, (key0_), S - 1, wave, lane); \
  } while (0)
  DQ_ISSUE(0, 0);
  bf16x8 bq[2][2], bd[2][2];
  float lq[2], dl[2];
  bool qv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int qi = q0 + wb * 32 + j * 16 + l15;
    qv[j] = qi < S;
    const int q = min(qi, S - 1);
    const bf16_t* qr = base + (size_t)q * ld + h * 64 + kq * 8;
    const bf16_t* dr = dout + (size_t)(s0 + q) * ldd + h * 64 + kq * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bq[ks][j] = *reinterpret_cast<const bf16x8*>(qr + ks * 32);
      bd[ks][j] = *reinterpret_cast<const bf16x8*>(dr + ks * 32);
    }
    lq[j] = lse[(size_t)(s0 + q) * hq + h];
    dl[j] = delta[(size_t)(s0 + q) * hq + h];
  }
  f32x4 dq[4][2];   // [d tile][query tile of this wave]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) dq[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int buf = 0;
  for (int key0 = 0; key0 < S; key0 += 64, buf ^= 1) {
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();
    if (key0 + 64 < S) DQ_ISSUE(key0 + 64, buf ^ 1);
    const uint4* kt = tiles + buf * 512;
    const uint4* vt = tiles + 1024 + buf * 512;
    // S^T[key][q], dP^T[key][q]: A = K / V rows (keys), B = Q / dO rows (queries, registers)
    f32x4 sp[2][2], dp[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) { sp[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 ak[2], av[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ak[i] = frag_row(kt, wa * 32 + i * 16 + l15, ks * 4 + kq);
        av[i] = frag_row(vt, wa * 32 + i * 16 + l15, ks * 4 + kq);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          sp[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak[i], bq[ks][j], sp[i][j], 0, 0, 0);
          dp[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bd[ks][j], dp[i][j], 0, 0, 0);
        }
    }
    bf16x8 akt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) akt[i] = frag_colp(kt, wa * 32, i * 16, lane);   // rows = d (16 i + l15), k = this wave's 32 keys
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = key0 + wa * 32 + i * 16 + kq * 4 + e;
          const float p = (qv[j] && key < S) ? __expf(sp[i][j][e] * scale - lq[j]) : 0.f;
          dp[i][j][e] = p * (dp[i][j][e] - dl[j]) * scale;
        }
    bf16x8 bs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bs[j] = pack_pair(dp[0][j], dp[1][j]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) dq[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akt[i], bs[j], dq[i][j], 0, 0, 0);
  }
#undef DQ_ISSUE
  // sum the two key halves: wave wa keeps d tiles {2wa, 2wa+1}
  uint4* red = tiles;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) red[(((wb * 2 + wa) * 2 + i) * 2 + j) * 64 + lane] = __builtin_bit_cast(uint4, dq[(1 - wa) * 2 + i][j]);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ik = wa * 2 + i;
      const f32x4 pq = __builtin_bit_cast(f32x4, red[(((wb * 2 + (1 - wa)) * 2 + i) * 2 + j) * 64 + lane]);
      const int q = q0 + wb * 32 + j * 16 + l15, d0 = ik * 16 + kq * 4;
      if (q < S) {
        f32x4 gq = dq[ik][j] + pq;
        if (rope_cs) gq = rope_inverse4(gq, rope_cs + (size_t)(s0 + q) * 64 + (d0 >> 1));
        Vec4<bf16_t>::store(dqkvg + (size_t)(s0 + q) * ldg + h * 64 + d0, gq);
      }
    }
}

// Both halves of the attention backward in ONE grid ("horizontal fusion"): they are independent (same inputs, disjoint output
// columns), and launched one after the other each leaves a tail - at the benchmark batch dK/dV is 1152 blocks on 768 resident
// slots (second round half empty) and dQ 2304 blocks on 1024 (third round a quarter full).  The long blocks come first (dK/dV: 36
// steps each), the short ones (dQ: 18 steps) fill in behind them, so only the very end of the grid runs below full occupancy.
__global__ __launch_bounds__(256, 2) void k_attn_bwd(const bf16_t* __restrict__ qkvg, int ld, const bf16_t* __restrict__ dout, int ldd,
                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                     const int* __restrict__ cu, const int* __restrict__ blocks, int n_blocks,
                                                     bf16_t* __restrict__ dqkvg, int ldg, int hq, int hkv, float scale,
                                                     const float* __restrict__ rope_cs, const int* __restrict__ qlim_desc) {
  __shared__ __attribute__((aligned(16))) uint4 tiles[4 * 512];
  __shared__ __attribute__((aligned(16))) float ls[2][2][64];
  const int n_dkv = n_blocks * hkv;
  int b = blockIdx.x;
  if (b < n_dkv) {
    attn_bwd_dkv_block(tiles, ls, b % n_blocks, b / n_blocks, qkvg, ld, dout, ldd, lse, delta, cu, blocks, dqkvg, ldg, hq, hkv, scale, rope_cs, qlim_desc);
  } else {
    b -= n_dkv;
    attn_bwd_dq_block(tiles, b % n_blocks, b / n_blocks, qkvg, ld, dout, ldd, lse, delta, cu, blocks, dqkvg, ldg, hq, hkv, scale, rope_cs, qlim_desc);
  }
}

// blocks64: device int32 [n,2] = (sequence, first row) for 64-row blocks; row_seq: device int32 [L] sequence of every row
// (fp32 path); dkv_scratch: fp32 [L, 2g] zeroed by this function (fp32 path only).
int ttvk_attention_bwd(const void* qkvg, int ld, const void* o, int ldo, const void* dout, int ldd, const float* lse, float* delta,
                       const int* cu, const int* blocks64, int n_blocks64, const int* row_seq, void* dqkvg, int ldg, float* dkv_scratch,
                       int total_rows, int hq, int hkv, int dt, const float* rope_cs, hipStream_t s, int delta_ready, const int* qlim_desc) {
  if (total_rows == 0) return TTV_OK;
  TTV_CHECK_ARG(hq >= 1 && hkv >= 1 && hq % hkv == 0, "attention_bwd: %d q-heads on %d kv-heads", hq, hkv);
  const float scale = 0.125f;
  const int d_model = hq * 64, gqa = hkv * 64;
  if (dt == TTV_BF16 && !delta_ready) {    // delta_ready: the caller's gate backward already filled delta (same values: sum of the stored dO times O)
    hipLaunchKernelGGL((k_attn_delta<bf16_t>), dim3(ttv_cdiv(total_rows * hq, 256)), dim3(256), 0, s, (const bf16_t*)dout, ldd, (const bf16_t*)o, ldo, delta, total_rows, hq);
    TTV_CHECK_LAUNCH("attn_delta");
  }
  if (dt == TTV_BF16) {
    hipLaunchKernelGGL(k_attn_bwd, dim3(n_blocks64 * (hkv + hq)), dim3(256), 0, s, (const bf16_t*)qkvg, ld, (const bf16_t*)dout, ldd, lse, delta, cu,
                       blocks64, n_blocks64, (bf16_t*)dqkvg, ldg, hq, hkv, scale, rope_cs, qlim_desc);
    TTV_CHECK_LAUNCH("attn_bwd");
  } else {
    TTV_CHECK_ARG(dkv_scratch && row_seq, "attention_bwd: fp32 path needs scratch and row map");
    // the checking path replaces rowsum(dO * O) by the delta that is consistent with its own P and dP (k_attn_delta_f32_consistent)
    hipLaunchKernelGGL(k_attn_delta_f32_consistent, dim3(ttv_cdiv(total_rows * hq, 4)), dim3(256), 0, s, (const float*)qkvg, ld, (const float*)dout, ldd, lse, delta, cu, row_seq, total_rows, hq, hkv, scale, qlim_desc);
    TTV_CHECK_LAUNCH("attn_delta_f32_consistent");
    if (ttv_det()) {
      // dq as ever, dk / dv by an owner per (key row, kv-head): the same [L, 2g] scratch, written whole
      hipLaunchKernelGGL(k_attn_bwd_f32<false>, dim3(ttv_cdiv(total_rows * hq, 4)), dim3(256), 0, s, (const float*)qkvg, ld, (const float*)dout, ldd, lse, delta, cu, row_seq, (float*)dqkvg, ldg, dkv_scratch, total_rows, hq, hkv, scale, qlim_desc);
      hipLaunchKernelGGL(k_attn_bwd_f32_dkv, dim3(ttv_cdiv(total_rows * hkv, 4)), dim3(256), 0, s, (const float*)qkvg, ld, (const float*)dout, ldd, lse, delta, cu, row_seq, dkv_scratch, total_rows, hq, hkv, scale, qlim_desc);
    } else {
      (void)hipMemsetAsync(dkv_scratch, 0, (size_t)total_rows * 2 * gqa * sizeof(float), s);
      hipLaunchKernelGGL(k_attn_bwd_f32<true>, dim3(ttv_cdiv(total_rows * hq, 4)), dim3(256), 0, s, (const float*)qkvg, ld, (const float*)dout, ldd, lse, delta, cu, row_seq, (float*)dqkvg, ldg, dkv_scratch, total_rows, hq, hkv, scale, qlim_desc);
    }
    TTV_CHECK_LAUNCH("attn_bwd_f32");
    // copy dk|dv scratch [L, 2g] into the k, v columns of dqkvg
    (void)hipMemcpy2DAsync((float*)dqkvg + 2 * d_model, (size_t)ldg * sizeof(float), dkv_scratch, (size_t)2 * gqa * sizeof(float),
                           (size_t)2 * gqa * sizeof(float), total_rows, hipMemcpyDeviceToDevice, s);
    if (rope_cs) {   // the bf16 kernels rotate in their store; the checking path uses the stand-alone kernel
      int rc = ttvk_rope_apply_dir(dqkvg, dt, ldg, total_rows, hq, rope_cs, 1, s);
      if (rc == TTV_OK) rc = ttvk_rope_apply_dir((float*)dqkvg + 2 * d_model, dt, ldg, total_rows, hkv, rope_cs, 1, s);
      if (rc != TTV_OK) return rc;
    }
  }
  return TTV_OK;
}

// ------------------------------------------------------------------------------------------------
// L1 reconstruction term of the generator loss (model/losses/loss_module.py:118 applied per clip, train.py:70):
//   loss = mean over clips of mean |target - recon| ; d loss / d recon[c][i] = sign(recon - target) / (n_c * B)
// One launch for value and gradient of every clip (the per-clip torch ops cost ~10 launches per clip).
// ------------------------------------------------------------------------------------------------
struct L1Clips { const void* recon[TTV_MAX_CLIPS_PER_LAUNCH]; const void* target[TTV_MAX_CLIPS_PER_LAUNCH]; void* grad[TTV_MAX_CLIPS_PER_LAUNCH];
                 int n[TTV_MAX_CLIPS_PER_LAUNCH]; };

// DET: loss is the [clip][block] partial array
template <typename T, bool DET>
__global__ __launch_bounds__(256) void k_l1_loss(L1Clips c, float inv_clips, float* __restrict__ loss) {
  __shared__ float red[4];
  const int ci = blockIdx.y, n = c.n[ci];
  const T* r = reinterpret_cast<const T*>(c.recon[ci]);
  const T* t = reinterpret_cast<const T*>(c.target[ci]);
  T* g = reinterpret_cast<T*>(c.grad[ci]);
  const float w = inv_clips / (float)n;
  float acc = 0.f;
  // 16-byte accesses (8 bf16 / 4 fp32 per thread and step) when the three pointers allow it; scalar tail / fallback below
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec_ok = (((uintptr_t)r | (uintptr_t)t | (uintptr_t)g) & 15) == 0;
  const int nv = vec_ok ? n / V : 0;
  const int stride = gridDim.x * 256;
  for (int i0 = blockIdx.x * 256 + threadIdx.x; i0 < nv; i0 += 2 * stride) {     // two 16-byte vectors of each operand in flight
    T rv[2][V], tv[2][V], gv[V];
    const int i1 = i0 + stride;
    *reinterpret_cast<uint4*>(rv[0]) = reinterpret_cast<const uint4*>(r)[i0];
    *reinterpret_cast<uint4*>(tv[0]) = reinterpret_cast<const uint4*>(t)[i0];
    if (i1 < nv) {
      *reinterpret_cast<uint4*>(rv[1]) = reinterpret_cast<const uint4*>(r)[i1];
      *reinterpret_cast<uint4*>(tv[1]) = reinterpret_cast<const uint4*>(t)[i1];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && i1 >= nv) break;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = (float)rv[u][e] - (float)tv[u][e];
        acc += fabsf(d);
        gv[e] = (T)(d > 0.f ? w : (d < 0.f ? -w : 0.f));
      }
      if (g) reinterpret_cast<uint4*>(g)[u ? i1 : i0] = *reinterpret_cast<const uint4*>(gv);
    }
  }
  for (int i = nv * V + blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float d = (float)r[i] - (float)t[i];
    acc += fabsf(d);
    if (g) g[i] = (T)(d > 0.f ? w : (d < 0.f ? -w : 0.f));
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (red[0] + red[1] + red[2] + red[3]) * w;
    if (DET) loss[blockIdx.y * gridDim.x + blockIdx.x] = v; else atomicAdd(loss, v);
  }
}

// Squared error of clamp(recon, -1, 1) against target, summed over the clips of a call into a double accumulator (the statistic
// behind the reference's PSNR: model/metrics/eval_metrics.py:19,32-36 = torchmetrics PeakSignalNoiseRatio(data_range=2), which keeps
// the running sum of squared errors and the element count over all update() calls).  acc[0] += sum (clamp(r) - t)^2, acc[1] += count.
// DET: acc2 is the [clip][block][2] partial array (sum of squares, element count - the count in a clip's block 0, zero in the others)
template <typename T, bool DET>
__global__ __launch_bounds__(256) void k_sq_err(L1Clips c, int clamp, double* __restrict__ acc2) {
  __shared__ float red[4];
  const int ci = blockIdx.y, n = c.n[ci];
  const T* r = reinterpret_cast<const T*>(c.recon[ci]);
  const T* t = reinterpret_cast<const T*>(c.target[ci]);
  float acc = 0.f;
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec_ok = (((uintptr_t)r | (uintptr_t)t) & 15) == 0;
  const int nv = vec_ok ? n / V : 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
    T rv[V], tv[V];
    *reinterpret_cast<uint4*>(rv) = reinterpret_cast<const uint4*>(r)[i];
    *reinterpret_cast<uint4*>(tv) = reinterpret_cast<const uint4*>(t)[i];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float x = (float)rv[e];
      if (clamp) x = __builtin_amdgcn_fmed3f(x, -1.0f, 1.0f);
      const float d = x - (float)tv[e];
      acc = fmaf(d, d, acc);
    }
  }
  for (int i = nv * V + blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    float x = (float)r[i];
    if (clamp) x = __builtin_amdgcn_fmed3f(x, -1.0f, 1.0f);
    const float d = x - (float)t[i];
    acc = fmaf(d, d, acc);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double v = (double)(red[0] + red[1] + red[2] + red[3]);
    if (DET) {
      double* mine = acc2 + 2 * (size_t)(blockIdx.y * gridDim.x + blockIdx.x);
      mine[0] = v;
      mine[1] = blockIdx.x == 0 ? (double)n : 0.0;
    } else {
      atomicAdd(&acc2[0], v);
      if (blockIdx.x == 0) atomicAdd(&acc2[1], (double)n);
    }
  }
}

// blocks per clip of the two launches above (one geometry for both modes)
static inline int sq_err_bx(const int* sizes, int n_clips) {
  int mx = 0;
  for (int i = 0; i < n_clips; ++i) mx = sizes[i] > mx ? sizes[i] : mx;
  const int bx = ttv_cdiv(mx, 256 * 8);
  return bx < 1 ? 1 : (bx > 256 ? 256 : bx);
}
static inline int l1_loss_bx(const int* sizes, int n_clips) {
  int mx = 0;
  for (int i = 0; i < n_clips; ++i) mx = sizes[i] > mx ? sizes[i] : mx;
  // ~1024 blocks in all: every block ends in ONE atomicAdd on the loss scalar, and same-address atomics retire one after the other
  // at the memory side - with 256 blocks per clip (8192 at the benchmark batch) that tail was most of the launch (110 -> ~45 us)
  const int bx = ttv_cdiv(mx, 256 * 8);
  const int cap = 1024 / n_clips > 8 ? 1024 / n_clips : 8;
  return bx < 1 ? 1 : (bx > cap ? cap : bx);
}
int64_t ttvk_det_clips_bytes(const int* sizes, int n_clips, bool l1) {
  int64_t most = 0;
  for (int c0 = 0; c0 < n_clips; c0 += TTV_MAX_CLIPS_PER_LAUNCH) {
    const int n = n_clips - c0 < TTV_MAX_CLIPS_PER_LAUNCH ? n_clips - c0 : TTV_MAX_CLIPS_PER_LAUNCH;
    const int64_t v = l1 ? (int64_t)l1_loss_bx(sizes + c0, n) * n * 4 : (int64_t)sq_err_bx(sizes + c0, n) * n * 16;
    most = v > most ? v : most;
  }
  return most;
}

int ttvk_sq_err(void* const* recon, void* const* target, const int* sizes, int n_clips, int dtype, int clamp, double* acc2, hipStream_t s,
                const DetScratch* det) {
  TTV_CHECK_ARG(n_clips >= 0 && n_clips <= TTV_MAX_CLIPS_PER_LAUNCH, "sq_err: at most %d clips per call", TTV_MAX_CLIPS_PER_LAUNCH);
  if (n_clips == 0) return TTV_OK;
  TTV_CHECK_ARG(recon && target && sizes && acc2, "sq_err: null argument");
  L1Clips c;
  for (int i = 0; i < n_clips; ++i) {
    c.recon[i] = recon[i]; c.target[i] = target[i]; c.grad[i] = nullptr; c.n[i] = sizes[i];
    TTV_CHECK_ARG(sizes[i] > 0 && recon[i] && target[i], "sq_err: empty clip");
  }
  const int bx = sq_err_bx(sizes, n_clips);
  if (ttv_det()) {
    TTV_CHECK_DET(det, (int64_t)bx * n_clips * 16, "sq_err");
    double* part = (double*)det->p;
    if (dtype == TTV_BF16) hipLaunchKernelGGL((k_sq_err<bf16_t, true>), dim3(bx, n_clips), dim3(256), 0, s, c, clamp, part);
    else hipLaunchKernelGGL((k_sq_err<float, true>), dim3(bx, n_clips), dim3(256), 0, s, c, clamp, part);
    TTV_CHECK_LAUNCH("sq_err");
    return det_fold<double>(part, bx * n_clips, 2, 2, 0, 1, acc2, s);
  }
  if (dtype == TTV_BF16) hipLaunchKernelGGL((k_sq_err<bf16_t, false>), dim3(bx, n_clips), dim3(256), 0, s, c, clamp, acc2);
  else hipLaunchKernelGGL((k_sq_err<float, false>), dim3(bx, n_clips), dim3(256), 0, s, c, clamp, acc2);
  TTV_CHECK_LAUNCH("sq_err");
  return TTV_OK;
}

int ttvk_l1_loss(void* const* recon, void* const* target, void* const* grad, const int* sizes, int n_clips, int total_clips, int dtype,
                 float* loss, hipStream_t s, const DetScratch* det) {
  TTV_CHECK_ARG(n_clips >= 0 && n_clips <= TTV_MAX_CLIPS_PER_LAUNCH && total_clips >= n_clips, "l1_loss: at most %d clips per call", TTV_MAX_CLIPS_PER_LAUNCH);
  if (n_clips == 0) return TTV_OK;
  TTV_CHECK_ARG(recon && target && sizes && loss, "l1_loss: null argument");
  L1Clips c;
  for (int i = 0; i < n_clips; ++i) {
    c.recon[i] = recon[i]; c.target[i] = target[i]; c.grad[i] = grad ? grad[i] : nullptr; c.n[i] = sizes[i];
    TTV_CHECK_ARG(sizes[i] > 0 && recon[i] && target[i], "l1_loss: empty clip");
  }
  const int bx = l1_loss_bx(sizes, n_clips);
  if (ttv_det()) {
    TTV_CHECK_DET(det, (int64_t)bx * n_clips * 4, "l1_loss");
    float* part = (float*)det->p;
    if (dtype == TTV_BF16) hipLaunchKernelGGL((k_l1_loss<bf16_t, true>), dim3(bx, n_clips), dim3(256), 0, s, c, 1.0f / (float)total_clips, part);
    else hipLaunchKernelGGL((k_l1_loss<float, true>), dim3(bx, n_clips), dim3(256), 0, s, c, 1.0f / (float)total_clips, part);
    TTV_CHECK_LAUNCH("l1_loss");
    return det_fold<float>(part, bx * n_clips, 1, 1, 0, 0, loss, s);
  }
  if (dtype == TTV_BF16) hipLaunchKernelGGL((k_l1_loss<bf16_t, false>), dim3(bx, n_clips), dim3(256), 0, s, c, 1.0f / (float)total_clips, loss);
  else hipLaunchKernelGGL((k_l1_loss<float, false>), dim3(bx, n_clips), dim3(256), 0, s, c, 1.0f / (float)total_clips, loss);
  TTV_CHECK_LAUNCH("l1_loss");
  return TTV_OK;
}
