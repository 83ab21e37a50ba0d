// What a VQ training loop needs around the nearest-entry quantiser of ttv_vq.hip: the commitment term and its gradient, the per-entry
// statistics of an EMA codebook update, and the update itself with the restart of dead entries.  include/titok_hip.h states the values
// and the order of every sum; nothing here uses a float atomic, so every result is the same bits run to run.
//
// Kernels (all on the caller's stream, no host synchronisation; the work is tens of MB at most, so the launches are latency-bound)
//   k_vq_commit_partial : a block owns VQC_ROWS rows whatever the grid: a thread folds its elements (z - e)^2 with fmaf in element
//                         order, the 256 threads meet in an LDS tree; one partial per block.
//   k_vq_commit_finish  : one block folds the partials (thread t takes t, t + 256, .. in order, then the same tree) and scales.
//   k_vq_commit_bwd     : dz = g + scale (z - e), formed in fp64 and rounded once to fp32 (and once more to bf16 for bf16 rows).
//   k_vq_ema_stats      : a block owns EMA_E consecutive entries and scans the index vector (128 KB at 32 k rows, L2-resident) twice:
//                         pass 1 counts the rows below its range and per entry (integer LDS atomics), pass 2 compacts the row ids of
//                         its range in row order (ballot + popcount; each wave owns a contiguous quarter of the rows, so no barrier
//                         inside the scan); a wave per entry then splits that list by entry, still in row order; last, C lanes per
//                         entry add the rows of z in ascending row order, 16 row loads in flight per lane (the collapse case - every
//                         row on one entry - is one chain of `rows` dependent adds behind batched loads, not one lane behind a launch).
//                         The same lanes write the restart candidate of a dead entry: the row of z that Philox4x32-10 names.
//   k_vq_ema_total      : one block: the new cluster sizes and their sum in a fixed order (thread t takes t, t + 1024, .., then a tree).
//   k_vq_ema_apply      : a block owns 64 entries = one contiguous stretch of every [N, C] array: the new moving sums, the codebook, its
//                         compute-dtype copy; the stretch goes through LDS so that one lane per entry forms ||c||^2 with the fmaf chain
//                         of k_vq_norms (the same bits as a rebuild), writes the cluster size and, once, bumps the step counter.
// No spills: VGPRs 17 / 7 / 12 / 59 / 12 / 24 in the order above (bf16; -Rpass-analysis=kernel-resource-usage), scratch 0.
#include "ttv_common.h"
#include "ttv_kernels.h"

namespace {

constexpr int VQC_ROWS = 64;     // rows per block of the commitment sum: fixed, so the partials do not depend on the grid
constexpr int EMA_E = 32;        // entries per block of the statistics
constexpr int EMA_TILE = 64;     // entries per block of the update
constexpr int EMA_BATCH = 16;    // row loads in flight per lane while an entry's rows are added

// sh[0] = sum of the 256 values, by halves: 128 pairs (t, t + 128), then 64, ..: the order include/titok_hip.h gives
__device__ __forceinline__ float tree256(float v, float* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

template <typename T>
__global__ __launch_bounds__(256) void k_vq_commit_partial(const T* __restrict__ z, int ldz, const T* __restrict__ cb, int ldc,
                                                           const int* __restrict__ idx, int rows, int N, int C, float* __restrict__ partial) {
  __shared__ float sh[256];
  const int r0 = blockIdx.x * VQC_ROWS;
  const int n_el = min(VQC_ROWS, rows - r0) * C;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_el; i += 256) {
    const int rr = i / C, c = i - rr * C, r = r0 + rr;
    const int k = min(max(idx[r], 0), N - 1);
    const float d = Cvt<T>::to_f(z[(size_t)r * ldz + c]) - Cvt<T>::to_f(cb[(size_t)k * ldc + c]);
    acc = fmaf(d, d, acc);
  }
  const float s = tree256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_vq_commit_finish(const float* __restrict__ partial, int n_partial, float inv_count, float* __restrict__ loss) {
  __shared__ float sh[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
  const float s = tree256(acc, sh);
  if (threadIdx.x == 0) loss[0] = s * inv_count;
}

template <typename T>
__global__ __launch_bounds__(256) void k_vq_commit_bwd(const T* __restrict__ g, int ldg, const T* __restrict__ z, int ldz, const T* __restrict__ e, int lde,
                                                       int rows, int C, double scale, T* __restrict__ dz, int ldd) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)rows * C) return;
  const int r = (int)(i / C), c = (int)(i - (long)r * C);
  const double zz = (double)Cvt<T>::to_f(z[(size_t)r * ldz + c]), ee = (double)Cvt<T>::to_f(e[(size_t)r * lde + c]);
  const double v = (double)Cvt<T>::to_f(g[(size_t)r * ldg + c]) + scale * (zz - ee);
  dz[(size_t)r * ldd + c] = Cvt<T>::from_f((float)v);
}

// lpe: lanes per entry of the adding stage, the power of two >= C
template <typename T>
__global__ __launch_bounds__(256) void k_vq_ema_stats(const T* __restrict__ z, int ldz, const int* __restrict__ idx, int rows, int N, int C, int lpe,
                                                      const float* __restrict__ cluster_size, float thr, uint32_t k0, uint32_t k1,
                                                      const int64_t* __restrict__ ema_step, int rank, int world, float* __restrict__ stats,
                                                      int* __restrict__ seg_row, int* __restrict__ seg_key, int* __restrict__ order) {
  __shared__ int hist[EMA_E], excl[EMA_E], wbelow[4], wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * EMA_E;
  if (tid < EMA_E) hist[tid] = 0;
  if (tid < 4) { wbelow[tid] = 0; wcnt[tid] = 0; }
  __syncthreads();
  // pass 1: wave w owns rows [w q, (w + 1) q): how many lie below this block's entries, how many on each of them
  const int q = (rows + 255) / 256 * 64;
  const int r0 = wave * q, r1 = min(rows, r0 + q);
  int below = 0, mine = 0;
  for (int r = r0 + lane; r < r1; r += 64) {
    const int k = idx[r];
    below += k < n0;
    if ((unsigned)(k - n0) < (unsigned)EMA_E && k < N) {
      atomicAdd(&hist[k - n0], 1);
      ++mine;
    }
  }
  atomicAdd(&wbelow[wave], below);
  atomicAdd(&wcnt[wave], mine);
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int e = 0; e < EMA_E; ++e) { excl[e] = run; run += hist[e]; }
  }
  __syncthreads();
  const int base = wbelow[0] + wbelow[1] + wbelow[2] + wbelow[3];      // this block's stretch of the sorted list: [base, base + len)
  const int len = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  if (tid < EMA_E && n0 + tid < N) stats[n0 + tid] = (float)hist[tid];
  // pass 2: the row ids (and entries) of this block's range in ascending row order
  {
    int pos = base;
    for (int w = 0; w < wave; ++w) pos += wcnt[w];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = r0 + lane; r - lane < r1; r += 64) {
      const int k = r < r1 ? idx[r] : -1;
      const bool in = (unsigned)(k - n0) < (unsigned)EMA_E && k < N;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(in);
      if (in) {
        const int p = pos + __popcll(m & lt);
        seg_row[p] = r;
        seg_key[p] = k - n0;
      }
      pos += __popcll(m);
    }
  }
  __threadfence_block();
  __syncthreads();
  // split by entry, a wave per entry, still in row order: order[base + excl[e] ..] = the rows of entry e
  {
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int e = wave; e < EMA_E; e += 4) {
      int dst = base + excl[e];
      const int end = dst + hist[e];
      for (int i = 0; i < len && dst < end; i += 64) {
        const int j = i + lane;
        const bool hit = j < len && seg_key[base + j] == e;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        if (hit) order[dst + __popcll(m & lt)] = seg_row[base + j];
        dst += __popcll(m);
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  // the sums: lpe lanes per entry, rows added one after the other in fp32; and the restart candidate of a dead entry
  const int grp = tid / lpe, c = tid - grp * lpe, n_grp = 256 / lpe;
  float* __restrict__ sum = stats + N;
  float* __restrict__ cand = stats + N + (size_t)N * C;
  for (int e = grp; e < EMA_E; e += n_grp) {
    const int n = n0 + e;
    if (n >= N || c >= C) continue;
    const int cnt = hist[e];
    const int* __restrict__ ord = order + base + excl[e];
    float s = 0.f;
    for (int i = 0; i < cnt; i += EMA_BATCH) {
      float v[EMA_BATCH];
#pragma unroll
      for (int k = 0; k < EMA_BATCH; ++k) v[k] = Cvt<T>::to_f(z[(size_t)ord[min(i + k, cnt - 1)] * ldz + c]);
#pragma unroll
      for (int k = 0; k < EMA_BATCH; ++k)
        if (i + k < cnt) s += v[k];
    }
    sum[(size_t)n * C + c] = s;
    float cv = 0.f;
    if (cluster_size && cluster_size[n] < thr) {
      const uint64_t step = (uint64_t)ema_step[0];
      uint32_t w[4] = {(uint32_t)n, 0u, (uint32_t)step, (uint32_t)(step >> 32)};
      philox4x32_10(w, k0, k1);
      if ((int)(w[0] % (uint32_t)world) == rank) cv = Cvt<T>::to_f(z[(size_t)(w[1] % (uint32_t)rows) * ldz + c]);
    }
    cand[(size_t)n * C + c] = cv;
  }
}

__global__ __launch_bounds__(1024) void k_vq_ema_total(const float* __restrict__ count, const float* __restrict__ cs_old, int N, float d, float omd,
                                                       float thr, float* __restrict__ cs_new) {
  __shared__ float sh[1024];
  const int tid = threadIdx.x;
  float p = 0.f;
  for (int n = tid; n < N; n += 1024) {
    const float o = cs_old[n];
    const float v = o < thr ? thr : fmaf(d, o, omd * count[n]);
    cs_new[n] = v;
    p += v;
  }
  sh[tid] = p;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  if (tid == 0) cs_new[N] = sh[0];
}

template <typename T, bool COPY>
__global__ __launch_bounds__(256) void k_vq_ema_apply(const float* __restrict__ stats, float* __restrict__ cluster_size, float* __restrict__ embed_avg,
                                                      float* __restrict__ codebook, T* __restrict__ copy, float* __restrict__ cnorm,
                                                      int64_t* __restrict__ ema_step, const float* __restrict__ cs_new, int N, int C, float d, float omd,
                                                      float eps, float thr) {
  __shared__ float tile[EMA_TILE * (EMA_TILE + 1)];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * EMA_TILE, ne = min(EMA_TILE, N - n0);
  const float total = cs_new[N];
  const float denom = fmaf((float)N, eps, total);      // written out: -ffp-contract=on would fuse total + N * eps anyway
  const float* __restrict__ sum = stats + N;
  const float* __restrict__ cand = stats + N + (size_t)N * C;
  for (int i = tid; i < ne * C; i += 256) {
    const int e = i / C, c = i - e * C, n = n0 + e;
    const size_t gi = (size_t)n0 * C + i;
    float ea, cb;
    if (cluster_size[n] < thr) {          // the value from before this update: the lane of the entry writes the new one after the barrier
      cb = cand[gi];
      ea = thr * cb;
    } else {
      ea = fmaf(d, embed_avg[gi], omd * sum[gi]);
      const float smoothed = __fdiv_rn(cs_new[n] + eps, denom) * total;
      cb = __fdiv_rn(ea, smoothed);
    }
    embed_avg[gi] = ea;
    codebook[gi] = cb;
    float seen = cb;                       // the value the argmin reads
    if (COPY) {
      const T t = Cvt<T>::from_f(cb);
      copy[gi] = t;
      seen = Cvt<T>::to_f(t);
    }
    tile[e * (EMA_TILE + 1) + c] = seen;
  }
  __syncthreads();
  if (tid < ne) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = tile[tid * (EMA_TILE + 1) + c];
      s = fmaf(v, v, s);
    }
    cnorm[n0 + tid] = s;
    cluster_size[n0 + tid] = cs_new[n0 + tid];
  }
  if (blockIdx.x == 0 && tid == 0) ema_step[0] += 1;
}

// workspace layout (bytes): commitment partials | seg_row | seg_key | order | new cluster sizes + total
struct Ws {
  float* partial;
  int *seg_row, *seg_key, *order;
  float* cs_new;
};
Ws carve(void* ws, int rows, int N) {
  char* p = (char*)ws;
  Ws w;
  w.partial = (float*)p; p += align256((int64_t)ttv_cdiv(rows, VQC_ROWS) * 4);
  w.seg_row = (int*)p;   p += align256((int64_t)rows * 4);
  w.seg_key = (int*)p;   p += align256((int64_t)rows * 4);
  w.order = (int*)p;     p += align256((int64_t)rows * 4);
  w.cs_new = (float*)p;
  return w;
}

}  // namespace

int64_t ttvk_vq_train_workspace_bytes(int rows, int N) {
  return align256((int64_t)ttv_cdiv(rows, VQC_ROWS) * 4) + 3 * align256((int64_t)rows * 4) + align256(((int64_t)N + 1) * 4);
}

#define VQT_COMMON(what)                                                                                                      \
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, what ": dtype %d is neither TTV_BF16 nor TTV_F32", dtype);             \
  TTV_CHECK_ARG(C >= 1 && C <= TTV_MAX_TOKEN, what ": codebook dim %d unsupported (1..64)", C);                               \
  TTV_CHECK_ARG(rows >= 1 && rows < (1 << 24), what ": %d rows (1 .. 2^24 - 1: a per-entry count must stay exact in fp32)", rows)

int ttvk_vq_commit_forward(const void* z, int dtype, int ldz, const void* cb, int ldc, const int* idx, int rows, int N, int C, float* loss,
                           void* workspace, int64_t workspace_bytes, hipStream_t s) {
  VQT_COMMON("vq_commit_forward");
  TTV_CHECK_ARG(N >= 1 && ldz >= C && ldc >= C, "vq_commit_forward: %d entries, leading dims %d, %d for dim %d", N, ldz, ldc, C);
  TTV_CHECK_ARG(((uintptr_t)z | (uintptr_t)cb | (uintptr_t)workspace) % 16 == 0 && ((uintptr_t)idx | (uintptr_t)loss) % 4 == 0,
                "vq_commit_forward: a buffer is not aligned (z, codebook, workspace: 16 bytes; indices, loss: 4)");
  TTV_CHECK_ARG(workspace_bytes >= ttvk_vq_train_workspace_bytes(rows, N), "vq_commit_forward: workspace too small");
  const Ws w = carve(workspace, rows, N);
  const int nb = ttv_cdiv(rows, VQC_ROWS);
  if (dtype == TTV_BF16) hipLaunchKernelGGL((k_vq_commit_partial<bf16_t>), dim3(nb), dim3(256), 0, s, (const bf16_t*)z, ldz, (const bf16_t*)cb, ldc, idx, rows, N, C, w.partial);
  else hipLaunchKernelGGL((k_vq_commit_partial<float>), dim3(nb), dim3(256), 0, s, (const float*)z, ldz, (const float*)cb, ldc, idx, rows, N, C, w.partial);
  TTV_CHECK_LAUNCH("vq_commit_partial");
  hipLaunchKernelGGL(k_vq_commit_finish, dim3(1), dim3(256), 0, s, w.partial, nb, (float)(1.0 / ((double)rows * C)), loss);
  TTV_CHECK_LAUNCH("vq_commit_finish");
  return TTV_OK;
}

int ttvk_vq_commit_backward(const void* g, int ldg, const void* z, int ldz, const void* e, int lde, int dtype, int rows, int C, double scale,
                            void* dz, int ldd, hipStream_t s) {
  VQT_COMMON("vq_commit_backward");
  TTV_CHECK_ARG(ldg >= C && ldz >= C && lde >= C && ldd >= C, "vq_commit_backward: a leading dim is smaller than the codebook dim %d", C);
  TTV_CHECK_ARG(((uintptr_t)g | (uintptr_t)z | (uintptr_t)e | (uintptr_t)dz) % 16 == 0, "vq_commit_backward: a buffer is not 16-byte aligned");
  dim3 grid((unsigned)(((long)rows * C + 255) / 256));
  if (dtype == TTV_BF16) hipLaunchKernelGGL((k_vq_commit_bwd<bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)g, ldg, (const bf16_t*)z, ldz, (const bf16_t*)e, lde, rows, C, scale, (bf16_t*)dz, ldd);
  else hipLaunchKernelGGL((k_vq_commit_bwd<float>), grid, dim3(256), 0, s, (const float*)g, ldg, (const float*)z, ldz, (const float*)e, lde, rows, C, scale, (float*)dz, ldd);
  TTV_CHECK_LAUNCH("vq_commit_bwd");
  return TTV_OK;
}

int ttvk_vq_ema_stats(const void* z, int dtype, int ldz, const int* idx, int rows, int N, int C, const float* cluster_size, float dead_threshold,
                      uint64_t seed, const int64_t* ema_step, int rank, int world_size, float* stats, void* workspace, int64_t workspace_bytes,
                      hipStream_t s) {
  VQT_COMMON("vq_ema_stats");
  TTV_CHECK_ARG(N >= 1 && ldz >= C, "vq_ema_stats: %d entries, leading dim %d for dim %d", N, ldz, C);
  TTV_CHECK_ARG(world_size >= 1 && rank >= 0 && rank < world_size, "vq_ema_stats: rank %d of %d", rank, world_size);
  TTV_CHECK_ARG(!cluster_size || (ema_step && dead_threshold >= 0.f), "vq_ema_stats: restarts need the step counter and a threshold >= 0");
  TTV_CHECK_ARG(((uintptr_t)z | (uintptr_t)workspace) % 16 == 0 && ((uintptr_t)idx | (uintptr_t)stats | (uintptr_t)cluster_size) % 4 == 0 &&
                    (uintptr_t)ema_step % 8 == 0,
                "vq_ema_stats: a buffer is not aligned (z, workspace: 16 bytes; step: 8; indices, stats, cluster_size: 4)");
  TTV_CHECK_ARG(workspace_bytes >= ttvk_vq_train_workspace_bytes(rows, N), "vq_ema_stats: workspace too small");
  const Ws w = carve(workspace, rows, N);
  int lpe = 1;
  while (lpe < C) lpe *= 2;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  dim3 grid(ttv_cdiv(N, EMA_E));
  if (dtype == TTV_BF16) hipLaunchKernelGGL((k_vq_ema_stats<bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)z, ldz, idx, rows, N, C, lpe, cluster_size, dead_threshold, k0, k1, ema_step, rank, world_size, stats, w.seg_row, w.seg_key, w.order);
  else hipLaunchKernelGGL((k_vq_ema_stats<float>), grid, dim3(256), 0, s, (const float*)z, ldz, idx, rows, N, C, lpe, cluster_size, dead_threshold, k0, k1, ema_step, rank, world_size, stats, w.seg_row, w.seg_key, w.order);
  TTV_CHECK_LAUNCH("vq_ema_stats");
  return TTV_OK;
}

int ttvk_vq_ema_update(const float* stats, float* cluster_size, float* embed_avg, float* codebook, void* copy, int copy_dtype, float* cnorm,
                       int64_t* ema_step, int N, int C, float decay, float one_minus_decay, float eps, float dead_threshold, void* workspace,
                       int64_t workspace_bytes, hipStream_t s) {
  TTV_CHECK_ARG(copy_dtype == TTV_BF16 || copy_dtype == TTV_F32, "vq_ema_update: dtype %d is neither TTV_BF16 nor TTV_F32", copy_dtype);
  TTV_CHECK_ARG(N >= 1 && C >= 1 && C <= TTV_MAX_TOKEN, "vq_ema_update: codebook %d x %d unsupported (dim 1..64)", N, C);
  TTV_CHECK_ARG(decay > 0.f && decay < 1.f && one_minus_decay > 0.f && eps > 0.f && dead_threshold >= 0.f,
                "vq_ema_update: decay %g (0..1), eps %g (> 0), threshold %g (>= 0)", (double)decay, (double)eps, (double)dead_threshold);
  TTV_CHECK_ARG(((uintptr_t)stats | (uintptr_t)cluster_size | (uintptr_t)embed_avg | (uintptr_t)codebook | (uintptr_t)cnorm) % 4 == 0 &&
                    (uintptr_t)copy % 2 == 0 && (uintptr_t)ema_step % 8 == 0 && (uintptr_t)workspace % 16 == 0,
                "vq_ema_update: a buffer is not aligned (workspace: 16 bytes; step: 8; fp32 arrays: 4)");
  TTV_CHECK_ARG(copy_dtype == TTV_BF16 || copy == (void*)codebook, "vq_ema_update: an fp32 copy must be the codebook itself");
  TTV_CHECK_ARG(workspace_bytes >= ((int64_t)N + 1) * 4, "vq_ema_update: workspace too small");
  float* cs_new = (float*)workspace;       // N new cluster sizes and their sum (the statistics' use of the workspace is over: same stream)
  hipLaunchKernelGGL(k_vq_ema_total, dim3(1), dim3(1024), 0, s, stats, cluster_size, N, decay, one_minus_decay, dead_threshold, cs_new);
  TTV_CHECK_LAUNCH("vq_ema_total");
  dim3 grid(ttv_cdiv(N, EMA_TILE));
  if (copy_dtype == TTV_BF16) hipLaunchKernelGGL((k_vq_ema_apply<bf16_t, true>), grid, dim3(256), 0, s, stats, cluster_size, embed_avg, codebook, (bf16_t*)copy, cnorm, ema_step, cs_new, N, C, decay, one_minus_decay, eps, dead_threshold);
  else hipLaunchKernelGGL((k_vq_ema_apply<float, false>), grid, dim3(256), 0, s, stats, cluster_size, embed_avg, codebook, (float*)nullptr, cnorm, ema_step, cs_new, N, C, decay, one_minus_decay, eps, dead_threshold);
  TTV_CHECK_LAUNCH("vq_ema_apply");
  return TTV_OK;
}
