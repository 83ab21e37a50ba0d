// Kernels over a list of parameter tensors: gradient-norm clip + AdamW with the scalar state on the host or on the device, per-parameter
// gradient norms, and the weight EMA (update, apply / restore).  All of them read one device table of OptEntry and one list of
// (entry, first element) chunks of OPT_CHUNK elements, one block per chunk (titok_video_amd/optim.py and ema.py build both).
#include "ttv_common.h"

// ------------------------------------------------------------------------------------------------ optimizer step
// Gradient-norm clip + AdamW over a list of parameter tensors in two launches (reference train.py:76-77 clip_gradients, :183-190 AdamW;
// what torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW compute).  torch's multi-tensor path takes 7 launches and ~230 us per
// step for the 7 M parameters of the tiny tokenizer (98 MB of traffic in bf16: 0.4 TB/s); these two move the same bytes once:
//   k_opt_gradsq: one block per 8 192-element chunk of a tensor -> partial[chunk] = sum g^2 (fixed order inside the block)
//   k_opt_adamw : every block first sums ALL partials in one fixed order (the same value in every block, bit-reproducible run to run -
//                 no atomics), derives the clip factor min(1, max_norm / (norm + 1e-6)) (NaN for a NaN norm, as torch), then updates its chunk; the gradient is scaled in
//                 registers and NOT rewritten (clip_grad_norm_ scales p.grad in place: the only difference a caller could see).
// fp32 arithmetic whatever the tensors' dtype (fp32 or bf16; state in the parameter's dtype), operation order of torch's fused kernel:
//   p -= lr wd p ; m = lerp(m, g, 1 - b1) ; v = b2 v + (1 - b2) g g ; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
#define OPT_CHUNK 8192
struct OptEntry { void* p; const void* g; void* m; void* v; long long n; };
template <typename T> struct OptVec;
template <> struct OptVec<float> {
  static __device__ __forceinline__ void load(const float* q, float (&o)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(q), b = *reinterpret_cast<const f32x4*>(q + 4);
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
  }
  static __device__ __forceinline__ void store(float* q, const float (&o)[8]) {
    *reinterpret_cast<f32x4*>(q) = (f32x4){o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(q + 4) = (f32x4){o[4], o[5], o[6], o[7]};
  }
};
template <> struct OptVec<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* q, float (&o)[8]) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(q);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)a[e];
  }
  static __device__ __forceinline__ void store(bf16_t* q, const float (&o)[8]) {
    bf16x8 a;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = (bf16_t)o[e];
    *reinterpret_cast<bf16x8*>(q) = a;
  }
};
// The walk of every kernel below over its block's chunk, elements [first, end) of table entry e.  With every tensor the kernel touches
// on the 16-byte grid (the caller ORs exactly those pointers into `ptrs`): vec(i) on whole groups of 8 from first + tid * 8 in strides
// of 2 048, then one(j) on the tail - under 8 elements, all on the one thread whose next group the end cuts short, in index order.
// Off the grid: one(j) element-strided over the whole chunk.
struct OptChunk { OptEntry e; long long first, end; };
__device__ __forceinline__ OptChunk opt_chunk(const OptEntry* __restrict__ tab, const int2* __restrict__ chunks) {
  const int2 c = chunks[blockIdx.x];
  OptChunk k;
  k.e = tab[c.x];
  k.first = c.y;
  k.end = k.e.n < (long long)c.y + OPT_CHUNK ? k.e.n : (long long)c.y + OPT_CHUNK;
  return k;
}
template <typename Vec, typename One>
__device__ __forceinline__ void opt_walk(const OptChunk& k, uintptr_t ptrs, Vec vec, One one) {
  if ((ptrs & 15) == 0) {
    long long i = k.first + threadIdx.x * 8;
    for (; i + 8 <= k.end; i += 256 * 8) vec(i);
    for (; i < k.end; ++i) one(i);
  } else {
    for (long long j = k.first + threadIdx.x; j < k.end; j += 256) one(j);
  }
}
// block-wide sum in a fixed order: lanes by DPP / permlane inside the wave, the four waves through LDS
__device__ __forceinline__ float opt_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
template <typename T>
__global__ __launch_bounds__(256) void k_opt_gradsq(const OptEntry* __restrict__ tab, const int2* __restrict__ chunks, float* __restrict__ partial) {
  __shared__ float red[4];
  const OptChunk c = opt_chunk(tab, chunks);
  const T* g = (const T*)c.e.g;
  float acc = 0.f;
  opt_walk(c, (uintptr_t)g,
           [&](long long i) {
             float v[8];
             OptVec<T>::load(g + i, v);
#pragma unroll
             for (int k = 0; k < 8; ++k) acc = fmaf(v[k], v[k], acc);
           },
           [&](long long j) { const float v = (float)g[j]; acc = fmaf(v, v, acc); });
  const float t = opt_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
// Per-parameter gradient norms (the log of reference train.py:78-79, :102-103: Lightning's grad_norm(module, 2)) from the partials
// k_opt_gradsq has just written: the segmented sum of numbers the step already has, in one launch.  The chunk table lists every
// entry's chunks together, entries ascending (optim.py builds it so): a thread finds its entry's first chunk by bisection and adds the
// entry's partials in ascending chunk order - a fixed order, no atomics, identical calls give identical bits.  The last block sums
// ALL partials of the table in ascending order for slot n_entries: the waves stage 2 048 of them at a time in LDS and one lane adds
// (a few hundred terms for the tiny tokenizer; the per-entry sums are a handful each, 44 for its largest matrix).
// Both sums are one lane's dependent chain, as long as the chunk list: the price of the ascending order include/titok_hip.h
// promises.  Tiny tokenizer (under 900 chunks): lost in the 0.1 ms the log adds to a step.  At the size of the base configs' towers
// (20 480 chunks = 168 M elements, the largest entry 2 048 chunks; tools/val_bench.py builds that table) the launch takes 0.30 ms,
// once per logged step, beside a training step of tens of milliseconds: not worth a tree, which would change the stated order.
#define OPT_NORM_TILE 2048
__global__ __launch_bounds__(256) void k_opt_param_norms(const int2* __restrict__ chunks, int n_chunks, int n_entries,
                                                         const float* __restrict__ partial, float* __restrict__ norms) {
  __shared__ float tile[OPT_NORM_TILE];
  if (blockIdx.x == gridDim.x - 1) {
    float acc = 0.f;
    for (int c0 = 0; c0 < n_chunks; c0 += OPT_NORM_TILE) {
      const int n = n_chunks - c0 < OPT_NORM_TILE ? n_chunks - c0 : OPT_NORM_TILE;
      __syncthreads();
      for (int i = threadIdx.x; i < n; i += 256) tile[i] = partial[c0 + i];
      __syncthreads();
      if (threadIdx.x == 0)
        for (int i = 0; i < n; ++i) acc += tile[i];
    }
    if (threadIdx.x == 0) norms[n_entries] = sqrtf(acc);
    return;
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  int lo = 0, hi = n_chunks;             // the first chunk whose entry is >= e
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (chunks[mid].x < e) lo = mid + 1;
    else hi = mid;
  }
  float acc = 0.f;                       // an entry without elements has no chunk: norm 0
  for (int c = lo; c < n_chunks && chunks[c].x == e; ++c) acc += partial[c];
  norms[e] = sqrtf(acc);
}
// om_beta1 / om_beta2 are 1 - beta formed in double by the caller and rounded once, as bc1 and bc2_sqrt are (1.0f - (float)0.999 is
// 1.3e-5 below 0.001: a constant bias of that size on exp_avg_sq); the lerp's 1 - w for beta1 <= 0.5 is then beta1 itself.
struct OptHyper { float lr, beta1, beta2, om_beta1, om_beta2, eps, wd, bc1, bc2_sqrt, max_norm; };
__device__ __forceinline__ void opt_update(float& p, float g, float& m, float& v, const OptHyper& h, float step_size) {
  p -= h.lr * h.wd * p;
  const float w = h.om_beta1;
  m = w < 0.5f ? m + w * (g - m) : g - (g - m) * h.beta1;        // at::native::lerp
  v = h.beta2 * v + h.om_beta2 * g * g;
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p -= step_size * m / denom;
}
// The update of the block's chunk: the one body of k_opt_adamw and k_opt_adamw_dev, which differ only in where h.lr, h.bc1, h.bc2_sqrt
// and coef come from - equal scalars give equal bits by construction.
template <typename T>
__device__ __forceinline__ void opt_adamw_chunk(const OptEntry* __restrict__ tab, const int2* __restrict__ chunks, const OptHyper& h, float coef,
                                                float step_size) {
  const OptChunk c = opt_chunk(tab, chunks);
  T* p = (T*)c.e.p; const T* g = (const T*)c.e.g; T* m = (T*)c.e.m; T* v = (T*)c.e.v;
  opt_walk(c, (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v,
           [&](long long i) {
             float pv[8], gv[8], mv[8], vv[8];
             OptVec<T>::load(p + i, pv); OptVec<T>::load(g + i, gv); OptVec<T>::load(m + i, mv); OptVec<T>::load(v + i, vv);
#pragma unroll
             for (int k = 0; k < 8; ++k) opt_update(pv[k], gv[k] * coef, mv[k], vv[k], h, step_size);
             OptVec<T>::store(p + i, pv); OptVec<T>::store(m + i, mv); OptVec<T>::store(v + i, vv);
           },
           [&](long long j) {
             float pv = (float)p[j], mv = (float)m[j], vv = (float)v[j];
             opt_update(pv, (float)g[j] * coef, mv, vv, h, step_size);
             p[j] = (T)pv; m[j] = (T)mv; v[j] = (T)vv;
           });
}
// The gradient norm from the partials - thread-strided sums, then opt_block_sum - and the clip factor: the one body of k_opt_adamw
// (every block for itself) and k_opt_prepare (one block, once), so both paths hold the same bits by construction.  Without partials:
// norm 0, factor 1.
__device__ __forceinline__ float opt_norm_coef(const float* __restrict__ partial, int n_partial, float max_norm, float* red, float& coef) {
  coef = 1.0f;
  if (n_partial <= 0) return 0.f;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
  const float norm = sqrtf(opt_block_sum(acc, red));
  if (max_norm > 0.f) {
    // torch.clamp(max_norm / (norm + 1e-6), max=1): a NaN norm gives a NaN factor that reaches every gradient (fminf would return 1)
    const float r = max_norm / (norm + 1e-6f);
    coef = r >= 1.0f ? 1.0f : r;
  }
  return norm;
}
template <typename T>
__global__ __launch_bounds__(256) void k_opt_adamw(const OptEntry* __restrict__ tab, const int2* __restrict__ chunks, const float* __restrict__ partial,
                                                   int n_partial, OptHyper h, float* __restrict__ out_norm) {
  __shared__ float red[4];
  float coef;
  const float norm = opt_norm_coef(partial, n_partial, h.max_norm, red, coef);
  if (out_norm && n_partial > 0 && blockIdx.x == 0 && threadIdx.x == 0) out_norm[0] = norm;
  opt_adamw_chunk<T>(tab, chunks, h, coef, h.lr / h.bc1);
}

// The step with its scalar state on the device (include/titok_hip.h, ttv_opt_state): k_opt_prepare, one block, does once what every
// block of k_opt_adamw does for itself - the norm and the clip factor, through the same opt_norm_coef - and what the host does for
// k_opt_adamw: t, both bias corrections and the learning rate in double, each rounded to float once.  k_opt_adamw_dev is
// k_opt_adamw's update (the same opt_adamw_chunk) with those four floats read from the block.
// The doubles are formed without contraction: the schedule is held bit for bit to the reference's Python, which has no fma.
__device__ __forceinline__ double opt_schedule_lr(const ttv_opt_schedule& s, long long index) {
#pragma clang fp contract(off)
  double factor;
  if (index < s.warmup_steps) {
    factor = (double)index / (double)(s.warmup_steps > 1 ? s.warmup_steps : 1);
  } else {
    const long long span = s.training_steps - s.warmup_steps;
    const double progress = (double)(index - s.warmup_steps) / (double)(span > 1 ? span : 1);
    const double c = 0.5 * (1.0 + cos(3.141592653589793 * s.num_cycles * 2.0 * progress));
    const double ratio = c > 0.0 ? c : 0.0;
    factor = (s.end_lr + (s.base_lr - s.end_lr) * ratio) / s.base_lr;
  }
  return s.initial_lr * factor;
}
__global__ __launch_bounds__(256) void k_opt_prepare(ttv_opt_state* __restrict__ st, ttv_opt_schedule sched, double beta1, double beta2,
                                                     double lr_constant, float max_norm, const float* __restrict__ partial, int n_partial,
                                                     int flags, float* __restrict__ out_norm) {
  __shared__ float red[4];
  float coef;
  const float norm = opt_norm_coef(partial, n_partial, max_norm, red, coef);
  if (threadIdx.x != 0) return;
  if (out_norm && n_partial > 0) out_norm[0] = norm;
  st->norm = norm;
  st->clip_coef = coef;
  if ((flags & TTV_OPT_SKIP_NONFINITE) && !(fabsf(norm) <= 3.402823466e38f)) {          // NaN or infinite
    st->skip_now = 1;
    st->skipped += 1;
    return;
  }
  const long long u = st->updates, t = u + 1;
  long long index = 0;
  double lr = lr_constant;
  if (sched.kind == TTV_OPT_SCHEDULE_COSINE) {
    index = sched.first + sched.stride * u;
    if (index < 0) index = 0;
    lr = opt_schedule_lr(sched, index);
  }
  st->skip_now = 0;
  st->schedule_index = index;
  st->lr = (float)lr;
  st->bc1 = (float)(1.0 - pow(beta1, (double)t));
  st->bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)t));
  st->updates = t;
}
template <typename T>
__global__ __launch_bounds__(256) void k_opt_adamw_dev(const OptEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                       const ttv_opt_state* __restrict__ st, OptHyper h) {
  if (st->skip_now) return;          // the same word for every block: nobody touches a tensor
  h.lr = st->lr; h.bc1 = st->bc1; h.bc2_sqrt = st->bc2_sqrt;
  opt_adamw_chunk<T>(tab, chunks, h, st->clip_coef, h.lr / h.bc1);
}

// ------------------------------------------------------------------------------------------------ weight EMA
// fp32 shadow weights of a parameter list (titok_video_amd/ema.py::WeightEMA; not a reference module: the reference validates its raw
// weights).  The OptEntry table and chunk list of the optimizer step, one block per chunk, the same opt_walk:
//   k_opt_ema_update  : p = parameter (T, read only), m = shadow (ALWAYS float, whatever T: a bf16 shadow at decay 0.9999 never moves,
//                       the increment is below half an ulp), g and v unused.  d = (float)p - s ; s = s + weight d, in that order in fp32
//                       (the compiler may contract the last two roundings into one fma).  12 bytes per element for fp32 parameters
//                       (4 read + 4 read + 4 written), 10 for bf16.
//   k_opt_ema_exchange: p (written), m = shadow (const float), v = backup (T, the size of p).  mode 0: backup = p ; p = (T)shadow - for
//                       bf16 the round-to-nearest-even cast of OptVec<bf16_t>::store.  mode 1: p = backup.  The shadow is only read.
// weight = 1 - decay is formed in double by the caller and rounded once, as om_beta1 / om_beta2 above are.
template <typename T>
__global__ __launch_bounds__(256) void k_opt_ema_update(const OptEntry* __restrict__ tab, const int2* __restrict__ chunks, float weight) {
  const OptChunk c = opt_chunk(tab, chunks);
  const T* p = (const T*)c.e.p; float* s = (float*)c.e.m;
  opt_walk(c, (uintptr_t)p | (uintptr_t)s,
           [&](long long i) {
             float pv[8], sv[8];
             OptVec<T>::load(p + i, pv); OptVec<float>::load(s + i, sv);
#pragma unroll
             for (int k = 0; k < 8; ++k) { const float d = pv[k] - sv[k]; sv[k] = sv[k] + weight * d; }
             OptVec<float>::store(s + i, sv);
           },
           [&](long long j) { const float sv = s[j], d = (float)p[j] - sv; s[j] = sv + weight * d; });
}
template <typename T>
__global__ __launch_bounds__(256) void k_opt_ema_exchange(const OptEntry* __restrict__ tab, const int2* __restrict__ chunks, int mode) {
  const OptChunk c = opt_chunk(tab, chunks);
  T* p = (T*)c.e.p; const float* s = (const float*)c.e.m; T* b = (T*)c.e.v;
  opt_walk(c, (uintptr_t)p | (uintptr_t)s | (uintptr_t)b,
           [&](long long i) {
             if (mode == 0) {
               // the parameter's bits go to the backup as they are (OptVec<bf16_t> would widen and round: a signalling NaN would come back quiet)
               *reinterpret_cast<uint4*>(b + i) = *reinterpret_cast<const uint4*>(p + i);
               if (sizeof(T) == 4) *reinterpret_cast<uint4*>(b + i + 4) = *reinterpret_cast<const uint4*>(p + i + 4);
               float sv[8];
               OptVec<float>::load(s + i, sv);
               OptVec<T>::store(p + i, sv);
             } else {
               *reinterpret_cast<uint4*>(p + i) = *reinterpret_cast<const uint4*>(b + i);
               if (sizeof(T) == 4) *reinterpret_cast<uint4*>(p + i + 4) = *reinterpret_cast<const uint4*>(b + i + 4);
             }
           },
           [&](long long j) {
             if (mode == 0) { b[j] = p[j]; p[j] = (T)s[j]; }
             else p[j] = b[j];
           });
}

// k<bf16_t> or k<float> by dtype (checked by the caller), one block of 256 per chunk; every templated kernel takes the table and the chunk list first
#define OPT_LAUNCH(k, dtype, table, chunks, n_chunks, stream, ...)                                                                              \
  do {                                                                                                                                            \
    if ((dtype) == TTV_BF16)                                                                                                                      \
      hipLaunchKernelGGL((k<bf16_t>), dim3(n_chunks), dim3(256), 0, (hipStream_t)(stream), (const OptEntry*)(table), (const int2*)(chunks), __VA_ARGS__); \
    else                                                                                                                                          \
      hipLaunchKernelGGL((k<float>), dim3(n_chunks), dim3(256), 0, (hipStream_t)(stream), (const OptEntry*)(table), (const int2*)(chunks), __VA_ARGS__);  \
  } while (0)

extern "C" {

int ttv_opt_grad_sumsq(const void* table, const int32_t* chunks, int n_chunks, int dtype, float* partials, void* stream) {
  if (n_chunks == 0) return TTV_OK;
  TTV_CHECK_ARG(n_chunks > 0 && table && chunks && partials, "opt_grad_sumsq: null buffer");
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "opt_grad_sumsq: dtype");
  OPT_LAUNCH(k_opt_gradsq, dtype, table, chunks, n_chunks, stream, partials);
  TTV_CHECK_LAUNCH("opt_grad_sumsq");
  return TTV_OK;
}

int ttv_opt_param_norms(const void* table, const int32_t* chunks, int n_chunks, int n_entries, const float* partials, float* norms,
                        void* stream) {
  TTV_CHECK_ARG(n_chunks >= 0 && n_entries >= 0 && norms, "opt_param_norms: %d chunks, %d entries, or no destination", n_chunks, n_entries);
  TTV_CHECK_ARG(n_chunks == 0 || (table && chunks && partials), "opt_param_norms: null buffer");
  hipLaunchKernelGGL(k_opt_param_norms, dim3((unsigned)((n_entries + 255) / 256 + 1)), dim3(256), 0, (hipStream_t)stream, (const int2*)chunks,
                     n_chunks, n_entries, partials, norms);
  TTV_CHECK_LAUNCH("opt_param_norms");
  return TTV_OK;
}

int ttv_opt_adamw_step(const void* table, const int32_t* chunks, int n_chunks, int dtype, const float* partials, int n_partials, float lr,
                       float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                       float bias_correction1, float bias_correction2_sqrt, float max_norm, float* out_norm, void* stream) {
  if (n_chunks == 0) return TTV_OK;
  TTV_CHECK_ARG(n_chunks > 0 && table && chunks, "opt_adamw_step: null buffer");
  TTV_CHECK_ARG(n_partials == 0 || partials, "opt_adamw_step: partials missing");
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "opt_adamw_step: dtype");
  TTV_CHECK_ARG(bias_correction1 > 0.f && bias_correction2_sqrt > 0.f, "opt_adamw_step: bias corrections must be positive");
  const OptHyper h = {lr, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt, max_norm};
  OPT_LAUNCH(k_opt_adamw, dtype, table, chunks, n_chunks, stream, partials, n_partials, h, out_norm);
  TTV_CHECK_LAUNCH("opt_adamw_step");
  return TTV_OK;
}

int ttv_opt_prepare(ttv_opt_state* state, ttv_opt_schedule schedule, double beta1, double beta2, double lr_constant, float max_norm,
                    const float* partials, int n_partials, int flags, float* out_norm, void* stream) {
  TTV_CHECK_ARG(state, "opt_prepare: null state");
  TTV_CHECK_ARG(n_partials >= 0, "opt_prepare: n_partials %d is negative", n_partials);
  TTV_CHECK_ARG(n_partials == 0 || partials, "opt_prepare: null partials");
  TTV_CHECK_ARG(schedule.kind == TTV_OPT_SCHEDULE_NONE || schedule.kind == TTV_OPT_SCHEDULE_COSINE, "opt_prepare: schedule kind %d is unknown",
                schedule.kind);
  if (schedule.kind == TTV_OPT_SCHEDULE_COSINE) {
    TTV_CHECK_ARG(schedule.warmup_steps >= 0 && schedule.training_steps >= schedule.warmup_steps,
                  "opt_prepare: training_steps %lld below warmup_steps %lld (or a negative warm-up)", (long long)schedule.training_steps,
                  (long long)schedule.warmup_steps);
    TTV_CHECK_ARG(schedule.stride >= 1, "opt_prepare: stride %lld is below 1", (long long)schedule.stride);
  }
  hipLaunchKernelGGL(k_opt_prepare, dim3(1), dim3(256), 0, (hipStream_t)stream, state, schedule, beta1, beta2, lr_constant, max_norm, partials,
                     n_partials, flags, out_norm);
  TTV_CHECK_LAUNCH("opt_prepare");
  return TTV_OK;
}

int ttv_opt_adamw_step_dev(const void* table, const int32_t* chunks, int n_chunks, int dtype, const ttv_opt_state* state, float beta1,
                           float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay, void* stream) {
  TTV_CHECK_ARG(state, "opt_adamw_step_dev: null state");
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "opt_adamw_step_dev: dtype");
  if (n_chunks == 0) return TTV_OK;
  TTV_CHECK_ARG(n_chunks > 0 && table && chunks, "opt_adamw_step_dev: null buffer");
  const OptHyper h = {0.f, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, 1.f, 1.f, 0.f};          // lr, bc1, bc2_sqrt: from the block
  OPT_LAUNCH(k_opt_adamw_dev, dtype, table, chunks, n_chunks, stream, state, h);
  TTV_CHECK_LAUNCH("opt_adamw_step_dev");
  return TTV_OK;
}

int ttv_opt_ema_update(const void* table, const int32_t* chunks, int n_chunks, int dtype, float weight, void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "opt_ema_update: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  if (n_chunks == 0) return TTV_OK;
  TTV_CHECK_ARG(n_chunks > 0 && table && chunks, "opt_ema_update: null buffer");
  // s + 0 * d is s only for finite d and s other than -0: weight 0 keeps every shadow bit by not launching
  if (weight == 0.0f) return TTV_OK;
  OPT_LAUNCH(k_opt_ema_update, dtype, table, chunks, n_chunks, stream, weight);
  TTV_CHECK_LAUNCH("opt_ema_update");
  return TTV_OK;
}

int ttv_opt_ema_exchange(const void* table, const int32_t* chunks, int n_chunks, int dtype, int mode, void* stream) {
  TTV_CHECK_ARG(dtype == TTV_BF16 || dtype == TTV_F32, "opt_ema_exchange: dtype %d is neither TTV_BF16 nor TTV_F32", dtype);
  TTV_CHECK_ARG(mode == 0 || mode == 1, "opt_ema_exchange: mode %d is neither 0 (apply) nor 1 (restore)", mode);
  if (n_chunks == 0) return TTV_OK;
  TTV_CHECK_ARG(n_chunks > 0 && table && chunks, "opt_ema_exchange: null buffer");
  OPT_LAUNCH(k_opt_ema_exchange, dtype, table, chunks, n_chunks, stream, mode);
  TTV_CHECK_LAUNCH("opt_ema_exchange");
  return TTV_OK;
}

}  // extern "C"
