// Batch plans, device side (include/titok_hip.h, "batch plans"): the per-row tables of a ttv_batch - latent_rows, patch_rows, row_seq,
// rope_ids - are pure functions of cu_seqlens and clip_desc, so one kernel writes them in place behind the async copy of the host
// segment (ttv_plan_host.cpp) instead of the host building, staging and uploading 20 bytes per packed row.  Enqueue only.
#include <string.h>

#include "ttv_common.h"
#include "ttv_kernels.h"

// Clip b of the batch: rows [cu[b], cu[b+1]), its K latent rows first, then its P = gt * gh * gw patch rows in (t, h, w) raster order.
// Position of a clip's first entry in latent_rows: cu[b] - pbase[b] (pbase = clip_desc[b][6], the clip's first entry in patch_rows).
struct PlanRowsArgs {
  const int* cu;           // [n + 1]  (device copy of the host segment)
  const int* desc;         // [n, 8]
  int* latent_rows;        // [sum_tokens]
  int* patch_rows;         // [sum_patches]
  int* row_seq;            // [L]
  int* rope_ids;           // [L, 2] = four uint16: ids of axes t, h, w and the identity row
  int n, L, sum_tokens, sum_patches, n_ids;
};

// first b in [0, n) with end(b) > v, for a non-decreasing end() whose last value is > v
template <typename End>
__device__ __forceinline__ int plan_find(int n, int v, End end) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (end(mid) > v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// One thread per group of four consecutive entries of a table: 16-byte stores (every table starts 16-byte aligned, a group starts at a
// multiple of four), except the last group of a table whose length is no multiple of four - it stores its entries one by one, so no word
// behind a table is written.  Threads [0, gA): row_seq + rope_ids, [gA, gA + gB): latent_rows, [gA + gB, gA + gB + gC): patch_rows.
__global__ __launch_bounds__(256) void k_plan_rows(PlanRowsArgs a) {
  const int gA = (a.L + 3) >> 2, gB = (a.sum_tokens + 3) >> 2, gC = (a.sum_patches + 3) >> 2;
  int g = blockIdx.x * 256 + threadIdx.x;
  const int n = a.n;
  if (g < gA) {
    const int r0 = g * 4, cnt = min(4, a.L - r0);
    int b = plan_find(n, r0, [&](int i) { return a.cu[i + 1]; });
    int seq[4], w0[4], w1[4];
    int lo = a.cu[b], hi = a.cu[b + 1];
    int gh = a.desc[b * 8 + 4], gw = a.desc[b * 8 + 5];
    int K = (hi - lo) - a.desc[b * 8 + 3] * gh * gw;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = r0 + e;
      if (e < cnt) {
        while (r >= hi && b + 1 < n) {      // sequences are not empty: at most n steps in all
          ++b;
          lo = hi; hi = a.cu[b + 1];
          gh = a.desc[b * 8 + 4]; gw = a.desc[b * 8 + 5];
          K = (hi - lo) - a.desc[b * 8 + 3] * gh * gw;
        }
        const int i = r - lo;
        int t, h, w;
        if (i < K) t = h = w = i;
        else {
          const int j = i - K;
          w = min(j % gw + K, a.n_ids - 1);
          h = min((j / gw) % gh + K, a.n_ids - 1);
          t = min(j / (gw * gh) + K, a.n_ids - 1);
        }
        seq[e] = b;
        w0[e] = (int)(((unsigned)t & 0xFFFFu) | ((unsigned)h << 16));
        w1[e] = (int)(((unsigned)w & 0xFFFFu) | ((unsigned)a.n_ids << 16));
      } else {
        seq[e] = 0; w0[e] = 0; w1[e] = 0;
      }
    }
    if (cnt == 4) {
      *reinterpret_cast<int4*>(a.row_seq + r0) = make_int4(seq[0], seq[1], seq[2], seq[3]);
      int4* ids = reinterpret_cast<int4*>(a.rope_ids + (size_t)r0 * 2);
      ids[0] = make_int4(w0[0], w1[0], w0[1], w1[1]);
      ids[1] = make_int4(w0[2], w1[2], w0[3], w1[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (e < cnt) {
          a.row_seq[r0 + e] = seq[e];
          a.rope_ids[(size_t)(r0 + e) * 2] = w0[e];
          a.rope_ids[(size_t)(r0 + e) * 2 + 1] = w1[e];
        }
    }
    return;
  }
  g -= gA;
  // latent_rows[m] / patch_rows[m]: the packed row of the m-th latent / patch token.  first(b) = the clip's first entry of the table.
  const bool lat = g < gB;
  if (!lat) g -= gB;
  if (g >= (lat ? gB : gC)) return;
  const int total = lat ? a.sum_tokens : a.sum_patches;
  int* out = lat ? a.latent_rows : a.patch_rows;
  auto pbase = [&](int i) { return i < n ? a.desc[i * 8 + 6] : a.sum_patches; };
  auto first = [&](int i) { return lat ? a.cu[i] - pbase(i) : pbase(i); };
  const int m0 = g * 4, cnt = min(4, total - m0);
  int b = plan_find(n, m0, [&](int i) { return first(i + 1); });
  int v[4];
  int end = first(b + 1);
  // entry m of clip b is row cu[b] + (m - first(b)) of the latent rows, and K_b rows further down for a patch: cu[b+1] - (first(b+1) - m)
  int shift = lat ? a.cu[b] - first(b) : a.cu[b + 1] - end;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int m = m0 + e;
    if (e < cnt) {
      while (m >= end && b + 1 < n) {       // skips clips without latent tokens; at most n steps in all
        ++b;
        end = first(b + 1);
        shift = lat ? a.cu[b] - first(b) : a.cu[b + 1] - end;
      }
      v[e] = m + shift;
    } else v[e] = 0;
  }
  if (cnt == 4) *reinterpret_cast<int4*>(out + m0) = make_int4(v[0], v[1], v[2], v[3]);
  else {
#pragma unroll
    for (int e = 0; e < 3; ++e)
      if (e < cnt) out[m0 + e] = v[e];
  }
}

extern "C" int ttv_plan_rows_build(const ttv_plan_sizes* sz, const int32_t* host_segment, int32_t* dev_segment, const float* base_cos,
                                   const float* base_sin, int n_freqs, float* rope_cs, const float* rope_base, ttv_batch* batch, void* stream) {
  TTV_CHECK_ARG(sz && host_segment && dev_segment && base_cos && base_sin && rope_cs && batch, "plan_rows_build: null argument");
  TTV_CHECK_ARG(sz->n_clips >= 1 && sz->total_rows >= 1 && sz->sum_tokens >= 0 && sz->sum_patches >= 1 &&
                    (int64_t)sz->sum_tokens + sz->sum_patches == sz->total_rows && sz->total_rows <= INT32_MAX / 2,
                "plan_rows_build: sizes are not those of ttv_plan_rows_sizes");
  TTV_CHECK_ARG(sz->n_rope_ids >= 1 && sz->n_rope_ids <= 65535, "plan_rows_build: %d rotary position ids", sz->n_rope_ids);
  TTV_CHECK_ARG(n_freqs >= 1 && 3 * n_freqs <= 32, "plan_rows_build: bad rotary table shape");
  TTV_CHECK_ARG(sz->host_words >= 4 && sz->dev_words >= sz->host_words && ((uintptr_t)dev_segment & 15) == 0,
                "plan_rows_build: the device segment must be 16-byte aligned and hold dev_words words");
  hipStream_t s = (hipStream_t)stream;
  // the caller's host segment is pinned and stays untouched until the stream has passed this copy
  if (hipMemcpyAsync(dev_segment, host_segment, (size_t)sz->host_words * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
    (void)hipGetLastError();
    ttv_set_error("plan_rows_build: hipMemcpyAsync failed");
    return TTV_ERR_LAUNCH;
  }
  PlanRowsArgs a;
  a.cu = dev_segment + sz->off_cu_seqlens;
  a.desc = dev_segment + sz->off_clip_desc;
  a.latent_rows = dev_segment + sz->off_latent_rows;
  a.patch_rows = dev_segment + sz->off_patch_rows;
  a.row_seq = dev_segment + sz->off_row_seq;
  a.rope_ids = dev_segment + sz->off_rope_ids;
  a.n = sz->n_clips; a.L = sz->total_rows; a.sum_tokens = sz->sum_tokens; a.sum_patches = sz->sum_patches; a.n_ids = sz->n_rope_ids;
  const int groups = (a.L + 3) / 4 + (a.sum_tokens + 3) / 4 + (a.sum_patches + 3) / 4;
  hipLaunchKernelGGL(k_plan_rows, dim3(ttv_cdiv(groups, 256)), dim3(256), 0, s, a);
  TTV_CHECK_LAUNCH("plan_rows");
  // rope_cs [L, 64] by the kernel ttv_rope_table_build runs (it reads the row_seq written above: stream order)
  const int rc = ttvk_rope_build(base_cos, base_sin, sz->n_rope_ids, n_freqs, a.desc, a.cu, a.row_seq, rope_cs, a.L, s);
  if (rc != TTV_OK) return rc;

  memset(batch, 0, sizeof(*batch));
  batch->n_clips = sz->n_clips;
  batch->total_rows = sz->total_rows;
  batch->sum_tokens = sz->sum_tokens;
  batch->sum_patches = sz->sum_patches;
  batch->max_patches_per_clip = sz->max_patches_per_clip;
  batch->cu_seqlens = a.cu;
  batch->latent_rows = a.latent_rows;
  batch->patch_rows = a.patch_rows;
  batch->clip_desc = a.desc;
  batch->rope_cs = rope_cs;
  batch->blocks64 = dev_segment + sz->off_blocks64;
  batch->row_seq = a.row_seq;
  batch->n_blocks64 = sz->n_blocks64;
  if (rope_base) {
    batch->rope_ids = a.rope_ids;
    batch->rope_base = rope_base;
  }
  return TTV_OK;
}

extern "C" int ttv_plan_attn_set(const ttv_plan_attn* sz, const int32_t* host_tables, int32_t* dev_tables, ttv_batch* batch, void* stream) {
  TTV_CHECK_ARG(sz && host_tables && dev_tables && batch, "plan_attn_set: null argument");
  TTV_CHECK_ARG(sz->n_qblocks >= 1 && sz->words >= 4 * (int64_t)sz->n_qblocks && ((uintptr_t)dev_tables & 15) == 0,
                "plan_attn_set: sizes are not those of ttv_plan_attn_sizes, or the device buffer is not 16-byte aligned");
  if (hipMemcpyAsync(dev_tables, host_tables, (size_t)sz->words * 4, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) {
    (void)hipGetLastError();
    ttv_set_error("plan_attn_set: hipMemcpyAsync failed");
    return TTV_ERR_LAUNCH;
  }
  batch->qblocks = dev_tables + sz->off_qblocks;
  batch->n_qblocks = sz->n_qblocks;
  batch->qblocks_paired = 0;
  batch->qblocks_all_full = sz->qblocks_all_full;
  batch->items64 = nullptr;
  batch->n_items64 = 0;
  batch->qblocks_latent = sz->n_qblocks_latent ? dev_tables + sz->off_qblocks_latent : nullptr;
  batch->n_qblocks_latent = sz->n_qblocks_latent;
  batch->qblocks_patch = sz->n_qblocks_patch ? dev_tables + sz->off_qblocks_patch : nullptr;
  batch->n_qblocks_patch = sz->n_qblocks_patch;
  batch->tokens_per_clip = sz->tokens_per_clip;
  return TTV_OK;
}
