// Batch plans without Python (include/titok_hip.h, "batch plans"): the host tables of a ttv_batch - cu_seqlens, clip descriptors,
// the attention backward's 64-row blocks, the XCD-interleaved attention work tables - and the rotary base table.
// Plain C++: no HIP call, no device, no environment read.  Every table is built exactly as titok_video_amd/plan.py builds it
// (BatchPlan is the definition; tests/test_native_plan_cpu.py compares element for element).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/titok_hip.h"

void ttv_set_error(const char* fmt, ...);      // ttv_api.hip (thread-local message behind ttv_error_string)

#define PLAN_CHECK(cond, ...)       \
  do {                              \
    if (!(cond)) {                  \
      ttv_set_error(__VA_ARGS__);   \
      return TTV_ERR_INVALID;       \
    }                               \
  } while (0)

namespace {

constexpr int QBLOCK = 128;          // query rows per attention workgroup (ttv_attn.hip QB)
constexpr int ATTN_SLOTS = 1024;     // plan.py ATTN_SLOTS: below this many items the last third of every sequence's blocks are half items
constexpr int XCDS = 8;

inline int64_t pad4(int64_t words) { return (words + 3) / 4 * 4; }      // every table starts 16-byte aligned

// ---- rows -------------------------------------------------------------------------------------------------------------------------------
struct Rows {
  std::vector<int32_t> grid;      // [n,3] patch grid
  std::vector<int32_t> patches;   // [n]   P_b
  std::vector<int32_t> cu;        // [n+1]
  ttv_plan_sizes sz;
};

int rows_geometry(const int32_t* pixel_dims, const int32_t* token_counts, int n_clips, const int32_t* patch, Rows& r) {
  PLAN_CHECK(pixel_dims && token_counts && patch, "plan: null argument");
  PLAN_CHECK(n_clips >= 1, "plan: no clips (n_clips = %d)", n_clips);
  PLAN_CHECK(patch[0] > 0 && patch[1] > 0 && patch[2] > 0, "plan: patch (%d, %d, %d) is not positive", patch[0], patch[1], patch[2]);
  r.grid.resize((size_t)3 * n_clips);
  r.patches.resize(n_clips);
  r.cu.assign((size_t)n_clips + 1, 0);
  int64_t rows = 0, sum_k = 0, sum_p = 0, max_p = 0, max_s = 0, max_id = 0;
  for (int b = 0; b < n_clips; ++b) {
    const int32_t* pd = pixel_dims + 3 * b;
    int64_t p = 1, gmax = 0;
    for (int a = 0; a < 3; ++a) {
      PLAN_CHECK(pd[a] > 0 && pd[a] % patch[a] == 0, "plan: clip %d shape (%d, %d, %d) is not a positive multiple of patch size (%d, %d, %d)", b,
                 pd[0], pd[1], pd[2], patch[0], patch[1], patch[2]);
      const int32_t g = pd[a] / patch[a];
      r.grid[3 * b + a] = g;
      p *= g;
      gmax = std::max<int64_t>(gmax, g);
    }
    const int64_t k = token_counts[b];
    PLAN_CHECK(k >= 0, "plan: token count %d of clip %d is negative", (int)k, b);
    PLAN_CHECK(k + p > 0, "plan: empty sequence (clip %d)", b);
    rows += k + p;
    PLAN_CHECK(p <= INT32_MAX && rows <= INT32_MAX / 2, "plan: %lld packed rows do not fit the int32 tables", (long long)rows);
    r.patches[b] = (int32_t)p;
    r.cu[b + 1] = (int32_t)rows;
    sum_k += k; sum_p += p;
    max_p = std::max(max_p, p);
    max_s = std::max(max_s, k + p);
    max_id = std::max(max_id, k + gmax);
  }
  // the smallest power of two that is >= 512 and > max(K_b + max(grid_b)); the identity row's index (= n_ids) is a uint16 slot of rope_ids
  int64_t n_ids = 512;
  while (n_ids < max_id + 1) n_ids *= 2;
  PLAN_CHECK(n_ids <= 65535, "plan: %lld rotary position ids do not fit the uint16 slots of rope_ids", (long long)n_ids);
  int64_t n_blocks = 0;
  for (int b = 0; b < n_clips; ++b) n_blocks += (r.cu[b + 1] - r.cu[b] + 63) / 64;

  ttv_plan_sizes& s = r.sz;
  memset(&s, 0, sizeof(s));
  s.n_clips = n_clips;
  s.total_rows = (int32_t)rows;
  s.sum_tokens = (int32_t)sum_k;
  s.sum_patches = (int32_t)sum_p;
  s.max_patches_per_clip = (int32_t)max_p;
  s.max_seqlen = (int32_t)max_s;
  s.n_rope_ids = (int32_t)n_ids;
  s.n_blocks64 = (int32_t)n_blocks;
  int64_t o = 0;
  s.off_cu_seqlens = o;  o += pad4((int64_t)n_clips + 1);
  s.off_clip_desc = o;   o += pad4((int64_t)8 * n_clips);
  s.off_blocks64 = o;    o += pad4(2 * n_blocks);
  s.host_words = o;
  s.off_latent_rows = o; o += pad4(sum_k);
  s.off_patch_rows = o;  o += pad4(sum_p);
  s.off_row_seq = o;     o += pad4(rows);
  s.off_rope_ids = o;    o += pad4(2 * rows);
  s.dev_words = o;
  return TTV_OK;
}

// Greedy deal of weighted units over the 8 XCD lists (plan.py: `sorted(..., reverse=True)` is stable, `min(range(8), key=...)` takes the
// first list of minimum weight).  Returns the units of every list in the order they were dealt.
void deal(const std::vector<int64_t>& weight, std::vector<int> (&lists)[XCDS]) {
  std::vector<int> order(weight.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return weight[a] > weight[b]; });
  int64_t load[XCDS] = {0};
  for (int i : order) {
    int x = 0;
    for (int j = 1; j < XCDS; ++j)
      if (load[j] < load[x]) x = j;
    lists[x].push_back(i);
    load[x] += weight[i];
  }
}

// ---- attention work tables ----------------------------------------------------------------------------------------------------------------
// One (sequence, kv-head) unit of one table: full items of the query blocks [f0, f1) first; behind all first parts of its XCD list the
// blocks [s0, s1), as half items (two per block, the second only where its 64 rows begin inside the sequence) or as full items.
struct Unit {
  int b, kvh, len;
  int f0, f1, s0, s1;
  bool second_half;
};

struct Table {
  std::vector<Unit> units;
  std::vector<int> lists[XCDS];
  int64_t len[XCDS];
  int rep;
  int64_t n_entries;      // entries of the flat table after dropping the trailing padding entries
  int64_t n_half;

  int64_t count_first(const Unit& u) const { return (int64_t)(u.f1 - u.f0) * rep; }
  int64_t count_second(const Unit& u) const {
    if (!u.second_half) return (int64_t)(u.s1 - u.s0) * rep;
    int64_t n = 0;
    for (int qb = u.s0; qb < u.s1; ++qb) n += (qb * QBLOCK + 64 < u.len) ? 2 : 1;
    return n * rep;
  }
  void finish(int rep_) {
    rep = rep_;
    std::vector<int64_t> w(units.size());
    n_half = 0;
    for (size_t i = 0; i < units.size(); ++i) {
      const int64_t c2 = count_second(units[i]);
      w[i] = 2 * count_first(units[i]) + (units[i].second_half ? c2 : 2 * c2);       // 2 * full + half: the order of full + half / 2
      if (units[i].second_half) n_half += c2;
    }
    deal(w, lists);
    n_entries = 0;
    for (int x = 0; x < XCDS; ++x) {
      len[x] = 0;
      for (int i : lists[x]) len[x] += count_first(units[i]) + count_second(units[i]);
      if (len[x] > 0) n_entries = std::max(n_entries, (len[x] - 1) * XCDS + x + 1);
    }
  }
  // flat [n_entries, 4] = (sequence, first query row, q-head, mode); entry i belongs to list i % 8, shorter lists are padded with -1
  void write(int32_t* out) const {
    for (int64_t i = 0; i < 4 * n_entries; ++i) out[i] = -1;
    for (int x = 0; x < XCDS; ++x) {
      int64_t k = 0;
      auto put = [&](int b, int q0, int head, int mode) {
        int32_t* e = out + 4 * (k * XCDS + x);
        e[0] = b; e[1] = q0; e[2] = head; e[3] = mode;
        ++k;
      };
      for (int i : lists[x]) {
        const Unit& u = units[i];
        for (int qb = u.f0; qb < u.f1; ++qb)
          for (int r = 0; r < rep; ++r) put(u.b, qb * QBLOCK, u.kvh * rep + r, 0);
      }
      for (int i : lists[x]) {
        const Unit& u = units[i];
        for (int qb = u.s0; qb < u.s1; ++qb)
          for (int r = 0; r < rep; ++r) {
            if (!u.second_half) { put(u.b, qb * QBLOCK, u.kvh * rep + r, 0); continue; }
            put(u.b, qb * QBLOCK, u.kvh * rep + r, 1);
            if (qb * QBLOCK + 64 < u.len) put(u.b, qb * QBLOCK + 64, u.kvh * rep + r, 1);
          }
      }
    }
  }
};

struct Attn {
  Table full, latent, patch, l0;
  bool has_latent, has_patch;
  ttv_plan_attn sz;
};

int attn_build(const int32_t* cu, const int32_t* token_counts, int n_clips, int q_heads, int kv_heads, int split, int tail_div, Attn& a) {
  PLAN_CHECK(cu && token_counts, "plan_attn: null argument");
  PLAN_CHECK(n_clips >= 1, "plan_attn: no clips (n_clips = %d)", n_clips);
  PLAN_CHECK(q_heads >= 1 && kv_heads >= 1 && q_heads % kv_heads == 0, "plan_attn: %d query heads over %d key/value heads", q_heads, kv_heads);
  PLAN_CHECK(split >= -1 && split <= 1, "plan_attn: split = %d (-1: the rule, 0: never, 1: every item)", split);
  int64_t blocks = 0, sum_k = 0;
  for (int b = 0; b < n_clips; ++b) {
    const int64_t s = (int64_t)cu[b + 1] - cu[b];
    PLAN_CHECK(s > 0, "plan_attn: empty sequence (clip %d)", b);
    PLAN_CHECK(token_counts[b] >= 0 && token_counts[b] <= s, "plan_attn: token count %d of clip %d outside its %lld rows", token_counts[b], b, (long long)s);
    blocks += (s + QBLOCK - 1) / QBLOCK;
    sum_k += token_counts[b];
  }
  PLAN_CHECK(blocks * q_heads <= INT32_MAX / 16, "plan_attn: %lld work items do not fit the int32 tables", (long long)(blocks * q_heads));
  const int rep = q_heads / kv_heads;
  const bool small_grid = blocks * q_heads < ATTN_SLOTS;
  const int div = small_grid ? 3 : tail_div;
  int64_t dropped = 0;
  bool patch_any = false;
  for (int b = 0; b < n_clips; ++b) {
    const int s = cu[b + 1] - cu[b], k = token_counts[b];
    const int nq = (s + QBLOCK - 1) / QBLOCK;
    const int first_half = split == 1 ? 0 : ((split == 0 || div <= 0) ? nq : nq - nq / div);
    const int lat_blocks = (k + QBLOCK - 1) / QBLOCK;      // query blocks that hold latent rows
    const int lat_only = k / QBLOCK;                       // query blocks that hold latent rows only
    dropped += lat_only;
    patch_any = patch_any || lat_only < nq;
    for (int kvh = 0; kvh < kv_heads; ++kvh) {
      a.full.units.push_back({b, kvh, s, 0, first_half, first_half, nq, true});
      a.latent.units.push_back({b, kvh, s, 0, lat_blocks, 0, 0, false});
      a.patch.units.push_back({b, kvh, s, lat_only, nq, 0, 0, false});
      a.l0.units.push_back({b, kvh, s, 0, lat_only, lat_only, nq, false});
    }
  }
  a.full.finish(rep);
  a.l0.finish(rep);
  a.has_latent = sum_k > 0;
  if (a.has_latent) a.latent.finish(rep);
  // beside a table of full items only, and only when a block was dropped and one remains (plan.py attention_table_patch / batch_for)
  a.has_patch = a.full.n_half == 0 && dropped > 0 && patch_any;
  if (a.has_patch) a.patch.finish(rep);

  ttv_plan_attn& z = a.sz;
  memset(&z, 0, sizeof(z));
  z.n_qblocks = (int32_t)a.full.n_entries;
  z.qblocks_all_full = a.full.n_half == 0 ? 1 : 0;
  z.n_qblocks_latent = a.has_latent ? (int32_t)a.latent.n_entries : 0;
  z.n_qblocks_patch = a.has_patch ? (int32_t)a.patch.n_entries : 0;
  z.n_qblocks_l0 = (int32_t)a.l0.n_entries;
  bool uniform = true;
  for (int b = 1; b < n_clips; ++b) uniform = uniform && token_counts[b] == token_counts[0] && cu[b + 1] - cu[b] == cu[1] - cu[0];
  z.tokens_per_clip = uniform ? token_counts[0] : 0;
  int64_t o = 0;
  z.off_qblocks = o;        o += 4 * (int64_t)z.n_qblocks;
  z.off_qblocks_latent = o; o += 4 * (int64_t)z.n_qblocks_latent;
  z.off_qblocks_patch = o;  o += 4 * (int64_t)z.n_qblocks_patch;
  z.off_qblocks_l0 = o;     o += 4 * (int64_t)z.n_qblocks_l0;
  z.words = o;
  return TTV_OK;
}

}  // namespace

extern "C" {

int ttv_plan_rows_sizes(const int32_t* pixel_dims, const int32_t* token_counts, int n_clips, const int32_t* patch, ttv_plan_sizes* sizes) {
  PLAN_CHECK(sizes, "plan_rows_sizes: null argument");
  Rows r;
  const int rc = rows_geometry(pixel_dims, token_counts, n_clips, patch, r);
  if (rc != TTV_OK) return rc;
  *sizes = r.sz;
  return TTV_OK;
}

int ttv_plan_rows_fill(const int32_t* pixel_dims, const int32_t* token_counts, int n_clips, const int32_t* patch, int bwd_xcd,
                       int32_t* host_segment, int64_t host_words) {
  PLAN_CHECK(host_segment, "plan_rows_fill: null argument");
  Rows r;
  const int rc = rows_geometry(pixel_dims, token_counts, n_clips, patch, r);
  if (rc != TTV_OK) return rc;
  const ttv_plan_sizes& s = r.sz;
  PLAN_CHECK(host_words >= s.host_words, "plan_rows_fill: host segment too small (%lld < %lld words)", (long long)host_words, (long long)s.host_words);
  memset(host_segment, 0, (size_t)s.host_words * 4);
  int32_t* cu = host_segment + s.off_cu_seqlens;
  for (int b = 0; b <= n_clips; ++b) cu[b] = r.cu[b];
  int32_t* desc = host_segment + s.off_clip_desc;      // (T, H, W, grid t, h, w, first patch of the clip, 3)
  int32_t pbase = 0;
  for (int b = 0; b < n_clips; ++b) {
    int32_t* d = desc + 8 * b;
    for (int a = 0; a < 3; ++a) { d[a] = pixel_dims[3 * b + a]; d[3 + a] = r.grid[3 * b + a]; }
    d[6] = pbase; d[7] = 3;
    pbase += r.patches[b];
  }
  // the attention backward's 64-row blocks (plan.py _xcd_interleave): whole sequences dealt over 8 lists by block count, entry i from
  // list i % 8 while every list has one, the rest in list order (no padding entries); bwd_xcd = 0: sequence-major
  int32_t* blk = host_segment + s.off_blocks64;
  int64_t n = 0;
  auto put = [&](int b, int k) { blk[2 * n] = b; blk[2 * n + 1] = 64 * k; ++n; };
  std::vector<int64_t> nb(n_clips);
  for (int b = 0; b < n_clips; ++b) nb[b] = (r.cu[b + 1] - r.cu[b] + 63) / 64;
  if (!bwd_xcd) {
    for (int b = 0; b < n_clips; ++b)
      for (int k = 0; k < nb[b]; ++k) put(b, k);
    return TTV_OK;
  }
  std::vector<int> lists[XCDS];
  deal(nb, lists);
  std::vector<std::pair<int, int>> flat[XCDS];
  size_t depth = SIZE_MAX;
  for (int x = 0; x < XCDS; ++x) {
    for (int b : lists[x])
      for (int k = 0; k < nb[b]; ++k) flat[x].push_back({b, k});
    depth = std::min(depth, flat[x].size());
  }
  for (size_t k = 0; k < depth; ++k)
    for (int x = 0; x < XCDS; ++x) put(flat[x][k].first, flat[x][k].second);
  for (int x = 0; x < XCDS; ++x)
    for (size_t k = depth; k < flat[x].size(); ++k) put(flat[x][k].first, flat[x][k].second);
  return TTV_OK;
}

int ttv_plan_attn_sizes(const int32_t* cu_seqlens, const int32_t* token_counts, int n_clips, int q_heads, int kv_heads, int split, int tail_div,
                        ttv_plan_attn* sizes) {
  PLAN_CHECK(sizes, "plan_attn_sizes: null argument");
  Attn a;
  const int rc = attn_build(cu_seqlens, token_counts, n_clips, q_heads, kv_heads, split, tail_div, a);
  if (rc != TTV_OK) return rc;
  *sizes = a.sz;
  return TTV_OK;
}

int ttv_plan_attn_fill(const int32_t* cu_seqlens, const int32_t* token_counts, int n_clips, int q_heads, int kv_heads, int split, int tail_div,
                       int32_t* host_tables, int64_t host_words) {
  PLAN_CHECK(host_tables, "plan_attn_fill: null argument");
  Attn a;
  const int rc = attn_build(cu_seqlens, token_counts, n_clips, q_heads, kv_heads, split, tail_div, a);
  if (rc != TTV_OK) return rc;
  PLAN_CHECK(host_words >= a.sz.words, "plan_attn_fill: host buffer too small (%lld < %lld words)", (long long)host_words, (long long)a.sz.words);
  a.full.write(host_tables + a.sz.off_qblocks);
  if (a.has_latent) a.latent.write(host_tables + a.sz.off_qblocks_latent);
  if (a.has_patch) a.patch.write(host_tables + a.sz.off_qblocks_patch);
  a.l0.write(host_tables + a.sz.off_qblocks_l0);
  return TTV_OK;
}

int ttv_rope_base_table(int head_dim, int nd, int n_ids, double theta, float* base_cos, float* base_sin) {
  PLAN_CHECK(base_cos && base_sin, "rope_base_table: null argument");
  PLAN_CHECK(nd >= 1 && head_dim >= 2 * nd && n_ids >= 1 && theta > 0.0, "rope_base_table: head_dim %d, %d axes, %d ids, theta %g", head_dim, nd,
             n_ids, theta);
  const int F = head_dim / (2 * nd);
  // rope.py:40-54 in float64: theta ** linspace(0, 1, F) * pi / 2.  torch's linspace is step * i below the middle and 1 - step * (F - 1 - i)
  // above it (not i / (F - 1)); the position id passes through fp32 before the fp64 product; the result is cast to fp32.
  std::vector<double> inv(F);
  const double step = F > 1 ? 1.0 / (double)(F - 1) : 0.0;
  for (int f = 0; f < F; ++f) {
    const double lin = f < F / 2 ? step * (double)f : 1.0 - step * (double)(F - 1 - f);
    inv[f] = pow(theta, F > 1 ? lin : 0.0) * M_PI / 2.0;
  }
  for (int i = 0; i < n_ids; ++i) {
    const double id = (double)(float)i;
    for (int f = 0; f < F; ++f) {
      const double ang = id * inv[f];
      base_cos[(size_t)i * F + f] = (float)cos(ang);
      base_sin[(size_t)i * F + f] = (float)sin(ang);
    }
  }
  return TTV_OK;
}

}  // extern "C"
