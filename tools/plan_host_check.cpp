// Stand-alone check of the host-side plan builder (titok_video_amd/csrc/ttv_plan_host.cpp) for a sanitizer build: no Python, no HIP,
// no GPU.  It runs the batches of tests/test_native_plan_cpu.py - the named cases, 200 seeded ragged batches, the invalid inputs - into
// buffers of exactly the size the sizes calls report (so a write past a table is a heap overflow the sanitizer sees), and checks what
// can be checked without BatchPlan: every (row, q-head) is covered exactly once by `qblocks`, every 64-row block exactly once by
// blocks64, a refused call leaves its output as it was.  Also a small example of the calls a C host makes.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/plan_host_check.cpp
//       titok_video_amd/csrc/ttv_plan_host.cpp -o plan_host_check && ./plan_host_check
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "titok_hip.h"

static char g_err[512];
void ttv_set_error(const char* fmt, ...) {      // the library keeps this in ttv_api.hip
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define REQUIRE(cond)                                                   \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_err); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

typedef std::vector<int32_t> Ints;
static const int32_t PATCH[3] = {4, 8, 8};
static long g_plans = 0;

static void check_table(const int32_t* t, int n, const Ints& cu, int q_heads, int kv_heads, bool cover_all) {
  std::map<std::tuple<int, int, int>, int> seen;      // (sequence, head, 64-row slice) -> count
  std::map<std::pair<int, int>, int> unit_list;
  REQUIRE(n > 0 && t[4 * (n - 1)] >= 0);              // the trailing padding entries are dropped
  for (int i = 0; i < n; ++i) {
    const int b = t[4 * i], q0 = t[4 * i + 1], head = t[4 * i + 2], mode = t[4 * i + 3];
    if (b < 0) continue;
    const int s = cu[b + 1] - cu[b], rows = mode ? 64 : 128;
    REQUIRE(b < (int)cu.size() - 1 && (mode == 0 || mode == 1) && q0 % rows == 0 && q0 < s && head >= 0 && head < q_heads);
    for (int r = q0; r < q0 + rows && r < s; r += 64) ++seen[std::make_tuple(b, head, r / 64)];
    auto it = unit_list.emplace(std::make_pair(b, head / (q_heads / kv_heads)), i % 8);
    REQUIRE(it.first->second == i % 8);               // one XCD list per (sequence, kv-head) unit
  }
  long want = 0;
  for (size_t b = 0; b + 1 < cu.size(); ++b) want += (long)((cu[b + 1] - cu[b] + 63) / 64) * q_heads;
  for (auto& kv : seen) REQUIRE(kv.second == 1);
  if (cover_all) REQUIRE((long)seen.size() == want);
}

static void run(const Ints& dims, const Ints& counts, int q_heads, int kv_heads, int split, int tail_div, int bwd_xcd) {
  const int n = (int)counts.size();
  ttv_plan_sizes sz;
  REQUIRE(ttv_plan_rows_sizes(dims.data(), counts.data(), n, PATCH, &sz) == TTV_OK);
  Ints seg((size_t)sz.host_words);                    // exactly host_words: an overrun is a heap-buffer-overflow
  REQUIRE(ttv_plan_rows_fill(dims.data(), counts.data(), n, PATCH, bwd_xcd, seg.data(), sz.host_words) == TTV_OK);
  Ints cu(seg.begin() + sz.off_cu_seqlens, seg.begin() + sz.off_cu_seqlens + n + 1);
  REQUIRE(cu[0] == 0 && cu[n] == sz.total_rows && sz.sum_tokens + sz.sum_patches == sz.total_rows);
  REQUIRE(sz.n_rope_ids >= 512 && (sz.n_rope_ids & (sz.n_rope_ids - 1)) == 0);
  std::map<std::pair<int, int>, int> blocks;
  for (int i = 0; i < sz.n_blocks64; ++i) {
    const int b = seg[sz.off_blocks64 + 2 * i], r0 = seg[sz.off_blocks64 + 2 * i + 1];
    REQUIRE(b >= 0 && b < n && r0 % 64 == 0 && r0 < cu[b + 1] - cu[b]);
    const int times = ++blocks[std::make_pair(b, r0)];
    REQUIRE(times == 1);
  }
  ttv_plan_attn az;
  REQUIRE(ttv_plan_attn_sizes(cu.data(), counts.data(), n, q_heads, kv_heads, split, tail_div, &az) == TTV_OK);
  Ints tab((size_t)az.words);
  REQUIRE(ttv_plan_attn_fill(cu.data(), counts.data(), n, q_heads, kv_heads, split, tail_div, tab.data(), az.words) == TTV_OK);
  check_table(tab.data() + az.off_qblocks, az.n_qblocks, cu, q_heads, kv_heads, true);
  check_table(tab.data() + az.off_qblocks_l0, az.n_qblocks_l0, cu, q_heads, kv_heads, true);
  if (az.n_qblocks_latent) check_table(tab.data() + az.off_qblocks_latent, az.n_qblocks_latent, cu, q_heads, kv_heads, false);
  if (az.n_qblocks_patch) check_table(tab.data() + az.off_qblocks_patch, az.n_qblocks_patch, cu, q_heads, kv_heads, false);
  ++g_plans;
}

static Ints repeat(const Ints& v, int times) {
  Ints out;
  for (int i = 0; i < times; ++i) out.insert(out.end(), v.begin(), v.end());
  return out;
}

template <typename Sizes, typename Call>
static void refused(Call call, const char* message) {
  Sizes sz;
  memset(&sz, 0x5A, sizeof(sz));
  Ints out(4096, 0x5A5A5A5A);
  g_err[0] = 0;
  REQUIRE(call(&sz, out.data(), (int64_t)out.size()) == 2 * TTV_ERR_INVALID);      // both calls refuse
  REQUIRE(strstr(g_err, message) != nullptr);
  const unsigned char* p = (const unsigned char*)&sz;
  for (size_t i = 0; i < sizeof(sz); ++i) REQUIRE(p[i] == 0x5A);
  for (int32_t v : out) REQUIRE(v == 0x5A5A5A5A);
}

int main() {
  const int heads[2][2] = {{4, 2}, {12, 4}};
  const Ints big = {16, 128, 128};
  const Ints ragged = {16, 128, 128, 8, 64, 96, 4, 8, 8, 12, 96, 128}, ragged_k = {128, 0, 1, 37};
  const Ints ties = repeat({8, 64, 64, 16, 128, 128, 8, 64, 64, 8, 64, 64, 16, 128, 128, 4, 64, 64, 8, 64, 64}, 2);
  for (auto& h : heads) {
    run(repeat(big, 32), Ints(32, 128), h[0], h[1], -1, 0, 1);
    run(repeat(big, 5), Ints(5, 128), h[0], h[1], -1, 0, 1);
    run(ragged, ragged_k, h[0], h[1], -1, 0, 1);
    run({4, 128, 128, 8, 64, 64}, {256, 130}, h[0], h[1], -1, 0, 1);
    run({8, 64, 64}, {600}, h[0], h[1], -1, 0, 1);
    run(repeat(big, 32), Ints(32, 128), h[0], h[1], -1, 8, 1);
    run(ragged, ragged_k, h[0], h[1], 0, 0, 1);
    run(ragged, ragged_k, h[0], h[1], 1, 0, 1);
    run(ragged, ragged_k, h[0], h[1], -1, 0, 0);
    run(ties, repeat({64, 128, 64, 64, 128, 64, 64}, 2), h[0], h[1], -1, 0, 1);
  }
  std::mt19937 rng(0);
  const int32_t shapes[6][3] = {{16, 128, 128}, {8, 64, 96}, {16, 64, 64}, {4, 128, 96}, {12, 96, 128}, {16, 96, 96}};
  const int32_t ks[3] = {32, 64, 128};
  for (int i = 0; i < 200; ++i) {
    const int n = 4 + (int)(rng() % 4);
    Ints dims, counts;
    for (int b = 0; b < n; ++b) {
      const int32_t* s = shapes[rng() % 6];
      dims.insert(dims.end(), s, s + 3);
      counts.push_back(ks[rng() % 3]);
    }
    run(dims, counts, 4, 2, -1, 0, 1);
  }

  const Ints d2 = {16, 128, 128, 8, 64, 96}, k2 = {128, 0};
  auto rows = [&](const int32_t* d, const int32_t* k, int n, const int32_t* p) {
    return [=](ttv_plan_sizes* sz, int32_t* out, int64_t words) {
      return ttv_plan_rows_sizes(d, k, n, p, sz) + ttv_plan_rows_fill(d, k, n, p, 1, out, words);
    };
  };
  const Ints odd = {16, 130, 128, 8, 64, 96}, zero = {16, 128, 128, 0, 64, 96}, neg = {128, -1}, far = {128, 40000};
  const int32_t patch0[3] = {4, 0, 8};
  refused<ttv_plan_sizes>(rows(odd.data(), k2.data(), 2, PATCH), "not a positive multiple");
  refused<ttv_plan_sizes>(rows(zero.data(), k2.data(), 2, PATCH), "not a positive multiple");
  refused<ttv_plan_sizes>(rows(d2.data(), neg.data(), 2, PATCH), "negative");
  refused<ttv_plan_sizes>(rows(d2.data(), k2.data(), 0, PATCH), "no clips");
  refused<ttv_plan_sizes>(rows(nullptr, k2.data(), 2, PATCH), "null");
  refused<ttv_plan_sizes>(rows(d2.data(), nullptr, 2, PATCH), "null");
  refused<ttv_plan_sizes>(rows(d2.data(), k2.data(), 2, nullptr), "null");
  refused<ttv_plan_sizes>(rows(d2.data(), k2.data(), 2, patch0), "patch");
  refused<ttv_plan_sizes>(rows(d2.data(), far.data(), 2, PATCH), "uint16");
  auto attn = [&](const int32_t* cu, const int32_t* k, int n, int hq, int hkv, int split) {
    return [=](ttv_plan_attn* sz, int32_t* out, int64_t words) {
      return ttv_plan_attn_sizes(cu, k, n, hq, hkv, split, 0, sz) + ttv_plan_attn_fill(cu, k, n, hq, hkv, split, 0, out, words);
    };
  };
  const Ints cu_ok = {0, 1152, 1248}, cu_empty = {0, 1152, 1152}, k_far = {128, 97};
  refused<ttv_plan_attn>(attn(cu_empty.data(), k2.data(), 2, 4, 2, -1), "empty sequence");
  refused<ttv_plan_attn>(attn(cu_ok.data(), neg.data(), 2, 4, 2, -1), "token count");
  refused<ttv_plan_attn>(attn(cu_ok.data(), k_far.data(), 2, 4, 2, -1), "token count");
  refused<ttv_plan_attn>(attn(cu_ok.data(), k2.data(), 0, 4, 2, -1), "no clips");
  refused<ttv_plan_attn>(attn(nullptr, k2.data(), 2, 4, 2, -1), "null");
  refused<ttv_plan_attn>(attn(cu_ok.data(), k2.data(), 2, 4, 3, -1), "heads");
  refused<ttv_plan_attn>(attn(cu_ok.data(), k2.data(), 2, 4, 2, 2), "split");

  for (int n_ids : {512, 1024, 4096}) {
    std::vector<float> c((size_t)n_ids * 10), s((size_t)n_ids * 10);
    REQUIRE(ttv_rope_base_table(64, 3, n_ids, 10000.0, c.data(), s.data()) == TTV_OK);
    REQUIRE(c[0] == 1.0f && s[0] == 0.0f);
    for (size_t i = 0; i < c.size(); ++i) REQUIRE(c[i] >= -1.0f && c[i] <= 1.0f && s[i] >= -1.0f && s[i] <= 1.0f);
  }
  REQUIRE(ttv_rope_base_table(64, 3, 512, 10000.0, nullptr, nullptr) == TTV_ERR_INVALID);
  printf("plan_host_check: %ld plans, every refusal as expected\n", g_plans);
  return 0;
}
