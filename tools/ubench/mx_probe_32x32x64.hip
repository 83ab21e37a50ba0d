// Probe of v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 A and B): the A / B lane -> k map, the D lane map and the scale-operand semantics.
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/mx_probe_32x32x64.hip -o tools/ubench/mx_probe_32x32x64 && tools/ubench/mx_probe_32x32x64
// Exact-integer, asymmetric data: a lane holds 32 operand bytes; lane = 32 h + row (A) or 32 h + col (B).  Every product below is a
// small power of two or an e4m3-exact value, so every D element is exact and identifies its operands.
// Result (MI355X): profiles/pv8_mx_probe.txt; consumed by csrc/ttv_attn_pv8.hip.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
typedef int v8i32 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int OPSEL>
__global__ void probe(const int* sa, const int* sb, const unsigned char* adata, const unsigned char* bdata, float* out) {
  const int lane = threadIdx.x;
  v8i32 a, b;
  const int* ap = reinterpret_cast<const int*>(adata + lane * 32);
  const int* bp = reinterpret_cast<const int*>(bdata + lane * 32);
  for (int i = 0; i < 8; ++i) { a[i] = ap[i]; b[i] = bp[i]; }
  f32x16 c;
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
  c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, OPSEL, sa[lane], OPSEL, sb[lane]);
  for (int e = 0; e < 16; ++e) out[lane * 16 + e] = c[e];     // raw: [lane][register]
}

static int *sa, *sb;
static unsigned char *ad, *bd;
static float* out;

static void run(int opsel) {
  switch (opsel) {
    case 0: probe<0><<<1, 64>>>(sa, sb, ad, bd, out); break;
    case 1: probe<1><<<1, 64>>>(sa, sb, ad, bd, out); break;
    case 2: probe<2><<<1, 64>>>(sa, sb, ad, bd, out); break;
    default: probe<3><<<1, 64>>>(sa, sb, ad, bd, out); break;
  }
  if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(1); }
}
static void unit_scales() { for (int l = 0; l < 64; ++l) { sa[l] = 0x7F7F7F7F; sb[l] = 0x7F7F7F7F; } }
// e4m3 byte 0x20 + i, i = 0 .. 63: 64 distinct positive normal values (1 + (i & 7) / 8) * 2^((i >> 3) + 4 - 7)
static float tag_value(int i) { return (1.f + (i & 7) / 8.f) * ldexpf(1.f, (i >> 3) - 3); }
static int tag_of(float v) { for (int i = 0; i < 64; ++i) if (tag_value(i) == v) return i; return -1; }

int main() {
  hipHostMalloc(&sa, 256); hipHostMalloc(&sb, 256); hipHostMalloc(&ad, 2048); hipHostMalloc(&bd, 2048); hipHostMalloc(&out, 4096);

  // 1. D lane map: A row i = 1.0 in every k, B col j = tag(i-independent) ... done per (i, j) pair with one-hot rows / cols:
  //    A nonzero only in row 3 (value 1.0, all k), B nonzero only in col 7 (1.0, all k): the one D element that is 64 is D[3][7].
  printf("== D map: only D[i][j] is non-zero; it sits in (lane, register)\n");
  const int pi[6] = {3, 0, 31, 12, 21, 9}, pj[6] = {7, 31, 0, 5, 18, 30};
  for (int t = 0; t < 6; ++t) {
    unit_scales();
    memset(ad, 0, 2048); memset(bd, 0, 2048);
    for (int h = 0; h < 2; ++h) for (int b = 0; b < 32; ++b) { ad[(32 * h + pi[t]) * 32 + b] = 0x38; bd[(32 * h + pj[t]) * 32 + b] = 0x38; }
    run(0);
    printf("D[%2d][%2d]:", pi[t], pj[t]);
    for (int l = 0; l < 64; ++l) for (int e = 0; e < 16; ++e) if (out[l * 16 + e] != 0.f) printf(" lane %d reg %d = %g", l, e, out[l * 16 + e]);
    printf("\n");
  }

  // 2. k pairing: A row 3 one-hot (h, b) = 1.0; B col 7 holds a distinct tag in each of its 64 (h', b').  D[3][7] = the partner's tag.
  //    The position of D[3][7] is taken from step 1's first line (searched again here: the only non-zero element).
  printf("== k pairing: A(h, byte) <-> B(h', byte')\n");
  int mism = 0;
  for (int h = 0; h < 2; ++h) for (int b = 0; b < 32; ++b) {
    unit_scales();
    memset(ad, 0, 2048); memset(bd, 0, 2048);
    ad[(32 * h + 3) * 32 + b] = 0x38;
    for (int h2 = 0; h2 < 2; ++h2) for (int b2 = 0; b2 < 32; ++b2) bd[(32 * h2 + 7) * 32 + b2] = 0x20 + 32 * h2 + b2;
    run(0);
    float v = 0.f; int nz = 0;
    for (int i = 0; i < 1024; ++i) if (out[i] != 0.f) { v = out[i]; ++nz; }
    const int tg = tag_of(v);
    printf("A(%d,%2d) <-> B(%d,%2d)%s\n", h, b, tg >> 5, tg & 31, nz == 1 ? "" : "  (!! not exactly one non-zero)");
    if (tg != 32 * h + b) ++mism;
  }
  printf("k pairing identical (h, byte) on both sides: %s\n", mism ? "NO" : "yes");

  // 3. scale ownership: A = 1.0 one-hot at (row 3, h, b), B = 1.0 everywhere; the A scale of lane 32 hs + 3 is 2^1, all others 2^0.
  //    D[3][*] == 2 names the owner.  Then the same for B (col 7).  Scales of another row's lanes must not matter (lane 32 hs + 4).
  for (int which = 0; which < 2; ++which) {
    printf("== scale ownership, %s: element (h, byte) is multiplied by the scale byte of lane half ...\n", which ? "B" : "A");
    for (int h = 0; h < 2; ++h) for (int b = 0; b < 32; ++b) {
      printf("%s(%d,%2d):", which ? "B" : "A", h, b);
      for (int hs = 0; hs < 2; ++hs) for (int other = 0; other < 2; ++other) {
        unit_scales();
        memset(ad, which ? 0x38 : 0, 2048); memset(bd, which ? 0 : 0x38, 2048);
        (which ? bd : ad)[(32 * h + (which ? 7 : 3)) * 32 + b] = 0x38;
        (which ? sb : sa)[32 * hs + (which ? 7 : 3) + other] = 0x7F7F7F80;
        run(0);
        // D[3][0] (A) or D[0][7] (B): found as the value of the non-zero elements of row 3 / col 7 (all equal)
        float v = 0.f;
        for (int i = 0; i < 1024; ++i) if (out[i] != 0.f) { v = out[i]; break; }
        if (v == 2.f) printf(other ? " (!! neighbour lane of half %d)" : " half %d", hs);
      }
      printf("\n");
    }
  }

  // 4. op_sel: the A scale 2^1 of lane 3 / 35 sits in byte p of the register; which op_sel sees it
  printf("== op_sel: A scale 2^1 in byte p of lanes 3 and 35, A = B = 1.0: D[3][0] / 64 under op_sel 0..3\n");
  for (int p = 0; p < 4; ++p) {
    memset(ad, 0, 2048); memset(bd, 0x38, 2048);
    for (int h = 0; h < 2; ++h) for (int b = 0; b < 32; ++b) ad[(32 * h + 3) * 32 + b] = 0x38;
    printf("byte %d:", p);
    for (int o = 0; o < 4; ++o) {
      unit_scales();
      sa[3] = sa[35] = 0x7F7F7F7F + (1 << (8 * p));
      run(o);
      float v = 0.f;
      for (int i = 0; i < 1024; ++i) if (out[i] != 0.f) { v = out[i]; break; }
      printf(" opsel%d %g", o, v / 64.f);
    }
    printf("\n");
  }

  // 5. scale magnitude: byte E multiplies by 2^(E - 127) exactly, here E = 120 .. 134 on A's block of half 0, one-hot element 1.0
  printf("== scale value: A scale byte E of lanes 3 / 35, one-hot A(0, 0) = 1.0: D[3][0]\n");
  for (int E = 120; E <= 134; E += 7) {
    unit_scales();
    memset(ad, 0, 2048); memset(bd, 0x38, 2048);
    ad[3 * 32] = 0x38;
    sa[3] = sa[35] = 0x7F7F7F00 + E;
    run(0);
    float v = 0.f;
    for (int i = 0; i < 1024; ++i) if (out[i] != 0.f) { v = out[i]; break; }
    printf("E %d: %g (2^%d)\n", E, v, (int)lrintf(log2f(v)));
  }
  return 0;
}
