// Stand-alone driver of fold_ln_gamma (csrc/pack.cpp) for tests/test_pack_lnfold_cpu.py: seeded 1x1
// weights from the LCG of tests/pack_driver.cpp (restated in the test) with its three special rows,
// a seeded gamma with a zero, a negative, a power of two and a tiny entry, W' = fold_ln_gamma(W,
// gamma) and its pack_x3 buffers for the (Cout, Cin, bm) of the test's table (the 1x1 tiles: two
// channel groups), the raw buffers written to the directory given as argv[1]. Links pack.cpp only;
// built with -fsanitize=address,undefined by the test.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pack.h"

using namespace extdm;

static std::string g_dir;

template <class T>
static void dump(const std::string& name, const std::vector<T>& v) {
  FILE* f = fopen((g_dir + "/" + name + ".bin").c_str(), "wb");
  if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) { fprintf(stderr, "cannot write %s\n", name.c_str()); exit(2); }
  fclose(f);
}

// n values in (-0.25, 0.25): x <- 1664525 x + 1013904223 (mod 2^32), v = ((x >> 8) - 2^23) / 2^25
static std::vector<float> gen(size_t n, uint32_t seed) {
  std::vector<float> v(n);
  uint32_t x = seed;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    v[i] = (float)((int)(x >> 8) - 8388608) / 33554432.0f;
  }
  return v;
}
// w [M][K]: row 0 all zero, row 1 with largest magnitude exactly 2^-1, row 2 with one tiny value
static std::vector<float> weights(int M, int K, uint32_t seed) {
  std::vector<float> w = gen((size_t)M * K, seed);
  for (int i = 0; i < K; ++i) w[i] = 0.f;
  w[(size_t)1 * K + 0] = 0.5f;
  w[(size_t)2 * K + 1] = 1.2345e-6f;
  return w;
}
// gamma = 1 + 4 v (in (0, 2)), then gamma[0] = 2 (row 1's largest product stays a power of two),
// gamma[1] = 1e-3, gamma[2] = 0, gamma[3] = -1.5
static std::vector<float> gamma_of(int K, uint32_t seed) {
  std::vector<float> g = gen((size_t)K, seed);
  for (float& v : g) v = 1.f + 4.f * v;
  g[0] = 2.f; g[1] = 1e-3f; g[2] = 0.f; g[3] = -1.5f;
  return g;
}

static void fold_case(int co, int ci, int bm, uint32_t seed) {
  const std::string tag = "_" + std::to_string(co) + "_" + std::to_string(ci) + "_" + std::to_string(bm);
  const std::vector<float> f = fold_ln_gamma(weights(co, ci, seed), gamma_of(ci, seed + 100), co, ci);
  dump("fold" + tag + ".w", f);
  const Frags x = pack_x3(f, 1, co, ci, bm, 2);
  dump("fold" + tag + ".g", x.g);
  dump("fold" + tag + ".rs", x.rs);
  dump("fold" + tag + ".n", std::vector<float>(1, (float)x.n));
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: pack_lnfold_driver OUTDIR\n"); return 2; }
  g_dir = argv[1];
  fold_case(40, 32, 64, 70);    // one partial m-tile, whole channel blocks
  fold_case(40, 48, 64, 71);    // a half-filled last channel block (Cin % 32 = 16)
  fold_case(160, 64, 128, 72);  // two m-tiles, the second partial
  return 0;
}
