// Stand-alone driver of the two-tap packers of csrc/pack.cpp (pack_x3_deconv, pack_x3_down) for
// tests/test_pack_updown_cpu.py: seeded weights from the LCG of tests/pack_driver.cpp (restated in
// the test) with its three special rows, one pack per (Cin, Cout, bm) of the test's table, the raw
// buffers written to the directory given as argv[1]. Links pack.cpp only; built with
// -fsanitize=address,undefined by the test.
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
// w [outer][M][inner], row m = all (o, m, i): row 0 all zero, row 1 with largest magnitude exactly
// 2^-1, row 2 with one value whose scaled lo half is subnormal in fp16
static std::vector<float> weights(int outer, int M, int inner, uint32_t seed) {
  std::vector<float> w = gen((size_t)outer * M * inner, seed);
  for (int o = 0; o < outer; ++o)
    for (int i = 0; i < inner; ++i) w[((size_t)o * M + 0) * inner + i] = 0.f;
  w[(size_t)1 * inner + 0] = 0.5f;
  w[(size_t)2 * inner + 1] = 1.2345e-6f;
  return w;
}

static void updown_case(int ci, int co, int bm, uint32_t seed) {
  const std::string tag = "_" + std::to_string(ci) + "_" + std::to_string(co) + "_" + std::to_string(bm);
  const Frags u = pack_x3_deconv(weights(ci, co, 16, seed), ci, co, bm);  // W[ci][co][4][4]
  dump("up" + tag + ".g", u.g);
  dump("up" + tag + ".rs", u.rs);
  dump("up" + tag + ".n", std::vector<float>(1, (float)u.n));
  const Frags d = pack_x3_down(weights(1, co, ci * 16, seed + 100), co, ci, bm);  // W[co][ci][4][4]
  dump("down" + tag + ".g", d.g);
  dump("down" + tag + ".rs", d.rs);
  dump("down" + tag + ".n", std::vector<float>(1, (float)d.n));
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: pack_updown_driver OUTDIR\n"); return 2; }
  g_dir = argv[1];
  uint32_t seed = 50;
  for (int ci : {16, 32})
    for (int co : {16, 80}) {
      updown_case(ci, co, 64, seed++);              // Cout 80: two m-tiles per phase, the second partial
      if (co > 64) updown_case(ci, co, 128, seed++);  // the 128-row tile x3_tile picks above 64
    }
  return 0;
}
