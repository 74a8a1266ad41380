// Stand-alone driver of pack_conv2d (csrc/pack.cpp) for tests/test_lpips_cpu.py: seeded weights
// from the LCG of tests/pack_driver.cpp, the three shapes of the test's table, the raw output
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

// n values in (-0.25, 0.25): x <- 1664525 x + 1013904223 (mod 2^32), v = ((x >> 8) - 2^23) / 2^25;
// row 0 all zero, row 1 with largest magnitude exactly 2^-1, row 2 with one value whose scaled lo
// half is subnormal in fp16 (the special rows of tests/pack_driver.cpp)
static std::vector<float> weights(int M, int rowlen, uint32_t seed) {
  std::vector<float> w((size_t)M * rowlen);
  uint32_t x = seed;
  for (float& v : w) {
    x = x * 1664525u + 1013904223u;
    v = (float)((int)(x >> 8) - 8388608) / 33554432.0f;
  }
  for (int i = 0; i < rowlen; ++i) w[i] = 0.f;
  w[(size_t)1 * rowlen] = 0.5f;
  w[(size_t)2 * rowlen + 1] = 1.2345e-6f;
  return w;
}

static void conv_case(const std::string& name, int M, int Cin, int KS, int bm, int stem_row, uint32_t seed) {
  const int Cpad = (Cin + 7) / 8 * 8;
  const Frags p = pack_conv2d(weights(M, Cin * KS * KS, seed), M, Cin, Cpad, KS, bm, stem_row);
  dump(name + ".g", p.g);
  dump(name + ".rs", p.rs);
  dump(name + ".dims", std::vector<float>{(float)p.n});
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: pack_lpips_driver OUTDIR\n"); return 2; }
  g_dir = argv[1];
  conv_case("stem", 64, 3, 11, 64, 40, 51);  // K = 440: not a multiple of the 32-wide k-tile
  conv_case("c5", 192, 8, 5, 128, 0, 52);    // Cout 192 at BM 128: a partial second m-tile
  conv_case("c3", 40, 16, 3, 64, 0, 53);
  return 0;
}
