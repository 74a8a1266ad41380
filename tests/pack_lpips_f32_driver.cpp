// Stand-alone driver of the fp32 tile layouts of the LPIPS exact-fp32 convolution
// (pack_conv2d_f32 and its stem variant, csrc/pack.cpp) for tests/test_pack_lpips_f32_cpu.py:
// seeded weights from the LCG of tests/pack_driver.cpp, the five AlexNet shapes of the test's table
// and one small odd shape, the raw output buffers written to the directory given as argv[1]. Links
// pack.cpp only; built with -fsanitize=address,undefined by the test.
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
// row 0 all zero
static std::vector<float> weights(int M, int rowlen, uint32_t seed) {
  std::vector<float> w((size_t)M * rowlen);
  uint32_t x = seed;
  for (float& v : w) {
    x = x * 1664525u + 1013904223u;
    v = (float)((int)(x >> 8) - 8388608) / 33554432.0f;
  }
  for (int i = 0; i < rowlen; ++i) w[i] = 0.f;
  return w;
}

static void put(const std::string& name, const TilesF32& p) {
  dump(name + ".a", p.a);
  dump(name + ".dims", std::vector<float>{(float)p.nkt});
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: pack_lpips_f32_driver OUTDIR\n"); return 2; }
  g_dir = argv[1];
  // name, M, Cin, KS, bm: AlexNet's convs 2 - 5 at the 64-row m-tile the runtime gives them
  // (kLpipsF32Bm), and a small one whose Cout is no multiple of the tile and whose Cin is no
  // multiple of the channel pad
  struct Case { const char* name; int M, Cin, KS, bm; };
  const Case cs[] = {{"conv2", 192, 64, 5, 64}, {"conv3", 384, 192, 3, 64}, {"conv4", 256, 384, 3, 64},
                     {"conv5", 256, 256, 3, 64}, {"odd", 40, 5, 3, 64}};
  uint32_t seed = 81;
  for (const Case& c : cs)
    put(c.name, pack_conv2d_f32(weights(c.M, c.Cin * c.KS * c.KS, seed++), c.M, c.Cin, (c.Cin + 7) / 8 * 8, c.KS, c.bm));
  // the stem: 33 of 40 per ky row, K = 440, no multiple of the 32-wide k-tile; and 40 rows of a
  // 64-row tile
  put("stem", pack_conv2d_f32_stem(weights(64, 3 * 121, seed++), 64, 3, 11, 64, 40));
  put("stem40", pack_conv2d_f32_stem(weights(40, 3 * 121, seed++), 40, 3, 11, 64, 40));
  return 0;
}
