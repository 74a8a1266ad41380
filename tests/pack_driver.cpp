// Stand-alone driver of csrc/pack.cpp for tests/test_pack_cpu.py: seeded weights from a fixed
// LCG (restated in the test), every packer once per shape of the test's table, the raw output
// buffers written to the directory given as argv[1]. Links pack.cpp only; built with
// -fsanitize=address,undefined by the test.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
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
static void special(std::vector<float>& w, int outer, int M, int inner) {
  for (int o = 0; o < outer; ++o)
    for (int i = 0; i < inner; ++i) w[((size_t)o * M + 0) * inner + i] = 0.f;
  w[(size_t)1 * inner + 0] = 0.5f;
  w[(size_t)2 * inner + 1] = 1.2345e-6f;
}
static std::vector<float> weights(int M, int rowlen, uint32_t seed) {
  std::vector<float> w = gen((size_t)M * rowlen, seed);
  special(w, 1, M, rowlen);
  return w;
}
static std::vector<float> ints(std::initializer_list<int> l) { return std::vector<float>(l.begin(), l.end()); }

static void gemm_case(const std::string& name, int M, int ci, int kk, int bm, uint32_t seed) {
  const std::vector<float> w = weights(M, ci * kk, seed);
  const GemmPlane p = pack_gemm_plane(w, M, ci * kk, bm);
  const Frags g = pack_gemm_x3(p, 1, M, ci * kk, bm, kk);
  dump(name + ".plane", p.a);
  dump(name + ".g", g.g);
  dump(name + ".rs", g.rs);
  dump(name + ".gt", g.tap_major);
  dump(name + ".dims", ints({p.Mpad, p.Kpad, g.n}));
}

static void attn_case(const std::string& name, int C, int hid, int uh, int dim_head, uint32_t seed) {
  std::vector<float> wq = weights(3 * hid, C, seed), wp = weights(C, hid, seed + 1);
  const std::vector<float> ng = gen(C, seed + 2), nb = gen(C, seed + 3);
  const float q_scale = 1.0f / std::sqrt((float)dim_head);
  const AttnX3Pack a = pack_attn_x3(wq, wp, ng, &nb, C, hid, uh, q_scale);
  dump(name + ".a", a.a);
  dump(name + ".sc", std::vector<float>(a.sc, a.sc + 5));
  dump(name + ".s2", std::vector<float>(1, a.s2));
  const AttnX3Pack a0 = pack_attn_x3(wq, wp, ng, nullptr, C, hid, uh, q_scale);
  dump(name + ".sc_nobias", std::vector<float>(a0.sc, a0.sc + 5));
  dump(name + ".qkv", pack_stw_rows(wq, 3, hid, C));
  dump(name + ".proj", pack_stw_rows(wp, 1, C, hid));
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: pack_driver OUTDIR\n"); return 2; }
  g_dir = argv[1];

  gemm_case("gemm3x3", 40, 8, 9, 64, 1);  // K = 72 = 2 * 32 + 8, tap-major copy present
  gemm_case("gemm_ci6", 40, 6, 9, 64, 2);  // ci % 8 != 0: no tap-major copy
  gemm_case("gemm1x1", 40, 8, 1, 64, 3);   // 1x1: no tap-major copy
  {  // deconv: W[ci = 3][co = 40][4][4], four parity planes with K = 12
    std::vector<float> w = gen((size_t)3 * 40 * 16, 4);
    special(w, 3, 40, 16);
    const GemmPlane p = pack_deconv_planes(w, 3, 40, 64);
    const Frags g = pack_gemm_x3(p, 4, 40, 12, 64, 4);
    dump("deconv.plane", p.a);
    dump("deconv.g", g.g);
    dump("deconv.rs", g.rs);
    dump("deconv.gt", g.tap_major);
  }
  {  // I3D unit: M = 40, Cin = 12, KS = 3 (Cpad = 16); stem: M = 64, Cin = 3, KS = 7, rows of 24
    const Frags u = pack_unit3d(weights(40, 12 * 27, 5), 40, 12, 16, 3, 64, 0);
    dump("unit3d.g", u.g);
    dump("unit3d.rs", u.rs);
    const Frags st = pack_unit3d(weights(64, 3 * 343, 6), 64, 3, 8, 7, 64, 24);
    dump("stem.g", st.g);
    dump("stem.rs", st.rs);
    dump("stem.dims", ints({u.n, st.n}));
  }
  {
    const Frags a = pack_x3(weights(40, 24 * 9, 7), 3, 40, 24, 64, 1);
    dump("x3_k3.a", a.g);
    dump("x3_k3.rs", a.rs);
    const Frags b = pack_x3(weights(40, 40, 8), 1, 40, 40, 64, 2);
    dump("x3_k1.a", b.g);
    dump("x3_k1.rs", b.rs);
    dump("x3.dims", ints({a.n, b.n}));
  }
  {
    const HaloPack h = pack_halo(weights(40, 10 * 9, 9), 3, 40, 10, 64, 4);
    dump("halo.a", h.a);
    dump("halo.dims", ints({h.stages}));
  }
  dump("narrow3.a", pack_narrow(weights(3, 5 * 49, 10), 49, 3, 5, 3));
  dump("narrow21.a", pack_narrow(weights(21, 5 * 49, 11), 49, 21, 5, 8));
  dump("time3", reorder_time3(gen((size_t)5 * 3 * 3 * 9, 12), 5, 3, 3, 9));
  {
    const std::vector<float> w = gen((size_t)6 * 8 * 49, 13);
    dump("split.x", split_channels(w, 6, 8, 49, 0, 3));
    dump("split.f", split_channels(w, 6, 8, 49, 3, 8));
  }
  {
    const Frags c = pack_conv7c3(weights(40, 147, 14), 40);
    dump("conv7.g", c.g);
    dump("conv7.rs", c.rs);
  }
  {  // x-branch classes: Cm = 8, Co = 40, Cin = 13, L = 16
    const XPathPack x = pack_xpath(weights(8, 147, 15), gen(8, 16), weights(40, 13 * 49, 17), gen(40, 18), 8, 40, 13, 16);
    dump("xpath.g", x.g);
    dump("xpath.rs", x.rs);
    dump("xpath.cb", x.cb);
  }
  {  // phase weights: Co = 8, Cf = 16, n = 16
    const FeaPhasePack f = pack_fea_phase(weights(8, 16 * 49, 19), 8, 16, 16);
    dump("fea.k5", f.k5);
    dump("fea.side", f.side);
    dump("fea.side_scale", f.side_scale);
    dump("fea.corner", f.corner);
  }
  attn_case("attn32", 64, 64, 16384, 32, 20);  // two units of one head each
  attn_case("attn16", 64, 64, 16384, 16, 30);  // two heads per unit
  {  // both BatchNorm folds: 7 channels, running_var = 0 in channel 3
    const std::vector<float> w = gen(7, 40), b = gen(7, 41), rm = gen(7, 42);
    std::vector<float> rv = gen(7, 43);
    for (float& v : rv) v = v < 0 ? -v : v;
    rv[3] = 0.f;
    const Affine f32 = bn_fold_f32(w, b, rm, rv), f64 = bn_fold_f64(w, b, rm, rv);
    dump("bn32.a", f32.a);
    dump("bn32.b", f32.b);
    dump("bn64.a", f64.a);
    dump("bn64.b", f64.b);
  }
  return 0;
}
