// The weight layouts of pack.h, checked on the CPU by tests/test_pack_cpu.py.
#include "pack.h"

#include <algorithm>
#include <cmath>

namespace extdm {

template <class T>
int pow2_row_exp(T mx, float& rs) {
  int e = 0;
  if (mx > T(0)) { std::frexp(mx, &e); e = 15 - e; }  // mx * 2^e in [2^14, 2^15)
  rs = std::ldexp(1.f, -e);
  return e;
}
template int pow2_row_exp<float>(float, float&);
template int pow2_row_exp<double>(double, float&);

void put_hilo(half_t* dst, float v) {
  const half_t hi = (half_t)v;
  dst[0] = hi;
  dst[512] = (_Float16)(v - (float)hi);
}

// element (row m, column col < 16) of the 32-row [hi|lo][lane][8] fragment pair at blk
static half_t* afrag(half_t* blk, int m, int col) { return blk + ((m % 32) + 32 * (col / 8)) * 8 + col % 8; }

// pow2_row_exp of the largest |p[i]|
template <class T>
static int row_exp(const T* p, size_t n, float& rs) {
  T mx = 0;
  for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(p[i]));
  return pow2_row_exp(mx, rs);
}

// 2^e bringing the largest |p[i]| to [2^14, 2^15); inv = 2^-e
static float pow2_scale(const float* p, size_t n, float& inv) { return std::ldexp(1.f, row_exp(p, n, inv)); }

// e with v * 2^e in [1, 2), clamped to +-30; 0 for v == 0 or non-finite
static int pow2_exp(double v) {
  if (!(v > 0.0) || !std::isfinite(v)) return 0;
  int e = 0;
  std::frexp(v, &e);
  return std::min(30, std::max(-30, 1 - e));
}

GemmPlane pack_gemm_plane(const fvec& w, int M, int K, int bm) {
  GemmPlane p{{}, (M + bm - 1) / bm * bm, (K + 15) / 16 * 16};
  p.a.assign((size_t)p.Kpad * p.Mpad, 0.f);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < K; ++k) p.a[(size_t)k * p.Mpad + m] = w[(size_t)m * K + k];
  return p;
}

GemmPlane pack_deconv_planes(const fvec& w, int ci, int co, int bm) {
  GemmPlane p{{}, (co + bm - 1) / bm * bm, (ci * 4 + 15) / 16 * 16};
  const size_t plane = (size_t)p.Kpad * p.Mpad;
  p.a.assign(4 * plane, 0.f);
  for (int par = 0; par < 4; ++par) {
    const int py = par >> 1, px = par & 1;
    for (int c = 0; c < ci; ++c)
      for (int ky = 0; ky < 2; ++ky)
        for (int kx = 0; kx < 2; ++kx) {
          const int k = c * 4 + ky * 2 + kx, sy = 3 - py - 2 * ky, sx = 3 - px - 2 * kx;
          for (int m = 0; m < co; ++m)
            p.a[par * plane + (size_t)k * p.Mpad + m] = w[(((size_t)c * co + m) * 4 + sy) * 4 + sx];
        }
  }
  return p;
}

Frags pack_gemm_x3(const GemmPlane& p, int npar, int M, int K, int bm, int kk) {
  const size_t plane = (size_t)p.Kpad * p.Mpad;
  const int ci = K / kk;
  Frags r = pack_frags(npar, M, K, bm, [&](int par, int m, int k, float& v) {
    v = p.a[par * plane + (size_t)k * p.Mpad + m];
    return true;
  });
  if (npar == 1 && kk > 1 && 32 % kk != 0 && ci % 8 == 0)
    r.tap_major = pack_frags(1, M, K, bm, [&](int, int m, int k, float& v) {
                    const int tap = k / ci, c = k - tap * ci;
                    v = p.a[(size_t)(c * kk + tap) * p.Mpad + m];
                    return true;
                  }).g;
  return r;
}

Frags pack_unit3d(const fvec& w, int M, int Cin, int Cpad, int KS, int bm, int stem_row) {
  const int KK = KS * KS * KS, K = stem_row ? KS * KS * stem_row : KK * Cpad;
  return pack_frags(1, M, K, bm, [&](int, int m, int k, float& v) {
    int tap = k / Cpad, ci = k - tap * Cpad;
    if (stem_row) {
      const int row = k / stem_row, j = k - row * stem_row;
      if (j >= KS * Cin) return false;
      tap = row * KS + j / Cin;
      ci = j % Cin;
    }
    if (ci >= Cin) return false;
    v = w[((size_t)m * Cin + ci) * KK + tap];
    return true;
  });
}

Frags pack_conv2d(const fvec& w, int M, int Cin, int Cpad, int KS, int bm, int stem_row) {
  const int KK = KS * KS, K = stem_row ? KS * stem_row : KK * Cpad;
  return pack_frags(1, M, K, bm, [&](int, int m, int k, float& v) {
    int tap = k / Cpad, ci = k - tap * Cpad;
    if (stem_row) {
      const int ky = k / stem_row, j = k - ky * stem_row;
      if (j >= KS * Cin) return false;
      tap = ky * KS + j / Cin;
      ci = j % Cin;
    }
    if (ci >= Cin) return false;
    v = w[((size_t)m * Cin + ci) * KK + tap];
    return true;
  });
}

// elem(m, k, v): element (m, k) of the dense matrix, or false where it has none
template <class F>
static TilesF32 tiles_f32(int M, int K, int bm, F&& elem) {
  const int nkt = (K + 31) / 32, mt = (M + bm - 1) / bm;
  TilesF32 r{fvec((size_t)mt * nkt * 32 * bm, 0.f), nkt};
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < K; ++k) {
      float v;
      if (!elem(m, k, v)) continue;
      r.a[(((size_t)(m / bm) * nkt + k / 32) * 32 + k % 32) * bm + m % bm] = v;
    }
  return r;
}

// `rows` rows of KS taps (KS kx * Cin ci elements, j = kx * Cin + ci) padded to stem_row
static TilesF32 stem_tiles_f32(const fvec& w, int M, int Cin, int KS, int KK, int rows, int bm, int stem_row) {
  return tiles_f32(M, rows * stem_row, bm, [&](int m, int k, float& v) {
    const int row = k / stem_row, j = k - row * stem_row;
    if (j >= KS * Cin) return false;
    v = w[((size_t)m * Cin + j % Cin) * KK + row * KS + j / Cin];
    return true;
  });
}

static TilesF32 tap_major_f32(const fvec& w, int M, int Cin, int Cpad, int KK, int bm) {
  return tiles_f32(M, KK * Cpad, bm, [&](int m, int k, float& v) {
    const int tap = k / Cpad, ci = k - tap * Cpad;
    if (ci >= Cin) return false;
    v = w[((size_t)m * Cin + ci) * KK + tap];
    return true;
  });
}

TilesF32 pack_conv3d_f32(const fvec& w, int M, int Cin, int Cpad, int KS, int bm) {
  return tap_major_f32(w, M, Cin, Cpad, KS * KS * KS, bm);
}
TilesF32 pack_conv3d_f32_stem(const fvec& w, int M, int Cin, int KS, int bm, int stem_row) {
  return stem_tiles_f32(w, M, Cin, KS, KS * KS * KS, KS * KS, bm, stem_row);
}
TilesF32 pack_conv2d_f32(const fvec& w, int M, int Cin, int Cpad, int KS, int bm) {
  return tap_major_f32(w, M, Cin, Cpad, KS * KS, bm);
}
TilesF32 pack_conv2d_f32_stem(const fvec& w, int M, int Cin, int KS, int bm, int stem_row) {
  return stem_tiles_f32(w, M, Cin, KS, KS * KS, KS, bm, stem_row);
}

Frags pack_x3(const fvec& w, int ks, int co, int ci, int bm, int ng) {
  const int kk = ks * ks, cib = 16 * ng, ncgb = (ci + cib - 1) / cib, mt = (co + bm - 1) / bm;
  const int m32 = bm / 32, steps = ng * ks;
  const size_t ah = (size_t)steps * m32 * 2 * 512;
  Frags r{std::vector<half_t>((size_t)mt * ncgb * ks * ah), fvec(co), ncgb};
  fvec scale(co);
  for (int m = 0; m < co; ++m) scale[m] = std::ldexp(1.f, row_exp(&w[(size_t)m * ci * kk], (size_t)ci * kk, r.rs[m]));
  for (int mtile = 0; mtile < mt; ++mtile)
    for (int cb = 0; cb < ncgb; ++cb)
      for (int ky = 0; ky < ks; ++ky)
        for (int g = 0; g < ng; ++g)
          for (int kx = 0; kx < ks; ++kx)
            for (int q = 0; q < m32; ++q)
              for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                  const int m = mtile * bm + q * 32 + (l & 31);
                  const int c = cb * cib + g * 16 + 8 * (l >> 5) + e;
                  if (m >= co || c >= ci) continue;
                  const size_t base = (((((size_t)mtile * ncgb + cb) * ks + ky) * steps + g * ks + kx) * m32 + q) * 2;
                  put_hilo(&r.g[base * 512 + l * 8 + e], w[((size_t)m * ci + c) * kk + ky * ks + kx] * scale[m]);
                }
  return r;
}

// [mtile][cblk][ky'][kx'][m32][hi|lo][lane][8] of elem(mtile, row in tile, cblk, ky', kx', channel
// in block, v): false where the layout has no element (stays zero); v comes scaled
template <class F>
static std::vector<half_t> pack_two_tap(int mt, int cblks, int bm, F&& elem) {
  const int m32 = bm / 32;
  std::vector<half_t> g((size_t)mt * cblks * 4 * m32 * 1024);
  for (int mtile = 0; mtile < mt; ++mtile)
    for (int cb = 0; cb < cblks; ++cb)
      for (int ky = 0; ky < 2; ++ky)
        for (int kx = 0; kx < 2; ++kx)
          for (int q = 0; q < m32; ++q)
            for (int l = 0; l < 64; ++l)
              for (int e = 0; e < 8; ++e) {
                float v;
                if (!elem(mtile, q * 32 + (l & 31), cb, ky, kx, 8 * (l >> 5) + e, v)) continue;
                const size_t base = (((((size_t)mtile * cblks + cb) * 2 + ky) * 2 + kx) * m32 + q) * 2;
                put_hilo(&g[base * 512 + l * 8 + e], v);
              }
  return g;
}

Frags pack_x3_deconv(const fvec& w, int ci, int co, int bm) {
  const int ncb = (ci + 15) / 16, mtc = (co + bm - 1) / bm;
  Frags r{{}, fvec(co), ncb};
  fvec scale(co);
  for (int m = 0; m < co; ++m) {
    float mx = 0.f;
    for (int c = 0; c < ci; ++c)
      for (int tap = 0; tap < 16; ++tap) mx = std::max(mx, std::fabs(w[((size_t)c * co + m) * 16 + tap]));
    scale[m] = std::ldexp(1.f, pow2_row_exp(mx, r.rs[m]));
  }
  r.g = pack_two_tap(4 * mtc, ncb, bm, [&](int mtile, int row, int cb, int ky, int kx, int cc, float& v) {
    const int ph = mtile / mtc, m = (mtile % mtc) * bm + row, c = cb * 16 + cc;
    if (m >= co || c >= ci) return false;
    v = w[(((size_t)c * co + m) * 4 + 3 - (ph >> 1) - 2 * ky) * 4 + 3 - (ph & 1) - 2 * kx] * scale[m];
    return true;
  });
  return r;
}

Frags pack_x3_down(const fvec& w, int co, int ci, int bm) {
  const int ncb = (ci + 15) / 16, mt = (co + bm - 1) / bm;
  Frags r{{}, fvec(co), 4 * ncb};
  fvec scale(co);
  for (int m = 0; m < co; ++m) scale[m] = std::ldexp(1.f, row_exp(&w[(size_t)m * ci * 16], (size_t)ci * 16, r.rs[m]));
  r.g = pack_two_tap(mt, 4 * ncb, bm, [&](int mtile, int row, int cblk, int ky, int kx, int cc, float& v) {
    const int q = cblk / ncb, m = mtile * bm + row, c = (cblk % ncb) * 16 + cc;
    if (m >= co || c >= ci) return false;
    v = w[(((size_t)m * ci + c) * 4 + 2 * ky + 1 - (q >> 1)) * 4 + 2 * kx + 1 - (q & 1)] * scale[m];
    return true;
  });
  return r;
}

HaloPack pack_halo(const fvec& w, int ks, int co, int ci, int bm, int ch) {
  const int kk = ks * ks, cib = 2 * ch, stages = (ci + cib - 1) / cib, mt = (co + bm - 1) / bm;
  const size_t afl = (size_t)ch * kk * 2 * bm;
  HaloPack r{fvec((size_t)mt * stages * afl, 0.f), stages};
  for (int m = 0; m < co; ++m) {
    const int mtile = m / bm, mm = m % bm;
    for (int c = 0; c < ci; ++c) {
      const int st = c / cib, rem = c % cib, half = rem / ch, cp = rem % ch;
      for (int tap = 0; tap < kk; ++tap)
        r.a[((size_t)mtile * stages + st) * afl + ((size_t)(cp * kk + tap) * 2 + half) * bm + mm] = w[((size_t)m * ci + c) * kk + tap];
    }
  }
  return r;
}

fvec pack_narrow(const fvec& w, int kk, int co, int ci, int cot) {
  const int ng = (co + cot - 1) / cot, cotp = (cot + 3) & ~3;
  fvec a((size_t)ng * ci * kk * cotp, 0.f);
  for (int m = 0; m < co; ++m)
    for (int c = 0; c < ci; ++c)
      for (int tap = 0; tap < kk; ++tap)
        a[(((size_t)(m / cot) * ci + c) * kk + tap) * cotp + m % cot] = w[((size_t)m * ci + c) * kk + tap];
  return a;
}

fvec reorder_time3(const fvec& w, int co, int ci, int kt, int kk) {
  fvec r(w.size());
  for (int m = 0; m < co; ++m)
    for (int c = 0; c < ci; ++c)
      for (int z = 0; z < kt; ++z)
        for (int q = 0; q < kk; ++q)
          r[(((size_t)m * kt * ci) + (size_t)z * ci + c) * kk + q] = w[(((size_t)m * ci + c) * kt + z) * kk + q];
  return r;
}

fvec split_channels(const fvec& w, int Co, int Cin, int kk, int lo, int hi) {
  fvec r((size_t)Co * (hi - lo) * kk);
  for (int m = 0; m < Co; ++m)
    std::copy(w.begin() + ((size_t)m * Cin + lo) * kk, w.begin() + ((size_t)m * Cin + hi) * kk,
              r.begin() + (size_t)m * (hi - lo) * kk);
  return r;
}

fvec fold_ln_gamma(const fvec& w, const fvec& gamma, int Co, int Cin) {
  fvec r((size_t)Co * Cin);
  for (int m = 0; m < Co; ++m)
    for (int c = 0; c < Cin; ++c)
      r[(size_t)m * Cin + c] = (float)((double)w[(size_t)m * Cin + c] * (double)gamma[c]);
  return r;
}

XPathPack pack_xpath(const fvec& wn, const fvec& bn, const fvec& wi, const fvec& bi, int Cm, int Co, int Cin, int L) {
  const int M32 = (Co + 31) / 32, MP = M32 * 32;
  // V[m][ci][a][b][e][f] = sum_c' Wa[m][c'][a][b] Wn[c'][ci][e][f]; U[m][a][b] = sum_c' Wa bn
  std::vector<double> V((size_t)Co * 3 * 49 * 49, 0.0), U((size_t)Co * 49, 0.0);
  for (int m = 0; m < Co; ++m)
    for (int ab = 0; ab < 49; ++ab)
      for (int c = 0; c < Cm; ++c) {
        const double wa = wi[((size_t)m * Cin + c) * 49 + ab];
        if (wa == 0.0) continue;
        U[(size_t)m * 49 + ab] += wa * bn[c];
        for (int ci = 0; ci < 3; ++ci) {
          const float* pn = &wn[((size_t)c * 3 + ci) * 49];
          double* pv = &V[(((size_t)m * 3 + ci) * 49 + ab) * 49];
          for (int ef = 0; ef < 49; ++ef) pv[ef] += wa * pn[ef];
        }
      }
  // tap a of a class (offset a - 3 from p) is valid iff p + a - 3 lies in [0, L)
  auto valid = [&](int cls1, int a) {
    const int p = cls1 < 3 ? cls1 : (cls1 == 3 ? 3 : L - 7 + cls1), q = p + a - 3;
    return cls1 == 3 || (q >= 0 && q < L);
  };
  const size_t per_cls = (size_t)3 * 13 * M32 * 1024;
  XPathPack r{std::vector<half_t>(49 * per_cls), fvec((size_t)49 * MP), fvec((size_t)49 * MP)};
  std::vector<double> K((size_t)Co * 3 * 169);
  for (int cls = 0; cls < 49; ++cls) {
    const int cy = cls / 7, cx = cls % 7;
    std::fill(K.begin(), K.end(), 0.0);
    for (int m = 0; m < Co; ++m) {
      double cbv = bi[m];
      for (int a = 0; a < 7; ++a)
        for (int b = 0; b < 7; ++b) {
          if (!valid(cy, a) || !valid(cx, b)) continue;
          cbv += U[(size_t)m * 49 + a * 7 + b];
          for (int ci = 0; ci < 3; ++ci) {
            const double* pv = &V[(((size_t)m * 3 + ci) * 49 + a * 7 + b) * 49];
            double* pk = &K[((size_t)m * 3 + ci) * 169];
            for (int e = 0; e < 7; ++e)
              for (int f = 0; f < 7; ++f) pk[(a + e) * 13 + (b + f)] += pv[e * 7 + f];
          }
        }
      r.cb[(size_t)cls * MP + m] = (float)cbv;
      const int e2 = row_exp(&K[(size_t)m * 3 * 169], 3 * 169, r.rs[(size_t)cls * MP + m]);
      for (int ci = 0; ci < 3; ++ci)
        for (int dy = 0; dy < 13; ++dy)
          for (int dx = 0; dx < 13; ++dx) {
            const float v = (float)std::ldexp(K[((size_t)m * 3 + ci) * 169 + dy * 13 + dx], e2);
            put_hilo(afrag(&r.g[(size_t)cls * per_cls + ((size_t)(ci * 13 + dy) * M32 + m / 32) * 1024], m, dx), v);
          }
    }
  }
  return r;
}

Frags pack_conv7c3(const fvec& w, int Cm) {
  const int M32 = (Cm + 31) / 32;
  Frags r{std::vector<half_t>((size_t)12 * M32 * 1024), fvec(M32 * 32, 0.f)};
  for (int m = 0; m < Cm; ++m) {
    const int e2 = row_exp(&w[(size_t)m * 147], 147, r.rs[m]);
    for (int ci = 0; ci < 3; ++ci)
      for (int dy = 0; dy < 7; ++dy)
        for (int dx = 0; dx < 7; ++dx) {
          const float v = std::ldexp(w[(((size_t)m * 3 + ci) * 7 + dy) * 7 + dx], e2);
          put_hilo(afrag(&r.g[((size_t)(ci * 4 + dy / 2) * M32 + m / 32) * 1024], m, 8 * (dy % 2) + dx), v);
        }
  }
  return r;
}

// up2 of a length-n axis, align_corners=False, as F.interpolate: weight of F[k] in row r
// (0 outside [0, 2n): the 7x7's zero padding), and the unclamped interpolation of the
// zero-padded F (any integer r)
static double up_true(int r, int k, int n) {
  if (r < 0 || r >= 2 * n) return 0.0;
  const double src = std::max(0.0, (r + 0.5) * 0.5 - 0.5);
  const int k0 = (int)src, k1 = k0 < n - 1 ? k0 + 1 : k0;
  const double lam = src - k0;
  return (k == k0 ? 1.0 - lam : 0.0) + (k == k1 ? lam : 0.0);
}
static double up_inf(int r, int k) {
  const int j = (r >= 0 ? r : r - 1) / 2;  // floor(r / 2)
  if (k == j) return 0.75;
  return (r - 2 * j == 0 ? k == j - 1 : k == j + 1) ? 0.25 : 0.0;
}

FeaPhasePack pack_fea_phase(const fvec& wt, int Co, int Cf, int n) {
  auto W = [&](int co, int ci, int dy, int dx) { return (double)wt[(((size_t)co * Cf + ci) * 7 + dy) * 7 + dx]; };
  // interior composition A[p][l][d]: weight of tap l (F[m - 2 + l]) in row 2m + p + d - 3 (any m)
  double A[2][5][7];
  for (int p = 0; p < 2; ++p)
    for (int l = 0; l < 5; ++l)
      for (int d = 0; d < 7; ++d) A[p][l][d] = up_inf(2 * 8 + p + d - 3, 8 - 2 + l);
  // edge deltas: U - Uinf at column ke of output row r (nonzero for ke = 0 / n - 1 only)
  auto delta = [&](int r, int ke) { return up_true(r, ke, n) - up_inf(r, ke); };
  FeaPhasePack r;
  // main 5x5 phase kernels, row ph * Co + co, ph = 2 py + px
  r.k5.assign((size_t)4 * Co * Cf * 25, 0.f);
  std::vector<double> t(7 * 5);
  for (int co = 0; co < Co; ++co)
    for (int ci = 0; ci < Cf; ++ci)
      for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
          // t[dy][lx] = sum_dx W[dy][dx] A[px][lx][dx]
          for (int dy = 0; dy < 7; ++dy)
            for (int lx = 0; lx < 5; ++lx) {
              double s_ = 0.0;
              for (int dx = 0; dx < 7; ++dx) s_ += W(co, ci, dy, dx) * A[px][lx][dx];
              t[dy * 5 + lx] = s_;
            }
          for (int ly = 0; ly < 5; ++ly)
            for (int lx = 0; lx < 5; ++lx) {
              double s_ = 0.0;
              for (int dy = 0; dy < 7; ++dy) s_ += A[py][ly][dy] * t[dy * 5 + lx];
              r.k5[((((size_t)(2 * py + px) * Co + co) * Cf + ci) * 5 + ly) * 5 + lx] = (float)s_;
            }
        }
  // edge lines: [pair][side][row m = co * 8 + (d*2 + py)*2 + px][ci][tap], then f16x3-packed
  const int R = 8 * Co, MT = (R + 127) / 128, RP = MT * 128, ncb = Cf / 16;
  std::vector<double> ws((size_t)4 * R * Cf * 5, 0.0);
  for (int pair = 0; pair < 2; ++pair)
    for (int side = 0; side < 2; ++side) {
      const int ke = side ? n - 1 : 0, base = side ? 2 * n - 4 : 0;
      for (int d = 0; d < 2; ++d)
        for (int py = 0; py < 2; ++py)
          for (int px = 0; px < 2; ++px) {
            // pair 0: output row y = base + 2d + py (the delta axis), columns by phase px;
            // pair 1: output column x = base + 2d + px, rows by phase py
            const int e = base + 2 * d + (pair ? px : py), ip = pair ? py : px;
            double dl[7];
            for (int k = 0; k < 7; ++k) dl[k] = delta(e + k - 3, ke);
            for (int co = 0; co < Co; ++co) {
              const int m = co * 8 + (d * 2 + py) * 2 + px;  // fea_x3.hip row order
              for (int ci = 0; ci < Cf; ++ci)
                for (int l = 0; l < 5; ++l) {
                  double s_ = 0.0;
                  for (int dy = 0; dy < 7; ++dy)
                    for (int dx = 0; dx < 7; ++dx)
                      s_ += W(co, ci, dy, dx) * (pair ? dl[dx] * A[ip][l][dy] : dl[dy] * A[ip][l][dx]);
                  ws[((((size_t)pair * 2 + side) * R + m) * Cf + ci) * 5 + l] = s_;
                }
            }
          }
    }
  const size_t ah = (size_t)5 * 4 * 2 * 512;  // halves per (mtile, cb): [tap][m32][hl][lane][8]
  r.side.assign((size_t)4 * MT * ncb * ah, (half_t)0.f);
  r.side_scale.assign((size_t)4 * RP, 1.f);
  for (int ps = 0; ps < 4; ++ps)
    for (int m = 0; m < R; ++m) {
      const int e2 = row_exp(&ws[((size_t)ps * R + m) * Cf * 5], (size_t)Cf * 5, r.side_scale[(size_t)ps * RP + m]);
      const int mtile = m / 128, m32 = (m % 128) / 32;
      for (int ci = 0; ci < Cf; ++ci)
        for (int l = 0; l < 5; ++l) {
          const float v = (float)std::ldexp(ws[(((size_t)ps * R + m) * Cf + ci) * 5 + l], e2);
          const size_t b0 = ((((size_t)ps * MT + mtile) * ncb + ci / 16) * ah) + (size_t)((l * 4 + m32) * 2) * 512;
          put_hilo(afrag(&r.side[b0], m, ci % 16), v);
        }
    }
  // corners [corner = 2 (bottom) + (right)][ci][co][p = yy * 4 + xx]
  r.corner.assign((size_t)4 * 16 * Cf * Co, 0.f);
  for (int corner = 0; corner < 4; ++corner) {
    const int ky = (corner >> 1) ? n - 1 : 0, kx = (corner & 1) ? n - 1 : 0;
    const int yb = (corner >> 1) ? 2 * n - 4 : 0, xb = (corner & 1) ? 2 * n - 4 : 0;
    for (int p = 0; p < 16; ++p) {
      double dy_[7], dx_[7];
      for (int k = 0; k < 7; ++k) {
        dy_[k] = delta(yb + p / 4 + k - 3, ky);
        dx_[k] = delta(xb + p % 4 + k - 3, kx);
      }
      for (int ci = 0; ci < Cf; ++ci)
        for (int co = 0; co < Co; ++co) {
          double s_ = 0.0;
          for (int dy = 0; dy < 7; ++dy)
            for (int dx = 0; dx < 7; ++dx) s_ += W(co, ci, dy, dx) * dy_[dy] * dx_[dx];
          r.corner[(((size_t)corner * Cf + ci) * Co + co) * 16 + p] = (float)s_;
        }
    }
  }
  return r;
}

fvec pack_stw_rows(const fvec& w, int nmat, int rows, int K) {
  fvec a((size_t)(rows / 32) * (K / 2) * nmat * 64);
  for (int u = 0; u < rows / 32; ++u)
    for (int s2 = 0; s2 < K / 2; ++s2)
      for (int wh = 0; wh < nmat; ++wh)
        for (int l = 0; l < 64; ++l)
          a[(((size_t)u * (K / 2) + s2) * nmat + wh) * 64 + l] =
              w[(size_t)(wh * rows + u * 32 + (l & 31)) * K + 2 * s2 + (l >> 5)];
  return a;
}

AttnX3Pack pack_attn_x3(const fvec& wqkv, const fvec& wproj, const fvec& ng, const fvec* nb, int C, int hid, int uh,
                        float q_scale) {
  const int units = hid / 32, KS = C / 16, CT = C / 32;
  float inv[4], sc[4];
  for (int m = 0; m < 3; ++m) sc[m] = pow2_scale(wqkv.data() + (size_t)m * hid * C, (size_t)hid * C, inv[m]);
  sc[3] = pow2_scale(wproj.data(), wproj.size(), inv[3]);
  AttnX3Pack r;
  r.a.resize((size_t)units * uh);
  for (int u = 0; u < units; ++u) {
    const size_t ub = (size_t)u * uh;
    for (int m = 0; m < 3; ++m)
      for (int s2 = 0; s2 < KS; ++s2)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 8; ++e) {
            const int row = m * hid + u * 32 + (l & 31), c = 16 * s2 + 8 * (l >> 5) + e;
            put_hilo(&r.a[ub + ((size_t)m * KS + s2) * 1024 + l * 8 + e], wqkv[(size_t)row * C + c] * sc[m]);
          }
    for (int ct = 0; ct < CT; ++ct)
      for (int s2 = 0; s2 < 2; ++s2)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 8; ++e) {
            const int c = ct * 32 + (l & 31);
            const int hd = u * 32 + 16 * s2 + 8 * (e >> 2) + 4 * (l >> 5) + (e & 3);
            put_hilo(&r.a[ub + ((size_t)3 * KS + ct * 2 + s2) * 1024 + l * 8 + e], wproj[(size_t)c * hid + hd] * sc[3]);
          }
  }
  // Operand exponents (stw_x3.hip kernel header). Relative to a split input of largest
  // |value| in [1, 2) (the kernel's 2^e_w carries a further 2^8, folded back through the
  // factors below); channel c of it is then ~ (|g_c| + |b_c|) * 2^e_x / 4 (e_x
  // brings the largest affine to [1, 2); a unit-variance z peaks near 4). e_q / e_k / e_v
  // bring the largest expected row norm of q * q_scale, k, v (weights times those channel
  // scales) to [1, 2). Powers of two: the scaling itself is exact.
  std::vector<double> sx(C);
  double mx = 0.0;
  for (int c = 0; c < C; ++c) {
    sx[c] = std::fabs((double)ng[c]) + (nb ? std::fabs((double)(*nb)[c]) : 0.0);
    mx = std::max(mx, sx[c]);
  }
  const int ex = pow2_exp(mx);
  int em[3];
  for (int m = 0; m < 3; ++m) {
    double best = 0.0;
    for (int d = 0; d < hid; ++d) {
      double n2 = 0.0;
      for (int c = 0; c < C; ++c) {
        const double w = (double)wqkv[((size_t)m * hid + d) * C + c] * std::ldexp(sx[c], ex) * 0.25;
        n2 += w * w;
      }
      best = std::max(best, std::sqrt(n2));
    }
    // to [2^4, 2^5) for q and k, [2^2, 2^3) for v: values down to 2^-7 / 2^-5 of the typical
    // one keep a normal lo, with headroom to 65504 (O = P' v' <= 16 max|v'| with P' = 16 P)
    em[m] = pow2_exp(best * (m == 0 ? (double)q_scale : 1.0)) + (m < 2 ? 4 : 2);
  }
  for (int m = 0; m < 3; ++m) r.sc[m] = std::ldexp(inv[m], em[m]);
  r.sc[3] = std::ldexp(inv[3], -(em[2] + 4));
  r.sc[4] = (float)std::ldexp(1.4426950408889634, -(em[0] + em[1]));
  r.s2 = std::ldexp(1.f, em[0] + em[1]);
  return r;
}

Affine bn_fold_f32(const fvec& w, const fvec& b, const fvec& rm, const fvec& rv) {
  Affine r{fvec(w.size()), fvec(w.size())};
  for (size_t i = 0; i < w.size(); ++i) {
    volatile float inv = 1.0f / std::sqrt(rv[i] + 1e-5f);
    r.a[i] = inv * w[i];
    volatile float t = rm[i] * r.a[i];
    r.b[i] = b[i] - t;
  }
  return r;
}

// BatchNorm3d (eval, eps 1e-5; pytorch_i3d.py:69): y = x * a + b, computed in fp64
Affine bn_fold_f64(const fvec& w, const fvec& b, const fvec& rm, const fvec& rv) {
  Affine r{fvec(w.size()), fvec(w.size())};
  for (size_t m = 0; m < w.size(); ++m) {
    const double s_ = (double)w[m] / std::sqrt((double)rv[m] + 1e-5);
    r.a[m] = (float)s_;
    r.b[m] = (float)((double)b[m] - (double)rm[m] * s_);
  }
  return r;
}

}  // namespace extdm
