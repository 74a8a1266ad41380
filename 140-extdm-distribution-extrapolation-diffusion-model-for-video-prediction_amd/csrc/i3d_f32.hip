// The exact-fp32 route of InceptionI3d: conv3d_f32_kernel (every Unit3D, the counterpart of
// i3d.hip's conv3d_x3_kernel) as an implicit GEMM on v_mfma_f32_32x32x2_f32 (the instruction and
// operand layout of conv.hip):
//   C[m][n] = sum_k A[m][k] B[k][n],  m = output channel, n = (b, to, oy, ox),
//   k = tap * Cpad + ci (tap-major, Cpad = Cin rounded up to 8), or the stem's padded rows
//   (kStemRow 24).
// The tile loop and its arithmetic (exact fp32 products, k ascending, a partial accumulator added
// to the total every KCHUNK K tiles, the BM x 128 x 32 block of 4 waves) are f32_tiles.h's, shared
// with lpips_f32.hip. A column is computed by one lane group whatever its
// tile, the m-tile depends on Cout alone and there is no split-K, so an output does not depend on
// the batch it sits in. A packed per (mtile, ktile) as [k 32][BM]
// (pack_conv3d_f32). The gather is the TAPK scheme of the f16x3 kernels: a
// thread's 8-element group is 8 channels of one tap, so the tap, the in-volume test and the voxel's
// byte offset are computed once per group and the channel volumes are wave-uniform bases (4-byte
// buffer loads: voxel offset in voffset, the channel in soffset). Out-of-volume taps read 0.
#include "f32_tiles.h"
#include "i3d.h"
#include "kernels.h"

namespace extdm {

namespace {

using namespace f32gemm;  // f32x16, BN, BK, KCHUNK, f32_tiles, column_tile, lds_bytes

struct C3Args {
  const float* in; long ib, ic;
  int Cin, Cpad, Ti, Hi, Wi;
  const float* w; int nkt;
  float* out; long ob, oc, ot;
  int Cout, To, Ho, Wo;
  int stride, pt, ph, pw;  // front pads
  const float* post_scale; const float* post_shift; int relu;
  long N;
};

// STEM: the 3 -> 64 7x7x7 stride-2 unit in the (kt, ky)-row layout of conv3d_x3_kernel,
//   k = (kt * 7 + ky) * 24 + kx * 3 + ci,   K = 1176.
template <int KS, int BM, bool STEM = false>
__global__ __launch_bounds__(256) void conv3d_f32_kernel(C3Args a) {
  constexpr int WAVES_M = BM >= 64 ? 2 : 1;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int TM = BM / (32 * WAVES_M);
  constexpr int TN = BN / (32 * WAVES_N);
  constexpr int KK = KS * KS * KS;

  extern __shared__ __attribute__((aligned(16))) float smf[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int h = lane >> 5, lc = lane & 31;
  const long n0 = column_tile() * BN;
  const int mt = blockIdx.y;

  // ---- per-thread gather column (B operand) ----
  const long n = n0 + (tid & (BN - 1));
  const bool nvalid = n < a.N;
  int it0, iy0, ix0;
  long base;
  {
    long nn = nvalid ? n : 0;
    const int ox = (int)(nn % a.Wo); nn /= a.Wo;
    const int oy = (int)(nn % a.Ho); nn /= a.Ho;
    const int to = (int)(nn % a.To);
    const int b = (int)(nn / a.To);
    it0 = to * a.stride - a.pt;
    iy0 = oy * a.stride - a.ph;
    ix0 = ox * a.stride - a.pw;
    base = (long)b * a.ib;
  }

  auto gather = [&](int kb, float (&v8)[8]) __attribute__((always_inline)) {
    if constexpr (STEM) {
      const int row = kb / 24, j0 = kb - row * 24;  // row = kt * 7 + ky
      const int kt_ = row / 7, ky = row - kt_ * 7;
      const int it = it0 + kt_, iy = iy0 + ky;
      const bool okr = nvalid && row < 49 && it >= 0 && it < a.Ti && iy >= 0 && iy < a.Hi;
      const long rowoff = base + ((long)it * a.Hi + iy) * a.Wi;
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, -1, 0x00020000);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = j0 + e, kx = j / 3, ci = j - 3 * kx;  // wave-uniform
        const int ix = ix0 + kx;
        const bool ok = okr && j < 21 && ix >= 0 && ix < a.Wi;
        const unsigned vo = ok ? (unsigned)((rowoff + ix) * 4) : 0u;
        const float v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, (int)(ci * a.ic * 4), 0));
        v8[e] = ok ? v : 0.f;
      }
    } else {
      const int tap = kb / a.Cpad, ci0 = kb - tap * a.Cpad;
      const int kt_ = tap / (KS * KS), r = tap - kt_ * (KS * KS);
      const int ky = r / KS, kx = r - ky * KS;
      const int it = it0 + kt_, iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = nvalid && tap < KK && it >= 0 && it < a.Ti && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
      const unsigned vo = ok ? (unsigned)((base + ((long)it * a.Hi + iy) * a.Wi + ix) * 4) : 0u;
      const int cb = tap < KK ? ci0 : 0;
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + (long)cb * a.ic), 0, -1, 0x00020000);
      const int cst4 = (int)(a.ic * 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = 0.f;
        if (cb + e < a.Cin) v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, e * cst4, 0));
        v8[e] = ok ? v : 0.f;
      }
    }
  };

  f32x16 acc[TM][TN];
  f32_tiles<BM>(a.w + (long)mt * a.nkt * (BK * BM), a.nkt, smf, gather, acc);

  // ---- epilogue (C/D map: col = lane & 31, row = (r&3) + 8(r>>2) + 4h); rows past Cout (the
  // packing's pad rows) are not stored ----
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long nn0 = n0 + (wn * TN + j) * 32 + lc;
    if (nn0 >= a.N) continue;
    long nn = nn0;
    const int ox = (int)(nn % a.Wo); nn /= a.Wo;
    const int oy = (int)(nn % a.Ho); nn /= a.Ho;
    const int to = (int)(nn % a.To);
    const int b = (int)(nn / a.To);
    const long obase = (long)b * a.ob + (long)to * a.ot + (long)oy * a.Wo + ox;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mt * BM + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m >= a.Cout) continue;
        float v = acc[i][j][r];
        if (a.post_scale) v = v * a.post_scale[m] + a.post_shift[m];
        if (a.relu) v = v > 0.f ? v : 0.f;
        a.out[obase + (long)m * a.oc] = v;
      }
    }
  }
}

template <int KS, int BM, bool STEM = false>
void launch_c3(hipStream_t s, const C3Args& a, dim3 grid) {
  // set on every launch: the attribute belongs to the current device's copy of the kernel, and a
  // host call per launch is noise beside a convolution (the 128-row tile needs 64 KiB)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3d_f32_kernel<KS, BM, STEM>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(BM));
  hipLaunchKernelGGL((conv3d_f32_kernel<KS, BM, STEM>), grid, dim3(256), lds_bytes(BM), s, a);
}

template <int KS>
bool launch_c3_bm(hipStream_t s, const C3Args& a, int bm, dim3 grid) {
  if (bm == 128) launch_c3<KS, 128>(s, a, grid);
  else if (bm == 64) launch_c3<KS, 64>(s, a, grid);
  else if (bm == 32) launch_c3<KS, 32>(s, a, grid);
  else return false;
  return true;
}

}  // namespace

bool conv3d_f32_forward(hipStream_t s, const Vol& in, const Conv3dW& w, int stride, float* out, long ob, long oc,
                        long ot, const float* post_scale, const float* post_shift, bool relu) {
  if (!w.w || w.wscale || in.C != w.Cin || (stride != 1 && stride != 2)) return false;
  C3Args a{};
  a.in = in.p; a.ib = in.sb; a.ic = in.sc;
  a.Cin = w.Cin; a.Cpad = w.Cpad; a.Ti = in.T; a.Hi = in.H; a.Wi = in.W;
  a.w = reinterpret_cast<const float*>(w.w); a.nkt = w.nkt;
  a.out = out; a.ob = ob; a.oc = oc; a.ot = ot;
  a.Cout = w.M;
  a.To = same_out(in.T, stride); a.Ho = same_out(in.H, stride); a.Wo = same_out(in.W, stride);
  a.stride = stride;
  a.pt = same_pad(in.T, w.KS, stride) / 2;
  a.ph = same_pad(in.H, w.KS, stride) / 2;
  a.pw = same_pad(in.W, w.KS, stride) / 2;
  a.post_scale = post_scale; a.post_shift = post_shift; a.relu = relu ? 1 : 0;
  a.N = (long)in.B * a.To * a.Ho * a.Wo;
  // a voxel's byte offset from its channel volume (the batch base included) plus the soffset of
  // channel 7 of a group stay below 2^32; the soffset itself below 2^31
  const long e0 = ((long)(in.B - 1) * in.sb + in.thw()) * 4, c7 = 7 * 4 * in.sc;
  if (e0 + c7 >= (1L << 32) - 1 || c7 >= (1L << 31) || a.N <= 0) return false;
  const long ntile = (a.N + BN - 1) / BN;
  if (ntile > 0x7fffffffL) return false;
  dim3 grid((unsigned)ntile, (unsigned)((w.M + w.bm - 1) / w.bm), 1);
  if (w.stem) {
    if (w.KS != 7 || w.Cin != 3 || w.bm != 64) return false;
    launch_c3<7, 64, true>(s, a, grid);
    return true;
  }
  if (w.Cpad % 8 != 0 || w.Cpad < w.Cin) return false;
  if (w.KS == 1) return launch_c3_bm<1>(s, a, w.bm, grid);
  if (w.KS == 3) return launch_c3_bm<3>(s, a, w.bm, grid);
  if (w.KS == 7) return launch_c3_bm<7>(s, a, w.bm, grid);
  return false;
}

}  // namespace extdm
