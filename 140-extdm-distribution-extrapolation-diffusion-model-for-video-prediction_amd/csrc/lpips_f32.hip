// The exact-fp32 route of LPIPS (EXTDM_LPIPS_FP32): conv2d_f32_kernel, the counterpart of
// lpips.hip's conv2d_x3_kernel for AlexNet's five convs, as an implicit GEMM on
// v_mfma_f32_32x32x2_f32:
//   C[m][n] = sum_k A[m][k] B[k][n],  m = output channel, n = (image, oy, ox),
//   k = (ky * KS + kx) * Cpad + ci (tap-major), or the stem's padded ky rows
//   (k = ky * 40 + kx * 3 + ci, K = 440).
// The tile loop and its arithmetic (exact fp32 products, k ascending, a partial accumulator added
// to the total every KCHUNK K tiles, the BM x 128 x 32 block of 4 waves) are f32_tiles.h's, shared
// with i3d_f32.hip: no hi / lo split, no row scale, no range flag. A column is computed by one lane
// group whatever its tile, the m-tile is 64 rows for every Cout (kLpipsF32Bm) and there is no
// split-K, so an output does not depend on the batch it sits in. A packed per (mtile, ktile) as [k 32][BM]
// (pack_conv2d_f32). The gather is conv2d_x3_kernel's: a thread's 8-element group is 8 channels of
// one tap (the stem: 8 (kx, ci) elements of one ky row), so the tap, the in-image test and the
// pixel's byte offset are computed once per group and the channel planes are wave-uniform bases
// (4-byte buffer loads: pixel offset in voffset, the channel in soffset). Out-of-image taps read 0.
// The stem's front end (LpipsFront) runs on each gathered value as it does there. The epilogue is
// bias + ReLU.
#include "f32_tiles.h"
#include "lpips.h"

namespace extdm {

namespace {

using namespace f32gemm;  // f32x16, BN, BK, f32_tiles, column_tile, lds_bytes

struct C2F32Args {
  const float* in; long ib, ic;
  int Cin, Cpad, Hi, Wi;
  const float* w; int nkt;
  const float* bias;
  float* out;
  int Cout, Ho, Wo;
  int stride, pad;
  int pre; float sh0, sh1, sh2;  // the stem's front end (LpipsFront)
  long N;
};

template <int KS, int BM, bool STEM = false>
__global__ __launch_bounds__(256) void conv2d_f32_kernel(C2F32Args a) {
  constexpr int WAVES_M = BM >= 64 ? 2 : 1;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int TM = BM / (32 * WAVES_M);
  constexpr int TN = BN / (32 * WAVES_N);
  constexpr int KK = KS * KS;

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
  int iy0, ix0;
  long base;
  {
    long nn = nvalid ? n : 0;
    const int ox = (int)(nn % a.Wo); nn /= a.Wo;
    const int oy = (int)(nn % a.Ho);
    const int b = (int)(nn / a.Ho);
    iy0 = oy * a.stride - a.pad;
    ix0 = ox * a.stride - a.pad;
    base = (long)b * a.ib;
  }

  auto gather = [&](int kb, float (&v8)[8]) __attribute__((always_inline)) {
    if constexpr (STEM) {
      const int ky = kb / kLpipsStemRow, j0 = kb - ky * kLpipsStemRow;
      const int iy = iy0 + ky;
      const bool okr = nvalid && ky < KS && iy >= 0 && iy < a.Hi;
      const long rowoff = base + (long)iy * a.Wi;
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, -1, 0x00020000);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = j0 + e, kx = j / 3, ci = j - 3 * kx;  // wave-uniform
        const int ix = ix0 + kx;
        const bool ok = okr && j < 3 * KS && ix >= 0 && ix < a.Wi;
        const unsigned vo = ok ? (unsigned)((rowoff + ix) * 4) : 0u;
        float v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, (int)(ci * a.ic * 4), 0));
        if (a.pre > 0) v = v * 2.f - 1.f;
        if (a.pre > 1) v = v * 2.f - 1.f;
        v = v - (ci == 0 ? a.sh0 : (ci == 1 ? a.sh1 : a.sh2));
        v8[e] = ok ? v : 0.f;
      }
    } else {
      const int tap = kb / a.Cpad, ci0 = kb - tap * a.Cpad;
      const int ky = tap / KS, kx = tap - ky * KS;
      const int iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = nvalid && tap < KK && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
      const unsigned vo = ok ? (unsigned)((base + (long)iy * a.Wi + ix) * 4) : 0u;
      const int cb = tap < KK ? ci0 : 0;
      // the group's first channel plane as the (uniform) buffer base: pixel offset in voffset,
      // channel e's plane offset in soffset
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
  const long hw = (long)a.Ho * a.Wo;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long nn0 = n0 + (wn * TN + j) * 32 + lc;
    if (nn0 >= a.N) continue;
    const long b = nn0 / hw, pix = nn0 - b * hw;
    const long obase = b * a.Cout * hw + pix;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mt * BM + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m >= a.Cout) continue;
        const float v = acc[i][j][r] + a.bias[m];
        a.out[obase + (long)m * hw] = v > 0.f ? v : 0.f;
      }
    }
  }
}

template <int KS, int BM, bool STEM = false>
void launch_c2f(hipStream_t s, const C2F32Args& a, dim3 grid) {
  // set on every launch: the attribute belongs to the current device's copy of the kernel, and a
  // host call per launch is noise beside a convolution
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_f32_kernel<KS, BM, STEM>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(BM));
  hipLaunchKernelGGL((conv2d_f32_kernel<KS, BM, STEM>), grid, dim3(256), lds_bytes(BM), s, a);
}

}  // namespace

bool conv2d_f32_forward(hipStream_t s, const float* in, long ib, long ic, int B, int Hi, int Wi, const Conv2dW& w,
                        const LpipsFront* front, float* out) {
  if (!w.w || w.wscale || !w.bias || w.bm != kLpipsF32Bm || (w.stem != (front != nullptr))) return false;
  C2F32Args a{};
  a.in = in; a.ib = ib; a.ic = ic;
  a.Cin = w.Cin; a.Cpad = w.Cpad; a.Hi = Hi; a.Wi = Wi;
  a.w = reinterpret_cast<const float*>(w.w); a.nkt = w.nkt;
  a.bias = w.bias;
  a.out = out;
  a.Cout = w.M;
  a.Ho = conv2d_out(Hi, w.KS, w.stride, w.pad); a.Wo = conv2d_out(Wi, w.KS, w.stride, w.pad);
  a.stride = w.stride; a.pad = w.pad;
  if (front) { a.pre = front->pre; a.sh0 = front->shift[0]; a.sh1 = front->shift[1]; a.sh2 = front->shift[2]; }
  if (B <= 0 || a.Ho <= 0 || a.Wo <= 0) return false;
  a.N = (long)B * a.Ho * a.Wo;
  // a pixel's byte offset from its channel plane (the batch base included) plus the soffset of
  // channel 7 of a group stay below 2^32; the soffset itself below 2^31
  const long e0 = ((long)(B - 1) * ib + (long)Hi * Wi) * 4, c7 = 7 * 4 * ic;
  if (ib < 0 || ic < 0 || e0 + c7 >= (1L << 32) - 1 || c7 >= (1L << 31)) return false;
  const long ntile = (a.N + BN - 1) / BN;
  if (ntile > 0x7fffffffL) return false;
  const dim3 grid((unsigned)ntile, (unsigned)((w.M + w.bm - 1) / w.bm), 1);
  if (w.stem) {
    if (w.KS != 11 || w.Cin != 3 || w.stride != 4 || w.nkt != (11 * kLpipsStemRow + BK - 1) / BK) return false;
    launch_c2f<11, kLpipsF32Bm, true>(s, a, grid);
    return true;
  }
  if (w.Cin % 8 != 0 || w.Cpad != w.Cin || w.stride != 1 || w.nkt != (w.KS * w.KS * w.Cpad + BK - 1) / BK) return false;
  if (w.KS == 5) launch_c2f<5, kLpipsF32Bm>(s, a, grid);
  else if (w.KS == 3) launch_c2f<3, kLpipsF32Bm>(s, a, grid);
  else return false;
  return true;
}

}  // namespace extdm
