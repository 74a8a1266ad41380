// LPIPS (lpips.LPIPS(net='alex', version='0.1'), the metric of metrics/calculate_lpips.py): the
// five AlexNet feature convolutions as one f16x3 implicit GEMM across images, MaxPool2d(3, 2), the
// fused distance head (channel norms, squared difference, 1x1 lin), the weighted mean of the
// upsampled map and the spatial map itself.
//
// conv2d_x3_kernel is the 2-D member of the conv_gemm_x3.hip / i3d.hip family and shares its
// arithmetic (fp32 storage, hi / lo fp16 split while staging, three v_mfma_f32_32x32x16_f16
// products into fp32 accumulators, A rows pre-scaled by powers of two, the sticky |v| >= 65504
// flag):
//   C[m][n] = sum_k A[m][k] B[k][n],  m = output channel, n = (image, oy, ox),
//   k = (ky * KS + kx) * Cpad + ci   (tap-major; Cin is a multiple of 8 past the stem).
// n runs across images, so a 128-column tile spans many of the 3x3 or 7x7 maps of a 64x64 input.
// Block tile BM x 128 x 32, 256 threads = 4 waves, LDS double buffer with a register prefetch of
// the next K tile; A packed per (mtile, ktile) as [step][m32][hi|lo][lane][8] (pack_conv2d). The
// gather is the TAPK scheme of conv3d_x3_kernel: a thread's 8-element group is 8 channels of one
// tap, so the tap, the in-image test and the pixel's byte offset are computed once per group and
// the channel planes are wave-uniform bases (buffer loads: pixel offset in voffset, the channel in
// soffset). Out-of-image taps read 0. The epilogue is bias + ReLU.
#include "lpips.h"
#include "kernels.h"

namespace extdm {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int BN = 128;
constexpr int BK = 32;

struct C2Args {
  const float* in; long ib, ic;
  int Cin, Cpad, Hi, Wi;
  const _Float16* w; const float* wscale; int nkt;
  const float* bias;
  float* out;
  int Cout, Ho, Wo;
  int stride, pad;
  int pre; float sh0, sh1, sh2;  // the stem's front end (LpipsFront)
  long N;
  int* range;
};

// STEM (the 3 -> 64 11x11 stride-4 conv, 363 terms): padding 3 channels to 8 per tap would make
// K = 968. Instead a ky row of taps is the unit, as in conv3d_x3_kernel<7, 64, STEM>: its 33
// (kx, ci) elements padded to 40,
//   k = ky * 40 + kx * 3 + ci,   K = 440 (+21 %),
// so a thread's 8-element group shares ky (the row test and the row's byte offset are computed once
// per group) and each element adds its own kx (x test, 4 kx bytes) and channel (soffset). The
// front end runs on each gathered value: `pre` times v * 2 - 1, then v - shift[ci]; the
// ScalingLayer's division is folded into the packed weights (w / scale[ci], lpips.cpp), and an
// out-of-image tap is 0 after it, as torch pads the scaled input.
template <int KS, int BM, bool STEM = false>
__global__ __launch_bounds__(256) void conv2d_x3_kernel(C2Args a) {
  constexpr int WAVES_M = BM >= 64 ? 2 : 1;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int TM = BM / (32 * WAVES_M);
  constexpr int TN = BN / (32 * WAVES_N);
  constexpr int KK = KS * KS;
  constexpr int M32 = BM / 32;
  constexpr int AH = 2 * M32 * 2 * 512;  // halves per A tile (2 steps, hi + lo)
  constexpr int BH = 2 * 2 * BN * 16;    // halves per B tile ([hl][step][n][16])
  constexpr int APASS = AH / 2048;       // 16-B chunks of 256 threads per A tile

  extern __shared__ __attribute__((aligned(16))) _Float16 smc[];
  _Float16* As0 = smc;
  _Float16* As1 = smc + AH;
  _Float16* Bs0 = smc + 2 * AH;
  _Float16* Bs1 = Bs0 + BH;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int h = lane >> 5, lc = lane & 31;
  // XCD-contiguous column-tile order (conv_gemm_x3.hip)
  const long nb = (gridDim.x & 7) ? (long)blockIdx.x : (long)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3));
  const long n0 = nb * BN;
  const int mt = blockIdx.y;
  const _Float16* wbase = a.w + (long)mt * a.nkt * AH;

  // ---- per-thread gather column (B operand): column col, k groups kg and kg + 2 ----
  const int col = tid & (BN - 1);
  const int kg = tid >> 7;  // 0/1, uniform per wave
  const long n = n0 + col;
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

  float breg[2][8];
  u32x4 areg[APASS];
  int bad = 0;

  auto load_tile = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
      const int kb = __builtin_amdgcn_readfirstlane(kt * BK + 8 * (kg + 2 * g2));
      if constexpr (STEM) {
        const int ky = kb / 40, j0 = kb - ky * 40;
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
          breg[g2][e] = ok ? v : 0.f;
        }
        continue;
      }
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
        breg[g2][e] = ok ? v : 0.f;
      }
    }
    const u32x4* ap = reinterpret_cast<const u32x4*>(wbase + (long)kt * AH);
#pragma unroll
    for (int p = 0; p < APASS; ++p) areg[p] = ap[p * 256 + tid];
  };
  auto store_tile = [&](_Float16* As, _Float16* Bs) __attribute__((always_inline)) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
      const int g = kg + 2 * g2;  // 8-k group: step g >> 1, half g & 1
      unsigned hw[4], lw[4];
      float am = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        split2s(breg[g2][2 * e], breg[g2][2 * e + 1], hw[e], lw[e]);
        amax2(am, breg[g2][2 * e], breg[g2][2 * e + 1]);
      }
      bad |= am >= 65504.f;
      const h8 hi = __builtin_bit_cast(h8, u32x4{hw[0], hw[1], hw[2], hw[3]});
      const h8 lo = __builtin_bit_cast(h8, u32x4{lw[0], lw[1], lw[2], lw[3]});
      _Float16* d = Bs + ((g >> 1) * BN + col) * 16 + 8 * ((g & 1) ^ ((col >> 3) & 1));
      *reinterpret_cast<h8*>(d) = hi;
      *reinterpret_cast<h8*>(d + 2 * BN * 16) = lo;
    }
    u32x4* ad = reinterpret_cast<u32x4*>(As);
#pragma unroll
    for (int p = 0; p < APASS; ++p) ad[p * 256 + tid] = areg[p];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  load_tile(0);
  store_tile(As0, Bs0);
  __syncthreads();
  for (int kt = 0; kt < a.nkt; ++kt) {
    const _Float16* As = (kt & 1) ? As1 : As0;
    const _Float16* Bs = (kt & 1) ? Bs1 : Bs0;
    // unconditional prefetch (the last tile re-loads itself into the idle buffer), as in
    // conv_gemm_x3_kernel
    load_tile(kt + 1 < a.nkt ? kt + 1 : kt);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      h8 ah[TM], al[TM], ad[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const _Float16* p = As + ((s * M32 + wm * TM + i) * 2) * 512 + lane * 8;
        ah[i] = *reinterpret_cast<const h8*>(p);
        al[i] = *reinterpret_cast<const h8*>(p + 512);
        ad[i] = lo_dn(ah[i]);  // pairs with the scaled B lo (split2s, kernels.h)
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int nc = (wn * TN + j) * 32 + lc;
        const _Float16* p = Bs + (s * BN + nc) * 16 + 8 * (h ^ ((nc >> 3) & 1));
        bh[j] = *reinterpret_cast<const h8*>(p);
        bl[j] = *reinterpret_cast<const h8*>(p + 2 * BN * 16);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ad[i], bl[j], acc[i][j], 0, 0, 0);
        }
    }
    store_tile((kt & 1) ? As0 : As1, (kt & 1) ? Bs0 : Bs1);
    __syncthreads();
  }
  if (bad) atomicOr(a.range, 1);

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
        const float v = acc[i][j][r] * a.wscale[m] + a.bias[m];
        a.out[obase + (long)m * hw] = v > 0.f ? v : 0.f;
      }
    }
  }
}

template <int KS, int BM, bool STEM = false>
void launch_c2(hipStream_t s, const C2Args& a, dim3 grid) {
  constexpr int AH = 2 * (BM / 32) * 2 * 512, BH = 2 * 2 * BN * 16;
  const size_t lds = (size_t)2 * (AH + BH) * sizeof(_Float16);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_x3_kernel<KS, BM, STEM>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((conv2d_x3_kernel<KS, BM, STEM>), grid, dim3(256), lds, s, a);
}

// One output element per thread; every window lies inside the plane (no padding, floor), so the
// nine loads are unconditional.
__global__ __launch_bounds__(256) void maxpool2d_32_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           int H, int W, int Ho, int Wo, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % Wo);
  const long r = idx / Wo;
  const int oy = (int)(r % Ho);
  const long plane = r / Ho;
  const float* p = in + plane * ((long)H * W) + (long)(2 * oy) * W + 2 * ox;
  float m = p[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, p[dy * W + dx]);
  out[idx] = m;
}

// One thread per (pair, pixel). The squared channel norms as four interleaved partial sums over c
// (c % 4), combined as (s0 + s1) + (s2 + s3); the weighted squared differences the same way: a
// fixed order, so a pair's value does not depend on its batch or slot. f / (norm + 1e-10) as an
// IEEE division on both sides (a reciprocal's rounding would scale a whole pixel's f^ coherently,
// and the difference of two near-equal f^ amplifies that) and no contraction: d(x, x) is exactly 0
// and d(a, b) == d(b, a) bitwise. C % 4 == 0.
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ f0, long set_off,
                                                         const float* __restrict__ w, float* __restrict__ lin, int C,
                                                         int hw, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long n = idx / hw;
  const int p = (int)(idx - n * hw);
  const float* a = f0 + n * C * (long)hw + p;
  const float* b = a + set_off;
  float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; c += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float va = a[(long)(c + q) * hw], vb = b[(long)(c + q) * hw];
      sa[q] += va * va;
      sb[q] += vb * vb;
    }
  }
  const float na = sqrtf((sa[0] + sa[1]) + (sa[2] + sa[3])) + 1e-10f;
  const float nb = sqrtf((sb[0] + sb[1]) + (sb[2] + sb[3])) + 1e-10f;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; c += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float d = a[(long)(c + q) * hw] / na - b[(long)(c + q) * hw] / nb;
      t[q] += w[c + q] * (d * d);
    }
  }
  lin[idx] = (t[0] + t[1]) + (t[2] + t[3]);
}

// One thread per pair: the 5 small lin maps against their separable fp64 weights, k, i, j ascending
__global__ __launch_bounds__(256) void lpips_mean_kernel(LpipsTaps t, float* __restrict__ mean_out, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int h = t.h[k], w = t.w[k];
    const float* m = t.lin[k] + (long)n * h * w;
    const double* wy = t.wy[k];
    const double* wx = t.wx[k];
    for (int i = 0; i < h; ++i) {
      double row = 0.0;
      for (int j = 0; j < w; ++j) row += wx[j] * (double)m[i * w + j];
      tot += wy[i] * row;
    }
  }
  mean_out[n] = (float)tot;
}

// torch upsample_bilinear2d, align_corners=False, scale = in / out (the arithmetic of
// fvd_preprocess_kernel, i3d.hip lin_idx3)
__device__ __forceinline__ void lin_idx2(int o, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

__global__ __launch_bounds__(256) void lpips_map_kernel(LpipsTaps t, float* __restrict__ map_out, int H, int W,
                                                        long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W);
  const long r = idx / W;
  const int y = (int)(r % H);
  const long n = r / H;
  float val = 0.f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int h = t.h[k], w = t.w[k];
    const float* p = t.lin[k] + n * h * w;
    int ya, yb, xa, xb;
    float ly0, ly1, lx0, lx1;
    lin_idx2(y, h, H, ya, yb, ly0, ly1);
    lin_idx2(x, w, W, xa, xb, lx0, lx1);
    const float v = ly0 * (lx0 * p[ya * w + xa] + lx1 * p[ya * w + xb]) +
                    ly1 * (lx0 * p[yb * w + xa] + lx1 * p[yb * w + xb]);
    val = k == 0 ? v : val + v;
  }
  map_out[idx] = val;
}

unsigned nblk256(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

bool conv2d_x3_forward(hipStream_t s, const float* in, long ib, long ic, int B, int Hi, int Wi, const Conv2dW& w,
                       const LpipsFront* front, float* out, int* range) {
  if (!w.w || !w.bias || (w.stem != (front != nullptr))) return false;
  C2Args a{};
  a.in = in; a.ib = ib; a.ic = ic;
  a.Cin = w.Cin; a.Cpad = w.Cpad; a.Hi = Hi; a.Wi = Wi;
  a.w = reinterpret_cast<const _Float16*>(w.w); a.wscale = w.wscale; a.nkt = w.nkt;
  a.bias = w.bias;
  a.out = out;
  a.Cout = w.M;
  a.Ho = conv2d_out(Hi, w.KS, w.stride, w.pad); a.Wo = conv2d_out(Wi, w.KS, w.stride, w.pad);
  a.stride = w.stride; a.pad = w.pad;
  if (front) { a.pre = front->pre; a.sh0 = front->shift[0]; a.sh1 = front->shift[1]; a.sh2 = front->shift[2]; }
  if (B <= 0 || a.Ho <= 0 || a.Wo <= 0) return false;
  a.N = (long)B * a.Ho * a.Wo;
  a.range = range;
  // a pixel's byte offset from its channel plane (the batch base included) plus the soffset of
  // channel 7 of a group stay below 2^32; the soffset itself below 2^31
  const long e0 = ((long)(B - 1) * ib + (long)Hi * Wi) * 4, c7 = 7 * 4 * ic;
  if (ib < 0 || ic < 0 || e0 + c7 >= (1L << 32) - 1 || c7 >= (1L << 31)) return false;
  const long ntile = (a.N + BN - 1) / BN;
  if (ntile > 0x7fffffffL) return false;
  const dim3 grid((unsigned)ntile, (unsigned)((w.M + w.bm - 1) / w.bm), 1);
  if (w.stem) {
    if (w.KS != 11 || w.Cin != 3 || w.bm != 64 || w.stride != 4) return false;
    launch_c2<11, 64, true>(s, a, grid);
    return true;
  }
  if (w.Cin % 8 != 0 || w.Cpad != w.Cin || w.stride != 1) return false;
  if (w.KS == 5 && w.bm == 128) launch_c2<5, 128>(s, a, grid);
  else if (w.KS == 3 && w.bm == 128) launch_c2<3, 128>(s, a, grid);
  else return false;
  return true;
}

void maxpool2d_32(hipStream_t s, const float* in, float* out, long planes, int H, int W) {
  const int Ho = pool32_out(H), Wo = pool32_out(W);
  const long total = planes * Ho * Wo;
  if (total <= 0) return;
  hipLaunchKernelGGL(maxpool2d_32_kernel, dim3(nblk256(total)), dim3(256), 0, s, in, out, H, W, Ho, Wo, total);
}

void lpips_head(hipStream_t s, const float* f0, long set_off, const float* w, float* lin, int N, int C, int hw) {
  const long total = (long)N * hw;
  hipLaunchKernelGGL(lpips_head_kernel, dim3(nblk256(total)), dim3(256), 0, s, f0, set_off, w, lin, C, hw, total);
}

void lpips_mean(hipStream_t s, const LpipsTaps& t, float* mean_out, int N) {
  hipLaunchKernelGGL(lpips_mean_kernel, dim3(nblk256(N)), dim3(256), 0, s, t, mean_out, N);
}

void lpips_map(hipStream_t s, const LpipsTaps& t, float* map_out, int N, int H, int W) {
  const long total = (long)N * H * W;
  hipLaunchKernelGGL(lpips_map_kernel, dim3(nblk256(total)), dim3(256), 0, s, t, map_out, H, W, total);
}

}  // namespace extdm
