// InceptionI3d (metrics/pytorch_i3d.py), the feature network of FVD: true 3-D convolution as an
// f16x3 implicit GEMM, the 'same'-padded 3-D max pools, the avg-pool / logits head and the
// trans + preprocess_single front end.
//
// conv3d_x3_kernel is the 3-D member of the conv_gemm_x3.hip family and shares its arithmetic
// (fp32 storage, hi / lo fp16 split while staging, three v_mfma_f32_32x32x16_f16 products into
// fp32 accumulators, A rows pre-scaled by powers of two, the sticky |v| >= 65504 flag):
//   C[m][n] = sum_k A[m][k] B[k][n],  m = output channel, n = (b, to, oy, ox),
//   k = ((kt * KS + ky) * KS + kx) * Cpad + ci   (tap-major, Cpad = Cin rounded up to 8).
// Block tile BM x 128 x 32, 256 threads = 4 waves, LDS double buffer with a register prefetch of
// the next K tile; A packed per (mtile, ktile) as [step][m32][hi|lo][lane][8]. The gather is the
// TAPK scheme: a thread's 8-element group is 8 channels of one tap, so the tap, the in-volume
// test in three dimensions and the voxel's byte offset are computed once per group, and the
// channel volumes are wave-uniform bases (buffer loads: voxel offset in voffset, the channel in
// soffset). Out-of-volume taps read 0; channels past Cin (the stem's 3 of 8) are not loaded.
// The 'same' pads (pytorch_i3d.py:71-95) come from the host as front offsets per dimension.
#include "i3d.h"
#include "kernels.h"

namespace extdm {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int BN = 128;
constexpr int BK = 32;

struct C3Args {
  const float* in; long ib, ic;
  int Cin, Cpad, Ti, Hi, Wi;
  const _Float16* w; const float* wscale; int nkt;
  float* out; long ob, oc, ot;
  int Cout, To, Ho, Wo;
  int stride, pt, ph, pw;  // front pads
  const float* post_scale; const float* post_shift; int relu;
  long N;
  int* range;
};

// STEM (the 3 -> 64 7x7x7 stride-2 unit, K = 1029): padding 3 channels to 8 per tap would make
// K = 2744. Instead a (kt, ky) row of taps is the unit: its 21 (kx, ci) elements padded to 24,
//   k = (kt * 7 + ky) * 24 + kx * 3 + ci,   K = 1176 (+14 %),
// so a thread's 8-element group shares kt and ky (the in-volume test in t and y and the row's byte
// offset are computed once per group) and each element adds its own kx (x test, 4 kx bytes) and
// channel (soffset).
template <int KS, int BM, bool STEM = false>
__global__ __launch_bounds__(256) void conv3d_x3_kernel(C3Args a) {
  constexpr int WAVES_M = BM >= 64 ? 2 : 1;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int TM = BM / (32 * WAVES_M);
  constexpr int TN = BN / (32 * WAVES_N);
  constexpr int KK = KS * KS * KS;
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
  // XCD-contiguous column-tile order (conv_gemm_x3.hip): XCD k takes a contiguous range of
  // column tiles, so the voxels neighbouring tiles both gather come from its L2
  const long nb = (gridDim.x & 7) ? (long)blockIdx.x : (long)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3));
  const long n0 = nb * BN;
  const int mt = blockIdx.y;
  const _Float16* wbase = a.w + (long)mt * a.nkt * AH;

  // ---- per-thread gather column (B operand): column col, k groups kg and kg + 2 ----
  const int col = tid & (BN - 1);
  const int kg = tid >> 7;  // 0/1, uniform per wave
  const long n = n0 + col;
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

  float breg[2][8];
  u32x4 areg[APASS];
  int bad = 0;

  auto load_tile = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
      const int kb = __builtin_amdgcn_readfirstlane(kt * BK + 8 * (kg + 2 * g2));
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
          breg[g2][e] = ok ? v : 0.f;
        }
        continue;
      }
      const int tap = kb / a.Cpad, ci0 = kb - tap * a.Cpad;
      const int kt_ = tap / (KS * KS), r = tap - kt_ * (KS * KS);
      const int ky = r / KS, kx = r - ky * KS;
      const int it = it0 + kt_, iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = nvalid && tap < KK && it >= 0 && it < a.Ti && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
      const unsigned vo = ok ? (unsigned)((base + ((long)it * a.Hi + iy) * a.Wi + ix) * 4) : 0u;
      const int cb = tap < KK ? ci0 : 0;
      // the group's first channel volume as the (uniform) buffer base: voxel offset in voffset,
      // channel e's volume offset in soffset
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
        float v = acc[i][j][r] * a.wscale[m];
        if (a.post_scale) v = v * a.post_scale[m] + a.post_shift[m];
        if (a.relu) v = v > 0.f ? v : 0.f;
        a.out[obase + (long)m * a.oc] = v;
      }
    }
  }
}

template <int KS, int BM, bool STEM = false>
void launch_c3(hipStream_t s, const C3Args& a, dim3 grid) {
  constexpr int AH = 2 * (BM / 32) * 2 * 512, BH = 2 * 2 * BN * 16;
  const size_t lds = (size_t)2 * (AH + BH) * sizeof(_Float16);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3d_x3_kernel<KS, BM, STEM>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((conv3d_x3_kernel<KS, BM, STEM>), grid, dim3(256), lds, s, a);
}

template <int KS>
bool launch_c3_bm(hipStream_t s, const C3Args& a, int bm, dim3 grid) {
  if (bm == 128) launch_c3<KS, 128>(s, a, grid);
  else if (bm == 64) launch_c3<KS, 64>(s, a, grid);
  else if (bm == 32) launch_c3<KS, 32>(s, a, grid);
  else return false;
  return true;
}

// One output element per thread; the window's taps outside the volume are the reference's zero
// padding and take part in the max as 0 (pytorch_i3d.py:33-34 pads, then pools).
// The window is a template constant (the network has three: [1,3,3], [3,3,3], [2,2,2]), so the tap
// loops unroll and the (clamped, unconditional) loads of a window issue together: with run-time
// loops and a load under each tap's test the pools took 1.8x as long.
template <int KT, int KH, int KW>
__global__ __launch_bounds__(256) void maxpool3d_same_kernel(const float* __restrict__ in, long ib, long ic,
                                                             float* __restrict__ out, int C, int Ti, int Hi, int Wi,
                                                             int To, int Ho, int Wo, int st, int sh, int sw, int pt,
                                                             int ph, int pw) {
  // grid: x over the output plane, y = (c, to), z = b -- 32-bit index math only
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= Ho * Wo) return;
  const int oy = pix / Wo, ox = pix - oy * Wo;
  const int c = blockIdx.y / To, to = blockIdx.y - c * To;
  const int b = blockIdx.z;
  const float* p = in + (long)b * ib + (long)c * ic;
  constexpr int kt = KT, kh = KH, kw = KW;
  float m = -INFINITY;
#pragma unroll
  for (int dt = 0; dt < kt; ++dt) {
    const int t = to * st - pt + dt;
    const bool okt = t >= 0 && t < Ti;
    const int tc = min(max(t, 0), Ti - 1);
#pragma unroll
    for (int dy = 0; dy < kh; ++dy) {
      const int y = oy * sh - ph + dy;
      const bool oky = okt && y >= 0 && y < Hi;
      const float* row = p + ((long)tc * Hi + min(max(y, 0), Hi - 1)) * Wi;
#pragma unroll
      for (int dx = 0; dx < kw; ++dx) {
        const int x = ox * sw - pw + dx;
        const bool ok = oky && x >= 0 && x < Wi;
        const float v = row[min(max(x, 0), Wi - 1)];  // always in the volume
        m = fmaxf(m, ok ? v : 0.f);
      }
    }
  }
  out[(((long)b * C + c) * To + to) * ((long)Ho * Wo) + pix] = m;
}

// One wave per (n, c, s): the 98 values of frames s, s + 1 are contiguous; lane l sums elements
// l and l + 64, then a fixed-order butterfly (the same order for every sample).
__global__ __launch_bounds__(256) void i3d_avgpool_kernel(const float* __restrict__ x, float* __restrict__ pooled,
                                                          int T, long total) {
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= total) return;
  const int lane = threadIdx.x & 63;
  const int S = T - 1;
  const long nc = w / S;
  const int s = (int)(w - nc * S);
  const float* p = x + (nc * T + s) * 49;
  float v = p[lane];
  if (lane + 64 < 98) v += p[lane + 64];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) pooled[w] = v / 98.f;
}

// One thread per (sample, class): per time slot the 1024-term dot product in a fixed order (four
// interleaved partial sums), + bias, then the mean over the slots. No atomics: a sample's logits
// do not depend on the batch.
__global__ __launch_bounds__(256) void i3d_logits_kernel(const float* __restrict__ pooled,
                                                         const float* __restrict__ wt,
                                                         const float* __restrict__ bias, float* __restrict__ logits,
                                                         int C, int S, int K) {
  extern __shared__ float ps[];  // [C] of the current slot
  const int n = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  float tot = 0.f;
  for (int s = 0; s < S; ++s) {
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) ps[c] = pooled[((long)n * C + c) * S + s];
    __syncthreads();
    if (k < K) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int c = 0;
      for (; c + 3 < C; c += 4) {
        a0 += wt[(long)c * K + k] * ps[c];
        a1 += wt[(long)(c + 1) * K + k] * ps[c + 1];
        a2 += wt[(long)(c + 2) * K + k] * ps[c + 2];
        a3 += wt[(long)(c + 3) * K + k] * ps[c + 3];
      }
      for (; c < C; ++c) a0 += wt[(long)c * K + k] * ps[c];
      tot += ((a0 + a1) + (a2 + a3)) + bias[k];
    }
  }
  if (k < K) logits[(long)n * K + k] = tot / (float)S;
}

// torch upsample_bilinear2d, align_corners=False, scale = in / out (the arithmetic of
// extdm_bilinear_frames, norm.hip lin_idx)
__device__ __forceinline__ void lin_idx3(int o, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

__global__ __launch_bounds__(256) void fvd_preprocess_kernel(const float* __restrict__ in, long sb, long st, long sc,
                                                             int C, int To, int H, int W, int Hr, int Wr, int y0,
                                                             int x0, int R, float* __restrict__ out, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % R);
  long r = idx / R;
  const int y = (int)(r % R); r /= R;
  const int t = (int)(r % To); r /= To;
  const int c = (int)(r % 3);
  const int b = (int)(r / 3);
  const float* p = in + (long)b * sb + (long)t * st + (long)(C == 1 ? 0 : c) * sc;
  int ya, yb, xa, xb;
  float ly0, ly1, lx0, lx1;
  lin_idx3(y + y0, H, Hr, ya, yb, ly0, ly1);
  lin_idx3(x + x0, W, Wr, xa, xb, lx0, lx1);
  const float v = ly0 * (lx0 * p[ya * W + xa] + lx1 * p[ya * W + xb]) +
                  ly1 * (lx0 * p[yb * W + xa] + lx1 * p[yb * W + xb]);
  out[idx] = (v - 0.5f) * 2.f;
}

unsigned nblk256(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

bool conv3d_x3_forward(hipStream_t s, const Vol& in, const Conv3dW& w, int stride, float* out, long ob, long oc,
                       long ot, const float* post_scale, const float* post_shift, bool relu, int* range) {
  if (!w.w || in.C != w.Cin || (stride != 1 && stride != 2)) return false;
  C3Args a{};
  a.in = in.p; a.ib = in.sb; a.ic = in.sc;
  a.Cin = w.Cin; a.Cpad = w.Cpad; a.Ti = in.T; a.Hi = in.H; a.Wi = in.W;
  a.w = reinterpret_cast<const _Float16*>(w.w); a.wscale = w.wscale; a.nkt = w.nkt;
  a.out = out; a.ob = ob; a.oc = oc; a.ot = ot;
  a.Cout = w.M;
  a.To = same_out(in.T, stride); a.Ho = same_out(in.H, stride); a.Wo = same_out(in.W, stride);
  a.stride = stride;
  a.pt = same_pad(in.T, w.KS, stride) / 2;
  a.ph = same_pad(in.H, w.KS, stride) / 2;
  a.pw = same_pad(in.W, w.KS, stride) / 2;
  a.post_scale = post_scale; a.post_shift = post_shift; a.relu = relu ? 1 : 0;
  a.N = (long)in.B * a.To * a.Ho * a.Wo;
  a.range = range;
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
  if (w.KS == 1) return launch_c3_bm<1>(s, a, w.bm, grid);
  if (w.KS == 3) return launch_c3_bm<3>(s, a, w.bm, grid);
  if (w.KS == 7) return launch_c3_bm<7>(s, a, w.bm, grid);
  return false;
}

bool maxpool3d_same(hipStream_t s, const Vol& in, float* out, int kt, int kh, int kw, int st, int sh, int sw) {
  const int To = same_out(in.T, st), Ho = same_out(in.H, sh), Wo = same_out(in.W, sw);
  if ((long)in.C * To > 65535 || in.B > 65535 || (long)Ho * Wo > 0x7fffffffL) return false;
  const dim3 grid(nblk256((long)Ho * Wo), (unsigned)(in.C * To), (unsigned)in.B);
  const int pt = same_pad(in.T, kt, st) / 2, ph = same_pad(in.H, kh, sh) / 2, pw = same_pad(in.W, kw, sw) / 2;
#define EXTDM_POOL(KT, KH, KW)                                                                                     \
  hipLaunchKernelGGL((maxpool3d_same_kernel<KT, KH, KW>), grid, dim3(256), 0, s, in.p, in.sb, in.sc, out, in.C, in.T, \
                     in.H, in.W, To, Ho, Wo, st, sh, sw, pt, ph, pw)
  bool done = true;
  if (kt == 1 && kh == 3 && kw == 3) EXTDM_POOL(1, 3, 3);
  else if (kt == 3 && kh == 3 && kw == 3) EXTDM_POOL(3, 3, 3);
  else if (kt == 2 && kh == 2 && kw == 2) EXTDM_POOL(2, 2, 2);
  else done = false;
#undef EXTDM_POOL
  return done;
}

void i3d_avgpool(hipStream_t s, const float* x, float* pooled, int N, int C, int T) {
  const long total = (long)N * C * (T - 1);
  hipLaunchKernelGGL(i3d_avgpool_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, x, pooled, T, total);
}

void i3d_logits(hipStream_t s, const float* pooled, const float* wt, const float* bias, float* logits, int N, int C,
                int S, int K) {
  hipLaunchKernelGGL(i3d_logits_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)N), dim3(256),
                     (size_t)C * sizeof(float), s, pooled, wt, bias, logits, C, S, K);
}

void fvd_preprocess(hipStream_t s, const float* in, long sb, long st, long sc, int B, int C, int To, int H, int W,
                    int Hr, int Wr, int y0, int x0, int R, float* out) {
  const long total = (long)B * 3 * To * R * R;
  hipLaunchKernelGGL(fvd_preprocess_kernel, dim3(nblk256(total)), dim3(256), 0, s, in, sb, st, sc, C, To, H, W, Hr, Wr,
                     y0, x0, R, out, total);
}

}  // namespace extdm
