// Weight layouts of the MFMA / VALU kernels as pure host functions (no HIP, no kernels.h): host
// vectors and the tile parameters the kernel files choose in, host vectors out. runtime.cpp,
// fvd.cpp and lpips.cpp upload the results; tests/pack_driver.cpp, tests/pack_lpips_driver.cpp,
// tests/pack_updown_driver.cpp, tests/pack_f32_driver.cpp and tests/pack_lpips_f32_driver.cpp run
// the same functions on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace extdm {

using half_t = _Float16;
using fvec = std::vector<float>;

// e with mx * 2^e in [2^14, 2^15), 0 for mx == 0 (float and double); rs = 2^-e
template <class T>
int pow2_row_exp(T mx, float& rs);
// the f16x3 split of v: dst[0] = hi = fp16(v), dst[512] = lo = fp16(v - hi) (the [hi|lo][lane][8]
// pair of 512-half fragments every layout below ends in)
void put_hilo(half_t* dst, float v);

// The generic fragment layout [par][mtile][ktile][step][m32][hi|lo][lane][8], row m = mtile*BM +
// m32*32 + (lane & 31), k = ktile*32 + step*16 + 8*(lane >> 5) + e. elem(par, m, k, v) gives
// element (m, k) of parity par, or false where the layout has none (stays zero). Row m is scaled
// by 2^s(m) over all parities (max |w| -> [2^14, 2^15)), undone by rs[m] = 2^-s(m).
struct Frags {
  std::vector<half_t> g;
  fvec rs;    // [M]
  int n = 0;  // k-tiles (pack_frags, pack_gemm_x3, pack_unit3d) / channel blocks ncgb (pack_x3)
  std::vector<half_t> tap_major;  // pack_gemm_x3 only
};
template <class F>
Frags pack_frags(int npar, int M, int K, int bm, F&& elem) {
  const int nkt = (K + 31) / 32, mt = (M + bm - 1) / bm, m32 = bm / 32;
  const size_t ah = (size_t)2 * m32 * 2 * 512;
  Frags r{std::vector<half_t>((size_t)npar * mt * nkt * ah), fvec(M), nkt};
  fvec scale(M);
  for (int m = 0; m < M; ++m) {
    float mx = 0.f, v;
    for (int par = 0; par < npar; ++par)
      for (int k = 0; k < K; ++k)
        if (elem(par, m, k, v)) mx = std::max(mx, std::fabs(v));
    scale[m] = std::ldexp(1.f, pow2_row_exp(mx, r.rs[m]));
  }
  for (int par = 0; par < npar; ++par)
    for (int mtile = 0; mtile < mt; ++mtile)
      for (int kt = 0; kt < nkt; ++kt)
        for (int st = 0; st < 2; ++st)
          for (int q = 0; q < m32; ++q)
            for (int l = 0; l < 64; ++l)
              for (int e = 0; e < 8; ++e) {
                const int m = mtile * bm + q * 32 + (l & 31), k = kt * 32 + st * 16 + 8 * (l >> 5) + e;
                float v;
                if (m >= M || k >= K || !elem(par, m, k, v)) continue;
                const size_t base = (((size_t)par * mt + mtile) * nkt + kt) * ah + (size_t)((st * m32 + q) * 2) * 512;
                put_hilo(&r.g[base + l * 8 + e], v * scale[m]);
              }
  return r;
}

// fp32 GEMM plane of a conv weight W[M][K] (K = ci*kh*kw + ky*kw + kx) or linear: A[k][m],
// zero padded to [Kpad][Mpad], Mpad = M up to bm, Kpad = K up to 16
struct GemmPlane { fvec a; int Mpad = 0, Kpad = 0; };
GemmPlane pack_gemm_plane(const fvec& w, int M, int K, int bm);
// ConvTranspose3d(1,4,4)/s2/p1 weight W[ci][co][1][4][4] -> four 2x2 parity GEMM planes
// [4][Kpad][Mpad], K = ci*4: parity (py,px) tap (ky',kx') uses W[..][3-py-2ky'][3-px-2kx'].
GemmPlane pack_deconv_planes(const fvec& w, int ci, int co, int bm);
// f16x3 implicit-GEMM layout (conv_gemm_x3.hip) from the fp32 planes [npar][Kpad][Mpad]: pack_frags
// in ci-major k order and, for npar == 1, kk > 1, 32 % kk != 0 and ci % 8 == 0, its tap-major copy
// (k = tap * ci + c reads row c * kk + tap; tap_major empty otherwise)
Frags pack_gemm_x3(const GemmPlane& p, int npar, int M, int K, int bm, int kk);
// Unit3D weight [M][Cin][KS]^3 for conv3d_x3_kernel: pack_frags with k = tap * Cpad + ci (channels
// past Cin absent). stem_row > 0: the 3-channel stem's (kt, ky) rows of 7 kx * 3 ci = 21 elements
// padded to stem_row, K = KS*KS*stem_row (i3d.hip STEM)
Frags pack_unit3d(const fvec& w, int M, int Cin, int Cpad, int KS, int bm, int stem_row);
// Conv2d weight [M][Cin][KS][KS] for conv2d_x3_kernel (lpips.hip): pack_frags with k = (ky * KS +
// kx) * Cpad + ci (channels past Cin absent). stem_row > 0: the 3-channel stem's ky rows of
// KS kx * Cin ci elements (j = kx * Cin + ci) padded to stem_row, k = ky * stem_row + j,
// K = KS * stem_row (AlexNet's 11x11: 33 of 40, K = 440)
Frags pack_conv2d(const fvec& w, int M, int Cin, int Cpad, int KS, int bm, int stem_row);
// fp32 tile layout of the exact-fp32 convolutions (f32_tiles.h: i3d_f32.hip, lpips_f32.hip):
// a[((mtile * nkt + ktile) * 32 + r) * bm + c] = element (row m = mtile*bm + c, k = ktile*32 + r) of
// the dense [M][K] matrix, nkt = ceil(K / 32), ceil(M / bm) m-tiles; 0 for m >= M, k >= K and where
// the matrix has no element (pad channels, the stem rows' pad columns). No scaling.
struct TilesF32 { fvec a; int nkt = 0; };
// Unit3D weight [M][Cin][KS]^3 for conv3d_f32_kernel: k = tap * Cpad + ci, tap = (kt*KS + ky)*KS + kx
// (channels ci >= Cin zero), K = KS^3 * Cpad
TilesF32 pack_conv3d_f32(const fvec& w, int M, int Cin, int Cpad, int KS, int bm);
// its stem variant: (kt, ky) rows of KS kx * Cin ci elements (j = kx * Cin + ci) padded to stem_row,
// k = (kt*KS + ky) * stem_row + j, K = KS*KS*stem_row (the 3-channel 7x7x7 unit: 21 of 24, K = 1176)
TilesF32 pack_conv3d_f32_stem(const fvec& w, int M, int Cin, int KS, int bm, int stem_row);
// Conv2d weight [M][Cin][KS][KS] for conv2d_f32_kernel (lpips_f32.hip): k = tap * Cpad + ci,
// tap = ky*KS + kx (channels ci >= Cin zero), K = KS^2 * Cpad; element (m, k) = w[m][ci][ky][kx]
TilesF32 pack_conv2d_f32(const fvec& w, int M, int Cin, int Cpad, int KS, int bm);
// its stem variant: ky rows of KS kx * Cin ci elements (j = kx * Cin + ci) padded to stem_row,
// k = ky * stem_row + j, K = KS * stem_row; element (m, k) = w[m][j % Cin][ky][j / Cin] for
// j < KS * Cin, zero for the pad columns (AlexNet's 3-channel 11x11: 33 of 40, K = 440)
TilesF32 pack_conv2d_f32_stem(const fvec& w, int M, int Cin, int KS, int bm, int stem_row);
// f16x3 layout (conv_x3.hip): [mtile][cb*KS + ky][(g, kx)][m32][hi|lo][lane][8], lane = (h, lc): row
// m = mtile*BM + m32*32 + lc, input channel cb*16NG + g*16 + 8h + e. Rows scaled as in pack_frags.
Frags pack_x3(const fvec& w, int ks, int co, int ci, int bm, int ng);
// Two-tap f16x3 layouts (conv_x3.hip, TT mode): the stride-2 (1,4,4)/p1 convs as sums of 2x2-tap
// stride-1 convs over a 3x3-style halo tile, [mtile][cblk][ky'][kx'][m32][hi|lo][lane][8] with 16
// input channels per block (lane = (h, lc): channel 16*cb + 8h + e) and rows scaled by 2^s(co)
// over the whole 4x4 kernel, undone by rs[co]; Frags::n = channel blocks per m-tile.
// ConvTranspose W[ci][co][1][4][4]: mtile = ph*MTC + ct (ph = 2py + px the output phase, MTC =
// ceil(co / bm)), row co = ct*bm + m32*32 + lc, cblk = cb < ci/16; element
// W[16cb + 8h + e][co][3 - py - 2ky'][3 - px - 2kx'] (the taps of pack_deconv_planes).
Frags pack_x3_deconv(const fvec& w, int ci, int co, int bm);
// Downsample W[co][ci][1][4][4]: mtile = ct, row co = ct*bm + m32*32 + lc, cblk = q*(ci/16) + cb
// (q = 2qy + qx the input phase plane in[2Y + qy][2X + qx]); element
// W[co][16cb + 8h + e][2ky' + 1 - qy][2kx' + 1 - qx].
Frags pack_x3_down(const fvec& w, int co, int ci, int bm);
// Direct-conv layout [mtile][stage][step][half][BM]: step = (cp*k + ky)*k + kx,
// input channel = stage*2CH + half*CH + cp (conv_halo.hip).
struct HaloPack { fvec a; int stages = 0; };
HaloPack pack_halo(const fvec& w, int ks, int co, int ci, int bm, int ch);
// fp32 direct VALU layout (conv_narrow.hip): [group][ci][tap][cot rounded up to 4], m = group * cot + o
fvec pack_narrow(const fvec& w, int kk, int co, int ci, int cot);
// Conv3d weight W[co][ci][kt][kk] as a (1,kh,kw) conv over kt*ci channels: W'[co][z*ci + c] = W[co][c][z]
fvec reorder_time3(const fvec& w, int co, int ci, int kt, int kk);
// input channels [lo, hi) of W[Co][Cin][kk]
fvec split_channels(const fvec& w, int Co, int Cin, int kk, int lo, int hi);
// A 1x1 conv behind a channel LayerNorm with the norm's gamma folded in: W'[co][ci] = W[co][ci] *
// gamma[ci], the product in double (exact) rounded once to fp32; the conv then reads (x - mean) *
// rinv (conv_x3.hip AFF = 2) and pack_x3 splits W' as any weight.
fvec fold_ln_gamma(const fvec& w, const fvec& gamma, int Co, int Cin);

// init_conv's x-branch composed with init_noise_conv (xpath_x3.hip): 49 border-class 13x13 kernels
// over the 3 latent channels, built in fp64, packed as f16x3 A fragments [class][kstep = (ci, dy)]
// [m32][hi|lo][lane][8] (row m = m32*32 + (lane & 31), column dx = 8*(lane >> 5) + e, zero for
// dx >= 13), rows scaled by 2^s(class, m); rs [49][MP] the inverse scales, cb [49][MP] the composed
// bias (MP = Co up to 32). wn [Cm][3][7][7], bn [Cm], wi [Co][Cin][7][7], bi [Co]; L the latent size.
struct XPathPack { std::vector<half_t> g; fvec rs, cb; };
XPathPack pack_xpath(const fvec& wn, const fvec& bn, const fvec& wi, const fvec& bi, int Cm, int Co, int Cin, int L);
// A 3 -> Cm (1,7,7) conv for noise_pool_x3_kernel and conv7c3_x3_kernel: A fragments [kstep = (ci,
// row pair)][m32][hi|lo][lane][8], k = 8*(lane >> 5) + e -> (dy = 2*pair + (lane >> 5), dx = e),
// zero for dy or dx = 7; rows scaled by 2^s(m).
Frags pack_conv7c3(const fvec& w, int Cm);
// init_conv's cond_fea branch over F at fea_size n instead of its bilinear x2 upsample
// (fea_x3.hip header, u12:1034-1041), composed in fp64 from wt [Co][Cf][7][7]: the 5x5 phase
// kernels k5 [4 Co][Cf][5][5] (row ph * Co + co, ph = 2 py + px), the f16x3 edge-line weights
// [pair][side] x [mtile][cb][tap][m32][hi|lo][lane][8] over rows m = co * 8 + (d*2 + py)*2 + px with
// their inverse scales [4][RP], and the fp32 corner weights [corner][ci][co][p = yy * 4 + xx].
struct FeaPhasePack { fvec k5, side_scale, corner; std::vector<half_t> side; };
FeaPhasePack pack_fea_phase(const fvec& wt, int Co, int Cf, int n);

// Packed weights of the fused attention kernels (stw_fused.hip header): nmat matrices of `rows`
// rows each, w [nmat * rows][K], as [rows / 32][K / 2][nmat][lane]: row 32 u + (lane & 31), column
// 2 s + (lane >> 5). qkv: nmat 3, rows hid (32-row units: one head of dim 32 / two of dim 16).
fvec pack_stw_rows(const fvec& w, int nmat, int rows, int K);
// f16x3 attention weights (stw_x3.hip): per unit u of 32 qkv rows (uh halves each), fragments
// of [hi|lo][lane][8] for q, k, v (row u*32 + lc, channels 16s + 8h + e) and the projection (row
// ct*32 + lc, hid u*32 + 16s' + 8(e>>2) + 4h + (e&3): the row order of the O^T accumulator). Each
// matrix is scaled by one power of two. sc: [q, k, v, proj factors, softmax exp2 factor] (stw_x3.hip
// kernel header); s2 = 2^(e_q + e_k), the factor of the scores (and of their bias / mask table).
// ng / nb: the affine of the norm whose output the kernel splits (MODE 0: the PreNorm gamma;
// MODE 1: the inner LayerNorm's weight and bias; nb null without a bias)
struct AttnX3Pack { std::vector<half_t> a; float sc[5] = {}, s2 = 1.f; };
AttnX3Pack pack_attn_x3(const fvec& wqkv, const fvec& wproj, const fvec& ng, const fvec* nb, int C, int hid, int uh,
                        float q_scale);

// Eval BatchNorm as a per-channel affine: alpha = w / sqrt(rv + eps), beta = b - rm * alpha,
// eps 1e-5. The LFAE decoder's in fp32 (rounded after every operation), InceptionI3d's in fp64.
struct Affine { fvec a, b; };
Affine bn_fold_f32(const fvec& w, const fvec& b, const fvec& rm, const fvec& rv);
Affine bn_fold_f64(const fvec& w, const fvec& b, const fvec& rm, const fvec& rv);

}  // namespace extdm
