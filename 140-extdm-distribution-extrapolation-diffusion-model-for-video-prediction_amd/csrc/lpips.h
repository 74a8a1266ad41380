// LPIPS (AlexNet, version 0.1) -- kernels of lpips.hip and lpips_f32.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace extdm {

// AlexNet `features` geometry: Conv2d(k, s, p) output extent and MaxPool2d(3, 2) (no padding, floor)
inline int conv2d_out(int size, int k, int stride, int pad) {
  return size + 2 * pad < k ? 0 : (size + 2 * pad - k) / stride + 1;
}
inline int pool32_out(int size) { return size < 3 ? 0 : (size - 3) / 2 + 1; }

// f16x3 packing of a Conv2d weight [M][Cin][KS][KS] (pack_conv2d): tap-major K, or the 3-channel
// 11x11 stem's ky-row layout (stem: k = ky * 40 + kx * 3 + ci, K = 440). The exact-fp32 route
// (lpips_f32.hip) describes its fp32 tiles (pack_conv2d_f32, the same k order) with the same
// struct: w the float tiles, wscale null.
struct Conv2dW {
  const void* w = nullptr;
  const float* wscale = nullptr;
  const float* bias = nullptr;
  int M = 0, Cin = 0, Cpad = 0, KS = 1, stride = 1, pad = 0, bm = 0, nkt = 0;
  bool stem = false;
};
constexpr int kLpipsStemRow = 40;  // 11 kx * 3 ci = 33 elements of a ky row, padded to five groups of 8
inline int conv2d_bm(int M) { return M >= 128 ? 128 : 64; }
// The exact-fp32 route's m-tile, for every Cout: the 128-row tile holds two accumulator sets
// (partial and total, 290 registers a lane) and runs one workgroup per CU; 64 rows run three, and
// 4096 pairs of 64 x 64 take 2.15 us per pair instead of 3.02 (Cout 192 is three full tiles).
constexpr int kLpipsF32Bm = 64;

// The stem's front end, applied while gathering: `pre` times v <- v * 2 - 1 (trans of
// calculate_lpips.py:15-23 and / or LPIPS.forward's normalize), then the ScalingLayer's v - shift[ci];
// its division by scale[ci] is folded into the packed stem weights (lpips.cpp). Taps outside the
// image contribute 0 (torch pads after scaling).
struct LpipsFront {
  int pre = 0;
  float shift[3] = {0.f, 0.f, 0.f};
};

// out [B][M][Ho][Wo] (contiguous) = relu(conv2d(in, w) + bias); in [B][Cin][Hi][Wi] through the
// batch / channel element strides ib / ic (planes contiguous; ic = 0 replicates a grey plane).
// front: non-null for the stem only. False if the launch is not covered (offsets past 32 bits).
bool conv2d_x3_forward(hipStream_t s, const float* in, long ib, long ic, int B, int Hi, int Wi, const Conv2dW& w,
                       const LpipsFront* front, float* out, int* range);

// The same convolution on the exact-fp32 route (lpips_f32.hip, v_mfma_f32_32x32x2_f32): w the fp32
// tiles of pack_conv2d_f32 / pack_conv2d_f32_stem (wscale null). No range flag.
bool conv2d_f32_forward(hipStream_t s, const float* in, long ib, long ic, int B, int Hi, int Wi, const Conv2dW& w,
                        const LpipsFront* front, float* out);

// MaxPool2d(3, 2), no padding, floor: contiguous [B * C][H][W] -> [B * C][(H-3)/2+1][(W-3)/2+1]
void maxpool2d_32(hipStream_t s, const float* in, float* out, long planes, int H, int W);

// lin[n][p] = sum_c w[c] (f0[n][c][p] / (|f0[n][:][p]| + 1e-10) - f1[n][c][p] / (|f1[n][:][p]| + 1e-10))^2
// with f1 = f0 + set_off; fixed summation order per (n, p)
void lpips_head(hipStream_t s, const float* f0, long set_off, const float* w, float* lin, int N, int C, int hw);

struct LpipsTaps {
  const float* lin[5];  // [N][h][w] per tap
  int h[5], w[5];
  const double* wy[5];  // separable mean weights per tap (extdm_lpips_mean_weights)
  const double* wx[5];
};
// mean_out[n] = sum_k sum_ij wy_k[i] wx_k[j] lin_k[n][i][j] in fp64, k, i, j ascending
void lpips_mean(hipStream_t s, const LpipsTaps& t, float* mean_out, int N);
// map_out[n][y][x] = sum_k bilinear(lin_k[n], H x W, align_corners=False)[y][x]
void lpips_map(hipStream_t s, const LpipsTaps& t, float* map_out, int N, int H, int W);

}  // namespace extdm
