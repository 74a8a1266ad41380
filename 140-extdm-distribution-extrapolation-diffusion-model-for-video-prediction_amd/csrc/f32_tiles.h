// The tile loop of the exact-fp32 convolutions (conv3d_f32_kernel in i3d_f32.hip, conv2d_f32_kernel
// in lpips_f32.hip): an implicit GEMM on v_mfma_f32_32x32x2_f32 whose B gather is the caller's.
//   C[m][n] = sum_k A[m][k] B[k][n]
// The products are exact fp32 and a column's K order is fixed: k ascending, two per MFMA, into a
// partial accumulator that is added to the total and cleared every KCHUNK K tiles (a two-level sum:
// the rounding error grows with 32 KCHUNK + K / (32 KCHUNK) terms instead of K, which is what a
// blocked fp32 convolution on a CPU or in a vendor library gets from its vector lanes). No
// hi / lo split, no row scaling, no range flag.
// Block tile BM x 128 x 32, 256 threads = 4 waves, LDS double buffer ([k][BM] and [k][128] floats)
// with a register prefetch of the next K tile; A packed per (mtile, ktile) as [k 32][BM] (TilesF32,
// pack.h).
#pragma once
#include <hip/hip_runtime.h>

namespace extdm {
namespace f32gemm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BN = 128;
constexpr int BK = 32;
constexpr int KCHUNK = 4;  // K tiles per partial sum

// The tile loop: gather(kb, v) fills the 8 B values of the thread's column
// for k = kb .. kb + 7 (kb wave-uniform). Leaves the accumulators of the wave's TM x TN 32x32
// tiles in acc.
template <int BM, int TM, int TN, class G>
__device__ __forceinline__ void f32_tiles(const float* __restrict__ wbase, int nkt, float* sm, G&& gather,
                                          f32x16 (&acc)[TM][TN]) {
  constexpr int WAVES_M = BM >= 64 ? 2 : 1;
  constexpr int WAVES_N = 4 / WAVES_M;
  static_assert(TM == BM / (32 * WAVES_M) && TN == BN / (32 * WAVES_N), "accumulator tile");
  constexpr int AF = BK * BM;       // floats per A tile
  constexpr int BF = BK * BN;       // floats per B tile
  constexpr int APASS = AF / 1024;  // 16-B chunks of 256 threads per A tile

  float* As0 = sm;
  float* As1 = sm + AF;
  float* Bs0 = sm + 2 * AF;
  float* Bs1 = Bs0 + BF;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int h = lane >> 5, lc = lane & 31;
  const int col = tid & (BN - 1);
  const int kg = tid >> 7;  // 0/1, uniform per wave

  float breg[2][8];
  float4 areg[APASS];

  auto load_tile = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
      const int kb = __builtin_amdgcn_readfirstlane(kt * BK + 8 * (kg + 2 * g2));
      gather(kb, breg[g2]);
    }
    const float4* ap = reinterpret_cast<const float4*>(wbase + (long)kt * AF);
#pragma unroll
    for (int p = 0; p < APASS; ++p) areg[p] = ap[p * 256 + tid];
  };
  auto store_tile = [&](float* As, float* Bs) __attribute__((always_inline)) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
      for (int e = 0; e < 8; ++e) Bs[(8 * (kg + 2 * g2) + e) * BN + col] = breg[g2][e];
    float4* ad = reinterpret_cast<float4*>(As);
#pragma unroll
    for (int p = 0; p < APASS; ++p) ad[p * 256 + tid] = areg[p];
  };

#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  f32x16 part[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) part[i][j] = acc[i][j];

  load_tile(0);
  store_tile(As0, Bs0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const float* As = (kt & 1) ? As1 : As0;
    const float* Bs = (kt & 1) ? Bs1 : Bs0;
    // unconditional prefetch (the last tile re-loads itself into the idle buffer), as in the
    // f16x3 kernels
    load_tile(kt + 1 < nkt ? kt + 1 : kt);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = As[(kk + h) * BM + (wm * TM + i) * 32 + lc];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = Bs[(kk + h) * BN + (wn * TN + j) * 32 + lc];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          part[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], part[i][j], 0, 0, 0);
    }
    if ((kt & (KCHUNK - 1)) == KCHUNK - 1 || kt == nkt - 1) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            acc[i][j][r] += part[i][j][r];
            part[i][j][r] = 0.f;
          }
    }
    store_tile((kt & 1) ? As0 : As1, (kt & 1) ? Bs0 : Bs1);
    __syncthreads();
  }
}

// XCD-contiguous column-tile order (conv_gemm_x3.hip)
__device__ __forceinline__ long column_tile() {
  return (gridDim.x & 7) ? (long)blockIdx.x : (long)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3));
}

// dynamic LDS of a BM-row block (the 128-row tile needs 64 KiB)
constexpr size_t lds_bytes(int bm) { return (size_t)2 * BK * (bm + BN) * sizeof(float); }

}  // namespace f32gemm
}  // namespace extdm
