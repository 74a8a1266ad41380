// The two-wave 64-token attention core of stw64_x3.hip (3-D windows of up to 64 tokens) and
// temporal64_x3.hip (33..64 frames of a pixel). A 64-token group (a window / a pixel) is two
// WAVES, each owning one 32-token tile (tokens 32 tt .. 32 tt + 31, tt = wave & 1); a workgroup
// holds NW / 2 groups. The kernels differ in where a token lies, how x is staged, which norms
// precede the core and which residual follows it; from the normalised token in registers to the
// projection accumulators everything is here. stw64_x3_kernel calls all of it; temporal64_x3_kernel
// takes the layout and the launch pieces and, for now, keeps a textual copy of load_unit,
// scale_split and unit_loop (its file head says why: 19 instructions per wave, 0.28 %), so a
// change to those three is made there too and the two stay bit-compatible:
//   load_unit     a unit's packed weight slice (UnitLayout, attn_x3_ops.h) into a ring slot by LDS-DMA
//   scale_split   the normalised channels times the wave's power of two, as fp16 hi / lo fragments
//   unit_loop     per unit of 32 qkv rows (one dim-32 head or two dim-16 heads), the weights
//                 arriving through the two-slot ring:
//                   Q^T, K^T = Wq Xn^T, Wk Xn^T (rows = head dims, lane = token), V = Xn Wv^T
//                   scale + RoPE (rotary position = token index in the group), split into operands;
//                 the wave's K and V operand fragments go to LDS (8 KB per wave; bf16: 4 KB), ONE
//                 barrier, and each wave then reads the K / V fragments of BOTH tiles of its group:
//                   S^T[kt] = K[kt] Q^T + bias          (kt = 0, 1: 64 keys x the wave's 32 queries)
//                   softmax over the 64 keys (in-lane over 32 registers, then the partner half lane ^ 32)
//                   O^T    = sum_kt V[kt]^T P[kt]^T    (P^T straight from the score registers)
//                   Y     += Wp O^T                    (projection accumulators, C / 32 tiles)
//                 nothing of q, k, v, the scores or O touches HBM.
//   xcd_slot / xcd_grid / allow_full_lds   the launch pieces both kernels share.
// LDS: [ring: 2 unit slices][exchange: NW waves x XS slots x 64 lanes x 16 B]; a kernel's x tile
// may alias the exchange region outside unit_loop.
#pragma once
#include <mutex>

#include "attn_x3_ops.h"

namespace extdm {
namespace attn_ops {

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// unit u's weight slice by LDS-DMA, UnitLayout<C>::HALVES / 512 pieces of 1 KiB over the waves
template <int C, int NW>
__device__ __forceinline__ void load_unit(const _Float16* __restrict__ wpk, int u, _Float16* dst, int wave, int lane) {
  using UL = UnitLayout<C>;
  static_assert((UL::HALVES / 512) % NW == 0, "unit slice pieces per wave");
  const _Float16* src = wpk + (long)u * UL::HALVES;
#pragma unroll
  for (int i = 0; i < UL::HALVES / 512 / NW; ++i) {
    const int pc = wave + i * NW;
    __builtin_amdgcn_global_load_lds((const void*)(src + pc * 512 + lane * 8), (lds_ptr_t)(dst + pc * 512), 16, 0, 0);
  }
}

// The wave's largest |value| of the normalised xv to [2^8, 2^9) (stw_x3.hip: e_w; exact
// power-of-two scaling, folded back through the q / k / v factors by gi = 2^-e_w, so the two waves
// of a group may differ; a wave is one group of one sample: bitwise batch independence), then the
// hi / lo fragments of the k-slices.
template <int KS>
__device__ __forceinline__ void scale_split(float (&xv)[KS][8], h8* xh, h8* xl, float& gi, int& bad) {
  float am = 0.f;
#pragma unroll
  for (int k = 0; k < KS; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(xv[k][e]));
  am = xh_max(am);
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) am = fmaxf(am, __shfl_xor(am, off));
  int ew = am > 0.f && am < INFINITY ? 9 - __builtin_amdgcn_frexp_expf(am) : 0;
  ew = ew < -100 ? -100 : (ew > 100 ? 100 : ew);
  const float gs = __builtin_amdgcn_ldexpf(1.f, ew);
  gi = __builtin_amdgcn_ldexpf(1.f, -ew);
#pragma unroll
  for (int k = 0; k < KS; ++k) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const f2 t = pair(xv[k][e], xv[k][e + 1]) * splat(gs);
      xv[k][e] = t.x; xv[k][e + 1] = t.y;
    }
    split8(xv[k], xh[k], xl[k], bad);
  }
}

// The unit loop of one wave: token tk = 32 (wave & 1) + (lane & 31) of its group, half h = lane >> 5,
// normalised input xh / xl (scale_split), q / k / v factors sq, sk, sv (wsc times gi), softmax factor
// csm. wsm: the ring (unit 0's load_unit already issued), xch: the exchange region behind it.
// Bias + masks: rs_mb holds tables [8 heads][64 queries][64 keys] carrying the scores' factor
// 2^(e_q + e_k) (stw_x3.hip operand-scale note), the wave's table at byte offset mb_wave
// (wave-uniform); a lane reads its query's row at byte offset mb_lane = (tk * 64 + 4 h) * 4, 4 x 16-B
// pieces per key tile and head. Adds Y into pacc (zeroed by the caller) and ORs a failed range /
// finite check into bad.
template <int C, int DH, int NW, bool BF>
__device__ __forceinline__ void unit_loop(_Float16* wsm, const _Float16* __restrict__ wpk, h8* xch, int wave, int lane,
                                          int h, int tk, bool active, bool valid, __amdgpu_buffer_rsrc_t rs_mb,
                                          int mb_lane, int mb_wave, const h8* xh, const h8* xl, float sq, float sk,
                                          float sv, float csm, const float* __restrict__ rcos,
                                          const float* __restrict__ rsin, f32x16* pacc, int& bad) {
  using UL = UnitLayout<C>;
  constexpr int KS = UL::KS;
  constexpr int UNITS = 8 * DH / 32;  // heads 8
  constexpr int HPU = 32 / DH;
  constexpr int RH = DH / 2;
  constexpr int CT = C / 32;
  constexpr int XS = 2 * 2 * Op<BF>::SLOTS;  // exchange slots per lane: K and V, 2 k-steps
  constexpr bool FOLD = C == 64;             // q / k scales folded into the RoPE factors

  // RoPE factors of the lane's (token, dim pair) registers, the same for every unit
  float rcq[8], rsq[8], rck[8], rsk[8];
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int pi = (dof(r, h) % DH) >> 1;
    const float c = rcos[tk * RH + pi], sn = rsin[tk * RH + pi];
    rcq[r >> 1] = FOLD ? c * sq : c; rsq[r >> 1] = FOLD ? sn * sq : sn;
    rck[r >> 1] = FOLD ? c * sk : c; rsk[r >> 1] = FOLD ? sn * sk : sn;
  }

  h8* const mine = xch + wave * XS * 64 + lane;
  const h8* const kv0 = xch + (wave & ~1) * XS * 64 + lane;  // the group's key tile 0
  const h8* const kv1 = kv0 + XS * 64;                        // and key tile 1
  constexpr int VOFF = 2 * Op<BF>::SLOTS * 64;                 // V behind K in a wave's slots

  for (int u = 0; u < UNITS; ++u) {
    const _Float16* W = wsm + (u & 1) * UL::HALVES;
    // unit u's slice has landed (LDS-DMA completion is per issuing wave: drain, then barrier),
    // slot (u + 1) & 1 and every wave's exchange slots of unit u - 1 are free (u = 0: every wave
    // has read its values from an x tile that aliases the exchange slots)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the bias / mask rows of the unit's first head, issued ahead of the next unit's weight DMA
    // (vmcnt retires in issue order, so waiting for them does not wait for the DMA); a second
    // head's (dim 16) are issued once the first head's have been added, into the same registers
    f32x16 bia[2];
    auto load_bias = [&](int hh) __attribute__((always_inline)) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const auto v4 = __builtin_amdgcn_raw_buffer_load_b128(rs_mb, mb_lane + (32 * kt + 8 * q) * 4,
                                                                mb_wave + (u * HPU + hh) * 4096 * 4, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) bia[kt][4 * q + e] = __uint_as_float(v4[e]);
        }
    };
    load_bias(0);
    if (u + 1 < UNITS) load_unit<C, NW>(wpk, u + 1, wsm + ((u + 1) & 1) * UL::HALVES, wave, lane);

    Op<BF> qf[2];
    if (active) {
      // Q^T, K^T (rows = dims, lane = token): the next k-step's fragments read from LDS while
      // this step's MFMAs run (stw_x3.hip qkv_mfma)
      f32x16 q, k, v;
#pragma unroll
      for (int r = 0; r < 16; ++r) { q[r] = 0.f; k[r] = 0.f; v[r] = 0.f; }
      h8 fr[2][4];
      auto ld = [&](int s, h8* f) __attribute__((always_inline)) {
        const _Float16* fq = W + UL::Q + s * UL::FRAG + lane * 8;
        const _Float16* fk = W + UL::K + s * UL::FRAG + lane * 8;
        f[0] = *reinterpret_cast<const h8*>(fq); f[1] = *reinterpret_cast<const h8*>(fq + 512);
        f[2] = *reinterpret_cast<const h8*>(fk); f[3] = *reinterpret_cast<const h8*>(fk + 512);
      };
      ld(0, fr[0]);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if (s + 1 < KS) ld(s + 1, fr[(s + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        const h8* f = fr[s & 1];
        q = mma3(f[0], f[1], xh[s], xl[s], q);
        k = mma3(f[2], f[3], xh[s], xl[s], k);
        __builtin_amdgcn_sched_barrier(0);
      }
      // V (rows = tokens, lane = dim)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const _Float16* fv = W + UL::V + s * UL::FRAG + lane * 8;
        v = mma3(xh[s], xl[s], *reinterpret_cast<const h8*>(fv), *reinterpret_cast<const h8*>(fv + 512), v);
      }
      // scale, RoPE on (d, d + 1) = registers (r, r + 1), as packed pairs:
      // (x0, x1) <- (x0, x1) c + (-x1, x0) s
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        float q0 = q[r], q1 = q[r + 1], k0 = k[r], k1 = k[r + 1];
        if (!FOLD) { q0 *= sq; q1 *= sq; k0 *= sk; k1 *= sk; }
        q[r] = fmaf(q0, rcq[r >> 1], -(q1 * rsq[r >> 1]));
        q[r + 1] = fmaf(q1, rcq[r >> 1], q0 * rsq[r >> 1]);
        k[r] = fmaf(k0, rck[r >> 1], -(k1 * rsk[r >> 1]));
        k[r + 1] = fmaf(k1, rck[r >> 1], k0 * rsk[r >> 1]);
      }
      // operands; this wave's K and V go to its exchange slots. V is scaled before the exchange:
      // the two waves' sv differ (their e_w), and PV needs both tiles' V at one scale
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float tq[8], tk_[8], tv[8];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          tq[e] = q[8 * s + e]; tq[e + 1] = q[8 * s + e + 1];
          tk_[e] = k[8 * s + e]; tk_[e + 1] = k[8 * s + e + 1];
          const f2 t = pair(v[8 * s + e], v[8 * s + e + 1]) * splat(sv);
          tv[e] = t.x; tv[e + 1] = t.y;
        }
        Op<BF> kf, vf;
        qf[s].set(tq, bad);
        kf.set(tk_, bad);
        vf.set(tv, bad);
        kf.put(mine + s * Op<BF>::SLOTS * 64);
        vf.put(mine + VOFF + s * Op<BF>::SLOTS * 64);
      }
    }
    __syncthreads();  // both tiles' K / V are in LDS
    if (!active) continue;

    // O^T per head: a dim-16 unit's two heads accumulate apart over the whole V (no per-lane
    // masking of the other head's V rows: 64 v_cndmask per unit) and the projection takes rows
    // 0-7 of the registers (dims 0-15: head 0) from o[0] and rows 8-15 from o[1]
    f32x16 o[HPU];
#pragma unroll
    for (int hh = 0; hh < HPU; ++hh)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[hh][r] = 0.f;
#pragma unroll
    for (int hh = 0; hh < HPU; ++hh) {
      // S^T[kt] = bias + K[kt] Q^T (rows = keys of tile kt, lane = query): the bias / mask rows are
      // the chain's initial accumulator (no separate add; the chain rounds at the bias's scale)
      f32x16 sc_[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        sc_[kt] = bia[kt];
#pragma unroll
        for (int s = 0; s < 2; ++s)
          if (HPU == 1 || s == hh) {
            Op<BF> kf;
            kf.get((kt ? kv1 : kv0) + s * Op<BF>::SLOTS * 64);
            sc_[kt] = mmo(kf, qf[s], sc_[kt]);
          }
      }
      if (hh + 1 < HPU) load_bias(hh + 1);
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc_[kt][r]);
      mx = xh_max(mx);
      // P' = 16 exp(s - mx) = v_exp_f32 of fma(s, log2 e 2^-(e_q+e_k), 4 - mx ...) (masked -inf -> 0),
      // unnormalised: O is scaled by 16 / sum P' after PV (16 or 8 products instead of 32)
      const float sum = xh_sum(exp2_sum<2>(sc_, csm, mx * csm - 4.f));
      const float inv = 16.f * __builtin_amdgcn_rcpf(sum);  // O carries P = 16 p
      // O^T[dd][i] += sum_j V^T[dd][j] P'^T[j][i]
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float tp[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) tp[e] = sc_[kt][8 * s + e];
          Op<BF> pf, vf;
          pf.set(tp, bad);
          vf.get((kt ? kv1 : kv0) + VOFF + s * Op<BF>::SLOTS * 64);
          o[hh] = mmo(vf, pf, o[hh]);
        }
      // the head's rows: all 16 registers (dim 32), registers 8 hh .. 8 hh + 7 (dim 16)
#pragma unroll
      for (int r = 0; r < 16; r += 2)
        if (HPU == 1 || (r >> 3) == hh) {
          const f2 t = pair(o[hh][r], o[hh][r + 1]) * splat(inv);
          o[hh][r] = t.x; o[hh][r + 1] = t.y;
        }
    }
    // projection / to_out: Y[c][i] += sum_dd Wp[c][u*32 + dd] O^T[dd][i] (f16x3)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float to[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) to[e] = o[HPU == 1 ? 0 : s][8 * s + e];
      h8 oh, ol;
      split8<false>(to, oh, ol, bad);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const _Float16* fp = W + UL::P + (ct * 2 + s) * UL::FRAG + lane * 8;
        pacc[ct] = mma3(*reinterpret_cast<const h8*>(fp), *reinterpret_cast<const h8*>(fp + 512), oh, ol, pacc[ct]);
      }
    }
  }
  // one finite check of the token's accumulators covers the loop's unchecked splits (stw_x3.hip)
  float chk = 0.f;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) chk += pacc[ct][r];
  bad |= valid && !__builtin_isfinite(chk);
}

// XCD-contiguous workgroup order (remap: the grid is a multiple of 8, xcd_grid): workgroup b runs on
// XCD b mod 8 and takes logical slot (b mod 8) G / 8 + b / 8, so consecutive logical workgroups,
// whose tiles share 128-B lines, run on one XCD and their partial lines merge in its L2 instead of
// leaving it as separate partial-line write-backs
__device__ __forceinline__ int xcd_slot(int remap) {
  const int G8 = (int)gridDim.x;
  return remap ? (int)((blockIdx.x & 7) * (G8 >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x;
}

// Host: the grid for `total` groups, NW / 2 per workgroup. xcd and at least 64 workgroups: remap = 1
// and the grid rounded up to a multiple of 8 (the extra workgroups' groups lie past `total`:
// inactive); else dispatch order.
inline int xcd_grid(int total, int NW, bool xcd, int& remap) {
  const int grid = (total + NW / 2 - 1) / (NW / 2);
  remap = xcd && grid >= 64 ? 1 : 0;
  return remap ? (grid + 7) & ~7 : grid;
}

// Host: ring + exchange bytes, the exchange region grown to a tile that aliases it
template <int C, int NW, bool BF>
inline size_t attn64_lds(size_t tile_bytes) {
  const size_t ring = (size_t)2 * UnitLayout<C>::HALVES * sizeof(_Float16);
  const size_t xch = (size_t)NW * 2 * 2 * Op<BF>::SLOTS * 64 * 16;
  return ring + (tile_bytes > xch ? tile_bytes : xch);
}

// Host: lets a kernel's per-lane and tile instantiations (the same one where there is no tile
// path) take the whole 160 KB of LDS, once per device
template <auto PLAIN, auto TILED>
inline void allow_full_lds() {
  static std::once_flag once[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::call_once(once[dev & 63], [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(PLAIN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(TILED), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
}

}  // namespace attn_ops
}  // namespace extdm
