// Fused Residual(PreNorm(chanLN, AttentionLayer)) over the frames of every pixel for clips of
// 33..64 frames (u12:236-327, 903-915; the ada / ada_u22 / wo_ref modules alike):
//   out = x + chanLN(x) + to_out(attn(LN(chanLN(x))))
// C in {64, 128}, 8 heads of dim 32 or 16. The MODE 1 prologue and epilogue of attn_x3_kernel
// (stw_x3.hip: double LayerNorm, r = x + y, no projection bias) around the two-wave 64-token
// core of stw64_x3_kernel (stw64_x3.hip), on the packed_attn_x3 weights: qkv and to_out on
// f16x3 MFMA, QK^T and PV as f16x3 (BF = false) or on bf16 MFMA (BF = true, BF16_ATTN).
//
// A pixel is two WAVES, each owning one 32-frame tile (frames 32 tt .. 32 tt + 31, tt = wave & 1;
// frames >= D are masked slots); a workgroup holds NW / 2 pixels. Per wave (lane = frame lc,
// half h):
//  1. the lane loads the channels of its MFMA k-slices (16 s + 8 h + e) of its frame, applies
//     the channel LayerNorm (gamma) and the inner LayerNorm (w, b), scales by the wave's power of
//     two and keeps the result as fp16 hi / lo fragments; the first norm's mean and 1 / std stay
//     in two registers for the residual;
//  2. per unit of 32 qkv rows (one dim-32 head or two dim-16 heads), weights through the
//     two-slot LDS-DMA ring: Q^T, K^T, V, scale + RoPE (rotary position = frame index), the
//     wave's K / V operand fragments to LDS, ONE barrier, then S^T[kt] = K[kt] Q^T + bias over
//     both key tiles, softmax over the 64 keys, O^T = sum_kt V[kt]^T P[kt]^T, Y += Wo O^T;
//  3. epilogue: out = Y + (x + (x - mean) / std * gamma).
// Bias + mask: one table [8 heads][64 queries][64 keys] (temporal_mask_bias64, runtime.cpp): the
// T5 bias of (query frame, key frame), -inf for key frames >= D, times 2^(e_q + e_k).
//
// Access pattern. A wave's 32 tokens are 32 frames of one pixel, H*W floats apart: per-lane 4-B
// loads and stores touch 32 lines per instruction and use 4 B of each. TILE (C = 64, 8 waves):
// the workgroup's four pixels are adjacent along H*W (16 B of one line per channel and frame),
// and the workgroup's C x 64 frames x 4 pixels of x are staged into LDS by LDS-DMA, one 1-KiB
// instruction per channel (lane l loads the 16 B of frame l; slots l >= D re-read frame D - 1 and
// are masked, never stored), layout [c][frame][4 px]: every line is touched once per workgroup
// with 16 B used, a quarter of the per-lane instructions, and the eight workgroups that share a
// 128-B line are consecutive, so under the XCD-contiguous order they run on one XCD and the line
// is fetched from HBM once and merged in that L2 on the way out. The lanes read their frame's
// channels from the tile (ds_read_b32 at a 16-B stride: 4-way bank conflicts over 32 reads per
// lane, once per kernel). The tile aliases the K / V exchange region, so the epilogue stages x
// again the same way (an L2 hit), adds Y + the residual in place (each (channel, frame, pixel) is
// one lane's) and the tile leaves as the same 16-B pieces. C = 128 (4 waves, two pixels per
// workgroup, ring + exchange fill the LDS) and unaligned geometries take the per-lane path.
//
// The unit loop below is still this file's own copy of attn64_core.h's unit_loop (and of its
// load_unit / scale_split): calling the shared functions compiled to 19 more instructions per wave
// outside the loop (64-bit vector addresses for unit 0's weight DMA, two SGPR spills, unpaired
// zeroing moves) and measured 0.28 % slower on the 50-frame KTH layer, past the parent's 0.24 %
// spread (profiles/attn64_core_refactor.json). A fix to the core goes into both places. The
// layout, the XCD slot and the launch pieces are the shared ones.
#include <cstdlib>

#include "attn64_core.h"
#include "host_util.h"

namespace extdm {

namespace {

using namespace attn_ops;

template <int C, int DH, int NW, bool BF, bool TILE>
__global__ __launch_bounds__(NW * 64) void temporal64_x3_kernel(const float* x, float* out, long sb, long sc, long st,
                                                                int D, int HW, const float* __restrict__ gamma,
                                                                const float* __restrict__ ln_w,
                                                                const float* __restrict__ ln_b,
                                                                const _Float16* __restrict__ wpk,
                                                                const float* __restrict__ wsc,  // 2^-s: q, k, v, proj, exp2
                                                                const float* __restrict__ mbias,
                                                                const float* __restrict__ rcos,
                                                                const float* __restrict__ rsin, float q_scale,
                                                                int total_groups, int* __restrict__ range_flag,
                                                                int remap) {
  using UL = UnitLayout<C>;
  constexpr int KS = UL::KS;
  constexpr int UNITS = 8 * DH / 32;  // heads 8
  constexpr int HPU = 32 / DH;
  constexpr int RH = DH / 2;
  constexpr int CT = C / 32;
  constexpr int XS = 2 * 2 * Op<BF>::SLOTS;  // exchange slots per lane: K and V, 2 k-steps
  constexpr bool FOLD = C == 64;             // q / k scales folded into the RoPE factors
  constexpr int WPG = NW / 2;                // pixels per workgroup
  static_assert(!TILE || (C == 64 && NW == 8), "tile path: C = 64, 8 waves (4 pixels = 16 B)");
  extern __shared__ __attribute__((aligned(16))) _Float16 wsm[];
  h8* const xch = reinterpret_cast<h8*>(wsm + 2 * UL::HALVES);  // [NW][XS][64 lanes]
  float* const tileL = reinterpret_cast<float*>(wsm + 2 * UL::HALVES);  // TILE: [C][64 frames][4 px]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tt = wave & 1;
  const int h = lane >> 5, lc = lane & 31;
  // XCD-contiguous order: consecutive logical workgroups, whose pixels share 128-B lines, on one XCD
  const int bid = xcd_slot(remap);
  const int gidx = bid * WPG + (wave >> 1);  // the wave's pixel
  const bool active = gidx < total_groups;
  // TILE: HW is a multiple of WPG (host), so a workgroup is wholly inside one sample or inactive
  if (TILE && bid * WPG >= total_groups) return;
  const int b = active ? gidx / HW : 0;
  const int hw = active ? gidx % HW : 0;
  const float* const xb = x + (long)b * sb;
  float* const ob = out + (long)b * sb;

  // buffer descriptors: the lane's token (and channel half) in the 32-bit offset, the channel
  // row in the wave-uniform soffset, invalid tokens past the extent (host checks 31 bits)
  constexpr int OOB = 0x40000000;
  const int x_bytes = (int)(((long)(C - 1) * sc + (long)D * st) * 4);
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, x_bytes, 0x00020000);
  const auto rs_o = __builtin_amdgcn_make_buffer_rsrc(ob, 0, x_bytes, 0x00020000);
  const auto rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gamma), 0, C * 4, 0x00020000);
  const auto rs_lw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ln_w), 0, C * 4, 0x00020000);
  const auto rs_lb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ln_b), 0, C * 4, 0x00020000);
  const auto rs_mb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(mbias), 0, 8 * 4096 * 4, 0x00020000);
  auto ldb = [](const __amdgpu_buffer_rsrc_t& r, int vo, int so) __attribute__((always_inline)) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
  };

  // a unit's weight slice by LDS-DMA, UL::HALVES / 512 pieces of 1 KiB over the waves
  static_assert((UL::HALVES / 512) % NW == 0, "unit slice pieces per wave");
  auto load_unit = [&](int u, _Float16* dst) __attribute__((always_inline)) {
    const _Float16* src = wpk + (long)u * UL::HALVES;
#pragma unroll
    for (int i = 0; i < UL::HALVES / 512 / NW; ++i) {
      const int pc = wave + i * NW;
      __builtin_amdgcn_global_load_lds((const void*)(src + pc * 512 + lane * 8), (lds_ptr_t)(dst + pc * 512), 16, 0, 0);
    }
  };
  load_unit(0, wsm);

  // ---- the lane's token: frame tk = 32 tt + lc of pixel hw ----
  const int tk = 32 * tt + lc;
  const bool valid = active && tk < D;
  const long pos = (long)tk * st + hw;
  const int mb_lane = (tk * 64 + 4 * h) * 4;
  // TILE: the workgroup's 4 pixels x 64 frame slots of every channel, one 1-KiB LDS-DMA per channel
  // (lane = frame slot; slots >= D re-read frame D - 1)
  const int hw0 = TILE ? (bid * WPG) % HW : 0;  // the workgroup's first pixel (a multiple of 4)
  const long toff = (long)(lane < D ? lane : D - 1) * st + hw0;
  auto stage_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < C / NW; ++i) {
      const int c = wave + i * NW;
      __builtin_amdgcn_global_load_lds((const void*)(xb + (long)c * sc + toff), (lds_ptr_t)(tileL + c * 256), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  if (TILE) stage_tile();  // (also waits for unit 0's weights: one drain)
  const int tix = tk * 4 + (wave >> 1);  // the lane's (frame, pixel) in a channel plane of the tile

  // ---- 1. channel LayerNorm, inner LayerNorm, into register fragments ----
  const float sq0 = wsc[0] * q_scale, sk0 = wsc[1], sv0 = wsc[2], csm = wsc[4];
  const int vpro = valid ? (int)((8 * h * sc + pos) * 4) : OOB;  // channel 8h + (16k + e)
  int bad = 0;
  h8 xh[KS], xl[KS];
  float gi = 1.f, m1 = 0.f, rden1 = 1.f;
  {
    float xv[KS][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xv[k][e] = TILE ? tileL[(16 * k + 8 * h + e) * 256 + tix] : ldb(rs_x, vpro, (int)((16 * k + e) * sc * 4));
        s += xv[k][e];
      }
    s = xh_sum(s);
    m1 = s / C;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = xv[k][e] - m1; v += d * d; }
    v = xh_sum(v);
    // one reciprocal instead of a division per element, here and in the epilogue (stw_x3.hip)
    rden1 = 1.f / sqrtf(v / C + 1e-5f);
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xv[k][e] = (xv[k][e] - m1) * rden1 * ldb(rs_g, 32 * h, (16 * k + e) * 4);
        s2 += xv[k][e];
      }
    s2 = xh_sum(s2);
    const float m2 = s2 / C;
    float v2 = 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = xv[k][e] - m2; v2 += d * d; }
    v2 = xh_sum(v2);
    const float rstd2 = 1.0f / sqrtf(v2 / C + 1e-5f);
    // masked frame slots normalise to 0 through a 0 factor (stw_x3.hip: no select per element)
    const float vm = valid ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        xv[k][e] = ((xv[k][e] - m2) * rstd2 * ldb(rs_lw, 32 * h, (16 * k + e) * 4) +
                    ldb(rs_lb, 32 * h, (16 * k + e) * 4)) * vm;
    // the wave's largest |value| to [2^8, 2^9) (stw_x3.hip: e_w; exact power-of-two scaling,
    // folded back through the q / k / v factors, so the two waves of a pixel may differ; a wave
    // is one pixel of one sample: bitwise batch independence)
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
  const float sq = sq0 * gi, sk = sk0 * gi, sv = sv0 * gi;

  f32x16 pacc[CT];
#pragma unroll
  for (int i = 0; i < CT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) pacc[i][r] = 0.f;

  // RoPE factors of the lane's (frame, dim pair) registers, the same for every unit
  float rcq[8], rsq[8], rck[8], rsk[8];
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int pi = (dof(r, h) % DH) >> 1;
    const float c = rcos[tk * RH + pi], sn = rsin[tk * RH + pi];
    rcq[r >> 1] = FOLD ? c * sq : c; rsq[r >> 1] = FOLD ? sn * sq : sn;
    rck[r >> 1] = FOLD ? c * sk : c; rsk[r >> 1] = FOLD ? sn * sk : sn;
  }

  h8* const mine = xch + wave * XS * 64 + lane;
  const h8* const kv0 = xch + (wave & ~1) * XS * 64 + lane;  // the pixel's key tile 0
  const h8* const kv1 = kv0 + XS * 64;                        // and key tile 1
  constexpr int VOFF = 2 * Op<BF>::SLOTS * 64;                 // V behind K in a wave's slots

  for (int u = 0; u < UNITS; ++u) {
    const _Float16* W = wsm + (u & 1) * UL::HALVES;
    // unit u's slice has landed (LDS-DMA completion is per issuing wave: drain, then barrier),
    // slot (u + 1) & 1 and every wave's exchange slots of unit u - 1 are free (u = 0: every
    // wave has read its tile values, which the exchange slots alias)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the bias / mask rows of the unit's first head, issued ahead of the next unit's weight DMA
    f32x16 bia[2];
    auto load_bias = [&](int hh) __attribute__((always_inline)) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const auto v4 = __builtin_amdgcn_raw_buffer_load_b128(rs_mb, mb_lane + (32 * kt + 8 * q) * 4,
                                                                (u * HPU + hh) * 4096 * 4, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) bia[kt][4 * q + e] = __uint_as_float(v4[e]);
        }
    };
    load_bias(0);
    if (u + 1 < UNITS) load_unit(u + 1, wsm + ((u + 1) & 1) * UL::HALVES);

    Op<BF> qf[2];
    if (active) {
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
      // V (rows = frames, lane = dim)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const _Float16* fv = W + UL::V + s * UL::FRAG + lane * 8;
        v = mma3(xh[s], xl[s], *reinterpret_cast<const h8*>(fv), *reinterpret_cast<const h8*>(fv + 512), v);
      }
      // scale, RoPE on (d, d + 1) = registers (r, r + 1): (x0, x1) <- (x0, x1) c + (-x1, x0) s
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        float q0 = q[r], q1 = q[r + 1], k0 = k[r], k1 = k[r + 1];
        if (!FOLD) { q0 *= sq; q1 *= sq; k0 *= sk; k1 *= sk; }
        q[r] = fmaf(q0, rcq[r >> 1], -(q1 * rsq[r >> 1]));
        q[r + 1] = fmaf(q1, rcq[r >> 1], q0 * rsq[r >> 1]);
        k[r] = fmaf(k0, rck[r >> 1], -(k1 * rsk[r >> 1]));
        k[r + 1] = fmaf(k1, rck[r >> 1], k0 * rsk[r >> 1]);
      }
      // operands; this wave's K and V go to its exchange slots
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float tq[8], tk_[8], tv[8];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          tq[e] = q[8 * s + e]; tq[e + 1] = q[8 * s + e + 1];
          tk_[e] = k[8 * s + e]; tk_[e + 1] = k[8 * s + e + 1];
          const f2 t = pair(v[8 * s + e], v[8 * s + e + 1]) * splat(sv);  // both tiles' V at one scale
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

    // O^T per head (a dim-16 unit's two heads accumulate apart over the whole V: stw64_x3.hip)
    f32x16 o[HPU];
#pragma unroll
    for (int hh = 0; hh < HPU; ++hh)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[hh][r] = 0.f;
#pragma unroll
    for (int hh = 0; hh < HPU; ++hh) {
      // S^T[kt] = bias + K[kt] Q^T (rows = key frames of tile kt, lane = query frame)
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
      // P' = 16 exp(s - mx), unnormalised: O is scaled by 16 / sum P' after PV (stw64_x3.hip)
      const float sum = xh_sum(exp2_sum<2>(sc_, csm, mx * csm - 4.f));
      const float inv = 16.f * __builtin_amdgcn_rcpf(sum);
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
#pragma unroll
      for (int r = 0; r < 16; r += 2)
        if (HPU == 1 || (r >> 3) == hh) {
          const f2 t = pair(o[hh][r], o[hh][r + 1]) * splat(inv);
          o[hh][r] = t.x; o[hh][r + 1] = t.y;
        }
    }
    // to_out: Y[c][i] += sum_dd Wo[c][u*32 + dd] O^T[dd][i] (f16x3)
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
  {
    float chk = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) chk += pacc[ct][r];
    bad |= valid && !__builtin_isfinite(chk);
  }
  if (bad) atomicOr(range_flag, 2);
  // ---- 3. out = Y + (x + chanLN(x)) (row cu + 4h of register r) ----
  const float spj = wsc[3];
  if (TILE) {
    // x again into the tile (its exchange alias is free once every wave is past the loop), the
    // result in place, then the tile leaves as the DMA's 16-B pieces in reverse
    __syncthreads();
    stage_tile();
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float* tp = tileL + ch * 256 + tix;
        const float xv = *tp;
        *tp = pacc[ct][r] * spj + (xv + (xv - m1) * rden1 * ldb(rs_g, 16 * h, (ch - 4 * h) * 4));
      }
    __syncthreads();
    float* const o0 = ob + (long)lane * st + hw0;
#pragma unroll
    for (int i = 0; i < C / NW; ++i) {
      const int c = wave + i * NW;
      const float4 v = *reinterpret_cast<const float4*>(tileL + c * 256 + 4 * lane);
      if (lane < D) *reinterpret_cast<float4*>(o0 + (long)c * sc) = v;
    }
  } else if (valid) {
    const int vex = (int)((4 * h * sc + pos) * 4);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cu = ct * 32 + (r & 3) + 8 * (r >> 2);
        const float pb = ldb(rs_g, 16 * h, cu * 4);
        const float xv = ldb(rs_x, vex, (int)(cu * sc * 4));
        const float res = pacc[ct][r] * spj + (xv + (xv - m1) * rden1 * pb);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(res), rs_o, vex, (int)(cu * sc * 4), 0);
      }
  }
}

// The TILE path's geometry (kernel note): whole 4-pixel workgroups inside a sample and 16-B
// aligned pieces; EXTDM_T64_NO_TILE=1 (read per call) forces the per-lane path (A/B, tests)
bool t64_tile_ok(const View& x, const View& out, int HW) {
  const bool off = env_flag("EXTDM_T64_NO_TILE");
  return !off && x.C == 64 && HW % 4 == 0 && x.st % 4 == 0 && x.sc % 4 == 0 && x.sb % 4 == 0 &&
         ((uintptr_t)x.p & 15) == 0 && ((uintptr_t)out.p & 15) == 0;
}

template <int C, int DH, int NW, bool BF>
void launch(hipStream_t s, const View& x, const View& out, const AttnGeom& g, const float* gamma, const float* ln_w,
            const float* ln_b, const void* wpk, const float* wsc, const float* mbias, const float* rcos,
            const float* rsin, float q_scale) {
  constexpr bool TILE_OK = C == 64 && NW == 8;
  const int HW = g.H * g.W;
  const bool tile = TILE_OK && t64_tile_ok(x, out, HW);
  const size_t lds = attn64_lds<C, NW, BF>(tile ? (size_t)C * 256 * sizeof(float) : 0);
  allow_full_lds<&temporal64_x3_kernel<C, DH, NW, BF, false>, &temporal64_x3_kernel<C, DH, NW, BF, TILE_OK>>();
  const int total = x.B * HW;
  // EXTDM_T64_XCD=0: dispatch order (A/B)
  static const bool xcd = [] { const char* v = getenv("EXTDM_T64_XCD"); return !(v && v[0] == '0'); }();
  int remap;
  const int grid = xcd_grid(total, NW, xcd, remap);
  note_kernel("temporal64_x3_kernel<%d, %d, %d, %s, %s>", C, DH, NW, BF ? "true" : "false", tile ? "true" : "false");
  auto kern = tile ? &temporal64_x3_kernel<C, DH, NW, BF, TILE_OK> : &temporal64_x3_kernel<C, DH, NW, BF, false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, s, x.p, out.p, x.sb, x.sc, x.st, g.D, HW, gamma, ln_w, ln_b,
                     reinterpret_cast<const _Float16*>(wpk), wsc, mbias, rcos, rsin, q_scale, total, x3_range_ptr(),
                     remap);
}

template <int DH, bool BF>
bool dispatch(hipStream_t s, const View& x, const View& out, const AttnGeom& g, const float* gamma, const float* ln_w,
              const float* ln_b, const void* wpk, const float* wsc, const float* mbias, const float* rcos,
              const float* rsin, float q_scale) {
  // C = 64: 8 waves (four pixels, 128 KB of LDS); C = 128: 4 waves (two pixels; ring 128 KB +
  // exchange 32 KB = the whole 160 KB)
  if (x.C == 64) launch<64, DH, 8, BF>(s, x, out, g, gamma, ln_w, ln_b, wpk, wsc, mbias, rcos, rsin, q_scale);
  else if (x.C == 128) launch<128, DH, 4, BF>(s, x, out, g, gamma, ln_w, ln_b, wpk, wsc, mbias, rcos, rsin, q_scale);
  else return false;
  return true;
}

}  // namespace

bool temporal64_x3_supported(int C, int frames, int dim_head, int heads) {
  return heads == 8 && (C == 64 || C == 128) && frames > 32 && frames <= 64 && (dim_head == 32 || dim_head == 16) &&
         attn_x3_unit_halves(C) == (C == 64 ? UnitLayout<64>::HALVES : UnitLayout<128>::HALVES);
}

bool temporal64_x3(hipStream_t s, const View& x, const View& out, const AttnGeom& g, int heads, int dim_head,
                   const float* gamma, const float* ln_w, const float* ln_b, const void* wpk, const float* wsc,
                   const float* mbias, const float* rcos, const float* rsin, float q_scale, bool bf16) {
  if (!temporal64_x3_supported(x.C, g.D, dim_head, heads)) return false;
  // out shares x's strides; 31-bit buffer offsets per sample
  if (out.sb != x.sb || out.sc != x.sc || out.st != x.st || x.st != (long)x.H * x.W || out.C != x.C) return false;
  if (((long)(x.C - 1) * x.sc + (long)g.D * x.st) * 4 >= (1L << 30)) return false;
  if (dim_head == 32) {
    return bf16 ? dispatch<32, true>(s, x, out, g, gamma, ln_w, ln_b, wpk, wsc, mbias, rcos, rsin, q_scale)
                : dispatch<32, false>(s, x, out, g, gamma, ln_w, ln_b, wpk, wsc, mbias, rcos, rsin, q_scale);
  }
  // BF16_ATTN at dim_head 16 is not this kernel's: temporal_long() sends it to the fp32 route
  return !bf16 && dispatch<16, false>(s, x, out, g, gamma, ln_w, ln_b, wpk, wsc, mbias, rcos, rsin, q_scale);
}

}  // namespace extdm
