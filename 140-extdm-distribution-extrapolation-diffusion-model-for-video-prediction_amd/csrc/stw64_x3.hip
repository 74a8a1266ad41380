// Fused Residual(PreNorm(STWAttentionLayer)) over 3-D windows of up to 64 tokens: the
// ada / ada_u22 denoisers' 4x4x4 windows (…_ada.py:408-559, …_ada_u22.py:531-700; the
// layer as u12:138-158, 408-559, 961-963), in place on x:
//   x[:, win] += proj(attn(qkv(chanLN(x[:, win])))) + b
// qkv and proj run on f16x3 MFMA (three v_mfma_f32_32x32x16_f16 per fp32 product, the
// convention of stw_x3.hip); the attention contractions QK^T and PV run either as f16x3
// (BF = false, EXTDM_PRECISION_F16X3: fp32-faithful) or on v_mfma_f32_32x32x16_bf16
// (BF = true, EXTDM_PRECISION_BF16_ATTN: q, k, v and the probabilities rounded to bf16,
// fp32 accumulation — the UCF-101 256 configuration's "bf16 MFMA attention").
//
// A window is two WAVES, each owning one 32-token tile (tokens 32 tt .. 32 tt + 31 of the
// window, tt = wave & 1); a workgroup holds NW / 2 windows. Per wave (lane = token lc, half h):
//  1. the lane loads exactly the channels of its MFMA k-slices (16 s + 8 h + e) of its token,
//     channel-LayerNorms them (mean / variance over the two halves), scales them by the
//     wave's power of two and keeps them as fp16 hi / lo fragments in registers;
//  2. the two-wave 64-token core (attn64_core.h unit_loop): qkv, RoPE (rotary position = window
//     token index), the K / V exchange, scores + softmax over the 64 keys, PV and the projection
//     into the accumulators Y, on the packed_attn_x3 weights;
//  3. epilogue: Y + bias + residual to the token's positions (buffer stores; padded tokens'
//     offsets lie past the descriptor's extent).
// Bias + masks: one table [npat][8 heads][64 queries][64 keys] per layer (stw_mask_bias64,
// runtime.cpp): the dense relative-position bias, -100 where a shifted window's region labels
// differ (u12:414-436), -inf for keys past the window's N tokens, times the scores' factor
// 2^(e_q + e_k); the window's class pat selects the table the core reads.
#include <cstdlib>

#include "attn64_core.h"
#include "host_util.h"

namespace extdm {

namespace {

using namespace attn_ops;

// TILE (host check stw64_tile_ok; C = 64 on 8 waves): the workgroup's NW / 2 windows are consecutive
// along W (one (wd, wh) window row, W a multiple of 16, no H / W padding), so together they cover
// C x 4 frames x 4 rows x 16 columns of x. That block is staged once into LDS by coalesced 8-B
// loads per lane (each 64-B row segment read by 8 adjacent lanes; a shifted row wraps only between
// 8-B pieces), the lanes read their token's channels from it (row stride 20, channel stride 324
// floats: the 32 tokens of a half-wave hit 32 banks, the two halves the other 32), and the epilogue
// writes Y + bias back into it and leaves as the same 8-B pieces plus the residual — instead of
// per-lane 4-B accesses that touch 16 lines per instruction (the per-lane prologue and epilogue
// took 40-55 % of the kernel at KTH / UCF level 0). The tile aliases the K / V exchange region
// (used only inside the unit loop).
template <int C, int DH, int NW, bool BF, bool TILE>
__global__ __launch_bounds__(NW * 64) void stw64_x3_kernel(float* x, long sb, long sc, long st, AttnGeom g,
                                                           const float* __restrict__ gamma,
                                                           const _Float16* __restrict__ wpk,
                                                           const float* __restrict__ wsc,  // 2^-s: q, k, v, proj, exp2
                                                           const float* __restrict__ bp,
                                                           const float* __restrict__ mbias, int npat,
                                                           const float* __restrict__ rcos,
                                                           const float* __restrict__ rsin, float q_scale,
                                                           int groups_per_sample, int total_groups,
                                                           int* __restrict__ range_flag, int remap) {
  using UL = UnitLayout<C>;
  constexpr int KS = UL::KS;
  constexpr int CT = C / 32;
  extern __shared__ __attribute__((aligned(16))) _Float16 wsm[];
  h8* const xch = reinterpret_cast<h8*>(wsm + 2 * UL::HALVES);  // [NW][XS][64 lanes]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tt = wave & 1;
  const int h = lane >> 5, lc = lane & 31;
  // XCD-contiguous order: the workgroups whose tiles share 128-B output lines (the two 16-column
  // halves of a 32-column row) run on one XCD
  const int bid = xcd_slot(remap);
  const int gidx = bid * (NW / 2) + (wave >> 1);  // the wave's window
  const bool active = gidx < total_groups;
  const int b = active ? gidx / groups_per_sample : 0;
  const int grp = active ? gidx % groups_per_sample : 0;
  float* const xb = x + (long)b * sb;
  constexpr int WPG = NW / 2;       // windows per workgroup
  constexpr int TC = 4 * WPG;       // tile columns
  constexpr int TRS = TC + 4;       // tile row stride (floats)
  constexpr int TCS = 16 * TRS + 4; // tile channel stride: 8 TCS = 32 mod 64 banks
  constexpr int NPC = 16 * TC / 2;  // 8-B pieces per channel
  constexpr int PPW = TILE ? C * NPC / (NW * 64) : 1;  // piece instructions per wave
  static_assert(!TILE || (C * NPC) % (NW * 64) == 0, "tile pieces per wave");
  float* const tileL = reinterpret_cast<float*>(wsm + 2 * UL::HALVES);

  // buffer descriptors: the lane's token (and channel half) in the 32-bit offset, the channel
  // row in the wave-uniform soffset, invalid tokens past the extent (host checks 31 bits)
  constexpr int OOB = 0x40000000;
  const int x_bytes = (int)(((long)(C - 1) * sc + (long)g.D * st) * 4);
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc(xb, 0, x_bytes, 0x00020000);
  const auto rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gamma), 0, C * 4, 0x00020000);
  const auto rs_mb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(mbias), 0, npat * 8 * 4096 * 4, 0x00020000);
  auto ldb = [](const __amdgpu_buffer_rsrc_t& r, int vo, int so) __attribute__((always_inline)) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
  };

  load_unit<C, NW>(wpk, 0, wsm, wave, lane);

  // ---- the lane's token: window (wd, wh, ww) of grp, token tk = 32 tt + lc ----
  const int nWw = g.Wp / g.ws2, nWh = g.Hp / g.ws1, nWd = g.Dp / g.ws0;
  const int ww = grp % nWw, wh = (grp / nWw) % nWh, wd = grp / (nWw * nWh);
  const int N = g.ws0 * g.ws1 * g.ws2;
  const int tk = 32 * tt + lc;
  long pos;
  bool valid;
  {
    const int td = tk / (g.ws1 * g.ws2), th = (tk / g.ws2) % g.ws1, tw = tk % g.ws2;
    const int od = (wd * g.ws0 + td + g.ss0) % g.Dp, oh = (wh * g.ws1 + th + g.ss1) % g.Hp,
              ow = (ww * g.ws2 + tw + g.ss2) % g.Wp;
    valid = active && tk < N && od < g.D && oh < g.H && ow < g.W;
    pos = (long)od * st + (long)oh * g.W + ow;
  }
  // window class of the bias / mask table: bit d for the last window along a shifted dim d
  const int pat = npat > 1 ? ((g.ss0 && wd == nWd - 1 ? 1 : 0) | (g.ss1 && wh == nWh - 1 ? 2 : 0) |
                              (g.ss2 && ww == nWw - 1 ? 4 : 0))
                           : 0;
  const int mb_lane = (tk * 64 + 4 * h) * 4;
  const int mb_wave = __builtin_amdgcn_readfirstlane(pat * 8 * 4096 * 4);
  // TILE: the workgroup's first window (all its windows share (b, wd, wh)) and the lane's k-th
  // 8-B piece: LDS float offset, global byte offset (past the extent for a padded frame)
  const int grp0 = TILE ? (bid * WPG) % groups_per_sample : 0;
  const int ww0 = grp0 % nWw, wh0 = (grp0 / nWw) % nWh, wd0 = grp0 / (nWw * nWh);
  // piece i of the lane: channel c0 + CPI i, the same (frame, row, column pair) for every i, so the
  // offsets are a base + i x a stride (32-bit: the host checks the sample's extent < 2^30 B)
  constexpr int CPI = NW * 64 / NPC;  // channels per wave instruction
  static_assert(!TILE || (NW * 64) % NPC == 0, "whole channels per piece instruction");
  struct Piece { int lbase, gbase; };
  auto piece_base = [&](int ln) __attribute__((always_inline)) {
    const int q = wave * 64 + ln;
    const int c = q / NPC, rem = q % NPC, pr = rem / (TC / 2), k = rem % (TC / 2);
    const int f = pr >> 2, r = pr & 3;
    // (the shifted coordinates stay below twice the padded extent: a conditional subtract, not a
    // division)
    int gd = wd0 * 4 + f + g.ss0, gh = wh0 * 4 + r + g.ss1, gw = ww0 * 4 + 2 * k + g.ss2;
    gd -= gd >= g.Dp ? g.Dp : 0;
    gh -= gh >= g.Hp ? g.Hp : 0;
    gw -= gw >= g.Wp ? g.Wp : 0;
    Piece pc;
    pc.lbase = c * TCS + pr * TRS + 2 * k;
    pc.gbase = active && gd < g.D ? (c * (int)sc + gd * (int)st + gh * g.W + gw) * 4 : OOB;
    return pc;
  };
  const int gstep = CPI * (int)sc * 4;  // bytes per piece index
  auto goff_of = [&](const Piece& pc, int i) __attribute__((always_inline)) {
    return pc.gbase == OOB ? OOB : pc.gbase + i * gstep;
  };
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  if (TILE) {
    u32x2 pv[PPW];
    const Piece pc = piece_base(lane);
#pragma unroll
    for (int i = 0; i < PPW; ++i) pv[i] = __builtin_amdgcn_raw_buffer_load_b64(rs_x, goff_of(pc, i), 0, 0);
#pragma unroll
    for (int i = 0; i < PPW; ++i) *reinterpret_cast<u32x2*>(tileL + pc.lbase + i * CPI * TCS) = pv[i];
    __syncthreads();
  }
  // the lane's token in the tile: frame td, row th, column 4 (window in the workgroup) + tw
  const int tpos = ((tk >> 4) * 4 + ((tk >> 2) & 3)) * TRS + 4 * (wave >> 1) + (tk & 3);

  // ---- 1. channel LayerNorm into register fragments ----
  const float sq0 = wsc[0] * q_scale, sk0 = wsc[1], sv0 = wsc[2], csm = wsc[4];
  const int vpro = valid ? (int)((8 * h * sc + pos) * 4) : OOB;  // channel 8h + (16k + e)
  int bad = 0;
  h8 xh[KS], xl[KS];
  float gi = 1.f;
  {
    float xv[KS][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xv[k][e] = TILE ? tileL[(16 * k + 8 * h + e) * TCS + tpos] : ldb(rs_x, vpro, (int)((16 * k + e) * sc * 4));
        s += xv[k][e];
      }
    s = xh_sum(s);
    const float m1 = s / C;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = xv[k][e] - m1; v += d * d; }
    v = xh_sum(v);
    // padded tokens normalise to 0 through a 0 factor (stw_x3.hip: no select per element); packed
    // pairs, the same operation order as the scalar ((x - m) rv) gamma
    const float rv = (1.f / sqrtf(v / C + 1e-5f)) * (valid ? 1.f : 0.f);
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        const f2 t = (pair(xv[k][e], xv[k][e + 1]) - splat(m1)) * splat(rv) *
                     pair(ldb(rs_g, 32 * h, (16 * k + e) * 4), ldb(rs_g, 32 * h, (16 * k + e + 1) * 4));
        xv[k][e] = t.x; xv[k][e + 1] = t.y;
      }
    scale_split<KS>(xv, xh, xl, gi, bad);
  }
  const float sq = sq0 * gi, sk = sk0 * gi, sv = sv0 * gi;

  // ---- 2. the 64-token core ----
  f32x16 pacc[CT];
#pragma unroll
  for (int i = 0; i < CT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) pacc[i][r] = 0.f;
  unit_loop<C, DH, NW, BF>(wsm, wpk, xch, wave, lane, h, tk, active, valid, rs_mb, mb_lane, mb_wave, xh, xl, sq, sk, sv,
                           csm, rcos, rsin, pacc, bad);
  if (bad) atomicOr(range_flag, 2);
  // ---- 3. bias + residual, in place (row cu + 4h of register r) ----
  if (TILE) {
    // Y + bias into the tile (its exchange alias is free once every wave is past the loop), then
    // the tile's 8-B pieces + the residual leave as the prologue's coalesced pieces; padded
    // frames' offsets lie past the extent (stores dropped). The sum order is the per-lane
    // path's: (Y + bias) + x.
    const float spj = wsc[3];
    const auto rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bp), 0, C * 4, 0x00020000);
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const int cu = ct * 32 + (r & 3) + 8 * (r >> 2);  // r + 1: row cu + 1
        const f2 y = pair(pacc[ct][r], pacc[ct][r + 1]) * splat(spj) +
                     pair(ldb(rs_b, 16 * h, cu * 4), ldb(rs_b, 16 * h, (cu + 1) * 4));
        tileL[(cu + 4 * h) * TCS + tpos] = y.x;
        tileL[(cu + 1 + 4 * h) * TCS + tpos] = y.y;
      }
    __syncthreads();
    u32x2 xr[PPW];
    // an opaque lane id: the two offsets recomputed here rather than kept live through the unit
    // loop from the prologue (hipcc would CSE them)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const Piece pc = piece_base(ln);
#pragma unroll
    for (int i = 0; i < PPW; ++i) xr[i] = __builtin_amdgcn_raw_buffer_load_b64(rs_x, goff_of(pc, i), 0, 0);
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const u32x2 y = *reinterpret_cast<const u32x2*>(tileL + pc.lbase + i * CPI * TCS);
      const f2 sum2 = __builtin_bit_cast(f2, y) + __builtin_bit_cast(f2, xr[i]);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, sum2), rs_x, goff_of(pc, i), 0, 0);
    }
  } else if (valid) {
    const float spj = wsc[3];
    const int vex = (int)((4 * h * sc + pos) * 4);
    const auto rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bp), 0, C * 4, 0x00020000);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cu = ct * 32 + (r & 3) + 8 * (r >> 2);
        const float pb = ldb(rs_b, 16 * h, cu * 4);
        const float xv = ldb(rs_x, vex, (int)(cu * sc * 4));
        const float res = (pacc[ct][r] * spj + pb) + xv;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(res), rs_x, vex, (int)(cu * sc * 4), 0);
      }
  }
}

// The TILE path's geometry (kernel note): 4x4x4 windows without H / W padding, W a multiple of 16
// (whole 4-window groups per window row), 8-B aligned rows; EXTDM_STW64_NO_TILE=1 forces the
// per-lane path (A/B)
bool stw64_tile_ok(const View& x, const AttnGeom& g, int groups) {
  static const bool off = env_flag("EXTDM_STW64_NO_TILE");
  return !off && x.C == 64 && g.ws0 == 4 && g.ws1 == 4 && g.ws2 == 4 && g.H == g.Hp && g.W == g.Wp && g.W % 16 == 0 &&
         groups % 4 == 0 && x.st == (long)x.H * x.W && x.sc % 2 == 0 && x.sb % 2 == 0 && x.st % 2 == 0 &&
         ((uintptr_t)x.p & 7) == 0;
}

template <int C, int DH, int NW, bool BF>
void launch(hipStream_t s, const View& x, const AttnGeom& g, int groups, const float* gamma, const void* wpk,
            const float* wsc, const float* bp, const float* mbias, int npat, const float* rcos, const float* rsin,
            float q_scale) {
  constexpr bool TILE_OK = C == 64 && NW == 8;
  const bool tile = TILE_OK && stw64_tile_ok(x, g, groups);
  const size_t tileb = (size_t)C * (16 * (2 * NW + 4) + 4) * sizeof(float);  // TCS floats per channel
  const size_t lds = attn64_lds<C, NW, BF>(tile ? tileb : 0);
  allow_full_lds<&stw64_x3_kernel<C, DH, NW, BF, false>, &stw64_x3_kernel<C, DH, NW, BF, TILE_OK>>();
  const int total = x.B * groups;
  // EXTDM_STW64_XCD=0: dispatch order (A/B)
  static const bool xcd = [] { const char* v = getenv("EXTDM_STW64_XCD"); return !(v && v[0] == '0'); }();
  int remap;
  const int grid = xcd_grid(total, NW, xcd, remap);
  note_kernel("stw64_x3_kernel<%d, %d, %d, %s, %s>", C, DH, NW, BF ? "true" : "false", tile ? "true" : "false");
  auto kern = tile ? &stw64_x3_kernel<C, DH, NW, BF, TILE_OK> : &stw64_x3_kernel<C, DH, NW, BF, false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, s, x.p, x.sb, x.sc, x.st, g, gamma,
                     reinterpret_cast<const _Float16*>(wpk), wsc, bp, mbias, npat, rcos, rsin, q_scale, groups, total,
                     x3_range_ptr(), remap);
}

template <int DH, bool BF>
bool dispatch(hipStream_t s, const View& x, const AttnGeom& g, int groups, const float* gamma, const void* wpk,
              const float* wsc, const float* bp, const float* mbias, int npat, const float* rcos, const float* rsin,
              float q_scale) {
  // C = 64: 8 waves (two per SIMD, 128 KB of LDS); C = 128: 4 waves (one per SIMD: its
  // registers), ring 128 KB + exchange 32 KB = the whole 160 KB
  if (x.C == 64) launch<64, DH, 8, BF>(s, x, g, groups, gamma, wpk, wsc, bp, mbias, npat, rcos, rsin, q_scale);
  else if (x.C == 128) launch<128, DH, 4, BF>(s, x, g, groups, gamma, wpk, wsc, bp, mbias, npat, rcos, rsin, q_scale);
  else return false;
  return true;
}

}  // namespace

bool stw64_x3_supported(int C, int ntok, int dim_head, int heads) {
  return heads == 8 && (C == 64 || C == 128) && ntok <= 64 && (dim_head == 32 || dim_head == 16) &&
         attn_x3_unit_halves(C) == (C == 64 ? UnitLayout<64>::HALVES : UnitLayout<128>::HALVES);
}

bool stw64_x3(hipStream_t s, const View& x, const AttnGeom& g, int heads, int dim_head, const float* gamma,
              const void* wpk, const float* wsc, const float* bp, const float* mbias, int npat, const float* rcos,
              const float* rsin, float q_scale, bool bf16) {
  const int N = g.ws0 * g.ws1 * g.ws2;
  if (!stw64_x3_supported(x.C, N, dim_head, heads)) return false;
  // 31-bit buffer offsets per sample
  if (((long)(x.C - 1) * x.sc + (long)g.D * x.st) * 4 >= (1L << 30) || x.st != (long)x.H * x.W) return false;
  const int groups = (g.Dp / g.ws0) * (g.Hp / g.ws1) * (g.Wp / g.ws2);
  if (dim_head == 32) {
    return bf16 ? dispatch<32, true>(s, x, g, groups, gamma, wpk, wsc, bp, mbias, npat, rcos, rsin, q_scale)
                : dispatch<32, false>(s, x, g, groups, gamma, wpk, wsc, bp, mbias, npat, rcos, rsin, q_scale);
  }
  return bf16 ? dispatch<16, true>(s, x, g, groups, gamma, wpk, wsc, bp, mbias, npat, rcos, rsin, q_scale)
              : dispatch<16, false>(s, x, g, groups, gamma, wpk, wsc, bp, mbias, npat, rcos, rsin, q_scale);
}

}  // namespace extdm
