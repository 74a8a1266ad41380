"""CPU check of the weight layouts (csrc/pack.cpp): tests/pack_driver.cpp, built with
AddressSanitizer and UBSan, packs seeded weights; every buffer is recomputed here in numpy from
the index formula of its layout comment in csrc/pack.h -- one gather per output element, not the
C++ loop nest -- and compared byte for byte. The fp64 compositions (x-branch classes, phase
weights) are restated with the same summation order per element and compared bit for bit too.

Every weight set carries three special rows: row 0 all zero (exponent 0, zero fragments), row 1
with largest magnitude exactly 2^-1 (the frexp boundary), row 2 with a value whose scaled lo
half is subnormal in fp16."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_fea_phase_math import up_inf, up_true

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, '140-extdm-distribution-extrapolation-diffusion-model-for-video-prediction_amd', 'csrc')
f32 = np.float32


def _compiler():
    for c in ('/opt/rocm/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++')):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope='module')
def out(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('pack')
    exe = str(d / 'pack_driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', CSRC, os.path.join(REPO, 'tests', 'pack_driver.cpp'),
                    os.path.join(CSRC, 'pack.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return lambda name, dt=np.float32: np.fromfile(str(d / (name + '.bin')), dtype=dt)


# ------------------------------------------------------------------ the driver's weights
def gen(n, seed):
    x, v = seed, np.empty(n, np.int64)
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        v[i] = (x >> 8) - 8388608
    return v.astype(f32) / f32(33554432.0)


def weights(M, rowlen, seed, outer=1):
    w = gen(outer * M * rowlen, seed).reshape(outer, M, rowlen)
    w[:, 0, :] = 0
    w[0, 1, 0] = 0.5
    w[0, 2, 1] = f32(1.2345e-6)
    return w if outer > 1 else w[0]


# ------------------------------------------------------------------------- primitives
def row_exp(mx):
    """e with mx * 2^e in [2^14, 2^15), 0 for mx == 0"""
    mx = np.asarray(mx, np.float64)
    e = np.where(mx > 0, 14 - np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 0).astype(np.int64)
    s = mx * np.exp2(e.astype(np.float64))
    assert np.all((mx == 0) | ((s >= 2.0 ** 14) & (s < 2.0 ** 15)))
    return e


def hilo(v):
    """v float32 -> (hi, lo) float16, hi = fp16(v), lo = fp16(v - hi)"""
    v = v.astype(f32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(f32)).astype(np.float16)


def same(got, want):
    want = np.ascontiguousarray(want)
    assert got.size == want.size, (got.size, want.size)
    assert got.tobytes() == want.tobytes(), 'differs at flat index %s' % np.flatnonzero(
        got.view(np.uint8) != want.reshape(-1).view(np.uint8))[:8]


def pow2(e):
    return np.exp2(np.asarray(e, np.float64)).astype(f32)


def frags(dense, present, bm):
    """The generic fragment layout [par][mtile][ktile][step][m32][hi|lo][lane][8] of dense
    [npar][M][K] (present: which elements exist); returns (fragments, rs)."""
    npar, M, K = dense.shape
    mt, nkt, m32 = -(-M // bm), -(-K // 32), bm // 32
    e = row_exp(np.abs(np.where(present, dense, 0)).transpose(1, 0, 2).reshape(M, -1).max(axis=1))
    par, mtile, kt, st, q, hl, lane, el = np.indices((npar, mt, nkt, 2, m32, 2, 64, 8))
    m = mtile * bm + q * 32 + (lane & 31)
    k = kt * 32 + st * 16 + 8 * (lane >> 5) + el
    ok = (m < M) & (k < K)
    mc, kc = np.minimum(m, M - 1), np.minimum(k, K - 1)
    ok &= present[par, mc, kc]
    hi, lo = hilo(dense[par, mc, kc] * pow2(e)[mc])
    return np.where(ok, np.where(hl == 0, hi, lo), np.float16(0)), pow2(-e)


def special_rows_checked(g, rs, bm=64):
    """row 0: rs = 1 and zero fragments; row 1 (max 2^-1): rs = 2^-15"""
    assert rs[0] == 1.0 and rs[1] == 2.0 ** -15
    assert not g.reshape(-1, bm // 32, 2, 64, 8)[:, 0, :, 0, :].any()


# ------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize('name,ci,kk,seed', [('gemm3x3', 8, 9, 1), ('gemm_ci6', 6, 9, 2), ('gemm1x1', 8, 1, 3)])
def test_gemm_plane_and_fragments(out, name, ci, kk, seed):
    M, K, bm = 40, ci * kk, 64
    w = weights(M, K, seed)
    Mpad, Kpad = 64, -(-K // 16) * 16
    same(out(name + '.dims'), np.array([Mpad, Kpad, -(-K // 32)], f32))
    plane = np.zeros((Kpad, Mpad), f32)
    plane[:K, :M] = w.T  # A[k][m]
    same(out(name + '.plane'), plane)
    g, rs = frags(w[None], np.ones((1, M, K), bool), bm)
    same(out(name + '.g', np.float16), g)
    same(out(name + '.rs'), rs)
    special_rows_checked(g, rs)
    gt = out(name + '.gt', np.float16)
    if ci % 8 == 0 and kk > 1 and 32 % kk != 0:
        # tap-major: k = tap * ci + c
        wt = w.reshape(M, ci, kk).transpose(0, 2, 1).reshape(1, M, K)
        same(gt, frags(wt, np.ones((1, M, K), bool), bm)[0])
    else:
        assert gt.size == 0


def test_lo_half_subnormal_in_the_special_row(out):
    # row 2, k = 1 of the 3x3 GEMM: mtile 0, ktile 0, step 0, m32 0, lane 2, e 1
    g = out('gemm3x3.g', np.float16).reshape(1, 3, 2, 2, 2, 64, 8)
    lo = g[0, 0, 0, 0, 1, 2, 1]
    assert lo != 0 and abs(float(lo)) < 2.0 ** -14


def test_deconv_parities(out):
    ci, co, bm = 3, 40, 64
    w = weights(co, 16, 4, outer=ci).reshape(ci, co, 4, 4)
    dense = np.zeros((4, co, ci * 4), f32)
    for par in range(4):
        py, px = par >> 1, par & 1
        for ky in range(2):
            for kx in range(2):  # parity (py,px) tap (ky',kx') uses W[..][3-py-2ky'][3-px-2kx']
                dense[par, :, np.arange(ci) * 4 + ky * 2 + kx] = w[:, :, 3 - py - 2 * ky, 3 - px - 2 * kx]
    plane = np.zeros((4, 16, 64), f32)
    plane[:, :12, :co] = dense.transpose(0, 2, 1)
    same(out('deconv.plane'), plane)
    g, rs = frags(dense, np.ones(dense.shape, bool), bm)
    same(out('deconv.g', np.float16), g)
    same(out('deconv.rs'), rs)
    special_rows_checked(g, rs)
    assert out('deconv.gt', np.float16).size == 0


def test_i3d_unit_and_stem(out):
    # unit: k = tap * Cpad + ci, channels past Cin absent
    M, Cin, KS, Cpad = 40, 12, 3, 16
    w = weights(M, Cin * 27, 5).reshape(M, Cin, 27)
    dense = np.zeros((1, M, 27, Cpad), f32)
    dense[0, :, :, :Cin] = w.transpose(0, 2, 1)
    present = np.zeros(dense.shape, bool)
    present[..., :Cin] = True
    g, rs = frags(dense.reshape(1, M, -1), present.reshape(1, M, -1), 64)
    same(out('unit3d.g', np.float16), g)
    same(out('unit3d.rs'), rs)
    special_rows_checked(g, rs)
    # stem: k = (kt * 7 + ky) * 24 + kx * 3 + ci, j = kx * 3 + ci >= 21 absent
    M, Cin = 64, 3
    w = weights(M, 3 * 343, 6).reshape(M, Cin, 49, 7)  # [m][ci][(kt, ky)][kx]
    dense = np.zeros((1, M, 49, 24), f32)
    dense[0, :, :, :21] = w.transpose(0, 2, 3, 1).reshape(M, 49, 21)
    present = np.zeros(dense.shape, bool)
    present[..., :21] = True
    g, rs = frags(dense.reshape(1, M, -1), present.reshape(1, M, -1), 64)
    same(out('stem.g', np.float16), g)
    same(out('stem.rs'), rs)
    special_rows_checked(g, rs)
    same(out('stem.dims'), np.array([27 * 16 // 32 + 1, 49 * 24 // 32 + 1], f32))


# ------------------------------------------------------------------- direct-conv layouts
@pytest.mark.parametrize('name,ks,ci,ng,seed', [('x3_k3', 3, 24, 1, 7), ('x3_k1', 1, 40, 2, 8)])
def test_pack_x3(out, name, ks, ci, ng, seed):
    co, bm = 40, 64
    w = weights(co, ci * ks * ks, seed).reshape(co, ci, ks, ks)
    ncgb, mt, m32 = -(-ci // (16 * ng)), 1, bm // 32
    e = row_exp(np.abs(w).reshape(co, -1).max(axis=1))
    # [mtile][cb][ky][g][kx][m32][hi|lo][lane][8]: row m = mtile*BM + m32*32 + lc, channel cb*16NG + g*16 + 8h + e
    mtile, cb, ky, g_, kx, q, hl, lane, el = np.indices((mt, ncgb, ks, ng, ks, m32, 2, 64, 8))
    m = mtile * bm + q * 32 + (lane & 31)
    c = cb * 16 * ng + g_ * 16 + 8 * (lane >> 5) + el
    ok = (m < co) & (c < ci)
    mc, cc = np.minimum(m, co - 1), np.minimum(c, ci - 1)
    hi, lo = hilo(w[mc, cc, ky, kx] * pow2(e)[mc])
    a = np.where(ok, np.where(hl == 0, hi, lo), np.float16(0))
    same(out(name + '.a', np.float16), a)
    same(out(name + '.rs'), pow2(-e))
    assert out('x3.dims')[0 if ks == 3 else 1] == ncgb
    assert pow2(-e)[0] == 1.0 and pow2(-e)[1] == 2.0 ** -15 and not a[:, :, :, :, :, 0, :, 0, :].any()


def test_pack_halo(out):
    ks, co, bm, ch, ci = 3, 40, 64, 4, 10
    kk = ks * ks
    w = weights(co, ci * kk, 9).reshape(co, ci, kk)
    stages = -(-ci // (2 * ch))
    # [mtile][stage][step = cp*kk + tap][half][BM], input channel = stage*2CH + half*CH + cp
    mtile, st, cp, tap, half, mm = np.indices((1, stages, ch, kk, 2, bm))
    m, c = mtile * bm + mm, st * 2 * ch + half * ch + cp
    ok = (m < co) & (c < ci)
    a = np.where(ok, w[np.minimum(m, co - 1), np.minimum(c, ci - 1), tap], f32(0))
    same(out('halo.a'), a)
    assert out('halo.dims')[0] == stages


@pytest.mark.parametrize('name,co,cot,seed', [('narrow3', 3, 3, 10), ('narrow21', 21, 8, 11)])
def test_pack_narrow(out, name, co, cot, seed):
    ci, kk = 5, 49
    w = weights(co, ci * kk, seed).reshape(co, ci, kk)
    ng, cotp = -(-co // cot), (cot + 3) // 4 * 4
    # [group][ci][tap][cot rounded up to 4], m = group * cot + o
    g_, c, tap, o = np.indices((ng, ci, kk, cotp))
    m = g_ * cot + o
    ok = (o < cot) & (m < co)
    same(out(name + '.a'), np.where(ok, w[np.minimum(m, co - 1), c, tap], f32(0)))


def test_time3_reorder_and_channel_split(out):
    w = gen(5 * 3 * 3 * 9, 12).reshape(5, 3, 3, 9)  # [co][ci][kt][kk]
    same(out('time3'), w.transpose(0, 2, 1, 3))      # W'[co][z*ci + c] = W[co][c][z]
    w = gen(6 * 8 * 49, 13).reshape(6, 8, 49)
    same(out('split.x'), w[:, :3])
    same(out('split.f'), w[:, 3:])


def test_pack_conv7c3(out):
    Cm, M32 = 40, 2
    w = weights(Cm, 147, 14).reshape(Cm, 3, 7, 7)
    e = row_exp(np.abs(w).reshape(Cm, -1).max(axis=1))
    # [kstep = (ci, row pair)][m32][hi|lo][lane][8]: dy = 2*pair + (lane >> 5), dx = e, zero for dy or dx = 7
    ci, pair, q, hl, lane, el = np.indices((3, 4, M32, 2, 64, 8))
    m, dy = q * 32 + (lane & 31), 2 * pair + (lane >> 5)
    ok = (m < Cm) & (dy < 7) & (el < 7)
    mc = np.minimum(m, Cm - 1)
    hi, lo = hilo(w[mc, ci, np.minimum(dy, 6), np.minimum(el, 6)] * pow2(e)[mc])
    same(out('conv7.g', np.float16), np.where(ok, np.where(hl == 0, hi, lo), np.float16(0)))
    rs = np.zeros(64, f32)
    rs[:Cm] = pow2(-e)
    same(out('conv7.rs'), rs)
    assert rs[0] == 1.0 and rs[1] == 2.0 ** -15


# --------------------------------------------------------------------- fp64 compositions
def test_xpath_classes(out):
    Cm, Co, Cin, L, M32, MP = 8, 40, 13, 16, 2, 64
    wn = weights(Cm, 147, 15).reshape(Cm, 3, 7, 7).astype(np.float64)
    bn = gen(Cm, 16).astype(np.float64)
    wi = weights(Co, Cin * 49, 17).reshape(Co, Cin, 7, 7).astype(np.float64)
    bi = gen(Co, 18).astype(np.float64)
    # V[m][ci][a][b][e][f] = sum_c' Wa[m][c'][a][b] Wn[c'][ci][e][f]; U[m][a][b] = sum_c' Wa bn (c' ascending)
    V, U = np.zeros((Co, 3, 7, 7, 7, 7)), np.zeros((Co, 7, 7))
    for c in range(Cm):
        V += wi[:, c, None, :, :, None, None] * wn[c][None, :, None, None, :, :]
        U += wi[:, c] * bn[c]

    def taps(cls1):  # tap a of a class (offset a - 3 from p) is valid iff p + a - 3 lies in [0, L)
        p = cls1 if cls1 < 3 else (3 if cls1 == 3 else L - 7 + cls1)
        return [a for a in range(7) if cls1 == 3 or 0 <= p + a - 3 < L]

    g = np.zeros((49, 3, 13, M32, 2, 64, 8), np.float16)
    rs, cb = np.zeros((49, MP), f32), np.zeros((49, MP), f32)
    patterns = set()
    for cls in range(49):
        K, cbv = np.zeros((Co, 3, 13, 13)), bi.copy()
        ta, tb = taps(cls // 7), taps(cls % 7)
        patterns.add((tuple(ta), tuple(tb)))
        for a in ta:  # each element of K and cb sums its (a, b) terms in ascending (a, b)
            for b in tb:
                cbv += U[:, a, b]
                K[:, :, a:a + 7, b:b + 7] += V[:, :, a, b]
        cb[cls, :Co] = cbv.astype(f32)
        e = row_exp(np.abs(K).reshape(Co, -1).max(axis=1))
        rs[cls, :Co] = pow2(-e)
        # [class][kstep = (ci, dy)][m32][hi|lo][lane][8]: row m = m32*32 + (lane & 31), dx = 8*(lane >> 5) + e
        ci, dy, q, hl, lane, el = np.indices((3, 13, M32, 2, 64, 8))
        m, dx = q * 32 + (lane & 31), 8 * (lane >> 5) + el
        ok = (m < Co) & (dx < 13)
        mc = np.minimum(m, Co - 1)
        v = (K * np.exp2(e.astype(np.float64))[:, None, None, None]).astype(f32)
        hi, lo = hilo(v[mc, ci, dy, np.minimum(dx, 12)])
        g[cls] = np.where(ok, np.where(hl == 0, hi, lo), np.float16(0))
    assert len(patterns) == 49
    same(out('xpath.cb'), cb)
    same(out('xpath.rs'), rs)
    same(out('xpath.g', np.float16), g)
    assert np.all(rs[:, 0] == 1.0) and not g[:, :, :, 0, :, 0, :].any()


def test_fea_phase_weights(out):
    Co, Cf, n = 8, 16, 16
    W = weights(Co, Cf * 49, 19).reshape(Co, Cf, 7, 7).astype(np.float64)
    # interior composition A[p][l][d]: weight of tap l (F[m - 2 + l]) in row 2m + p + d - 3
    A = np.array([[[up_inf(2 * 8 + p + d - 3, 8 - 2 + l) for d in range(7)] for l in range(5)] for p in range(2)])
    delta = lambda r, ke: up_true(r, ke, n) - up_inf(r, ke)  # noqa: E731
    # k5 [ph = 2 py + px][co][ci][ly][lx] = sum_dy A[py][ly][dy] (sum_dx W[dy][dx] A[px][lx][dx]), ascending
    k5 = np.zeros((2, 2, Co, Cf, 5, 5))
    for px in range(2):
        t = np.zeros((Co, Cf, 7, 5))
        for dx in range(7):
            t += W[:, :, :, dx, None] * A[px][:, dx]
        for py in range(2):
            for dy in range(7):
                k5[py, px] += A[py][:, dy][:, None] * t[:, :, dy, None, :]
    same(out('fea.k5'), k5.astype(f32))
    # edge lines, row m = co * 8 + (d*2 + py)*2 + px: sum over (dy, dx) ascending of
    # W[dy][dx] * (delta[dy] A[px][l][dx]) (pair 0, rows) or W * (delta[dx] A[py][l][dy]) (pair 1, columns)
    R, RP = 8 * Co, 128
    ws = np.zeros((2, 2, Co, 2, 2, 2, Cf, 5))
    for pair in range(2):
        for sd in range(2):
            ke, base = (n - 1, 2 * n - 4) if sd else (0, 0)
            for d in range(2):
                for py in range(2):
                    for px in range(2):
                        e0 = base + 2 * d + (px if pair else py)
                        ip = py if pair else px
                        dl = [delta(e0 + k - 3, ke) for k in range(7)]
                        s = np.zeros((Co, Cf, 5))
                        for dy in range(7):
                            for dx in range(7):
                                s += W[:, :, dy, dx, None] * (dl[dx] * A[ip][:, dy] if pair else dl[dy] * A[ip][:, dx])
                        ws[pair, sd, :, d, py, px] = s
    ws = ws.reshape(4, R, Cf, 5)
    e = row_exp(np.abs(ws).reshape(4, R, -1).max(axis=2))
    scale = np.ones((4, RP), f32)
    scale[:, :R] = pow2(-e)
    same(out('fea.side_scale'), scale)
    # [pair, side][mtile][cb][tap][m32][hi|lo][lane][8]: row m = mtile*128 + m32*32 + (lane & 31), ci = cb*16 + 8*(lane >> 5) + e
    ps, mtile, cb, l, q, hl, lane, el = np.indices((4, 1, Cf // 16, 5, 4, 2, 64, 8))
    m, ci = mtile * 128 + q * 32 + (lane & 31), cb * 16 + 8 * (lane >> 5) + el
    ok = m < R
    mc = np.minimum(m, R - 1)
    v = (ws * np.exp2(e.astype(np.float64))[:, :, None, None]).astype(f32)
    hi, lo = hilo(v[ps, mc, ci, l])
    same(out('fea.side', np.float16), np.where(ok, np.where(hl == 0, hi, lo), np.float16(0)))
    # corners [corner = 2 (bottom) + (right)][ci][co][p = yy * 4 + xx] = sum W * dy * dx, (dy, dx) ascending
    cw = np.zeros((4, Cf, Co, 16))
    for c in range(4):
        ky, kx = (n - 1 if c >> 1 else 0), (n - 1 if c & 1 else 0)
        yb, xb = (2 * n - 4 if c >> 1 else 0), (2 * n - 4 if c & 1 else 0)
        for p in range(16):
            s = np.zeros((Co, Cf))
            for dy in range(7):
                for dx in range(7):
                    s += W[:, :, dy, dx] * delta(yb + p // 4 + dy - 3, ky) * delta(xb + p % 4 + dx - 3, kx)
            cw[c, :, :, p] = s.T
    same(out('fea.corner'), cw.astype(f32))


# ------------------------------------------------------------------------------ attention
def exp1(v):
    """e with v * 2^e in [1, 2), clamped to +-30; 0 for v == 0"""
    return 0 if not v > 0 else int(min(30, max(-30, -np.floor(np.log2(v)))))


@pytest.mark.parametrize('name,dim_head,seed', [('attn32', 32, 20), ('attn16', 16, 30)])
def test_attention_packs(out, name, dim_head, seed):
    C = hid = 64
    units, KS, CT = hid // 32, C // 16, C // 32
    wq, wp = weights(3 * hid, C, seed), weights(C, hid, seed + 1)
    ng, nb = gen(C, seed + 2), gen(C, seed + 3)
    # fused fp32 layouts: [unit][C/2][q|k|v][lane] / [ctile][K/2][lane], row 32 u + (lane & 31), column 2 s + (lane >> 5)
    u, s2, wh, lane = np.indices((units, C // 2, 3, 64))
    same(out(name + '.qkv'), wq[wh * hid + u * 32 + (lane & 31), 2 * s2 + (lane >> 5)])
    tl, s2, lane = np.indices((C // 32, hid // 2, 64))
    same(out(name + '.proj'), wp[tl * 32 + (lane & 31), 2 * s2 + (lane >> 5)])
    # f16x3: each matrix scaled by one power of two (largest |w| -> [2^14, 2^15))
    eq = [int(row_exp(np.abs(wq[m * hid:(m + 1) * hid]).max())) for m in range(3)]
    ep = int(row_exp(np.abs(wp).max()))
    a = np.zeros((units, 3 * KS + 2 * CT, 2, 64, 8), np.float16)
    u, m, s, hl, lane, el = np.indices((units, 3, KS, 2, 64, 8))
    hi, lo = hilo(wq[m * hid + u * 32 + (lane & 31), 16 * s + 8 * (lane >> 5) + el] * pow2(eq)[m])
    a[:, :3 * KS] = np.where(hl == 0, hi, lo).reshape(units, 3 * KS, 2, 64, 8)
    # projection: row ct*32 + lc, hid u*32 + 16s' + 8(e>>2) + 4h + (e&3)
    u, ct, s, hl, lane, el = np.indices((units, CT, 2, 2, 64, 8))
    hi, lo = hilo(wp[ct * 32 + (lane & 31), u * 32 + 16 * s + 8 * (el >> 2) + 4 * (lane >> 5) + (el & 3)] * pow2(ep))
    a[:, 3 * KS:] = np.where(hl == 0, hi, lo).reshape(units, 2 * CT, 2, 64, 8)
    same(out(name + '.a', np.float16), a)
    # exponents: channel scales (|g| + |b|) 2^e_x / 4, row norms of q * q_scale, k, v to [2^4, 2^5) / [2^2, 2^3)
    q_scale = f32(1.0) / np.sqrt(f32(dim_head))
    for bias, buf in ((nb, '.sc'), (None, '.sc_nobias')):
        sx = np.abs(ng.astype(np.float64)) + (np.abs(nb.astype(np.float64)) if bias is not None else 0.0)
        ex = exp1(sx.max())
        em = []
        for m in range(3):
            wsc = wq[m * hid:(m + 1) * hid].astype(np.float64) * (sx * 2.0 ** ex) * 0.25
            n2 = np.zeros(hid)
            for c in range(C):  # ascending c, as the packer sums
                n2 += wsc[:, c] * wsc[:, c]
            em.append(exp1(np.sqrt(n2).max() * (float(q_scale) if m == 0 else 1.0)) + (4 if m < 2 else 2))
        sc = np.array([2.0 ** (-eq[0] + em[0]), 2.0 ** (-eq[1] + em[1]), 2.0 ** (-eq[2] + em[2]),
                       2.0 ** (-ep - em[2] - 4), 1.4426950408889634 * 2.0 ** -(em[0] + em[1])]).astype(f32)
        same(out(name + buf), sc)
        if bias is not None:
            same(out(name + '.s2'), np.array([2.0 ** (em[0] + em[1])], f32))


# ------------------------------------------------------------------------- BatchNorm folds
def test_bn_folds(out):
    w, b, rm = gen(7, 40), gen(7, 41), gen(7, 42)
    rv = np.abs(gen(7, 43))
    rv[3] = 0
    # fp32, rounded after every operation
    inv = f32(1.0) / np.sqrt(rv + f32(1e-5), dtype=f32)
    a = (inv * w).astype(f32)
    same(out('bn32.a'), a)
    same(out('bn32.b'), (b - (rm * a).astype(f32)).astype(f32))
    # fp64, eps 1e-5
    s = w.astype(np.float64) / np.sqrt(rv.astype(np.float64) + 1e-5)
    same(out('bn64.a'), s.astype(f32))
    same(out('bn64.b'), (b.astype(np.float64) - rm.astype(np.float64) * s).astype(f32))
