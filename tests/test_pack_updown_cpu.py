"""CPU check of the two-tap weight layouts of the stride-2 convs (csrc/pack.cpp pack_x3_deconv /
pack_x3_down, read by conv_x3.hip's TT mode): tests/pack_updown_driver.cpp, built with
AddressSanitizer and UBSan, packs seeded weights with the three special rows of test_pack_cpu.py.

1. Every packed buffer is recomputed in numpy from the index formula of the layout comment in
   csrc/pack.h, one gather per output element, and compared byte for byte.
2. The kernel's index arithmetic (pixel tile, zero-haloed tile position, tap origin, phase store;
   conv_x3.hip) is restated in numpy on the unpacked hi + lo weights, and the whole conv compared
   with the fp64 conv_transpose2d / conv2d of the original weights. The only difference is the
   representation error of hi + lo: 2^-22 relative per weight (two 11-bit halves), or 2^-25 of the
   row's scaled unit where lo is subnormal; the bound below is twice that, summed over the taps."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.test_pack_cpu import CSRC, REPO, _compiler, f32, hilo, pow2, row_exp, same, weights

# (Cin, Cout, bm, seed) in the driver's order
CASES = [(16, 16, 64, 50), (16, 80, 64, 51), (16, 80, 128, 52), (32, 16, 64, 53), (32, 80, 64, 54), (32, 80, 128, 55)]
IDS = ['ci%d-co%d-bm%d' % c[:3] for c in CASES]


@pytest.fixture(scope='module')
def out(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('pack_updown')
    exe = str(d / 'pack_updown_driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', CSRC, os.path.join(REPO, 'tests', 'pack_updown_driver.cpp'),
                    os.path.join(CSRC, 'pack.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return lambda name, dt=np.float32: np.fromfile(str(d / (name + '.bin')), dtype=dt)


def up_weight(ci, co, seed):
    return weights(co, 16, seed, outer=ci).reshape(ci, co, 4, 4)


def down_weight(ci, co, seed):
    return weights(co, ci * 16, seed + 100).reshape(co, ci, 4, 4)


# ------------------------------------------------------------------ 1. the layouts, byte for byte
@pytest.mark.parametrize('ci,co,bm,seed', CASES, ids=IDS)
def test_deconv_two_tap_layout(out, ci, co, bm, seed):
    w = up_weight(ci, co, seed)
    mtc, ncb, m32 = -(-co // bm), ci // 16, bm // 32
    e = row_exp(np.abs(w).transpose(1, 0, 2, 3).reshape(co, -1).max(axis=1))
    # [mtile = ph*MTC + ct][cb][ky'][kx'][m32][hi|lo][lane][8]: row co = ct*bm + m32*32 + lc, channel
    # 16cb + 8h + e, element W[ci][co][3 - py - 2ky'][3 - px - 2kx']
    mtile, cb, ky, kx, q, hl, lane, el = np.indices((4 * mtc, ncb, 2, 2, m32, 2, 64, 8))
    ph, ct = mtile // mtc, mtile % mtc
    m, c = ct * bm + q * 32 + (lane & 31), cb * 16 + 8 * (lane >> 5) + el
    mc = np.minimum(m, co - 1)
    hi, lo = hilo(w[c, mc, 3 - (ph >> 1) - 2 * ky, 3 - (ph & 1) - 2 * kx] * pow2(e)[mc])
    a = np.where(m < co, np.where(hl == 0, hi, lo), np.float16(0))
    tag = 'up_%d_%d_%d' % (ci, co, bm)
    same(out(tag + '.g', np.float16), a)
    same(out(tag + '.rs'), pow2(-e))
    assert out(tag + '.n')[0] == ncb
    # special rows: row 0 zero (rs = 1, zero fragments in every phase), row 1 at the frexp boundary
    assert pow2(-e)[0] == 1.0 and pow2(-e)[1] == 2.0 ** -15
    assert not a[::mtc, :, :, :, 0, :, ::32, :].any()
    # row 2, W[0][2][0][1]: phase (1, 0) tap (1, 1), m-tile 2 MTC, lane 2, e 0 -- a subnormal lo half
    lo2 = a[2 * mtc, 0, 1, 1, 0, 1, 2, 0]
    assert lo2 != 0 and abs(float(lo2)) < 2.0 ** -14


@pytest.mark.parametrize('ci,co,bm,seed', CASES, ids=IDS)
def test_down_two_tap_layout(out, ci, co, bm, seed):
    w = down_weight(ci, co, seed)
    mt, ncb, m32 = -(-co // bm), ci // 16, bm // 32
    e = row_exp(np.abs(w).reshape(co, -1).max(axis=1))
    # [mtile = ct][cblk = q*ncb + cb][ky'][kx'][m32][hi|lo][lane][8]: row co = ct*bm + m32*32 + lc,
    # channel 16cb + 8h + e, element W[co][ci][2ky' + 1 - qy][2kx' + 1 - qx]
    mtile, cblk, ky, kx, q, hl, lane, el = np.indices((mt, 4 * ncb, 2, 2, m32, 2, 64, 8))
    qi, cb = cblk // ncb, cblk % ncb
    m, c = mtile * bm + q * 32 + (lane & 31), cb * 16 + 8 * (lane >> 5) + el
    mc = np.minimum(m, co - 1)
    hi, lo = hilo(w[mc, c, 2 * ky + 1 - (qi >> 1), 2 * kx + 1 - (qi & 1)] * pow2(e)[mc])
    a = np.where(m < co, np.where(hl == 0, hi, lo), np.float16(0))
    tag = 'down_%d_%d_%d' % (ci, co, bm)
    same(out(tag + '.g', np.float16), a)
    same(out(tag + '.rs'), pow2(-e))
    assert out(tag + '.n')[0] == 4 * ncb
    assert pow2(-e)[0] == 1.0 and pow2(-e)[1] == 2.0 ** -15
    assert not a[0, :, :, :, 0, :, ::32, :].any()
    # row 2, W[2][0][0][1]: ky = 0 -> (qy 1, ky' 0), kx = 1 -> (qx 0, kx' 0): phase 2, block 2 ncb
    lo2 = a[0, 2 * ncb, 0, 0, 0, 1, 2, 0]
    assert lo2 != 0 and abs(float(lo2)) < 2.0 ** -14


# ------------------------------------------- 2. the kernel's index arithmetic on hi + lo weights
def unpack(g, lead, bm):
    """fragments [lead...][ky'][kx'][m32][hi|lo][(h, lc)][8] -> hi + lo as fp64 [lead...][ky'][kx'][bm][16]"""
    a = g.astype(np.float64).reshape(lead + (2, 2, bm // 32, 2, 2, 32, 8)).sum(axis=-4)  # [.., m32, h, lc, e]
    return np.moveaxis(a, -3, -2).reshape(lead + (2, 2, bm, 16))


def tiles(P, H, W, bn):
    """The pixel tiles of x3_setup: (plane0, row0) per tile, and the tile's geometry"""
    TH = min(H, bn // W)
    NP = bn // (TH * W)
    assert bn % W == 0 and bn % (TH * W) == 0
    nrow = -(-H // TH)
    geo = dict(TH=TH, NP=NP, RS=W + 2, THK=TH + 2, XPOS=NP * (TH + 2) * (W + 2))
    return [((t // nrow) * NP, (t % nrow) * TH) for t in range(-(-P // NP) * nrow)], geo


def halo_tile(plane, P, H, W, plane0, row0, geo):
    """Zero-haloed tile [XPOS][C] of plane(q, iy, ix) -> [C]: position pos = (p*THK + rr)*RS + cc holds
    pixel (row0 + rr - 1, cc - 1) of plane plane0 + p, zero outside the image or past the last plane"""
    THK, RS = geo['THK'], geo['RS']
    pos = np.arange(geo['XPOS'])
    p, r2 = pos // (THK * RS), pos % (THK * RS)
    q, iy, ix = plane0 + p, row0 + r2 // RS - 1, r2 % RS - 1
    ok = (q < P) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    x = plane(np.where(ok, q, 0), np.where(ok, iy, 0), np.where(ok, ix, 0))
    return np.where(ok[:, None], x, 0.0)


def tile_pixels(bn, W, geo):
    n = np.arange(bn)
    p, r, c = n // (geo['TH'] * W), (n // W) % geo['TH'], n % W
    return p, r, c, (p * geo['THK'] + r) * geo['RS'] + c


def direct_up(g, rs, x, co, bm, bn):
    P, ci, H, W = x.shape
    mtc, ncb = -(-co // bm), ci // 16
    A = unpack(g, (4 * mtc, ncb), bm)
    out = np.full((P, co, 2 * H, 2 * W), np.nan)
    tl, geo = tiles(P, H, W, bn)
    p, r, c, bpos = tile_pixels(bn, W, geo)
    for plane0, row0 in tl:
        X = halo_tile(lambda q, iy, ix: x[q, :, iy, ix], P, H, W, plane0, row0, geo)
        for mtile in range(4 * mtc):
            ph, ct = mtile // mtc, mtile % mtc
            py, px = ph >> 1, ph & 1
            acc = np.zeros((bm, bn))
            for cb in range(ncb):
                for ky in range(2):
                    for kx in range(2):  # tap origin (py, px) inside the 3x3 window
                        acc += A[mtile, cb, ky, kx] @ X[bpos + (py + ky) * geo['RS'] + px + kx, 16 * cb:16 * cb + 16].T
            q, row, m = plane0 + p, row0 + r, ct * bm + np.arange(bm)
            okn, okm = (q < P) & (row < H), m < co
            out[q[okn][None, :], m[okm][:, None], (2 * row + py)[okn][None, :], (2 * c + px)[okn][None, :]] = \
                (acc * np.pad(rs, (0, mtc * bm - co))[m][:, None])[okm][:, okn]
    return out


def direct_down(g, rs, x, co, bm, bn):
    P, ci, H2, W2 = x.shape
    H, W = H2 // 2, W2 // 2
    mt, ncb = -(-co // bm), ci // 16
    A = unpack(g, (mt, 4 * ncb), bm)
    out = np.full((P, co, H, W), np.nan)
    tl, geo = tiles(P, H, W, bn)
    p, r, c, bpos = tile_pixels(bn, W, geo)
    for plane0, row0 in tl:
        acc = np.zeros((mt, bm, bn))
        for cblk in range(4 * ncb):  # (input phase, 16-channel block)
            qi, cb = cblk // ncb, cblk % ncb
            qy, qx = qi >> 1, qi & 1
            X = halo_tile(lambda q, iy, ix: x[q, 16 * cb:16 * cb + 16, 2 * iy + qy, 2 * ix + qx], P, H, W, plane0, row0, geo)
            for ky in range(2):
                for kx in range(2):  # tap origin (1 - qy, 1 - qx)
                    acc += A[:, cblk, ky, kx] @ X[bpos + (1 - qy + ky) * geo['RS'] + 1 - qx + kx].T
        q, row = plane0 + p, row0 + r
        okn = (q < P) & (row < H)
        for ct in range(mt):
            m = ct * bm + np.arange(bm)
            okm = m < co
            out[q[okn][None, :], m[okm][:, None], row[okn][None, :], c[okn][None, :]] = \
                (acc[ct] * np.pad(rs, (0, mt * bm - co))[m][:, None])[okm][:, okn]
    return out


def rep_bound(conv, x, w, rs_rows):
    """2 x (2^-22 |w| + 2^-25 rs[row]) |x| summed over the taps"""
    ax, aw = torch.from_numpy(np.abs(x)), torch.from_numpy(np.abs(w))
    return (2.0 ** -21 * conv(ax, aw) + 2.0 ** -24 * conv(ax, torch.ones_like(aw)) * rs_rows).numpy()


@pytest.mark.parametrize('L', [2, 8])
@pytest.mark.parametrize('ci,co,bm,seed', CASES, ids=IDS)
def test_deconv_index_arithmetic_vs_fp64(out, ci, co, bm, seed, L):
    P, bn = 5, 256 if bm == 64 else 128
    w = up_weight(ci, co, seed).astype(np.float64)
    x = np.random.default_rng(seed + L).standard_normal((P, ci, L, L)).astype(f32).astype(np.float64)
    tag = 'up_%d_%d_%d' % (ci, co, bm)
    rs = out(tag + '.rs').astype(np.float64)
    got = direct_up(out(tag + '.g', np.float16), rs, x, co, bm, bn)
    conv = lambda a, b: torch.nn.functional.conv_transpose2d(a, b, stride=2, padding=1)  # noqa: E731
    ref = conv(torch.from_numpy(x), torch.from_numpy(w)).numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()  # every output element written
    bound = rep_bound(conv, x, w, torch.from_numpy(rs)[None, :, None, None])
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize('L', [2, 8])
@pytest.mark.parametrize('ci,co,bm,seed', CASES, ids=IDS)
def test_down_index_arithmetic_vs_fp64(out, ci, co, bm, seed, L):
    P, bn = 5, 256 if bm == 64 else 128
    w = down_weight(ci, co, seed).astype(np.float64)
    x = np.random.default_rng(seed + 10 + L).standard_normal((P, ci, 2 * L, 2 * L)).astype(f32).astype(np.float64)
    tag = 'down_%d_%d_%d' % (ci, co, bm)
    rs = out(tag + '.rs').astype(np.float64)
    got = direct_down(out(tag + '.g', np.float16), rs, x, co, bm, bn)
    conv = lambda a, b: torch.nn.functional.conv2d(a, b, stride=2, padding=1)  # noqa: E731
    ref = conv(torch.from_numpy(x), torch.from_numpy(w)).numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    bound = rep_bound(conv, x, w, torch.from_numpy(rs)[None, :, None, None])
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())
