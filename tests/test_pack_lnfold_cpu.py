"""CPU check of the gamma-folded 1x1 weights of a channel LayerNorm + conv pair (csrc/pack.cpp
fold_ln_gamma, read by conv_x3.hip's per-pixel input affine): tests/pack_lnfold_driver.cpp, built
with AddressSanitizer and UBSan, folds seeded weights (the three special rows of test_pack_cpu.py)
with a seeded gamma (a zero, a negative, a power of two and a tiny entry) and packs the result with
pack_x3 on the 1x1 tiles (two channel groups per block).

W' = fp32(fp64(W) * fp64(gamma)) -- the fp64 product of two fp32 values is exact, so this is the
single rounding of the real product -- and the packed fragments and row scales are recomputed in
numpy from the layout comment in csrc/pack.h; both compared byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_pack_cpu import CSRC, REPO, _compiler, f32, gen, hilo, pow2, row_exp, same, weights

# (Cout, Cin, bm, seed) in the driver's order
CASES = [(40, 32, 64, 70), (40, 48, 64, 71), (160, 64, 128, 72)]
IDS = ['co%d-ci%d-bm%d' % c[:3] for c in CASES]


@pytest.fixture(scope='module')
def out(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('pack_lnfold')
    exe = str(d / 'pack_lnfold_driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', CSRC, os.path.join(REPO, 'tests', 'pack_lnfold_driver.cpp'),
                    os.path.join(CSRC, 'pack.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return lambda name, dt=np.float32: np.fromfile(str(d / (name + '.bin')), dtype=dt)


def gamma_of(ci, seed):
    g = f32(1) + f32(4) * gen(ci, seed)
    g[:4] = [2.0, 1e-3, 0.0, -1.5]
    return g.astype(f32)


def folded(co, ci, seed):
    w, g = weights(co, ci, seed), gamma_of(ci, seed + 100)
    return w, g, (w.astype(np.float64) * g.astype(np.float64)[None, :]).astype(f32)


@pytest.mark.parametrize('co,ci,bm,seed', CASES, ids=IDS)
def test_fold_is_the_once_rounded_product(out, co, ci, bm, seed):
    w, g, f = folded(co, ci, seed)
    same(out('fold_%d_%d_%d.w' % (co, ci, bm)), f)
    # the special entries: a zero gamma column and the zero row stay exactly zero, the power-of-two
    # gamma is exact, the negative one flips the sign
    assert not f[:, 2].any() and not f[0].any()
    assert f[1, 0] == 1.0 and np.array_equal(f[:, 3], (w[:, 3] * f32(-1.5)).astype(f32))
    # one rounding: within half an ulp of the exact product (fp64 holds it exactly)
    exact = w.astype(np.float64) * g.astype(np.float64)
    assert (np.abs(f.astype(np.float64) - exact) <= np.spacing(np.abs(f)).astype(np.float64) / 2).all()


@pytest.mark.parametrize('co,ci,bm,seed', CASES, ids=IDS)
def test_folded_weight_packs_as_any_weight(out, co, ci, bm, seed):
    f = folded(co, ci, seed)[2]
    ng = 2
    ncgb, mt, m32 = -(-ci // (16 * ng)), -(-co // bm), bm // 32
    e = row_exp(np.abs(f).max(axis=1))
    # [mtile][cb][g][m32][hi|lo][lane][8] (ks = 1): row m = mtile*BM + m32*32 + lc, channel cb*32 + g*16 + 8h + e
    mtile, cb, g_, q, hl, lane, el = np.indices((mt, ncgb, ng, m32, 2, 64, 8))
    m = mtile * bm + q * 32 + (lane & 31)
    c = cb * 16 * ng + g_ * 16 + 8 * (lane >> 5) + el
    ok = (m < co) & (c < ci)
    mc, cc = np.minimum(m, co - 1), np.minimum(c, ci - 1)
    hi, lo = hilo(f[mc, cc] * pow2(e)[mc])
    a = np.where(ok, np.where(hl == 0, hi, lo), np.float16(0))
    tag = 'fold_%d_%d_%d' % (co, ci, bm)
    same(out(tag + '.g', np.float16), a)
    same(out(tag + '.rs'), pow2(-e))
    assert out(tag + '.n')[0] == ncgb
    # row 0 folds to zero (rs = 1, zero fragments); row 1's largest product is 0.5 * 2 = 2^0
    assert pow2(-e)[0] == 1.0 and pow2(-e)[1] == 2.0 ** -14 and not a[0, :, :, 0, :, ::32, :].any()
