"""CPU check of the fp32 tile layouts of the LPIPS exact-fp32 convolution (pack_conv2d_f32 and its
stem variant, csrc/pack.cpp): tests/pack_lpips_f32_driver.cpp, built with AddressSanitizer and
UBSan and run as a program, packs seeded weights with one all-zero row; every buffer is recomputed
here in numpy from the index formula of its layout comment in csrc/pack.h -- one gather per output
element -- and compared byte for byte. The shapes are AlexNet's five convs at the 64-row m-tile the
runtime gives them, a small conv whose Cout is no multiple of the tile and whose Cin is no multiple
of the channel pad of 8, and the stem with 40 rows of a 64-row tile."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_pack_f32_cpu import CSRC, _compiler, checked, stem_rows, tap_major, weights as lcg_loop

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# name -> (M, Cin, KS, bm), in the driver's order (seeds 81, 82, ...)
C2 = {'conv2': (192, 64, 5, 64), 'conv3': (384, 192, 3, 64), 'conv4': (256, 384, 3, 64),
      'conv5': (256, 256, 3, 64), 'odd': (40, 5, 3, 64)}
STEMS = {'stem': 64, 'stem40': 40}
SEEDS = {name: 81 + i for i, name in enumerate(list(C2) + list(STEMS))}


@pytest.fixture(scope='module')
def out(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('pack_lpips_f32')
    exe = str(d / 'pack_lpips_f32_driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', CSRC,
                    os.path.join(REPO, 'tests', 'pack_lpips_f32_driver.cpp'), os.path.join(CSRC, 'pack.cpp'),
                    '-o', exe], check=True)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return lambda name, dt=np.float32: np.fromfile(str(d / (name + '.bin')), dtype=dt)


def weights(M, rowlen, seed, block=4096):
    """The driver's LCG (x <- 1664525 x + 1013904223 mod 2^32), row 0 all zero: the first `block`
    states one by one, the rest `block` steps at a time (x[i + block] = A x[i] + C)."""
    n, mask = M * rowlen, 0xffffffff
    xs = np.empty(n, np.uint64)
    x = seed
    for i in range(min(block, n)):
        x = (x * 1664525 + 1013904223) & mask
        xs[i] = x
    A, C = 1, 0
    for _ in range(block):
        A, C = (A * 1664525) & mask, (C * 1664525 + 1013904223) & mask
    for s in range(block, n, block):
        m = min(block, n - s)
        xs[s:s + m] = (np.uint64(A) * xs[s - block:s - block + m] + np.uint64(C)) & np.uint64(mask)
    v = (xs >> np.uint64(8)).astype(np.int64) - 8388608
    w = (v.astype(f32) / f32(33554432.0)).reshape(M, rowlen)
    w[0] = 0
    return w


def test_weights_are_the_drivers_lcg():
    assert np.array_equal(weights(3, 3001, 77), lcg_loop(3, 3001, 77))


@pytest.mark.parametrize('name', list(C2))
def test_conv2d_f32(out, name):
    """k = (ky * KS + kx) * Cpad + ci, channels ci >= Cin zero."""
    M, Cin, KS, bm = C2[name]
    KK, Cpad = KS * KS, -(-Cin // 8) * 8
    w = weights(M, Cin * KK, SEEDS[name])
    t = checked(out, name, *tap_major(w, M, Cin, KK), bm, M)
    assert t.shape == (-(-M // bm), -(-KK * Cpad // 32), 32, bm)
    if M % bm:
        assert not t[-1, :, :, M % bm:].any() and t[-1, :, :, M % bm - 1].any()
    # spot value: m 7, (ky 1, kx 2, ci 3)
    k = (1 * KS + 2) * Cpad + 3
    assert t[0, k // 32, k % 32, 7] == w.reshape(M, Cin, KS, KS)[7, 3, 1, 2] != 0


@pytest.mark.parametrize('name', list(STEMS))
def test_stem(out, name):
    """k = ky * 40 + kx * 3 + ci, j = kx * 3 + ci >= 33 zero; K = 440 = 13 k-tiles + 24."""
    M, bm = STEMS[name], 64
    w = weights(M, 3 * 121, SEEDS[name])
    t = checked(out, name, *stem_rows(w, M, 3, 11, 121, 11, 40), bm, M)
    assert t.shape == (1, 14, 32, 64)
    assert not t[0, :, :, M:].any()
    # the pad columns of every ky row and the k past 440
    flat = t[0].reshape(14 * 32, 64)
    assert not flat[440:].any()
    assert not flat[:440].reshape(11, 40, 64)[:, 33:].any()
    # spot value: m 5, (ky 3, kx 4, ci 1) -> k = 3 * 40 + 4 * 3 + 1
    k = 3 * 40 + 13
    assert t[0, k // 32, k % 32, 5] == w.reshape(M, 3, 11, 11)[5, 1, 3, 4] != 0
