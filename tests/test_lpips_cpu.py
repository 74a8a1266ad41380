"""LPIPS without a GPU: the test-side torch restatement (tests/lpips_torch.py) against the fixture
(tests/golden/make_golden_lpips.py), the mirror's state_dict layout and signatures, the new ABI
symbols, the host mean weights and feature-size rule, and pack_conv2d (csrc/pack.cpp) through a
stand-alone sanitizer-built driver against a numpy gather written from the layout comment."""
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_inputs as I
from tests import lpips_torch as T
from tests.golden_inputs import PKG
from tests.test_pack_cpu import CSRC, _compiler, frags, same, special_rows_checked, weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
pkg = importlib.import_module(PKG)
M = pkg.metrics
f32 = np.float32


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'lpips.npz'))


@pytest.fixture(scope='module')
def sd64():
    return T.cast(I.make_lpips_sd(), torch.float64)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(pkg._lib.LIB_PATH):
        pytest.skip('library not built here (run __graft_entry__.build())')
    return pkg._lib.load()


def test_fixture_is_small_and_records_the_reference_defect(gold):
    assert os.path.getsize(os.path.join(GOLD, 'lpips.npz')) < 1 << 20
    # calculate_lpips.py:66 indexes a list of lists with [:, t]
    assert 'list indices must be integers or slices, not tuple' in str(gold['calc_typeerror'])


def test_restatement_reproduces_the_taps(gold, sd64):
    """fp64 against the stored fp64 taps: the same operations, so the difference is fp64
    summation-order noise plus the stored pair's own 6e-14 + 2^-35 |ref|."""
    for case, (shape, _, cs) in I.TAP_CASES.items():
        with torch.no_grad():
            got = T.taps(sd64, I.tap_input(case).double())
        for name, g in zip(I.TAPS, got):
            key = f'tap_{case}_{name}'
            ref = I.decode64(gold[key + '_hi'], gold[key + '_lo'])
            assert ref.size > 1000 and g[:, ::cs].shape == ref.shape
            assert np.abs(g[:, ::cs].numpy() - ref).max() < 1e-11 + 1e-10 * np.abs(ref).max(), key
            assert (g[:, list(I.DEAD)] == 0).all() and (g > 0).any(), key


def test_restatement_reproduces_distances_and_the_reference_reductions(gold, sd64):
    with torch.no_grad():
        for case, (_, _, ms) in I.DIST_CASES.items():
            a, b = (t.double() for t in I.dist_inputs(case))
            m = T.forward(sd64, a, b, spatial=True)[:, 0]
            key = f'dist_{case}'
            assert np.abs(m.mean([1, 2]).numpy() - gold[key + '_mean_ref']).max() < 1e-13
            ref = I.decode64(gold[key + '_map_hi'], gold[key + '_map_lo'])
            # the stored pair is exact to 6e-14 + 2^-35 |ref|
            assert np.abs(m[:, ::ms, ::ms].numpy() - ref).max() < 1e-11 + 1e-10 * np.abs(ref).max()
            p = T.forward(sd64, a, b, spatial=False).flatten()
            assert np.abs(p.numpy() - gold[key + '_plain_ref']).max() < 1e-13
        # the reference's loops: trans, one pair per forward, .mean(), then numpy
        v1, v2 = (T.trans(v.double()) for v in I.videos())
        fr = np.array([[T.forward(sd64, x[None], y[None], spatial=True).mean().item() for x, y in zip(a, b)]
                       for a, b in zip(v1, v2)])
    assert np.abs(fr - gold['frames_ref']).max() < 1e-13
    assert abs(np.mean(fr) - gold['red1_ref'][0]) < 1e-13 and abs(np.std(fr) - gold['red1_ref'][1]) < 1e-13
    assert abs(np.min(np.mean(fr, axis=-1)) - float(gold['red2_ref'])) < 1e-13
    assert np.abs(np.mean(fr, axis=-1) - gold['red3_ref']).max() < 1e-13
    # the fp32 run the reference itself does sits within its own error of the fp64 one
    assert abs(float(gold['red2_ref32']) - float(gold['red2_ref'])) <= float(gold['frames_err32'][0])
    for name in I.POOL_SHAPES:
        assert np.array_equal(F.max_pool2d(I.pool_input(name), 3, 2).numpy(), gold['pool_' + name])


def test_mean_of_the_upsample_is_a_separable_weighted_sum(lib):
    """mean(upsample(m)) = sum_ij wy[i] wx[j] m[i][j], checked in fp64 on a 3 x 5 map to 37 x 50."""
    g = np.random.Generator(np.random.PCG64(520))
    m = torch.from_numpy(g.uniform(0, 1, (1, 1, 3, 5)))
    up = F.interpolate(m, size=(37, 50), mode='bilinear', align_corners=False)
    wy, wx = pkg._lib.lpips_mean_weights(3, 37), pkg._lib.lpips_mean_weights(5, 50)
    assert abs(float(up.mean()) - float(wy @ m[0, 0].numpy() @ wx)) < 1e-15
    assert abs(float(up.mean()) - float(m.mean())) > 1e-5  # and not the plain mean


@pytest.mark.parametrize('n_in,n_out', [(3, 64), (1, 37), (2, 50), (15, 256)])
def test_mean_weights_against_interpolate_of_identity_columns(lib, n_in, n_out):
    w = pkg._lib.lpips_mean_weights(n_in, n_out)
    eye = torch.eye(n_in, dtype=torch.float64)[:, None, :, None]  # column i: a unit map along H
    up = F.interpolate(eye, size=(n_out, 1), mode='bilinear', align_corners=False)
    want = up[:, 0, :, 0].mean(dim=1).numpy()
    assert w.dtype == np.float64 and w.shape == (n_in,)
    assert abs(w.sum() - 1.0) < 1e-12
    assert np.abs(w - want).max() < 1e-12
    assert pkg._lib.load().extdm_lpips_mean_weights(0, 4, None) == -1


def test_feature_size_rule(lib):
    """extdm_lpips_feature_shape for sizes 31 - 70 against the layers' own rules, and against torch
    on a few sizes."""
    chans = [c[1] for c in I.CONVS]
    for h in range(31, 71):
        w = 31 + (h * 7) % 40
        a, b, c = T.feature_hw(h, w)
        want = [a, b, c, c, c]
        for k in range(5):
            assert pkg._lib.lpips_feature_shape(h, w, k) == (chans[k], *want[k]), (h, w, k)
        assert min(c) >= 1
    sd = I.make_lpips_sd()
    for h, w in ((31, 31), (37, 50), (48, 64), (64, 64), (70, 33)):
        with torch.no_grad():
            got = [tuple(t.shape[1:]) for t in T.taps(sd, torch.zeros(1, 3, h, w))]
        assert got == [pkg._lib.lpips_feature_shape(h, w, k) for k in range(5)]
    # the table of the issue
    assert [pkg._lib.lpips_feature_shape(s, s, k)[1] for s in (64, 128, 256) for k in (0, 1, 2)] == \
        [15, 7, 3, 31, 15, 7, 63, 31, 15]
    # below 31 the second pool has no output
    assert pkg._lib.lpips_feature_shape(30, 64, 2)[1] == 0 and pkg._lib.lpips_feature_shape(64, 30, 4)[2] == 0


def test_state_dict_keys_shapes_and_aliases():
    net = M.LPIPS()
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert len(got) == 22
    assert list(got) == list(I.key_shapes()) and got == I.key_shapes()
    sdict = net.state_dict()
    for k in range(5):  # the lins aliases share storage, as the package's do
        assert sdict[f'lin{k}.model.1.weight'].data_ptr() == sdict[f'lins.{k}.model.1.weight'].data_ptr()
    assert torch.equal(sdict['scaling_layer.shift'].flatten(), torch.tensor(I.SHIFT))
    assert torch.equal(sdict['scaling_layer.scale'].flatten(), torch.tensor(I.SCALE))
    net.load_state_dict(I.make_lpips_sd(), strict=True)


def test_signatures_and_refusals(tmp_path):
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert dict(params(M.LPIPS.__init__)[1:]) == dict(
        pretrained=True, net='alex', version='0.1', lpips=True, spatial=False, pnet_rand=False, pnet_tune=False,
        use_dropout=True, model_path=None, eval_mode=True, verbose=True)
    assert params(M.LPIPS.forward)[1:] == [('in0', E), ('in1', E), ('retPerLayer', False), ('normalize', False)]
    for f in (M.calculate_lpips, M.calculate_lpips1, M.calculate_lpips2, M.calculate_lpips3):
        assert params(f) == [('videos1', E), ('videos2', E), ('device', E), ('loss_fn', None)]
    assert params(M.load_lpips_pretrained) == [('device', E), ('alexnet_path', E), ('lin_path', E)]
    assert ('lpips', None) in params(M.eval_metrics)
    for name in ('LPIPS', 'load_lpips_pretrained', 'calculate_lpips', 'calculate_lpips1', 'calculate_lpips2',
                 'calculate_lpips3', 'best_of_n_lpips'):
        assert getattr(pkg, name) is getattr(M, name)
    for kw in (dict(net='vgg'), dict(net='squeeze'), dict(lpips=False), dict(version='0.0')):
        with pytest.raises(NotImplementedError):
            M.LPIPS(**kw)
    net = M.LPIPS(spatial=True)
    with pytest.raises(RuntimeError, match='ROCm device'):
        net(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match='ROCm device'):
        M.calculate_lpips1(torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 2, 3, 64, 64), 'cpu', loss_fn=net)
    with pytest.raises(ValueError, match='loss_fn'):
        M.calculate_lpips2(torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 2, 3, 64, 64), 'cpu')
    # trans of calculate_lpips.py:15-23
    x = torch.rand(1, 2, 1, 4, 4)
    assert torch.equal(M.lpips_trans(x), T.trans(x)) and M.lpips_trans(x).shape == (1, 2, 3, 4, 4)
    # the two files users have
    sd = I.make_lpips_sd()
    alex = {k.replace('net.slice', 'features.').split('.', 2)[0] + '.' + k.split('.', 2)[2]: v
            for k, v in sd.items() if k.startswith('net.')}
    assert 'features.10.bias' in alex and len(alex) == 10
    alex['classifier.1.weight'] = torch.zeros(2, 2)  # the rest of torchvision's file is ignored
    lin = {k: v for k, v in sd.items() if k.startswith('lin') and not k.startswith('lins')}
    pa, pl = str(tmp_path / 'alexnet.pth'), str(tmp_path / 'alex.pth')
    with pytest.raises(FileNotFoundError, match='alexnet.pth'):
        M.load_lpips_pretrained(torch.device('cpu'), pa, pl)
    torch.save(alex, pa)
    torch.save(lin, pl)
    got = M.load_lpips_pretrained(torch.device('cpu'), pa, pl).state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k


def test_new_abi_symbols_are_bound_and_digit_free():
    src = open(os.path.join(REPO, 'include', 'extdm.h')).read()
    decl = set(re.findall(r'\b(extdm_lpips\w*)\s*\(', src))
    assert {'extdm_lpips_create', 'extdm_lpips_load_weight', 'extdm_lpips_finalize', 'extdm_lpips_destroy',
            'extdm_lpips_distance', 'extdm_lpips_features', 'extdm_lpips_feature_shape', 'extdm_lpips_maxpool',
            'extdm_lpips_mean_weights', 'extdm_lpips_range_flag'} == decl
    for name in decl:
        assert re.fullmatch(r'extdm_[a-z_]+', name), name  # the pattern tests/test_abi.py scans with
        assert name in pkg._lib.EXPORTS, name


# ------------------------------------------------------------------ pack_conv2d
@pytest.fixture(scope='module')
def out(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('pack_lpips')
    exe = str(d / 'pack_lpips_driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', CSRC, os.path.join(REPO, 'tests', 'pack_lpips_driver.cpp'),
                    os.path.join(CSRC, 'pack.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return lambda name, dt=np.float32: np.fromfile(str(d / (name + '.bin')), dtype=dt)


def test_pack_conv2d_stem_rows(out):
    """k = ky * 40 + kx * 3 + ci, j = kx * 3 + ci >= 33 absent; K = 440 = 13 k-tiles + 24."""
    Mo, Cin, KS = 64, 3, 11
    w = weights(Mo, Cin * KS * KS, 51).reshape(Mo, Cin, KS, KS)  # [m][ci][ky][kx]
    dense = np.zeros((1, Mo, KS, 40), f32)
    dense[0, :, :, :33] = w.transpose(0, 2, 3, 1).reshape(Mo, KS, 33)
    present = np.zeros(dense.shape, bool)
    present[..., :33] = True
    g, rs = frags(dense.reshape(1, Mo, 440), present.reshape(1, Mo, 440), 64)
    assert out('stem.dims')[0] == 14 and g.shape[2] == 14
    same(out('stem.g', np.float16), g)
    same(out('stem.rs'), rs)
    special_rows_checked(g, rs)


@pytest.mark.parametrize('name,Mo,Cin,KS,bm,seed', [('c5', 192, 8, 5, 128, 52), ('c3', 40, 16, 3, 64, 53)])
def test_pack_conv2d_tap_major(out, name, Mo, Cin, KS, bm, seed):
    """k = (ky * KS + kx) * Cpad + ci; Cout 192 at BM 128 leaves the second m-tile half empty."""
    w = weights(Mo, Cin * KS * KS, seed).reshape(Mo, Cin, KS * KS)
    dense = w.transpose(0, 2, 1).reshape(1, Mo, KS * KS * Cin)
    g, rs = frags(dense, np.ones(dense.shape, bool), bm)
    assert out(name + '.dims')[0] == -(-(KS * KS * Cin) // 32)
    same(out(name + '.g', np.float16), g)
    same(out(name + '.rs'), rs)
    special_rows_checked(g[:, :1], rs, bm)  # the special rows sit in m-tile 0
    # [par][mtile][ktile][step][m32][hi|lo][lane][8]: the 32-row blocks past Cout stay zero
    assert g.shape[1] == -(-Mo // bm)
    assert not g[0, -1, :, :, -(-(Mo % bm) // 32):].any() and g[0, -1, :, :, (Mo % bm - 1) // 32].any()
