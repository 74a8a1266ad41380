"""InceptionI3d / FVD front end without a GPU: the mirror's state_dict layout and signatures, the
new ABI symbols, the host pad arithmetic, and the test-side torch restatement (tests/i3d_torch.py)
against the fixtures the reference itself produced (tests/golden/make_golden_i3d.py)."""
import ctypes
import importlib
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import i3d_inputs as I
from tests import i3d_torch as T
from tests.golden_inputs import PKG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
pkg = importlib.import_module(PKG)
M = pkg.metrics


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'i3d.npz'))


@pytest.fixture(scope='module')
def sd():
    return I.make_i3d_sd()


def test_state_dict_keys_and_shapes_match_the_reference():
    keys = json.load(open(os.path.join(GOLD, 'i3d_keys.json')))
    assert len(keys) == 344
    net = M.InceptionI3d()
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(keys)  # the reference's order too
    assert got == keys
    # the seeded test weights follow the same layout and load strictly
    assert I.key_shapes() == keys
    net.load_state_dict(I.make_i3d_sd(), strict=True)
    # replace_logits changes the two logits entries only
    net.replace_logits(7)
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert got['logits.conv3d.weight'] == [7, 1024, 1, 1, 1] and got['logits.conv3d.bias'] == [7]
    assert {k: v for k, v in got.items() if not k.startswith('logits')} == \
        {k: v for k, v in keys.items() if not k.startswith('logits')}


def test_signatures_mirror_the_reference():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(M.InceptionI3d.__init__)[1:] == [('num_classes', 400), ('spatial_squeeze', True),
                                                   ('final_endpoint', 'Logits'), ('name', 'inception_i3d'),
                                                   ('in_channels', 3), ('dropout_keep_prob', 0.5)]
    assert params(M.trans) == [('x', E)]
    assert params(M.preprocess_single) == [('video', E), ('resolution', 224), ('sequence_length', None)]
    assert params(M.get_fvd_feats) == [('videos', E), ('i3d', E), ('device', E), ('bs', 10)]
    assert params(M.get_feats) == [('videos', E), ('device', E), ('mini_bs', 10), ('i3d', None)]
    assert params(M.calculate_fvd)[:3] == [('videos1', E), ('videos2', E), ('device', E)]
    assert params(M.calculate_fvd1)[:4] == [('videos1', E), ('videos2', E), ('device', E), ('mini_bs', 10)]
    assert params(M.calculate_fvd2) == [('feats1', E), ('feats2', E)]
    assert params(M.load_i3d_pretrained) == [('device', E), ('path', None)]
    assert ('i3d', None) in params(M.eval_metrics)
    assert M.InceptionI3d.VALID_ENDPOINTS[:16] == T.ENDPOINTS
    for name in ('InceptionI3d', 'load_i3d_pretrained', 'get_feats', 'get_fvd_feats', 'calculate_fvd',
                 'calculate_fvd1', 'calculate_fvd2'):
        assert getattr(pkg, name) is getattr(M, name)
    with pytest.raises(ValueError, match='Unknown final endpoint'):
        M.InceptionI3d(final_endpoint='nope')


def test_new_abi_symbols_are_bound_and_digit_free():
    src = open(os.path.join(REPO, 'include', 'extdm.h')).read()
    decl = set(re.findall(r'\b(extdm_fvd\w*)\s*\(', src))
    assert {'extdm_fvd_create', 'extdm_fvd_load_weight', 'extdm_fvd_finalize', 'extdm_fvd_preprocess',
            'extdm_fvd_features', 'extdm_fvd_endpoint', 'extdm_fvd_endpoint_shape', 'extdm_fvd_range_flag',
            'extdm_fvd_destroy', 'extdm_fvd_same_pad', 'extdm_fvd_maxpool'} <= decl
    for name in decl:
        assert re.fullmatch(r'extdm_[a-z_]+', name), name  # the pattern tests/test_abi.py scans with
        assert name in pkg._lib.EXPORTS, name


def test_cpu_tensors_and_missing_weights_file_are_refused(tmp_path):
    net = M.InceptionI3d()
    with pytest.raises(RuntimeError, match='ROCm device'):
        net(torch.zeros(1, 3, 10, 224, 224))
    with pytest.raises(RuntimeError, match='ROCm device'):
        net.extract_features(torch.zeros(1, 3, 10, 224, 224))
    with pytest.raises(RuntimeError, match='ROCm device'):
        M.preprocess_single(torch.zeros(3, 10, 64, 64))
    missing = str(tmp_path / 'i3d_pretrained_400.pt')
    with pytest.raises(FileNotFoundError, match='i3d_pretrained_400.pt'):
        M.load_i3d_pretrained(torch.device('cpu'), path=missing)
    # a state_dict file in the public layout loads
    torch.save(I.make_i3d_sd(), missing)
    got = M.load_i3d_pretrained(torch.device('cpu'), path=missing)
    assert torch.equal(got.state_dict()['Mixed_4e.b2b.conv3d.weight'], I.make_i3d_sd()['Mixed_4e.b2b.conv3d.weight'])


def test_host_pad_arithmetic():
    """extdm_fvd_same_pad against the rule of pytorch_i3d.py:71-95, written out here."""
    if not os.path.exists(pkg._lib.LIB_PATH):
        pytest.skip('library not built here (run __graft_entry__.build())')
    L = pkg._lib.load()
    for stride in (1, 2):
        for k in (1, 2, 3, 7):
            for size in range(1, 21):
                pad = max(k - stride, 0) if size % stride == 0 else max(k - size % stride, 0)
                f, b = ctypes.c_int(-9), ctypes.c_int(-9)
                out = L.extdm_fvd_same_pad(size, k, stride, ctypes.byref(f), ctypes.byref(b))
                assert (out, f.value, b.value) == (-(-size // stride), pad // 2, pad - pad // 2), (size, k, stride)
                assert T.compute_pad(size, k, stride) == pad
    assert L.extdm_fvd_same_pad(0, 3, 1, None, None) == -1


def test_restatement_reproduces_the_endpoint_taps(sd):
    """tests/i3d_torch.py in fp64 against the reference's fp64 taps: the same operations, so the
    difference is summation-order noise of fp64 (bar 1e-11, far below every fp32 effect)."""
    x = I.tap_input().double()
    with torch.no_grad():
        got = T.endpoints(sd, x)
    for ep in I.TAPS:
        g = np.load(os.path.join(GOLD, I.TAP_FILES.get(ep, 'i3d_taps3.npz')))
        ref = I.decode64(g[ep + '_hi'], g[ep + '_lo'])
        assert ref.size > 1000 and got[ep].shape == ref.shape
        # the stored pair itself is exact to 6e-14 + 2^-35 |ref|
        assert np.abs(got[ep].numpy() - ref).max() < 1e-11 + 1e-10 * np.abs(ref).max(), ep


def test_restatement_reproduces_the_full_forward(sd, gold):
    x = I.full_input('t10').double()
    with torch.no_grad():
        logits, pooled = T.forward(sd, x), T.extract_features(sd, x)
    assert logits.shape == (1, 400) and pooled.shape == (1, 1024, 1, 1, 1)
    assert np.abs(logits.numpy() - gold['t10_logits_ref']).max() < 1e-10
    assert np.abs(pooled.numpy() - gold['t10_pooled_ref']).max() < 1e-10


def test_restatement_reproduces_pools_and_preprocess(gold):
    x = I.pool_input()
    for name, (k, s) in I.POOLS.items():
        assert np.array_equal(T.maxpool_same(x, k, s).numpy(), gold['pool_' + name]), name
    # a padded zero beats negative values (the reference pads with zeros, then pools)
    assert T.maxpool_same(-torch.ones(1, 1, 1, 2, 2), (1, 3, 3), (1, 2, 2)).max().item() == 0.0
    for name, (shape, seq) in I.PRE_CASES.items():
        v = T.trans(I.pre_input(name)).double()
        y = torch.stack([T.preprocess_single(u, sequence_length=seq) for u in v])
        assert list(y.shape) == list(gold['pre_' + name + '_shape']), name
        assert np.abs(y[I.PRE_SUB].numpy() - gold['pre_' + name + '_ref']).max() < 1e-12, name
