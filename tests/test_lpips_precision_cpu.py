"""The `precision` attribute of LPIPS without a GPU: the default, the refused values, the route
rule of 'fp32' and 'auto', the one-shot fallback on the library's range text, the unchanged
state_dict and constructor parameter list, the CPU-tensor refusal on every route, and the
EXTDM_LPIPS_FP32 flag in the header and the binding with the extdm_lpips_* symbol set unchanged."""
import importlib
import inspect
import os
import re
import warnings

import pytest
import torch

from tests import lpips_inputs as I
from tests.golden_inputs import PKG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module(PKG)
M = pkg.metrics

RANGE_TEXT = 'lpips: activation out of fp16 range (|v| >= 65504) in an f16x3 convolution'


def test_precision_attribute():
    net = M.LPIPS()
    assert net.precision == 'f16x3' and net._route() == 'f16x3'
    for bad in ('bf16_attn', 'fp16', 'FP32', None, 0, 8):
        with pytest.raises(ValueError, match='precision'):
            net.precision = bad
    assert net.precision == 'f16x3'
    net.precision = 'fp32'
    assert net.precision == 'fp32' and net._route() == 'fp32'
    net.precision = 'auto'
    assert net.precision == 'auto' and net._route() == 'f16x3'
    # another instance keeps the default
    assert M.LPIPS().precision == 'f16x3'


def test_precision_is_not_state():
    net = M.LPIPS()
    net.precision = 'fp32'
    sd = net.state_dict()
    assert list(sd) == list(I.key_shapes()) and not any('precision' in k for k in sd)
    assert not any('precision' in n for n, _ in list(net.named_parameters()) + list(net.named_buffers()))
    other = M.LPIPS()
    other.load_state_dict(sd, strict=True)
    assert other.precision == 'f16x3'


def test_constructor_parameters_unchanged():
    params = [(p.name, p.default) for p in inspect.signature(M.LPIPS.__init__).parameters.values()]
    assert params[1:] == [('pretrained', True), ('net', 'alex'), ('version', '0.1'), ('lpips', True),
                          ('spatial', False), ('pnet_rand', False), ('pnet_tune', False), ('use_dropout', True),
                          ('model_path', None), ('eval_mode', True), ('verbose', True)]
    with pytest.raises(TypeError):
        M.LPIPS(precision='fp32')


def test_auto_falls_back_once_on_the_range_error_only():
    """_on_route without a device: the library's range error switches 'auto' to fp32 with one
    warning and re-runs; any other error, and the range error on the other settings, pass through."""
    net = M.LPIPS()
    net.precision = 'auto'
    routes = []

    def run():
        routes.append(net._route())
        if routes[-1] == 'f16x3':
            raise RuntimeError(RANGE_TEXT)
        return 7
    with pytest.warns(RuntimeWarning, match='FP32') as rec:
        assert net._on_route(run) == 7
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert routes == ['f16x3', 'fp32'] and net._route() == 'fp32' and net.precision == 'auto'
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert net._on_route(run) == 7  # stays on fp32, no second warning
    assert routes[-1] == 'fp32'

    def other():
        raise RuntimeError('lpips: 65 pairs exceed max_pairs 64')
    net.precision = 'auto'  # setting it starts over on f16x3
    assert net._route() == 'f16x3'
    with pytest.raises(RuntimeError, match='max_pairs'):
        net._on_route(other)
    assert net._route() == 'f16x3'

    def ranged():
        raise RuntimeError(RANGE_TEXT)
    for p in ('f16x3', 'fp32'):
        net.precision = p
        with pytest.raises(RuntimeError, match='65504'):
            net._on_route(ranged)
        assert net._route() == p
    # the text the fallback matches is the text the runtime raises
    text = open(os.path.join(os.path.dirname(pkg.__file__), 'csrc', 'lpips.cpp')).read()
    assert M.LPIPS._RANGE_MSG in text and RANGE_TEXT in text and M.LPIPS._RANGE_MSG in RANGE_TEXT


@pytest.mark.parametrize('precision', ['f16x3', 'fp32', 'auto'])
def test_cpu_tensors_are_refused_on_every_route(precision):
    net = M.LPIPS(spatial=True)
    net.precision = precision
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match='ROCm device'):
        net(x, x)
    with pytest.raises(RuntimeError, match='ROCm device'):
        net.distance(x, x)
    with pytest.raises(RuntimeError, match='ROCm device'):
        net.features(x, 'relu3')
    with pytest.raises(RuntimeError, match='ROCm device'):
        M.calculate_lpips1(torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 2, 3, 64, 64), 'cpu', loss_fn=net)
    assert net.precision == precision


def test_flag_in_the_header_and_the_binding():
    hdr = open(os.path.join(REPO, 'include', 'extdm.h')).read()
    flags = {n: int(v) for n, v in re.findall(r'^#define (EXTDM_LPIPS_\w+) (\d+)\b', hdr, re.M)}
    assert flags == {'EXTDM_LPIPS_NORMALIZE': 1, 'EXTDM_LPIPS_TRANS': 2, 'EXTDM_LPIPS_PLAIN_MEAN': 4,
                     'EXTDM_LPIPS_FP32': 8}
    L = pkg._lib
    assert (L.LPIPS_NORMALIZE, L.LPIPS_TRANS, L.LPIPS_PLAIN_MEAN, L.LPIPS_FP32) == (1, 2, 4, 8)
    # the route is a flag of the two calls that take one: no symbol is added, renamed or removed
    decl = set(re.findall(r'\b(extdm_lpips\w*)\s*\(', hdr))
    assert decl == {'extdm_lpips_create', 'extdm_lpips_load_weight', 'extdm_lpips_finalize', 'extdm_lpips_destroy',
                    'extdm_lpips_distance', 'extdm_lpips_features', 'extdm_lpips_feature_shape',
                    'extdm_lpips_maxpool', 'extdm_lpips_mean_weights', 'extdm_lpips_range_flag'}
    assert {n for n in L.EXPORTS if n.startswith('extdm_lpips')} == decl
