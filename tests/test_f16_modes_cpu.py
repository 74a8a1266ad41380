"""The one-term fp16 conv modes ('f16_conv' = EXTDM_PRECISION_F16_CONV, 'f16' = EXTDM_PRECISION_F16)
without a GPU: the names and values of the modes in the binding and the header, where they are
accepted (the denoiser) and refused (the metric networks), and the yardstick of the GPU bars -- the
CPU emulation (tests/f16_emul.py) against the reference's golden vectors.

Emulation error / max|golden| measured on the CPU: small 1.02e-3, ada_small 8.1e-4, u22_small 9.7e-4,
woref_small 1.02e-3, bair 1.11e-3, ada_kth 9.7e-4, u22_city 1.03e-3, woref_smmnist 8.2e-4."""
import importlib
import os
import re

import numpy as np
import pytest

from tests import f16_emul
from tests.golden_inputs import CONFIGS, PKG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module(PKG)
L = pkg._lib
REL_TOL = 5e-3  # BF16_ATTN's stated tolerance (tests/test_gpu_bf16_attn.py)


def test_precision_names_and_values():
    assert L.PRECISIONS['f16_conv'] == 3 and L.PRECISIONS['f16'] == 4
    assert L.PRECISIONS['fp32'] == 0 and L.PRECISIONS['f16x3'] == 1 and L.PRECISIONS['bf16_attn'] == 2
    assert 'fp16' not in L.PRECISIONS
    assert L.FVD_PRECISIONS == ('f16x3', 'fp32')


def test_header_enum_names_both_modes():
    hdr = open(os.path.join(REPO, 'include', 'extdm.h')).read()
    m = re.search(r'enum\s*\{[^}]*EXTDM_PRECISION_FP32[^}]*\}', hdr)
    assert m, 'no EXTDM_PRECISION_* enum in include/extdm.h'
    vals = dict((k, int(v)) for k, v in re.findall(r'(EXTDM_PRECISION_\w+)\s*=\s*(\d+)', m.group(0)))
    assert vals == {'EXTDM_PRECISION_FP32': 0, 'EXTDM_PRECISION_F16X3': 1, 'EXTDM_PRECISION_BF16_ATTN': 2,
                    'EXTDM_PRECISION_F16_CONV': 3, 'EXTDM_PRECISION_F16': 4}
    # the binding's table is the header's
    assert {('EXTDM_PRECISION_' + k.upper()): v for k, v in L.PRECISIONS.items()} == vals


def test_handle_refuses_fp16():
    with pytest.raises(ValueError, match='precision'):
        L.Handle(CONFIGS['small'], 1000, 1, 0, precision='fp16')


@pytest.mark.parametrize('name', ['f16_conv', 'f16'])
def test_metric_networks_refuse_the_modes(name):
    with pytest.raises(ValueError, match='precision'):
        L.FvdHandle(400, 3, 1, 10, 0, name)
    i3d = pkg.metrics.InceptionI3d()
    with pytest.raises(ValueError, match='precision'):
        i3d.precision = name
    assert i3d.precision == 'f16x3'
    lp = pkg.metrics.LPIPS()
    with pytest.raises(ValueError, match='precision'):
        lp.precision = name
    assert lp.precision == 'f16x3'


@pytest.mark.parametrize('name', ['f16_conv', 'f16'])
def test_unet_accepts_the_modes(name):
    cfg = CONFIGS['small']
    u = pkg.Unet3D(dim=cfg.dim, channels=512, dim_mults=cfg.dim_mults, cond_num=cfg.tc, pred_num=cfg.tp,
                   framesize=cfg.latent)
    u.precision = name
    assert u.precision == name and name in L.PRECISIONS
    assert not any('precision' in k for k in u.state_dict())
    # the range-error fallback to FP32 is keyed on the message the runtime raises in every x3 mode
    text = open(os.path.join(os.path.dirname(pkg.__file__), 'csrc', 'runtime.cpp')).read()
    assert pkg.GaussianDiffusion._RANGE_MSG in text


@pytest.mark.parametrize('name', f16_emul.EMUL_CONFIGS)
def test_emulation_error_is_below_the_bf16_bar(name):
    """The yardstick itself: rounding every conv operand to fp16 costs less than the bf16 attention
    bar the project already states, so a GPU bar of twice this error is never loose."""
    err, scale = f16_emul.emulated_error(name)
    print(f'{name}: emulated max|err| {err:.3e} = {err / scale:.2e} x max|eps|')
    assert np.isfinite(f16_emul.emulated_eps(name)).all()
    assert 0 < err < REL_TOL * scale, (name, err, scale)
    # and the wrappers are gone again
    import torch.nn.functional as F
    assert F.conv3d.__name__ == 'conv3d' and F.conv2d.__name__ == 'conv2d'
