"""CPU emulation of the one-term fp16 convolution modes (EXTDM_PRECISION_F16_CONV / _F16): the
project's oracle with every torch.nn.functional conv3d / conv2d / conv_transpose3d rounding its
input and its weight to fp16 (fp32 accumulation, fp32 bias). It is the yardstick of the new modes'
bars: its own error against the reference's golden vectors is what operand rounding costs, measured
on the CPU and never against the code under test. One rounding realisation (torch's fp32 summation
order), so the GPU bars allow twice its error (tests/test_gpu_f16_modes.py)."""
import contextlib
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import extdm_oracle as O
from tests.golden_inputs import CONFIGS, GOLDEN_BATCH, make_sd, unet_inputs

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
# the configs the modes are tested on: the reduced ones (implicit GEMM) and the dataset sizes
# (direct tiles, two-tap, split-K, the register-resident 1x1)
EMUL_CONFIGS = ('small', 'ada_small', 'u22_small', 'woref_small', 'bair', 'ada_kth', 'u22_city', 'woref_smmnist')
_WRAPPED = ('conv3d', 'conv2d', 'conv_transpose3d')


def _h(t):
    return t.half().float()


@contextlib.contextmanager
def fp16_conv_operands():
    """Inside: F.conv3d / conv2d / conv_transpose3d see fp16-rounded input and weight. The
    functions are restored on exit, whatever happens inside."""
    saved = {n: getattr(F, n) for n in _WRAPPED}

    def wrap(fn):
        def rounded(inp, weight, *args, **kw):
            return fn(_h(inp), _h(weight), *args, **kw)
        return rounded
    try:
        for n, fn in saved.items():
            setattr(F, n, wrap(fn))
        yield
    finally:
        for n, fn in saved.items():
            setattr(F, n, fn)


def golden_eps(name):
    return np.load(os.path.join(GOLD, f'unet_{name}.npz'))['eps']


@functools.lru_cache(maxsize=None)
def emulated_eps(name):
    """eps of config `name` on its golden inputs with fp16-rounded conv operands (numpy, read-only)."""
    cfg = CONFIGS[name]
    x, t, cond, fea = unet_inputs(cfg, B=GOLDEN_BATCH.get(name, 2))
    sd = make_sd(cfg)
    with torch.no_grad(), fp16_conv_operands():
        eps = O.unet_forward(sd, cfg.as_dict(), x, t, cond, fea)
    out = eps.numpy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated_error(name):
    """(max|emulated_eps - golden|, max|golden|) of config `name`."""
    g = golden_eps(name)
    return float(np.abs(emulated_eps(name) - g).max()), float(np.abs(g).max())


@functools.lru_cache(maxsize=None)
def emulated_chain(kind):
    """The DDPM-10 ('ddpm10') or DDIM-10 ('ddim10') chain of tests/golden/sampler_small.npz through the
    oracle's sampler with the emulated forward, on the golden's injected noise (numpy, read-only)."""
    cfg = CONFIGS['small']
    x, _, cond, fea = unet_inputs(cfg)
    sd = make_sd(cfg)

    def den(xx, tt):
        with fp16_conv_operands():
            return O.unet_forward(sd, cfg.as_dict(), xx, tt, cond, fea)
    with torch.no_grad():
        if kind == 'ddpm10':
            torch.manual_seed(7)
            xT = torch.randn(x.shape)
            noises = [torch.randn(x.shape) for _ in range(10)]
            out = O.p_sample_loop(O.schedule(10), den, xT, noises)
        else:
            torch.manual_seed(11)
            xT = torch.randn(x.shape)
            noises = [torch.randn(x.shape) for _ in range(10)]
            out = O.ddim_sample(O.schedule(1000), den, xT, noises, 10)
    out = out.numpy()
    out.setflags(write=False)
    return out
