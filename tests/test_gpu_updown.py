"""The stride-2 convs (Downsample Conv3d (1,4,4)/s2/p1, Upsample ConvTranspose3d (1,4,4)/s2/p1) on
the direct kernel's two-tap mode (conv_x3.hip TT) against the implicit GEMM they replace: the
`small` u12 forward (dim 16: C = 16 / 32 / 64 / 64, maps 16 -> 8 -> 4 -> 2) at B = 3 -- 24 planes,
so the 4 x 4 level's 16-plane tiles end in a partial one -- with the route on (default) and with
EXTDM_NO_X3_UPDOWN=1 (consulted per launch decision, so two handles in one process), both against
the fp64 evaluation of the oracle. The 2 x 2 maps (64 planes per tile: a halo tile past the
kernel's staging slots) stay on the implicit GEMM in both runs.

The bars: the new route's max and rms error within 2x the fp32 CPU oracle's own error against fp64
(the contract of test_f16x3_error_vs_fp64_matches_fp32), and within 2x the old route's error on the
same input."""
import os

import pytest
import torch

from tests import parity_log
from tests.golden_inputs import CONFIGS, make_sd, unet_inputs
from tests.test_gpu_parity import gpu_eps, pkg
from tests.test_gpu_precision import _fp64_eps

pytestmark = pytest.mark.gpu


def _handle(cfg, B):
    h = pkg._lib.Handle(cfg, 1000, B, 0)
    sd = make_sd(cfg)
    sd.update(pkg.schedule_buffers(1000))
    h.load_state(sd)
    h.finalize()
    return h


def _stats(e, ref):
    d = e.double() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def test_updown_direct_route_vs_fp64_and_implicit_gemm():
    from oracle import extdm_oracle as O
    cfg = CONFIGS['small']
    x, t, cond, fea = unet_inputs(cfg, B=3, seed=43)
    os.environ.pop('EXTDM_NO_X3_UPDOWN', None)
    h = _handle(cfg, 3)
    h.range_flag(reset=True)
    new = gpu_eps(h, x, t, cond, fea)
    assert h.range_flag() == 0
    # the level-0 launches took the direct kernel (the test cannot pass on the fallback)
    for layer in (18, 19):
        h.bench_layer(3, layer, 1)
        assert 'conv_x3_kernel' in h.bench_layer_kernel(layer), (layer, h.bench_layer_kernel(layer))
    # clip 0 does not depend on its batch
    one = gpu_eps(_handle(cfg, 1), x[:1], t[:1], cond[:1], fea[:1])
    assert torch.equal(new[:1], one)
    os.environ['EXTDM_NO_X3_UPDOWN'] = '1'
    try:
        h_old = _handle(cfg, 3)
        h_old.range_flag(reset=True)
        old = gpu_eps(h_old, x, t, cond, fea)
        assert h_old.range_flag() == 0
        h_old.bench_layer(3, 18, 1)
        assert 'conv_x3_kernel' not in h_old.bench_layer_kernel(18)
    finally:
        os.environ.pop('EXTDM_NO_X3_UPDOWN', None)
    assert torch.isfinite(new).all() and not torch.equal(new, old)  # the switch selects another route

    ref = _fp64_eps(cfg, x, t, cond, fea)
    with torch.no_grad():
        cpu32 = O.unet_forward(make_sd(cfg), cfg.as_dict(), x, t, cond, fea)
    (m_cpu, r_cpu), (m_new, r_new), (m_old, r_old) = _stats(cpu32, ref), _stats(new, ref), _stats(old, ref)
    print(f'vs fp64: cpu-fp32 max {m_cpu:.3e} rms {r_cpu:.3e} | direct max {m_new:.3e} rms {r_new:.3e} | '
          f'implicit GEMM max {m_old:.3e} rms {r_old:.3e}')
    parity_log.check(m_new, 2.0 * m_cpu, 'direct max vs 2x cpu-fp32')
    parity_log.check(r_new, 2.0 * r_cpu, 'direct rms vs 2x cpu-fp32')
    parity_log.check(m_new, 2.0 * m_old, 'direct max vs 2x implicit GEMM')
    parity_log.check(r_new, 2.0 * r_old, 'direct rms vs 2x implicit GEMM')


def test_updown_bench_layers_take_the_direct_kernel_on_bair():
    os.environ.pop('EXTDM_NO_X3_UPDOWN', None)
    h = _handle(CONFIGS['bair'], 2)
    for layer in (18, 19):
        ms, flop = h.bench_layer(2, layer, 1)
        k = h.bench_layer_kernel(layer)
        assert 'conv_x3_kernel' in k and ms > 0 and flop > 0, (layer, k, ms, flop)
