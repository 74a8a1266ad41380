"""DPM-Solver++(2M) without a GPU: the two time grids, the solver's order on a toy problem with a
closed-form answer (tests/dpmpp_ref.py, fp64), and the interface (attribute defaults, the exported
symbol, the CPU-tensor refusal).

The toy: cosine schedule at T = 1000, x0 ~ N(0, 0.2^2) with the optimal linear denoiser, so the
probability-flow ODE from x_T at t_0 ends at 0.2 / sqrt(0.04 abar(t_0) + 1 - abar(t_0)) x_T.
Relative RMS error against it, measured with these inputs:
  steps   order 1, ddim   2M, ddim   order 1, logsnr   2M, logsnr
    10      2.73e-1        2.20e-1      1.61e-1          1.48e-2
    40      8.18e-2        1.69e-2      5.13e-2          2.24e-3
    80      4.29e-2        3.60e-3
so 2M falls 4.7x from 40 to 80 steps (second order: 4x) and first order 1.9x (2x)."""
import importlib
import os
import re

import pytest
import torch

from tests import dpmpp_ref as R
from tests.golden_inputs import PKG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module(PKG)
SCHED = {T: pkg.schedule_buffers(T) for T in (100, 1000)}


# ---- grids ----
@pytest.mark.parametrize('T,S', [(1000, 5), (1000, 10), (1000, 50), (100, 10)])
def test_ddim_grid_is_the_ddim_loops_timesteps(T, S):
    want = [p[0] for p in pkg.ddim_time_pairs(T, S)]
    assert pkg.dpmpp_times(T, S, 'ddim', SCHED[T]['alphas_cumprod']) == want
    assert R.times(T, S, 'ddim', SCHED[T]['alphas_cumprod']) == want


@pytest.mark.parametrize('T,S', [(1000, 5), (1000, 10), (1000, 20), (1000, 40), (100, 5), (100, 10)])
def test_logsnr_grid_strictly_decreasing_and_non_negative(T, S):
    ts = pkg.dpmpp_times(T, S, 'logsnr', SCHED[T]['alphas_cumprod'])
    assert len(ts) == S and ts[0] == pkg.ddim_time_pairs(T, S)[0][0]
    assert all(a > b for a, b in zip(ts[:-1], ts[1:])) and ts[-1] >= 0, ts
    assert ts == R.times(T, S, 'logsnr', SCHED[T]['alphas_cumprod'])


def test_logsnr_grid_values_at_ten_steps():
    ts = pkg.dpmpp_times(1000, 10, 'logsnr', SCHED[1000]['alphas_cumprod'])
    assert ts[:4] == [909, 821, 665, 449] and ts[-3:] == [26, 10, 3], ts


@pytest.mark.parametrize('spacing', ['ddim', 'logsnr'])
def test_more_steps_than_timesteps_raise(spacing):
    T, S = 100, 120
    assert S > pkg.ddim_time_pairs(T, S)[0][0] + 1
    with pytest.raises(ValueError):
        pkg.dpmpp_times(T, S, spacing, SCHED[T]['alphas_cumprod'])


def test_unknown_spacing_raises():
    with pytest.raises(ValueError, match='spacing'):
        pkg.dpmpp_times(1000, 10, 'karras', SCHED[1000]['alphas_cumprod'])


# ---- convergence on the toy ----
@pytest.fixture(scope='module')
def toy():
    s = SCHED[1000]
    x_T = torch.randn(1, 4096, generator=torch.Generator().manual_seed(20221102), dtype=torch.float64)
    err, peak = {}, 0.
    for order, spacing, S in [(2, 'ddim', 40), (2, 'ddim', 80), (1, 'ddim', 40), (1, 'ddim', 80), (2, 'logsnr', 10)]:
        ts = pkg.dpmpp_times(1000, S, spacing, s['alphas_cumprod'])
        x, pk = R.toy_solve(s, ts, x_T, order)
        err[order, spacing, S] = R.rel_rms(x, R.toy_exact(s, ts[0], x_T))
        peak = max(peak, pk)
    print('toy errors', {k: f'{v:.3e}' for k, v in err.items()}, 'max |x0|', peak)
    return err, peak


def test_toy_threshold_inactive(toy):
    assert toy[1] < 1.0, toy[1]  # s = 1 throughout: the closed form applies


def test_toy_second_order_convergence(toy):
    err = toy[0]
    assert err[2, 'ddim', 40] / err[2, 'ddim', 80] > 3.5, err


def test_toy_first_order_convergence(toy):
    err = toy[0]
    assert err[1, 'ddim', 40] / err[1, 'ddim', 80] < 2.5, err


def test_toy_ten_logsnr_steps_beat_eighty_first_order_steps(toy):
    err = toy[0]
    assert err[2, 'logsnr', 10] < err[1, 'ddim', 80], err


# ---- interface ----
def _diffusion():
    u = pkg.Unet3D(dim=16, channels=512, dim_mults=(1, 2, 4, 4), cond_num=2, pred_num=6, framesize=16)
    return pkg.GaussianDiffusion(u, image_size=16, num_frames=8, timesteps=1000, sampling_timesteps=10)


def test_sampler_attributes_default_and_stay_out_of_the_state_dict():
    d = _diffusion()
    assert d.sampler is None and d.sampler_spacing == 'ddim'
    d.sampler, d.sampler_spacing = 'dpmpp_2m', 'logsnr'
    assert not any('sampler' in k for k in d.state_dict())
    assert _diffusion().sampler is None


def test_symbol_is_declared_and_bound():
    name = 'extdm_sampler_step_hist'
    assert name in pkg._lib.EXPORTS
    header = open(os.path.join(REPO, 'include', 'extdm.h')).read()
    assert re.search(r'\bint ' + name + r'\s*\(', header)
    assert 'EXTDM_SAMPLER_DPMPP = 2' in header and pkg._lib.SAMPLER_DPMPP == 2
    assert hasattr(pkg._lib.Handle, 'sampler_step_hist')


def test_cpu_tensors_are_rejected():
    d = _diffusion()
    cond, fea = torch.zeros(1, 3, 2, 16, 16), torch.zeros(1, 256, 8, 8, 8)
    with pytest.raises(RuntimeError, match='ROCm device'):
        d.dpmpp_sample(cond, (1, 3, 6, 16, 16), fea)
    d.sampler = 'dpmpp_2m'
    with pytest.raises(RuntimeError, match='ROCm device'):
        d.sample(cond, fea)
