"""The teacher-forced evaluation step, checks that need no GPU: the fixture tests/golden/teacher.npz
(tests/golden/make_golden_teacher.py, outputs of the reference itself) is consistent with the
reference formulas (Diffusion.py:276-319); the new GaussianDiffusion methods carry the reference's
parameter names; FlowDiffusion(is_train=True) constructs; the C ABI declares and exports the new
entry points."""
import ctypes
import dataclasses
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.golden_inputs import FD_UNET, LFAE_CFG, PKG, lfae_config_dict
from tests.teacher_inputs import SMALL, WRAP_TEACHER, replay_t_noise, small_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
pkg = importlib.import_module(PKG)


def test_fixture_follows_from_the_reference_formulas():
    """x_t, pred_x0, s and both losses follow from the stored eps, the seeded x_start / noise and
    schedule_1000.npz. x_t / pred_x0 / s bitwise (the same fp32 torch ops on the same CPU); the
    losses to 1e-6 relative (fp32 mean in the reference vs fp64 here)."""
    g = np.load(os.path.join(GOLD, 'teacher.npz'))
    sch = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, 'schedule_1000.npz')).items()}
    _, x0, _, _, t, noise = small_case()
    B = SMALL['B']
    ex = lambda a: a[t].reshape(B, 1, 1, 1, 1)
    xt = ex(sch['sqrt_alphas_cumprod']) * x0 + ex(sch['sqrt_one_minus_alphas_cumprod']) * noise
    assert np.array_equal(xt.numpy(), g['small_x_t'])
    eps = torch.from_numpy(g['small_eps'])
    raw = ex(sch['sqrt_recip_alphas_cumprod']) * xt - ex(sch['sqrt_recipm1_alphas_cumprod']) * eps
    s = torch.quantile(raw.reshape(B, -1).abs(), 0.9, dim=-1).clamp(min=1.)
    assert np.array_equal(s.numpy(), g['small_s'])
    assert (s[:2] > 1).all() and (s[2:] == 1).all()  # two dynamic thresholds, two at the floor
    sv = s.reshape(B, 1, 1, 1, 1)
    assert np.array_equal((raw.clamp(-sv, sv) / sv).numpy(), g['small_pred_x0'])
    l1 = (noise.double() - eps.double()).abs().mean().item()
    l2 = ((noise * 10).double() - (eps * 10).double()).pow(2).mean().item()
    assert abs(l1 - float(g['small_loss_l1'])) <= 1e-6 * l1
    assert abs(l2 - float(g['small_loss_l2'])) <= 1e-6 * l2


@pytest.mark.parametrize('tag', sorted(WRAP_TEACHER))
def test_wrapper_fixture_draws_replay(tag):
    g = np.load(os.path.join(GOLD, 'teacher.npz'))
    t, noise = replay_t_noise(tag)
    assert np.array_equal(t.numpy(), g[f'{tag}_t'])
    assert np.array_equal(noise.numpy(), g[f'{tag}_noise'])
    u = WRAP_TEACHER[tag]['unet']
    assert g[f'{tag}_fake_vid_grid'].shape == (WRAP_TEACHER[tag]['B'], 2, u.tp, u.latent, u.latent)


def test_method_signatures_start_with_the_reference_names():
    want = {'q_sample': ['self', 'x_start', 't', 'noise'],
            'p_losses': ['self', 'x_start_cond', 'x_start_pred', 'cond_fea', 't', 'cond', 'noise', 'clip_denoised'],
            'forward': ['self', 'x_cond', 'x_pred', 'cond_fea']}
    for name, params in want.items():
        got = list(inspect.signature(getattr(pkg.GaussianDiffusion, name)).parameters)
        assert got[:len(params)] == params, (name, got)
    sig = inspect.signature(pkg.GaussianDiffusion.p_losses).parameters
    assert sig['noise'].default is None and sig['clip_denoised'].default is True


def test_unknown_loss_type_raises_like_the_reference():
    u = pkg.Unet3D(dim=16, channels=512, dim_mults=(1, 2, 4, 4), cond_num=2, pred_num=6, framesize=16)
    d = pkg.GaussianDiffusion(u, image_size=16, num_frames=8, loss_type='huber')
    z = torch.zeros(1, 3, 6, 16, 16)
    with pytest.raises(NotImplementedError):
        d.p_losses(torch.zeros(1, 3, 2, 16, 16), z, torch.zeros(1, 256, 8, 8, 8), torch.zeros(1, dtype=torch.long))
    d.loss_type = 'l1'
    with pytest.raises(RuntimeError, match='ROCm device'):  # no CPU fallback
        d.q_sample(z, torch.zeros(1, dtype=torch.long))


def test_flow_diffusion_constructs_for_evaluation():
    lc = dataclasses.replace(LFAE_CFG, pf_estimate_occlusion_map=True)
    fd = pkg.FlowDiffusion(config=lfae_config_dict(lc, FD_UNET, True), is_train=True, dim_mults=FD_UNET.dim_mults,
                           Unet3D_architecture='DenoiseNet_STWAtt_w_w_ref_adaptor_cross_multi_traj_u12').eval()
    assert fd.is_train and callable(fd.forward)
    assert list(inspect.signature(fd.forward).parameters)[:1] == ['real_vid']


def test_abi_declares_and_exports_the_teacher_entry_points():
    names = ['extdm_q_sample', 'extdm_x0_loss', 'extdm_p_losses', 'extdm_sampler_step_t', 'extdm_abs_diff_sum']
    src = open(os.path.join(REPO, 'include', 'extdm.h')).read()
    for n in names:
        assert re.search(r'\bint ' + n + r'\(', src), n
        assert n in pkg._lib.EXPORTS + pkg._lib.EXPORTS_DIGIT, n
    assert os.path.exists(pkg._lib.LIB_PATH), 'library not built (run __graft_entry__.build())'
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
