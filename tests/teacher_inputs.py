"""Seeds and cases of the teacher-forced evaluation step (q_sample / p_losses / FlowDiffusion.forward),
shared by tests/golden/make_golden_teacher.py and the tests. Everything is regenerated from seeds."""
import dataclasses

import torch

from tests.golden_inputs import (CONFIGS, FD_UNET, LFAE_CFG, WRAP_CASES, lfae_config_dict, unet_inputs,
                                 video_inputs)

# GaussianDiffusion.p_losses on the reduced u12 denoiser: two samples with a dynamic threshold
# (t = 999, 500) and two at the floor s = 1 (t = 37, 0)
SMALL = {'config': 'small', 'B': 4, 'seed': 81, 'noise_seed': 82, 't': [999, 500, 37, 0]}


def small_case():
    """cfg, x_start, cond, fea, t, noise of the `small` case (CPU tensors)."""
    cfg = CONFIGS[SMALL['config']]
    x, _, cond, fea = unet_inputs(cfg, B=SMALL['B'], seed=SMALL['seed'])
    x_start = (x * 0.5).clamp(-1, 1)
    t = torch.tensor(SMALL['t'], dtype=torch.long)
    g = torch.Generator().manual_seed(SMALL['noise_seed'])
    noise = torch.randn(x_start.shape, generator=g)
    return cfg, x_start, cond, fea, t, noise


# FlowDiffusion(is_train=True).eval().forward(real_vid) of the three wrappers: the wrapper cases of
# tests/golden_inputs.py with clips of tc + tp frames. The reference draws t, then the noise, from the
# CPU stream after torch.manual_seed(noise_seed) (Diffusion.py:325, 288).
WRAP_TEACHER = {
    'fd': {'module': 'VideoFlowDiffusion_multi_w_ref', 'wrapper': 'multi_w_ref', 'unet': FD_UNET, 'B': 2, 'seed': 8,
           'noise_seed': 91, 'out_bar': 1.2e-4},
    'u22': dict(WRAP_CASES['u22'], noise_seed=92, out_bar=2.5e-4),
    'm1248': dict(WRAP_CASES['m1248'], noise_seed=93, out_bar=2.5e-4),
}
OUT_STRIDE = 2  # fake_out_vid is stored at every second pixel (fixture size)


def wrapper_config(tag):
    """The config/DM-style dict of a wrapper case (occlusion head on)."""
    case = WRAP_TEACHER[tag]
    if tag == 'fd':
        lc = dataclasses.replace(LFAE_CFG, pf_estimate_occlusion_map=True)
        return lfae_config_dict(lc, FD_UNET, True)
    return case['config']()


def wrapper_video(tag, image):
    case = WRAP_TEACHER[tag]
    u = case['unet']
    return video_inputs(B=case['B'], T=u.tc + u.tp, S=image, seed=case['seed'])


def replay_t_noise(tag, timesteps=1000):
    """The reference forward's CPU draws after torch.manual_seed(noise_seed): t, then the noise."""
    case = WRAP_TEACHER[tag]
    u = case['unet']
    torch.manual_seed(case['noise_seed'])
    t = torch.randint(0, timesteps, (case['B'],)).long()
    noise = torch.randn(case['B'], 3, u.tp, u.latent, u.latent)
    return t, noise
