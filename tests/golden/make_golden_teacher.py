"""Generate tests/golden/teacher.npz by running the REFERENCE itself on CPU in the build container
(like make_golden.py: the reference is imported through the shims at generation time only, and only
data leaves this script): the teacher-forced evaluation step.

  small_*   GaussianDiffusion.q_sample / p_losses (Diffusion.py:276-319) on the reduced u12 denoiser
            with the inputs of tests/teacher_inputs.small_case: x_t, the reference's eps, pred_x0
            (the same for both loss types), the thresholds s and the l1 / l2 losses
  <tag>_*   FlowDiffusion(is_train=True).eval().forward(real_vid) of the three wrappers
            (tests/teacher_inputs.WRAP_TEACHER): the replayed t and noise, loss, rec_loss,
            rec_warp_loss, fake_vid_grid, fake_vid_conf and fake_out_vid at every OUT_STRIDE-th pixel

Usage (build container only):  python tests/golden/make_golden_teacher.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from tests.golden_inputs import PKG, make_lfae_sd, make_sd  # noqa: E402
from tests.teacher_inputs import (OUT_STRIDE, WRAP_TEACHER, replay_t_noise, small_case, wrapper_config,  # noqa: E402
                                  wrapper_video)
from make_golden import _load_lfae, build_ref_unet, import_reference  # noqa: E402

spec = importlib.import_module(PKG + '.spec')


def small(out):
    Unet3D, GD, _ = import_reference()
    cfg, x0, cond, fea, t, noise = small_case()
    net = build_ref_unet(Unet3D, cfg)
    net.load_state_dict(make_sd(cfg), strict=True)
    net.eval()
    B = x0.shape[0]
    for lt in ('l1', 'l2'):
        d = GD(net, image_size=cfg.latent, num_frames=cfg.tc + cfg.tp, timesteps=1000, sampling_timesteps=1000,
               loss_type=lt, null_cond_prob=0.0).eval()
        with torch.no_grad():
            loss, px0 = d.p_losses(cond, x0, fea, t, noise=noise)
            xt = d.q_sample(x0, t, noise)
            eps = net(xt, t, cond, cond_fea=fea)
            raw = d.predict_start_from_noise(xt, t, eps)
        s = torch.quantile(raw.reshape(B, -1).abs(), 0.9, dim=-1).clamp(min=1.)
        out[f'small_loss_{lt}'] = np.float32(loss.item())
        if lt == 'l1':
            out.update(small_x_t=xt.numpy(), small_eps=eps.numpy(), small_pred_x0=px0.numpy(), small_s=s.numpy())
        else:
            assert np.array_equal(out['small_pred_x0'], px0.numpy())
        print('small', lt, float(loss), 's', s.tolist())


def wrappers(out):
    import_reference()
    for tag, case in WRAP_TEACHER.items():
        mod = importlib.import_module('model.BaseDM_adaptor.' + case['module'])
        cfgd = wrapper_config(tag)
        lc = spec.LfaeConfig.from_config(cfgd)
        u = case['unet']
        kw = {'device_ids': ['cpu', 'cpu', 'cpu']} if case['module'].endswith('_u22') else {}
        if tag == 'fd':
            kw.update(dim_mults=u.dim_mults,
                      Unet3D_architecture='DenoiseNet_STWAtt_w_w_ref_adaptor_cross_multi_traj_u12')
        fd = mod.FlowDiffusion(config=cfgd, pretrained_pth='', is_train=True, **kw).eval()
        _load_lfae(fd, make_lfae_sd(lc))
        fd.unet.load_state_dict(make_sd(u), strict=True)
        vid = wrapper_video(tag, lc.image)
        # record the t and the noise the forward draws (Diffusion.py:325, 288) ...
        seen = {}
        q_sample = fd.diffusion.q_sample

        def recording_q_sample(x_start, t, noise=None):
            seen['t'], seen['noise'] = t.clone(), noise.clone()
            return q_sample(x_start=x_start, t=t, noise=noise)
        fd.diffusion.q_sample = recording_q_sample
        x0_hat = fd.diffusion.predict_start_from_noise

        def recording_x0_hat(x_t, t, noise):
            seen['raw'] = x0_hat(x_t, t, noise)
            return seen['raw']
        fd.diffusion.predict_start_from_noise = recording_x0_hat
        torch.manual_seed(case['noise_seed'])
        with torch.no_grad():
            ret = fd(vid.clone())
        # ... and check that tests/teacher_inputs.replay_t_noise replays them
        t, noise = replay_t_noise(tag)
        assert torch.equal(t, seen['t']) and torch.equal(noise, seen['noise']), tag
        out[f'{tag}_t'] = t.numpy()
        out[f'{tag}_noise'] = noise.numpy()
        # the thresholds s of the reference's own x0_hat (the parity bar of the grids depends on them)
        out[f'{tag}_s'] = torch.quantile(seen['raw'].reshape(case['B'], -1).abs(), 0.9, dim=-1).clamp(min=1.).numpy()
        for k in ('loss', 'rec_loss', 'rec_warp_loss'):
            out[f'{tag}_{k}'] = np.float32(ret[k].item())
        out[f'{tag}_fake_vid_grid'] = ret['fake_vid_grid'].numpy()
        out[f'{tag}_fake_vid_conf'] = ret['fake_vid_conf'].numpy()
        out[f'{tag}_fake_out_vid'] = ret['fake_out_vid'][..., ::OUT_STRIDE, ::OUT_STRIDE].contiguous().numpy()
        print('wrapper', tag, 't', t.tolist(), {k: float(ret[k]) for k in ('loss', 'rec_loss', 'rec_warp_loss')},
              'keys', sorted(ret))


def main():
    torch.set_num_threads(8)
    out = {}
    small(out)
    wrappers(out)
    path = os.path.join(HERE, 'teacher.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
