"""GPU: the DPM-Solver++(2M) sampler (EXTDM_SAMPLER_DPMPP, sampler.hip's history kernels) on the
`small` denoiser, n = 4608 per sample = one full 4096-element chunk + one partial chunk.

  one step (first / middle / final) vs the torch restatement tests/dpmpp_ref.py: thresholds bitwise
      torch.quantile's; x and the written-back x0_prev within 2x the fp32 restatement's own error
      against its fp64 twin (the margin covers another, fixed association of the three-term sum)
  one-workgroup form == multi-workgroup form, bit for bit (two helper processes)
  extdm_sample (graph and eager) == a Python loop of unet_forward + extdm_sampler_step_hist, bit
      for bit, thresholds included, on both grids
  shard and repeat invariance; the history buffer does not leak into DDIM or across calls
  GaussianDiffusion.sample dispatch through the `sampler` attribute

The solver is not in the reference, so nothing here is pinned against it."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

from tests import dpmpp_ref as R
from tests import parity_log
from tests.dpmpp_run import (LOOP_B, STEP_B, STEP_CASES, T, loop_inputs, loop_times, run_all, run_loop, run_step,
                             small_handle, step_inputs)
from tests.golden_inputs import CONFIGS, PKG, unet_inputs

pytestmark = pytest.mark.gpu
pkg = importlib.import_module(PKG)
DEV = torch.device('cuda:0')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCH = pkg.schedule_buffers(T)
_H = []


def handle():
    if not _H:
        _H.append(small_handle(4))
    return _H[0]


@pytest.mark.parametrize('case', list(STEP_CASES))
def test_step_matches_restatement(case):
    t_prev, t, t_next = STEP_CASES[case]
    x, eps, prev = step_inputs()
    c = R.coefs(SCH['alphas_cumprod'], t_prev, t, t_next)
    sra, srm1 = SCH['sqrt_recip_alphas_cumprod'][t], SCH['sqrt_recipm1_alphas_cumprod'][t]
    x32, p32, s32 = R.step32(x, eps, prev, sra, srm1, c)
    x64, p64, _ = R.step64(x, eps, prev, sra, srm1, c)
    xn, pn, sn = run_step(handle(), case, DEV)
    assert float(s32[0]) > 1.0 and float(s32[1]) == 1.0, s32  # one sample thresholds, one does not
    assert torch.equal(sn, s32), (sn, s32)
    for what, nat, r32, r64 in (('x', xn, x32, x64), ('x0_prev', pn, p32, p64)):
        e_ref = float((r32.double() - r64).abs().max())
        e_nat = float((nat.double() - r64).abs().max())
        parity_log.check(e_nat, 2 * e_ref, f'{case} {what} native vs fp64 (fp32 restatement vs fp64: {e_ref:.3e})')
    if t_prev < 0:
        # the first-order start: the history weight is 0, the history is still written
        assert c[2] == 0.0
    assert not torch.equal(pn, prev)


def test_step_on_unaligned_tensors_equals_aligned():
    """x, eps and x0_prev one element past a 16-byte boundary: the multi-workgroup form takes its
    element-wise path instead of the 16-byte one; same arithmetic, so bitwise the aligned result."""
    h = handle()
    xa, pa, sa = run_step(h, 'middle', DEV)
    views = []
    for v in step_inputs():
        buf = torch.empty(v.numel() + 1, device=DEV)
        u = buf[1:].view(v.shape)
        u.copy_(v)
        assert u.is_contiguous() and u.data_ptr() % 16 == 4
        views.append(u)
    x, eps, prev = views
    th = torch.full((STEP_B,), -1., device=DEV)
    h.sampler_step_hist(*STEP_CASES['middle'], x, eps, prev, th)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), xa) and torch.equal(prev.cpu(), pa) and torch.equal(th.cpu(), sa)


def test_one_workgroup_form_equals_multi_workgroup(tmp_path):
    """The three steps and one graph sampling call in two helper processes, EXTDM_SAMPLER_1WG=0 / 1."""
    res = {}
    for form in ('0', '1'):
        dump = tmp_path / f'form{form}.pt'
        env = dict(os.environ, EXTDM_SAMPLER_1WG=form)
        p = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'dpmpp_run.py'), '--out', str(dump)],
                           cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        res[form] = torch.load(dump, weights_only=True)
    here = run_all(handle(), DEV)  # this process's library state
    assert set(res['0']) == set(res['1']) == set(here)
    for k in res['0']:
        assert torch.equal(res['0'][k], res['1'][k]), k
        assert torch.equal(res['0'][k], here[k]), k
    assert bool((res['0']['loop_thresh'] >= 1).all())


@pytest.mark.parametrize('spacing', ['ddim', 'logsnr'])
def test_loop_equals_steps(spacing):
    h = handle()
    times = loop_times(spacing)
    S = len(times)
    out_g, rec_g = run_loop(h, times, DEV, use_graph=True)
    out_e, rec_e = run_loop(h, times, DEV, use_graph=False)
    cond, fea, xT = loop_inputs()
    x = xT.to(DEV).contiguous()
    cd, fd = cond.to(DEV), fea.to(DEV)
    prev = torch.zeros_like(x)
    rec = torch.full((S, LOOP_B), -1., device=DEV)
    for k, t in enumerate(times):
        eps = torch.empty_like(x)
        h.unet_forward(x, torch.full((LOOP_B,), t, dtype=torch.long, device=DEV), cd, fd, eps)
        h.sampler_step_hist(times[k - 1] if k else -1, t, times[k + 1] if k + 1 < S else -1, x, eps, prev, rec[k])
    torch.cuda.synchronize()
    assert torch.isfinite(out_g).all()
    assert torch.equal(out_g, out_e) and torch.equal(out_g, x.cpu())
    assert torch.equal(rec_g, rec_e) and torch.equal(rec_g, rec.cpu())
    assert bool((rec_g >= 1).all())
    # the final step ends at the thresholded x0, which is also the history it leaves
    assert torch.equal(x, prev)


def _dpmpp(h, cond, fea, times, base, seed=99):
    cfg = CONFIGS['small']
    out = torch.empty((cond.shape[0], 3, cfg.tp, cfg.latent, cfg.latent), device=DEV)
    h.sample(pkg._lib.SAMPLER_DPMPP, times, None, 0., cond.contiguous(), fea.contiguous(), out, seed=seed,
             sample_base=base, use_graph=True)
    torch.cuda.synchronize()
    return out.cpu()


def _ddim(h, cond, fea, seed=99):
    cfg = CONFIGS['small']
    pairs = pkg.ddim_time_pairs(T, 4)
    out = torch.empty((cond.shape[0], 3, cfg.tp, cfg.latent, cfg.latent), device=DEV)
    h.sample(pkg._lib.SAMPLER_DDIM, [p[0] for p in pairs], [p[1] for p in pairs], 1.0, cond.contiguous(),
             fea.contiguous(), out, seed=seed, use_graph=True)
    torch.cuda.synchronize()
    return out.cpu()


def test_shard_and_repeat_invariance_and_no_history_leak():
    h = handle()
    _, _, cond, fea = unet_inputs(CONFIGS['small'], B=4, seed=73)
    cd, fd = cond.to(DEV), fea.to(DEV)
    times = loop_times('logsnr')
    ddim_before = _ddim(h, cd, fd)
    whole = _dpmpp(h, cd, fd, times, 0)
    assert torch.isfinite(whole).all()
    halves = [_dpmpp(h, cd[b:b + 2], fd[b:b + 2], times, b) for b in (0, 2)]
    assert torch.equal(torch.cat(halves), whole)
    assert torch.equal(_dpmpp(h, cd, fd, times, 0), whole)
    # a DDIM call between two DPM-Solver++ calls: none of the three changes
    assert torch.equal(_ddim(h, cd, fd), ddim_before)
    assert torch.equal(_dpmpp(h, cd, fd, times, 0), whole)
    # and the history left by a 4-sample call does not reach a later 2-sample call
    assert torch.equal(_dpmpp(h, cd[2:4], fd[2:4], times, 2), halves[1])


def test_python_surface():
    cfg = CONFIGS['small']
    u = pkg.Unet3D(dim=cfg.dim, channels=512, dim_mults=cfg.dim_mults, cond_num=cfg.tc, pred_num=cfg.tp,
                   framesize=cfg.latent).to(DEV)
    d = pkg.GaussianDiffusion(u, image_size=cfg.latent, num_frames=cfg.tc + cfg.tp, timesteps=T,
                              sampling_timesteps=6).to(DEV)
    _, _, cond, fea = unet_inputs(cfg)
    cd, fd = cond.to(DEV), fea.to(DEV)
    shape = (2, 3, cfg.tp, cfg.latent, cfg.latent)
    assert d.sampler is None
    assert torch.equal(d.sample(cd, cond_fea=fd, seed=7), d.ddim_sample(cd, shape, fd, seed=7))
    d.sampler = 'dpmpp_2m'
    for spacing in ('ddim', 'logsnr'):
        d.sampler_spacing = spacing
        a = d.sample(cd, cond_fea=fd, seed=7)
        assert torch.isfinite(a).all()
        assert torch.equal(a, d.dpmpp_sample(cd, shape, fd, spacing=spacing, seed=7))
    assert not torch.equal(d.dpmpp_sample(cd, shape, fd, spacing='ddim', seed=7), a)
    assert torch.equal(d.dpmpp_sample(cd, shape, fd, steps=6, spacing='logsnr', seed=7), a)
    with pytest.raises(ValueError, match='no noise'):
        d.sample(cd, cond_fea=fd, noise=torch.zeros(6, *shape, device=DEV))
    # the single-step entry points of the other samplers refuse the new id
    h = handle()
    x, eps, _ = [v.to(DEV).contiguous() for v in step_inputs()]
    with pytest.raises(RuntimeError, match='extdm_sampler_step_hist'):
        h.sampler_step(pkg._lib.SAMPLER_DPMPP, 500, 400, 0., x, eps)
    tt = torch.full((STEP_B,), 500, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match='multistep'):
        h.sampler_step_t(pkg._lib.SAMPLER_DPMPP, tt, tt - 100, 0., x, eps)
    with pytest.raises(RuntimeError, match='takes no noise'):
        cond, fea, xT = loop_inputs()
        out = torch.empty(xT.shape, device=DEV)
        h.sample(pkg._lib.SAMPLER_DPMPP, loop_times('ddim'), None, 0., cond.to(DEV), fea.to(DEV), out,
                 x_T=xT.to(DEV), noise=torch.zeros(6, *xT.shape, device=DEV))
