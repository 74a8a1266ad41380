"""GPU: the teacher-forced evaluation step (Diffusion.py:276-327 and the wrappers' forward) against
outputs of the reference itself (tests/golden/teacher.npz, tests/golden/make_golden_teacher.py).

  1  q_sample == the three-op fp32 torch expression, bitwise; seeded noise reproducible and
     independent of how the batch is sharded
  2  x0_loss on the reference's eps: thresholds bitwise vs torch.quantile, pred_x0 within 1e-6 (the
     one-update bar of test_ddpm_steps_vs_reference_golden), loss_sum within 1e-6 relative of an
     fp64 evaluation of the same fp32 tensors; at BAIR size (11 chunks, ties, mixed t and scales)
     thresholds and the unclipped x0 bitwise
  3  p_losses end to end, f16x3 and fp32. With e the forward's eps bar (1e-4 for u12),
     pred_x0 within 2 e max_b(sqrt_recipm1[t_b] / s_b) (x0_hat and s are both 1-Lipschitz in eps),
     l1 within e + 1e-6 |ref|, l2 within 100 (2 sqrt(ref / 100) e + e^2) + 1e-6 |ref|
  4  loss_sum[b] / pred_x0[b] bitwise for B = 4 vs two B = 2 halves vs a repeat
  5  p_sample / one DDIM update with a mixed t == the shared-t path per sample, bitwise
  6  FlowDiffusion(is_train=True).forward of the three wrappers vs the reference's
"""
import dataclasses
import importlib

import numpy as np
import pytest
import torch

from tests import parity_log
from tests.golden_inputs import CONFIGS, LFAE_CFG, PKG, lfae_config_dict, make_lfae_sd, make_sd
from tests.teacher_inputs import (OUT_STRIDE, SMALL, WRAP_TEACHER, replay_t_noise, small_case, wrapper_config,
                                  wrapper_video)
from tests.test_oracle_golden import load

pytestmark = pytest.mark.gpu
pkg = importlib.import_module(PKG)
spec = importlib.import_module(PKG + '.spec')
DEV = torch.device('cuda:0')
SCH = pkg.schedule_buffers(1000)
EPS_BAR = {'u12': 1e-4, 'ada_u22': 2e-4, 'wo_ref': 2e-4}  # DESIGN §7, Unet3D eps vs the reference
_H = {}


def handle(name, precision=None):
    if (name, precision) not in _H:
        cfg = CONFIGS[name]
        h = pkg._lib.Handle(cfg, 1000, 4, 0, precision=precision)
        sd = make_sd(cfg)
        sd.update(SCH)
        h.load_state(sd)
        h.finalize()
        _H[(name, precision)] = h
    return _H[(name, precision)]


def ex(name, t, B):
    return SCH[name][t.cpu()].reshape(B, 1, 1, 1, 1)


def dev(*xs):
    return [x.to(DEV).contiguous() for x in xs]


def x0_loss(h, t, xt, eps, noise, loss_type='l1', clip=True):
    B = xt.shape[0]
    pred = torch.empty_like(xt)
    sums = torch.full((B,), -1., device=DEV, dtype=torch.float64)
    th = torch.full((B,), -1., device=DEV)
    h.x0_loss(t, xt, eps, noise, loss_type, clip, pred, sums, th)
    torch.cuda.synchronize()
    return pred.cpu(), sums.cpu(), th.cpu()


def loss_terms64(noise, eps, loss_type):
    """Per-sample fp64 sums of the fp32 terms the reference's loss averages."""
    if loss_type == 'l1':
        term = (noise - eps).abs()
    else:
        d = noise * 10 - eps * 10
        term = d * d
    return term.double().reshape(term.shape[0], -1).sum(-1)


# ---- 1 ----
def test_q_sample_bitwise_seeded_and_shard_invariant():
    cfg, x0, _, _, t, noise = small_case()
    h = handle('small')
    B = x0.shape[0]
    want = ex('sqrt_alphas_cumprod', t, B) * x0 + ex('sqrt_one_minus_alphas_cumprod', t, B) * noise
    x0d, td, nd = dev(x0, t, noise)
    out = torch.empty_like(x0d)
    h.q_sample(td, x0d, out, noise=nd)
    assert torch.equal(out.cpu(), want)
    assert np.array_equal(out.cpu().numpy(), load('teacher.npz')['small_x_t'])
    # the seeded stream: reproducible, standard normal, x_t from the drawn noise bitwise
    runs = []
    for _ in range(2):
        z, o = torch.empty_like(x0d), torch.empty_like(x0d)
        h.q_sample(td, x0d, o, seed=1234, noise_out=z)
        runs.append((o.cpu(), z.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    o, z = runs[0]
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1) < 0.02
    assert torch.equal(o, ex('sqrt_alphas_cumprod', t, B) * x0 + ex('sqrt_one_minus_alphas_cumprod', t, B) * z)
    # another seed gives other noise
    z2 = torch.empty_like(x0d)
    h.q_sample(td, x0d, torch.empty_like(x0d), seed=1235, noise_out=z2)
    assert not torch.equal(z2.cpu(), z)
    # two B = 2 shards
    for base in (0, 2):
        zs, os_ = torch.empty_like(x0d[:2]), torch.empty_like(x0d[:2])
        h.q_sample(td[base:base + 2].contiguous(), x0d[base:base + 2].contiguous(), os_, seed=1234, sample_base=base,
                   noise_out=zs)
        assert torch.equal(zs.cpu(), z[base:base + 2]) and torch.equal(os_.cpu(), o[base:base + 2])


# ---- 2 ----
@pytest.mark.parametrize('loss_type', ['l1', 'l2'])
def test_x0_loss_on_reference_eps(loss_type):
    """n = 4608: two chunks, the second ragged (512 elements)."""
    g = load('teacher.npz')
    _, _, _, _, t, noise = small_case()
    B = SMALL['B']
    xt, eps = torch.from_numpy(g['small_x_t']), torch.from_numpy(g['small_eps'])
    pred, sums, th = x0_loss(handle('small'), *dev(t, xt, eps, noise), loss_type)
    raw = ex('sqrt_recip_alphas_cumprod', t, B) * xt - ex('sqrt_recipm1_alphas_cumprod', t, B) * eps
    ref_s = torch.quantile(raw.reshape(B, -1).abs(), 0.9, dim=-1).clamp(min=1.)
    assert torch.equal(th, ref_s), (th, ref_s)
    assert np.array_equal(th.numpy(), g['small_s'])
    parity_log.check(np.abs(pred.numpy() - g['small_pred_x0']).max(), 1e-6, 'pred_x0')
    want = loss_terms64(noise, eps, loss_type)
    parity_log.check(float(((sums - want).abs() / want).max()), 1e-6, f'loss_sum rel {loss_type}')
    ref = float(g[f'small_loss_{loss_type}'])
    parity_log.check(abs(float(sums.sum() / xt.numel()) - ref) / ref, 1e-6, f'mean loss rel {loss_type}')


def test_x0_loss_bair_size_ties_mixed_t():
    """n = 43 008 (11 chunks, the last ragged), heavy ties in one sample, mixed t and scales."""
    cfg = CONFIGS['bair']
    h = handle('bair')
    B, n = 4, 3 * cfg.tp * cfg.latent * cfg.latent
    assert n == 43008
    gen = torch.Generator().manual_seed(3)
    t = torch.tensor([999, 500, 3, 100])
    scale = torch.tensor([1.0, 3.0, 0.2, 50.0]).reshape(B, 1, 1, 1, 1)
    xt = torch.randn(B, 3, cfg.tp, cfg.latent, cfg.latent, generator=gen) * scale
    eps = torch.randn(xt.shape, generator=gen)
    noise = torch.randn(xt.shape, generator=gen)
    xt[1].view(-1)[: n // 2] = 0.25  # heavy ties
    raw = ex('sqrt_recip_alphas_cumprod', t, B) * xt - ex('sqrt_recipm1_alphas_cumprod', t, B) * eps
    ref_s = torch.quantile(raw.reshape(B, -1).abs(), 0.9, dim=-1).clamp(min=1.)
    args = dev(t, xt, eps, noise)
    pred, sums, th = x0_loss(h, *args, 'l2')
    assert torch.equal(th, ref_s), (th, ref_s)
    sv = ref_s.reshape(B, 1, 1, 1, 1)
    parity_log.check(float((pred - raw.clamp(-sv, sv) / sv).abs().max()), 1e-6, 'pred_x0 vs torch')
    want = loss_terms64(noise, eps, 'l2')
    parity_log.check(float(((sums - want).abs() / want).max()), 1e-6, 'loss_sum rel')
    # clip_denoised = 0: the raw x0_hat, no select passes (the threshold slot stays untouched)
    pred0, sums0, th0 = x0_loss(h, *args, 'l2', clip=False)
    assert torch.equal(pred0, raw)
    assert torch.equal(sums0, sums) and bool((th0 == -1).all())


# ---- 3 ----
def small_diffusion(loss_type, precision):
    cfg = CONFIGS['small']
    u = pkg.Unet3D(dim=cfg.dim, channels=512, dim_mults=cfg.dim_mults, cond_num=cfg.tc, pred_num=cfg.tp,
                   framesize=cfg.latent).to(DEV)
    u.load_state_dict(make_sd(cfg))
    u.precision = precision
    d = pkg.GaussianDiffusion(u, image_size=cfg.latent, num_frames=cfg.tc + cfg.tp, timesteps=1000,
                              sampling_timesteps=1000, loss_type=loss_type, null_cond_prob=0.0).to(DEV)
    d.max_batch = SMALL['B']
    return d


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_p_losses_vs_reference(precision):
    g = load('teacher.npz')
    _, x0, cond, fea, t, noise = small_case()
    e = EPS_BAR['u12']
    s = torch.from_numpy(g['small_s'])
    bar_x0 = 2 * e * float((SCH['sqrt_recipm1_alphas_cumprod'][t] / s).max())
    assert abs(bar_x0 - 4.8e-5) < 1e-6
    x0d, cd, fd, td, nd = dev(x0, cond, fea, t, noise)
    for lt in ('l1', 'l2'):
        d = small_diffusion(lt, precision)
        loss, pred = d.p_losses(cd, x0d, fd, td, noise=nd)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        ref = float(g[f'small_loss_{lt}'])
        bar = e + 1e-6 * ref if lt == 'l1' else 100 * (2 * (ref / 100) ** 0.5 * e + e * e) + 1e-6 * ref
        parity_log.check(abs(float(loss) - ref), bar, f'{lt} loss {precision}')
        parity_log.check(np.abs(pred.cpu().numpy() - g['small_pred_x0']).max(), bar_x0, f'pred_x0 {lt} {precision}')
    # forward: the same call with t given; a drawn t / seeded noise runs and is reproducible
    loss_f, pred_f = d.forward(cd, x0d, fd, t=td, noise=nd)
    assert torch.equal(loss_f, loss) and torch.equal(pred_f, pred)
    torch.manual_seed(3)
    a = d(cd, x0d, fd)
    torch.manual_seed(3)
    b = d(cd, x0d, fd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[1]).all())


# ---- 4 ----
def test_p_losses_batch_and_shard_invariant():
    _, x0, cond, fea, t, noise = small_case()
    x0d, cd, fd, td, nd = dev(x0, cond, fea, t, noise)
    d = small_diffusion('l1', None)
    full = d.p_losses(cd, x0d, fd, td, noise=nd, return_sums=True)
    again = d.p_losses(cd, x0d, fd, td, noise=nd, return_sums=True)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    seeded = d.p_losses(cd, x0d, fd, td, seed=5, return_sums=True)
    for base in (0, 2):
        sl = slice(base, base + 2)
        part = d.p_losses(cd[sl].contiguous(), x0d[sl].contiguous(), fd[sl].contiguous(), td[sl].contiguous(),
                          noise=nd[sl].contiguous(), return_sums=True)
        assert torch.equal(part[1], full[1][sl]) and torch.equal(part[2], full[2][sl])
        part = d.p_losses(cd[sl].contiguous(), x0d[sl].contiguous(), fd[sl].contiguous(), td[sl].contiguous(), seed=5,
                          sample_base=base, return_sums=True)
        assert torch.equal(part[1], seeded[1][sl]) and torch.equal(part[2], seeded[2][sl])
    assert float(full[0]) == float((full[2].sum() / x0.numel()).to(torch.float32))


# ---- 5 ----
def test_mixed_t_step_equals_shared_t_steps():
    _, x, cond, fea, _, noise = small_case()
    t = torch.tensor([999, 500, 1, 0])
    B = 4
    d = small_diffusion('l1', None)
    xd, cd, fd, td, nd = dev(x * 2, cond, fea, t, noise)
    mixed = d.p_sample(cd, xd, fd, td, noise=nd)
    for b in range(B):
        # the existing shared-t path: p_sample of the whole batch at t_b, sample b of it
        one = d.p_sample(cd, xd, fd, torch.full((B,), int(t[b]), dtype=torch.long, device=DEV), noise=nd)
        assert torch.equal(mixed[b], one[b]), b
    h = d._native(B, DEV, fea.shape[-1])
    eps = torch.empty_like(xd)
    h.unet_forward(xd, td, cd, fd, eps)
    # the Handle level takes int64 t only (the library reads B int64 values)
    with pytest.raises(RuntimeError, match='int64'):
        h.sampler_step_t(pkg._lib.SAMPLER_DDPM, td.int(), None, 0., xd.clone(), eps, nd)
    # one DDIM update (eta = 1), time pairs of DDIM-10 incl. a final step without noise
    tn = torch.tensor([899, 400, 0, 0])
    tm = torch.tensor([999, 500, 100, 100])
    out = xd.clone()
    th = torch.zeros(B, device=DEV)
    h.sampler_step_t(pkg._lib.SAMPLER_DDIM, *dev(tm, tn), 1.0, out, eps, nd, th)
    for b in range(B):
        one = xd.clone()
        th1 = torch.zeros(B, device=DEV)
        h.sampler_step(pkg._lib.SAMPLER_DDIM, int(tm[b]), int(tn[b]), 1.0, one, eps, nd[None].contiguous(), th1)
        torch.cuda.synchronize()
        assert torch.equal(out[b], one[b]) and th[b] == th1[b], b


# ---- 6 ----
_FD = {}


def wrapper_model(tag):
    if tag not in _FD:
        _FD[tag] = _wrapper_model(tag)
    return _FD[tag]


def _wrapper_model(tag):
    case = WRAP_TEACHER[tag]
    u = case['unet']
    cfgd = wrapper_config(tag)
    lc = spec.LfaeConfig.from_config(cfgd)
    fd = pkg.FlowDiffusion(config=cfgd, is_train=True, wrapper=case['wrapper'], dim_mults=u.dim_mults,
                           Unet3D_architecture=u.arch).to(DEV).eval()
    sds = make_lfae_sd(lc)
    fd.generator.load_state_dict(sds['generator'])
    fd.region_predictor.load_state_dict(sds['region_predictor'])
    fd.bg_predictor.load_state_dict(sds['bg_predictor'])
    fd.unet.load_state_dict(make_sd(u))
    return fd, lc


@pytest.mark.parametrize('tag', sorted(WRAP_TEACHER))
def test_wrapper_forward_vs_reference(tag):
    g = load('teacher.npz')
    case = WRAP_TEACHER[tag]
    u = case['unet']
    fd, lc = wrapper_model(tag)
    vid = wrapper_video(tag, lc.image).to(DEV)
    t, noise = replay_t_noise(tag)
    ret = fd(vid, t=t.to(DEV), noise=noise.to(DEV))
    assert sorted(ret) == ['fake_out_vid', 'fake_vid_conf', 'fake_vid_grid', 'fake_warped_vid', 'loss', 'real_out_vid',
                           'real_vid_conf', 'real_vid_grid', 'real_warped_vid', 'rec_loss', 'rec_warp_loss']
    assert ret['real_vid_grid'].shape[2] == u.tc + u.tp
    e = EPS_BAR[u.short]
    bar_x0 = 2 * e * float((SCH['sqrt_recipm1_alphas_cumprod'][t] / torch.from_numpy(g[f'{tag}_s'])).max())
    ref = float(g[f'{tag}_loss'])  # the configs' loss_type is l2
    assert fd.diffusion.loss_type == 'l2'
    parity_log.check(abs(float(ret['loss']) - ref), 100 * (2 * (ref / 100) ** 0.5 * e + e * e) + 1e-6 * ref, 'loss')
    for k in ('fake_vid_grid', 'fake_vid_conf'):
        parity_log.check(np.abs(ret[k].cpu().numpy() - g[f'{tag}_{k}']).max(), bar_x0, k)
    out = ret['fake_out_vid'][..., ::OUT_STRIDE, ::OUT_STRIDE].cpu().numpy()
    parity_log.check(np.abs(out - g[f'{tag}_fake_out_vid']).max(), case['out_bar'], 'fake_out_vid')
    scale = 10 if case['wrapper'] == 'multi_w_ref_u22' else 1  # both rec losses x 10 (multi_w_ref_u22.py:397-398)
    for k in ('rec_loss', 'rec_warp_loss'):
        assert ret[k].dim() == 0
        parity_log.check(abs(float(ret[k]) - float(g[f'{tag}_{k}'])), case['out_bar'], k)
    tgt = vid[:, :, u.tc:].contiguous()
    want = (tgt.double() * scale - ret['fake_out_vid'].double() * scale).abs().mean()
    assert abs(float(ret['rec_loss']) - float(want)) <= 1e-6 * float(want)


def test_wrapper_forward_eval_mode_and_missing_occlusion():
    fd, lc = wrapper_model('fd')
    fd.is_train = False  # as constructed with is_train=False: the real_* keys only, like the reference
    try:
        ret = fd(wrapper_video('fd', lc.image).to(DEV))
    finally:
        fd.is_train = True
    assert sorted(ret) == ['real_out_vid', 'real_vid_conf', 'real_vid_grid', 'real_warped_vid']
    lc0 = dataclasses.replace(LFAE_CFG, pf_estimate_occlusion_map=False)
    u = WRAP_TEACHER['fd']['unet']
    fd0 = pkg.FlowDiffusion(config=lfae_config_dict(lc0, u, False), is_train=True, dim_mults=u.dim_mults,
                            Unet3D_architecture=u.arch)  # raises before any device work
    with pytest.raises(KeyError, match='occlusion_map'):
        fd0(wrapper_video('fd', lc0.image).to(DEV))


def test_abs_diff_sum_fixed_order():
    gen = torch.Generator().manual_seed(9)
    a = torch.randn(3, 3, 5, 37, 41, generator=gen)  # n = 22 755: odd, six chunks, no 16-byte path
    b = torch.randn(a.shape, generator=gen)
    ad, bd = dev(a, b)
    s1, s2 = pkg._lib.abs_diff_sum(ad, bd), pkg._lib.abs_diff_sum(ad, bd)
    want = (a - b).abs().double().reshape(3, -1).sum(-1)
    assert torch.equal(s1, s2)
    assert float(((s1.cpu() - want).abs() / want).max()) <= 1e-12
    assert torch.equal(pkg._lib.abs_diff_sum(ad[1:].contiguous(), bd[1:].contiguous()), s1[1:])
