"""GPU: the one-term fp16 conv modes, 'f16_conv' (EXTDM_PRECISION_F16_CONV: one fp16 MFMA per
product, hi(a) hi(b), in the convolutions of the denoiser forward; everything else as f16x3) and
'f16' (the same plus the bf16 attention routing of 'bf16_attn').

Not fp32-faithful. The yardstick is the CPU emulation of tests/f16_emul.py (the oracle with every
conv operand rounded to fp16), measured against the reference's golden vectors, never against the
library. With err = max|eps - golden|, scale = max|golden|, emu = max|emulated_eps - golden|:

    f16_conv:  err <= 2 emu
    f16:       err <= 2 emu + 5e-3 scale     (the bf16 attention bar of tests/test_gpu_bf16_attn.py)

2 x: the emulation is one rounding realisation with another fp32 summation order; the library rounds
the same operands (a subset where a kernel stays three-term; composed weights in the phase-composed
cond_fea conv), and the emulated error spreads +-15 % over the eight configs.

Every case prints err, emu and the f16x3 error with -s and logs them through tests/parity_log.py."""
import dataclasses
import functools
import importlib
import re
import warnings

import numpy as np
import pytest
import torch

from tests import f16_emul, parity_log
from tests.golden_inputs import (CONFIGS, FD_UNET, GOLDEN_BATCH, LFAE_CFG, PKG, decoder_inputs, lfae_config_dict,
                                 make_gen_sd, make_lfae_sd, make_sd, unet_inputs, video_inputs)
from tests.test_oracle_golden import load

pytestmark = pytest.mark.gpu
pkg = importlib.import_module(PKG)
DEV = torch.device('cuda:0')
BF16_REL = 5e-3
MODES = ('f16_conv', 'f16')


def make_handle(name, precision, max_batch=2, timesteps=1000):
    cfg = CONFIGS[name]
    h = pkg._lib.Handle(cfg, timesteps, max_batch, 0, precision=precision)
    sd = make_sd(cfg)
    sd.update(pkg.schedule_buffers(timesteps))
    h.load_state(sd)
    h.finalize()
    return h


@functools.lru_cache(maxsize=None)
def handle(name, precision):
    return make_handle(name, precision)


def forward(h, x, t, cond, fea):
    out = torch.empty(x.shape, device=DEV)
    h.unet_forward(x.to(DEV).contiguous(), t.to(DEV), cond.to(DEV).contiguous(), fea.to(DEV).contiguous(), out)
    torch.cuda.synchronize()
    return out.cpu()


def golden_forward(name, precision, h=None):
    cfg = CONFIGS[name]
    x, t, cond, fea = unet_inputs(cfg, B=GOLDEN_BATCH.get(name, 2))
    return forward(h or handle(name, precision), x, t, cond, fea).numpy()


@functools.lru_cache(maxsize=None)
def eps_of(name, precision):
    """eps of the golden inputs in one mode, computed once per session and left unchanged."""
    e = golden_forward(name, precision)
    e.setflags(write=False)
    return e


# ---- 1. the forward within the bar, 2. the mode is really on -----------------------------------
@pytest.mark.parametrize('name', f16_emul.EMUL_CONFIGS)
@pytest.mark.parametrize('mode', MODES)
def test_forward_within_twice_the_emulated_error(mode, name):
    g = f16_emul.golden_eps(name)
    emu, scale = f16_emul.emulated_error(name)
    e = eps_of(name, mode)
    e3 = eps_of(name, 'f16x3')
    err = np.abs(e - g).max()
    err3 = np.abs(e3 - g).max()
    print(f'{name} {mode}: max|err| {err:.3e} = {err / scale:.2e} x max|eps| (emulated {emu / scale:.2e}, '
          f'f16x3 {err3 / scale:.2e})')
    assert np.isfinite(e).all()
    bar = 2 * emu + (BF16_REL * scale if mode == 'f16' else 0.0)
    parity_log.check(err, bar, f'{mode} {name}, emulated {emu:.3e}, max|eps_ref| {scale:.3e}')
    # the mode is on: a different arithmetic from f16x3, and its error is the operand rounding's,
    # three orders of magnitude above f16x3's (10 x leaves two on either side)
    assert not np.array_equal(e, e3)
    if mode == 'f16_conv':
        assert err > 10 * err3, (err, err3)


def test_f16_differs_from_f16_conv_where_the_bf16_attention_runs():
    assert not np.array_equal(eps_of('bair', 'f16'), eps_of('bair', 'f16_conv'))
    # and f16 is not bf16_attn either: its convs are one-term
    assert not np.array_equal(eps_of('bair', 'f16'), eps_of('bair', 'bf16_attn'))


# ---- 3. routes ---------------------------------------------------------------------------------
# conv_x3_kernel's parameters after the ten tile ones: XOP, RGN, SPL, PH, WS, BX, TT, AFF, TERMS
X3_TRAILING = ['false', 'false', '0', 'false', 'false', 'false', '0', '0', '3']
TERM_FAMILIES = ('conv_x3_kernel', 'conv_gemm_x3_kernel', 'pw_x3_kernel')
BENCH_LAYERS = (0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 18, 19, 20, 21)


def parse_kernel(name):
    m = re.fullmatch(r'(\w+)<(.*)>', name)
    assert m, name
    args = [a.strip() for a in m.group(2).split(',')]
    if m.group(1) == 'conv_x3_kernel':
        assert 10 <= len(args) <= 19, name
        args = args + X3_TRAILING[len(args) - 10:]
    return m.group(1), args


def bench_kernels(precision):
    h = handle('bair', precision)
    names = {}
    for layer in BENCH_LAYERS:
        try:
            h.bench_layer(2, layer, 1)
        except RuntimeError:
            continue  # a layer this config does not have
        names[layer] = h.bench_layer_kernel(layer)
    return names


def test_bench_layers_name_the_one_term_instantiations():
    k3 = bench_kernels('f16x3')
    term_layers = [l for l, n in k3.items() if n.startswith(TERM_FAMILIES)]
    assert len(term_layers) >= 6, k3  # the hot convs of a BAIR step are among the ids
    for mode in MODES:
        km = bench_kernels(mode)
        assert sorted(km) == sorted(k3)
        for layer, n3 in k3.items():
            if layer not in term_layers:
                # attention, and the kernels documented as three-term in every mode
                if not n3.startswith(('stw', 'temporal', 'attn')):
                    assert km[layer] == n3, (mode, layer, km[layer], n3)
                continue
            id3, a3 = parse_kernel(n3)
            idm, am = parse_kernel(km[layer])
            print(f'layer {layer} {mode}: {km[layer]}')
            assert idm == id3 and am[:-1] == a3[:-1], (mode, layer, km[layer], n3)
            assert a3[-1] == '3' and am[-1] == '1', (mode, layer, km[layer], n3)


# ---- 4. no leak between handles ----------------------------------------------------------------
@pytest.mark.parametrize('name', ['small', 'bair'])
def test_no_leak_between_handles_of_different_modes(name):
    first = golden_forward(name, 'f16x3', make_handle(name, 'f16x3'))
    h16 = make_handle(name, 'f16')
    e16 = golden_forward(name, 'f16', h16)
    del h16
    h3 = make_handle(name, 'f16x3')
    last = golden_forward(name, 'f16x3', h3)
    assert np.array_equal(first, last)
    assert not np.array_equal(first, e16)
    # both alive, alternating calls
    h16 = make_handle(name, 'f16')
    for _ in range(2):
        assert np.array_equal(golden_forward(name, 'f16', h16), e16)
        assert np.array_equal(golden_forward(name, 'f16x3', h3), first)


# ---- 5. scope: the LFAE entry points run f16x3 bit for bit ------------------------------------
def _lfae_outputs():
    src, flow, occ = decoder_inputs()
    gen = pkg.Generator()
    gen.load_state_dict(make_gen_sd())
    dec = gen.forward_with_flow(src.to(DEV), flow.to(DEV), occ.to(DEV))
    lc = dataclasses.replace(LFAE_CFG, pf_estimate_occlusion_map=True)
    fd = pkg.FlowDiffusion(config=lfae_config_dict(lc, FD_UNET, True), is_train=False, dim_mults=FD_UNET.dim_mults,
                           Unet3D_architecture='DenoiseNet_STWAtt_w_w_ref_adaptor_cross_multi_traj_u12').to(DEV)
    fd.region_predictor.load_state_dict(make_lfae_sd(lc)['region_predictor'])
    rp = fd.region_predictor(video_inputs()[:, :, 1].contiguous().to(DEV))
    assert gen._handle[4].precision == fd.region_predictor._handle[4].precision == pkg._lib.DEFAULT_PRECISION
    out = {'prediction': dec['prediction'], 'deformed': dec['deformed']}
    out.update({'rp_' + k: rp[k] for k in ('shift', 'covar', 'affine', 'heatmap')})
    return {k: v.cpu() for k, v in out.items()}


def test_decode_and_region_params_do_not_change_in_mode_f16(monkeypatch):
    """EXTDM_PRECISION=f16 (_lib.DEFAULT_PRECISION) reaches the LFAE modules' handles too; extdm_decode
    on the inputs of tests/golden/decoder.npz and extdm_region_params on the LFAE golden inputs give
    the bits of an f16x3 handle holding the same weights."""
    monkeypatch.setattr(pkg._lib, 'DEFAULT_PRECISION', 'f16x3')
    a = _lfae_outputs()
    monkeypatch.setattr(pkg._lib, 'DEFAULT_PRECISION', 'f16')
    b = _lfae_outputs()
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    g = load('decoder.npz')
    parity_log.check(np.abs(b['prediction'].numpy() - g['pred_occ']).max(), 2e-5, 'decoder in f16')


# ---- 6. the range flag --------------------------------------------------------------------------
def test_range_flag_and_fp32_fallback():
    """A one-term conversion of |v| >= 65520 is an inf: the staging raises the range flag at
    |v| >= 65504 as in f16x3, extdm_sample rejects the call and GaussianDiffusion re-runs it on FP32
    with one warning (modelled on test_gpu_parity.test_range_guard_falls_back_to_fp32)."""
    cfg = CONFIGS['small']
    x, t, cond, fea = unet_inputs(cfg)
    big = fea * 1e5  # TrajWarp's k / v projection inputs past the fp16 range
    h = handle('small', 'f16_conv')
    h.range_flag(reset=True)
    forward(h, x, t, cond, fea)
    assert h.range_flag(reset=True) == 0
    forward(h, x, t, cond, big)
    assert h.range_flag(reset=True) & 1
    assert h.range_flag() == 0

    def make(precision):
        u = pkg.Unet3D(dim=cfg.dim, channels=512, dim_mults=cfg.dim_mults, cond_num=cfg.tc, pred_num=cfg.tp,
                       framesize=cfg.latent).to(DEV)
        u.precision = precision
        return pkg.GaussianDiffusion(u, image_size=cfg.latent, num_frames=cfg.tc + cfg.tp, timesteps=1000,
                                     sampling_timesteps=3).to(DEV)
    shape = (2, 3, cfg.tp, cfg.latent, cfg.latent)
    ref = make('fp32').ddim_sample(cond.to(DEV), shape, big.to(DEV), seed=11)
    for mode in MODES:
        d = make(mode)
        with pytest.warns(RuntimeWarning, match='65504') as rec:
            a = d.ddim_sample(cond.to(DEV), shape, big.to(DEV), seed=11)
        assert len([w for w in rec if '65504' in str(w.message)]) == 1
        assert d._fp32_fallback and d.denoise_fn.precision == mode
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(ref))
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            c = d.ddim_sample(cond.to(DEV), shape, big.to(DEV), seed=11)
        assert torch.equal(torch.nan_to_num(c), torch.nan_to_num(ref))


# ---- 7. determinism ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['small', 'bair'])
def test_mode_f16_is_deterministic(name):
    cfg = CONFIGS[name]
    h = handle(name, 'f16')
    x, t, cond, fea = unet_inputs(cfg, B=2)
    t = torch.tensor([500, 500])
    a = forward(h, x, t, cond, fea)
    assert torch.equal(a, forward(h, x, t, cond, fea))
    # a clip's bits do not depend on the batch it is in
    one = forward(h, x[:1], t[:1], cond[:1], fea[:1])
    assert torch.equal(a[:1], one)
    two = forward(h, x[1:], t[1:], cond[1:], fea[1:])
    assert torch.equal(a[1:], two)
    # the captured step equals the eager one over 3 DDIM steps
    pairs = pkg.ddim_time_pairs(1000, 3)
    outs = {}
    for use_graph in (True, False):
        o = torch.empty(x.shape, device=DEV)
        h.sample(1, [p[0] for p in pairs], [p[1] for p in pairs], 1.0, cond.to(DEV), fea.to(DEV), o, seed=1234,
                 use_graph=use_graph)
        torch.cuda.synchronize()
        outs[use_graph] = o.cpu()
    assert torch.isfinite(outs[True]).all()
    assert torch.equal(outs[True], outs[False])


# ---- 8. chains -------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ddpm10', 'ddim10'])
@pytest.mark.parametrize('mode', MODES)
def test_chain_within_twice_the_emulated_chain(mode, kind):
    """The DDPM-10 / DDIM-10 chains of tests/golden/sampler_small.npz with their injected noise (as
    test_gpu_parity runs them): the final sample's error against the golden is at most twice that of
    the same chain through the oracle's sampler with the emulated forward (+ the bf16 term in 'f16')."""
    cfg = CONFIGS['small']
    x, _, cond, fea = unet_inputs(cfg)
    g = load('sampler_small.npz')[kind]
    out = torch.empty(x.shape, device=DEV)
    if kind == 'ddpm10':
        h = make_handle('small', mode, timesteps=10)
        torch.manual_seed(7)
        xT = torch.randn(x.shape)
        noises = torch.stack([torch.randn(x.shape) for _ in range(10)])
        h.sample(0, list(range(9, -1, -1)), None, 0., cond.to(DEV), fea.to(DEV), out, x_T=xT.to(DEV),
                 noise=noises.to(DEV).contiguous())
    else:
        h = handle('small', mode)
        pairs = pkg.ddim_time_pairs(1000, 10)
        torch.manual_seed(11)
        xT = torch.randn(x.shape)
        noises = torch.stack([torch.randn(x.shape) for _ in range(10)])
        h.sample(1, [p[0] for p in pairs], [p[1] for p in pairs], 1.0, cond.to(DEV), fea.to(DEV), out,
                 x_T=xT.to(DEV), noise=noises.to(DEV).contiguous())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isfinite(o).all()
    err = np.abs(o - g).max()
    emu = np.abs(f16_emul.emulated_chain(kind) - g).max()
    scale = np.abs(g).max()
    print(f'{kind} {mode}: final-sample max|err| {err:.3e} (emulated chain {emu:.3e}, max|x0| {scale:.3e})')
    bar = 2 * emu + (BF16_REL * scale if mode == 'f16' else 0.0)
    parity_log.check(err, bar, f'{mode} {kind}, emulated {emu:.3e}')
