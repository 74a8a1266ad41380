"""GPU: clips of 33..64 model frames — the 64-slot temporal attention (one pixel's frames in a
64-token group, T5 table [heads][64][64]) through single layers, whole forwards and the sampler,
against the CPU oracle (pinned to the reference beyond 32 frames by tests/test_long_clips_cpu.py).

Reduced configs (latent 16, cond_fea 8; wo_ref: 16) at the reference's long horizons:
  u12      2 -> 31   D = 33   one live slot in the second 32-token tile
  ada     10 -> 40   D = 50   dim_head 16, the KTH long horizon
  ada_u22  4 -> 60   D = 64   the full group, no masked key
Per-level temporal layers exist only in ada_u22 (downs.i.5); u12 / ada / wo_ref have
init_temporal_attn (C = 64), ada also cond_temporal_attn (C = 256, dim_head 16, on cond_fea).

Bars: the attention layers' ATT_BAR (tests/test_gpu_attn.py: 6e-6 on |out| ~ 1-4), the bf16 bar
of the 64-token windows (1e-2 x max|attention increment|), 1e-4 on eps (tests/test_gpu_parity.py)
and, for the sampler, 1e-4 on x after a step (tests/test_gpu_sampler.py: the eps bar carried
through the update), here on the chain's output after its four steps.

The cases are the reference's own sizes at dim 64: its MotionAdaptor Tmodulator weights grow with
the square of the frame count (0.28 / 0.79 / 1.1 G parameters at 33 / 50 / 64 frames), so building a
handle, not the launches, is what a case costs; handles and weights are shared per config."""
import importlib

import pytest
import torch

from tests import parity_log
from tests.golden_inputs import PKG, make_sd, unet_inputs

pytestmark = pytest.mark.gpu
ATT_BAR = 6e-6
pkg = importlib.import_module(PKG)
spec = pkg.spec
DEV = torch.device('cuda:0')
_for = spec.UnetConfig.for_arch

LONG = {
    'u12_33': spec.UnetConfig(tc=2, tp=31, latent=16, fea_size=8),
    'ada_50': _for(spec.ARCH_ADA, tc=10, tp=40, latent=16, fea_size=8),
    'u22_64': _for(spec.ARCH_ADA_U22, tc=4, tp=60, latent=16, fea_size=8),
    'woref_39': _for(spec.ARCH_WO_REF, tc=10, tp=30, latent=16),
    'u12_40_dim16': spec.UnetConfig(dim=16, tc=2, tp=38, latent=16, fea_size=8),
}
_H = {}
_SD = {}


def sd_of(name):
    if name not in _SD:
        _SD[name] = make_sd(LONG[name])
    return _SD[name]


def handle(name, precision='f16x3'):
    """One handle per (config, precision); ada_50's holds 3 clips for the batch-independence test."""
    key = (name, precision)
    max_batch = 3 if name == 'ada_50' else 2
    if key not in _H:
        h = pkg._lib.Handle(LONG[name], 1000, max_batch, 0, precision=precision)
        sd = dict(sd_of(name))
        sd.update(pkg.schedule_buffers(1000))
        h.load_state(sd)
        h.finalize()
        _H[key] = h
    return _H[key]


def layer_case(name, prefix, level, precision, seed=61):
    """One temporal layer at B = 2 on randn * 1.5 + 0.3, launched twice (bit-equal)."""
    from oracle import extdm_oracle as O
    cfg = LONG[name]
    h, sd = handle(name, precision), sd_of(name)
    C = sd[prefix + '.fn.fn.fn.attn.to_qkv.weight'].shape[1]
    L = cfg.fea_size if prefix == 'cond_temporal_attn' else cfg.latent >> level
    gen = torch.Generator().manual_seed(seed + level)
    x = torch.randn(2, C, cfg.frames, L, L, generator=gen) * 1.5 + 0.3
    out = torch.empty(x.shape, device=DEV)
    h.attn_layer(prefix, x.to(DEV), out, shifted=False)
    torch.cuda.synchronize()
    out2 = torch.empty(x.shape, device=DEV)
    h.attn_layer(prefix, x.to(DEV), out2, shifted=False)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), out2.cpu())
    with torch.no_grad():
        ref = O.temporal_attention(sd, prefix, x, O.time_pos_bias(sd, cfg.frames), cfg.heads, cfg.dim_head)
    return x, out.cpu(), ref, C


# (config, layer, latent halvings): C = 64 and C = 128 layers
F16X3_LAYERS = [('u12_33', 'init_temporal_attn', 0), ('ada_50', 'init_temporal_attn', 0),
                ('u22_64', 'init_temporal_attn', 0), ('u22_64', 'downs.1.5', 1)]


@pytest.mark.parametrize('name,prefix,level', F16X3_LAYERS)
def test_temporal_layer_f16x3_vs_oracle(name, prefix, level):
    x, out, ref, C = layer_case(name, prefix, level, 'f16x3')
    assert C == (64 if level == 0 else 128)
    err = (out - ref).abs().max().item()
    parity_log.check(err, ATT_BAR, f'{name} {prefix} C={C} D={LONG[name].frames}')


@pytest.mark.parametrize('name', ['u12_33', 'ada_50'])
def test_temporal_layer_f16x3_per_lane_path_vs_oracle(name, monkeypatch):
    """The fused kernel's per-lane loads and stores (what C = 128 and unaligned geometries take)
    with masked frame slots, forced at C = 64 by EXTDM_T64_NO_TILE (read per call): the bits of
    the LDS-tile path."""
    x, tile, ref, _ = layer_case(name, 'init_temporal_attn', 0, 'f16x3')
    monkeypatch.setenv('EXTDM_T64_NO_TILE', '1')
    _, out, _, _ = layer_case(name, 'init_temporal_attn', 0, 'f16x3')
    assert torch.equal(out, tile)
    parity_log.check((out - ref).abs().max().item(), ATT_BAR, f'{name} per-lane D={LONG[name].frames}')


@pytest.mark.parametrize('name,prefix,level', [('ada_50', 'cond_temporal_attn', 1), ('u22_64', 'downs.2.5', 2)])
def test_temporal_layer_c256_core_vs_oracle(name, prefix, level):
    """C = 256: the unfused route with the 64-slot attention core (dim_head 16 at D = 50: ada's
    cond_temporal_attn on cond_fea; dim_head 32 at D = 64: ada_u22 level 2)."""
    x, out, ref, C = layer_case(name, prefix, level, 'f16x3')
    assert C == 256
    err = (out - ref).abs().max().item()
    parity_log.check(err, ATT_BAR, f'{name} {prefix} C=256 D={LONG[name].frames}')


def test_temporal_layer_bf16_attn_vs_oracle():
    """The D = 64 case with the attention contractions on bf16 MFMA (BF16_ATTN): the bar of the
    64-token windows, 1e-2 x max|attention increment| (ref - x)."""
    x, out, ref, _ = layer_case('u22_64', 'init_temporal_attn', 0, 'bf16_attn')
    err = (out - ref).abs().max().item()
    inc = (ref - x).abs().max().item()
    parity_log.check(err, 1e-2 * inc, f'bf16, max|increment| {inc:.3e}')
    assert err > 1e-7  # a different arithmetic from the fp32-faithful mode


@pytest.mark.parametrize('name', ['u12_33', 'ada_50'])
def test_temporal_layer_fp32_vs_oracle(name):
    x, out, ref, _ = layer_case(name, 'init_temporal_attn', 0, 'fp32')
    err = (out - ref).abs().max().item()
    parity_log.check(err, ATT_BAR, f'{name} fp32 D={LONG[name].frames}')


def gpu_eps(h, x, t, cond, fea):
    out = torch.empty(x.shape, device=DEV)
    h.unet_forward(x.to(DEV), t.to(DEV), cond.to(DEV), fea.to(DEV), out)
    torch.cuda.synchronize()
    return out.cpu()


_ORACLE_EPS = {}


def oracle_eps(name, B, seed):
    """The oracle forward of a config's seeded inputs, computed once per (config, B, seed)."""
    from oracle import extdm_oracle as O
    key = (name, B, seed)
    if key not in _ORACLE_EPS:
        cfg = LONG[name]
        x, t, cond, fea = unet_inputs(cfg, B=B, seed=seed)
        with torch.no_grad():
            _ORACLE_EPS[key] = O.unet_forward(sd_of(name), cfg.as_dict(), x, t, cond, fea)
    return _ORACLE_EPS[key]


@pytest.mark.parametrize('name', ['ada_50', 'woref_39', 'u12_40_dim16'])
def test_unet_forward_long_vs_oracle(name):
    """ada 10 -> 40 at dim 64; wo_ref 10 -> 30 (39 model frames, C up to 512); u12 2 -> 38 at dim
    16, the 'small' geometry whose attention layers all run unfused."""
    cfg = LONG[name]
    x, t, cond, fea = unet_inputs(cfg, B=2, seed=99)
    eps = gpu_eps(handle(name), x, t, cond, fea)
    err = (eps - oracle_eps(name, 2, 99)).abs().max().item()
    parity_log.check(err, 1e-4, f'{name} eps, {cfg.frames} frames')


def test_batch_independence_bitwise_long():
    """ada 10 -> 40: clip 0 of a B = 3 forward has the bits of its B = 1 forward."""
    cfg = LONG['ada_50']
    x, t, cond, fea = unet_inputs(cfg, B=3, seed=3)
    t = torch.tensor([10, 500, 990])
    h = handle('ada_50')
    full = gpu_eps(h, x, t, cond, fea)
    one = gpu_eps(h, x[:1].contiguous(), t[:1], cond[:1].contiguous(), fea[:1].contiguous())
    assert torch.equal(full[:1], one)


def test_ddim4_graph_long_vs_oracle():
    """DDIM, 4 sampling steps over the 1000-step schedule through GaussianDiffusion.ddim_sample
    (captured-graph replay) on the ada 10 -> 40 reduced config, x_T and the per-step noise injected,
    against the oracle's DDIM with the same stream. Bar: x after a step <= 1e-4
    (tests/test_gpu_sampler.py: the eps bar of the forward carried through the update)."""
    from oracle import extdm_oracle as O
    cfg = LONG['ada_50']
    sd = sd_of('ada_50')
    _, _, cond, fea = unet_inputs(cfg, B=2, seed=27)
    u = pkg.Unet3DAda(dim=cfg.dim, channels=cfg.channels, dim_mults=cfg.dim_mults, cond_num=cfg.tc, pred_num=cfg.tp,
                      framesize=cfg.latent).to(DEV)
    u.load_state_dict(sd)
    d = pkg.GaussianDiffusion(u, image_size=cfg.latent, num_frames=cfg.tc + cfg.tp, timesteps=1000,
                              sampling_timesteps=4).to(DEV)
    d.use_graph = True
    shape = (2, 3, cfg.tp, cfg.latent, cfg.latent)
    gen = torch.Generator().manual_seed(29)
    xT = torch.randn(shape, generator=gen)
    noises = torch.stack([torch.randn(shape, generator=gen) for _ in range(4)])
    out = d.ddim_sample(cond.to(DEV), shape, fea.to(DEV), x_T=xT.to(DEV), noise=noises.to(DEV).contiguous())
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = O.ddim_sample(O.schedule(1000), lambda xx, tt: O.unet_forward(sd, cfg.as_dict(), xx, tt, cond, fea),
                            xT, list(noises), 4)
    err = (out.cpu() - ref).abs().max().item()
    parity_log.check(err, 1e-4, 'x after 4 DDIM steps, 50 frames')
