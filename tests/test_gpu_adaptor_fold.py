"""The MotionAdaptor's normalisation passes folded into its convs (runtime.cpp adaptor / ln_conv,
conv_x3.hip AFF) against the passes they replace: the `small` u12 forward (dim 16; adaptors at C = 64
on 4 x 4 maps -- one 256-pixel tile spans planes of all three samples, so a wrong per-lane sample
index shows -- and on 2 x 2 maps, which stay on the separate passes) at B = 3, with both folds on
(default), with EXTDM_NO_ADAPTOR_FOLD=1, with EXTDM_NO_LN_FOLD=1 and with both (read per handle, so
four handles in one process), against the fp64 evaluation of the oracle. The `ada_small` forward runs
the same comparison on the second denoiser (its LayerNorm folds; its C = 256 extrapolators on 4 x 4
maps run on the 8-wave 3x3 tile, which has no affine form, and keep the separate passes), and one
case shifts x by 50 so that the adaptor sees a mean far above its std (the affine is (x - m) * r,
never x * r - m * r).

The bars: the folded route's max and rms error within 2x the fp32 CPU oracle's own error against fp64
(the contract of test_f16x3_error_vs_fp64_matches_fp32), and within 2x the unfolded route's error on
the same input."""
import os

import pytest
import torch

from tests import parity_log
from tests.golden_inputs import CONFIGS, make_sd, unet_inputs
from tests.test_gpu_parity import gpu_eps, pkg
from tests.test_gpu_precision import _fp64_eps

pytestmark = pytest.mark.gpu

SWITCHES = ('EXTDM_NO_ADAPTOR_FOLD', 'EXTDM_NO_LN_FOLD')
_REF = {}


def _handle(cfg, B, off=()):
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k in off:
        os.environ[k] = '1'
    try:
        h = pkg._lib.Handle(cfg, 1000, B, 0)
        sd = make_sd(cfg)
        sd.update(pkg.schedule_buffers(1000))
        h.load_state(sd)
        h.finalize()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
    return h


def _inputs(name, shift):
    x, t, cond, fea = unet_inputs(CONFIGS[name], B=3, seed=47)
    return x + shift, t, cond, fea


def _refs(name, shift):
    """fp64 and fp32 CPU evaluations of the oracle, once per input"""
    if (name, shift) not in _REF:
        from oracle import extdm_oracle as O
        cfg = CONFIGS[name]
        x, t, cond, fea = _inputs(name, shift)
        ref = _fp64_eps(cfg, x, t, cond, fea)
        with torch.no_grad():
            cpu32 = O.unet_forward(make_sd(cfg), cfg.as_dict(), x, t, cond, fea)
        _REF[(name, shift)] = (ref, cpu32)
    return _REF[(name, shift)]


def _stats(e, ref):
    d = e.double() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _run(h, inp):
    h.range_flag(reset=True)
    out = gpu_eps(h, *inp)
    assert h.range_flag() == 0
    assert torch.isfinite(out).all()
    return out


def _aff(h, layer, B=3):
    """the input-affine mode (last template argument) of the conv bench layer `layer` launches; 0: none"""
    h.bench_layer(B, layer, 1)
    k = h.bench_layer_kernel(layer)
    if 'conv_x3_kernel' not in k or k.count(',') < 17:
        return 0, k
    return int(k.rstrip('>').split(',')[-1]), k


def _error_bars(tag, new, old, ref, cpu32):
    (m_cpu, r_cpu), (m_new, r_new), (m_old, r_old) = _stats(cpu32, ref), _stats(new, ref), _stats(old, ref)
    print(f'{tag} vs fp64: cpu-fp32 max {m_cpu:.3e} rms {r_cpu:.3e} | folded max {m_new:.3e} rms {r_new:.3e} | '
          f'separate passes max {m_old:.3e} rms {r_old:.3e}')
    parity_log.check(m_new, 2.0 * m_cpu, tag + ' folded max vs 2x cpu-fp32')
    parity_log.check(r_new, 2.0 * r_cpu, tag + ' folded rms vs 2x cpu-fp32')
    parity_log.check(m_new, 2.0 * m_old, tag + ' folded max vs 2x separate passes')
    parity_log.check(r_new, 2.0 * r_old, tag + ' folded rms vs 2x separate passes')


def test_folds_and_their_switches_on_small_u12():
    cfg = CONFIGS['small']
    inp = _inputs('small', 0.0)
    ref, cpu32 = _refs('small', 0.0)
    h = _handle(cfg, 3)
    new = _run(h, inp)
    assert torch.equal(new, _run(h, inp))  # two runs, identical bits
    # the first adaptor's last extrapolator and its fuser took the affine templates
    assert _aff(h, 20)[0] == 1, _aff(h, 20)
    assert _aff(h, 21)[0] == 2, _aff(h, 21)
    # clip 0 does not depend on its batch
    one = _run(_handle(cfg, 1), [v[:1] for v in inp])
    assert torch.equal(new[:1], one)

    outs = {}
    for off, want in ((SWITCHES[:1], (0, 2)), (SWITCHES[1:], (1, 0)), (SWITCHES, (0, 0))):
        ho = _handle(cfg, 3, off)
        outs[off] = _run(ho, inp)
        assert (_aff(ho, 20)[0], _aff(ho, 21)[0]) == want, (off, _aff(ho, 20), _aff(ho, 21))
    old = outs[SWITCHES]
    # every switch selects another route, and the two folds are independent of each other
    for off in outs:
        assert not torch.equal(new, outs[off]), off
    assert not torch.equal(outs[SWITCHES[:1]], old) and not torch.equal(outs[SWITCHES[1:]], old)

    _error_bars('small', new, old, ref, cpu32)
    for off in (SWITCHES[:1], SWITCHES[1:]):  # each fold on its own
        _error_bars('small, %s off' % off[0][9:].lower(), outs[off], old, ref, cpu32)


def test_folds_on_small_ada():
    cfg = CONFIGS['ada_small']
    inp = _inputs('ada_small', 0.0)
    ref, cpu32 = _refs('ada_small', 0.0)
    h = _handle(cfg, 3)
    new = _run(h, inp)
    # the two-source fuser and the predictor fold; this denoiser's first adaptor has C = 256 on 4 x 4
    # maps, whose extrapolator convs run on the 8-wave tile and stay on the separate passes
    assert _aff(h, 21)[0] == 2, _aff(h, 21)
    one = _run(_handle(cfg, 1), [v[:1] for v in inp])
    assert torch.equal(new[:1], one)
    old = _run(_handle(cfg, 3, SWITCHES), inp)
    assert not torch.equal(new, old)
    _error_bars('ada_small', new, old, ref, cpu32)


def test_adaptor_mean_far_above_std():
    cfg = CONFIGS['small']
    inp = _inputs('small', 50.0)
    ref, cpu32 = _refs('small', 50.0)
    new = _run(_handle(cfg, 3), inp)
    old = _run(_handle(cfg, 3, SWITCHES), inp)
    assert not torch.equal(new, old)
    _error_bars('small, x + 50', new, old, ref, cpu32)


def test_fold_bench_layers_take_the_affine_templates_on_bair():
    h = _handle(CONFIGS['bair'], 2)
    for layer, mode in ((20, 1), (21, 2)):
        ms, flop = h.bench_layer(2, layer, 1)
        assert _aff(h, layer, 2)[0] == mode and ms > 0 and flop > 0, (layer, _aff(h, layer, 2), ms, flop)
