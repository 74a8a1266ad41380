"""InceptionI3d on the device (csrc/i3d.hip through extdm_fvd_*) against the reference's fp64
fixtures (tests/golden/make_golden_i3d.py): endpoint taps, the full forward, the max pools, the
preprocess front end, get_fvd_feats and the FVD value, batch invariance, the refusals, and
eval_metrics(i3d=...). Every figure is printed before it is asserted."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import i3d_inputs as I
from tests.golden_inputs import PKG

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
pkg = importlib.import_module(PKG)
M = pkg.metrics
DEV = torch.device('cuda:0')

# Bars at 3x the error measured on an MI355X (the convention of DESIGN §7), each beside its
# measured value; the fp32 reference's own error against fp64 (the fixture's *_err32) is printed
# with every figure, and a measured error above 10x that one is a bug, not a bar.
#   logits (rms 4.5 / 5.9, max 16 / 21): fp32 reference 4.4e-6 / 6.5e-6; pooled: 5.6e-6 / 9.8e-6
LOGITS_MEASURED = {'t10': 9.16e-6, 't17': 1.19e-5}  # max-abs vs fp64
POOLED_MEASURED = {'t10': 1.36e-5, 't17': 2.23e-5}
PRE_MEASURED = 7.97e-6       # max-abs vs the fp64 reference, values in [-1, 1] (fp32 reference 1.0e-5)
FEATS_MEASURED = 4.44e-6     # max-abs vs fp64, get_fvd_feats on 12-frame clips (fp32 reference 3.6e-6)
FVD_REL_MEASURED = 9.65e-8   # |fvd - ref| / ref of frechet_distance on five-video sets (fp32 reference 4.8e-7)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'i3d.npz'))


@pytest.fixture(scope='module')
def sd():
    return I.make_i3d_sd()


@pytest.fixture(scope='module')
def net(sd):
    n = M.InceptionI3d()
    n.load_state_dict(sd)
    n = n.to(DEV)
    n._h(DEV, 3, 17)  # one handle for every shape below
    return n


@pytest.fixture(scope='module')
def full(net):
    """The forward of the two full-size cases, computed once: name -> (x, logits, pooled)."""
    out = {}
    for name in I.FULL_SHAPES:
        x = I.full_input(name).to(DEV)
        out[name] = (x, net(x), net.extract_features(x))
    return out


def test_endpoint_taps(net):
    """(a): rms error per tap at most 2x the fp32 reference's own rms error against fp64 -- the
    bar test_f16x3_error_vs_fp64_across_activation_scales sets for this arithmetic."""
    x = I.tap_input().to(DEV)
    bad = []
    for ep in I.TAPS:
        g = np.load(os.path.join(GOLD, I.TAP_FILES.get(ep, 'i3d_taps3.npz')))
        ref = I.decode64(g[ep + '_hi'], g[ep + '_lo'])
        got = net.endpoint(x, ep)
        assert tuple(got.shape) == ref.shape and ref.size > 1000
        assert torch.isfinite(got).all(), ep
        d = got.double().cpu().numpy() - ref
        rms, ref_rms = float(np.sqrt(np.mean(d * d))), float(g[ep + '_err32'][1])
        print(f'{ep}: rms {rms:.3e} max {np.abs(d).max():.3e}; fp32 reference rms {ref_rms:.3e} '
              f'max {g[ep + "_err32"][0]:.3e}; ratio {rms / ref_rms:.2f}')
        if not rms <= 2 * ref_rms:
            bad.append((ep, rms, ref_rms))
    assert not bad, bad


@pytest.mark.parametrize('name', list(I.FULL_SHAPES))
def test_full_forward(full, gold, name):
    """(b): logits and extract_features against the fp64 reference."""
    x, logits, pooled = full[name]
    N = x.shape[0]
    assert logits.shape == (N, 400) and tuple(pooled.shape) == gold[name + '_pooled_ref'].shape
    el = np.abs(logits.double().cpu().numpy() - gold[name + '_logits_ref']).max()
    ep = np.abs(pooled.double().cpu().numpy() - gold[name + '_pooled_ref']).max()
    print(f'{name}: logits max-abs {el:.3e} (fp32 reference {gold[name + "_logits_err32"][0]:.3e}), '
          f'pooled max-abs {ep:.3e} (fp32 reference {gold[name + "_pooled_err32"][0]:.3e})')
    assert torch.isfinite(logits).all() and torch.isfinite(pooled).all()
    assert el <= 3 * LOGITS_MEASURED[name]
    assert ep <= 3 * POOLED_MEASURED[name]


def test_max_pools_bitwise(gold):
    """(c): a max involves no rounding; the padded zeros take part (signed input)."""
    L = pkg._lib.load()
    x = I.pool_input().to(DEV)
    assert (x < 0).any()
    B, C, T, H, W = x.shape
    for name, (k, s) in I.POOLS.items():
        ref = gold['pool_' + name]
        out = torch.empty(ref.shape, device=DEV)
        pkg._lib.check(L.extdm_fvd_maxpool(pkg._lib._ptr(x), B, C, T, H, W, *k, *s, pkg._lib._ptr(out),
                                           pkg._lib._stream()))
        assert np.array_equal(out.cpu().numpy(), ref), name


def test_preprocess(gold):
    """(d): trans + preprocess_single against the fp64 reference (the stored part of each output);
    a grey clip equals the 3-channel run of the replicated input bitwise."""
    worst = 0.0
    for name, (shape, seq) in I.PRE_CASES.items():
        v = I.pre_input(name).to(DEV)
        y = pkg._lib.fvd_preprocess(v, seq)
        assert list(y.shape) == list(gold['pre_' + name + '_shape']), name
        # the Python mirror, one video at a time, is the same launch per video
        y1 = torch.stack([M.preprocess_single(u, sequence_length=seq) for u in M.trans(v)])
        assert torch.equal(y, y1), name
        e = np.abs(y[I.PRE_SUB].double().cpu().numpy() - gold['pre_' + name + '_ref']).max()
        print(f'preprocess {name}: max-abs {e:.3e} (fp32 reference {gold["pre_" + name + "_err32"][0]:.3e})')
        assert float(y.min()) >= -1.0 and float(y.max()) <= 1.0
        worst = max(worst, e)
    assert worst <= 3 * PRE_MEASURED
    grey = I.pre_input('grey').to(DEV)
    assert torch.equal(pkg._lib.fvd_preprocess(grey), pkg._lib.fvd_preprocess(grey.repeat(1, 1, 3, 1, 1)))
    # sequence_length crops in time only
    rgb = I.pre_input('rgb').to(DEV)
    assert torch.equal(pkg._lib.fvd_preprocess(rgb, 10), pkg._lib.fvd_preprocess(rgb)[:, :, :10])


def test_fvd_feats_and_value(net, gold):
    """(e): get_fvd_feats with a ragged last mini-batch, and calculate_fvd2 of the two sets."""
    feats = []
    for which in (0, 1):
        v = M.trans(I.feat_videos(which).to(DEV))
        f = M.get_fvd_feats(v, net, DEV, bs=3)
        assert f.shape == (5, 400) and f.dtype == np.float64
        e = np.abs(f - gold[f'feats{which}_ref']).max()
        print(f'feats{which}: max-abs {e:.3e} (fp32 reference {gold[f"feats{which}_err32"][0]:.3e})')
        assert e <= 3 * FEATS_MEASURED
        feats.append(f)
    fvd, ref = M.calculate_fvd2(feats[0], feats[1]), float(gold['fvd_ref'])
    rel = abs(fvd - ref) / ref
    print(f'fvd {fvd!r} reference {ref!r} rel {rel:.3e} (fp32 reference '
          f'{abs(float(gold["fvd_ref32"]) - ref) / ref:.3e})')
    assert rel <= 3 * FVD_REL_MEASURED


def test_batch_invariance(net, full):
    """A video's features are bitwise independent of its batch, its position and the mini-batch
    size; repeats are bitwise equal."""
    x, logits, pooled = full['t17']
    a = x[:1].contiguous()
    assert torch.equal(net(a), logits[:1]) and torch.equal(net.extract_features(a), pooled[:1])
    x3 = torch.cat([I.uniform((1, 3, 17, 224, 224), 499).to(DEV), x[1:], x[:1]])
    l3, p3 = net(x3), net.extract_features(x3)
    assert torch.equal(l3[2], logits[0]) and torch.equal(l3[1], logits[1])
    assert torch.equal(p3[2], pooled[0]) and torch.equal(p3[1], pooled[1])
    assert torch.equal(net(x), logits) and torch.equal(net(x), logits)
    v = M.trans(I.feat_videos(0).to(DEV))
    f1, f3 = M.get_fvd_feats(v, net, DEV, bs=1), M.get_fvd_feats(v, net, DEV, bs=3)
    assert np.array_equal(f1, f3)
    assert np.array_equal(f3, M.get_fvd_feats(v, net, DEV, bs=3))


def test_refusals(net, sd):
    with pytest.raises(ValueError, match='at least 9 frames'):
        net(torch.zeros(1, 3, 8, 224, 224, device=DEV))
    with pytest.raises(ValueError, match='224 x 224'):
        net(torch.zeros(1, 3, 10, 231, 231, device=DEV))
    with pytest.raises(RuntimeError, match='ROCm device'):
        net(torch.zeros(1, 3, 10, 224, 224))
    # the C ABI refuses short clips itself
    h = net._h(DEV, 1, 10)
    with pytest.raises(RuntimeError, match='at least 9 frames'):
        h.features(torch.zeros(1, 3, 8, 224, 224, device=DEV), logits=torch.empty(1, 400, device=DEV))
    missing = 'Mixed_4d.b2a.bn.running_mean'
    h2 = pkg._lib.FvdHandle(400, 3, 1, 10, 0)
    h2.load_state({k: v for k, v in sd.items() if k != missing})
    with pytest.raises(RuntimeError, match=missing):
        h2.finalize()
    # an input past the fp16 range of the f16x3 split raises through the range flag
    x = I.full_input('t10').to(DEV)
    with pytest.raises(RuntimeError, match='65504'):
        net(x * 1e5)
    assert h.range_flag(reset=True) == 1 and h.range_flag() == 0
    net(x)  # and the next call is clean


def test_eval_metrics_with_detector(net):
    """eval_metrics(i3d=net) equals eval_metrics with the same features passed in."""
    b, n, t = 3, 2, 12
    g = np.random.Generator(np.random.PCG64(410))
    coarse = torch.from_numpy(g.uniform(0, 1, (b * (n + 1), 3, t, 8, 8)).astype(np.float32))
    v = torch.nn.functional.interpolate(coarse, size=(t, 64, 64), mode='trilinear', align_corners=True)
    v = v.permute(0, 2, 1, 3, 4).contiguous().to(DEV)  # [(b (n + 1)), t, c, h, w]
    origin = v[:b, None].expand(b, n, t, 3, 64, 64).contiguous()
    result = v[b:].view(b, n, t, 3, 64, 64)
    got = M.eval_metrics(origin, result, 2, i3d=net)
    of = M.get_feats(origin[:, 0], DEV, mini_bs=4, i3d=net)
    rf = M.get_feats(result.flatten(0, 1), DEV, mini_bs=4, i3d=net)
    want = M.eval_metrics(origin, result, 2, origin_feats=of, result_feats=rf)
    assert 'fvd_best' in got and set(got) == set(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
