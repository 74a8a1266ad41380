"""Clips of 33..64 model frames (cond + pred; wo_ref: cond - 1 + pred), the CPU side:
the Python frame-count limit, the state_dict layout, and the oracle pinned to the reference
beyond 32 frames (tests/golden/long_forward.npz, written by tests/golden/make_golden_long.py
from the reference itself)."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import extdm_oracle as O
from tests.golden_inputs import PKG, make_sd, unet_inputs

pkg = importlib.import_module(PKG)
spec = importlib.import_module(PKG + '.spec')
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
# the fixture's config (make_golden_long.py LONG_CFG): u12, dim 16, 2 -> 38 = 40 model frames
LONG_CFG = spec.UnetConfig(dim=16, tc=2, tp=38, latent=16, fea_size=8)


@pytest.mark.parametrize('cls,tc,tp', [('Unet3D', 2, 63), ('Unet3DAda', 10, 55), ('Unet3DWoRef', 10, 56)])
def test_more_than_64_frames_is_a_value_error(cls, tc, tp):
    """65 model frames: the constructor names the 64-frame limit (the library's finalize would
    refuse the handle only at the first forward)."""
    with pytest.raises(ValueError, match='64'):
        getattr(pkg, cls)(dim=16, cond_num=tc, pred_num=tp, framesize=16)


@pytest.mark.parametrize('cls,tc,tp,frames', [('Unet3D', 4, 60, 64), ('Unet3DAda', 10, 40, 50),
                                              ('Unet3DWoRef', 10, 55, 64)])
def test_long_clips_construct_with_the_spec_layout(cls, tc, tp, frames):
    u = getattr(pkg, cls)(dim=16, cond_num=tc, pred_num=tp, framesize=16)
    assert u.ucfg.frames == frames
    want = [(n, tuple(s)) for n, s, _ in spec.unet_spec(u.ucfg)]
    got = [(k, tuple(v.shape)) for k, v in u.state_dict().items()]
    assert got == want


def test_fixture_holds_the_far_t5_buckets():
    """|i - j| >= 32 is the point of the fixture: those entries are present, and they carry the
    clamped bucket nb - 1 = 15 (+ 16 for the other sign) of the seeded embedding."""
    g = np.load(os.path.join(GOLD, 'long_forward.npz'))
    tb = g['time_bias50']
    assert tb.shape == (8, 50, 50)
    i, j = np.nonzero(np.abs(np.arange(50)[:, None] - np.arange(50)[None, :]) >= 32)
    assert len(i) == 2 * (18 * 19 // 2)
    emb = make_sd(LONG_CFG)['time_rel_pos_bias.relative_attention_bias.weight'].numpy()  # [32][heads]
    np.testing.assert_array_equal(tb[:, 49, 0], emb[15])  # n = i - j = 49: bucket 15
    np.testing.assert_array_equal(tb[:, 0, 49], emb[31])  # n < 0: 16 + 15
    assert g['eps'].shape == (1, 3, 38, 16, 16)


def test_oracle_time_pos_bias_beyond_32_frames():
    g = np.load(os.path.join(GOLD, 'long_forward.npz'))
    bias = O.time_pos_bias(make_sd(LONG_CFG), 50)
    np.testing.assert_array_equal(bias.numpy(), g['time_bias50'])


def test_oracle_forward_40_frames_vs_reference():
    """The tolerance test_oracle_golden.py uses for `small`. The reference ran B = 2 (its STW
    trips a view at B = 1 where the window collapses); the fixture keeps clip 0."""
    g = np.load(os.path.join(GOLD, 'long_forward.npz'))
    x, t, cond, fea = unet_inputs(LONG_CFG, B=2)
    with torch.no_grad():
        eps = O.unet_forward(make_sd(LONG_CFG), LONG_CFG.as_dict(), x, t, cond, fea)
    np.testing.assert_allclose(eps[:1].numpy(), g['eps'], atol=2e-5, rtol=1e-5)
