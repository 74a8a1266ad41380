"""Seeded InceptionI3d weights and inputs shared by tests/golden/make_golden_i3d.py and the I3D
tests. Everything is regenerated from seeds (NumPy PCG64), never stored.

The recipe keeps the activations of all 57 units at order one, so that the full forward gives
finite logits (rms ~2.6 at [1, 3, 10, 224, 224]): conv weights N(0, 2 / fan_in), BatchNorm weight
U(0.8, 1.2), bias and running_mean U(-0.2, 0.2), running_var U(0.7, 1.3), logits bias
U(-0.2, 0.2), inputs U(-1, 1)."""
import numpy as np
import torch

# InceptionModule tables (metrics/pytorch_i3d.py:229-272): name, in_channels, out_channels
MIXED = (('Mixed_3b', 192, (64, 96, 128, 16, 32, 32)), ('Mixed_3c', 256, (128, 128, 192, 32, 96, 64)),
         ('Mixed_4b', 480, (192, 96, 208, 16, 48, 64)), ('Mixed_4c', 512, (160, 112, 224, 24, 64, 64)),
         ('Mixed_4d', 512, (128, 128, 256, 24, 64, 64)), ('Mixed_4e', 512, (112, 144, 288, 32, 64, 64)),
         ('Mixed_4f', 528, (256, 160, 320, 32, 128, 128)), ('Mixed_5b', 832, (256, 160, 320, 32, 128, 128)),
         ('Mixed_5c', 832, (384, 192, 384, 48, 128, 128)))
# the endpoint taps of the parity fixture (tests/golden/i3d_taps*.npz)
TAPS = ('Conv3d_1a_7x7', 'MaxPool3d_2a_3x3', 'Conv3d_2c_3x3', 'Mixed_3b', 'MaxPool3d_4a_3x3', 'Mixed_4b',
        'MaxPool3d_5a_2x2', 'Mixed_5c')
TAP_FILES = {'Conv3d_1a_7x7': 'i3d_taps1.npz', 'MaxPool3d_2a_3x3': 'i3d_taps2.npz', 'Conv3d_2c_3x3': 'i3d_taps2.npz'}
TAP_SHAPE = (2, 3, 9, 37, 30)
FULL_SHAPES = {'t10': (1, 3, 10, 224, 224), 't17': (2, 3, 17, 224, 224)}
# MaxPool3dSamePadding kinds of the network: kernel, stride
POOLS = {'p133': ((1, 3, 3), (1, 2, 2)), 'p333s2': ((3, 3, 3), (2, 2, 2)), 'p222': ((2, 2, 2), (2, 2, 2)),
         'p333s1': ((3, 3, 3), (1, 1, 1))}
POOL_SHAPE = (1, 8, 5, 9, 10)
# preprocess cases: input shape [B, T, C, H, W], sequence_length
PRE_CASES = {'rgb': ((2, 12, 3, 64, 64), None), 'grey': ((1, 10, 1, 48, 64), None), 'rgb_seq10': ((2, 12, 3, 64, 64), 10)}
# the stored part of a preprocessed [B, 3, T, 224, 224] output (the whole is 14 MB)
PRE_SUB = (slice(None), slice(None), slice(None, None, 5), slice(None, None, 9), slice(None, None, 7))
FEAT_SHAPE = (5, 12, 3, 64, 64)


def unit_specs(num_classes=400, in_channels=3):
    """(unit name, Cout, Cin, kernel, batch norm) in the reference's state_dict order: `logits`
    is registered before the endpoints (pytorch_i3d.py:279-287)."""
    u = [('logits', num_classes, 1024, 1, False), ('Conv3d_1a_7x7', 64, in_channels, 7, True),
         ('Conv3d_2b_1x1', 64, 64, 1, True), ('Conv3d_2c_3x3', 192, 64, 3, True)]
    for name, cin, o in MIXED:
        u += [(f'{name}.b0', o[0], cin, 1, True), (f'{name}.b1a', o[1], cin, 1, True),
              (f'{name}.b1b', o[2], o[1], 3, True), (f'{name}.b2a', o[3], cin, 1, True),
              (f'{name}.b2b', o[4], o[3], 3, True), (f'{name}.b3b', o[5], cin, 1, True)]
    return u


def key_shapes(num_classes=400, in_channels=3):
    """Ordered {state_dict key: shape} of InceptionI3d (344 entries at the defaults)."""
    ks = {}
    for name, co, ci, k, bn in unit_specs(num_classes, in_channels):
        ks[f'{name}.conv3d.weight'] = [co, ci, k, k, k]
        if bn:
            for s in ('weight', 'bias', 'running_mean', 'running_var'):
                ks[f'{name}.bn.{s}'] = [co]
            ks[f'{name}.bn.num_batches_tracked'] = []
        else:
            ks[f'{name}.conv3d.bias'] = [co]
    return ks


def make_i3d_sd(seed=400, num_classes=400, in_channels=3):
    g = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape in key_shapes(num_classes, in_channels).items():
        if key.endswith('conv3d.weight'):
            v = g.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[1:]))
        elif key.endswith('bn.weight'):
            v = g.uniform(0.8, 1.2, shape)
        elif key.endswith('running_var'):
            v = g.uniform(0.7, 1.3, shape)
        elif key.endswith('num_batches_tracked'):
            sd[key] = torch.tensor(0, dtype=torch.int64)
            continue
        else:  # bn.bias, running_mean, logits bias
            v = g.uniform(-0.2, 0.2, shape)
        sd[key] = torch.from_numpy(v.astype(np.float32))
    return sd


def uniform(shape, seed, lo=-1.0, hi=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.uniform(lo, hi, shape).astype(np.float32))


def tap_input():
    return uniform(TAP_SHAPE, 401)


def full_input(name):
    return uniform(FULL_SHAPES[name], {'t10': 402, 't17': 403}[name])


def pool_input():
    return uniform(POOL_SHAPE, 404)


def pre_input(name):
    return uniform(PRE_CASES[name][0], {'rgb': 405, 'grey': 406, 'rgb_seq10': 405}[name], 0.0, 1.0)


def feat_videos(which):
    """Two sets of five videos in [0, 1]: smooth random fields, so the resize keeps structure."""
    g = np.random.Generator(np.random.PCG64(407 + which))
    b, t, c, h, w = FEAT_SHAPE
    coarse = torch.from_numpy(g.uniform(0, 1, (b, c, t, 8, 8)).astype(np.float32))
    v = torch.nn.functional.interpolate(coarse, size=(t, h, w), mode='trilinear', align_corners=True)
    return v.permute(0, 2, 1, 3, 4).contiguous()  # [B, T, C, H, W]


def encode64(ref):
    """An fp64 array as (fp32 hi, fp16 lo * 2^20): |ref - decode| <= 6e-14 + 2^-35 |ref|, at 6
    bytes a value (the taps would pass the size limit of a committed file as plain fp64)."""
    ref = np.asarray(ref, dtype=np.float64)
    hi = ref.astype(np.float32)
    lo = ((ref - hi.astype(np.float64)) * 2.0 ** 20).astype(np.float16)
    return hi, lo


def decode64(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -20
