"""A test-side restatement of the reference's InceptionI3d (metrics/pytorch_i3d.py) and FVD front
end (metrics/calculate_fvd.py, fvd.py) in torch functional calls over a state_dict. The fixtures
come from the reference's own classes (tests/golden/make_golden_i3d.py); tests/test_i3d_cpu.py
checks that this restatement reproduces them, so the GPU tests can use it where no fixture
exists (the reference is not available where they run)."""
import math

import torch
import torch.nn.functional as F

from tests.i3d_inputs import MIXED

ENDPOINTS = ('Conv3d_1a_7x7', 'MaxPool3d_2a_3x3', 'Conv3d_2b_1x1', 'Conv3d_2c_3x3', 'MaxPool3d_3a_3x3', 'Mixed_3b',
             'Mixed_3c', 'MaxPool3d_4a_3x3', 'Mixed_4b', 'Mixed_4c', 'Mixed_4d', 'Mixed_4e', 'Mixed_4f',
             'MaxPool3d_5a_2x2', 'Mixed_5b', 'Mixed_5c')


def compute_pad(size, k, stride):
    """pytorch_i3d.py:9-13 / 71-75."""
    if size % stride == 0:
        return max(k - stride, 0)
    return max(k - size % stride, 0)


def same_pad(x, kernel, stride):
    """pytorch_i3d.py:17-33 / 80-96: zero padding, front = pad // 2."""
    pads = []
    for dim in (2, 1, 0):  # F.pad takes the last dimension first
        p = compute_pad(x.shape[2 + dim], kernel[dim], stride[dim])
        pads += [p // 2, p - p // 2]
    return F.pad(x, pads)


def maxpool_same(x, kernel, stride):
    """MaxPool3dSamePadding.forward (pytorch_i3d.py:15-34)."""
    return F.max_pool3d(same_pad(x, kernel, stride), kernel, stride, 0)


def unit3d(sd, name, x, k, stride=1, bn=True, relu=True):
    """Unit3D.forward (pytorch_i3d.py:78-103)."""
    w = sd[name + '.conv3d.weight'].to(x.dtype)
    b = sd.get(name + '.conv3d.bias')
    x = F.conv3d(same_pad(x, (k,) * 3, (stride,) * 3), w, None if b is None else b.to(x.dtype), stride)
    if bn:
        x = F.batch_norm(x, sd[name + '.bn.running_mean'].to(x.dtype), sd[name + '.bn.running_var'].to(x.dtype),
                         sd[name + '.bn.weight'].to(x.dtype), sd[name + '.bn.bias'].to(x.dtype), False, 0.001, 1e-5)
    return F.relu(x) if relu else x


def mixed(sd, name, x):
    """InceptionModule.forward (pytorch_i3d.py:127-132)."""
    b0 = unit3d(sd, name + '.b0', x, 1)
    b1 = unit3d(sd, name + '.b1b', unit3d(sd, name + '.b1a', x, 1), 3)
    b2 = unit3d(sd, name + '.b2b', unit3d(sd, name + '.b2a', x, 1), 3)
    b3 = unit3d(sd, name + '.b3b', maxpool_same(x, (3, 3, 3), (1, 1, 1)), 1)
    return torch.cat([b0, b1, b2, b3], dim=1)


def endpoints(sd, x, last='Mixed_5c'):
    """The activations after every endpoint up to `last` (pytorch_i3d.py:204-273, 305-308)."""
    out = {}
    for ep in ENDPOINTS:
        if ep == 'Conv3d_1a_7x7':
            x = unit3d(sd, ep, x, 7, 2)
        elif ep == 'Conv3d_2b_1x1':
            x = unit3d(sd, ep, x, 1)
        elif ep == 'Conv3d_2c_3x3':
            x = unit3d(sd, ep, x, 3)
        elif ep in ('MaxPool3d_2a_3x3', 'MaxPool3d_3a_3x3'):
            x = maxpool_same(x, (1, 3, 3), (1, 2, 2))
        elif ep == 'MaxPool3d_4a_3x3':
            x = maxpool_same(x, (3, 3, 3), (2, 2, 2))
        elif ep == 'MaxPool3d_5a_2x2':
            x = maxpool_same(x, (2, 2, 2), (2, 2, 2))
        else:
            assert ep in [m[0] for m in MIXED]
            x = mixed(sd, ep, x)
        out[ep] = x
        if ep == last:
            break
    return out


def extract_features(sd, x):
    """pytorch_i3d.py:318-322."""
    return F.avg_pool3d(endpoints(sd, x)['Mixed_5c'], (2, 7, 7), (1, 1, 1))


def forward(sd, x):
    """pytorch_i3d.py:305-315 in eval mode (dropout is the identity)."""
    y = unit3d(sd, 'logits', extract_features(sd, x), 1, bn=False, relu=False)
    return y.squeeze(3).squeeze(3).mean(dim=2)


def trans(x):
    """calculate_fvd.py:6-14."""
    if x.shape[-3] == 1:
        x = x.repeat(1, 1, 3, 1, 1)
    return x.permute(0, 2, 1, 3, 4)


def preprocess_single(video, resolution=224, sequence_length=None):
    """fvd.py:161-187."""
    h, w = video.shape[-2:]
    if sequence_length is not None:
        assert sequence_length <= video.shape[1]
        video = video[:, :sequence_length]
    # the shorter side to `resolution`, the longer to ceil(side * resolution / shorter)
    factor = resolution / min(h, w)
    size = (resolution, math.ceil(w * factor)) if h < w else (math.ceil(h * factor), resolution)
    big = F.interpolate(video, size=size, mode='bilinear', align_corners=False)
    y0, x0 = (size[0] - resolution) // 2, (size[1] - resolution) // 2
    crop = big[:, :, y0:y0 + resolution, x0:x0 + resolution]
    return ((crop - 0.5) * 2).contiguous()
