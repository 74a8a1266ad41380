"""Seeded LPIPS (AlexNet, version 0.1) weights and inputs shared by
tests/golden/make_golden_lpips.py and the LPIPS tests. Everything is regenerated from seeds (NumPy
PCG64), never stored.

The recipe keeps the activations at order one: conv weights N(0, 2 / fan_in), biases U(-0.2, 0.2)
except the DEAD channels of every conv, whose bias of -50 keeps them at exactly 0 after the ReLU;
lin weights U(0, 1) (non-negative, as the published ones are); the scaling layer's published
constants."""
import numpy as np
import torch

# (key, Cout, Cin, kernel, stride, padding): torchvision alexnet().features indices
CONVS = (('net.slice1.0', 64, 3, 11, 4, 2), ('net.slice2.3', 192, 64, 5, 1, 2), ('net.slice3.6', 384, 192, 3, 1, 1),
         ('net.slice4.8', 256, 384, 3, 1, 1), ('net.slice5.10', 256, 256, 3, 1, 1))
TAPS = ('relu1', 'relu2', 'relu3', 'relu4', 'relu5')
DEAD = (4, 17, 40)  # channels with a strongly negative bias in every conv
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

# tap cases: the odd one is stored whole, the 64 x 64 one every 4th channel (file size)
TAP_CASES = {'odd': ((3, 3, 37, 50), 501, 1), 'sq': ((5, 3, 64, 64), 502, 4)}
# distance cases: shape of each image set, seed, stride of the stored part of the map
DIST_CASES = {'odd': ((6, 3, 37, 50), 503, 1), 'sq': ((10, 3, 64, 64), 504, 2), 'grey': ((2, 1, 48, 64), 505, 1)}
VIDEO_SHAPE = (2, 5, 3, 40, 48)  # [videos, frames, c, h, w] of the calculate_lpips1/2/3 case
POOL_SHAPES = {'p8x11': (2, 3, 8, 11), 'p15': (1, 4, 15, 15)}


def key_shapes():
    """Ordered {state_dict key: shape} of lpips.LPIPS(net='alex') (22 entries)."""
    ks = {'scaling_layer.shift': [1, 3, 1, 1], 'scaling_layer.scale': [1, 3, 1, 1]}
    for key, co, ci, k, _, _ in CONVS:
        ks[key + '.weight'] = [co, ci, k, k]
        ks[key + '.bias'] = [co]
    for pre in ('lin%d', 'lins.%d'):
        for i, c in enumerate(CONVS):
            ks[(pre % i) + '.model.1.weight'] = [1, c[1], 1, 1]
    return ks


def make_lpips_sd(seed=500):
    g = np.random.Generator(np.random.PCG64(seed))
    sd = {'scaling_layer.shift': torch.tensor(SHIFT, dtype=torch.float32)[None, :, None, None],
          'scaling_layer.scale': torch.tensor(SCALE, dtype=torch.float32)[None, :, None, None]}
    for key, co, ci, k, _, _ in CONVS:
        w = g.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))
        b = g.uniform(-0.2, 0.2, (co,))
        b[list(DEAD)] = -50.0
        sd[key + '.weight'] = torch.from_numpy(w.astype(np.float32))
        sd[key + '.bias'] = torch.from_numpy(b.astype(np.float32))
    for i, c in enumerate(CONVS):
        sd[f'lin{i}.model.1.weight'] = torch.from_numpy(g.uniform(0, 1, (1, c[1], 1, 1)).astype(np.float32))
    for i in range(5):
        sd[f'lins.{i}.model.1.weight'] = sd[f'lin{i}.model.1.weight']
    return sd


def uniform(shape, seed, lo=-1.0, hi=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.uniform(lo, hi, shape).astype(np.float32))


def tap_input(name):
    shape, seed, _ = TAP_CASES[name]
    return uniform(shape, seed)


def dist_inputs(name):
    """Two image sets in [-1, 1]: the second is the first plus noise, clipped, so the distances
    spread over a range instead of sitting at the value of unrelated images."""
    shape, seed, _ = DIST_CASES[name]
    a = uniform(shape, seed)
    amp = torch.linspace(0.05, 0.8, shape[0])[:, None, None, None]
    b = (a + amp * uniform(shape, seed + 50)).clamp(-1, 1)
    return a, b


def videos():
    """Two [videos, frames, c, h, w] sets in [0, 1] for the reductions."""
    a = uniform(VIDEO_SHAPE, 506, 0.0, 1.0)
    b = (a + 0.3 * uniform(VIDEO_SHAPE, 507)).clamp(0, 1)
    return a, b


def pool_input(name):
    return uniform(POOL_SHAPES[name], {'p8x11': 508, 'p15': 509}[name])


def encode64(ref):
    """i3d_inputs.encode64: an fp64 array as (fp32 hi, fp16 lo * 2^20)."""
    ref = np.asarray(ref, dtype=np.float64)
    hi = ref.astype(np.float32)
    lo = ((ref - hi.astype(np.float64)) * 2.0 ** 20).astype(np.float16)
    return hi, lo


def decode64(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -20
