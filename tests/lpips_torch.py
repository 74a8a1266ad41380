"""lpips.LPIPS(net='alex', version='0.1', lpips=True) restated in plain torch from the published
package (ScalingLayer, pretrained_networks.alexnet, normalize_tensor, NetLinLayer, upsample,
spatial_average, LPIPS.forward): the oracle of the LPIPS tests, run in fp64 and fp32 on the CPU.
tests/golden/shims/lpips puts it behind `import lpips` for the reference's calculate_lpips.py."""
import torch
import torch.nn as nn
import torch.nn.functional as F

# (key, stride, padding) of the five convs; MaxPool2d(3, 2) sits in front of the 2nd and the 3rd
CONVS = (('net.slice1.0', 4, 2), ('net.slice2.3', 1, 2), ('net.slice3.6', 1, 1), ('net.slice4.8', 1, 1),
         ('net.slice5.10', 1, 1))


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def feature_hw(h, w):
    """(h, w) of relu1, relu2, relu3..5 for an h x w input, by the layers' own rules."""
    def conv(n, k, s, p):
        return (n + 2 * p - k) // s + 1

    def pool(n):
        return (n - 3) // 2 + 1
    a = (conv(h, 11, 4, 2), conv(w, 11, 4, 2))
    b = (pool(a[0]), pool(a[1]))
    c = (pool(b[0]), pool(b[1]))
    return a, b, c


def taps(sd, x):
    """relu1 .. relu5 (post-ReLU, un-normalised) of x in [-1, 1]."""
    x = (x - sd['scaling_layer.shift']) / sd['scaling_layer.scale']
    out = []
    for k, (key, s, p) in enumerate(CONVS):
        if k in (1, 2):
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, sd[key + '.weight'], sd[key + '.bias'], stride=s, padding=p))
        out.append(x)
    return out


def normalize_tensor(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def lin_maps(sd, in0, in1):
    """The five [N, 1, h, w] maps lin_k((f0^ - f1^)^2)."""
    t0, t1 = taps(sd, in0), taps(sd, in1)
    return [F.conv2d((normalize_tensor(a) - normalize_tensor(b)) ** 2, sd[f'lin{k}.model.1.weight'])
            for k, (a, b) in enumerate(zip(t0, t1))]


def forward(sd, in0, in1, spatial=False, normalize=False):
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    maps = lin_maps(sd, in0, in1)
    if spatial:
        res = [F.interpolate(m, size=in0.shape[2:], mode='bilinear', align_corners=False) for m in maps]
    else:
        res = [m.mean([2, 3], keepdim=True) for m in maps]
    val = res[0]
    for r in res[1:]:
        val = val + r
    return val


class Net(nn.Module):
    """The restatement as a module with the package's forward signature; .double() / .to() move
    its weights."""

    def __init__(self, sd, spatial=False):
        super().__init__()
        self.spatial = spatial
        self._keys = [k for k in sd if not k.startswith('lins.')]
        for k in self._keys:
            self.register_buffer(k.replace('.', '__'), sd[k].clone())

    def sd(self):
        return {k: getattr(self, k.replace('.', '__')) for k in self._keys}

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        assert not retPerLayer
        return forward(self.sd(), in0, in1, self.spatial, normalize)


def trans(x):
    """calculate_lpips.py:15-23."""
    if x.shape[-3] == 1:
        x = x.repeat(1, 1, 3, 1, 1)
    return x * 2 - 1
