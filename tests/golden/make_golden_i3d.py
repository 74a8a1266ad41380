"""Generate the InceptionI3d / FVD fixtures by running the REFERENCE itself on the CPU (generation
time only, like make_golden.py): metrics/pytorch_i3d.py's InceptionI3d with the seeded weights of
tests/i3d_inputs.py, and the front end of metrics/calculate_fvd.py / fvd.py.

Every stored network output is the reference run in fp64 (`*_ref`; the big taps as the hi / lo
pair of i3d_inputs.encode64), with the fp32 reference's own max-abs and rms error against it
(`*_err32` = [max_abs, rms]): the tests' bars are multiples of that error.

  i3d_keys.json     state_dict keys and shapes of InceptionI3d() at the defaults
  i3d_taps{1,2,3}.npz   (a) endpoint taps of x [2, 3, 9, 37, 30]
  i3d.npz           (b) logits / extract_features at [1, 3, 10, 224, 224] and [2, 3, 17, 224, 224]
                    (c) the four MaxPool3dSamePadding kinds on a signed [1, 8, 5, 9, 10]
                    (d) trans + preprocess_single (a strided part of each output)
                    (e) get_fvd_feats of two sets of five videos, bs = 3, and calculate_fvd2

Usage (build container only):  python tests/golden/make_golden_i3d.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402
from tests import i3d_inputs as I  # noqa: E402

sys.path.insert(0, REF)
from metrics import pytorch_i3d as R  # noqa: E402
from metrics import fvd as RF  # noqa: E402
from metrics import calculate_fvd as RC  # noqa: E402


def err32(a32, ref64):
    d = a32.double() - ref64
    return np.array([d.abs().max().item(), d.pow(2).mean().sqrt().item()])


def run_taps(net, x):
    """The reference forward loop (pytorch_i3d.py:305-308), keeping every endpoint's output."""
    out = {}
    for ep in net.VALID_ENDPOINTS:
        if ep in net.end_points:
            x = net._modules[ep](x)
            out[ep] = x
    return out


def main():
    torch.manual_seed(0)
    net = R.InceptionI3d(400, in_channels=3).eval()
    json.dump({k: list(v.shape) for k, v in net.state_dict().items()}, open(os.path.join(HERE, 'i3d_keys.json'), 'w'),
              indent=0)
    sd = I.make_i3d_sd()
    net.load_state_dict(sd)
    net64 = R.InceptionI3d(400, in_channels=3).eval()
    net64.load_state_dict(sd)
    net64 = net64.double()
    out = {}
    with torch.no_grad():
        # (a)
        x = I.tap_input()
        t32, t64 = run_taps(net, x), run_taps(net64, x.double())
        files = {}
        for ep in I.TAPS:
            hi, lo = I.encode64(t64[ep].numpy())
            d = files.setdefault(I.TAP_FILES.get(ep, 'i3d_taps3.npz'), {})
            d[ep + '_hi'], d[ep + '_lo'], d[ep + '_err32'] = hi, lo, err32(t32[ep], t64[ep])
            print(ep, tuple(t64[ep].shape), d[ep + '_err32'])
        for f, d in files.items():
            np.savez_compressed(os.path.join(HERE, f), **d)
        # (b)
        for name in I.FULL_SHAPES:
            x = I.full_input(name)
            l64, p64 = net64(x.double()), net64.extract_features(x.double())
            out[name + '_logits_ref'], out[name + '_logits_err32'] = l64.numpy(), err32(net(x), l64)
            out[name + '_pooled_ref'], out[name + '_pooled_err32'] = p64.numpy(), err32(net.extract_features(x), p64)
            print(name, 'logits rms', l64.pow(2).mean().sqrt().item(), 'max', l64.abs().max().item(),
                  out[name + '_logits_err32'], out[name + '_pooled_err32'])
        # (c)
        x = I.pool_input()
        for name, (k, s) in I.POOLS.items():
            out['pool_' + name] = R.MaxPool3dSamePadding(kernel_size=list(k), stride=s, padding=0)(x).numpy()
        # (d)
        for name, (shape, seq) in I.PRE_CASES.items():
            v = RC.trans(I.pre_input(name))
            y = torch.stack([RF.preprocess_single(u, sequence_length=seq) for u in v])
            y64 = torch.stack([RF.preprocess_single(u.double(), sequence_length=seq) for u in v])
            out['pre_' + name + '_shape'] = np.array(y.shape)
            out['pre_' + name + '_ref'] = y64[I.PRE_SUB].numpy()
            out['pre_' + name + '_err32'] = err32(y, y64)
            print('pre', name, tuple(y.shape), out['pre_' + name + '_err32'])
        # (e) the detector is called with the TorchScript detector's keywords (fvd.py:45-49)
        feats = []
        for which in (0, 1):
            v = RC.trans(I.feat_videos(which))
            f32 = RF.get_fvd_feats(v, lambda x, **kw: net(x), torch.device('cpu'), bs=3)
            f64 = RF.get_fvd_feats(v.double(), lambda x, **kw: net64(x), torch.device('cpu'), bs=3)
            out[f'feats{which}_ref'] = f64
            out[f'feats{which}_err32'] = err32(torch.from_numpy(f32), torch.from_numpy(f64))
            feats.append((f32, f64))
            print('feats', which, f64.shape, out[f'feats{which}_err32'])
        out['fvd_ref'] = np.array(RC.calculate_fvd2(feats[0][1], feats[1][1]))
        out['fvd_ref32'] = np.array(RC.calculate_fvd2(feats[0][0], feats[1][0]))
        print('fvd', out['fvd_ref'], out['fvd_ref32'])
    np.savez_compressed(os.path.join(HERE, 'i3d.npz'), **out)
    for f in sorted(os.listdir(HERE)):
        if f.startswith('i3d'):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == '__main__':
    main()
