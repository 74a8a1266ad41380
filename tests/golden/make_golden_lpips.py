"""Generate the LPIPS fixture tests/golden/lpips.npz on the CPU (generation time only, like
make_golden_i3d.py). The `lpips` package is not available, so tests/golden/shims/lpips puts the
plain-torch restatement (tests/lpips_torch.py) with the seeded weights of tests/lpips_inputs.py
behind `import lpips`; the REFERENCE's own metrics/calculate_lpips.py is then imported and run: its
`trans`, its one-pair-per-forward loops and the reductions of calculate_lpips1/2/3 are what the
fixture pins, and the TypeError of calculate_lpips (line 66) is recorded.

Every stored network output is the fp64 run (`*_ref`, or the hi / lo pair of lpips_inputs.encode64),
with the fp32 run's own max-abs and rms error against it (`*_err32` = [max_abs, rms]): the tests'
bars are multiples of that error.

  tap_<case>_<relu>      relu1 .. relu5 of x [3, 3, 37, 50] (whole) and [5, 3, 64, 64] (every 4th channel)
  dist_<case>_*          per-pair mean of the spatial map, the map (part of it for 'sq'), and the
                         spatial=False value, at [6, 37x50], [10, 64x64], [2, 48x64 grey]
  frames_*, red{1,2,3}_* per-frame values and calculate_lpips1/2/3 of [2 videos, 5 frames]
  pool_*                 MaxPool2d(3, 2) on signed data

Usage (build container only):  python tests/golden/make_golden_lpips.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402
from tests import lpips_inputs as I  # noqa: E402
from tests import lpips_torch as T  # noqa: E402

sys.path.insert(0, os.path.join(HERE, 'shims'))
sys.path.insert(0, REF)
from metrics import calculate_lpips as RC  # noqa: E402


def err32(a32, ref64):
    d = a32.double() - ref64
    return np.array([d.abs().max().item(), d.pow(2).mean().sqrt().item()])


def per_frame(v1, v2):
    """The loop of calculate_lpips.py:83-93 with the module's current loss_fn, keeping every value."""
    v1, v2 = RC.trans(v1), RC.trans(v2)
    return np.array([[RC.loss_fn.forward(a[None], b[None]).mean().item() for a, b in zip(x, y)]
                     for x, y in zip(v1, v2)])


def main():
    sd = I.make_lpips_sd()
    sd64 = T.cast(sd, torch.float64)
    out = {}
    with torch.no_grad():
        for case, (shape, _, cs) in I.TAP_CASES.items():
            x = I.tap_input(case)
            t32, t64 = T.taps(sd, x), T.taps(sd64, x.double())
            for name, a, b in zip(I.TAPS, t32, t64):
                key = f'tap_{case}_{name}'
                out[key + '_hi'], out[key + '_lo'] = I.encode64(b[:, ::cs].numpy())
                out[key + '_err32'] = err32(a[:, ::cs], b[:, ::cs])  # of the stored part
                print(key, tuple(b.shape), 'rms', b.pow(2).mean().sqrt().item(), out[key + '_err32'])
        for case, (shape, _, ms) in I.DIST_CASES.items():
            a, b = I.dist_inputs(case)
            m32 = T.forward(sd, a, b, spatial=True)[:, 0]
            m64 = T.forward(sd64, a.double(), b.double(), spatial=True)[:, 0]
            key = f'dist_{case}'
            out[key + '_map_hi'], out[key + '_map_lo'] = I.encode64(m64[:, ::ms, ::ms].numpy())
            out[key + '_map_err32'] = err32(m32[:, ::ms, ::ms], m64[:, ::ms, ::ms])  # of the stored part
            out[key + '_mean_ref'] = m64.mean([1, 2]).numpy()
            out[key + '_mean_err32'] = err32(m32.mean([1, 2]), m64.mean([1, 2]))
            p32 = T.forward(sd, a, b, spatial=False).flatten()
            p64 = T.forward(sd64, a.double(), b.double(), spatial=False).flatten()
            out[key + '_plain_ref'], out[key + '_plain_err32'] = p64.numpy(), err32(p32, p64)
            print(key, out[key + '_mean_ref'], out[key + '_mean_err32'], out[key + '_map_err32'])
        # the reference's own reductions, fp32 as it runs them and with an fp64 loss_fn
        v1, v2 = I.videos()
        loss32 = RC.loss_fn
        assert loss32.spatial is True  # calculate_lpips.py:9-12
        f32 = per_frame(v1, v2)
        r32 = (RC.calculate_lpips1(v1, v2, 'cpu'), RC.calculate_lpips2(v1, v2, 'cpu'), RC.calculate_lpips3(v1, v2, 'cpu'))
        try:
            RC.calculate_lpips(v1, v2, 'cpu')
            raise SystemExit('calculate_lpips did not raise')
        except TypeError as e:
            out['calc_typeerror'] = np.array(str(e))
            print('calculate_lpips TypeError:', e)
        RC.loss_fn = T.Net(sd, spatial=True).double().eval()
        f64 = per_frame(v1.double(), v2.double())
        r64 = (RC.calculate_lpips1(v1.double(), v2.double(), 'cpu'), RC.calculate_lpips2(v1.double(), v2.double(), 'cpu'),
               RC.calculate_lpips3(v1.double(), v2.double(), 'cpu'))
        RC.loss_fn = loss32
        out['frames_ref'], out['frames_err32'] = f64, err32(torch.from_numpy(f32), torch.from_numpy(f64))
        out['red1_ref'], out['red1_ref32'] = np.array(r64[0]), np.array(r32[0])
        out['red2_ref'], out['red2_ref32'] = np.array(r64[1]), np.array(r32[1])
        out['red3_ref'], out['red3_ref32'] = np.array(r64[2]), np.array(r32[2])
        print('frames', f64, out['frames_err32'], 'red1', r64[0], 'red2', r64[1], 'red3', r64[2])
        for name in I.POOL_SHAPES:
            out['pool_' + name] = F.max_pool2d(I.pool_input(name), kernel_size=3, stride=2).numpy()
    path = os.path.join(HERE, 'lpips.npz')
    np.savez_compressed(path, **out)
    print('lpips.npz', os.path.getsize(path))


if __name__ == '__main__':
    main()
