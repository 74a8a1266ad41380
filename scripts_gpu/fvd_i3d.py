"""FVD feature extraction at the eval driver's shape (valid.py:203-204: 16 videos per mini-batch,
30 frames, 64 x 64 sources -> [16, 3, 30, 224, 224]): device-event time per video of the native
InceptionI3d against the same network in eager PyTorch-ROCm (the tests/i3d_torch.py restatement),
alternating in one process. Writes profiles/fvd_i3d.json (or --out).

  python scripts_gpu/fvd_i3d.py [--repeats 9] [--out profiles/fvd_i3d.json]
  rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python scripts_gpu/fvd_i3d.py --trace-run
  python scripts_gpu/fvd_i3d.py --trace-csv DIR/run_kernel_trace.csv --out profiles/fvd_i3d.json
      (adds the per-kernel shares of one native forward and the algorithmic FLOP/s of the three
      largest 3-D conv launches against the 838.9 TF/s f16x3 peak to the JSON)
"""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = '140-extdm-distribution-extrapolation-diffusion-model-for-video-prediction_amd'
B, T, SRC = 16, 30, 64
F16X3_PEAK = 838.9e12
TRACE_FORWARDS = 3


def conv_layers(n=B, t=T, size=224):
    """(name, kernel, FLOPs) of every Unit3D launch of one forward, in launch order."""
    from tests.i3d_inputs import MIXED
    up = lambda v, s: -(-v // s)  # noqa: E731
    d = [t, size, size]
    out = []

    def conv(name, cout, cin, k, s=1):
        o = [up(v, s) for v in d]
        out.append((name, k, 2.0 * n * cout * cin * k ** 3 * o[0] * o[1] * o[2]))
        return o
    d = conv('Conv3d_1a_7x7', 64, 3, 7, 2)
    d = [d[0], up(d[1], 2), up(d[2], 2)]
    d = conv('Conv3d_2b_1x1', 64, 64, 1)
    d = conv('Conv3d_2c_3x3', 192, 64, 3)
    d = [d[0], up(d[1], 2), up(d[2], 2)]
    for name, cin, o in MIXED:
        if name == 'Mixed_4b':
            d = [up(v, 2) for v in d]
        if name == 'Mixed_5b':
            d = [up(v, 2) for v in d]
        for br, co, ci, k in (('b0', o[0], cin, 1), ('b1a', o[1], cin, 1), ('b1b', o[2], o[1], 3),
                              ('b2a', o[3], cin, 1), ('b2b', o[4], o[3], 3), ('b3b', o[5], cin, 1)):
            conv(f'{name}.{br}', co, ci, k)
    return out


def setup():
    import torch
    pkg = importlib.import_module(PKG)
    from tests import i3d_inputs as I
    dev = torch.device('cuda:0')
    sd = I.make_i3d_sd()
    net = pkg.metrics.InceptionI3d()
    net.load_state_dict(sd)
    net = net.to(dev)
    videos = I.uniform((B, T, 3, SRC, SRC), 420, 0.0, 1.0).to(dev)
    return torch, pkg, dev, sd, net, videos


def timing(args):
    torch, pkg, dev, sd, net, videos = setup()
    from tests import i3d_torch as R
    M = pkg.metrics
    dsd = {k: v.to(dev) for k, v in sd.items()}

    def native():
        return M.get_feats(videos, dev, mini_bs=B, i3d=net)

    def native_fwd(x):
        return net(x)

    def eager():
        v = R.trans(videos)
        with torch.no_grad():
            x = torch.stack([R.preprocess_single(u) for u in v])
            return R.forward(dsd, x).cpu().numpy()

    def eager_fwd(x):
        with torch.no_grad():
            return R.forward(dsd, x)

    def timed(f, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f(*a)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    x = pkg._lib.fvd_preprocess(videos)
    for _ in range(2):  # warm-up: handle build, MIOpen's solver search
        fn, fe = native(), eager()
        native_fwd(x), eager_fwd(x)
    torch.cuda.synchronize()
    res = {k: [] for k in ('native', 'eager', 'native_forward', 'eager_forward')}
    for _ in range(args.repeats):
        res['native'].append(timed(native)[0])
        res['eager'].append(timed(eager)[0])
        res['native_forward'].append(timed(native_fwd, x)[0])
        res['eager_forward'].append(timed(eager_fwd, x)[0])
    import numpy as np
    out = {'shape': [B, 3, T, 224, 224], 'source': [B, T, 3, SRC, SRC], 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0),
           'max_abs_native_vs_eager_logits': float(np.abs(fn - fe).max())}
    for k, v in res.items():
        out[k + '_ms_per_video'] = {'median': statistics.median(v) / B, 'min': min(v) / B, 'max': max(v) / B}
    out['speedup_get_feats'] = statistics.median(res['eager']) / statistics.median(res['native'])
    out['speedup_forward'] = statistics.median(res['eager_forward']) / statistics.median(res['native_forward'])
    flops = sum(f for _, _, f in conv_layers())
    out['conv_gflop_per_video'] = flops / B / 1e9
    out['native_forward_conv_tflops'] = flops / (statistics.median(res['native_forward']) * 1e-3) / 1e12
    merge(args.out, out)
    print(json.dumps(out))


def trace_run():
    torch, pkg, dev, sd, net, videos = setup()
    x = pkg._lib.fvd_preprocess(videos)
    for _ in range(TRACE_FORWARDS):
        net(x)
    torch.cuda.synchronize()


def trace_csv(args):
    rows = sorted(csv.DictReader(open(args.trace_csv)), key=lambda r: int(r['Start_Timestamp']))
    rows = [r for r in rows if any(s in r['Kernel_Name'] for s in ('conv3d_x3', 'maxpool3d_same', 'i3d_avgpool',
                                                                    'i3d_logits'))]
    n = len(rows) // TRACE_FORWARDS
    rows = rows[-n:]  # the last forward
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3  # noqa: E731
    total = sum(dur(r) for r in rows)
    share = {}
    for r in rows:
        k = r['Kernel_Name'].replace('void ', '').replace('extdm::(anonymous namespace)::', '').split('(')[0]
        share[k] = share.get(k, 0.0) + dur(r)
    convs = [r for r in rows if 'conv3d_x3' in r['Kernel_Name']]
    layers = conv_layers()
    assert len(convs) == len(layers), (len(convs), len(layers))
    per = [{'layer': name, 'us': dur(r), 'gflop': f / 1e9, 'tflops': f / dur(r) / 1e6,
            'of_f16x3_peak': f / (dur(r) * 1e-6) / F16X3_PEAK} for (name, _, f), r in zip(layers, convs)]
    out = {'trace_forward_us': total,
           'kernel_share': {k: {'us': v, 'share': v / total} for k, v in sorted(share.items(), key=lambda kv: -kv[1])},
           'largest_conv_launches': sorted(per, key=lambda p: -p['gflop'])[:3],
           'slowest_conv_launches': sorted(per, key=lambda p: -p['us'])[:5]}
    merge(args.out, out)
    print(json.dumps(out))


def merge(path, new):
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(new)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, 'w'), indent=1)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'fvd_i3d.json'))
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--trace-csv')
    a = ap.parse_args()
    if a.trace_run:
        trace_run()
    elif a.trace_csv:
        trace_csv(a)
    else:
        timing(a)
