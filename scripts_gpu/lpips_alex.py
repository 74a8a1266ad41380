"""LPIPS at an eval run's scale (valid.py:222-228: every predicted frame of every sample; here 4096
pairs of 3 x 64 x 64): device-event time per pair of the native LPIPS against the same network in
eager PyTorch-ROCm (the tests/lpips_torch.py restatement) run batched on the same device, and
against the reference's one-pair-per-forward loop (calculate_lpips.py:102-112, timed on the first
LOOP_PAIRS pairs), alternating in one process. Writes profiles/lpips_alex.json (or --out).

  python scripts_gpu/lpips_alex.py [--repeats 9] [--out profiles/lpips_alex.json]
  rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python scripts_gpu/lpips_alex.py --trace-run
  python scripts_gpu/lpips_alex.py --trace-csv DIR/run_kernel_trace.csv --out profiles/lpips_alex.json
      (adds the per-kernel shares of one native call and the algorithmic FLOP/s of the three
      largest convs against the 838.9 TF/s f16x3 peak to the JSON)
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
N, SIZE = 4096, 64
LOOP_PAIRS = 256
F16X3_PEAK = 838.9e12
TRACE_CALLS = 3
KERNELS = ('conv2d_x3', 'maxpool2d_32', 'lpips_head', 'lpips_mean', 'lpips_map')


def conv_layers(n=2 * N, size=SIZE):
    """(name, FLOPs) of the five conv layers for n images (both sets), in launch order."""
    from tests.lpips_inputs import CONVS
    from tests.lpips_torch import feature_hw
    a, b, c = feature_hw(size, size)
    hw = [a, b, c, c, c]
    return [(key, 2.0 * n * co * ci * k * k * hw[i][0] * hw[i][1]) for i, (key, co, ci, k, _, _) in enumerate(CONVS)]


def setup():
    import torch
    pkg = importlib.import_module(PKG)
    from tests import lpips_inputs as I
    dev = torch.device('cuda:0')
    sd = I.make_lpips_sd()
    net = pkg.metrics.LPIPS(spatial=True)
    net.load_state_dict(sd)
    net = net.to(dev)
    net.chunk = N
    a = I.uniform((N, 3, SIZE, SIZE), 520, 0.0, 1.0).to(dev)
    b = (a + 0.3 * I.uniform((N, 3, SIZE, SIZE), 521).to(dev)).clamp(0, 1)
    return torch, pkg, dev, sd, net, a, b


def timing(args):
    torch, pkg, dev, sd, net, a, b = setup()
    from tests import lpips_torch as R
    L = pkg._lib
    dsd = {k: v.to(dev) for k, v in sd.items()}

    def native():
        return net.distance(a, b, L.LPIPS_TRANS)[0]

    def eager():  # trans, then the package's forward on all pairs at once, .mean() per pair
        with torch.no_grad():
            return R.forward(dsd, a * 2 - 1, b * 2 - 1, spatial=True).mean(dim=(1, 2, 3))

    def loop():  # calculate_lpips.py:102-112: one pair per forward
        with torch.no_grad():
            x, y = a[:LOOP_PAIRS] * 2 - 1, b[:LOOP_PAIRS] * 2 - 1
            return [R.forward(dsd, x[i:i + 1], y[i:i + 1], spatial=True).mean().detach().cpu().tolist()
                    for i in range(LOOP_PAIRS)]

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    for _ in range(2):  # warm-up: handle build, MIOpen's solver search
        vn, ve = native(), eager()
        loop()
    torch.cuda.synchronize()
    res = {k: [] for k in ('native', 'eager_batched', 'eager_loop')}
    for _ in range(args.repeats):
        res['native'].append(timed(native)[0] / N)
        res['eager_batched'].append(timed(eager)[0] / N)
        res['eager_loop'].append(timed(loop)[0] / LOOP_PAIRS)
    out = {'pairs': N, 'shape': [3, SIZE, SIZE], 'loop_pairs': LOOP_PAIRS, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0),
           'max_abs_native_vs_eager': float((vn - ve).abs().max())}
    for k, v in res.items():
        out[k + '_us_per_pair'] = {'median': 1e3 * statistics.median(v), 'min': 1e3 * min(v), 'max': 1e3 * max(v)}
    out['speedup_vs_eager_batched'] = statistics.median(res['eager_batched']) / statistics.median(res['native'])
    out['speedup_vs_eager_loop'] = statistics.median(res['eager_loop']) / statistics.median(res['native'])
    flops = sum(f for _, f in conv_layers())
    out['conv_mflop_per_image'] = flops / (2 * N) / 1e6
    out['native_conv_tflops'] = flops / (statistics.median(res['native']) * N * 1e-3) / 1e12
    merge(args.out, out)
    print(json.dumps(out))


def trace_run():
    torch, pkg, dev, sd, net, a, b = setup()
    for _ in range(TRACE_CALLS):
        net.distance(a, b, pkg._lib.LPIPS_TRANS)
    torch.cuda.synchronize()


def trace_csv(args):
    rows = sorted(csv.DictReader(open(args.trace_csv)), key=lambda r: int(r['Start_Timestamp']))
    rows = [r for r in rows if any(s in r['Kernel_Name'] for s in KERNELS)]
    n = len(rows) // TRACE_CALLS
    rows = rows[-n:]  # the last call
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3  # noqa: E731
    total = sum(dur(r) for r in rows)
    share = {}
    for r in rows:
        k = r['Kernel_Name'].replace('void ', '').replace('extdm::(anonymous namespace)::', '').split('(')[0]
        share[k] = share.get(k, 0.0) + dur(r)
    convs = [r for r in rows if 'conv2d_x3' in r['Kernel_Name']]
    layers = conv_layers()
    assert len(convs) == len(layers) + 1, (len(convs), len(layers))  # the stem runs once per image set
    us = [dur(convs[0]) + dur(convs[1])] + [dur(r) for r in convs[2:]]
    per = [{'layer': name, 'us': t, 'gflop': f / 1e9, 'tflops': f / t / 1e6, 'of_f16x3_peak': f / (t * 1e-6) / F16X3_PEAK}
           for (name, f), t in zip(layers, us)]
    out = {'trace_call_us': total, 'trace_us_per_pair': total / N,
           'kernel_share': {k: {'us': v, 'share': v / total} for k, v in sorted(share.items(), key=lambda kv: -kv[1])},
           'conv_layers': per,
           'largest_conv_launches': sorted(per, key=lambda p: -p['gflop'])[:3]}
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
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'lpips_alex.json'))
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--trace-csv')
    a = ap.parse_args()
    if a.trace_run:
        trace_run()
    elif a.trace_csv:
        trace_csv(a)
    else:
        timing(a)
