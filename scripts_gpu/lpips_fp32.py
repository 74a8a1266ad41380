"""LPIPS's exact-fp32 route (EXTDM_LPIPS_FP32, csrc/lpips_f32.hip) against the f16x3 route and the
batched eager PyTorch-ROCm fp32 baseline of scripts_gpu/lpips_alex.py, at its shape (4096 pairs of
3 x 64 x 64): device events, the three alternating in one process after two warm-up rounds, median
and range of --repeats, in microseconds per pair. Writes profiles/lpips_fp32.json (or --out).

  python scripts_gpu/lpips_fp32.py [--repeats 9] [--out profiles/lpips_fp32.json]
  rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python scripts_gpu/lpips_fp32.py --trace-run
  python scripts_gpu/lpips_fp32.py --trace-csv DIR/run_kernel_trace.csv --out profiles/lpips_fp32.json
      (adds the fp32 route's per-kernel shares and the algorithmic FLOP/s of its conv launches
      against the 157.3 TF/s fp32-MFMA peak to the JSON)
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_alex  # noqa: E402

REPO = lpips_alex.REPO
N = lpips_alex.N
FP32_PEAK = 157.3e12
TRACE_CALLS = 3
KERNELS = ('conv2d_f32', 'maxpool2d_32', 'lpips_head', 'lpips_mean', 'lpips_map')


def nets():
    """(torch, pkg, dev, state, {route: LPIPS}, a, b): both routes on one module's weights."""
    torch, pkg, dev, sd, net, a, b = lpips_alex.setup()
    net32 = pkg.metrics.LPIPS(spatial=True)
    net32.load_state_dict(sd)
    net32 = net32.to(dev)
    net32.chunk = N
    net32.precision = 'fp32'
    return torch, pkg, dev, sd, {'f16x3': net, 'fp32': net32}, a, b


def timing(args):
    torch, pkg, dev, sd, net, a, b = nets()
    from tests import lpips_torch as R
    L = pkg._lib
    dsd = {k: v.to(dev) for k, v in sd.items()}

    def eager():  # trans, then the package's forward on all pairs at once, .mean() per pair
        with torch.no_grad():
            return R.forward(dsd, a * 2 - 1, b * 2 - 1, spatial=True).mean(dim=(1, 2, 3))
    runs = {'fp32': lambda: net['fp32'].distance(a, b, L.LPIPS_TRANS)[0],
            'f16x3': lambda: net['f16x3'].distance(a, b, L.LPIPS_TRANS)[0],
            'eager_batched': eager}

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r
    last = {}
    for _ in range(2):  # warm-up: handle builds, the fp32 tiles' upload, MIOpen's solver search
        for k, f in runs.items():
            last[k] = f()
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, f in runs.items():
            res[k].append(timed(f)[0] / N)
    out = {'pairs': N, 'shape': [3, lpips_alex.SIZE, lpips_alex.SIZE], 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0),
           'max_abs_fp32_vs_f16x3': float((last['fp32'] - last['f16x3']).abs().max()),
           'max_abs_fp32_vs_eager': float((last['fp32'] - last['eager_batched']).abs().max())}
    for k, v in res.items():
        out[k + '_us_per_pair'] = {'median': 1e3 * statistics.median(v), 'min': 1e3 * min(v), 'max': 1e3 * max(v)}
    m = {k: statistics.median(v) for k, v in res.items()}
    out['fp32_over_f16x3'] = m['fp32'] / m['f16x3']
    out['eager_batched_over_fp32'] = m['eager_batched'] / m['fp32']
    out['eager_batched_over_f16x3'] = m['eager_batched'] / m['f16x3']
    flops = sum(f for _, f in lpips_alex.conv_layers())
    out['fp32_conv_tflops'] = flops / (m['fp32'] * N * 1e-3) / 1e12
    lpips_alex.merge(args.out, out)
    print(json.dumps(out))


def trace_run():
    torch, pkg, dev, sd, net, a, b = nets()
    for _ in range(TRACE_CALLS):
        net['fp32'].distance(a, b, pkg._lib.LPIPS_TRANS)
    torch.cuda.synchronize()


def trace_csv(args):
    rows = sorted(csv.DictReader(open(args.trace_csv)), key=lambda r: int(r['Start_Timestamp']))
    rows = [r for r in rows if any(s in r['Kernel_Name'] for s in KERNELS)]
    rows = rows[-(len(rows) // TRACE_CALLS):]  # the last call
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3  # noqa: E731
    total = sum(dur(r) for r in rows)
    share = {}
    for r in rows:
        k = r['Kernel_Name'].replace('void ', '').replace('extdm::(anonymous namespace)::', '').split('(')[0]
        share[k] = share.get(k, 0.0) + dur(r)
    convs = [r for r in rows if 'conv2d_f32' in r['Kernel_Name']]
    layers = lpips_alex.conv_layers()
    assert len(convs) == len(layers) + 1, (len(convs), len(layers))  # the stem runs once per image set
    us = [dur(convs[0]) + dur(convs[1])] + [dur(r) for r in convs[2:]]
    per = [{'layer': name, 'us': t, 'gflop': f / 1e9, 'tflops': f / t / 1e6, 'of_fp32_mfma_peak': f / (t * 1e-6) / FP32_PEAK}
           for (name, f), t in zip(layers, us)]
    out = {'trace_call_us': total, 'trace_us_per_pair': total / N,
           'kernel_share': {k: {'us': v, 'share': v / total} for k, v in sorted(share.items(), key=lambda kv: -kv[1])},
           'conv_layers': per}
    lpips_alex.merge(args.out, out)
    print(json.dumps(out))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'lpips_fp32.json'))
    ap.add_argument('--trace-run', action='store_true')
    ap.add_argument('--trace-csv')
    a = ap.parse_args()
    if a.trace_run:
        trace_run()
    elif a.trace_csv:
        trace_csv(a)
    else:
        timing(a)
