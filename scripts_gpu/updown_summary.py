"""Folds updown_ab.sh's outputs ($OUT, default bench_out/) into profiles/updown_direct.json: the six stride-2
launches' rows of both kernel-stats files, the level-0 launches on both routes, every whole-step
value of both libraries with the gain rule (a difference of the means counts only above three times
the larger min-max spread), the default generations and the PMC traffic of layers 18 / 19 (profiles/pmc_layer18.json, pmc_layer19.json).
Usage: updown_summary.py [DIR] [OUT.json]"""
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, os.environ.get('OUT', 'bench_out'))
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'updown_direct.json')


def stride2_rows(path):
    """rows of the stride-2 launches: the implicit GEMM's <2, 2, BM, 1 (deconv)> / <4, 4, BM, 0>, the direct kernel's TT != 0"""
    rows = {}
    for r in csv.DictReader(open(path)):
        n = r['Name']
        k = n[n.find('conv_'):n.find('>(') + 1] if '>(' in n else n
        gemm = k.startswith('conv_gemm_x3_kernel<2, 2,') or k.startswith('conv_gemm_x3_kernel<4, 4,')
        direct = k.startswith('conv_x3_kernel<') and k.endswith(('true, 1>', 'true, 2>'))
        if gemm or direct:
            rows[k] = {'calls': int(r['Calls']), 'avg_us': round(float(r['AverageNs']) / 1e3, 1),
                       'min_us': round(float(r['MinNs']) / 1e3, 1), 'max_us': round(float(r['MaxNs']) / 1e3, 1),
                       'stddev_us': round(float(r['StdDev']) / 1e3, 1)}
    return rows


def last_json(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


def per_step(d):
    return sum(v['avg_us'] * v['calls'] for v in d.values()) / 41.0  # 41 forwards in a DDIM-20 generation


res = {'command': 'scripts_gpu/updown_ab.sh', 'per_launch': {}}
for arm in ('parent', 'direct'):
    res['per_launch'][arm] = stride2_rows(os.path.join(src, f'updown_{arm}_kernel_stats.csv'))
res['per_launch']['us_per_step'] = {arm: round(per_step(res['per_launch'][arm]), 1) for arm in ('parent', 'direct')}
res['level0_layers_us'] = json.load(open(os.path.join(src, 'layer_ab.json')))
steps = {}
for arm in ('parent', 'direct'):
    vals = []
    for rep in range(1, 100):
        p = os.path.join(src, f'ab_{arm}_{rep}.json')
        if not os.path.exists(p):
            break
        vals.append(last_json(p)['ms_per_step'])
    steps[arm] = {'ms_per_step': vals, 'mean': round(sum(vals) / len(vals), 4), 'spread': round(max(vals) - min(vals), 4)}
diff = steps['parent']['mean'] - steps['direct']['mean']
margin = 3.0 * max(steps['parent']['spread'], steps['direct']['spread'])
res['whole_step'] = {'command': 'bench.py --gpus 1 --steps 20 --warmup 5, libraries alternating', **steps,
                     'mean_difference_ms': round(diff, 4), 'margin_ms': round(margin, 4), 'counts_as_gain': bool(diff > margin)}
res['default_generation'] = {}
for arm in ('parent', 'direct'):
    d = last_json(os.path.join(src, f'default_{arm}.json'))
    res['default_generation'][arm] = {'ms_per_step': d['ms_per_step'], 'value': d['value']}
res['pmc'] = {str(l): json.load(open(os.path.join(REPO, 'profiles', f'pmc_layer{l}.json'))) for l in (18, 19)}
json.dump(res, open(out, 'w'), indent=1)
print(json.dumps({k: res[k] for k in ('whole_step', 'default_generation')}, indent=1))
print(res['per_launch']['us_per_step'])
