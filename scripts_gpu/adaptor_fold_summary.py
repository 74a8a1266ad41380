"""Folds adaptor_fold_ab.sh's outputs ($OUT, default bench_out/) into profiles/adaptor_fold.json: per
library the kernel-stats rows of the passes the folds remove (adaptor_stats, adaptor_norm,
channel_ln*), of the statistics kernels that replace them and of every conv_x3 template whose launch
count differs between the two traces, with their per-step sums; the bench-layer timings; every
whole-step value of the four arms with the gain rule (a difference of the means counts only above
three times the larger min-max spread of the two series); the default generations and workspace_gb.
Usage: adaptor_fold_summary.py [DIR] [OUT.json]"""
import csv
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, os.environ.get('OUT', 'bench_out'))
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'adaptor_fold.json')
FORWARDS = 41.0  # forwards of a DDIM-20 generation (warm-up included)
PASSES = ('adaptor_stats_kernel', 'adaptor_norm_kernel', 'channel_ln4_kernel', 'channel_ln_kernel',
          'adaptor_stats_inc_kernel', 'channel_ln_stats4_kernel', 'channel_ln_stats_kernel')


def short(n):
    n = n.replace('extdm::(anonymous namespace)::', '').replace('void ', '')
    return n[:n.find('>(') + 1] if '>(' in n else n[:n.find('(')] if '(' in n else n


def rows(path):
    r = {}
    for x in csv.DictReader(open(path)):
        r[short(x['Name'])] = {'calls': int(x['Calls']), 'total_us': round(float(x['TotalDurationNs']) / 1e3, 1),
                               'avg_us': round(float(x['AverageNs']) / 1e3, 1), 'min_us': round(float(x['MinNs']) / 1e3, 1),
                               'max_us': round(float(x['MaxNs']) / 1e3, 1), 'stddev_us': round(float(x['StdDev']) / 1e3, 1)}
    return r


def last_json(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


def workspace_gb(path):
    m = re.search(r'"workspace_gb": ([0-9.]+)', open(path).read())  # nested in the result line
    return float(m.group(1)) if m else None


tr = {arm: rows(os.path.join(src, f'adaptor_fold_{arm}_kernel_stats.csv')) for arm in ('parent', 'fold')}
res = {'command': 'scripts_gpu/adaptor_fold_ab.sh', 'per_launch': {}}
# conv_x3 templates whose launch count changed: the convs that moved to (or from) an affine template
moved = sorted(k for k in set(tr['parent']) | set(tr['fold']) if k.startswith('conv_x3_kernel<') and
               tr['parent'].get(k, {}).get('calls', 0) != tr['fold'].get(k, {}).get('calls', 0))
for arm in ('parent', 'fold'):
    t = tr[arm]
    passes = {k: t[k] for k in PASSES if k in t}
    convs = {k: t[k] for k in moved if k in t}
    res['per_launch'][arm] = {
        'passes': passes, 'convs_whose_template_changed': convs,
        'passes_ms_per_step': round(sum(v['total_us'] for v in passes.values()) / FORWARDS / 1e3, 4),
        'convs_ms_per_step': round(sum(v['total_us'] for v in convs.values()) / FORWARDS / 1e3, 4),
        'launches_per_step': round(sum(v['calls'] for v in list(passes.values()) + list(convs.values())) / FORWARDS, 2),
        'all_kernels_ms_per_step': round(sum(v['total_us'] for v in t.values()) / FORWARDS / 1e3, 4)}
p, f = res['per_launch']['parent'], res['per_launch']['fold']
res['per_launch']['saving_ms_per_step'] = round(p['passes_ms_per_step'] + p['convs_ms_per_step'] -
                                                f['passes_ms_per_step'] - f['convs_ms_per_step'], 4)
lp = os.path.join(src, 'adaptor_fold_layers.json')
if os.path.exists(lp):
    res['bench_layers_20_21'] = json.load(open(lp))
steps = {}
for arm in ('parent', 'fold', 'no_adaptor', 'no_ln'):
    vals, ws = [], None
    for rep in range(1, 100):
        q = os.path.join(src, f'ab_{arm}_{rep}.json')
        if not os.path.exists(q):
            break
        d = last_json(q)
        vals.append(d['ms_per_step'])
        ws = workspace_gb(q)
    if vals:
        steps[arm] = {'ms_per_step': vals, 'mean': round(sum(vals) / len(vals), 4), 'spread': round(max(vals) - min(vals), 4),
                      'workspace_gb': ws}


def gain(a, b):
    diff = steps[a]['mean'] - steps[b]['mean']
    margin = 3.0 * max(steps[a]['spread'], steps[b]['spread'])
    return {'mean_difference_ms': round(diff, 4), 'margin_ms': round(margin, 4), 'counts_as_gain': bool(diff > margin)}


res['whole_step'] = {'command': 'bench.py --gpus 1 --steps 20 --warmup 5, arms alternating', **steps}
if 'parent' in steps and 'fold' in steps:
    res['whole_step']['parent_vs_fold'] = gain('parent', 'fold')
if 'no_adaptor' in steps and 'fold' in steps:
    res['whole_step']['adaptor_fold_alone'] = gain('no_adaptor', 'fold')
if 'no_ln' in steps and 'fold' in steps:
    res['whole_step']['ln_fold_alone'] = gain('no_ln', 'fold')
res['default_generation'] = {}
for arm in ('parent', 'fold'):
    q = os.path.join(src, f'default_{arm}.json')
    if os.path.exists(q):
        d = last_json(q)
        res['default_generation'][arm] = {'ms_per_step': d['ms_per_step'], 'value': d['value'], 'workspace_gb': workspace_gb(q)}
json.dump(res, open(out, 'w'), indent=1)
print(json.dumps({k: res[k] for k in ('whole_step', 'default_generation')}, indent=1))
print({k: v for k, v in res['per_launch'].items() if k == 'saving_ms_per_step'}, p['passes_ms_per_step'], f['passes_ms_per_step'],
      p['convs_ms_per_step'], f['convs_ms_per_step'])
