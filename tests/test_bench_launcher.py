"""bench.py's multi-rank path on CPU: `--gpus 2` without a launcher spawns two
ranks (gloo, the --stub workload), shards the clip batch, all-gathers it back in
global order, takes the max-over-ranks time and prints n_gpus = 2; `--steps K`
times exactly K steps (whole stub generations of 4, then the leading steps of the
next); a plain run prints one result line, `--full` the partial line first;
`--dump-outputs` writes what the last timed step delivered."""
import json
import os
import subprocess
import sys

import numpy as np

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--stub', *args], env=env,
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    return lines


def test_launcher_spawns_two_ranks():
    lines = _run('--gpus', '2', '--batch', '3', '--steps', '6', '--warmup', '0', '--full')
    assert len(lines) == 2 and lines[0]['partial'] and not lines[-1]['partial']
    res = lines[-1]
    assert res['n_gpus'] == 2
    assert res['config']['global_batch'] == 6
    assert res['steps'] == 6 and res['generations'] == 1.5  # one stub generation of 4 and 2 steps of the next
    assert res['value'] > 0 and res['scaling'] == 'weak'
    assert 'roofline' in res


def test_single_rank_default():
    res = _run('--batch', '2', '--steps', '1')[-1]
    assert res['n_gpus'] == 1 and res['steps'] == 1 and res['generations'] == 0.25
    res = _run('--batch', '2')[-1]
    assert res['steps'] == 4 and res['generations'] == 1  # the default: one generation


def test_plain_run_prints_one_line(tmp_path):
    """No --full: one result line without the roofline / CPU baseline legs; ms_per_step is the
    timed wall over the steps asked for, value the frames in proportion to them; the dumped
    array is the last timed step's, float32, the same from run to run."""
    outs = []
    for tag in ('a', 'b'):
        lines = _run('--batch', '3', '--steps', '8', '--warmup', '0', '--total-pred', '5',
                     '--dump-outputs', str(tmp_path / tag))
        assert len(lines) == 1 and not lines[0]['partial']
        res = lines[0]
        assert 'roofline' not in res and 'cpu_baseline' not in res
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in res
        assert res['steps'] == 8 and res['generations'] == 2
        assert abs(res['ms_per_step'] * 8 - res['timed_s'] * 1e3) < 1.0
        # 2 generations x 3 clips x 5 frames over the timed wall
        assert abs(res['value'] - 30 / (res['ms_per_step'] * 8e-3)) < 1e-2 * res['value']
        assert os.listdir(tmp_path / tag) == ['videos.npy']
        outs.append(np.load(tmp_path / tag / 'videos.npy'))
    assert outs[0].dtype == np.float32 and outs[0].shape == (3, 3, 2)
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][:, 0, 0], np.arange(3, dtype=np.float32))


def test_dump_inside_a_generation(tmp_path):
    _run('--batch', '2', '--steps', '5', '--warmup', '0', '--dump-outputs', str(tmp_path / 'd'))
    assert os.listdir(tmp_path / 'd') == ['latent.npy']


def test_dump_sample_is_fixed_and_bounded():
    small = np.arange(24, dtype=np.float64).reshape(4, 6)
    s = bench.dump_sample(small)
    assert s.dtype == np.float32 and np.array_equal(s, small)
    # 100 clips of 1 MiB: the budget holds 48 of them, the same ones every time, in ascending order
    big = np.broadcast_to(np.arange(100, dtype=np.float32)[:, None], (100, 2 ** 18))
    a, b = bench.dump_sample(big), bench.dump_sample(big)
    assert a.nbytes <= bench.DUMP_BYTES and a.shape == (48, 2 ** 18)
    assert np.array_equal(a, b)
    ids = a[:, 0]
    assert np.all(np.diff(ids) > 0) and np.array_equal(a, big[ids.astype(int)])
