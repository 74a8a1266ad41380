#!/bin/bash
# Closing evidence, part 2: one bench line per non-BAIR BASELINE workload (bench.py --full --config,
# with its CPU baseline and its own lead kernel's roofline) -> $OUT/r05_bench_<config>.json.
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp
for c in ucf cityscapes smmnist kth; do
  timeout -k 10 500 python -u bench.py --full --config $c > $OUT/r05_bench_$c.json 2> $OUT/r05_bench_$c.err
  rc=$?; echo "$c rc=$rc"; [ $rc -ne 0 ] && { tail -5 $OUT/r05_bench_$c.err; exit $rc; }
  tail -1 $OUT/r05_bench_$c.json | python -c "import json,sys; d=json.loads(sys.stdin.read()); r=d.get('roofline') or {}; print(d['config']['bench_config'], d['value'], d['ms_per_step'], (d.get('cpu_baseline') or {}).get('value'), r.get('kernel', '')[:50], r.get('frac'), r.get('traffic'))"
done
