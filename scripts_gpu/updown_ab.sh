#!/bin/bash
# The stride-2 convs on the direct two-tap kernel against the parent library $LIBA (built from the
# parent commit, e.g. build(variant=..., csrc=...)): the level-0 launches on both routes
# (updown_layers.py), one rocprofv3 kernel trace of a DDIM-20 BAIR generation per library, whole
# steps (bench.py --steps 20) alternating the two libraries $ROUNDS times, one default generation
# each, the PMC passes of bench layers 18 / 19. Everything but the PMC files lands in $OUT (default bench_out/);
# updown_summary.py folds it, with the PMC files once copied to profiles/, into profiles/updown_direct.json.
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp; export OUT
LIBA=${LIBA:?path of the parent commit\'s libextdm_hip.so}
case $LIBA in /*) ;; *) LIBA=$PWD/$LIBA;; esac
lib_env() { if [ $1 = parent ]; then echo "EXTDM_LIB=$LIBA"; else echo "X=0"; fi; }
timeout -k 10 200 python -u scripts_gpu/updown_layers.py > $OUT/updown_layers.log 2>&1
rc=$?; echo "layers rc=$rc"; tail -13 $OUT/updown_layers.log; [ $rc -ne 0 ] && exit $rc
for arm in parent direct; do
  P=$OUT/trace_$arm; rm -rf $P
  env $(lib_env $arm) timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $P -o run --output-format csv -- python bench.py --sampling-steps 20 --warmup 1 > $P.log 2>&1
  rc=$?; echo "trace $arm rc=$rc"; [ $rc -ne 0 ] && { tail -5 $P.log; exit $rc; }
  cp "$(find $P -name '*kernel_stats.csv' | head -1)" $OUT/updown_${arm}_kernel_stats.csv
  find $P -name "*trace*.csv" -delete
done
for rep in $(seq 1 ${ROUNDS:-5}); do
  for arm in parent direct; do
    env $(lib_env $arm) timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/ab_${arm}_$rep.json 2> $OUT/ab_${arm}_$rep.err
    rc=$?; [ $rc -ne 0 ] && { echo "ab $arm $rep rc=$rc"; tail -5 $OUT/ab_${arm}_$rep.err; exit $rc; }
    python -c "import json,os; d=json.loads(open(os.environ['OUT']+'/ab_${arm}_$rep.json').read().strip().splitlines()[-1]); print('ab', '$arm', $rep, d.get('ms_per_step'), d.get('value'))"
  done
done
for arm in parent direct; do
  env $(lib_env $arm) timeout -k 10 300 python bench.py --gpus 1 > $OUT/default_$arm.json 2> $OUT/default_$arm.err
  rc=$?; [ $rc -ne 0 ] && { echo "default $arm rc=$rc"; tail -5 $OUT/default_$arm.err; exit $rc; }
done
LAYERS="18 19" bash scripts_gpu/pmc_layers.sh
