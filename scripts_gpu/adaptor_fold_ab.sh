#!/bin/bash
# The MotionAdaptor's normalise / LayerNorm passes folded into its convs against the parent library
# $LIBA (built from the parent commit, e.g. build(variant=..., csrc=...)): the first adaptor's last
# extrapolator and fuser convs on every route (adaptor_fold_layers.py), one rocprofv3 kernel trace of
# a DDIM-20 BAIR generation per library, whole steps (bench.py --steps 20) alternating four arms
# $ROUNDS times -- the parent library, this library, and this library with either fold switched off
# -- and one default generation of the parent and of this library. Everything lands in $OUT
# (default bench_out/); adaptor_fold_summary.py folds it into profiles/adaptor_fold.json.
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT; export TMPDIR=/tmp; export OUT
LIBA=${LIBA:?path of the parent commit\'s libextdm_hip.so}
case $LIBA in /*) ;; *) LIBA=$PWD/$LIBA;; esac
arm_env() {
  case $1 in
    parent) echo "EXTDM_LIB=$LIBA";;
    no_adaptor) echo "EXTDM_NO_ADAPTOR_FOLD=1";;
    no_ln) echo "EXTDM_NO_LN_FOLD=1";;
    *) echo "X=0";;
  esac
}
timeout -k 10 200 python -u scripts_gpu/adaptor_fold_layers.py > $OUT/adaptor_fold_layers.log 2>&1
rc=$?; echo "layers rc=$rc"; tail -8 $OUT/adaptor_fold_layers.log; [ $rc -ne 0 ] && exit $rc
for arm in parent fold; do
  P=$OUT/trace_$arm; rm -rf $P
  env $(arm_env $arm) timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $P -o run --output-format csv -- python bench.py --sampling-steps 20 --warmup 1 > $P.log 2>&1
  rc=$?; echo "trace $arm rc=$rc"; [ $rc -ne 0 ] && { tail -5 $P.log; exit $rc; }
  cp "$(find $P -name '*kernel_stats.csv' | head -1)" $OUT/adaptor_fold_${arm}_kernel_stats.csv
  find $P -name "*trace*.csv" -delete
done
for rep in $(seq 1 ${ROUNDS:-5}); do
  for arm in parent fold no_adaptor no_ln; do
    env $(arm_env $arm) timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/ab_${arm}_$rep.json 2> $OUT/ab_${arm}_$rep.err
    rc=$?; [ $rc -ne 0 ] && { echo "ab $arm $rep rc=$rc"; tail -5 $OUT/ab_${arm}_$rep.err; exit $rc; }
    python -c "import json,os; d=json.loads(open(os.environ['OUT']+'/ab_${arm}_$rep.json').read().strip().splitlines()[-1]); print('ab', '$arm', $rep, d.get('ms_per_step'), d.get('workspace_gb'))"
  done
done
for arm in parent fold; do
  env $(arm_env $arm) timeout -k 10 300 python bench.py --gpus 1 > $OUT/default_$arm.json 2> $OUT/default_$arm.err
  rc=$?; [ $rc -ne 0 ] && { echo "default $arm rc=$rc"; tail -5 $OUT/default_$arm.err; exit $rc; }
done
echo done
