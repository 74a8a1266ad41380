#!/bin/bash
# Closing measurement on the in-tree library (TAG, default r05), each step under its own limit:
#   1. PMC FETCH / WRITE passes of every BAIR roofline kernel and of each other config's lead
#      (pmc_layers.sh -> gpurun_out/pmc_layer<id>.json, pmc_<config>_layer<id>.json; copied to
#      profiles/ by the caller: bench.py reports traffic only from PMC files of the same library sha)
#   2. one rocprofv3 kernel trace of a DDIM-20 BAIR generation (same kernels and shapes as DDPM-1000,
#      whose 2000 graph replays crash the profiler) -> ${TAG}_bair_ddim20_kernel_stats.csv + the
#      per-launch groups of the attention and conv kernels (kernel_launches.py)
# SKIP_PMC=1 skips 1; SKIP_PROF=1 skips 2.
cd "${GRAFT_REPO_ROOT:-/root/repo}"; mkdir -p gpurun_out; export TMPDIR=/tmp
TAG=${TAG:-r05}
( while sleep 45; do echo "heartbeat $(date +%T)" >> gpurun_out/${TAG}_heartbeat.log; done ) &
HB=$!
trap 'kill $HB' EXIT
sha256sum 140-extdm-distribution-extrapolation-diffusion-model-for-video-prediction_amd/libextdm_hip.so | cut -c1-16
if [ -z "$SKIP_PMC" ]; then
  CONFIG=bair bash scripts_gpu/pmc_layers.sh || exit 1
  for c in kth cityscapes ucf smmnist; do CONFIG=$c LAYERS=6 bash scripts_gpu/pmc_layers.sh || exit 1; done
fi
if [ -z "$SKIP_PROF" ]; then
  OUT=${OUT:-bench_out}; mkdir -p $OUT  # step 2 writes here
  P=$OUT/prof_$TAG
  rm -rf $P
  # no --steps: one whole generation (2 rounds x 20 steps), with the roofline's launches as before
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $P -o run --output-format csv -- python bench.py --sampling-steps 20 --warmup 1 --full --no-cpu-baseline > $P.log 2>&1
  rc=$?; echo "rocprof rc=$rc"; tail -2 $P.log; [ $rc -ne 0 ] && exit $rc
  cp "$(find $P -name '*kernel_stats.csv' | head -1)" $OUT/${TAG}_bair_ddim20_kernel_stats.csv
  for p in attn_x3_kernel cross_attn_x3p conv_x3_kernel xpath_x3 sampler; do python scripts_gpu/kernel_launches.py $P $p; done > $OUT/${TAG}_bair_ddim20_launches.txt
  find $P -name "*kernel_trace.csv" -delete
fi
