#!/bin/bash
# usage: [OUT=dir] scripts/round_profile.sh <round> [workloads]   (run on a machine with the GPU)
# GPU parity tests, one full bench line per workload, then rocprofv3 kernel stats + PMC
# passes (scripts/prof.sh) for each workload; everything lands under $OUT (default bench_out/).
set -o pipefail
RND=${1:-r03}; WLS=${2:-"c2 c3 c4 c5 ref"}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { echo "pytest failed"; tail -30 "$OUT/pytest_gpu.log"; exit 1; }
tail -2 "$OUT/pytest_gpu.log"
for wl in $WLS; do
  timeout -k 10 200 python -u bench.py --full --workload $wl --steps 10 --warmup 3 > "$OUT/${RND}_${wl}_bench.json" 2> "$OUT/bench_$wl.err" || { echo "bench $wl failed"; tail -20 "$OUT/bench_$wl.err"; exit 1; }
  cut -c 1-300 "$OUT/${RND}_${wl}_bench.json"
done
for wl in $WLS; do
  bash scripts/prof.sh $wl "$OUT/prof_$wl" > "$OUT/prof_$wl.log" 2>&1 || { echo "prof $wl failed"; tail -20 "$OUT/prof_$wl.log"; exit 1; }
  echo "profiled $wl"
done
