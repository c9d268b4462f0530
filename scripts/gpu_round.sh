#!/bin/bash
# usage: [OUT=dir] scripts/gpu_round.sh   (run on a machine with the GPU): GPU parity tests, then full bench lines;
# logs and lines land under $OUT (default bench_out/)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { echo "pytest failed"; tail -30 "$OUT/pytest_gpu.log"; exit 1; }
tail -3 "$OUT/pytest_gpu.log"
for wl in ${WLS:-c2 c4}; do
  timeout -k 10 200 python -u bench.py --full --workload $wl --steps 10 --warmup 3 > "$OUT/bench_$wl.json" 2> "$OUT/bench_$wl.err" || { echo "bench $wl failed"; tail -20 "$OUT/bench_$wl.err"; exit 1; }
  cat "$OUT/bench_$wl.json"
done
