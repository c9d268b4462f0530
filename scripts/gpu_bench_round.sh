#!/bin/bash
# usage (on a machine with the GPU): [OUT=dir] scripts/gpu_bench_round.sh <round> "<name:bench args;...>"
# one full bench line per entry (checks, roofline, CPU baseline included) -> $OUT/<round>_<name>_bench.json
# (OUT defaults to bench_out/)
set -o pipefail
RND=$1
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
IFS=';' read -ra BL <<< "$2"
for b in "${BL[@]}"; do
  name="${b%%:*}"; args="${b#*:}"
  timeout -k 10 400 python -u bench.py --full $args > "$OUT/${RND}_${name}_bench.json" 2> "$OUT/${RND}_${name}_bench.err"
  rc=$?
  [ $rc -eq 0 ] || { echo "bench $name failed (status $rc)"; tail -5 "$OUT/${RND}_${name}_bench.err"; exit 2; }
  cut -c 1-240 "$OUT/${RND}_${name}_bench.json"
done
