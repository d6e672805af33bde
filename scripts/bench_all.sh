#!/bin/bash
# the bench lines in full (headline bandit with its CPU baseline and sub-objects, linear, darkroom),
# then the training and DarkRoom per-step timings; output under bench_out/ (or $BENCH_OUT)
cd "$(dirname "$0")/.." || exit 1
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full > "$OUT/bench_bandit.log" 2>&1 || exit $?
timeout -k 10 600 python bench.py --full --workload linear --no-cpu-baseline > "$OUT/bench_linear.log" 2>&1 || exit $?
timeout -k 10 600 python bench.py --full --workload darkroom > "$OUT/bench_darkroom.log" 2>&1 || exit $?
timeout -k 10 600 python bench.py --full --workload darkroom --tasks 8192 > "$OUT/bench_darkroom_c5.log" 2>&1 || exit $?
timeout -k 10 300 python scripts/train_timing.py > "$OUT/train_timing.json" 2> "$OUT/train_timing.err" || exit $?
timeout -k 10 300 python scripts/dr_step_timing.py > "$OUT/dr_step_timing.json" 2> "$OUT/dr_step_timing.err"
