#!/bin/bash
# Samples the GPU's clock / power (rocm-smi) while bench.py runs: is the fp32 step held down by the power limit?
#   gpurun -- 'bash scripts/exp_clock_sample.sh [bench args...]'
cd "${GRAFT_REPO_ROOT:-.}"
BENCH_OUT=${BENCH_OUT:-bench_out}; export BENCH_OUT; mkdir -p "$BENCH_OUT"
python3 bench.py --full --cpu-frames 0 --no-roofline --steps 1500 --repeats 4 "$@" > "$BENCH_OUT/clock_bench.json" 2> "$BENCH_OUT/clock_bench.err" &
pid=$!
while kill -0 $pid 2>/dev/null; do
  rocm-smi --showclocks --showpower 2>/dev/null | grep -E "sclk|Power \(W\)" | sed -e 's/.*sclk clock level: [0-9S]*: //' -e 's/.*Power (W): / W /' | tr '\n' ' '
  echo
  sleep 0.7
done
wait $pid
python3 -c "
import json; d=json.loads(open('$BENCH_OUT/clock_bench.json').read().strip().splitlines()[-1]); print(d['value'], d['value_spread'], d.get('frames_per_s_one_batch_in_flight'))"
