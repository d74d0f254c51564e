#!/bin/bash
# lanes re-measured on the round's final library: B = 64 fp32 with 2 / 3 / 4 batches in flight, bf16 B = 256 with 2 / 3
set -eo pipefail
cd "${GRAFT_REPO_ROOT:-.}"
BENCH_OUT=${BENCH_OUT:-bench_out}; export BENCH_OUT; mkdir -p "$BENCH_OUT"
for rep in 1 2; do
for l in 3 2 4 5; do
  timeout -k 10 200 python3 bench.py --full --steps 100 --warmup 10 --no-other-configs --cpu-frames 0 --repeats 3 --no-roofline --lanes $l > "$BENCH_OUT/lanes_$l.json"
  python3 -c "import json;d=json.loads(open('$BENCH_OUT/lanes_$l.json').read().strip().splitlines()[-1]);print('fp32 B=64 lanes $l:', round(d['value']), d['value_spread']['min'], d['value_spread']['max'])"
done
for l in 2 3; do
  timeout -k 10 200 python3 bench.py --precision bf16 --batch 256 --steps 60 --warmup 10 --no-other-configs --cpu-frames 0 --repeats 3 --no-roofline --lanes $l --full > "$BENCH_OUT/lanes_bf16_$l.json"
  python3 -c "import json;d=json.loads(open('$BENCH_OUT/lanes_bf16_$l.json').read().strip().splitlines()[-1]);print('bf16 B=256 lanes $l:', round(d['value']), d['value_spread']['min'], d['value_spread']['max'])"
done
done
