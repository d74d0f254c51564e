#!/bin/bash
# Same-box A/B of BUILDS (scripts/ab_libs/<name>.so) inside the bf16 encoder at B=256: the whole-block kernels' rows of the layer table,
# the conv total, and the two-lane bench.   gpurun -- 'bash scripts/ab_libs_enc.sh OLD NEW'
set -eo pipefail
cd "${GRAFT_REPO_ROOT:-.}"
BENCH_OUT=${BENCH_OUT:-bench_out}; export BENCH_OUT; mkdir -p "$BENCH_OUT"
for round in 1 2; do
  for name in "$@"; do
    export POSERISK_LIB_PATH=$PWD/scripts/ab_libs/$name.so    # selected, never copied over the shipped library
    echo "== build $name (round $round)"
    python3 scripts/layer_table.py 256 bf16 2>/dev/null | grep -E "^L( 0|17|30) |total"
    timeout -k 10 200 python3 bench.py --full --precision bf16 --batch 256 --lanes 2 --cpu-frames 0 --no-roofline --steps 30 --repeats 3 > "$BENCH_OUT/ab_lib.json" 2>/dev/null
    python3 - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["BENCH_OUT"], "ab_lib.json")).read().strip().splitlines()[-1])
s = d["value_spread"]
print(f"bench {d['value']:9.1f} frames/s  ({s['min']:.0f} - {s['max']:.0f})")
PY
  done
done
