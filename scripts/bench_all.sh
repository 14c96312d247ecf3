#!/bin/bash
# All bench configurations (one JSON line each, --full: with the roofline and
# the CPU baselines); outputs under $OUT (default results/; copied into
# profiles/<round>/).
set -o pipefail
OUT=${OUT:-results}
mkdir -p $OUT
for cfg in ${@:-c2 vcm c3 c4}; do
  timeout -k 10 400 python3 -u bench.py --full --config $cfg > $OUT/bench_$cfg.log 2>&1 \
    || { echo "bench $cfg failed rc=$?"; tail -5 $OUT/bench_$cfg.log; exit 1; }
  tail -1 $OUT/bench_$cfg.log > $OUT/bench_$cfg.json
  echo "$cfg: $(python3 -c "import json; d=json.load(open('$OUT/bench_$cfg.json')); print(d['value'], d['unit'], 'cpu', d['cpu_baseline']['value'], d['cpu_baseline']['kind'], d['cpu_baseline'].get('film_bit_exact'))")"
done
