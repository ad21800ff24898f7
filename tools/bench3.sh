#!/bin/bash
# GPU box helper: parity tests + the three bench workloads, one line each
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; OUT=${OUT:-out}; mkdir -p $OUT
if [ "$1" != "notest" ]; then timeout 900 python -m pytest tests -m gpu -x -q > $OUT/t.log 2>&1; grep -E "passed|failed|rror" $OUT/t.log | tail -5; fi
for w in config2_100k_400x200_1pass config3_1M_400x200_4pass target_10M_400x200_4pass; do
  timeout 300 python bench.py --full --no-cpu-baseline --workload $w > $OUT/b_$w.log 2>&1
  echo $w $(grep -o "\"value\": [0-9.]*\|\"avg_launch_us\": [0-9.]*" $OUT/b_$w.log)
done
