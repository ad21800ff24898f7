#!/bin/bash
# GPU helper: the bench lines of every workload and of the launch shapes (20 steps, self-launch, force-slots) -> $OUT/<tag>_bench_*.json
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; tag=${1:-r05}; OUT=${OUT:-out}
tools/bench_all.sh $tag 2>&1 | tail -12
python bench.py --full --steps 20 --warmup 5 > $OUT/${tag}_bench_target_20.json 2>/dev/null
python bench.py --full --no-cpu-baseline --self-launch > $OUT/${tag}_bench_target_selflaunch.json 2>/dev/null
python bench.py --full --no-cpu-baseline --force-slots > $OUT/${tag}_bench_target_forceslots.json 2>/dev/null
python bench.py --full --no-cpu-baseline --force-slots --strong > $OUT/${tag}_bench_target_forceslots_strong.json 2>/dev/null
for f in target_20 target_selflaunch target_forceslots target_forceslots_strong; do echo "$f $(grep -o '"value": [0-9.]*' $OUT/${tag}_bench_$f.json | head -1)"; done
