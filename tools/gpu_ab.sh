#!/bin/bash
# scratch: A/B of option sets on the benchmark's headline figure in one box; usage: gpu_ab.sh "opts A" "opts B" ...
# (results under $OUT, default: out/ in the repo root)
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"
OUT=${OUT:-$ROOT/out}; mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
i=0
for O in "$@" "$1"; do
  i=$((i+1))
  AA_HIP_OPTIONS="$O" timeout -k 10 300 python bench.py $BENCH_ARGS > $OUT/ab_$i.json 2> $OUT/ab_$i.err || { echo "bench failed ($O)"; tail -5 $OUT/ab_$i.err; exit 1; }
  python3 -c "
import json; b=json.load(open('$OUT/ab_$i.json')); print('%-40s %.1f it/s  %.3f ms' % ('$O' or '(defaults)', b['value'], b['ms_per_step']))"
done
