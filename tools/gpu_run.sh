#!/bin/bash
# tests, bench and rocprofv3 kernel stats in one GPU session; results under $OUT (default: out/ in the repo root)
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"
OUT=${OUT:-$ROOT/out}; mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
TAG=${1:-x}
timeout -k 10 700 python -m pytest tests -q -m gpu --timeout 300 -p no:cacheprovider > $OUT/t_$TAG.log 2>&1
rc=$?; echo "pytest exit=$rc" >> $OUT/t_$TAG.log; tail -4 $OUT/t_$TAG.log
case $rc in 124|134|137|139) echo "pytest timed out or crashed ($rc); stopping"; exit 1;; esac
timeout -k 10 500 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
rc=$?; echo "bench exit=$rc"
if [ $rc -ne 0 ]; then tail -20 $OUT/bench_$TAG.err; exit 1; fi
cat $OUT/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $ROOT/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1
echo "rocprof exit=$?"
