#!/bin/bash
# scratch: kernel traces of the full benchmark run for several option sets + per-iteration budget
# (results under $OUT, default: out/ in the repo root)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out}; mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
TAG=${1:-x}; shift
cd /tmp && export TMPDIR=/tmp
i=0
for O in "$@"; do
  i=$((i+1))
  export AA_HIP_OPTIONS="$O"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_$i -- python3 $ROOT/bench.py --full --no-cpu-baseline --steps 40 $BENCH_ARGS > $OUT/prof_${TAG}_$i.log 2>&1 || { echo "profile $i failed"; tail -5 $OUT/prof_${TAG}_$i.log; exit 1; }
  echo "=== profile $i ($O)"
  python3 $ROOT/tools/trace_summary.py $OUT/prof_${TAG}_$i 30 | tee $OUT/prof_${TAG}_$i.summary
done
