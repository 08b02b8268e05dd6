#!/bin/bash
# the full bench line and a rocprofv3 profile of the full run; results under $OUT (default: out/ in the repo root)
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"
OUT=${OUT:-$ROOT/out}; mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd); export OUT
TAG=${1:-x}; export TAG
timeout -k 10 500 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
rc=$?; echo "bench exit=$rc"; if [ $rc -ne 0 ]; then tail -20 $OUT/bench_$TAG.err; exit 1; fi
python3 -c "
import json, os; b=json.load(open(os.path.join(os.environ['OUT'], 'bench_%s.json' % os.environ['TAG'])))
print({k:b[k] for k in ('value','ms_per_step','mfma_frac_outer_iteration')}); print(b['roofline']); print(b['qp']); print(b.get('parity_converged'))"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $ROOT/bench.py --full --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1
echo "rocprof exit=$?"
