#!/bin/bash
# round-4 artefacts in one call: HBM traffic counters (gpu_pmc.sh), MFMA-busy counters
# (gpu_pmc_mfma.sh), bench lines + rocprofv3 statistics (gpu_final.sh); summaries copied to profiles/
# (outputs under $OUT, default: out/ in the repo root)
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"
OUT=${OUT:-$ROOT/out}; mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd); export OUT
bash tools/gpu_pmc.sh > $OUT/final_pmc.log 2>&1 || { tail -5 $OUT/final_pmc.log; exit 1; }
cp $OUT/pmc_traffic.json profiles/pmc_traffic.json      # bench.py reads it from there
cd "$ROOT"
bash tools/gpu_pmc_mfma.sh > $OUT/final_pmc_mfma.log 2>&1 || { tail -5 $OUT/final_pmc_mfma.log; exit 1; }
cd "$ROOT"
[ -f $OUT/pmc_mfma.json ] && cp $OUT/pmc_mfma.json profiles/pmc_mfma.json
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE $OUT/pmcmfma_1 $OUT/pmcmfma_2
bash tools/gpu_final.sh
