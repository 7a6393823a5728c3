#!/bin/bash
# Importance-kernel occupancy evidence of one build: bash profiles/collect_occupancy.sh <tag> [other libgjx_hip.so]
#   1. rocprofv3 --kernel-trace --stats -- python bench.py            (durations per 32-pass launch)
#   2. two counter runs of the same command, on their own (never together with tracing)
# -> $OUT_ROOT/occupancy_<tag>/{trace,pmc1,pmc2} (OUT_ROOT defaults to build/profiles) and, by profiles/summarize_occupancy.py,
#    its summary.json: the figures quoted in profiles/occupancy_summary.md
set -o pipefail
TAG=$1
cd "$(dirname "$0")/.." || exit 1
if [ -n "$2" ]; then export GJX_HIP_LIB=$2; else unset GJX_HIP_LIB; fi
export TMPDIR=/tmp
OUT=${OUT_ROOT:-build/profiles}/occupancy_$TAG
rm -rf "$OUT"; mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o t -- python bench.py > "$OUT/trace.log" 2>&1 \
  || { echo "trace run failed"; tail -5 "$OUT/trace.log"; exit 1; }
timeout -k 10 400 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d "$OUT/pmc1" -o p -- python bench.py > "$OUT/pmc1.log" 2>&1 \
  || { echo "counter run 1 failed"; tail -5 "$OUT/pmc1.log"; exit 1; }
timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_INST_ANY --output-format csv -d "$OUT/pmc2" -o p -- python bench.py > "$OUT/pmc2.log" 2>&1 \
  || { echo "counter run 2 failed"; tail -5 "$OUT/pmc2.log"; exit 1; }
python3 profiles/summarize_occupancy.py "$TAG" "$OUT" "$OUT/summary.json" && cat "$OUT/summary.json"
# the raw per-dispatch tables are large: the summary is what is kept
find "$OUT" -name "*.csv" -size +256k -delete
