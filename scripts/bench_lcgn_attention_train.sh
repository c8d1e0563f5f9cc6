#!/bin/bash
# The LCGN attention's training benchmark and its kernel table: every GPU step under its own time limit, a failing step ends the run.
#   scripts/bench_lcgn_attention_train.sh [OUTDIR]     (default: profiles/)
set -u
cd "$(dirname "$0")/.."
OUT=${1:-profiles}
TMP=$(mktemp -d)
mkdir -p "$OUT"
timeout -k 10 480 python scripts/bench_lcgn_attention_train.py --pairs 20 --warmup 5 --out "$OUT/lcgn_attention_bwd_bench.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP" -o lcgn_att_bwd -- \
    python scripts/bench_lcgn_attention_train.py --profile &&
cp "$(find "$TMP" -name 'lcgn_att_bwd_kernel_stats.csv' | head -n 1)" "$OUT/lcgn_attention_bwd_kernel_stats.csv"
rc=$?
rm -rf "$TMP"
exit $rc
