#!/bin/bash
# The LCGN attention's training benchmark and its kernel table: every GPU step under its own time limit, a failing step ends the run.
#   scripts/bench_lcgn_attention_train.sh [OUTDIR] [bf16]     (default: profiles/; bf16: the bf16 node against the fp32 node)
set -u
cd "$(dirname "$0")/.."
OUT=${1:-profiles}
MODE=${2:-}
TMP=$(mktemp -d)
mkdir -p "$OUT"
if [ "$MODE" = bf16 ]; then
timeout -k 10 480 python scripts/bench_lcgn_attention_train.py --bf16 --pairs 20 --warmup 5 --out "$OUT/lcgn_attention_bf16_bwd_bench.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP" -o lcgn_att_bwd -- \
    python scripts/bench_lcgn_attention_train.py --bf16 --profile &&
cp "$(find "$TMP" -name 'lcgn_att_bwd_kernel_stats.csv' | head -n 1)" "$OUT/lcgn_attention_bf16_bwd_kernel_stats.csv"
else
timeout -k 10 480 python scripts/bench_lcgn_attention_train.py --pairs 20 --warmup 5 --out "$OUT/lcgn_attention_bwd_bench.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP" -o lcgn_att_bwd -- \
    python scripts/bench_lcgn_attention_train.py --profile &&
cp "$(find "$TMP" -name 'lcgn_att_bwd_kernel_stats.csv' | head -n 1)" "$OUT/lcgn_attention_bwd_kernel_stats.csv"
fi
rc=$?
rm -rf "$TMP"
exit $rc
