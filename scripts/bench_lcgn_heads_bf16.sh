#!/bin/bash
# lcgn_seq(gat_heads = 4): fp32 against bf16 node features, and the kernel table of both forwards.  Every GPU step under its own time
# limit, a failing step ends the run.
#   scripts/bench_lcgn_heads_bf16.sh [OUTDIR]     (default: profiles/)
set -u
cd "$(dirname "$0")/.."
OUT=${1:-profiles}
TMP=$(mktemp -d)
mkdir -p "$OUT"
timeout -k 10 300 python scripts/bench_lcgn_heads_bf16.py --pairs 20 --warmup 5 --out "$OUT/lcgn_heads_bf16_bench.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP" -o lcgn_heads_bf16 -- \
    python scripts/bench_lcgn_heads_bf16.py --profile &&
cp "$(find "$TMP" -name 'lcgn_heads_bf16_kernel_stats.csv' | head -n 1)" "$OUT/lcgn_heads_bf16_kernel_stats.csv"
rc=$?
rm -rf "$TMP"
exit $rc
