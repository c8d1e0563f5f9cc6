#!/usr/bin/env python3
"""Summarise the rocprofv3 PMC passes of bench.py into profiles/<tag>_pmc_hbm_cfg3.json.

Run on the GPU box (one counter per pass, counters in their own runs without any sys/hip trace, as gpurun requires):
    export TMPDIR=/tmp
    for c in FETCH_SIZE WRITE_SIZE; do
      rocprofv3 --pmc $c --kernel-trace --output-format csv -d gpurun_out/pmc_$c -o pmc -- \
          python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline
    done
    python scripts/collect_pmc.py gpurun_out r01g
FETCH_SIZE / WRITE_SIZE are in KiB; on gfx950 FETCH_SIZE counts 64 B per 128 B request of a wide coalesced stream
(MI355X_MICROARCH.md, HBM section), so read bytes = FETCH_SIZE * 1024 * 2; WRITE_SIZE * 1024 matches the known output."""
import csv, glob, json, os, sys, collections

root, tag = sys.argv[1], sys.argv[2]
kern = collections.defaultdict(dict)
for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
    files = glob.glob(os.path.join(root, f"pmc_{ctr}", "**", "*counter_collection.csv"), recursive=True)
    assert files, f"no counter_collection.csv for {ctr}"
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(files[0])):
        if r["Counter_Name"] == ctr:
            acc[r["Kernel_Name"].split("(")[0]].append(float(r["Counter_Value"]))
    for k, v in acc.items():
        kern[k][ctr] = {"launches": len(v), "avg_KiB": sum(v) / len(v)}
mp = next(k for k in kern if "k_gat_mp_tiled" in k)
rd = kern[mp]["FETCH_SIZE"]["avg_KiB"] * 1024 * 2
wr = kern[mp]["WRITE_SIZE"]["avg_KiB"] * 1024
out = {"source": "rocprofv3 --pmc <counter> --kernel-trace --output-format csv -- python bench.py --full --steps 3 --warmup 1 "
                 "--no-cpu-baseline (one pass per counter); scripts/collect_pmc.py",
       "unit_note": "FETCH_SIZE/WRITE_SIZE in KiB; gfx950 FETCH_SIZE counts 64 B per 128 B request for wide coalesced streams "
                    "(MI355X_MICROARCH.md, HBM) so read bytes = FETCH_SIZE*1024*2; WRITE_SIZE*1024 matches the known output size",
       "kernels": kern,
       "mp_kernel": {"name": mp, "read_bytes_per_launch": rd, "write_bytes_per_launch": wr, "hbm_bytes_per_launch": rd + wr,
                     "expected": {"xp": 536870912, "skip_h": 134217728, "out": 134217728}}}
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", f"{tag}_pmc_hbm_cfg3.json")
json.dump(out, open(path, "w"), indent=1)
print(path, json.dumps(out["mp_kernel"]))
