#!/usr/bin/env python3
"""The table gradient of the encoder's token-embedding sums (graphvqa_amd/sg_encoder.py `embed_sum`) on the GPU: the HIP road
(gvqa_embed_sum_backward: counting sort + segmented sum) against the torch road (the row gradients repeated per token into a
[rows T, D] tensor, torch's sort-based embedding_dense_backward), backward call only, one process, the roads alternating, `--warmup`
untimed pairs then `--reps` timed ones, device events; median [min - max] per road and the peak of torch.cuda.max_memory_allocated above
the level before the call.

Sizes: config 3's node call (rows = 65 536, T = 12, pad id ignored) and edge call (rows = 262 144, T = 1, every seventh row negated, on
the projected table: nothing ignored), V = 3000, D = 300.  Token sets: `uniform` (bench_pipeline_train.py's), and `gqa` -- 1-4 real
tokens per node row and then pad, one edge token on a quarter of the edges, the rest Zipf-like (p ~ 1 / rank).

The torch road timed here is the one in the tree (`_FORCE_TORCH_EMBED_BACKWARD`: ids clamped, `padding_idx = ignore_index` passed to
embedding_dense_backward), the road of vocabularies the kernels do not take -- not the code of the commit before `embed_sum`, which passed
-1 and zeroed the pad row in a second op.

The rule the encoder's default follows: the HIP road is taken when, on both token sets and both calls, its median does not exceed the
torch road's by more than the torch road's own min-to-max range.  One JSON document on stdout and, with --out, in a file.

    python scripts/bench_embed_backward.py [--reps 20] [--warmup 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphvqa_amd import synth  # noqa: E402
from graphvqa_amd import sg_encoder as SG  # noqa: E402

V, D, PAD, SELF = 3000, 300, 0, 3


def tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def zipf(rng, n, lo, hi):
    ids = np.arange(lo, hi)
    p = 1.0 / np.arange(1, ids.size + 1)
    return rng.choice(ids, size=n, p=p / p.sum()).astype(np.int64)


def token_sets(N, E):
    rng = np.random.default_rng(2024)
    k = rng.integers(1, 5, N)
    gx = zipf(rng, N * 12, 1, V).reshape(N, 12)
    gx[np.arange(12)[None, :] >= k[:, None]] = PAD
    ge = zipf(rng, E, 4, V)
    ge[rng.permutation(E)[: E // 4]] = SELF
    return {"uniform": (synth.randint(N * 12, 71, 0, V, stream=9).reshape(N, 12), synth.randint(E, 72, 1, V, stream=9).reshape(E, 1)),
            "gqa": (gx, ge.reshape(E, 1))}


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(once(f))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ts.items()}


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def roads(tokens, table, negate, ignore, dout):
    out = SG.embed_sum(tokens, table, negate, ignore)

    def road(force):
        def run():
            SG._FORCE_TORCH_EMBED_BACKWARD = force
            try:
                return torch.autograd.grad(out, table, dout, retain_graph=True)[0]
            finally:
                SG._FORCE_TORCH_EMBED_BACKWARD = False
        return run
    return {"hip": road(False), "torch": road(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(0)
    arch = getattr(pr, "gcnArchName", "").split(":")[0]
    gb = synth.config3_batch()
    N, E = gb.num_nodes, gb.num_edges
    doc = dict(box=f"{'AMD Instinct MI355X' if arch == 'gfx950' else 'not an MI355X'} ({arch or 'arch unknown'}, {pr.multi_processor_count} CUs)",
               clock="hip events on the current stream, backward call only", reps=a.reps, warmup=a.warmup, V=V, D=D, results=[])
    table = tt(synth.normal((V, D), 1), dev).requires_grad_(True)
    negate = torch.zeros(E, dtype=torch.uint8, device=dev)
    negate[::7] = 1
    wins = True
    for name, (x_tok, e_tok) in token_sets(N, E).items():
        for call, tok, neg, ignore in (("node", x_tok, None, PAD), ("edge", e_tok, negate, None)):
            tokens = tt(tok, dev)
            dout = tt(synth.normal((tok.shape[0], D), 2), dev)
            fns = roads(tokens, table, neg, ignore, dout)
            agree = float((fns["hip"]() - fns["torch"]()).abs().max())
            r = alternate(fns, a.reps, a.warmup)
            peak = {k: peak_above(f) for k, f in fns.items()}
            slack = r["torch"]["max_ms"] - r["torch"]["min_ms"]
            ok = r["hip"]["median_ms"] <= r["torch"]["median_ms"] + slack
            wins = wins and ok
            flat = np.clip(tok.reshape(-1), 0, V - 1)
            kept = flat[flat != ignore] if ignore is not None else flat
            doc["results"].append(dict(tokens=name, call=call, rows=int(tok.shape[0]), T=int(tok.shape[1]), ignore_index=ignore,
                                       kept_occurrences=int(kept.size), heaviest_token_count=int(np.bincount(kept).max()), times=r,
                                       peak_bytes_above_start=peak, torch_over_hip=r["torch"]["median_ms"] / r["hip"]["median_ms"],
                                       hip_within_rule=bool(ok), max_abs_difference_of_the_roads=agree))
    doc["hip_road_is_default"] = bool(wins)
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
