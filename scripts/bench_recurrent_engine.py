#!/usr/bin/env python3
"""RecurrentExecutionEngine and its neighbour-mean op (graphvqa_amd/recurrent_engine.py) on the GPU: device-event times on the current
stream, `--warmup` untimed runs then `--reps` timed ones per leg, the legs of one comparison alternating in one process.  ONE JSON line on
stdout and, with --out, in a file (profiles/recurrent_engine_bench.json).  Batches: synth.config2_batch() and synth.config3_batch() (the
graphs of configs 2 and 3), D = 300, Di = 512.

  * op    : `neighbor_mean` (fused: one CSR gather-reduce per direction) against the composed road (`edge_gather`, `edge_scatter_add`,
            `bincount().clamp(min=1)`, a divide) at F = 300: the forward under no_grad and forward + backward, median / min / max per leg;
            the fused forward's and backward's fraction of 8 TB/s on 4 (2 N F + E + N + 1) bytes (every row read once and written once,
            the CSR read once); and the wiring rule of DESIGN.md 4b: fused median <= composed median + the composed road's own range;
  * module: forward (no_grad) and the training step (forward + backward) of RecurrentExecutionEngine(300, 512) on the op and with
            recurrent_engine._FORCE_COMPOSED_MEAN.

    python scripts/bench_recurrent_engine.py [--reps 20] [--warmup 5] [--out FILE.json] [--only op,module]
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
from graphvqa_amd import recurrent_engine as RE  # noqa: E402
from graphvqa_amd.gat_skip import edge_gather, edge_scatter_add  # noqa: E402
from graphvqa_amd.graph import SceneGraphBatch  # noqa: E402

SHAPES = (("config2", synth.config2_batch), ("config3", synth.config3_batch))
D, DI, HBM_TBPS = 300, 512, 8.0


def tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def composed(x, graph):
    cnt = torch.bincount(graph._keep[0][1], minlength=graph.num_nodes).clamp(min=1).to(x.dtype)
    return edge_scatter_add(edge_gather(x, graph, "src"), graph) / cnt.view(-1, 1)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup):
    """the legs in turn: per leg median / min / max (ms) over `reps` timed runs after `warmup` untimed ones."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(once(f))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ts.items()}


def rule(r, fused, comp):
    """the fused leg is wired when its median is <= the composed median + the composed leg's own min-to-max range."""
    limit = r[comp]["median_ms"] + (r[comp]["max_ms"] - r[comp]["min_ms"])
    return dict(fused_median_ms=r[fused]["median_ms"], limit_ms=limit, holds=bool(r[fused]["median_ms"] <= limit),
                speedup=r[comp]["median_ms"] / r[fused]["median_ms"])


def bench_op(dev, a):
    res = {}
    for name, make in SHAPES:
        gb = make()
        N, E, B = gb.num_nodes, gb.num_edges, gb.num_graphs
        graph = SceneGraphBatch(tt(gb.edge_index, dev), tt(gb.batch, dev), N, B)
        graph.transposed()                                 # (a batch's handles are built once; not part of a step)
        x, dout = tt(synth.normal((N, D), 1), dev).requires_grad_(True), tt(synth.normal((N, D), 2), dev)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(x, graph)
            return run

        def fwd_bwd(fn):
            def run():
                x.grad = None
                fn(x, graph).backward(dout)
            return run
        r = alternate({"fused_fwd": fwd(RE.neighbor_mean), "composed_fwd": fwd(composed), "fused_fwd_bwd": fwd_bwd(RE.neighbor_mean),
                       "composed_fwd_bwd": fwd_bwd(composed)}, a.reps, a.warmup)
        out = RE.neighbor_mean(x, graph)
        r.update(alternate({"fused_bwd_only": lambda: torch.autograd.grad(out, x, dout, retain_graph=True)}, a.reps, a.warmup))
        nbytes = 4 * (2 * N * D + E + N + 1)
        res[name] = dict(N=N, E=E, B=B, F=D, times=r, rule_fwd=rule(r, "fused_fwd", "composed_fwd"),
                         rule_fwd_bwd=rule(r, "fused_fwd_bwd", "composed_fwd_bwd"), bytes_per_direction=nbytes,
                         fwd_fraction_of_8TBps=nbytes / (r["fused_fwd"]["median_ms"] * 1e-3) / 1e12 / HBM_TBPS,
                         bwd_fraction_of_8TBps=nbytes / (r["fused_bwd_only"]["median_ms"] * 1e-3) / 1e12 / HBM_TBPS)
    return res


def bench_module(dev, a):
    res = {}
    for name, make in SHAPES:
        gb = make()
        N, E, B = gb.num_nodes, gb.num_edges, gb.num_graphs
        torch.manual_seed(7)
        m = RE.RecurrentExecutionEngine(D, DI).to(dev)
        ei, batch = tt(gb.edge_index, dev), tt(gb.batch, dev)
        graph = SceneGraphBatch(ei, batch, N, B)
        graph.transposed()
        x, ins = tt(synth.normal((N, D), 3), dev).requires_grad_(True), tt(synth.normal((5, B, DI), 4), dev).requires_grad_(True)
        wb, wh = tt(synth.normal((N, 5), 5), dev), tt(synth.normal((5, B, DI), 6), dev)

        def fwd(force):
            def run():
                RE._FORCE_COMPOSED_MEAN = force
                with torch.no_grad():
                    m(x, ei, None, ins, batch, graph=graph)
            return run

        def step(force):
            def run():
                RE._FORCE_COMPOSED_MEAN = force
                x.grad = ins.grad = None
                for p in m.parameters():
                    p.grad = None
                _, bitmap, hv = m(x, ei, None, ins, batch, graph=graph)
                ((bitmap * wb).sum() + (hv * wh).sum()).backward()
            return run
        try:
            r = alternate({"fused_fwd": fwd(False), "composed_fwd": fwd(True), "fused_fwd_bwd": step(False), "composed_fwd_bwd": step(True)},
                          a.reps, a.warmup)
        finally:
            RE._FORCE_COMPOSED_MEAN = False
        res[name] = dict(N=N, E=E, B=B, D=D, Di=DI, times=r, rule_fwd=rule(r, "fused_fwd", "composed_fwd"),
                         rule_fwd_bwd=rule(r, "fused_fwd_bwd", "composed_fwd_bwd"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="op,module")
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 5, "at least 5 warm-ups and 20 timed iterations"
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(0)
    arch = getattr(pr, "gcnArchName", "").split(":")[0]
    box = f"{'AMD Instinct MI355X' if arch == 'gfx950' else 'not an MI355X'} ({arch or 'arch unknown'}, {pr.multi_processor_count} CUs; torch reports '{pr.name}')"
    d = dict(bench="recurrent_engine", box=box, clock="hip events on the current stream", reps=a.reps, warmup=a.warmup, legs="alternating")
    for k, f in (("op", bench_op), ("module", bench_module)):
        if k in a.only.split(","):
            d[k] = f(dev, a)
    line = json.dumps(d)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
