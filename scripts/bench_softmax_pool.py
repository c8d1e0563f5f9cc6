#!/usr/bin/env python3
"""Global attention pooling (graphvqa_amd/global_attention.py) on the GPU: device-event times on the current stream, `--warmup` untimed
runs then `--reps` timed ones per leg, the legs of one comparison alternating in one process.  ONE JSON line on stdout and, with --out, in
a file (profiles/softmax_pool_bench.json):

  * op    : forward + backward of `graph_attention_pool` (fused) against the composed road it replaces in the pooling module's training
            path (`graph_softmax`, `gate * x`, `graph_segment_sum` under torch autograd), at config 2's pooling size
            (synth.config2_batch(), C = 512) and config 3's (2048 graphs x 32 nodes, C = 512): median / min / max per leg, the algorithmic
            bytes (x read once in each direction, dx written once) and the rate they imply, and the wiring rule of DESIGN.md 4b:
            fused median <= composed median + the composed road's own min-to-max range;
  * module: the training step (forward + backward) of MyConditionalGlobalAttention(300, 512) at both sizes with the fused op and with
            pipeline_head._FORCE_COMPOSED_POOL;
  * sweep : one graph of 32 / 64 / 128 / 256 / 1024 / 4096 / 16384 nodes at C = 512, forward + backward, kernel form 1 (one workgroup per graph) against
            form 2 (split): where the auto rule's threshold comes from.

    python scripts/bench_softmax_pool.py [--reps 20] [--warmup 5] [--out FILE.json] [--only op,module,sweep]
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
from graphvqa_amd import pipeline_head as PH  # noqa: E402
from graphvqa_amd.gat_skip import graph_segment_sum, graph_softmax  # noqa: E402
from graphvqa_amd.global_attention import graph_attention_pool, graph_attention_pool_form  # noqa: E402
from graphvqa_amd.graph import SceneGraphBatch  # noqa: E402

SHAPES = (("config2", synth.config2_batch), ("config3", synth.config3_batch))


def tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def composed(score, x, graph, _form=None):
    gate = graph_softmax(score, graph)
    return graph_segment_sum(gate * x, graph)


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


def rule(r, fused="fused", comp="composed"):
    """the fused leg is wired when its median is <= the composed median + the composed leg's own min-to-max range."""
    limit = r[comp]["median_ms"] + (r[comp]["max_ms"] - r[comp]["min_ms"])
    return dict(fused_median_ms=r[fused]["median_ms"], limit_ms=limit, holds=bool(r[fused]["median_ms"] <= limit),
                speedup=r[comp]["median_ms"] / r[fused]["median_ms"])


def fwd_bwd(fn, score, x, dout, graph, form=None):
    def run():
        score.grad = x.grad = None
        (fn(score, x, graph, _form=form) * dout).sum().backward()       # (the product and the sum are part of every leg)
    return run


def bench_op(dev, a):
    res = {}
    for name, make in SHAPES:
        gb = make()
        N, B, Cw = gb.num_nodes, gb.num_graphs, 512
        graph = SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=dev), tt(gb.batch, dev), N, B)
        score, x = tt(synth.normal((N, 1), 1), dev).requires_grad_(True), tt(synth.normal((N, Cw), 2), dev).requires_grad_(True)
        dout = tt(synth.normal((B, Cw), 3), dev)
        r = alternate({"fused": fwd_bwd(graph_attention_pool, score, x, dout, graph), "composed": fwd_bwd(composed, score, x, dout, graph)}, a.reps, a.warmup)
        # the two calls alone: the forward under no_grad, the backward by autograd.grad on a retained graph
        out = graph_attention_pool(score, x, graph)

        def fwd_only():
            with torch.no_grad():
                graph_attention_pool(score, x, graph)
        r.update(alternate({"fused_fwd_only": fwd_only, "fused_bwd_only": lambda: torch.autograd.grad(out, (score, x), dout, retain_graph=True)}, a.reps, a.warmup))
        nc = 4 * N * Cw
        res[name] = dict(N=N, B=B, C=Cw, form=graph_attention_pool_form(graph, Cw), times=r, rule=rule(r), fwd_bytes=nc, bwd_bytes=2 * nc,
                         fwd_TBps=nc / (r["fused_fwd_only"]["median_ms"] * 1e-3) / 1e12,
                         bwd_TBps=2 * nc / (r["fused_bwd_only"]["median_ms"] * 1e-3) / 1e12)
    return res


def bench_module(dev, a):
    res = {}
    for name, make in SHAPES:
        gb = make()
        N, B, Dn, Cw = gb.num_nodes, gb.num_graphs, 300, 512
        pool = PH.MyConditionalGlobalAttention(Dn, Cw)
        pool.load_state_dict({k: torch.from_numpy(v) for k, v in synth.attention_pool_params(Dn, Cw, seed=811).items()})
        pool.to(dev).train()
        graph = SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=dev), tt(gb.batch, dev), N, B)
        x, u, w = tt(synth.normal((N, Dn), 4), dev).requires_grad_(True), tt(synth.normal((B, Cw), 5), dev).requires_grad_(True), tt(synth.normal((B, Cw), 6), dev)
        batch = tt(gb.batch, dev)

        def step(force):
            def run():
                PH._FORCE_COMPOSED_POOL = force
                x.grad = u.grad = None
                for p in pool.parameters():
                    p.grad = None
                (pool(x, u, batch, graph=graph) * w).sum().backward()
            return run
        try:
            r = alternate({"fused": step(False), "composed": step(True)}, a.reps, a.warmup)
        finally:
            PH._FORCE_COMPOSED_POOL = False
        res[name] = dict(N=N, B=B, Dn=Dn, C=Cw, times=r, rule=rule(r))
    return res


def bench_sweep(dev, a):
    res, Cw = [], 512
    for n in (32, 64, 128, 256, 1024, 4096, 16384):
        graph = SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=dev), None, n, 1)
        score, x = tt(synth.normal((n, 1), 7), dev).requires_grad_(True), tt(synth.normal((n, Cw), 8), dev).requires_grad_(True)
        dout = tt(synth.normal((1, Cw), 9), dev)
        r = alternate({"form1": fwd_bwd(graph_attention_pool, score, x, dout, graph, 1), "form2": fwd_bwd(graph_attention_pool, score, x, dout, graph, 2)},
                      a.reps, a.warmup)
        res.append(dict(nodes=n, C=Cw, elements=n * Cw, auto_form=graph_attention_pool_form(graph, Cw), times=r,
                        form1_not_slower=bool(r["form1"]["median_ms"] <= r["form2"]["median_ms"]),
                        form2_over_form1=r["form2"]["median_ms"] / r["form1"]["median_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="op,module,sweep")
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 5, "at least 5 warm-ups and 20 timed iterations"
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(0)
    arch = getattr(pr, "gcnArchName", "").split(":")[0]
    box = f"{'AMD Instinct MI355X' if arch == 'gfx950' else 'not an MI355X'} ({arch or 'arch unknown'}, {pr.multi_processor_count} CUs; torch reports '{pr.name}')"
    d = dict(bench="softmax_pool", box=box, clock="hip events on the current stream", reps=a.reps, warmup=a.warmup, legs="alternating, forward + backward")
    for k, f in (("op", bench_op), ("module", bench_module), ("sweep", bench_sweep)):
        if k in a.only.split(","):
            d[k] = f(dev, a)
    line = json.dumps(d)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
