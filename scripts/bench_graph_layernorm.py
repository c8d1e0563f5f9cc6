#!/usr/bin/env python3
"""Graph LayerNorm (graphvqa_amd/graph_layernorm.py) on the GPU, device-event times on the current stream, `--warmup` untimed runs then the
median of `--reps`; the roads of one comparison alternate in one process.  JSON lines on stdout and, with --out, in a file:

  * op     : forward and forward + backward of `graph_layernorm` against the composed formulation it replaces in the encoder's training
             path (two graph_segment_sum, two graph_rows, subtract, square, sqrt, divide, affine under torch autograd -- `composed` below),
             at config-3 size (2048 graphs x 32 nodes, D = 512) and config-2 size (1000 graphs of 20-40 nodes, D = 300), with the
             algorithmic bytes (forward: one read + one write of [N, D]; backward: two reads + one write) and the rate they imply;
  * encoder: the encoder's training step (forward + backward) at config-2 size with the fused op and with `composed` in its place;
  * cross  : one-graph batches of 64 ... 65536 nodes at D = 512, forward and forward + backward, kernel form 1 (one workgroup per graph)
             against form 2 (split): where the auto rule's threshold comes from.

    python scripts/bench_graph_layernorm.py [--reps 20] [--warmup 5] [--out FILE.jsonl] [--only op,encoder,cross]
"""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphvqa_amd import synth  # noqa: E402
from graphvqa_amd import sg_encoder as SG  # noqa: E402
from graphvqa_amd.gat_skip import graph_rows, graph_segment_sum  # noqa: E402
from graphvqa_amd.graph import SceneGraphBatch  # noqa: E402
from graphvqa_amd.graph_layernorm import graph_layernorm  # noqa: E402


def tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def composed(x2, graph, weight, bias, eps=1e-5, _form=None):
    """The encoder's training-path formulation before the fused op: per-graph reductions / broadcasts on the HIP per-graph ops, the rest
    torch element-wise ops, all under autograd."""
    D = x2.shape[1]
    gp = graph.graph_ptr.long()
    norm = ((gp[1:] - gp[:-1]).clamp(min=1) * D).to(x2.dtype).view(-1, 1)
    mean = graph_segment_sum(x2, graph).sum(dim=-1, keepdim=True) / norm
    xc = x2 - graph_rows(mean, graph)
    var = graph_segment_sum(xc * xc, graph).sum(dim=-1, keepdim=True) / norm
    out = xc / (graph_rows(var.sqrt(), graph) + eps)
    return out * weight + bias


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warmup):
    """the roads in turn: per road median / min / max (ms) over `reps` timed runs after `warmup` untimed ones."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(once(f))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ts.items()}


def op_roads(x, dout, graph, w, b, fn, form=None):
    def fwd():
        with torch.no_grad():
            fn(x, graph, w, b, 1e-5, _form=form)

    def fwd_bwd():
        x.grad = w.grad = b.grad = None
        (fn(x, graph, w, b, 1e-5, _form=form) * dout).sum().backward()       # (the product and the sum are part of both roads)
    return fwd, fwd_bwd


def bench_op(dev, emit, a):
    for name, gb, D in (("config3", synth.config3_batch(), 512), ("config2", synth.config2_batch(), 300)):
        N, B = gb.num_nodes, gb.num_graphs
        graph = SceneGraphBatch(tt(gb.edge_index, dev), tt(gb.batch, dev), N, B)
        x, dout = tt(synth.normal((N, D), 1), dev).requires_grad_(True), tt(synth.normal((N, D), 2), dev)
        w, b = torch.tensor([1.3], device=dev, requires_grad=True), torch.tensor([-0.2], device=dev, requires_grad=True)
        ff, fb = op_roads(x, dout, graph, w, b, graph_layernorm)
        cf, cb = op_roads(x, dout, graph, w, b, composed)
        r = alternate({"fused_fwd": ff, "composed_fwd": cf, "fused_fwd_bwd": fb, "composed_fwd_bwd": cb}, a.reps, a.warmup)
        # the backward call alone: forward once, then time autograd.grad on the retained graph
        out = graph_layernorm(x, graph, w, b, 1e-5)
        r.update(alternate({"fused_bwd_only": lambda: torch.autograd.grad(out, (x, w, b), dout, retain_graph=True)}, a.reps, a.warmup))
        nd = 4 * N * D
        emit(dict(kind="op", shape=name, N=N, B=B, D=D, times=r, fwd_bytes=2 * nd, bwd_bytes=3 * nd,
                  fwd_TBps=2 * nd / (r["fused_fwd"]["median_ms"] * 1e-3) / 1e12, bwd_TBps=3 * nd / (r["fused_bwd_only"]["median_ms"] * 1e-3) / 1e12,
                  speedup_fwd=r["composed_fwd"]["median_ms"] / r["fused_fwd"]["median_ms"],
                  speedup_fwd_bwd=r["composed_fwd_bwd"]["median_ms"] / r["fused_fwd_bwd"]["median_ms"]))


def bench_encoder(dev, emit, a):
    gb = synth.config2_batch()
    N, E, B, V, D = gb.num_nodes, gb.num_edges, gb.num_graphs, 3000, 300
    enc = SG.GroundTruth_SceneGraph_Encoder(V, 0, D)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.encoder_params(V, D, seed=1).items()})
    enc.to(dev).train()
    enc.validate_ids = "first"
    data = types.SimpleNamespace(x=tt(synth.randint(N * 12, 71, 0, V, stream=9).reshape(N, 12), dev),
                                 edge_attr=tt(synth.randint(E, 72, 1, V, stream=9).reshape(E, 1), dev), edge_index=tt(gb.edge_index, dev),
                                 batch=tt(gb.batch, dev), added_sym_edge=tt(np.arange(0, E, 7, dtype=np.int64), dev))
    g = SceneGraphBatch(data.edge_index, data.batch, N, B)
    g.transposed()

    def step(fn):
        def run():
            SG.graph_layernorm = fn
            for p in enc.parameters():
                p.grad = None
            xe, ee, _ = enc(data, graph=g)
            (xe.square().mean() + ee.square().mean()).backward()
        return run
    try:
        r = alternate({"fused": step(graph_layernorm), "composed": step(composed)}, a.reps, a.warmup)
    finally:
        SG.graph_layernorm = graph_layernorm
    emit(dict(kind="encoder_train_step", shape="config2", N=N, E=E, B=B, D=D, times=r,
              speedup=r["composed"]["median_ms"] / r["fused"]["median_ms"]))


def bench_cross(dev, emit, a):
    D = 512
    for n in (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
        graph = SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=dev), None, n, 1)
        x, dout = tt(synth.normal((n, D), 3), dev).requires_grad_(True), tt(synth.normal((n, D), 4), dev)
        w, b = torch.tensor([1.3], device=dev, requires_grad=True), torch.tensor([-0.2], device=dev, requires_grad=True)
        f1, b1 = op_roads(x, dout, graph, w, b, graph_layernorm, 1)
        f2, b2 = op_roads(x, dout, graph, w, b, graph_layernorm, 2)
        r = alternate({"form1_fwd": f1, "form2_fwd": f2, "form1_fwd_bwd": b1, "form2_fwd_bwd": b2}, a.reps, a.warmup)
        emit(dict(kind="crossover", nodes=n, D=D, elements=n * D, times={k: v["median_ms"] for k, v in r.items()},
                  form2_over_form1_fwd=r["form2_fwd"]["median_ms"] / r["form1_fwd"]["median_ms"],
                  form2_over_form1_fwd_bwd=r["form2_fwd_bwd"]["median_ms"] / r["form1_fwd_bwd"]["median_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="op,encoder,cross")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = open(a.out, "w") if a.out else None
    pr = torch.cuda.get_device_properties(0)
    arch = getattr(pr, "gcnArchName", "").split(":")[0]
    box = f"{'AMD Instinct MI355X' if arch == 'gfx950' else 'not an MI355X'} ({arch or 'arch unknown'}, {pr.multi_processor_count} CUs; torch reports '{pr.name}')"

    def emit(d):
        d = dict(d, box=box, clock="hip events on the current stream", reps=a.reps, warmup=a.warmup)
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for k, f in (("op", bench_op), ("encoder", bench_encoder), ("cross", bench_cross)):
        if k in a.only.split(","):
            f(dev, emit, a)


if __name__ == "__main__":
    main()
