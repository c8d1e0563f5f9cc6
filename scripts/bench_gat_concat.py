#!/usr/bin/env python3
"""Time the gat concat form at config 3's shape (N = 65 536, E = 262 144, B = 2048, H = 4, C = 512), device events, 5 warm-up and
20 timed runs, median [min - max]:
    kernel   gvqa_gat_message_passing_concat alone, and forward + gvqa_gat_mp_backward_concat
    module   gat(512, 512, 512, heads=4, concat=True).eval() forward under no_grad
Prints one JSON line per leg; --out FILE appends them to FILE.

    python scripts/bench_gat_concat.py [--legs kernel,module] [--repo ROOT] [--tag NAME] [--out FILE]

--repo ROOT imports graphvqa_amd from another checkout (with its own built library): the module leg of an older commit, run in a
process of its own, is the baseline of the module's default road (the new median may not exceed the old one by
more than the old min-to-max range).  The kernel leg needs a library that has the concat entry points."""
import argparse
import ctypes as C
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="kernel,module")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="head")
ap.add_argument("--out", default=None)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))

import numpy as np
import torch
from graphvqa_amd import synth, _lib
from graphvqa_amd.graph import SceneGraphBatch, _stream

dev = torch.device("cuda:0")
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
gb = synth.config3_batch()
N, E, B, Cc, H = gb.num_nodes, gb.num_edges, gb.num_graphs, 512, 4
HBM_PEAK = 8e12           # bytes / s, the data sheet's figure


def timed(run):
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_us=1e3 * ms[len(ms) // 2], min_us=1e3 * ms[0], max_us=1e3 * ms[-1], runs=len(ms), warmup=args.warmup)


def emit(rec):
    rec = dict(rec, tag=args.tag, N=N, E=E, B=B, H=H, C=Cc, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


graph = SceneGraphBatch(tt(gb.edge_index), tt(gb.batch), N, B)
gen = torch.Generator(device=dev).manual_seed(5)
rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)

if "kernel" in args.legs.split(","):
    lib = _lib.load()
    xp, a_node, a_edge, bias, dout = rnd(N, H * Cc), rnd(N, 2 * H), rnd(E, H), rnd(H * Cc), rnd(N, H * Cc)
    out, alpha = torch.empty(N, H * Cc, device=dev), torch.empty(E, H, device=dev)
    dxp, da_node, da_edge = torch.empty_like(xp), torch.empty_like(a_node), torch.empty_like(a_edge)
    ws = torch.empty(4 * E * H, dtype=torch.uint8, device=dev)
    st = _stream(dev)
    m = _lib.GatMpDesc()
    m.C, m.H, m.negative_slope = Cc, H, 0.2
    m.xp, m.a_node, m.a_edge, m.bias = xp.data_ptr(), a_node.data_ptr(), a_edge.data_ptr(), bias.data_ptr()
    m.out, m.alpha_out = out.data_ptr(), alpha.data_ptr()
    d = _lib.GatMpBwdDesc()
    d.C, d.H, d.negative_slope = Cc, H, 0.2
    d.xp, d.a_node, d.a_edge, d.alpha, d.dout = xp.data_ptr(), a_node.data_ptr(), a_edge.data_ptr(), alpha.data_ptr(), dout.data_ptr()
    d.dxp, d.da_node, d.da_edge = dxp.data_ptr(), da_node.data_ptr(), da_edge.data_ptr()
    gt = graph.transposed()
    plan = _lib.MpPlan()
    _lib.check(lib.gvqa_gat_mp_plan(C.byref(graph.c), Cc, H, C.byref(plan)))
    fwd = lambda: _lib.check(lib.gvqa_gat_message_passing_concat(C.byref(graph.c), C.byref(m), ws.data_ptr(), ws.numel(), st))
    bwd = lambda: _lib.check(lib.gvqa_gat_mp_backward_concat(C.byref(graph.c), C.byref(gt.c), C.byref(d), st))
    nbytes = 4 * (2 * N * H * Cc + 2 * E * H + 2 * E + N + 1 + H * Cc)
    r = timed(fwd)
    emit(dict(r, leg="kernel_forward", algorithmic_bytes=nbytes, hbm_fraction_of_8TBps=nbytes / (r["median_us"] * 1e-6) / HBM_PEAK,
              tiled=int(plan.tiled), channel_range=int(plan.channel_range), checksum=float(out.double().sum())))
    r = timed(lambda: (fwd(), bwd()))
    emit(dict(r, leg="kernel_forward_backward", checksum=float(dxp.double().sum())))

if "module" in args.legs.split(","):
    from graphvqa_amd.gat_skip import gat
    torch.manual_seed(7)
    conv = gat(Cc, Cc, Cc, heads=H, concat=True).to(dev).eval()
    x, ea, ei = rnd(N, Cc), rnd(E, Cc), tt(gb.edge_index)
    with torch.no_grad():
        res = [None]

        def run():
            res[0] = conv(x, ei, ea, graph=graph)
        r = timed(run)
        emit(dict(r, leg="module_forward_eval", checksum=float(res[0].double().sum())))
