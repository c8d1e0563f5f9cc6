"""Multi-head LCGN at BASELINE config 5's shape (config-2 batch, in = 300, O = 512, cmd = 512, L = 10; fp32, eval), device-event times
after warm-up:
  * lcgn_seq forward with gat_heads = 4;
  * the gat_lcgn layer alone (in = 3 O, as inside lcgn_seq; concat = False) for H = 1 and 4;
  * gvqa_lcgn_attention alone on precomputed [x_l | x_r | x_val] / [proj_cmd | cal_cmd] operands for H = 1 and 4, with its algorithmic
    bytes 4 (3 N H C + 2 B H C + N C_out + E H + 2 E + N + 1) and the share of 8 TB/s they imply;
  * lcgn_seq forward with gat_heads = 1 (its per-iteration attention is the k_lcgn_edge_logit_v + GAT message-passing pair: run
    this script under `rocprofv3 --kernel-trace --stats` to set that pair's per-call time beside k_lcgn_attention's).

    python scripts/bench_lcgn_heads.py [--iters 20] [--warmup 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphvqa_amd import synth  # noqa: E402
from graphvqa_amd.graph import SceneGraphBatch  # noqa: E402
from graphvqa_amd.lcgn import gat_lcgn, lcgn_seq, lcgn_attention  # noqa: E402

PEAK = 8.0e12


def tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    gb = synth.config2_batch()
    N, E, B, O, L, IN = gb.num_nodes, gb.num_edges, gb.num_graphs, 512, 10, 300
    ei, batch = tt(gb.edge_index, dev), tt(gb.batch, dev)
    g = SceneGraphBatch(ei, batch, N, B)
    x, q, lstm, xc = (tt(synth.normal((N, IN), 1), dev), tt(synth.normal((B, O), 5), dev), tt(synth.normal((L, B, O), 6), dev),
                      tt(synth.normal((N, O), 7), dev))
    res = dict(shape=dict(N=N, E=E, B=B, in_channels=IN, out_channels=O, cmd_dim=O, L=L), iters=a.iters, warmup=a.warmup,
               device=torch.cuda.get_device_name(0))
    for H in (4, 1):
        m = lcgn_seq(IN, O, IN, 5, gat_heads=H)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.lcgn_seq_params(IN, O, seed=808, heads=H).items()})
        m = m.to(dev).eval()
        res[f"lcgn_seq_h{H}_ms"] = timed(lambda: m(x, ei, batch, q, lstm, graph=g, x_ctx_init=xc), a.iters, a.warmup)
    xj, cmd = tt(synth.normal((N, 3 * O), 8), dev), tt(synth.normal((B, O), 9), dev)
    for H in (1, 4):
        layer = gat_lcgn(3 * O, O, 1, heads=H, concat=False, cmd_dim=O)
        layer.load_state_dict({k: torch.from_numpy(v) for k, v in synth.gat_lcgn_params(3 * O, O, H, 11, O, concat=False).items()})
        layer = layer.to(dev).eval()
        res[f"gat_lcgn_h{H}_ms"] = timed(lambda: layer(xj, ei, cmd, batch, graph=g), a.iters, a.warmup)
        HC = H * O
        J = tt(synth.normal((N, 3 * HC), 12), dev) * 0.05
        pc = tt(synth.normal((B, 2 * HC), 13), dev) * 0.05
        bias = tt(synth.normal((O,), 14), dev)
        ms = timed(lambda: lcgn_attention(J, pc, g, H, O, False, 0.2, bias), a.iters, a.warmup)
        nbytes = 4 * (3 * N * HC + 2 * B * HC + N * O + E * H + 2 * E + N + 1)
        res[f"attention_h{H}"] = dict(ms=ms, algorithmic_bytes=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12,
                                      share_of_8tbs=nbytes / (ms * 1e-3) / PEAK)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
