"""The differentiable LCGN attention (gvqa_lcgn_attention_train / gvqa_lcgn_attention_backward) against the composition it replaces
in training (_lcgn_attention_autograd), at BASELINE config 5's shape (config-2 batch, O = 512), fp32, device-event times:
  * forward + backward of lcgn_attention and of the composition on the same operands, for (H, concat) in (1, False), (4, False),
    (4, True), with and without a dropout mask (p = 0.1): one process, the two roads alternating, `--warmup` pairs then `--pairs`
    timed pairs; median, min and max of each road;
  * the lcgn_seq(gat_heads = 4, dropout = 0.1) training step (forward + backward) the same way, the composition forced through
    graphvqa_amd.lcgn._FORCE_COMPOSITION;
  * the backward alone (new road), with its algorithmic bytes
        4 (3 N HC [J] + N C_out [dout] + 3 E H [alpha; dz written and read] + 3 N HC [dJ] + 4 N HC [per-node rows written and read]
           + 4 B HC [pc, dpc] + 4 E + 3 N + 2 [indices])
    and the share of 8 TB/s they imply.
`--profile`: only a few steps of the new road, for a run under `rocprofv3 --kernel-trace --stats` (bench_lcgn_attention_train.sh).
`--bf16`: the bf16 attention node (gvqa_lcgn_attention_bf16_train / gvqa_lcgn_attention_bf16_backward: J rounded and saved as bf16)
against the fp32 node on J16.float(), the same way: forward + backward for the three (H, concat), with and without a mask; the
backward alone of both with its algorithmic bytes (the bf16 node's: the formula above with the J term halved); and the
lcgn_seq(gat_heads = 4, node_feature_dtype = bfloat16, dropout = 0.1) training step on the bf16 node against the road it replaces
(_StoreBf16, then the fp32 node; reached through _attention_bf16_supported), with each road's peak allocation.

    python scripts/bench_lcgn_attention_train.py [--pairs 20] [--warmup 5] [--out FILE.json] [--profile] [--bf16]
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
from graphvqa_amd import lcgn as L  # noqa: E402
from graphvqa_amd.graph import SceneGraphBatch  # noqa: E402

PEAK = 8.0e12
P_ATT = 0.1


def tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fa, fb, pairs, warmup):
    """fa and fb in turn: (stats of fa, stats of fb) over `pairs` timed pairs after `warmup` untimed ones."""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(pairs):
        ta.append(once(fa))
        tb.append(once(fb))
    st = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    return st(ta), st(tb)


def verdict(new, old):
    """The rule for a default: the new road's median below the composition's by more than the larger min-max range."""
    spread = max(new["max_ms"] - new["min_ms"], old["max_ms"] - old["min_ms"])
    return dict(new=new, composition=old, spread_ms=spread, speedup=old["median_ms"] / new["median_ms"],
                new_is_faster=bool(old["median_ms"] - new["median_ms"] > spread))


def backward_bytes(N, E, B, H, HC, cout, j_bytes):
    """Algorithmic bytes of the backward: J at `j_bytes` per element, everything else fp32 / int32."""
    return j_bytes * 3 * N * HC + 4 * (N * cout + 3 * E * H + 3 * N * HC + 4 * N * HC + 4 * B * HC + 4 * E + 3 * N + 2)


def verdict_bf16(new, old):
    """The acceptance rule of the bf16 road: its median does not exceed the fp32 road's by more than that road's own min-max range."""
    spread = old["max_ms"] - old["min_ms"]
    return dict(bf16=new, fp32=old, fp32_spread_ms=spread, speedup=old["median_ms"] / new["median_ms"],
                bf16_is_no_slower=bool(new["median_ms"] - old["median_ms"] <= spread))


def main_bf16(a):
    dev = torch.device("cuda:0")
    gb = synth.config2_batch()
    N, E, B, O, Lq, IN = gb.num_nodes, gb.num_edges, gb.num_graphs, 512, 10, 300
    ei, batch = tt(gb.edge_index, dev), tt(gb.batch, dev)
    g = SceneGraphBatch(ei, batch, N, B)
    g.transposed()
    res = dict(shape=dict(N=N, E=E, B=B, out_channels=O), pairs=a.pairs, warmup=a.warmup, p_att=P_ATT,
               device=torch.cuda.get_device_name(0), attention={}, backward={})
    for H, concat in ((1, False), (4, False), (4, True)):
        HC = H * O
        cout = HC if concat else O
        # the bf16 values of J as an fp32 leaf: the bf16 node rounds (exactly) and saves bf16, the fp32 node saves the leaf
        J = (tt(synth.normal((N, 3 * HC), 12), dev) * 0.05).bfloat16().float().requires_grad_(True)
        pc = (tt(synth.normal((B, 2 * HC), 13), dev) * 0.05).requires_grad_(True)
        bias = tt(synth.normal((cout,), 14), dev).requires_grad_(True)
        w = tt(synth.normal((N, cout), 15), dev)
        masks = {"": None, "_dropout": torch.bernoulli(torch.full((E, H), 1.0 - P_ATT, device=dev)) / (1.0 - P_ATT)}
        fwd = dict(bf16=lambda mask: L._lcgn_attention_store_bf16(J, pc, g, H, O, concat, 0.2, bias, mask),
                   fp32=lambda mask: L.lcgn_attention(J, pc, g, H, O, concat, 0.2, bias, want_alpha=True, mask=mask))

        def step(road, mask):
            J.grad = pc.grad = bias.grad = None
            out, _ = fwd[road](mask)
            out.backward(w)

        key = f"h{H}_{'concat' if concat else 'mean'}"
        if a.profile:
            for _ in range(3):
                step("bf16", masks["_dropout"])
            torch.cuda.synchronize()
            continue
        for tag, mask in masks.items():
            new, old = alternate(lambda: step("bf16", mask), lambda: step("fp32", mask), a.pairs, a.warmup)
            res["attention"][key + tag] = verdict_bf16(new, old)
        # the backward alone (its kernels + the bias column sum), the two nodes alternating
        outs = {road: fwd[road](masks["_dropout"])[0] for road in fwd}
        bw = {road: (lambda road=road: torch.autograd.grad(outs[road], (J, pc, bias), w, retain_graph=True)) for road in fwd}
        new, old = alternate(bw["bf16"], bw["fp32"], a.pairs, a.warmup)
        for road, st, jb in (("bf16", new, 2), ("fp32", old, 4)):
            nbytes = backward_bytes(N, E, B, H, HC, cout, jb)
            st.update(algorithmic_bytes=nbytes, tb_per_s=nbytes / (st["median_ms"] * 1e-3) / 1e12,
                      share_of_8tbs=nbytes / (st["median_ms"] * 1e-3) / PEAK)
        res["backward"][key] = verdict_bf16(new, old)
        del outs
    if not a.profile:
        H = 4
        m = L.lcgn_seq(IN, O, IN, 5, gat_heads=H, dropout=P_ATT, node_feature_dtype=torch.bfloat16)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.lcgn_seq_params(IN, O, seed=808, heads=H).items()})
        m = m.to(dev).train()
        x, q, lstm, xc, w = (tt(synth.normal((N, IN), 1), dev), tt(synth.normal((B, O), 5), dev), tt(synth.normal((Lq, B, O), 6), dev),
                             tt(synth.normal((N, O), 7), dev), tt(synth.normal((N, O), 8), dev))
        supported = L._attention_bf16_supported

        def seq_step(road):
            m.zero_grad(set_to_none=True)
            L._attention_bf16_supported = supported if road == "bf16" else (lambda heads, channels: False)
            try:
                out = m(x, ei, batch, q, lstm, graph=g, x_ctx_init=xc)
            finally:
                L._attention_bf16_supported = supported
            out.backward(w)

        new, old = alternate(lambda: seq_step("bf16"), lambda: seq_step("fp32"), a.pairs, a.warmup)
        v = verdict_bf16(new, old)
        for road in ("bf16", "fp32"):       # peak allocation of one step of each road, from the same resting state
            m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            seq_step(road)
            torch.cuda.synchronize()
            v[road].update(peak_allocated_bytes=torch.cuda.max_memory_allocated(), resting_allocated_bytes=base)
        v["expected_drop_bytes"] = m.MAX_ITER_NUM * N * 3 * H * O * 2
        v["measured_drop_bytes"] = v["fp32"]["peak_allocated_bytes"] - v["bf16"]["peak_allocated_bytes"]
        res["lcgn_seq_h4_bf16_train_step"] = v
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    a = ap.parse_args()
    if a.bf16:
        return main_bf16(a)
    dev = torch.device("cuda:0")
    gb = synth.config2_batch()
    N, E, B, O, Lq, IN = gb.num_nodes, gb.num_edges, gb.num_graphs, 512, 10, 300
    ei, batch = tt(gb.edge_index, dev), tt(gb.batch, dev)
    g = SceneGraphBatch(ei, batch, N, B)
    g.transposed()
    res = dict(shape=dict(N=N, E=E, B=B, out_channels=O), pairs=a.pairs, warmup=a.warmup, p_att=P_ATT,
               device=torch.cuda.get_device_name(0), attention={}, backward={})
    for H, concat in ((1, False), (4, False), (4, True)):
        HC = H * O
        cout = HC if concat else O
        J = (tt(synth.normal((N, 3 * HC), 12), dev) * 0.05).requires_grad_(True)
        pc = (tt(synth.normal((B, 2 * HC), 13), dev) * 0.05).requires_grad_(True)
        bias = tt(synth.normal((cout,), 14), dev).requires_grad_(True)
        w = tt(synth.normal((N, cout), 15), dev)

        def step(road, p_att):
            J.grad = pc.grad = bias.grad = None
            L._FORCE_COMPOSITION = road == "composition"
            try:
                out, _ = L._attention_train(J, pc, g, H, O, concat, 0.2, bias, p_att)
            finally:
                L._FORCE_COMPOSITION = False
            out.backward(w)

        key = f"h{H}_{'concat' if concat else 'mean'}"
        if a.profile:
            for _ in range(3):
                step("new", P_ATT)
            torch.cuda.synchronize()
            continue
        for tag, p_att in (("", 0.0), ("_dropout", P_ATT)):
            new, old = alternate(lambda: step("new", p_att), lambda: step("composition", p_att), a.pairs, a.warmup)
            res["attention"][key + tag] = verdict(new, old)
        # the backward alone: its kernels + the bias column sum
        out, _ = L.lcgn_attention(J, pc, g, H, O, concat, 0.2, bias)
        bw = lambda: torch.autograd.grad(out, (J, pc, bias), w, retain_graph=True)
        for _ in range(a.warmup):
            bw()
        ts = [once(bw) for _ in range(a.pairs)]
        ms = statistics.median(ts)
        nbytes = 4 * (3 * N * HC + N * cout + 3 * E * H + 3 * N * HC + 4 * N * HC + 4 * B * HC + 4 * E + 3 * N + 2)
        res["backward"][key] = dict(median_ms=ms, min_ms=min(ts), max_ms=max(ts), algorithmic_bytes=nbytes,
                                    tb_per_s=nbytes / (ms * 1e-3) / 1e12, share_of_8tbs=nbytes / (ms * 1e-3) / PEAK)
        del out
    if not a.profile:
        H = 4
        m = L.lcgn_seq(IN, O, IN, 5, gat_heads=H, dropout=P_ATT)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.lcgn_seq_params(IN, O, seed=808, heads=H).items()})
        m = m.to(dev).train()
        x, q, lstm, xc, w = (tt(synth.normal((N, IN), 1), dev), tt(synth.normal((B, O), 5), dev), tt(synth.normal((Lq, B, O), 6), dev),
                             tt(synth.normal((N, O), 7), dev), tt(synth.normal((N, O), 8), dev))

        def seq_step(road):
            m.zero_grad(set_to_none=True)
            L._FORCE_COMPOSITION = road == "composition"
            try:
                out = m(x, ei, batch, q, lstm, graph=g, x_ctx_init=xc)
            finally:
                L._FORCE_COMPOSITION = False
            out.backward(w)

        new, old = alternate(lambda: seq_step("new"), lambda: seq_step("composition"), a.pairs, a.warmup)
        res["lcgn_seq_h4_train_step"] = verdict(new, old)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
