"""lcgn_seq(gat_heads = 4) at BASELINE config 5's shape (config-2 batch, in = 300, O = 512, cmd = 512, L = 10; eval): fp32 node features
against node_feature_dtype = bfloat16 (two weight pieces), one process, device-event times.
  * the two forwards alternate: `--warmup` pairs, then `--pairs` timed pairs; median [min - max] of each;
  * the deviation of the bf16 forward from the fp32 forward of the same weights, in units of the output scale (the config-5-size
    check of the storage mode: tests hold the fp32 forward to the oracle at this shape);
  * torch.cuda.max_memory_allocated of one forward of each;
  * gvqa_lcgn_attention and gvqa_lcgn_attention_bf16 alone on the same operands, alternating, with their algorithmic bytes
        fp32: 4 (3 N HC + 2 B HC + N C_out + E H + 2 E + N + 1)
        bf16: 2 * 3 N HC + 4 * 2 B HC + 2 N C_out + 4 E H + 4 (2 E + N + 1)
    and the share of 8 TB/s they imply.

    python scripts/bench_lcgn_heads_bf16.py [--pairs 20] [--warmup 5] [--out FILE.json]
    python scripts/bench_lcgn_heads_bf16.py --profile        (a few forwards of each, for rocprofv3 --kernel-trace --stats)
scripts/bench_lcgn_heads_bf16.sh runs both under time limits and writes profiles/lcgn_heads_bf16_{bench.json,kernel_stats.csv}.
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
from graphvqa_amd.lcgn import lcgn_seq, lcgn_attention, lcgn_attention_bf16  # noqa: E402

PEAK = 8.0e12
H = 4


def tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def alternate(fa, fb, pairs, warmup):
    """fa and fb in turn; per-call device-event times of the timed pairs -> ([ms of fa], [ms of fb])."""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(pairs)]
    for e in ev:
        e[0].record(); fa(); e[1].record(); fb(); e[2].record()
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1]) for e in ev], [e[1].elapsed_time(e[2]) for e in ev]


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def fmt(s):
    return "%.3f ms [%.3f - %.3f]" % (s["median_ms"], s["min_ms"], s["max_ms"])


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    gb = synth.config2_batch()
    N, E, B, O, L, IN = gb.num_nodes, gb.num_edges, gb.num_graphs, 512, 10, 300
    ei, batch = tt(gb.edge_index, dev), tt(gb.batch, dev)
    g = SceneGraphBatch(ei, batch, N, B)
    x, q, lstm, xc = (tt(synth.normal((N, IN), 1), dev), tt(synth.normal((B, O), 2), dev), tt(synth.normal((L, B, O), 3), dev),
                      tt(synth.normal((N, O), 4), dev))
    params = {k: torch.from_numpy(v) for k, v in synth.lcgn_seq_params(IN, O, seed=808, heads=H).items()}
    mods = {}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        m = lcgn_seq(IN, O, IN, 5, gat_heads=H, node_feature_dtype=dtype)
        m.load_state_dict(params)
        mods[name] = m.to(dev).eval()
    f32 = lambda: mods["fp32"](x, ei, batch, q, lstm, graph=g, x_ctx_init=xc)
    f16 = lambda: mods["bf16"](x, ei, batch, q, lstm, graph=g, x_ctx_init=xc)
    HC = H * O
    J = tt(synth.normal((N, 3 * HC), 12), dev) * 0.05
    J16 = J.bfloat16()
    J = J16.float()                                # the same values for both kernels
    pc = tt(synth.normal((B, 2 * HC), 13), dev) * 0.05
    bias = tt(synth.normal((O,), 14), dev)
    out16 = torch.empty((N, O), dtype=torch.bfloat16, device=dev)
    a32 = lambda: lcgn_attention(J, pc, g, H, O, False, 0.2, bias, want_alpha=True)
    a16 = lambda: lcgn_attention_bf16(J16, pc, g, H, O, False, 0.2, bias, want_alpha=True, out=out16)
    if a.profile:
        for _ in range(3):
            f32(); f16(); a32(); a16()
        torch.cuda.synchronize()
        return
    res = dict(shape=dict(N=N, E=E, B=B, in_channels=IN, out_channels=O, cmd_dim=O, L=L, heads=H), pairs=a.pairs, warmup=a.warmup,
               device=torch.cuda.get_device_name(0))
    o32, o16 = f32(), f16()
    scale = float(o32.abs().max())
    res["bf16_vs_fp32_forward"] = dict(max_abs=float((o16 - o32).abs().max()), scale=scale,
                                       max_abs_over_scale=float((o16 - o32).abs().max()) / scale, finite=bool(torch.isfinite(o16).all()))
    t32, t16 = alternate(f32, f16, a.pairs, a.warmup)
    res["lcgn_seq_h4_fp32"], res["lcgn_seq_h4_bf16"] = stats(t32), stats(t16)
    res["lcgn_seq_h4_fp32"]["peak_bytes"], res["lcgn_seq_h4_bf16"]["peak_bytes"] = peak_bytes(f32), peak_bytes(f16)
    k32, k16 = alternate(a32, a16, a.pairs, a.warmup)
    ref = a32()[0]
    same = float((out16.float() == ref.bfloat16().float()).float().mean())
    csr = 4 * (2 * E + N + 1)
    for name, ms, nbytes in (("attention_h4_fp32", k32, 4 * (3 * N * HC + 2 * B * HC + N * O + E * H) + csr),
                             ("attention_h4_bf16", k16, 2 * 3 * N * HC + 4 * 2 * B * HC + 2 * N * O + 4 * E * H + csr)):
        s = stats(ms)
        s.update(algorithmic_bytes=nbytes, tb_per_s=nbytes / (s["median_ms"] * 1e-3) / 1e12, share_of_8tbs=nbytes / (s["median_ms"] * 1e-3) / PEAK)
        res[name] = s
    res["attention_h4_bf16"]["bit_equal_to_rounded_fp32_kernel"] = same
    print("lcgn_seq(gat_heads=4) forward  fp32 %s   bf16 %s" % (fmt(res["lcgn_seq_h4_fp32"]), fmt(res["lcgn_seq_h4_bf16"])))
    print("peak memory of a forward       fp32 %.0f MB   bf16 %.0f MB" % (res["lcgn_seq_h4_fp32"]["peak_bytes"] / 1e6, res["lcgn_seq_h4_bf16"]["peak_bytes"] / 1e6))
    print("bf16 forward vs fp32 forward   max-abs %.3e = %.3e of the output scale %.3f" %
          (res["bf16_vs_fp32_forward"]["max_abs"], res["bf16_vs_fp32_forward"]["max_abs_over_scale"], scale))
    for name in ("attention_h4_fp32", "attention_h4_bf16"):
        s = res[name]
        print("%s  %s   %.1f MB  %.2f TB/s = %.2f of 8 TB/s" % (name, fmt(s), s["algorithmic_bytes"] / 1e6, s["tb_per_s"], s["share_of_8tbs"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
