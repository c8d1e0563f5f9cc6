#!/usr/bin/env python3
"""Generate tests/golden/lcgn_heads_small.npz by running the REFERENCE'S OWN `gat_lcgn` and `lcgn_seq` with several heads.

Build-container only (needs the reference checkout, see make_golden.py).  Run as:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lcgn_heads.py

Same recipe as make_golden.py (whose helpers it imports): the reference's lcgn.py unmodified on top of `oracle/pyg_shim`,
parameters and inputs from `graphvqa_amd.synth` (pure functions of integer seeds), CPU fp32 forward, plain arrays stored:
  * the layer, H in {1, 2, 4, 8} x concat in {False, True}, out and alpha, on synth.lcgn_test_batch (multi-edges, an empty
    graph, a node without in-edges) and on its cross-graph form (three edges between graphs);
  * lcgn_seq(gat_heads = H), H in {2, 4}, on the same intra-graph batch.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets sys.path to the shim, the reference and the repo; fixes the thread count)
import torch  # noqa: E402

from graphvqa_amd import synth  # noqa: E402

IN, C, CMD, BATCH_SEED, PARAM_SEED = 12, 8, 16, 5, 808
SEQ_IN, SEQ_O, SEQ_L, SEQ_SEED, TORCH_SEED = 12, 8, 6, 909, 4321
SEEDS = dict(x=51, cmd=52, q=53, lstm=54, seq_x=55)


def main():
    import lcgn

    gb, gx = synth.lcgn_test_batch(BATCH_SEED), synth.lcgn_test_batch(BATCH_SEED, cross_graph=True)
    N, B = gb.num_nodes, gb.num_graphs
    x, cmd = MG.t(synth.normal((N, IN), SEEDS["x"])), MG.t(synth.normal((B, CMD), SEEDS["cmd"]))
    arrays = dict(edge_index=gb.edge_index, batch=gb.batch, x_edge_index=gx.edge_index)
    for H in (1, 2, 4, 8):
        for concat in (False, True):
            m = lcgn.gat_lcgn(in_channels=IN, out_channels=C, edge_in_channels=1, heads=H, concat=concat, negative_slope=0.2,
                              dropout=0.1, cmd_dim=CMD)
            MG.load_params(m, synth.gat_lcgn_params(IN, C, H, PARAM_SEED + H, CMD, concat=concat))
            for tag, g in (("layer", gb), ("xlayer", gx)):
                with torch.no_grad():
                    out, (_, alpha) = m(x, MG.t(g.edge_index), cmd, MG.t(g.batch), return_attention_weights=True)
                arrays[f"{tag}_h{H}_c{int(concat)}_out"] = out
                arrays[f"{tag}_h{H}_c{int(concat)}_alpha"] = alpha
    xs = MG.t(synth.normal((N, SEQ_IN), SEEDS["seq_x"]))
    q, lstm = MG.t(synth.normal((B, SEQ_O), SEEDS["q"])), MG.t(synth.normal((SEQ_L, B, SEQ_O), SEEDS["lstm"]))
    torch.manual_seed(TORCH_SEED)
    arrays["seq_x_ctx_init"] = torch.randn(N, SEQ_O)              # the draw lcgn.py:306 will make
    for H in (2, 4):
        m = lcgn.lcgn_seq(in_channels=SEQ_IN, out_channels=SEQ_O, edge_attr_dim=SEQ_IN, num_ins=5, gat_cmd_dim=SEQ_O,
                          question_dim=SEQ_O, MAX_ITER_NUM=4, dropout=0.1, gat_heads=H)
        MG.load_params(m, synth.lcgn_seq_params(SEQ_IN, SEQ_O, seed=SEQ_SEED + H, cmd_dim=SEQ_O, question_dim=SEQ_O, heads=H))
        torch.manual_seed(TORCH_SEED)
        with torch.no_grad():
            arrays[f"seq_h{H}_out"] = m(xs, MG.t(gb.edge_index), MG.t(gb.batch), q, lstm)
    MG.save("lcgn_heads_small", dict(case="gat_lcgn.forward / lcgn_seq.forward eval, several heads", ref="lcgn.py:63-323",
                                     in_channels=IN, out_channels=C, cmd_dim=CMD, batch_seed=BATCH_SEED, param_seed=PARAM_SEED,
                                     seq=dict(in_channels=SEQ_IN, out_channels=SEQ_O, L=SEQ_L, param_seed=SEQ_SEED,
                                              torch_seed=TORCH_SEED),
                                     input_seeds=SEEDS, negative_slope=0.2), **arrays)


if __name__ == "__main__":
    main()
