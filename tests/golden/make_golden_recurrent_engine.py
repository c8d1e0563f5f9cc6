#!/usr/bin/env python3
"""Generate tests/golden/recurrent_engine_small.npz by running the REFERENCE'S OWN `RecurrentExecutionEngine` (pipeline_model_gat.py:194-288).

Build-container only (needs the reference checkout, see make_golden.py).  Run as:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_recurrent_engine.py

Same recipe as make_golden_softmax_pool.py: the reference's class unmodified on top of `oracle/pyg_shim`, the dataset entry stubbed
(MAX_EXECUTION_STEP = 5), inputs and weights from `graphvqa_amd.synth` (pure functions of integer seeds), CPU fp32 forward and the
reference's own autograd for loss = sum(execution_bitmap * dB) + sum(history_vectors * dH).  The per-step LayerNorm outputs are captured
with a forward hook on `graph_layer_norm`.  Plain arrays stored: the inputs, every parameter (`p_<key>`), the three outputs, `ln_steps`
[5, N, D], and the gradients of x, instr_vectors and every parameter (`d_<key>`).

Graphs of [1, 6, 21, 40, 12, 3] nodes at D = 12, Di = 8: the 1-node graph has only its self-loop, the 3-node graph no edge at all (it is
the LAST graph, so the reference's `dim_size=None` still yields all six rows: its nodes exist), every other graph a self-loop on every node
but one plus 2 n seeded random directed intra-graph edges (duplicates allowed); all edges into node 17 of the 40-node graph are removed.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets sys.path to the shim, the reference and the repo; fixes the thread count)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphvqa_amd import synth  # noqa: E402

SIZES, D, DI, STEPS = [1, 6, 21, 40, 12, 3], 12, 8, 5
NO_LOOP = {1: 4, 2: 0, 3: 39, 4: 7}            # graph -> the local node without a self-loop
NO_IN_EDGE = (3, 17)                           # (graph, local node) whose in-edges are all removed
SEEDS = dict(x=91, instr=92, dB=93, dH=94, edges=95, params=960, ln=99)


def edges():
    off = np.concatenate([[0], np.cumsum(SIZES)])
    src, dst = [], []
    for g, n in enumerate(SIZES):
        if g == 0:
            s, d = np.array([0]), np.array([0])
        elif g == len(SIZES) - 1:
            continue
        else:
            loops = np.array([i for i in range(n) if i != NO_LOOP[g]])
            s = np.concatenate([loops, synth.randint(2 * n, SEEDS["edges"] + g, 0, n, stream=7)])
            d = np.concatenate([loops, synth.randint(2 * n, SEEDS["edges"] + g, 0, n, stream=8)])
            if g == NO_IN_EDGE[0]:
                keep = d != NO_IN_EDGE[1]
                s, d = s[keep], d[keep]
        src.append(s + off[g])
        dst.append(d + off[g])
    return np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)


def params():
    s, p = SEEDS["params"], {}
    cell, pred = "engine_one_step_execution_cell.", "softmax_bitmap_predictor."
    p.update(synth._linear(D, 2 * D, s + 1, prefix=cell + "node_mlp_1.0."))
    p.update(synth._linear(D, D, s + 2, prefix=cell + "node_mlp_1.2."))
    p.update(synth._linear(D, 2 * D + DI, s + 3, prefix=cell + "node_mlp_2.0."))
    p.update(synth._linear(D, D, s + 4, prefix=cell + "node_mlp_2.2."))
    p["graph_layer_norm.weight"] = synth.uniform((1,), SEEDS["ln"], 0.7, 1.3)
    p["graph_layer_norm.bias"] = synth.uniform((1,), SEEDS["ln"] + 1, -0.3, 0.3)
    p.update(synth._linear(D, D, s + 5, prefix=pred + "node_mlp_1.0."))
    p.update(synth._linear(1, D, s + 6, prefix=pred + "node_mlp_1.2."))
    p.update(synth._linear(DI, D, s + 7, prefix="history_vectors_mlp.0."))
    p.update(synth._linear(DI, DI, s + 8, prefix="history_vectors_mlp.2."))
    return p


def main():
    MG.stub_dataset_entry()
    import pipeline_model_gat as PM

    m = PM.RecurrentExecutionEngine(D, DI)
    p = params()
    MG.load_params(m, p)
    m.train()                                                  # (no mode-dependent layer; gradients wanted)
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    ei = edges()
    N, B = int(batch.shape[0]), len(SIZES)
    indeg = np.bincount(ei[1], minlength=N)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    assert indeg[off[NO_IN_EDGE[0]] + NO_IN_EDGE[1]] == 0 and (indeg[off[-2]:] == 0).all() and indeg[0] == 1
    assert (batch[ei[0]] == batch[ei[1]]).all() and len({(a, b) for a, b in ei.T}) < ei.shape[1], "intra-graph, with duplicates"
    x, ins = synth.normal((N, D), SEEDS["x"]), synth.normal((STEPS, B, DI), SEEDS["instr"])
    dB, dH = synth.normal((N, STEPS), SEEDS["dB"]), synth.normal((STEPS, B, DI), SEEDS["dH"])
    ln_steps = []
    hook = m.graph_layer_norm.register_forward_hook(lambda mod, a, o: ln_steps.append(o.detach().numpy().copy()))
    xt, it = MG.t(x).clone().requires_grad_(True), MG.t(ins).clone().requires_grad_(True)
    x_out, bitmap, hv = m(xt, MG.t(ei), None, it, MG.t(batch))
    hook.remove()
    assert x_out is xt and bitmap.shape == (N, STEPS) and hv.shape == (STEPS, B, DI) and len(ln_steps) == STEPS
    ((bitmap * MG.t(dB)).sum() + (hv * MG.t(dH)).sum()).backward()
    arrays = dict(batch=batch, edge_index=ei, x=x, instr_vectors=ins, dB=dB, dH=dH, execution_bitmap=bitmap, history_vectors=hv,
                  ln_steps=np.stack(ln_steps), d_x=xt.grad, d_instr_vectors=it.grad)
    for k, v in m.named_parameters():
        arrays["p_" + k] = v
        arrays["d_" + k] = v.grad
    MG.save("recurrent_engine_small",
            dict(case="RecurrentExecutionEngine forward + the reference's autograd, loss = sum(execution_bitmap * dB) + sum(history_vectors * dH)",
                 ref="pipeline_model_gat.py:194-288 (forward :211-229, NodeModel :236-259, GlobalModel :270-286)", sizes=SIZES, D=D, Di=DI,
                 steps=STEPS, input_seeds=SEEDS, no_self_loop=NO_LOOP, no_in_edge=list(NO_IN_EDGE),
                 params="synth._linear per Linear, seeds params + 1 .. params + 8 in state_dict order; LayerNorm weight / bias synth.uniform, seeds ln, ln + 1",
                 reference_state_dict={k: list(v.shape) for k, v in m.state_dict().items()}), **arrays)


if __name__ == "__main__":
    main()
