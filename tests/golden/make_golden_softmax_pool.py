#!/usr/bin/env python3
"""Generate tests/golden/softmax_pool_small.npz by running the REFERENCE'S OWN `GlobalModel` (pipeline_model_gat.py:270-286), reached as
`RecurrentExecutionEngine(D, Di).softmax_bitmap_predictor`.

Build-container only (needs the reference checkout, see make_golden.py).  Run as:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_softmax_pool.py

Same recipe as make_golden.py (whose helpers it imports): the reference's class unmodified on top of `oracle/pyg_shim`, inputs and the
`node_mlp_1` weights from `graphvqa_amd.synth` (pure functions of integer seeds), CPU fp32 forward and the reference's own autograd for a
fixed pair of upstream gradients (loss = sum(new_history_vector * dout) + sum(gate * dgate)), plain arrays stored: x, batch, the weights,
gate, new_history_vector, dx and the weight gradients.  Graph sizes [1, 6, 21, 40, 12] at D = 12.  The metadata records what
`GlobalAttention(gate_nn, None)` must look like when `gate_nn` is laid out as the reference's `node_mlp_1`: the reference's state_dict
keys under PyG's attribute name, and PyG's repr format around the reference's own repr of that Sequential.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets sys.path to the shim, the reference and the repo; fixes the thread count)
import numpy as np  # noqa: E402

from graphvqa_amd import synth  # noqa: E402

SIZES, D, DI = [1, 6, 21, 40, 12], 12, 8
SEEDS = dict(x=81, dout=82, dgate=83, lin0=84, lin2=85)


def main():
    MG.stub_dataset_entry()
    import pipeline_model_gat as PM

    m = PM.RecurrentExecutionEngine(D, DI).softmax_bitmap_predictor
    p = {}
    p.update(synth._linear(D, D, SEEDS["lin0"], prefix="node_mlp_1.0."))
    p.update(synth._linear(1, D, SEEDS["lin2"], prefix="node_mlp_1.2."))
    MG.load_params(m, p)
    m.train()                                                  # (no mode-dependent layer; gradients wanted)
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    N, B = int(batch.shape[0]), len(SIZES)
    x, dout, dgate = synth.normal((N, D), SEEDS["x"]), synth.normal((B, D), SEEDS["dout"]), synth.normal((N, 1), SEEDS["dgate"])
    xt = MG.t(x).clone().requires_grad_(True)
    gate, hist = m(xt, None, None, None, None, MG.t(batch))
    ((hist * MG.t(dout)).sum() + (gate * MG.t(dgate)).sum()).backward()
    arrays = dict(batch=batch, x=x, dout=dout, dgate=dgate, gate=gate, new_history_vector=hist, dx=xt.grad)
    for k, v in m.named_parameters():
        arrays["p_" + k] = v
        arrays["d_" + k] = v.grad
    state = {k.replace("node_mlp_1.", "gate_nn."): list(v.shape) for k, v in m.state_dict().items()}
    MG.save("softmax_pool_small", dict(case="GlobalModel forward + the reference's autograd, loss = sum(new_history_vector * dout) + sum(gate * dgate)",
                                       ref="pipeline_model_gat.py:270-286", sizes=SIZES, D=D, input_seeds=SEEDS,
                                       params="synth._linear(D, D, lin0, 'node_mlp_1.0.'), synth._linear(1, D, lin2, 'node_mlp_1.2.')",
                                       reference_state_dict={k: list(v.shape) for k, v in m.state_dict().items()},
                                       state_dict=state, repr="GlobalAttention(gate_nn={}, nn=None)".format(m.node_mlp_1)), **arrays)


if __name__ == "__main__":
    main()
