#!/usr/bin/env python3
"""Generate tests/golden/graph_layernorm_small.npz by running the REFERENCE'S OWN graph `LayerNorm` (graph_utils/my_graph_layernorm.py).

Build-container only (needs the reference checkout, see make_golden.py).  Run as:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_graph_layernorm.py

Same recipe as make_golden.py (whose helpers it imports): the reference's class unmodified on top of `oracle/pyg_shim`, inputs from
`graphvqa_amd.synth` (pure functions of integer seeds), CPU fp32 forward and the reference's own autograd for a fixed upstream gradient
(loss = sum(out * dout)), plain arrays stored.  Three cases:
  * affine : graph sizes [1, 6, 21, 40, 12] at D = 12, weight = 1.3, bias = -0.2  -> out, dx, dweight, dbias
  * plain  : the same with affine=False                                          -> out, dx
  * none   : batch=None on [37, 12] (one segment), weight = 1.3, bias = -0.2      -> out, dx, dweight, dbias
The metadata records the modules' state_dict keys and shapes.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets sys.path to the shim, the reference and the repo; fixes the thread count)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphvqa_amd import synth  # noqa: E402

SIZES, D, N_NONE, WEIGHT, BIAS = [1, 6, 21, 40, 12], 12, 37, 1.3, -0.2
SEEDS = dict(x=71, dout=72, x_none=73, dout_none=74)


def run(m, x, batch, dout):
    xt = MG.t(x).clone().requires_grad_(True)
    out = m(xt) if batch is None else m(xt, MG.t(batch))
    (out * MG.t(dout)).sum().backward()
    res = dict(out=out, dx=xt.grad)
    if m.weight is not None:
        res.update(dweight=m.weight.grad, dbias=m.bias.grad)
    return res


def main():
    from graph_utils.my_graph_layernorm import LayerNorm

    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    N = int(batch.shape[0])
    x, dout = synth.normal((N, D), SEEDS["x"]), synth.normal((N, D), SEEDS["dout"])
    xn, dn = synth.normal((N_NONE, D), SEEDS["x_none"]), synth.normal((N_NONE, D), SEEDS["dout_none"])
    arrays = dict(batch=batch, x=x, dout=dout, x_none=xn, dout_none=dn)
    state = {}
    for tag, affine, (xx, bb, dd) in (("affine", True, (x, batch, dout)), ("plain", False, (x, batch, dout)), ("none", True, (xn, None, dn))):
        m = LayerNorm(D, affine=affine)
        if affine:
            with torch.no_grad():
                m.weight.fill_(WEIGHT)
                m.bias.fill_(BIAS)
        state[tag] = {k: list(v.shape) for k, v in m.state_dict().items()}
        for k, v in run(m, xx, bb, dd).items():
            arrays[f"{tag}_{k}"] = v
    MG.save("graph_layernorm_small", dict(case="graph LayerNorm forward + the reference's autograd, loss = sum(out * dout)",
                                          ref="graph_utils/my_graph_layernorm.py:33-81", sizes=SIZES, D=D, n_none=N_NONE, weight=WEIGHT,
                                          bias=BIAS, eps=1e-5, input_seeds=SEEDS, state_dict=state, repr=repr(LayerNorm(D))), **arrays)


if __name__ == "__main__":
    main()
