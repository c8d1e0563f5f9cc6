"""CPU tier of the graph LayerNorm: the oracle against the fixture recorded from the reference's own class, the closed-form backward the
HIP kernels implement against the oracle's autograd, and the module's state_dict against the reference's."""
import ctypes as C

import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from tests.util import load_golden
from tests import graph_layernorm_ref as GR

TOL = 2e-5   # tests/test_oracle_golden.py: the fixture is fp32


@pytest.mark.parametrize("tag", ["affine", "plain", "none"])
def test_oracle_fp64_reproduces_the_reference_fixture(tag):
    meta, g = load_golden("graph_layernorm_small")
    x, dout = (g["x_none"], g["dout_none"]) if tag == "none" else (g["x"], g["dout"])
    batch = np.zeros(x.shape[0], dtype=np.int64) if tag == "none" else g["batch"]
    B = 1 if tag == "none" else len(meta["sizes"])
    w, b = (None, None) if tag == "plain" else (meta["weight"], meta["bias"])
    out, dx, dw, db = GR.autograd_reference(x, batch, B, w, b, dout, meta["eps"])
    assert GR.maxabs(out, g[f"{tag}_out"]) < TOL and GR.maxabs(dx, g[f"{tag}_dx"]) < TOL
    if tag != "plain":
        assert GR.maxabs(dw, g[f"{tag}_dweight"]) < TOL and GR.maxabs(db, g[f"{tag}_dbias"]) < TOL


@pytest.mark.parametrize("sizes,D", [([3, 0, 1, 7], 5), ([1, 1, 0], 4), (GR.SHAPE_SIZES, 3)])
def test_closed_form_backward_matches_fp64_autograd(sizes, D):
    """Batches with an empty graph and with a one-node graph: 1e-12 relative."""
    batch = GR.batch_of(sizes)
    x, dout = synth.normal((batch.shape[0], D), 11).astype(np.float64), synth.normal((batch.shape[0], D), 12).astype(np.float64)
    ref = GR.autograd_reference(x, batch, len(sizes), 1.3, -0.2, dout)
    got = GR.closed_form(x, batch, len(sizes), 1.3, -0.2, dout)
    for name, a, r in zip(("out", "dx", "dweight", "dbias"), got, ref):
        assert GR.rel(a, r) < 1e-12, (name, GR.rel(a, r))


def test_closed_form_constant_graph_drops_the_variance_term():
    """sigma == 0: out = bias, dx = (w dout - mean(w dout)) / eps, every gradient finite (the reference's autograd gives NaN there)."""
    batch = GR.batch_of([2, 3])
    x, dout = synth.normal((5, 4), 13).astype(np.float64), synth.normal((5, 4), 14).astype(np.float64)
    x[:2] = 0.75
    out, dx, dw, db = GR.closed_form(x, batch, 2, 1.3, -0.2, dout, 1e-5)
    assert torch.equal(out[:2], torch.full((2, 4), -0.2, dtype=torch.float64))
    gy = torch.from_numpy(dout[:2]) * 1.3
    assert GR.rel(dx[:2], (gy - gy.mean()) / 1e-5) < 1e-12
    assert all(bool(torch.isfinite(v).all()) for v in (dx, dw, db))


@pytest.mark.parametrize("affine,tag", [(True, "affine"), (False, "plain")])
def test_module_state_dict_matches_the_reference(affine, tag):
    from graphvqa_amd.graph_layernorm import LayerNorm
    meta, _ = load_golden("graph_layernorm_small")
    m = LayerNorm(meta["D"], affine=affine)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == meta["state_dict"][tag]
    assert repr(m) == meta["repr"]
    if affine:
        assert m.weight.item() == 1.0 and m.bias.item() == 0.0
    else:
        assert m.weight is None and m.bias is None


def test_c_entry_points_validate_their_arguments_without_gpu():
    """Status codes and messages of the two calls on a handle with hand-filled statistics (nothing is enqueued), the workspace size
    and the auto rule's answer for the workload's graphs and for one large segment."""
    from graphvqa_amd import _lib
    _graph = GR.fake_graph
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV, E_WS = _lib.E_INVALID, _lib.E_WORKSPACE
    g, fake = _graph(), 1 << 20                       # (never dereferenced: the checks come first)
    need = lib.gvqa_graph_layernorm_workspace_bytes(C.byref(g), 512)
    assert need >= 4 * 2 * 4 * 2 and lib.gvqa_graph_layernorm_workspace_bytes(C.byref(g), 0) == 0
    fwd = lambda g_, D, x=fake, ldx=None, form=0, ws=fake, nb=need: lib.gvqa_graph_layernorm_forward(
        g_, D, x, D if ldx is None else ldx, None, None, 1e-5, fake, D, None, form, ws, nb, None)
    bwd = lambda g_, D, x=fake, ldx=None, form=0, ws=fake, nb=need, st=fake: lib.gvqa_graph_layernorm_backward(
        g_, D, x, D if ldx is None else ldx, fake, D, None, 1e-5, st, fake, D, None, None, form, ws, nb, None)
    for call in (fwd, bwd):
        assert call(None, 512) == E_INV and "graph" in err()
        assert call(C.byref(_graph(finalized=0)), 512) == E_INV and "finalized" in err()
        assert call(C.byref(g), 0) == E_INV and "D must be" in err()
        assert call(C.byref(g), -3) == E_INV
        assert call(C.byref(g), 512, form=3) == E_INV and "form" in err()
        assert call(C.byref(g), 512, ldx=500) == E_INV and "row strides" in err()
        assert call(C.byref(g), 512, x=None) == E_INV and "null tensor" in err()
        assert call(C.byref(g), 512, nb=need - 1) == E_WS and "workspace" in err()
        assert call(C.byref(g), 512, ws=None) == E_WS
        assert call(C.byref(_graph(nodes=0, edges=0, graphs=0)), 512, x=None, ws=None, nb=0) == 0      # an empty batch enqueues nothing
    assert bwd(C.byref(g), 512, st=None) == E_INV and "null tensor" in err()
    # the auto rule: the workload's graphs (<= 40 nodes x 512) stay on one workgroup per graph, one large segment is split
    assert lib.gvqa_graph_layernorm_form(C.byref(g), 512) == 1
    assert lib.gvqa_graph_layernorm_form(C.byref(_graph(nodes=4097, edges=0, graphs=1, max_graph_nodes=4097)), 300) == 2
    assert lib.gvqa_graph_layernorm_form(C.byref(_graph(nodes=128, edges=0, graphs=1, max_graph_nodes=128)), 512) == 1     # 65 536: still form 1
    assert lib.gvqa_graph_layernorm_form(C.byref(_graph(nodes=129, edges=0, graphs=1, max_graph_nodes=129)), 512) == 2
    # one huge graph among very many small ones: the split form's grid (graphs x chunks) and with it the workspace stay bounded
    many = _graph(nodes=9_000_000, edges=0, graphs=100_000, max_graph_nodes=16_384)
    assert lib.gvqa_graph_layernorm_workspace_bytes(C.byref(many), 512) <= (1 << 22) * 8 + 100_000 * 8 + 512
    assert lib.gvqa_graph_layernorm_form(C.byref(many), 0) == E_INV
