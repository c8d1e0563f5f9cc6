"""CPU tier of the RecurrentExecutionEngine and its neighbour-mean op: the fp64 restatement (tests/recurrent_engine_ref.py) against the
fixture recorded from the reference's own class, the module's state_dict against the fixture's metadata, the library's entry points and
their binding, and the argument checks that need no GPU."""
import ctypes as C
import os

import numpy as np
import torch

from tests.util import load_golden
from tests import recurrent_engine_ref as RR

TOL = 2e-5   # tests/test_softmax_pool_host.py: an fp64 restatement against an fp32 recording
SYMBOLS = ["gvqa_graph_neighbor_mean_forward", "gvqa_graph_neighbor_mean_backward"]


def test_fp64_restatement_reproduces_the_reference_fixture():
    meta, g = load_golden("recurrent_engine_small")
    B = len(meta["sizes"])
    ref = RR.engine_autograd(g["x"], g["edge_index"], g["instr_vectors"], g["batch"], RR.fixture_params(g), B, g["dB"], g["dH"])
    assert ref["execution_bitmap"].shape == g["execution_bitmap"].shape == (g["x"].shape[0], meta["steps"])
    assert ref["history_vectors"].shape == g["history_vectors"].shape == (meta["steps"], B, meta["Di"])
    errs = {k: RR.maxabs(v, g[k]) for k, v in ref.items()}
    print({k: f"{e:.3g}" for k, e in errs.items()})
    assert set(errs) == {"execution_bitmap", "history_vectors", "ln_steps", "d_x", "d_instr_vectors"} | {"d_" + k for k in meta["reference_state_dict"]}
    bad = {k: e for k, e in errs.items() if not e < TOL}
    assert not bad, bad
    # the fixture's special nodes: the op's zero row, and a bitmap that sums to one per graph and step
    off = np.concatenate([[0], np.cumsum(meta["sizes"])])
    lone = int(off[meta["no_in_edge"][0]] + meta["no_in_edge"][1])
    mean = RR.neighbor_mean(RR.tt(g["x"]), RR.tt(g["edge_index"]), g["x"].shape[0])
    assert bool((mean[lone] == 0).all()) and bool((mean[off[-2]:] == 0).all()) and torch.equal(mean[0], RR.tt(g["x"])[0])
    sums = RR.rows_sum(ref["execution_bitmap"], RR.tt(g["batch"]), B)
    assert float((sums - 1).abs().max()) < 1e-12


def test_module_state_dict_matches_the_reference():
    import graphvqa_amd
    from graphvqa_amd import recurrent_engine as RE
    meta, _ = load_golden("recurrent_engine_small")
    m = RE.RecurrentExecutionEngine(meta["D"], meta["Di"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == meta["reference_state_dict"]
    assert list(m.state_dict()) == list(meta["reference_state_dict"]), "same order as the reference's"
    assert RE.RecurrentExecutionEngine(meta["D"], meta["Di"], dropout=0.5).num_instr_features == meta["Di"]
    assert "recurrent_engine" in graphvqa_amd.__all__ and callable(RE.neighbor_mean)
    assert RE._FORCE_COMPOSED_MEAN is False and RE.MAX_EXECUTION_STEP == meta["steps"]


def test_library_exports_and_binding():
    from graphvqa_amd import _lib
    from graphvqa_amd.build import LIB, SOURCES
    assert "neighbor_mean.hip" in SOURCES
    assert os.path.exists(LIB), "build the library first (python -m graphvqa_amd.build)"
    raw = C.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(raw, s), s
        assert s in _lib.PROTOTYPES, s
    lib = _lib.load()
    f, b = lib.gvqa_graph_neighbor_mean_forward, lib.gvqa_graph_neighbor_mean_backward
    assert f.restype is C.c_int and b.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(_lib.Graph), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    assert list(b.argtypes) == [C.POINTER(_lib.Graph), C.POINTER(_lib.Graph), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gvqa.h")).read()
    for s in SYMBOLS:
        assert "GVQA_API int " + s + "(const gvqa_graph* g, " in h, s


def test_c_entry_points_validate_their_arguments_without_gpu():
    """Status codes and messages on handles with hand-filled statistics: every check comes before the first HIP call."""
    from graphvqa_amd import _lib
    from tests.graph_layernorm_ref import fake_graph as _graph
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV = _lib.E_INVALID
    g, gt, fake = _graph(), _graph(), 1 << 20                       # (never dereferenced: the checks come first)
    fwd = lambda g_, F, x=fake, out=fake, ldx=None, ldo=None: lib.gvqa_graph_neighbor_mean_forward(
        g_, F, x, F if ldx is None else ldx, out, F if ldo is None else ldo, None)
    bwd = lambda g_, F, x=fake, out=fake, ldx=None, ldo=None, gt_=C.byref(gt): lib.gvqa_graph_neighbor_mean_backward(
        g_, gt_, F, x, F if ldx is None else ldx, out, F if ldo is None else ldo, None)
    for call in (fwd, bwd):
        assert call(None, 12) == E_INV and "graph" in err()
        assert call(C.byref(_graph(finalized=0)), 12) == E_INV and "finalized" in err()
        assert call(C.byref(g), 0) == E_INV and "F must be" in err()
        assert call(C.byref(g), -3) == E_INV
        assert call(C.byref(g), 12, ldx=11) == E_INV and "row strides" in err()
        assert call(C.byref(g), 12, ldo=8) == E_INV and "row strides" in err()
        assert call(C.byref(g), 12, x=None) == E_INV and "null tensor" in err()
        assert call(C.byref(g), 12, out=None) == E_INV and "null tensor" in err()
    empty = lambda: C.byref(_graph(nodes=0, edges=0, graphs=0))      # a batch without nodes enqueues nothing
    assert fwd(empty(), 12, x=None, out=None) == 0 and bwd(empty(), 12, x=None, out=None, gt_=empty()) == 0
    assert bwd(C.byref(g), 12, gt_=None) == E_INV and "transposed" in err()
    assert bwd(C.byref(g), 12, gt_=C.byref(_graph(finalized=0))) == E_INV and "transposed" in err()
    assert bwd(C.byref(g), 12, gt_=C.byref(_graph(edges=399))) == E_INV and "counts differ" in err()
