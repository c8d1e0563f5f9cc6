"""GPU tier of the global attention pooling (graphvqa_amd/global_attention.py, csrc/softmax_pool.hip): both kernel forms -- 1 = one workgroup
per graph, 2 = split -- against oracle.ref_torch.segment_softmax + scatter_add_rows under fp64 autograd on the CPU
(tests/softmax_pool_ref.py) and against the fixture recorded from the reference's own GlobalModel.  Bounds: 1e-5 max-abs forward (gate and
out), 1e-5 of the largest reference magnitude for gradients (the bounds of the graph LayerNorm and BatchNorm training ops).  The shapes are
the smallest at which the kernels take another path: C = 3 (scalar accesses), C = 300 (a partial column tile), an empty graph in the
middle, one-node graphs, 64 / 65 nodes (a wave), 257 (one past a 256-thread block), 300 (more than one chunk of form 1's gates), row
strides C + 4 (16-byte form) and C + 1 (scalar)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from tests.util import load_golden, t
from tests import softmax_pool_ref as PR

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-5, 1e-5
FORMS = [1, 2]
SIZES = tuple(PR.SHAPE_SIZES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(batch, N, B, dev):
    from graphvqa_amd.graph import SceneGraphBatch
    return SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=dev), None if batch is None else t(batch, device=dev), N, B)


@functools.lru_cache(maxsize=None)
def _inputs(sizes, Cw, scale, seed):
    batch = PR.batch_of(list(sizes))
    N, B = batch.shape[0], len(sizes)
    return (batch, (scale * synth.normal((N,), seed)).astype(np.float32), synth.normal((N, Cw), seed + 10), synth.normal((B, Cw), seed + 20),
            synth.normal((N,), seed + 30))


@functools.lru_cache(maxsize=None)
def _case(sizes, Cw, scale, seed, with_dgate=True):
    """inputs (numpy, fp32) and the fp64 reference (gate, out, dscore, dx) of a batch, computed once and shared (read-only)."""
    batch, score, x, dout, dgate = _inputs(sizes, Cw, scale, seed)
    dg = dgate if with_dgate else None
    return batch, score, x, dout, dg, PR.autograd_reference(score, x, batch, len(sizes), dout, dg)


def _run_op(dev, score, x, dout, dgate, graph, form, score_grad=True, x_grad=True):
    from graphvqa_amd.global_attention import graph_attention_pool
    sg, xg = t(score, device=dev).requires_grad_(score_grad), t(x, device=dev).requires_grad_(x_grad)
    out, gate = graph_attention_pool(sg, xg, graph, return_gate=True, _form=form)
    if out.requires_grad:
        loss = (out * t(dout, device=dev)).sum()
        if dgate is not None:
            loss = loss + (gate * t(dgate, device=dev).view(-1, 1)).sum()
        loss.backward()
    return gate.detach().view(-1), out.detach(), sg.grad, xg.grad


def _errors(got, ref):
    return dict(gate=PR.maxabs(got[0], ref[0]), out=PR.maxabs(got[1], ref[1]), dscore=PR.rel(got[2], ref[2]), dx=PR.rel(got[3], ref[3]))


def _check(got, ref):
    e = _errors(got, ref)
    print({k: f"{v:.3g}" for k, v in e.items()})
    assert e["gate"] < FWD_TOL and e["out"] < FWD_TOL and e["dscore"] < GRAD_TOL and e["dx"] < GRAD_TOL, e


# ---- fixture parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_module_matches_the_reference_fixture(dev, form):
    """GlobalAttention(gate_nn, None) with return_gate=True is the reference's GlobalModel: gate, out, dx and every gate_nn gradient."""
    from graphvqa_amd.global_attention import GlobalAttention
    meta, g = load_golden("softmax_pool_small")
    D = meta["D"]
    nn = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.ReLU(), torch.nn.Linear(D, 1))
    nn.load_state_dict({k[len("p_node_mlp_1."):]: t(v) for k, v in g.items() if k.startswith("p_node_mlp_1.")})
    m = GlobalAttention(nn, None)
    m.gate_nn.load_state_dict({k[len("p_node_mlp_1."):]: t(v) for k, v in g.items() if k.startswith("p_node_mlp_1.")})   # (the constructor resets)
    m = m.to(dev)
    xg = t(g["x"], device=dev).requires_grad_(True)
    gate, out = m(xg, t(g["batch"], device=dev), return_gate=True, _form=form)
    assert gate.shape == g["gate"].shape and out.shape == g["new_history_vector"].shape
    ((out * t(g["dout"], device=dev)).sum() + (gate * t(g["dgate"], device=dev)).sum()).backward()
    assert PR.maxabs(gate, g["gate"]) < FWD_TOL and PR.maxabs(out, g["new_history_vector"]) < FWD_TOL
    assert PR.rel(xg.grad, g["dx"]) < GRAD_TOL
    # every gate_nn gradient at 1e-5 of its own largest reference magnitude -- except the last bias: it shifts every score of a softmax, so its
    # gradient, the sum of the 80 dscore_i, is exactly zero and the fixture holds only the reference's own rounding of that sum (1.2e-7).
    # A zero has no magnitude of its own: it is held to 1e-5 of the largest magnitude among gate_nn's gradients, which are sums over the
    # same dscore_i.  (The floor of tests/test_gpu_backward.py, 1e-3 of the largest gradient, at this file's 1e-5 would ask for 1e-8 of
    # it, below fp32's 6e-8: the reference's own value would miss it.)
    family = max(float(np.abs(g["d_node_mlp_1." + k]).max()) for k, _ in m.gate_nn.named_parameters())
    for k, v in m.gate_nn.named_parameters():
        r = g["d_node_mlp_1." + k]
        scale = family if k == "2.bias" else float(np.abs(r).max())
        e = PR.maxabs(v.grad, r) / scale
        print(k, f"{e:.3g}")
        assert e < GRAD_TOL, (k, e)


# ---- shape matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_dgate", [True, False])
@pytest.mark.parametrize("Cw,scale,seed", [(3, 1.0, 11), (300, 1.0, 12), (512, 1.0, 13), (512, 50.0, 14)])
def test_shape_matrix(dev, Cw, scale, seed, with_dgate, form):
    """scale 50: a nearly one-hot softmax, scores spanning +-200."""
    batch, score, x, dout, dgate, ref = _case(SIZES, Cw, scale, seed, with_dgate)
    graph = _graph(batch, x.shape[0], len(SIZES), dev)
    got = _run_op(dev, score, x, dout, dgate, graph, form)
    _check(got, ref)
    assert bool((got[1][SIZES.index(0)] == 0).all()), "an empty graph pools to a zero row"


# ---- strided rows (C level) -------------------------------------------------------------------------------------------------------
def _c_call(dev, graph, Cw, sbuf, lds, xw, ldx, dw_, ldd, dgate, form, ld_out, ld_dx, want=("dscore", "dx"), guard=64):
    """forward + backward through the C ABI.  out / dx are [*, ld] buffers pre-filled with a poison value; gate, dscore, out and the
    workspace sit inside poisoned guard zones.  Returns (gate, outw, dscore, dxw) and the guard check."""
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream
    lib = _lib.load()
    N, B = graph.num_nodes, graph.num_graphs
    P = 777.0
    gbuf, dsbuf = torch.full((N + 2 * guard,), P, device=dev), torch.full((N + 2 * guard,), P, device=dev)
    obuf = torch.full((B * ld_out + 2 * guard,), P, device=dev)
    outw = obuf[guard:guard + B * ld_out].view(B, ld_out)
    dxw = torch.full((N, ld_dx), P, device=dev)
    need = lib.gvqa_graph_softmax_pool_workspace_bytes(C.byref(graph.c), Cw)
    wbuf = torch.full((need + 1024,), 0x5A, dtype=torch.uint8, device=dev)
    gate, dscore = gbuf[guard:guard + N], dsbuf[guard:guard + N]
    s = _stream(dev)
    _lib.check(lib.gvqa_graph_softmax_pool_forward(C.byref(graph.c), Cw, sbuf.data_ptr(), lds, xw.data_ptr(), ldx, gate.data_ptr(), outw.data_ptr(),
                                                   ld_out, form, wbuf[512:].data_ptr(), need, s))
    _lib.check(lib.gvqa_graph_softmax_pool_backward(C.byref(graph.c), Cw, xw.data_ptr(), ldx, gate.data_ptr(), dw_.data_ptr(), ldd,
                                                    None if dgate is None else dgate.data_ptr(),
                                                    dscore.data_ptr() if "dscore" in want else None, dxw.data_ptr() if "dx" in want else None,
                                                    ld_dx, form, wbuf[512:].data_ptr(), need, s))
    torch.cuda.synchronize(dev)
    clean = all(bool((b[:guard] == P).all()) and bool((b[-guard:] == P).all()) for b in (gbuf, dsbuf, obuf))
    clean = clean and bool((wbuf[:512] == 0x5A).all()) and bool((wbuf[512 + need:] == 0x5A).all())
    return gate, outw, dscore, dxw, clean


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pad", [4, 1])
def test_strided_rows(dev, pad, form):
    Cw = 300
    batch, score, x, dout, dgate, ref = _case(SIZES, Cw, 1.0, 12)
    N, B, ld = x.shape[0], len(SIZES), Cw + pad
    graph = _graph(batch, N, B, dev)
    xw, dw_ = torch.full((N, ld), 555.0, device=dev), torch.full((B, ld), 555.0, device=dev)
    xw[:, :Cw], dw_[:, :Cw] = t(x, device=dev), t(dout, device=dev)
    sbuf = torch.full((N, 2), 555.0, device=dev)
    sbuf[:, 0] = t(score, device=dev)
    gate, outw, dscore, dxw, clean = _c_call(dev, graph, Cw, sbuf, 2, xw, ld, dw_, ld, t(dgate, device=dev), form, ld, ld)
    _check((gate, outw[:, :Cw], dscore, dxw[:, :Cw]), ref)
    assert bool((outw[:, Cw:] == 777.0).all()) and bool((dxw[:, Cw:] == 777.0).all()), "padding columns were written"
    assert clean, "a write outside gate / out / dscore / the workspace"


# ---- large segments ---------------------------------------------------------------------------------------------------------------
def test_one_graph_of_4097_nodes(dev):
    """Both forced forms and the auto rule; auto is bit-identical to the form graph_attention_pool_form names."""
    from graphvqa_amd.global_attention import graph_attention_pool_form
    batch, score, x, dout, dgate, ref = _case((4097,), 300, 1.0, 15)
    graph = _graph(batch, 4097, 1, dev)
    got = {f: _run_op(dev, score, x, dout, dgate, graph, f) for f in (None, 1, 2)}
    for f in (None, 1, 2):
        _check(got[f], ref)
    named = graph_attention_pool_form(graph, 300)
    assert named in (1, 2)
    for a, c in zip(got[None], got[named]):
        assert torch.equal(a, c)
    assert graph_attention_pool_form(_graph(PR.batch_of([40, 6]), 46, 2, dev), 512) == 1       # the workload's graphs stay on form 1


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_equal_scores(dev, form):
    """All scores equal: gate = 1 / n and dscore = the centred t / n, t_i = <dout[b], x[i]> + dgate_i."""
    sizes, Cw = [5, 1, 300], 12
    batch, _, x, dout, dgate = _inputs(tuple(sizes), Cw, 1.0, 16)
    score = np.full(batch.shape[0], 0.375, dtype=np.float32)
    graph = _graph(batch, batch.shape[0], len(sizes), dev)
    gate, out, dscore, dx = _run_op(dev, score, x, dout, dgate, graph, form)
    n = np.repeat(np.asarray(sizes, dtype=np.float64), sizes)
    tt = (dout.astype(np.float64)[batch] * x.astype(np.float64)).sum(-1) + dgate.astype(np.float64)
    mean = np.concatenate([np.full(s, tt[batch == b].mean()) for b, s in enumerate(sizes)])
    assert PR.maxabs(gate, 1.0 / n) < FWD_TOL
    assert PR.rel(dscore, (tt - mean) / n) < GRAD_TOL
    _check((gate, out, dscore, dx), PR.autograd_reference(score, x, batch, len(sizes), dout, dgate))


@pytest.mark.parametrize("form", FORMS)
def test_trailing_empty_graphs_and_no_nodes(dev, form):
    from graphvqa_amd.global_attention import GlobalAttention, graph_attention_pool
    D = 8
    m = GlobalAttention(torch.nn.Linear(D, 1)).to(dev)
    batch = PR.batch_of([3, 0, 4])
    x = t(synth.normal((7, D), 17), device=dev).requires_grad_(True)
    out = m(x, t(batch, device=dev), size=6, _form=form)
    assert out.shape == (6, D) and bool((out[3:] == 0).all()) and bool((out[1] == 0).all())
    ref = m(x, t(batch, device=dev), _form=form)
    assert ref.shape == (3, D) and torch.equal(out[:3], ref)
    out.sum().backward()
    assert bool(torch.isfinite(x.grad).all())
    # N = 0: zero rows, gradients of the right shapes
    for B in (0, 2):
        graph = _graph(np.zeros(0, dtype=np.int64), 0, B, dev)
        s0, x0 = torch.zeros((0, 1), device=dev, requires_grad=True), torch.zeros((0, D), device=dev, requires_grad=True)
        o, gt = graph_attention_pool(s0, x0, graph, return_gate=True, _form=form)
        assert o.shape == (B, D) and gt.shape == (0, 1) and bool((o == 0).all())
        (o.sum() + gt.sum()).backward()
        assert s0.grad.shape == (0, 1) and x0.grad.shape == (0, D)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_two_runs_are_bit_identical(dev, form):
    batch, score, x, dout, dgate, _ = _case(SIZES, 512, 1.0, 13)
    graph = _graph(batch, x.shape[0], len(SIZES), dev)
    runs = [_run_op(dev, score, x, dout, dgate, graph, form) for _ in range(2)]
    for a, c in zip(*runs):
        assert torch.equal(a, c)


# ---- selective gradients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_selective_gradients(dev, form):
    Cw = 300
    batch, score, x, dout, dgate, ref = _case(SIZES, Cw, 1.0, 12)
    N, B = x.shape[0], len(SIZES)
    graph = _graph(batch, N, B, dev)
    full = _run_op(dev, score, x, dout, dgate, graph, form)
    got = _run_op(dev, score, x, dout, dgate, graph, form, score_grad=False)            # x only
    assert got[2] is None and torch.equal(got[3], full[3]) and torch.equal(got[1], full[1]) and torch.equal(got[0], full[0])
    got = _run_op(dev, score, x, dout, dgate, graph, form, x_grad=False)                # score only
    assert got[3] is None and torch.equal(got[2], full[2])
    # neither: no graph, nothing saved
    from graphvqa_amd.global_attention import graph_attention_pool
    out, gate = graph_attention_pool(t(score, device=dev), t(x, device=dev), graph, return_gate=True, _form=form)
    assert out.grad_fn is None and gate.grad_fn is None and not out.requires_grad
    assert torch.equal(out, full[1]) and torch.equal(gate.view(-1), full[0])
    out = graph_attention_pool(t(score, device=dev).requires_grad_(True), t(x, device=dev), graph, _form=form)
    assert [tuple(v.shape) for v in out.grad_fn.saved_tensors] == [(N, Cw), (N, 1)]
    # C level: with dscore == NULL / dx == NULL the call writes its other output and nothing around out, gate and the workspace
    xg, dg_, sg = t(x, device=dev), t(dout, device=dev), t(score, device=dev)
    for want in (("dx",), ("dscore",)):
        gate, outw, dscore, dxw, clean = _c_call(dev, graph, Cw, sg, 1, xg, Cw, dg_, Cw, t(dgate, device=dev), form, Cw, Cw, want=want)
        assert clean and torch.equal(outw, full[1]) and torch.equal(gate, full[0])
        if "dx" in want:
            assert torch.equal(dxw, full[3]) and bool((dscore == 777.0).all())
        else:
            assert torch.equal(dscore, full[2]) and bool((dxw == 777.0).all())


# ---- module -----------------------------------------------------------------------------------------------------------------------
def test_pooling_module_on_both_roads(dev, monkeypatch):
    """MyConditionalGlobalAttention's differentiable forward on the fused op and on the composed road (_FORCE_COMPOSED_POOL): output and
    every parameter gradient against fp64 autograd through the oracle, with the bounds of tests/test_gpu_backward.py's pooling test (1e-4
    output, 1e-4 of the gradient's scale with its floor); the eval no-grad output agrees with both."""
    from oracle import ref_torch as R
    from tests.util import tparams
    from graphvqa_amd import pipeline_head as PH
    gb = synth.make_graph_batch(7, seed=0x9001, nodes_lo=1, nodes_hi=25)
    N, B, D = gb.num_nodes, gb.num_graphs, 32
    pp = synth.attention_pool_params(D, D, seed=3)
    x, u, w = synth.normal((N, D), 1), synth.normal((B, D), 2), synth.normal((B, D), 3)
    rpp = {k: v.double().requires_grad_(True) for k, v in tparams(pp).items()}
    rs = [t(a).double().requires_grad_(True) for a in (x, u)]
    ref = R.global_attention_pool(rs[0], rs[1], t(gb.batch), rpp, B)
    (ref * t(w).double()).sum().backward()
    floor = 1e-3 * max(float(v.grad.abs().max()) for v in list(rpp.values()) + rs)
    rel = lambda a, b: PR.maxabs(a, b) / max(float(b.abs().max()), floor, 1e-12)
    outs = {}
    for road, composed in (("fused", False), ("composed", True)):
        monkeypatch.setattr(PH, "_FORCE_COMPOSED_POOL", composed)
        pool = PH.MyConditionalGlobalAttention(D, D)
        pool.load_state_dict({k: t(v) for k, v in pp.items()})
        pool = pool.to(dev).eval()
        xs = [t(a, device=dev).requires_grad_(True) for a in (x, u)]
        out = pool(xs[0], xs[1], t(gb.batch, device=dev))
        assert out.requires_grad
        (out * t(w, device=dev)).sum().backward()
        assert PR.maxabs(out, ref) < 1e-4, road
        assert rel(xs[0].grad, rs[0].grad) < 1e-4 and rel(xs[1].grad, rs[1].grad) < 1e-4, road
        for k, v in pool.named_parameters():
            assert rel(v.grad, rpp[k].grad) < 1e-4, (road, k)
        outs[road] = out.detach()
        with torch.no_grad():
            outs["eval"] = pool(xs[0], xs[1], t(gb.batch, device=dev))
    assert PR.maxabs(outs["eval"], outs["fused"]) < 1e-4 and PR.maxabs(outs["eval"], outs["composed"]) < 1e-4


# ---- error paths ------------------------------------------------------------------------------------------------------------------
def test_error_codes(dev):
    from graphvqa_amd import _lib
    from graphvqa_amd.global_attention import graph_attention_pool
    lib = _lib.load()
    Cw = 8
    graph = _graph(PR.batch_of([3, 2]), 5, 2, dev)
    x, dx, sc, gt = torch.zeros((5, Cw), device=dev), torch.zeros((5, Cw), device=dev), torch.zeros(5, device=dev), torch.zeros(5, device=dev)
    out = torch.zeros((2, Cw), device=dev)
    need = lib.gvqa_graph_softmax_pool_workspace_bytes(C.byref(graph.c), Cw)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    err = lambda: lib.gvqa_last_error().decode()
    g = C.byref(graph.c)
    fwd = lambda C_, xp, nbytes, ldx=Cw, form=0: lib.gvqa_graph_softmax_pool_forward(g, C_, sc.data_ptr(), 1, xp, ldx, gt.data_ptr(), out.data_ptr(), Cw,
                                                                                     form, ws.data_ptr(), nbytes, None)
    bwd = lambda C_, xp, nbytes, ldx=Cw, form=0: lib.gvqa_graph_softmax_pool_backward(g, C_, xp, ldx, gt.data_ptr(), out.data_ptr(), Cw, None, sc.data_ptr(),
                                                                                      dx.data_ptr(), Cw, form, ws.data_ptr(), nbytes, None)
    for call in (fwd, bwd):
        assert call(Cw, x.data_ptr(), need - 1) == _lib.E_WORKSPACE and "workspace" in err()
        assert call(Cw, None, need) == _lib.E_INVALID and "null" in err()
        assert call(0, x.data_ptr(), need) == _lib.E_INVALID and err()
        assert call(Cw, x.data_ptr(), need, ldx=Cw - 1) == _lib.E_INVALID and err()
        assert call(Cw, x.data_ptr(), need, form=3) == _lib.E_INVALID and "form" in err()
    empty = _lib.Graph()
    empty.valid = empty.finalized = 1                                                     # no graphs, no nodes
    assert lib.gvqa_graph_softmax_pool_forward(C.byref(empty), Cw, None, 1, None, Cw, None, None, Cw, 0, None, 0, None) == _lib.GVQA_OK
    with pytest.raises(TypeError):
        graph_attention_pool(sc, x.double(), graph)
    with pytest.raises(TypeError):
        graph_attention_pool(sc.double(), x, graph)
    with pytest.raises(RuntimeError):
        graph_attention_pool(sc.cpu(), x.cpu(), graph)
