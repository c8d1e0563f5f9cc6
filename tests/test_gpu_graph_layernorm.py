"""GPU tier of the graph LayerNorm (graphvqa_amd/graph_layernorm.py, csrc/graph_layernorm.hip): both kernel forms -- 1 = one workgroup per
graph, 2 = split -- against oracle.ref_torch.graph_layernorm in fp64 on the CPU (tests/graph_layernorm_ref.py) and against the fixture
recorded from the reference's own class.  Bounds: 1e-5 max-abs forward, 1e-5 of the largest reference magnitude for gradients (the
bounds of the BatchNorm training op, tests/test_gpu_backward.py).  The shapes are the smallest at which the kernels take another path:
D = 3 (scalar accesses), an empty graph in the middle, a one-node graph, a graph of 129 nodes (more than one chunk of the split form at
D >= 300), row strides D + 4 (16-byte form with a row / column split) and D + 1 (scalar)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from tests.util import load_golden, t
from tests import graph_layernorm_ref as GR

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-5, 1e-5
W, B_ = 1.3, -0.2
FORMS = [1, 2]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(batch, N, B, dev):
    from graphvqa_amd.graph import SceneGraphBatch
    return SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=dev), None if batch is None else t(batch, device=dev), N, B)


def _params(dev, w=W, b=B_):
    return (torch.tensor([w], device=dev, requires_grad=True), torch.tensor([b], device=dev, requires_grad=True))


@functools.lru_cache(maxsize=None)
def _case(sizes, D, scale, offset, seed=21):
    """inputs (numpy, fp32) and the fp64 reference of a batch, computed once and shared (read-only)."""
    batch = GR.batch_of(list(sizes))
    N = batch.shape[0]
    x = (offset + scale * synth.normal((N, D), seed)).astype(np.float32)
    dout = synth.normal((N, D), seed + 1)
    return batch, x, dout, GR.autograd_reference(x, batch, len(sizes), W, B_, dout)


def _run_op(dev, x, dout, graph, form, w=None, b=None, x_grad=True):
    from graphvqa_amd.graph_layernorm import graph_layernorm
    xg = t(x, device=dev).requires_grad_(x_grad)
    out = graph_layernorm(xg, graph, w, b, 1e-5, _form=form)
    if out.requires_grad:
        (out * t(dout, device=dev)).sum().backward()
    return out.detach(), xg.grad, None if w is None else w.grad, None if b is None else b.grad


def _check(got, ref, fwd_tol=FWD_TOL, tols=(GRAD_TOL, GRAD_TOL, GRAD_TOL)):
    out, dx, dw, db = got
    e = dict(out=GR.maxabs(out, ref[0]), dx=GR.rel(dx, ref[1]), dweight=GR.rel(dw, ref[2]), dbias=GR.rel(db, ref[3]))
    print({k: f"{v:.3g}" for k, v in e.items()})
    assert e["out"] < fwd_tol and e["dx"] < tols[0] and e["dweight"] < tols[1] and e["dbias"] < tols[2], e


# ---- fixture parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag", ["affine", "plain", "none"])
def test_module_matches_the_reference_fixture(dev, tag, form):
    from graphvqa_amd.graph_layernorm import LayerNorm
    meta, g = load_golden("graph_layernorm_small")
    m = LayerNorm(meta["D"], eps=meta["eps"], affine=tag != "plain").to(dev)
    if tag != "plain":
        with torch.no_grad():
            m.weight.fill_(meta["weight"]); m.bias.fill_(meta["bias"])
    x, dout = (g["x_none"], g["dout_none"]) if tag == "none" else (g["x"], g["dout"])
    xg = t(x, device=dev).requires_grad_(True)
    out = m(xg, _form=form) if tag == "none" else m(xg, t(g["batch"], device=dev), _form=form)
    (out * t(dout, device=dev)).sum().backward()
    assert GR.maxabs(out, g[f"{tag}_out"]) < FWD_TOL and GR.rel(xg.grad, g[f"{tag}_dx"]) < GRAD_TOL
    if tag != "plain":
        assert GR.rel(m.weight.grad, g[f"{tag}_dweight"]) < GRAD_TOL and GR.rel(m.bias.grad, g[f"{tag}_dbias"]) < GRAD_TOL


# ---- shape matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("D,scale", [(3, 1.0), (300, 1.0), (512, 1.0), (512, 5.0)])
def test_shape_matrix(dev, D, scale, form):
    batch, x, dout, ref = _case(tuple(GR.SHAPE_SIZES), D, scale, 0.0)
    graph = _graph(batch, x.shape[0], len(GR.SHAPE_SIZES), dev)
    w, b = _params(dev)
    _check(_run_op(dev, x, dout, graph, form, w, b), ref)


# ---- strided rows (C level: out and dx are column blocks too) -------------------------------------------------------------------------
def _c_call(dev, graph, D, xw, ld, dw_, form, w, b, want=("dx", "dw", "db"), stats=None, eps=1e-5):
    """forward + backward through the C ABI on [N, ld] buffers whose first D columns are the tensors; returns the wide out / dx buffers,
    dweight, dbias and stats.  Padding columns of out / dx are pre-filled with a poison value."""
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream
    lib = _lib.load()
    N = xw.shape[0]
    outw = torch.full((N, ld), 777.0, device=dev)
    dxw = torch.full((N, ld), 777.0, device=dev)
    st = torch.zeros((graph.num_graphs, 2), device=dev) if stats is None else stats
    dwt, dbt = torch.full((1,), 777.0, device=dev), torch.full((1,), 777.0, device=dev)
    ws = torch.empty(max(lib.gvqa_graph_layernorm_workspace_bytes(C.byref(graph.c), D), 256), dtype=torch.uint8, device=dev)
    s = _stream(dev)
    _lib.check(lib.gvqa_graph_layernorm_forward(C.byref(graph.c), D, xw.data_ptr(), ld, w.data_ptr(), b.data_ptr(), eps, outw.data_ptr(), ld,
                                                st.data_ptr(), form, ws.data_ptr(), ws.numel(), s))
    _lib.check(lib.gvqa_graph_layernorm_backward(C.byref(graph.c), D, xw.data_ptr(), ld, dw_.data_ptr(), ld, w.data_ptr(), eps, st.data_ptr(),
                                                 dxw.data_ptr() if "dx" in want else None, ld, dwt.data_ptr() if "dw" in want else None,
                                                 dbt.data_ptr() if "db" in want else None, form, ws.data_ptr(), ws.numel(), s))
    torch.cuda.synchronize(dev)
    return outw, dxw, dwt, dbt, st


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pad", [4, 1])
def test_strided_rows(dev, pad, form):
    D = 300
    batch, x, dout, ref = _case(tuple(GR.SHAPE_SIZES), D, 1.0, 0.0)
    N, ld = x.shape[0], D + pad
    graph = _graph(batch, N, len(GR.SHAPE_SIZES), dev)
    xw, dw_ = torch.full((N, ld), 555.0, device=dev), torch.full((N, ld), 555.0, device=dev)
    xw[:, :D], dw_[:, :D] = t(x, device=dev), t(dout, device=dev)
    w, b = torch.tensor([W], device=dev), torch.tensor([B_], device=dev)
    outw, dxw, dwt, dbt, _ = _c_call(dev, graph, D, xw, ld, dw_, form, w, b)
    _check((outw[:, :D], dxw[:, :D], dwt, dbt), ref)
    assert bool((outw[:, D:] == 777.0).all()) and bool((dxw[:, D:] == 777.0).all()), "padding columns were written"


# ---- large segments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_one_graph_of_3000_nodes(dev, form):
    """900 000 elements in one segment; on this input dweight cancels to 35.2 and dbias to 164.5 (fp64), so the relative bound is a bound
    on the summation order: one fp32 chain over the 3500 values a thread of form 1 owns is 7e-6 off in dbias, the kernels' two-level order 3e-7."""
    from graphvqa_amd._lib import GvqaUnsupported
    batch, x, dout, ref = _case((3000,), 300, 1.0, 0.0)
    graph = _graph(batch, 3000, 1, dev)
    w, b = _params(dev)
    try:
        got = _run_op(dev, x, dout, graph, form, w, b)
    except GvqaUnsupported:
        assert form == 1          # a forced form beyond its cap may refuse; auto and the split form never do
        return
    _check(got, ref)


def test_batch_none_takes_the_split_form(dev):
    from graphvqa_amd.graph_layernorm import LayerNorm, graph_layernorm_form
    N, D = 4097, 300
    batch, x, dout, ref = _case((N,), D, 1.0, 0.0, seed=31)
    graph = _graph(None, N, 1, dev)
    assert graph_layernorm_form(graph, D) == 2
    assert graph_layernorm_form(_graph(GR.batch_of([40, 6]), 46, 2, dev), 512) == 1       # the workload's graphs stay on form 1
    m = LayerNorm(D).to(dev)
    with torch.no_grad():
        m.weight.fill_(W); m.bias.fill_(B_)
    xg = t(x, device=dev).requires_grad_(True)
    out = m(xg)                                                                           # batch=None, auto rule
    (out * t(dout, device=dev)).sum().backward()
    _check((out.detach(), xg.grad, m.weight.grad, m.bias.grad), ref)
    # auto == forced split, bit for bit
    w, b = _params(dev)
    got = _run_op(dev, x, dout, graph, 2, w, b)
    assert torch.equal(got[0], out.detach()) and torch.equal(got[1], xg.grad) and torch.equal(got[2], m.weight.grad)


# ---- offset: a one-pass E[x^2] - mu^2 variance is about 2e-4 off here -----------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_offset_inputs(dev, form):
    """x = 30 + N(0, 1), D = 512.  Bound per quantity: max(1e-5, 2 x the error of the fp32 composition on the CPU against fp64) on the same
    inputs (measured: 5.0e-6 out, 2.0e-7 dx, 2.8e-6 dweight, so 1e-5 each)."""
    sizes = tuple(GR.SHAPE_SIZES)
    batch, x, dout, ref = _case(sizes, 512, 1.0, 30.0)
    c32 = GR.autograd_reference(x, batch, len(sizes), W, B_, dout, dtype=torch.float32)
    bound = dict(out=max(1e-5, 2 * GR.maxabs(c32[0], ref[0])), dx=max(1e-5, 2 * GR.rel(c32[1], ref[1])), dweight=max(1e-5, 2 * GR.rel(c32[2], ref[2])))
    print("composition bounds", bound)
    graph = _graph(batch, x.shape[0], len(sizes), dev)
    w, b = _params(dev)
    _check(_run_op(dev, x, dout, graph, form, w, b), ref, fwd_tol=bound["out"], tols=(bound["dx"], bound["dweight"], GRAD_TOL))


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_two_runs_are_bit_identical(dev, form):
    batch, x, dout, _ = _case(tuple(GR.SHAPE_SIZES), 512, 1.0, 0.0)
    graph = _graph(batch, x.shape[0], len(GR.SHAPE_SIZES), dev)
    runs = []
    for _ in range(2):
        w, b = _params(dev)
        runs.append(_run_op(dev, x, dout, graph, form, w, b))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


# ---- selective gradients -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_selective_gradients(dev, form, monkeypatch):
    D = 300
    batch, x, dout, ref = _case(tuple(GR.SHAPE_SIZES), D, 1.0, 0.0)
    N, nb = x.shape[0], len(GR.SHAPE_SIZES)
    graph = _graph(batch, N, nb, dev)
    w, b = _params(dev)
    full = _run_op(dev, x, dout, graph, form, w, b)
    # dx only: constant parameters
    got = _run_op(dev, x, dout, graph, form, torch.tensor([W], device=dev), torch.tensor([B_], device=dev))
    assert torch.equal(got[1], full[1]) and got[2] is None and got[3] is None
    # parameters only
    w2, b2 = _params(dev)
    got = _run_op(dev, x, dout, graph, form, w2, b2, x_grad=False)
    assert got[1] is None and torch.equal(got[2], full[2]) and torch.equal(got[3], full[3])
    # what the op hands the C call: a stats buffer and saved tensors only when something needs a gradient
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream
    lib = _lib.load()
    seen, real = [], lib.gvqa_graph_layernorm_forward
    monkeypatch.setattr(lib, "gvqa_graph_layernorm_forward", lambda *a: (seen.append(a[9]), real(*a))[1])
    from graphvqa_amd.graph_layernorm import graph_layernorm
    wc, bc = torch.tensor([W], device=dev), torch.tensor([B_], device=dev)
    out = graph_layernorm(t(x, device=dev), graph, wc, bc, 1e-5, _form=form)
    assert seen[-1] is None and out.grad_fn is None and not out.requires_grad and torch.equal(out, full[0])
    out = graph_layernorm(t(x, device=dev).requires_grad_(True), graph, wc, bc, 1e-5, _form=form)
    assert seen[-1] is not None and [None if v is None else tuple(v.shape) for v in out.grad_fn.saved_tensors] == [(N, D), (1,), (nb, 2)]
    monkeypatch.undo()
    # C level, out and the workspace inside poisoned buffers: with stats == NULL the call writes out and its workspace and nothing around them;
    # with stats it writes exactly [B, 2] rows, (0, 0) for the empty graph
    G = 64
    xg = t(x, device=dev)
    obuf = torch.full((N * D + 2 * G,), 777.0, device=dev)
    outb = obuf[G:G + N * D].view(N, D)
    need = lib.gvqa_graph_layernorm_workspace_bytes(C.byref(graph.c), D)
    wbuf = torch.full((need + 1024,), 0x5A, dtype=torch.uint8, device=dev)
    _lib.check(lib.gvqa_graph_layernorm_forward(C.byref(graph.c), D, xg.data_ptr(), D, wc.data_ptr(), bc.data_ptr(), 1e-5, outb.data_ptr(), D,
                                                None, form, wbuf[512:].data_ptr(), need, _stream(dev)))
    torch.cuda.synchronize(dev)
    assert torch.equal(outb, full[0]) and bool((obuf[:G] == 777.0).all()) and bool((obuf[G + N * D:] == 777.0).all())
    assert bool((wbuf[:512] == 0x5A).all()) and bool((wbuf[512 + need:] == 0x5A).all())
    poison = torch.full((nb + 2, 2), 777.0, device=dev)
    _lib.check(lib.gvqa_graph_layernorm_forward(C.byref(graph.c), D, xg.data_ptr(), D, wc.data_ptr(), bc.data_ptr(), 1e-5, outb.data_ptr(), D,
                                                poison[1:].data_ptr(), form, wbuf[512:].data_ptr(), need, _stream(dev)))
    torch.cuda.synchronize(dev)
    assert bool((poison[0] == 777.0).all()) and bool((poison[-1] == 777.0).all()) and bool((poison[1:-1] != 777.0).all())
    assert bool((poison[1 + GR.SHAPE_SIZES.index(0)] == 0).all()), "an empty graph's stats row is (0, 0)"


# ---- sigma == 0 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_constant_graph(dev, form):
    sizes, D = [5, 3, 7], 12
    batch = GR.batch_of(sizes)
    x, dout = synth.normal((15, D), 41), synth.normal((15, D), 42)
    x[5:8] = 0.75
    ref = GR.closed_form(x, batch, 3, W, B_, dout)
    graph = _graph(batch, 15, 3, dev)
    w, b = _params(dev)
    out, dx, dw, db = _run_op(dev, x, dout, graph, form, w, b)
    assert bool((out[5:8] == B_).all()), "forward of a constant graph is the bias"
    assert all(bool(torch.isfinite(v).all()) for v in (out, dx, dw, db))
    gy = torch.from_numpy(dout[5:8]).double() * W
    assert GR.rel(dx[5:8], (gy - gy.mean()) / 1e-5) < GRAD_TOL
    _check((out, dx, dw, db), ref)


# ---- encoder ---------------------------------------------------------------------------------------------------------------------------
def test_encoder_training_path_on_the_config1_debug_batch(dev):
    """The encoder's training forward runs graph_layernorm: output and parameter gradients against the fp64 oracle with the bounds of the
    end-to-end check of tests/test_gpu_backward.py (1e-4 output, 5e-4 of the gradient's scale with its floor); the eval output agrees."""
    import types
    from oracle import ref_torch as R
    from tests.util import tparams
    from graphvqa_amd.sg_encoder import GroundTruth_SceneGraph_Encoder
    meta, gg = load_golden("gat_seq_debug2_d300")
    ei, batch = gg["edge_index"], gg["batch"]
    N, E, B, V, D = batch.shape[0], ei.shape[1], 2, 50, 64
    x_tok = synth.randint(N * 12, 71, 0, V, stream=9).reshape(N, 12)
    e_tok = synth.randint(E, 72, 1, V, stream=9).reshape(E, 1)
    added = np.array([3, 17, 60], dtype=np.int64)
    w1, w2 = synth.normal((N, D), 76), synth.normal((E, D), 77)
    pe = synth.encoder_params(V, D, seed=1)
    enc = GroundTruth_SceneGraph_Encoder(V, 0, D)
    enc.load_state_dict({k: t(v) for k, v in pe.items()})
    enc.to(dev).eval()       # (the encoder has no mode-dependent layer: it takes its differentiable path whenever grad mode is on and a parameter
                             #  requires a gradient, sg_encoder.py forward -- the call below -- and the fused eval call under no_grad, further down)
    data = types.SimpleNamespace(x=t(x_tok, device=dev), edge_attr=t(e_tok, device=dev), edge_index=t(ei, device=dev),
                                 batch=t(batch, device=dev), added_sym_edge=t(added, device=dev))
    xe, ee, _ = enc(data)
    assert xe.requires_grad
    ((xe * t(w1, device=dev)).sum() + (ee * t(w2, device=dev)).sum()).backward()
    rp = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in tparams(pe).items()}
    rxe, ree = R.scene_graph_encoder(t(x_tok), t(ei), t(e_tok), t(added), t(batch), B, rp)
    ((rxe * t(w1).double()).sum() + (ree * t(w2).double()).sum()).backward()
    assert GR.maxabs(xe, rxe) < 1e-4 and GR.maxabs(ee, ree) < 1e-4
    floor = 1e-3 * max(float(v.grad.abs().max()) for v in rp.values() if isinstance(v, torch.Tensor) and v.requires_grad and v.grad is not None)
    bad = {}
    for k, v in enc.named_parameters():
        rg = rp[k].grad.clone()
        if k == "sg_vocab_embedding.weight":
            rg[0] = 0
        e = GR.maxabs(v.grad, rg) / max(float(rg.abs().max()), floor)
        if not e < 5e-4:
            bad[k] = e
    assert not bad, bad
    with torch.no_grad():
        xv, ev, _ = enc(data)
    assert GR.maxabs(xv, rxe) < 1e-4 and GR.maxabs(ev, ree) < 1e-4 and GR.maxabs(xv, xe) < 1e-4


# ---- error paths -------------------------------------------------------------------------------------------------------------------------
def test_error_codes(dev):
    from graphvqa_amd import _lib
    lib = _lib.load()
    D = 8
    graph = _graph(GR.batch_of([3, 2]), 5, 2, dev)
    x, out = torch.zeros((5, D), device=dev), torch.zeros((5, D), device=dev)
    st = torch.zeros((2, 2), device=dev)
    need = lib.gvqa_graph_layernorm_workspace_bytes(C.byref(graph.c), D)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    err = lambda: lib.gvqa_last_error().decode()
    g = C.byref(graph.c)
    fwd = lambda D_, xp, nbytes: lib.gvqa_graph_layernorm_forward(g, D_, xp, D, None, None, 1e-5, out.data_ptr(), D, None, 0, ws.data_ptr(), nbytes, None)
    bwd = lambda D_, xp, nbytes: lib.gvqa_graph_layernorm_backward(g, D_, xp, D, out.data_ptr(), D, None, 1e-5, st.data_ptr(), out.data_ptr(), D, None, None,
                                                                   0, ws.data_ptr(), nbytes, None)
    for call in (fwd, bwd):
        assert call(D, x.data_ptr(), need - 1) == _lib.E_WORKSPACE and "workspace" in err()
        assert call(D, None, need) == _lib.E_INVALID and "null" in err()
        assert call(0, x.data_ptr(), need) == _lib.E_INVALID and err()
    assert lib.gvqa_graph_layernorm_forward(g, D, x.data_ptr(), D, None, None, 1e-5, out.data_ptr(), D, None, 3, ws.data_ptr(), need, None) == _lib.E_INVALID
    assert lib.gvqa_graph_layernorm_forward(g, D, x.data_ptr(), D - 1, None, None, 1e-5, out.data_ptr(), D, None, 0, ws.data_ptr(), need, None) == _lib.E_INVALID
    empty = _lib.Graph()
    empty.valid = empty.finalized = 1                                                     # no graphs, no nodes
    assert lib.gvqa_graph_layernorm_forward(C.byref(empty), D, None, D, None, None, 1e-5, None, D, None, 0, None, 0, None) == _lib.GVQA_OK
    with pytest.raises(TypeError):
        from graphvqa_amd.graph_layernorm import graph_layernorm
        graph_layernorm(x.double(), graph)
    with pytest.raises(RuntimeError):
        graph_layernorm(x.cpu(), graph)
