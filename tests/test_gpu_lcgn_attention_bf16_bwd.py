"""GPU checks of the differentiable bf16 LCGN attention (gvqa_lcgn_attention_bf16_train / gvqa_lcgn_attention_bf16_backward behind
graphvqa_amd.lcgn.lcgn_attention_bf16 and lcgn_seq's bf16 training road): gradients against the dense fp64 restatement of
include/gvqa.h's formulas on the bf16 values of J, the training forward against the inference kernel bit for bit, determinism, the
edge cases, what autograd saves, and lcgn_seq's new road against the one it replaces (same seed, same mask, same rounded values).

Operands: tests/test_gpu_lcgn_heads_bf16.py::_kernel_case.  Bounds: those of tests/test_gpu_lcgn_attention_bwd.py (out 1e-5 x
max(1, |ref|max), alpha 1e-5, gradients 5e-4 relative under _grad_errors' floor) -- the kernels do fp32 arithmetic on values that
are exact in fp32, so the fp32 kernels' bounds apply; the reference is that file's _dense_ref in fp64 on J.bfloat16().double()."""
import ctypes as C

import pytest
import torch

from graphvqa_amd import synth
from tests.test_gpu_lcgn_attention_bwd import _dense_ref, _mask, _grad_errors, GRAD_TOL, SLOPE
from tests.test_gpu_lcgn_heads_bf16 import _kernel_case
from tests.util import t, maxabs

pytestmark = pytest.mark.gpu

CASES = [(1, 512, False), (4, 512, False), (4, 512, True), (3, 24, True), (8, 8, False), (2, 1032, False), (1, 2056, True)]
NAMES = ("dJ", "dpc", "dbias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _fp64_reference(J16, pc, bias, graph, H, Cc, concat, mask, w):
    """(out, alpha, {dJ, dpc, dbias}) of the dense fp64 form on the bf16 values of J, loss (out * w).sum()."""
    ei, batch = (v.cpu() for v in graph._keep)
    rs = [v.detach().cpu().double().requires_grad_(True) for v in (J16.float(), pc, bias)]
    ref, ref_alpha = _dense_ref(rs[0], rs[1], ei, batch, H, Cc, concat, rs[2], None if mask is None else mask.double())
    (ref * w.double()).sum().backward()
    return ref.detach(), ref_alpha.detach(), dict(zip(NAMES, (r.grad for r in rs)))


def _straight_through(J16, pc, bias, graph, H, Cc, concat, mask, w):
    """The node on an fp32 J (rounded inside, straight-through gradient): (out, alpha, {dJ, dpc, dbias})."""
    from graphvqa_amd.lcgn import _lcgn_attention_store_bf16
    ops = [v.detach().clone().requires_grad_(True) for v in (J16.float(), pc, bias)]
    out, alpha = _lcgn_attention_store_bf16(ops[0], ops[1], graph, H, Cc, concat, SLOPE, ops[2], mask)
    assert out.requires_grad and not alpha.requires_grad and out.dtype == torch.float32
    (out * w.to(out.device)).sum().backward()
    return out.detach(), alpha, dict(zip(NAMES, (o.grad for o in ops)))


def _bf16_leaf(J16, pc, bias, graph, H, Cc, concat, mask, w):
    from graphvqa_amd.lcgn import lcgn_attention_bf16
    ops = [v.detach().clone().requires_grad_(True) for v in (J16, pc, bias)]
    out, alpha = lcgn_attention_bf16(ops[0], ops[1], graph, H, Cc, concat, SLOPE, ops[2], want_alpha=True, out_dtype=torch.float32,
                                     mask=mask)
    assert out.requires_grad and not alpha.requires_grad and out.dtype == torch.float32
    (out * w.to(out.device)).sum().backward()
    return out.detach(), alpha, dict(zip(NAMES, (o.grad for o in ops)))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,Cc,concat", CASES)
def test_gradients_match_fp64(dev, H, Cc, concat, masked):
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, concat)
    for kind, graph in zip(("intra", "cross"), graphs):
        mask = _mask(graph.num_edges, H, 77) if masked else None
        dmask = None if mask is None else mask.to(dev)
        w = t(synth.normal((graph.num_nodes, H * Cc if concat else Cc), 9))
        ref, ref_alpha, want = _fp64_reference(J16, pc, bias, graph, H, Cc, concat, mask, w)
        out, alpha, got = _straight_through(J16, pc, bias, graph, H, Cc, concat, dmask, w)
        e_out, e_alpha, errs = maxabs(out, ref), maxabs(alpha, ref_alpha), _grad_errors(got, want)
        print(f"H={H} C={Cc} concat={concat} masked={masked} {kind}: out {e_out:.3g} alpha {e_alpha:.3g} grads {errs}")
        assert got["dJ"].dtype == torch.float32
        assert e_out < 1e-5 * max(1.0, float(ref.abs().max())), kind
        assert e_alpha < 1e-5, kind
        bad = {k: e for k, e in errs.items() if not e < GRAD_TOL}
        assert not bad, (kind, bad)
        # a bf16 leaf: the same kernels on the same values, dJ rounded once to bf16
        out16, alpha16, got16 = _bf16_leaf(J16, pc, bias, graph, H, Cc, concat, dmask, w)
        assert got16["dJ"].dtype == torch.bfloat16
        assert torch.equal(got16["dJ"], got["dJ"].bfloat16()), kind
        assert torch.equal(out16, out) and torch.equal(alpha16, alpha), kind
        assert torch.equal(got16["dpc"], got["dpc"]) and torch.equal(got16["dbias"], got["dbias"]), kind


@pytest.mark.parametrize("H,Cc,concat", CASES)
def test_training_forward_without_mask_is_the_inference_kernel(dev, H, Cc, concat):
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream
    lib = _lib.load()
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, concat)
    N, HC = J16.shape[0], H * Cc
    cout = HC if concat else Cc
    for graph in graphs:
        E = graph.num_edges
        outs = [torch.full((N, cout), float("nan"), device=dev) for _ in range(2)]
        alphas = [torch.full((E, H), float("nan"), device=dev) for _ in range(2)]
        _lib.check(lib.gvqa_lcgn_attention_bf16(C.byref(graph.c), H, Cc, int(concat), SLOPE, J16.data_ptr(), 3 * HC, pc.data_ptr(), 2 * HC,
                                                bias.data_ptr(), outs[0].data_ptr(), cout, 0, alphas[0].data_ptr(), _stream(dev)))
        _lib.check(lib.gvqa_lcgn_attention_bf16_train(C.byref(graph.c), H, Cc, int(concat), SLOPE, J16.data_ptr(), 3 * HC, pc.data_ptr(),
                                                      2 * HC, bias.data_ptr(), None, outs[1].data_ptr(), cout, alphas[1].data_ptr(),
                                                      _stream(dev)))
        torch.cuda.synchronize()
        assert not torch.isnan(outs[0]).any() and not torch.isnan(alphas[0]).any()
        assert torch.equal(outs[0], outs[1]) and torch.equal(alphas[0], alphas[1])


@pytest.mark.parametrize("H,Cc,concat", [(4, 512, False), (4, 512, True), (3, 24, True), (1, 2056, True)])
def test_backward_is_deterministic(dev, H, Cc, concat):
    from graphvqa_amd.lcgn import lcgn_attention_bf16
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, concat)
    graph = graphs[1]
    Jd, pcd = (v.detach().clone().requires_grad_(True) for v in (J16, pc))
    mask = _mask(graph.num_edges, H, 78).to(dev)
    out, _ = lcgn_attention_bf16(Jd, pcd, graph, H, Cc, concat, SLOPE, None, out_dtype=torch.float32, mask=mask)
    w = t(synth.normal(tuple(out.shape), 9), device=dev)
    a = torch.autograd.grad(out, (Jd, pcd), w, retain_graph=True)
    b = torch.autograd.grad(out, (Jd, pcd), w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0].float().abs().max()) > 0 and float(a[1].abs().max()) > 0


@pytest.mark.parametrize("H,Cc,concat", [(1, 8, False), (4, 8, False), (4, 8, True)])
def test_empty_graph_and_isolated_nodes(dev, H, Cc, concat):
    """synth.lcgn_test_batch: graph 1 has no nodes, node 2 no in-edges.  Node 2's output row is the bias; where fp64 gives an
    exact zero (the empty graph's dpc row, d x_r of a node without in-edges, d x_l / d x_val of a node without out-edges) the
    kernels give an exact zero; nothing is NaN."""
    from graphvqa_amd.graph import SceneGraphBatch
    for cross in (False, True):
        gb = synth.lcgn_test_batch(5, cross_graph=cross)
        N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
        assert 1 not in set(gb.batch.tolist()) and 2 not in set(gb.edge_index[1].tolist())
        graph = SceneGraphBatch(t(gb.edge_index, device=dev), t(gb.batch, device=dev), N, B)
        J16 = t(synth.normal((N, 3 * HC), 21), device=dev).bfloat16()
        pc = t(synth.normal((B, 2 * HC), 22), device=dev)
        bias = t(synth.normal((HC if concat else Cc,), 23), device=dev)
        mask = _mask(gb.num_edges, H, 5)
        w = t(synth.normal((N, HC if concat else Cc), 9))
        ref, ref_alpha, want = _fp64_reference(J16, pc, bias, graph, H, Cc, concat, mask, w)
        out, alpha, got = _straight_through(J16, pc, bias, graph, H, Cc, concat, mask.to(dev), w)
        assert maxabs(out, ref) < 1e-5 * max(1.0, float(ref.abs().max())) and maxabs(alpha, ref_alpha) < 1e-5
        assert torch.equal(out[2], bias)
        for v in (out, alpha, *got.values()):
            assert not torch.isnan(v).any()
        bad = {k: e for k, e in _grad_errors(got, want).items() if not e < GRAD_TOL}
        assert not bad, bad
        for k in ("dJ", "dpc"):
            zero = want[k] == 0
            assert bool(zero.any()) and float(got[k].cpu()[zero].abs().max()) == 0.0, k
        assert float(got["dpc"][1].abs().max()) == 0.0 and float(got["dJ"][2, HC:2 * HC].abs().max()) == 0.0


def test_noncontiguous_dout_is_copied(dev):
    from graphvqa_amd.graph import SceneGraphBatch
    from graphvqa_amd.lcgn import lcgn_attention_bf16
    H, Cc = 4, 8
    gb = synth.lcgn_test_batch(5)
    N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
    graph = SceneGraphBatch(t(gb.edge_index, device=dev), t(gb.batch, device=dev), N, B)
    Jd = t(synth.normal((N, 3 * HC), 21), device=dev).bfloat16().requires_grad_(True)
    pcd = t(synth.normal((B, 2 * HC), 22), device=dev).requires_grad_(True)
    out, _ = lcgn_attention_bf16(Jd, pcd, graph, H, Cc, True, SLOPE, out_dtype=torch.float32)
    wide = t(synth.normal((N, 2 * HC + 1), 9), device=dev)
    for view in (wide[:, 0:2 * HC:2], wide[:, 1:HC + 1], wide.t()[1:HC + 1].t()):
        assert not view.is_contiguous()
        a = torch.autograd.grad(out, (Jd, pcd), view, retain_graph=True)
        b = torch.autograd.grad(out, (Jd, pcd), view.contiguous(), retain_graph=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert float(a[0].float().abs().max()) > 0


def _record_saved(fn):
    saved = []

    def pack(v):
        saved.append((tuple(v.shape), v.dtype))
        return v

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda v: v):
        res = fn()
    return res, saved


def test_attention_saves_J_as_bf16_only(dev):
    from graphvqa_amd.lcgn import lcgn_attention_bf16, _lcgn_attention_store_bf16
    H, Cc = 4, 16
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, False)
    shape = tuple(J16.shape)
    leaf = J16.detach().clone().requires_grad_(True)
    (out, _), saved = _record_saved(lambda: lcgn_attention_bf16(leaf, pc, graphs[0], H, Cc, False, SLOPE, bias, out_dtype=torch.float32))
    assert out.requires_grad
    assert saved.count((shape, torch.bfloat16)) == 1 and (shape, torch.float32) not in saved, saved
    J32 = J16.float().requires_grad_(True)
    (out, _), saved = _record_saved(lambda: _lcgn_attention_store_bf16(J32, pc, graphs[0], H, Cc, False, SLOPE, bias))
    assert out.requires_grad
    assert saved.count((shape, torch.bfloat16)) == 1 and (shape, torch.float32) not in saved, saved


def _seq_module(Din, O, H, dev, seed, dropout=0.0):
    from graphvqa_amd.lcgn import lcgn_seq
    p = synth.lcgn_seq_params(Din, O, seed=seed, cmd_dim=O, question_dim=O, heads=H)
    m = lcgn_seq(Din, O, Din, 5, gat_cmd_dim=O, question_dim=O, gat_heads=H, dropout=dropout, node_feature_dtype=torch.bfloat16)
    m.load_state_dict({k: t(v) for k, v in p.items()}, strict=False)
    return m.to(dev).train()


def test_lcgn_seq_training_saves_J_as_bf16_only(dev):
    """The 12-graph batch of tests/test_gpu_lcgn_heads_bf16.py::test_lcgn_seq_bf16_heads_are_trainable: one bf16 [N, 3 H O] tensor
    saved per iteration's attention, no fp32 tensor of that shape anywhere in the graph."""
    H = 2
    gb = synth.make_graph_batch(12, seed=0xBF16, nodes_lo=4, nodes_hi=20, rel_per_node=1.5)
    N, B, O, L, Din = gb.num_nodes, gb.num_graphs, 64, 6, 40
    m = _seq_module(Din, O, H, dev, 21)
    x, q, lstm, xc = synth.normal((N, Din), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3), synth.normal((N, O), 4)
    ei, b = t(gb.edge_index, device=dev), t(gb.batch, device=dev)
    out, saved = _record_saved(lambda: m(t(x, device=dev), ei, b, t(q, device=dev), t(lstm, device=dev), x_ctx_init=t(xc, device=dev)))
    assert out.requires_grad
    shape = (N, 3 * H * O)
    assert saved.count((shape, torch.bfloat16)) == m.MAX_ITER_NUM, saved
    assert (shape, torch.float32) not in saved, saved


def test_lcgn_seq_with_dropout_matches_the_fp32_attention_road(dev, monkeypatch):
    """lcgn_seq(gat_heads = 2, bf16, dropout 0.1).train(), the shapes of
    tests/test_gpu_lcgn_attention_bwd.py::test_lcgn_seq_with_dropout_matches_the_composition and its bounds: the new road (J rounded
    and saved as bf16 inside the bf16 attention node) against today's (_StoreBf16, then the fp32 node), reached by making
    _attention_bf16_supported answer False.  One torch seed: the same mask; the same rounded values."""
    from graphvqa_amd import lcgn
    H = 2
    gb = synth.make_graph_batch(5, seed=0x1C6, nodes_lo=4, nodes_hi=14, rel_per_node=1.5)
    N, B, O, L = gb.num_nodes, gb.num_graphs, 32, 6
    m = _seq_module(20, O, H, dev, 11, dropout=0.1)
    x, q, lstm, xc, w = (synth.normal((N, 20), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3), synth.normal((N, O), 4),
                         synth.normal((N, O), 5))
    ei, b = t(gb.edge_index, device=dev), t(gb.batch, device=dev)
    J_bf16 = ((N, 3 * H * O), torch.bfloat16)

    def step():
        xs = [t(a, device=dev).requires_grad_(True) for a in (x, q, lstm)]
        m.zero_grad()
        torch.manual_seed(4321)
        out, saved = _record_saved(lambda: m(xs[0], ei, b, xs[1], xs[2], x_ctx_init=t(xc, device=dev)))
        (out * t(w, device=dev)).sum().backward()
        grads = {"x": xs[0].grad, "q": xs[1].grad, "lstm": xs[2].grad}
        grads.update({k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None})
        return (out.detach(), grads), saved.count(J_bf16)

    new, n_bf16 = step()
    assert n_bf16 == m.MAX_ITER_NUM                          # the new road: J saved as bf16, once per iteration
    monkeypatch.setattr(lcgn, "_attention_bf16_supported", lambda heads, channels: False)
    old, n_bf16 = step()
    assert n_bf16 == 0                                       # today's road
    assert set(new[1]) == set(old[1]) and "lcgn.lin_l.weight" in new[1]
    (out, grads), (ref, ref_grads) = new, old
    e_out = maxabs(out, ref)
    errs = _grad_errors(grads, {k: v.detach().cpu().double() for k, v in ref_grads.items()})
    print(f"lcgn_seq H=2 bf16: out {e_out:.3g} (|ref| {float(ref.abs().max()):.3g}) grads max {max(errs.values()):.3g}")
    assert e_out < 1e-5 * max(1.0, float(ref.abs().max()))
    bad = {k: e for k, e in errs.items() if not e < GRAD_TOL}
    assert not bad, bad


def test_differentiable_call_refuses_bf16_output_and_out_views(dev):
    from graphvqa_amd.lcgn import lcgn_attention_bf16
    H, Cc = 4, 16
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, False)
    N = J16.shape[0]
    msg = r"out_dtype must be torch\.float32 and out must be None when gradients are needed or a mask is given"
    leaf = J16.detach().clone().requires_grad_(True)
    with pytest.raises(ValueError, match=msg):
        lcgn_attention_bf16(leaf, pc, graphs[0], H, Cc, False, SLOPE, bias)                              # out_dtype: bfloat16
    with pytest.raises(ValueError, match=msg):
        lcgn_attention_bf16(leaf, pc, graphs[0], H, Cc, False, SLOPE, bias, out_dtype=torch.float32,
                            out=torch.empty((N, 2 * Cc), device=dev)[:, Cc:])
    with pytest.raises(ValueError, match=msg), torch.no_grad():                                          # a mask alone asks for it too
        lcgn_attention_bf16(J16, pc, graphs[0], H, Cc, False, SLOPE, bias, mask=_mask(graphs[0].num_edges, H, 3).to(dev))
    with torch.no_grad():                           # without gradients and without a mask: as before
        o16, _ = lcgn_attention_bf16(leaf, pc, graphs[0], H, Cc, False, SLOPE, bias)
    assert o16.dtype == torch.bfloat16 and not o16.requires_grad


@pytest.mark.parametrize("H,Cc,concat", [(3, 12, True), (2, 12, False)])
def test_shape_outside_the_bf16_limits_trains_on_the_fp32_kernels(dev, H, Cc, concat):
    """C % 8 != 0: lcgn_attention(J16.float(), ..., mask=mask), now with gradients: dJ (fp32, as that call computes it), dpc and
    dbias within GRAD_TOL of fp64; J16.grad is that dJ rounded once to bf16 by autograd on its way through J16.float()."""
    from graphvqa_amd.lcgn import _attention_bf16_supported, lcgn_attention
    assert not _attention_bf16_supported(H, Cc)
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, concat)
    for kind, graph in zip(("intra", "cross"), graphs):
        mask = _mask(graph.num_edges, H, 77)
        w = t(synth.normal((graph.num_nodes, H * Cc if concat else Cc), 9))
        ref, ref_alpha, want = _fp64_reference(J16, pc, bias, graph, H, Cc, concat, mask, w)
        out, alpha, got = _bf16_leaf(J16, pc, bias, graph, H, Cc, concat, mask.to(dev), w)
        assert maxabs(out, ref) < 1e-5 * max(1.0, float(ref.abs().max())) and maxabs(alpha, ref_alpha) < 1e-5
        J32 = J16.float().requires_grad_(True)
        out32, _ = lcgn_attention(J32, pc, graph, H, Cc, concat, SLOPE, bias, mask=mask.to(dev))
        (out32 * w.to(dev)).sum().backward()
        assert torch.equal(out32.detach(), out)
        errs = _grad_errors({"dJ": J32.grad, "dpc": got["dpc"], "dbias": got["dbias"]}, want)
        print(f"fallback H={H} C={Cc} {kind}: {errs}")
        bad = {k: e for k, e in errs.items() if not e < GRAD_TOL}
        assert not bad, (kind, bad)
        assert got["dJ"].dtype == torch.bfloat16 and torch.equal(got["dJ"], J32.grad.bfloat16()), kind
