"""GPU checks of the differentiable LCGN attention (gvqa_lcgn_attention_train / gvqa_lcgn_attention_backward behind
graphvqa_amd.lcgn.lcgn_attention): gradients against a dense fp64 restatement of the formulas in include/gvqa.h, the training
forward against the inference kernel bit for bit, determinism, the composition it replaces (with dropout, same seed), the
recorded reference gradients (tests/golden/lcgn_heads_grads.npz) and the edge cases.

Bounds.  Gradients: relative error below 5e-4 with the floor 1e-3 x the largest gradient entry (the bound of
tests/test_gpu_lcgn_heads.py::_grad_case_layer).  Kernel outputs: 1e-5 x max(1, |ref|max); alpha: 1e-5 (the bounds of
test_attention_kernel_matches_the_composition).  Outputs against the recorded reference: 1e-4 (the project's parity bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from tests.lcgn_ref import _dense_ref, _mask, _grad_errors, GRAD_TOL, SLOPE
from tests.test_lcgn_heads_host import _layer_oracle
from tests.util import load_golden, t, tparams, maxabs

pytestmark = pytest.mark.gpu

CASES = [(1, 512, False), (4, 512, False), (4, 512, True), (3, 20, True), (8, 8, False), (2, 1028, False), (1, 2052, True)]
PARAMS = ("lin_l.weight", "lin_r.weight", "cal_x.weight", "proj_cmd.weight", "cal_cmd.weight", "bias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _operands(H, Cc, concat, dev):
    gb = synth.make_graph_batch(6, seed=0xA77, nodes_lo=1, nodes_hi=12, rel_per_node=1.5)
    N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
    J, pc = synth.normal((N, 3 * HC), 11) * np.float32(0.3), synth.normal((B, 2 * HC), 12) * np.float32(0.3)
    bias = synth.normal((HC if concat else Cc,), 13)
    cross = gb.edge_index.copy()
    cross[0, ::7] = (cross[0, ::7] + 5) % N
    return gb, J, pc, bias, (gb.edge_index, cross)


def _run_pair(J, pc, bias, ei, batch, N, B, H, Cc, concat, mask, dev, wseed=9):
    """lcgn_attention on the GPU and the dense fp64 form, loss (out * w).sum(): (out, alpha, grads) of each."""
    from graphvqa_amd.graph import SceneGraphBatch
    from graphvqa_amd.lcgn import lcgn_attention
    graph = SceneGraphBatch(t(ei, device=dev), t(batch, device=dev), N, B)
    ops = [t(a, device=dev).requires_grad_(True) for a in (J, pc, bias)]
    out, alpha = lcgn_attention(ops[0], ops[1], graph, H, Cc, concat, SLOPE, ops[2], want_alpha=True,
                                mask=None if mask is None else mask.to(dev))
    assert out.requires_grad and not alpha.requires_grad
    w = synth.normal(tuple(out.shape), wseed)
    (out * t(w, device=dev)).sum().backward()
    rs = [t(a).double().requires_grad_(True) for a in (J, pc, bias)]
    ref, ref_alpha = _dense_ref(rs[0], rs[1], t(ei), t(batch), H, Cc, concat, rs[2], None if mask is None else mask.double())
    (ref * t(w).double()).sum().backward()
    names = ("dJ", "dpc", "dbias")
    return (out, alpha, dict(zip(names, (o.grad for o in ops)))), (ref, ref_alpha, dict(zip(names, (r.grad for r in rs))))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,Cc,concat", CASES)
def test_gradients_match_fp64(dev, H, Cc, concat, masked):
    gb, J, pc, bias, eis = _operands(H, Cc, concat, dev)
    for kind, ei in zip(("intra", "cross"), eis):
        mask = _mask(ei.shape[1], H, 77) if masked else None
        (out, alpha, got), (ref, ref_alpha, want) = _run_pair(J, pc, bias, ei, gb.batch, gb.num_nodes, gb.num_graphs, H, Cc, concat,
                                                              mask, dev)
        e_out, e_alpha, errs = maxabs(out, ref), maxabs(alpha, ref_alpha), _grad_errors(got, want)
        print(f"H={H} C={Cc} concat={concat} masked={masked} {kind}: out {e_out:.3g} alpha {e_alpha:.3g} grads {errs}")
        assert e_out < 1e-5 * max(1.0, float(ref.detach().abs().max())), kind
        assert e_alpha < 1e-5, kind
        bad = {k: e for k, e in errs.items() if not e < GRAD_TOL}
        assert not bad, (kind, bad)


@pytest.mark.parametrize("H,Cc,concat", CASES)
def test_training_forward_without_mask_is_the_inference_kernel(dev, H, Cc, concat):
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import SceneGraphBatch, _stream
    lib = _lib.load()
    gb, J, pc, bias, eis = _operands(H, Cc, concat, dev)
    N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
    cout = HC if concat else Cc
    Jd, pcd, bd = (t(a, device=dev) for a in (J, pc, bias))
    for ei in eis:
        graph = SceneGraphBatch(t(ei, device=dev), t(gb.batch, device=dev), N, B)
        E = graph.num_edges
        outs = [torch.full((N, cout), float("nan"), device=dev) for _ in range(2)]
        alphas = [torch.full((E, H), float("nan"), device=dev) for _ in range(2)]
        _lib.check(lib.gvqa_lcgn_attention(C.byref(graph.c), H, Cc, int(concat), SLOPE, Jd.data_ptr(), 3 * HC, pcd.data_ptr(), 2 * HC,
                                           bd.data_ptr(), outs[0].data_ptr(), cout, alphas[0].data_ptr(), _stream(dev)))
        _lib.check(lib.gvqa_lcgn_attention_train(C.byref(graph.c), H, Cc, int(concat), SLOPE, Jd.data_ptr(), 3 * HC, pcd.data_ptr(),
                                                 2 * HC, bd.data_ptr(), None, outs[1].data_ptr(), cout, alphas[1].data_ptr(),
                                                 _stream(dev)))
        torch.cuda.synchronize()
        assert not torch.isnan(outs[0]).any() and not torch.isnan(alphas[0]).any()
        assert torch.equal(outs[0], outs[1]) and torch.equal(alphas[0], alphas[1])


@pytest.mark.parametrize("H,Cc,concat", [(4, 512, False), (4, 512, True), (3, 20, True), (1, 2052, True)])
def test_backward_is_deterministic(dev, H, Cc, concat):
    from graphvqa_amd.graph import SceneGraphBatch
    from graphvqa_amd.lcgn import lcgn_attention
    gb, J, pc, bias, eis = _operands(H, Cc, concat, dev)
    ei = eis[1]
    graph = SceneGraphBatch(t(ei, device=dev), t(gb.batch, device=dev), gb.num_nodes, gb.num_graphs)
    Jd, pcd = (t(a, device=dev).requires_grad_(True) for a in (J, pc))
    mask = _mask(ei.shape[1], H, 78).to(dev)
    out, _ = lcgn_attention(Jd, pcd, graph, H, Cc, concat, SLOPE, None, mask=mask)
    w = t(synth.normal(tuple(out.shape), 9), device=dev)
    a = torch.autograd.grad(out, (Jd, pcd), w, retain_graph=True)
    b = torch.autograd.grad(out, (Jd, pcd), w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0


def _layer(meta, H, concat, dev, dropout=0.0, out_channels=None):
    from graphvqa_amd.lcgn import gat_lcgn
    Cc = meta["out_channels"] if out_channels is None else out_channels
    m = gat_lcgn(meta["in_channels"], Cc, 1, heads=H, concat=concat, dropout=dropout, cmd_dim=meta["cmd_dim"])
    p = synth.gat_lcgn_params(meta["in_channels"], Cc, H, meta["param_seed"] + H, meta["cmd_dim"], concat=concat)
    m.load_state_dict({k: t(v) for k, v in p.items()})
    return m.to(dev), p


def _both_roads(monkeypatch, step):
    """step() -> (out, {name: grad}) on the new road and with the composition forced."""
    from graphvqa_amd import lcgn
    monkeypatch.setattr(lcgn, "_FORCE_COMPOSITION", False)
    new = step()
    monkeypatch.setattr(lcgn, "_FORCE_COMPOSITION", True)
    old = step()
    monkeypatch.setattr(lcgn, "_FORCE_COMPOSITION", False)
    return new, old


def _assert_roads_agree(new, old, what):
    (out, grads), (ref, ref_grads) = new, old
    e_out = maxabs(out, ref)
    errs = _grad_errors(grads, {k: v.detach().cpu().double() for k, v in ref_grads.items()})
    print(f"{what}: out {e_out:.3g} grads max {max(errs.values()):.3g}")
    assert e_out < 1e-5 * max(1.0, float(ref.abs().max())), what
    bad = {k: e for k, e in errs.items() if not e < GRAD_TOL}
    assert not bad, (what, bad)


@pytest.mark.parametrize("concat", [False, True])
def test_layer_with_dropout_matches_the_composition(dev, monkeypatch, concat):
    """gat_lcgn(heads = 4, dropout = 0.1).train(): one torch seed gives one mask on both roads, applied after the softmax."""
    meta, g = load_golden("lcgn_heads_small")
    m, _ = _layer(meta, 4, concat, dev, dropout=0.1)
    m.train()
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    s = meta["input_seeds"]
    x, cmd = synth.normal((N, meta["in_channels"]), s["x"]), synth.normal((B, meta["cmd_dim"]), s["cmd"])

    def step():
        xs = [t(a, device=dev).requires_grad_(True) for a in (x, cmd)]
        m.zero_grad()
        torch.manual_seed(1234)
        out, (_, alpha) = m(xs[0], t(g["x_edge_index"], device=dev), xs[1], t(g["batch"], device=dev), return_attention_weights=True)
        (out * t(synth.normal(tuple(out.shape), 9), device=dev)).sum().backward()
        grads = {"x": xs[0].grad, "cmd": xs[1].grad, **{k: v.grad.clone() for k, v in m.named_parameters()}}
        return out.detach(), {**grads, "alpha": alpha}

    new, old = _both_roads(monkeypatch, step)
    assert maxabs(new[1].pop("alpha"), old[1].pop("alpha")) < 1e-5
    _assert_roads_agree(new, old, f"gat_lcgn concat={concat}")
    torch.manual_seed(1234)          # the mask has an effect: the same step without it differs
    with torch.no_grad():
        plain = m.eval()(t(x, device=dev), t(g["x_edge_index"], device=dev), t(cmd, device=dev), t(g["batch"], device=dev))
    assert maxabs(plain, new[0]) > 1e-3


def test_lcgn_seq_with_dropout_matches_the_composition(dev, monkeypatch):
    from graphvqa_amd.lcgn import lcgn_seq
    H = 2
    gb = synth.make_graph_batch(5, seed=0x1C6, nodes_lo=4, nodes_hi=14, rel_per_node=1.5)
    N, B, O, L = gb.num_nodes, gb.num_graphs, 32, 6
    p = synth.lcgn_seq_params(20, O, seed=11, cmd_dim=O, question_dim=O, heads=H)
    m = lcgn_seq(20, O, 20, 5, gat_cmd_dim=O, question_dim=O, gat_heads=H, dropout=0.1)
    m.load_state_dict({k: t(v) for k, v in p.items()}, strict=False)
    m = m.to(dev).train()
    x, q, lstm, xc, w = (synth.normal((N, 20), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3), synth.normal((N, O), 4),
                         synth.normal((N, O), 5))
    ei, b = t(gb.edge_index, device=dev), t(gb.batch, device=dev)

    def step():
        xs = [t(a, device=dev).requires_grad_(True) for a in (x, q, lstm)]
        m.zero_grad()
        torch.manual_seed(4321)
        out = m(xs[0], ei, b, xs[1], xs[2], x_ctx_init=t(xc, device=dev))
        (out * t(w, device=dev)).sum().backward()
        grads = {"x": xs[0].grad, "q": xs[1].grad, "lstm": xs[2].grad}
        grads.update({k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None})
        return out.detach(), grads

    new, old = _both_roads(monkeypatch, step)
    assert set(new[1]) == set(old[1]) and "lcgn.lin_l.weight" in new[1]
    _assert_roads_agree(new, old, "lcgn_seq H=2")


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("concat", [False, True])
def test_layer_gradients_match_the_recorded_reference(dev, H, concat):
    meta, g = load_golden("lcgn_heads_grads")
    m, _ = _layer(meta, H, concat, dev)
    m.train()
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    s = meta["input_seeds"]
    for tag, ei in (("layer", g["edge_index"]), ("xlayer", g["x_edge_index"])):
        key = f"{tag}_h{H}_c{int(concat)}"
        x = t(synth.normal((N, meta["in_channels"]), s["x"]), device=dev).requires_grad_(True)
        cmd = t(synth.normal((B, meta["cmd_dim"]), s["cmd"]), device=dev).requires_grad_(True)
        m.zero_grad()
        out = m(x, t(ei, device=dev), cmd, t(g["batch"], device=dev))
        (out * t(synth.normal(tuple(out.shape), meta["loss_seed"]), device=dev)).sum().backward()
        named = dict(m.named_parameters())
        got = {"dx": x.grad, "dcmd": cmd.grad, **{"d_" + k: named[k].grad for k in PARAMS}}
        want = {k: t(g[f"{key}_{k}"]).double() for k in got}
        e_out, errs = maxabs(out, g[key + "_out"]), _grad_errors(got, want)
        print(f"{key}: out {e_out:.3g} grads {errs}")
        assert e_out < 1e-4, key
        bad = {k: e for k, e in errs.items() if not e < GRAD_TOL}
        assert not bad, (key, bad)


@pytest.mark.parametrize("H,Cc,concat", [(1, 8, False), (4, 8, False), (4, 8, True)])
def test_empty_graph_and_isolated_nodes(dev, H, Cc, concat):
    """synth.lcgn_test_batch: graph 1 has no nodes, node 2 no in-edges.  Where fp64 gives an exact zero (the empty graph's dpc row,
    d x_r of a node without in-edges, d x_l / d x_val of a node without out-edges) the kernels give an exact zero."""
    for cross in (False, True):
        gb = synth.lcgn_test_batch(5, cross_graph=cross)
        N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
        assert 1 not in set(gb.batch.tolist()) and 2 not in set(gb.edge_index[1].tolist())
        J, pc = synth.normal((N, 3 * HC), 21), synth.normal((B, 2 * HC), 22)
        bias = synth.normal((HC if concat else Cc,), 23)
        (out, alpha, got), (ref, ref_alpha, want) = _run_pair(J, pc, bias, gb.edge_index, gb.batch, N, B, H, Cc, concat,
                                                              _mask(gb.num_edges, H, 5), dev)
        assert maxabs(out, ref) < 1e-5 * max(1.0, float(ref.detach().abs().max())) and maxabs(alpha, ref_alpha) < 1e-5
        bad = {k: e for k, e in _grad_errors(got, want).items() if not e < GRAD_TOL}
        assert not bad, bad
        for k in ("dJ", "dpc"):
            zero = want[k] == 0
            assert bool(zero.any()) and float(got[k].cpu()[zero].abs().max()) == 0.0, k
        assert float(want["dpc"][1].abs().max()) == 0.0 and float(want["dJ"][2, HC:2 * HC].abs().max()) == 0.0


def test_noncontiguous_dout_is_copied(dev):
    from graphvqa_amd.graph import SceneGraphBatch
    from graphvqa_amd.lcgn import lcgn_attention
    H, Cc = 4, 8
    gb = synth.lcgn_test_batch(5)
    N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
    graph = SceneGraphBatch(t(gb.edge_index, device=dev), t(gb.batch, device=dev), N, B)
    Jd = t(synth.normal((N, 3 * HC), 21), device=dev).requires_grad_(True)
    pcd = t(synth.normal((B, 2 * HC), 22), device=dev).requires_grad_(True)
    out, _ = lcgn_attention(Jd, pcd, graph, H, Cc, True, SLOPE)
    wide = t(synth.normal((N, 2 * HC + 1), 9), device=dev)
    for view in (wide[:, 0:2 * HC:2], wide[:, 1:HC + 1], wide.t()[1:HC + 1].t()):
        assert not view.is_contiguous()
        a = torch.autograd.grad(out, (Jd, pcd), view, retain_graph=True)
        b = torch.autograd.grad(out, (Jd, pcd), view.contiguous(), retain_graph=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_shape_outside_the_limits_trains_through_the_composition(dev):
    """C = 6 is not a multiple of 4: gvqa_lcgn_attention_train would refuse it, the layer still trains (the composition)."""
    meta, g = load_golden("lcgn_heads_small")
    H, Cc = 2, 6
    m, p = _layer(meta, H, False, dev, out_channels=Cc)
    m.train()
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    s = meta["input_seeds"]
    x, cmd = synth.normal((N, meta["in_channels"]), s["x"]), synth.normal((B, meta["cmd_dim"]), s["cmd"])
    xs = [t(a, device=dev).requires_grad_(True) for a in (x, cmd)]
    out = m(xs[0], t(g["x_edge_index"], device=dev), xs[1], t(g["batch"], device=dev))
    w = synth.normal(tuple(out.shape), 9)
    (out * t(w, device=dev)).sum().backward()
    rp = {k: v.double().requires_grad_(True) for k, v in tparams(p).items()}
    rs = [t(a).double().requires_grad_(True) for a in (x, cmd)]
    ref, _ = _layer_oracle(rs[0], t(g["x_edge_index"]), rs[1], t(g["batch"]), rp, H, False)
    (ref * t(w).double()).sum().backward()
    assert maxabs(out, ref) < 1e-4
    got = {"x": xs[0].grad, "cmd": xs[1].grad, **{k: v.grad for k, v in m.named_parameters()}}
    want = {"x": rs[0].grad, "cmd": rs[1].grad, **{k: rp[k].grad for k in rp}}
    bad = {k: e for k, e in _grad_errors(got, want).items() if not e < GRAD_TOL}
    assert not bad, bad
