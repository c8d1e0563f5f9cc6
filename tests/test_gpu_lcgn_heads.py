"""GPU checks of the multi-head LCGN surface: the gat_lcgn layer on its own (gvqa_gat_lcgn_forward), lcgn_seq(gat_heads > 1), their
differentiable forms, and the attention kernel against the composition it replaces.  Oracles: the recorded reference fixture
(tests/golden/lcgn_heads_small.npz) and oracle/ref_torch.py."""
import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from oracle import ref_torch as R
from tests.test_lcgn_heads_host import _layer_oracle
from tests.util import load_golden, t, tparams, maxabs

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rel(a, b, floor=0.0):
    b = b.detach().cpu().double()
    return maxabs(a, b) / max(float(b.abs().max()), floor, 1e-12)


def _layer(meta, H, concat, dev, dropout=0.0):
    from graphvqa_amd.lcgn import gat_lcgn
    m = gat_lcgn(meta["in_channels"], meta["out_channels"], 1, heads=H, concat=concat, dropout=dropout, cmd_dim=meta["cmd_dim"])
    p = synth.gat_lcgn_params(meta["in_channels"], meta["out_channels"], H, meta["param_seed"] + H, meta["cmd_dim"], concat=concat)
    m.load_state_dict({k: t(v) for k, v in p.items()})
    return m.to(dev).eval(), p


def _layer_inputs(meta, g):
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    s = meta["input_seeds"]
    return synth.normal((N, meta["in_channels"]), s["x"]), synth.normal((B, meta["cmd_dim"]), s["cmd"])


@pytest.mark.parametrize("H", [1, 2, 4, 8])
@pytest.mark.parametrize("concat", [False, True])
def test_gat_lcgn_eval_matches_reference(dev, H, concat):
    """The layer's eval path (one C call) on the recorded batches: intra-graph (multi-edges, an empty graph, a node without
    in-edges) and with edges across graphs; out and alpha against the fixture and the oracle; alpha sums to 1 per destination;
    run to run bit-identical."""
    meta, g = load_golden("lcgn_heads_small")
    m, p = _layer(meta, H, concat, dev)
    x, cmd = _layer_inputs(meta, g)
    for tag, ei in (("layer", g["edge_index"]), ("xlayer", g["x_edge_index"])):
        args = (t(x, device=dev), t(ei, device=dev), t(cmd, device=dev), t(g["batch"], device=dev))
        with torch.no_grad():
            out, (ei_out, alpha) = m(*args, return_attention_weights=True)
            out2, (_, alpha2) = m(*args, return_attention_weights=True)
            plain = m(*args)
        key = f"{tag}_h{H}_c{int(concat)}"
        assert maxabs(out, g[key + "_out"]) < TOL, key
        assert maxabs(alpha, g[key + "_alpha"]) < 1e-5, key
        ref, ref_alpha = _layer_oracle(t(x), t(ei), t(cmd), t(g["batch"]), tparams(p), H, concat)
        assert maxabs(out, ref) < TOL and maxabs(alpha, ref_alpha) < 1e-5, key
        assert torch.equal(out, out2) and torch.equal(alpha, alpha2) and torch.equal(out, plain)
        assert ei_out.data_ptr() == args[1].data_ptr()
        dst = torch.from_numpy(ei[1])
        sums = torch.zeros(x.shape[0], H, dtype=torch.float64).index_add_(0, dst, alpha.cpu().double())
        has_in = torch.bincount(dst, minlength=x.shape[0]) > 0
        assert float((sums[has_in] - 1).abs().max()) < 1e-5
        assert float(sums[~has_in].abs().max()) == 0.0
        assert maxabs(out[2], t(p["bias"])) == 0.0                       # node 2 has no in-edges: bias alone
        assert out.shape == (x.shape[0], H * meta["out_channels"] if concat else meta["out_channels"])


def test_gat_lcgn_without_bias_and_with_a_prebuilt_graph(dev):
    from graphvqa_amd.lcgn import gat_lcgn
    from graphvqa_amd.graph import SceneGraphBatch
    meta, g = load_golden("lcgn_heads_small")
    x, cmd = _layer_inputs(meta, g)
    H = 4
    m = gat_lcgn(meta["in_channels"], meta["out_channels"], 1, heads=H, concat=False, cmd_dim=meta["cmd_dim"], bias=False)
    p = synth.gat_lcgn_params(meta["in_channels"], meta["out_channels"], H, 3, meta["cmd_dim"], bias=False)
    m.load_state_dict({k: t(v) for k, v in p.items()})
    m = m.to(dev).eval()
    ei, b = t(g["edge_index"], device=dev), t(g["batch"], device=dev)
    graph = SceneGraphBatch(ei, b, x.shape[0], cmd.shape[0])
    with torch.no_grad():
        out = m(t(x, device=dev), ei, t(cmd, device=dev), b, graph=graph)
    ref, _ = _layer_oracle(t(x), t(g["edge_index"]), t(cmd), t(g["batch"]), tparams(p), H, False)
    assert maxabs(out, ref) < TOL
    assert float(out[2].abs().max()) == 0.0


def _seq_module(in_c, O, H, p, dev):
    from graphvqa_amd.lcgn import lcgn_seq
    m = lcgn_seq(in_c, O, in_c, 5, gat_cmd_dim=O, question_dim=O, gat_heads=H)
    missing, unexpected = m.load_state_dict({k: t(v) for k, v in p.items()}, strict=False)
    assert not unexpected and all(k.startswith("bns.") for k in missing), (missing, unexpected)
    return m.to(dev).eval()


@pytest.fixture(params=["split2h", "f32"])
def projection(request):
    from graphvqa_amd import _lib
    old = _lib.set_option(_lib.OPT_PROJECTION, _lib.PROJECTION_SPLIT2H if request.param == "split2h" else _lib.PROJECTION_F32)
    yield request.param
    _lib.set_option(_lib.OPT_PROJECTION, old)


@pytest.mark.parametrize("H", [2, 4])
def test_lcgn_seq_heads_small_vs_reference(dev, H, projection):
    meta, g = load_golden("lcgn_heads_small")
    sq, s = meta["seq"], meta["input_seeds"]
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    O = sq["out_channels"]
    p = synth.lcgn_seq_params(sq["in_channels"], O, seed=sq["param_seed"] + H, cmd_dim=O, question_dim=O, heads=H)
    m = _seq_module(sq["in_channels"], O, H, p, dev)
    x, q, lstm = synth.normal((N, sq["in_channels"]), s["seq_x"]), synth.normal((B, O), s["q"]), synth.normal((sq["L"], B, O), s["lstm"])
    args = [t(a, device=dev) for a in (x, g["edge_index"], g["batch"], q, lstm)]
    torch.manual_seed(sq["torch_seed"])            # the module draws x_ctx like the reference (lcgn.py:306)
    with torch.no_grad():
        out = m(*args)
        out2 = m(*args, x_ctx_init=t(g["seq_x_ctx_init"], device=dev))
    assert maxabs(out, g[f"seq_h{H}_out"]) < TOL
    ref = R.lcgn_seq(t(x), t(g["edge_index"]), t(g["batch"]), t(q), t(lstm), tparams(p), t(g["seq_x_ctx_init"]), heads=H)
    assert maxabs(out, ref) < TOL and torch.equal(out, out2)


_CFG5 = {}


def _cfg5_case():
    """BASELINE config 5's shape with H = 4: the config-2 batch, lcgn_seq(in=300, out=512, cmd=512, 4 iterations), L = 10; the fp32
    oracle computed once for both arithmetic modes."""
    if not _CFG5:
        gb = synth.config2_batch()
        N, B, O, L = gb.num_nodes, gb.num_graphs, 512, 10
        p = synth.lcgn_seq_params(300, O, seed=808, heads=4)
        x, q, lstm, xc = synth.normal((N, 300), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3), synth.normal((N, O), 4)
        ref = R.lcgn_seq(t(x), t(gb.edge_index), t(gb.batch), t(q), t(lstm), tparams(p), t(xc), heads=4)
        _CFG5.update(gb=gb, p=p, inputs=(x, gb.edge_index, gb.batch, q, lstm), xc=xc, ref=ref)
    return _CFG5


def test_lcgn_seq_heads_config5_shape_vs_oracle(dev, projection):
    c = _cfg5_case()
    m = _seq_module(300, 512, 4, c["p"], dev)
    with torch.no_grad():
        out = m(*[t(a, device=dev) for a in c["inputs"]], x_ctx_init=t(c["xc"], device=dev))
    assert maxabs(out, c["ref"]) < TOL


def _grad_case_layer(dev, concat):
    """gat_lcgn's differentiable form (dropout 0): gradients of every parameter and input against fp64 autograd through the
    oracle, on the cross-graph batch; the bounds of test_gpu_backward.py::test_lcgn_seq_gradients_vs_oracle."""
    meta, g = load_golden("lcgn_heads_small")
    H = 4
    m, p = _layer(meta, H, concat, dev)
    x, cmd = _layer_inputs(meta, g)
    rng = np.random.default_rng(7)
    p["bias"] = (p["bias"] + 0.1 * rng.standard_normal(p["bias"].shape)).astype(np.float32)
    m.load_state_dict({k: t(v) for k, v in p.items()})
    m.train()
    xs = [t(a, device=dev).requires_grad_(True) for a in (x, cmd)]
    ei, b = g["x_edge_index"], g["batch"]
    out, (_, alpha) = m(xs[0], t(ei, device=dev), xs[1], t(b, device=dev), return_attention_weights=True)
    w = synth.normal(tuple(out.shape), 9)
    (out * t(w, device=dev)).sum().backward()
    rp = {k: v.double().requires_grad_(True) for k, v in tparams(p).items()}
    rs = [t(a).double().requires_grad_(True) for a in (x, cmd)]
    ref, ref_alpha = _layer_oracle(rs[0], t(ei), rs[1], t(b), rp, H, concat)
    (ref * t(w).double()).sum().backward()
    assert maxabs(out, ref) < TOL and maxabs(alpha, ref_alpha) < 1e-5
    floor = 1e-3 * max(float(v.grad.abs().max()) for v in list(rp.values()) + rs)
    bad = {name: _rel(got.grad, r.grad, floor) for got, r, name in zip(xs, rs, ("x", "cmd"))}
    for k, v in m.named_parameters():
        bad[k] = _rel(v.grad, rp[k].grad, floor)
    bad = {k: e for k, e in bad.items() if not e < 5e-4}
    assert not bad, bad
    with torch.no_grad():
        ev = m.eval()(xs[0], t(ei, device=dev), xs[1], t(b, device=dev))
    assert maxabs(ev, out) < TOL                 # train() with dropout 0 == eval()


@pytest.mark.parametrize("concat", [False, True])
def test_gat_lcgn_gradients_vs_oracle(dev, concat):
    _grad_case_layer(dev, concat)


def test_lcgn_seq_heads_gradients_vs_oracle(dev):
    from graphvqa_amd.lcgn import lcgn_seq
    H = 2
    gb = synth.make_graph_batch(5, seed=0x1C6, nodes_lo=4, nodes_hi=14, rel_per_node=1.5)
    N, B, O, L = gb.num_nodes, gb.num_graphs, 32, 6
    p = synth.lcgn_seq_params(20, O, seed=11, cmd_dim=O, question_dim=O, heads=H)
    rng = np.random.default_rng(3)
    for k in list(p):
        if k.endswith("bias"):
            p[k] = (p[k] + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    m = _seq_module(20, O, H, p, dev).train()
    x, q, lstm, xc, w = (synth.normal((N, 20), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3),
                         synth.normal((N, O), 4), synth.normal((N, O), 5))
    xs = [t(a, device=dev).requires_grad_(True) for a in (x, q, lstm)]
    ei, b = t(gb.edge_index, device=dev), t(gb.batch, device=dev)
    out = m(xs[0], ei, b, xs[1], xs[2], x_ctx_init=t(xc, device=dev))
    (out * t(w, device=dev)).sum().backward()
    rp = {k: v.double().requires_grad_(True) for k, v in tparams(p).items() if v.is_floating_point()}
    rs = [t(a).double().requires_grad_(True) for a in (x, q, lstm)]
    ref = R.lcgn_seq(rs[0], t(gb.edge_index), t(gb.batch), rs[1], rs[2], rp, t(xc).double(), heads=H)
    (ref * t(w).double()).sum().backward()
    assert maxabs(out, ref) < 1e-4
    floor = 1e-3 * max(float(v.grad.abs().max()) for v in list(rp.values()) + rs if v.grad is not None)
    bad = {}
    for got, r, name in zip(xs, rs, ("x", "q_encoding", "lstm_outputs")):
        bad[name] = _rel(got.grad, r.grad, floor)
    for k, v in m.named_parameters():
        if k.startswith("bns."):
            continue
        rg = rp[k].grad if rp[k].grad is not None else torch.zeros_like(rp[k])
        bad[k] = _rel(v.grad if v.grad is not None else torch.zeros_like(v), rg, floor)
    bad = {k: e for k, e in bad.items() if not e < 5e-4}
    assert not bad, bad
    with torch.no_grad():
        fused = m.eval()(xs[0], ei, b, xs[1], xs[2], x_ctx_init=t(xc, device=dev))
    assert maxabs(fused, out) < 1e-4


@pytest.mark.parametrize("H,Cc,concat", [(1, 512, False), (4, 512, False), (4, 512, True), (3, 20, True), (8, 8, False),
                                         (2, 1028, False), (1, 2052, True)])
def test_attention_kernel_matches_the_composition(dev, H, Cc, concat):
    """gvqa_lcgn_attention against the differentiable composition it stands in for (under no_grad), on one set of operands: the
    one-wave and one-wave-per-head layouts, odd head counts, heads wider than 2048 channels; both batch kinds."""
    from graphvqa_amd.graph import SceneGraphBatch
    from graphvqa_amd.lcgn import lcgn_attention, _lcgn_attention_autograd
    gb = synth.make_graph_batch(6, seed=0xA77, nodes_lo=1, nodes_hi=12, rel_per_node=1.5)
    N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
    J = t(synth.normal((N, 3 * HC), 11), device=dev) * 0.3
    pc = t(synth.normal((B, 2 * HC), 12), device=dev) * 0.3
    bias = t(synth.normal((HC if concat else Cc,), 13), device=dev)
    cross = gb.edge_index.copy()
    cross[0, ::7] = (cross[0, ::7] + 5) % N
    for ei in (gb.edge_index, cross):
        graph = SceneGraphBatch(t(ei, device=dev), t(gb.batch, device=dev), N, B)
        with torch.no_grad():
            out, alpha = lcgn_attention(J, pc, graph, H, Cc, concat, 0.2, bias, want_alpha=True)
            ref, ref_alpha = _lcgn_attention_autograd(J, pc, graph, H, Cc, concat, 0.2, bias)
        assert maxabs(out, ref) < 1e-5 * max(1.0, float(ref.abs().max()))
        assert maxabs(alpha, ref_alpha) < 1e-5
