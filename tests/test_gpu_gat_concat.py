"""GPU tests of the gat concat form and the one-call layer: gvqa_gat_message_passing_concat (LDS-tiled and general kernels),
gvqa_gat_mp_backward_concat, gat_message_passing(concat=True), gvqa_gat_layer_forward and the road the `gat` module takes, against
the dense form in fp64 on the CPU (tests/gat_concat_ref.py) and the reference's own recording (tests/golden/gat_conv_concat_pair.npz).
Bounds: the kernel family's own (tests/test_gpu_backward.py): out 1e-5 x max(1, |ref|max), alpha 1e-6, gradients 2e-5 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from tests import gat_concat_ref as G
from tests.lcgn_ref import column_block, untouched
from tests.util import load_golden, t, maxabs

pytestmark = pytest.mark.gpu
SENTINEL = -777.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(c, dev):
    from graphvqa_amd.graph import SceneGraphBatch
    return SceneGraphBatch(c["ei"].to(dev), c["batch"].to(dev), c["N"], c["B"])


def _plan(g, Cc, H):
    from graphvqa_amd import _lib
    p = _lib.MpPlan()
    _lib.check(_lib.load().gvqa_gat_mp_plan_concat(C.byref(g.c), Cc, H, C.byref(p)))          # the plan the concat kernel runs with
    return p


def _dev_operands(c, dev):
    return {k: (None if c[k] is None else c[k].to(dev)) for k in ("xp", "a_node", "a_edge", "mask", "bias", "w")}


def _forward_c(g, Cc, H, xp, a_node, a_edge, mask, bias, force=0, out=None):
    """gvqa_gat_message_passing_concat on 2-D views (their row strides are the leading dimensions) -> (out, alpha)."""
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream, _ptr
    dev = xp.device
    if out is None:
        out = torch.full((g.num_nodes, H * Cc), float("nan"), dtype=torch.float32, device=dev)
    alpha = torch.full((g.num_edges, H), float("nan"), dtype=torch.float32, device=dev)
    m = _lib.GatMpDesc()
    m.C, m.H, m.negative_slope, m.force = Cc, H, G.SLOPE, force
    m.xp, m.xp_ld, m.a_node, m.a_edge = xp.data_ptr(), xp.stride(0), a_node.data_ptr(), a_edge.data_ptr()
    m.out, m.out_ld, m.alpha_out, m.alpha_mask, m.bias = out.data_ptr(), out.stride(0), alpha.data_ptr(), _ptr(mask), _ptr(bias)
    ws = torch.empty(max(4 * g.num_edges * H, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gvqa_gat_message_passing_concat(C.byref(g.c), C.byref(m), ws.data_ptr(), ws.numel(), _stream(dev)))
    return out, alpha


def _backward_c(g, Cc, H, xp, a_node, a_edge, alpha, mask, dout, dxp=None):
    """gvqa_gat_mp_backward_concat on 2-D views -> (dxp, da_node, da_edge)."""
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream, _ptr
    dev = xp.device
    if dxp is None:
        dxp = torch.full((g.num_nodes, H * Cc), float("nan"), dtype=torch.float32, device=dev)
    da_node = torch.full((g.num_nodes, 2 * H), float("nan"), dtype=torch.float32, device=dev)
    da_edge = torch.full((g.num_edges, H), float("nan"), dtype=torch.float32, device=dev)
    d = _lib.GatMpBwdDesc()
    d.C, d.H, d.negative_slope = Cc, H, G.SLOPE
    d.xp, d.xp_ld, d.a_node, d.a_edge = xp.data_ptr(), xp.stride(0), a_node.data_ptr(), a_edge.data_ptr()
    d.alpha, d.alpha_mask, d.dout, d.dout_ld = alpha.data_ptr(), _ptr(mask), dout.data_ptr(), dout.stride(0)
    d.dxp, d.dxp_ld, d.da_node, d.da_edge = dxp.data_ptr(), dxp.stride(0), da_node.data_ptr(), da_edge.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gvqa_gat_mp_backward_concat(C.byref(g.c), C.byref(g.transposed().c), C.byref(d), _stream(dev)))
    return dxp, da_node, da_edge


def _autograd(g, c, o):
    """Forward + backward through gat_message_passing(concat=True) -> (out, alpha, grads)."""
    from graphvqa_amd.gat_skip import gat_message_passing
    xs = [o[k].clone().requires_grad_(True) for k in ("xp", "a_node", "a_edge", "bias")]
    out, alpha = gat_message_passing(xs[0], xs[1], xs[2], g, c["H"], c["C"], G.SLOPE, o["mask"], bias=xs[3], concat=True)
    assert out.shape == (c["N"], c["H"] * c["C"])
    (out * o["w"]).sum().backward()
    return out.detach(), alpha.detach(), dict(zip(G.GRADS, (x.grad for x in xs)))


@pytest.mark.parametrize("Cc,H,with_mask", G.MATRIX)
def test_concat_matrix_vs_fp64(dev, Cc, H, with_mask):
    """Every case: the C entry on the general kernels (force = 2), on the LDS-tiled kernel (force = 1) wherever gvqa_gat_mp_plan_concat
    says tiled, and forward + backward through gat_message_passing(concat=True)."""
    c, ref = G.matrix_case(Cc, H, with_mask), G.matrix_reference(Cc, H, with_mask)
    g, o = _graph(c, dev), _dev_operands(G.matrix_case(Cc, H, with_mask), dev)
    for force in [2] + ([1] if _plan(g, Cc, H).tiled else []):
        out, alpha = _forward_c(g, Cc, H, o["xp"], o["a_node"], o["a_edge"], o["mask"], o["bias"], force)
        d = G.distances((out, alpha, {}), ref)
        print("force", force, d)
        assert G.within_bounds(d), (force, d)
    d = G.distances(_autograd(g, c, o), ref)
    print("autograd", d)
    assert G.within_bounds(d), d


def test_matrix_reaches_every_tiled_form(dev):
    """The matrix's tiled cases include one whose channel range is narrower than C with a narrower last range, and both accumulator
    counts of the kernel: an edit of the matrix or of the plan cannot drop a kernel form silently."""
    plans = {}
    for Cc, H, with_mask in G.MATRIX:
        p = _plan(_graph(G.matrix_case(Cc, H, with_mask), dev), Cc, H)
        if p.tiled:
            plans[(Cc, H)] = (p.channel_range, p.accumulators)
    print(plans)
    assert any(cw < Cc and Cc % cw != 0 for (Cc, H), (cw, acc) in plans.items()), plans
    assert {acc for cw, acc in plans.values()} == {2, 4}, plans
    assert {H for Cc, H in plans} == {1, 2, 4, 8}, plans
    assert (32, 3) not in plans and (30, 2) not in plans                     # H = 3 and C % 4 != 0: the general kernels


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("Cc,H", G.HARD)
def test_concat_hard_batch_vs_fp64(dev, Cc, H, kind):
    """In-degrees 0-9, a 301-edge hub, a one-node graph, an empty graph, a 301-node graph; kind 1: edges across graphs (general
    kernels).  The node without in-edges gets the bias exactly and an exactly zero destination-logit gradient; nothing is written
    outside out."""
    c, ref = G.hard_case(Cc, H, kind), G.hard_reference(Cc, H, kind)
    g, o = _graph(c, dev), _dev_operands(G.hard_case(Cc, H, kind), dev)
    assert g.intra_graph == (kind == 0)
    iso = c["info"]["isolated"]
    for force in ([0, 2] if kind == 0 else [0]):
        buf, view, _ = column_block(c["N"], H * Cc, 0, 0, SENTINEL, dev, guard_rows=2)
        out, alpha = _forward_c(g, Cc, H, o["xp"], o["a_node"], o["a_edge"], o["mask"], o["bias"], force, out=view)
        d = G.distances((out, alpha, {}), ref)
        print("force", force, d)
        assert G.within_bounds(d), (force, d)
        assert untouched(buf, view, SENTINEL)
        assert torch.equal(out[iso], o["bias"])
    got = _autograd(g, c, o)
    d = G.distances(got, ref)
    print("autograd", d)
    assert G.within_bounds(d), d
    assert torch.equal(got[0][iso], o["bias"])
    assert bool((got[2]["da_node"][iso, H:] == 0).all())


@pytest.mark.parametrize("Cc,H", [(12, 4), (128, 8)])
def test_concat_leading_dimensions(dev, Cc, H):
    """xp, out, dout and dxp as column blocks of wider buffers, every leading dimension different: every sentinel survives and the
    results equal the contiguous call's bit for bit."""
    c = G.matrix_case(Cc, H, True)
    g, o = _graph(c, dev), _dev_operands(c, dev)
    N, HC = c["N"], H * Cc
    out0, alpha0 = _forward_c(g, Cc, H, o["xp"], o["a_node"], o["a_edge"], o["mask"], o["bias"])
    dxp0, dan0, dae0 = _backward_c(g, Cc, H, o["xp"], o["a_node"], o["a_edge"], alpha0, o["mask"], o["w"])
    xb, xv, ldx = column_block(N, HC, 4, 8, float("nan"), dev)
    ob, ov, ldo = column_block(N, HC, 8, 8, SENTINEL, dev)
    db, dv, ldd = column_block(N, HC, 12, 8, float("nan"), dev)
    gb, gv, ldg = column_block(N, HC, 4, 4, SENTINEL, dev)
    assert len({HC, ldx, ldo, ldd, ldg}) == 5
    xv.copy_(o["xp"]); dv.copy_(o["w"])
    out1, alpha1 = _forward_c(g, Cc, H, xv, o["a_node"], o["a_edge"], o["mask"], o["bias"], out=ov)
    dxp1, dan1, dae1 = _backward_c(g, Cc, H, xv, o["a_node"], o["a_edge"], alpha1, o["mask"], dv, dxp=gv)
    assert untouched(ob, ov, SENTINEL) and untouched(gb, gv, SENTINEL)
    assert untouched(xb, xv, float("nan")) and untouched(db, dv, float("nan"))
    assert torch.equal(out1, out0) and torch.equal(alpha1, alpha0)
    assert torch.equal(dxp1, dxp0) and torch.equal(dan1, dan0) and torch.equal(dae1, dae0)
    assert bool(torch.isfinite(out0).all()) and bool(torch.isfinite(dxp0).all())


def test_concat_blocks_per_graph_and_determinism(dev):
    """One block per graph against the automatic split of the channel ranges, and the same call twice: identical bits."""
    from graphvqa_amd import _lib
    Cc, H = 512, 8
    c = G.matrix_case(Cc, H, False)
    g, o = _graph(c, dev), _dev_operands(c, dev)
    p = _plan(g, Cc, H)
    assert p.tiled and p.blocks_per_graph > 1
    run = lambda: _forward_c(g, Cc, H, o["xp"], o["a_node"], o["a_edge"], o["mask"], o["bias"], force=1)
    out_auto, alpha_auto = run()
    out_again, alpha_again = run()
    old = _lib.set_option(_lib.OPT_MP_PARTS, 1)
    try:
        out_one, alpha_one = run()
    finally:
        _lib.set_option(_lib.OPT_MP_PARTS, old)
    assert torch.equal(out_one, out_auto) and torch.equal(alpha_one, alpha_auto)
    assert torch.equal(out_again, out_auto) and torch.equal(alpha_again, alpha_auto)


def _layer_c(g, dev, in_l, in_r, e_in, Cc, H, concat, p, x_l, x_r, ea):
    """gvqa_gat_layer_forward -> (out, alpha).  p: lin_l, lin_r (or None), lin_e, att_l, att_r, att_e, bias device tensors."""
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream, _ptr
    lib = _lib.load()
    out = torch.full((g.num_nodes, H * Cc if concat else Cc), float("nan"), dtype=torch.float32, device=dev)
    alpha = torch.full((g.num_edges, H), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        need = lib.gvqa_gat_layer_workspace_bytes(C.byref(g.c), in_l, in_r, e_in, Cc, H)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.check(lib.gvqa_gat_layer_forward(C.byref(g.c), in_l, in_r, e_in, Cc, H, int(concat), 0.2, p["lin_l"].data_ptr(), _ptr(p["lin_r"]),
                                              p["lin_e"].data_ptr(), p["att_l"].data_ptr(), p["att_r"].data_ptr(), p["att_e"].data_ptr(),
                                              _ptr(p["bias"]), x_l.data_ptr(), _ptr(x_r), ea.data_ptr(), out.data_ptr(), alpha.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream(dev)))
    return out, alpha


def test_layer_forward_vs_reference_recording(dev):
    """gvqa_gat_layer_forward on the reference's own recording of the forms gat_seq never uses: concat with the shared weight and a
    single node tensor, separate lin_r with a pair (mean, and concat); x_r = NULL (the reference's x = (x_l, None)) against the
    oracle in fp64.  Bounds: those tests/test_gpu_gat.py holds the module to on this fixture."""
    from oracle import ref_torch as R
    from graphvqa_amd.graph import SceneGraphBatch
    TOL = 1e-4
    meta, gd = load_golden("gat_conv_concat_pair")
    H, Cc, e_in = meta["heads"], meta["out_channels"], meta["edge_in"]
    x, xr, ei, ea = (t(gd[k], device=dev) for k in ("x", "x_r", "edge_index", "edge_attr"))
    g = SceneGraphBatch(ei, None, x.shape[0], 1)
    flat = lambda k: t(gd[k], device=dev).reshape(-1).contiguous()
    base = dict(lin_l=t(gd["p_lin_l_weight"], device=dev), lin_e=t(gd["p_lin_e_weight"], device=dev), att_l=flat("p_att_l"),
                att_r=flat("p_att_r"), att_e=flat("p_att_e"))
    lin_r = t(gd["p_lin_r_weight"], device=dev)
    out, alpha = _layer_c(g, dev, 24, 24, e_in, Cc, H, True, dict(base, lin_r=None, bias=flat("p_bias_hc")), x, x, ea)
    assert maxabs(out, gd["out_concat"]) < TOL and maxabs(alpha, gd["alpha_concat"]) < 1e-5
    out, alpha = _layer_c(g, dev, 24, 16, e_in, Cc, H, False, dict(base, lin_r=lin_r, bias=flat("p_bias_c")), x, xr, ea)
    assert maxabs(out, gd["out_pair"]) < TOL and maxabs(alpha, gd["alpha_pair"]) < 1e-5
    out, alpha = _layer_c(g, dev, 24, 16, e_in, Cc, H, True, dict(base, lin_r=lin_r, bias=flat("p_bias_hc")), x, xr, ea)
    assert maxabs(out, gd["out_pair_concat"]) < TOL
    rp = {"lin_l.weight": t(gd["p_lin_l_weight"]).double(), "lin_r.weight": t(gd["p_lin_r_weight"]).double(),
          "lin_e.weight": t(gd["p_lin_e_weight"]).double(), "att_l": t(gd["p_att_l"]).double(), "att_r": t(gd["p_att_r"]).double(),
          "att_e": t(gd["p_att_e"]).double(), "bias": t(gd["p_bias_hc"]).double()}
    for concat in (True, False):
        rp["bias"] = t(gd["p_bias_hc" if concat else "p_bias_c"]).double()
        ref, ref_alpha = R.gat_conv((t(gd["x"]).double(), None), t(gd["edge_index"]), t(gd["edge_attr"]).double(), rp, heads=H, concat=concat,
                                    return_attention_weights=True)
        out, alpha = _layer_c(g, dev, 24, 16, e_in, Cc, H, concat, dict(base, lin_r=lin_r, bias=flat("p_bias_hc" if concat else "p_bias_c")),
                              x, None, ea)
        assert maxabs(out, ref) < TOL and maxabs(alpha, ref_alpha) < 1e-5, concat


def _mp_launches(fn):
    from graphvqa_amd import _lib
    try:
        _lib.prof_enable(True); _lib.prof_collect()
        res = fn()
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
    finally:
        _lib.prof_enable(False)
    return res, prof["mp"][1]


def test_concat_message_passing_is_one_launch(dev):
    """gat_message_passing(concat=True) is ONE launch in the message-passing stage for H heads, with and without gradients (the
    `gat` module's own road, once per head, records H; it moves to this call once the two are measured against each other)."""
    from graphvqa_amd.gat_skip import gat_message_passing
    Cc, H = 12, 4
    c = G.matrix_case(Cc, H, True)
    g, o = _graph(c, dev), _dev_operands(c, dev)
    call = lambda xp: gat_message_passing(xp, o["a_node"], o["a_edge"], g, H, Cc, G.SLOPE, o["mask"], bias=o["bias"], concat=True)
    with torch.no_grad():
        (out_eval, _), n = _mp_launches(lambda: call(o["xp"]))
    assert n == 1, n
    (out_grad, _), n = _mp_launches(lambda: call(o["xp"].clone().requires_grad_(True)))
    assert n == 1 and out_grad.requires_grad, n
    assert out_eval.shape == (c["N"], H * Cc) and torch.equal(out_eval, out_grad.detach())


@pytest.mark.parametrize("pair", [False, True])
def test_concat_layer_gradients_vs_oracle(dev, pair):
    """The concat layer and the pair + concat layer are differentiable: fp64 autograd through the oracle, at the bounds of
    tests/test_gpu_backward.py::test_gat_layer_gradients_vs_oracle."""
    from oracle import ref_torch as R
    from graphvqa_amd.gat_skip import gat
    gb = synth.make_graph_batch(4, seed=0x6A7, nodes_lo=6, nodes_hi=20, rel_per_node=1.5)
    N, E, H, Cc = gb.num_nodes, gb.num_edges, 4, 8
    conv = gat((24, 16) if pair else 24, Cc, 20, heads=H, concat=True, negative_slope=0.2, dropout=0.0, bias=True).to(dev)
    with torch.no_grad():
        conv.bias.copy_(t(synth.normal((H * Cc,), 7), device=dev))
    arrays = [synth.normal((N, 24), 1), synth.normal((E, 20), 2)] + ([synth.normal((N, 16), 4)] if pair else [])
    w = synth.normal((N, H * Cc), 3)
    xs = [t(a, device=dev).requires_grad_(True) for a in arrays]
    out = conv((xs[0], xs[2]) if pair else xs[0], t(gb.edge_index, device=dev), xs[1])
    (out * t(w, device=dev)).sum().backward()
    rp = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.state_dict().items() if pair or k != "lin_r.weight"}
    if not pair:
        rp["lin_r.weight"] = rp["lin_l.weight"]
    rs = [t(a).double().requires_grad_(True) for a in arrays]
    ref = R.gat_conv((rs[0], rs[2]) if pair else rs[0], t(gb.edge_index), rs[1], rp, heads=H, concat=True)
    (ref * t(w).double()).sum().backward()
    assert maxabs(out, ref) < 1e-5
    for got, r in zip(xs, rs):
        assert G.rel(got.grad, r.grad) < 1e-4
    for k, v in conv.named_parameters():
        assert G.rel(v.grad, rp[k].grad) < 1e-4, k
