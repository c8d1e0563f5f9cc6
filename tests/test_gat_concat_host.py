"""CPU-only checks of the gat concat / layer surface: argument validation of gvqa_gat_message_passing_concat,
gvqa_gat_mp_backward_concat, gvqa_gat_layer_workspace_bytes and gvqa_gat_layer_forward (status codes, nothing enqueued), and the
fairness of the GPU tests' bounds: the dense reference in fp32 must sit well inside them."""
import ctypes as C

import pytest
import torch

from tests import gat_concat_ref as G


def _graph(nodes=100, edges=400, graphs=4, intra=1, finalized=1):
    """A gvqa_graph with hand-filled statistics and no device memory: enough for the host-side checks."""
    from graphvqa_amd import _lib
    g = _lib.Graph()
    g.num_nodes, g.num_edges, g.num_graphs = nodes, edges, graphs
    g.max_graph_nodes, g.max_graph_edges, g.max_in_degree = 30, 120, 8
    g.intra_graph, g.valid, g.finalized = intra, 1, finalized
    return g


FAKE = 1 << 20          # a 16-byte aligned address that is never dereferenced: every check below fails before a launch


def test_message_passing_concat_rejects_bad_arguments_without_gpu():
    from graphvqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV, E_WS, E_UNS = _lib.E_INVALID, _lib.E_WORKSPACE, _lib.E_UNSUPPORTED
    g = _graph()
    call = lambda g_, m_, ws=None, n=0: lib.gvqa_gat_message_passing_concat(g_, m_, ws, n, None)

    def desc(**kw):
        m = _lib.GatMpDesc()
        m.C, m.H, m.negative_slope = 8, 4, 0.2
        m.xp, m.a_edge, m.out = FAKE, FAKE, FAKE
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert call(None, C.byref(desc())) == E_INV and "null" in err()
    assert call(C.byref(g), None) == E_INV and "null" in err()
    assert call(C.byref(g), C.byref(_lib.GatMpDesc())) == E_INV                       # no tensors, no dims
    assert call(C.byref(g), C.byref(desc(xp=None))) == E_INV and "null tensor" in err()
    assert call(C.byref(g), C.byref(desc(H=0))) == E_INV and "bad dims" in err()
    for field in ("skip", "graph_term", "graph_scale", "head_rows", "head_weight_out"):
        kw = {field: FAKE}
        if field == "graph_term":
            kw["graph_term_ld"] = 12
        assert call(C.byref(g), C.byref(desc(**kw))) == E_UNS and "must be NULL" in err(), field
    assert call(C.byref(g), C.byref(desc(bn_weight=FAKE, bn_bias=FAKE, bn_mean=FAKE, bn_var=FAKE))) == E_UNS
    assert call(C.byref(g), C.byref(desc(bn_weight=FAKE))) == E_INV                   # an incomplete BN is invalid first, as in the mean form
    # the tiled kernel cannot be forced where it does not apply; the general kernel needs 4*E*H workspace bytes
    assert call(C.byref(g), C.byref(desc(H=3, force=1))) == E_UNS and "tiled kernel not applicable" in err()
    assert call(C.byref(_graph(intra=0)), C.byref(desc(force=1))) == E_UNS
    assert call(C.byref(g), C.byref(desc(force=2))) == E_WS and "workspace" in err()
    assert call(C.byref(g), C.byref(desc(force=2)), FAKE, 4 * 400 * 4 - 1) == E_WS
    assert call(C.byref(g), C.byref(desc(H=3))) == E_WS                               # H = 3: the general kernels
    assert call(C.byref(_graph(nodes=0, edges=0)), C.byref(desc())) == 0              # an empty batch enqueues nothing


def test_mp_backward_concat_rejects_bad_arguments_without_gpu():
    from graphvqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV, E_UNS = _lib.E_INVALID, _lib.E_UNSUPPORTED
    g, gt = _graph(), _graph()

    def desc(**kw):
        d = _lib.GatMpBwdDesc()
        d.C, d.H, d.negative_slope = 8, 4, 0.2
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    call = lambda g_, gt_, d_: lib.gvqa_gat_mp_backward_concat(g_, gt_, d_, None)
    assert call(None, C.byref(gt), C.byref(desc())) == E_INV and "null" in err()
    assert call(C.byref(g), None, C.byref(desc())) == E_INV
    assert call(C.byref(g), C.byref(gt), None) == E_INV
    assert call(C.byref(g), C.byref(_graph(edges=399)), C.byref(desc())) == E_INV and "transposed" in err()
    assert call(C.byref(g), C.byref(gt), C.byref(desc(H=9))) == E_UNS
    assert call(C.byref(g), C.byref(gt), C.byref(desc(C=1028))) == E_UNS
    assert call(C.byref(g), C.byref(gt), C.byref(desc(dalpha_node=FAKE))) == E_UNS and "dalpha_node" in err()
    assert call(C.byref(g), C.byref(gt), C.byref(desc())) == E_INV and "null tensor" in err()
    e = _graph(nodes=0, edges=0)
    assert call(C.byref(e), C.byref(e), C.byref(desc())) == 0


def test_gat_layer_forward_rejects_bad_arguments_without_gpu():
    from graphvqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV, E_WS = _lib.E_INVALID, _lib.E_WORKSPACE
    g = _graph()

    def fwd(g_, in_l=12, in_r=12, de=6, Cc=8, H=4, w=FAKE, w_r=None, x_l=None, ws=None, ws_bytes=0):
        return lib.gvqa_gat_layer_forward(g_, in_l, in_r, de, Cc, H, 1, 0.2, w, w_r, w, w, w, w, None, x_l, None, None, None, None,
                                          ws, ws_bytes, None)

    assert fwd(None) == E_INV and "null" in err()
    for kw in (dict(in_l=0), dict(in_r=0), dict(de=0), dict(Cc=0), dict(H=0), dict(H=-1)):
        assert fwd(C.byref(g), **kw) == E_INV and "dimension" in err(), kw
        dims = dict(dict(in_l=12, in_r=12, de=6, Cc=8, H=4), **kw)
        assert lib.gvqa_gat_layer_workspace_bytes(C.byref(g), dims["in_l"], dims["in_r"], dims["de"], dims["Cc"], dims["H"]) == 0
    assert lib.gvqa_gat_layer_workspace_bytes(None, 12, 12, 6, 8, 4) == 0
    assert fwd(C.byref(g), w=None) == E_INV and "null weight" in err()
    assert fwd(C.byref(g), in_r=16) == E_INV and "shared weight" in err()              # no lin_r: in_r must equal in_l
    need = lib.gvqa_gat_layer_workspace_bytes(C.byref(g), 12, 16, 6, 8, 4)
    assert need >= 4 * (100 * 32 + 100 * 8 + 2 * 400 * 4 + 8 * 12 + 8 * 16 + 4 * 6)    # xp, a_node, a_edge + alpha, the three folds
    assert fwd(C.byref(g), in_r=16, w_r=FAKE) == E_WS and "workspace" in err()
    assert fwd(C.byref(g), in_r=16, w_r=FAKE, ws=FAKE, ws_bytes=need - 1) == E_WS
    assert fwd(C.byref(g), in_r=16, w_r=FAKE, ws=FAKE, ws_bytes=need) == E_INV and "null tensor" in err()


def _fp32_distance(case, ref64):
    return G.distances(G.reference(case, torch.float32), ref64)


@pytest.mark.parametrize("Cc,H,with_mask", G.MATRIX)
def test_bounds_are_fair_on_the_generated_batch(Cc, H, with_mask):
    """The dense form in fp32 stays below one fifth of every bound the GPU tests hold the kernels to: a correct fp32 kernel has room,
    the bounds cannot quietly become unfair.  Measured on these operands, both batches, at worst: 5.7e-8 of 1e-5 in out, 1.1e-7 of
    1e-6 in alpha, 1.7e-7 of 2e-5 in the gradients (the kernels themselves: 1.2e-7, 1.3e-7, 5.1e-7 on an MI355X)."""
    d = _fp32_distance(G.matrix_case(Cc, H, with_mask), G.matrix_reference(Cc, H, with_mask))
    print(d)
    assert G.within_bounds(d, 0.2), d


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("Cc,H", G.HARD)
def test_bounds_are_fair_on_the_hard_batch(Cc, H, kind):
    d = _fp32_distance(G.hard_case(Cc, H, kind), G.hard_reference(Cc, H, kind))
    print(d)
    assert G.within_bounds(d, 0.2), d


def test_concat_plan_is_the_concat_kernels_own():
    """gvqa_gat_mp_plan_concat plans with a bias of H*C floats: at H <= 4 it is the mean form's geometry without the skip stage, at
    H = 8 it needs more LDS than the mean plan of the same batch."""
    from graphvqa_amd import _lib
    lib = _lib.load()

    def plans(g, Cc, H):
        out = []
        for fn in (lib.gvqa_gat_mp_plan, lib.gvqa_gat_mp_plan_concat):
            p = _lib.MpPlan()
            assert fn(C.byref(g), Cc, H, C.byref(p)) == 0
            out.append(p)
        return out

    g = _graph(65536, 262144, 2048)
    g.max_graph_nodes, g.max_graph_edges = 32, 128
    mean, cat = plans(g, 512, 4)                                   # config 3
    assert cat.tiled == 1 and cat.channel_range == mean.channel_range == 128 and cat.accumulators == mean.accumulators
    assert cat.stages_per_graph == 4 * 4 and mean.stages_per_graph == 4 * 5 and cat.lds_bytes == mean.lds_bytes - 4 * 512
    mean, cat = plans(g, 512, 8)
    assert cat.tiled == 1 and cat.channel_range <= mean.channel_range
    if cat.channel_range == mean.channel_range:
        assert cat.lds_bytes == mean.lds_bytes + 3 * 4 * 512
    assert plans(_graph(intra=0), 32, 4)[1].tiled == 0 and plans(g, 30, 2)[1].tiled == 0 and plans(g, 32, 3)[1].tiled == 0
    assert lib.gvqa_gat_mp_plan_concat(None, 32, 4, C.byref(_lib.MpPlan())) == _lib.E_INVALID
