"""CPU-only checks of the multi-head LCGN surface: argument validation of gvqa_lcgn_attention / gvqa_gat_lcgn_forward (status
codes, nothing enqueued), the recorded reference fixture against the oracle, and the modules' state_dict contract."""
import ctypes as C

import pytest
import torch

from graphvqa_amd import synth
from oracle import ref_torch as R
from tests.util import load_golden, t, tparams, maxabs


def _graph(nodes=100, edges=400, graphs=4, intra=1, finalized=1):
    """A gvqa_graph with hand-filled statistics and no device memory: enough for the host-side checks."""
    from graphvqa_amd import _lib
    g = _lib.Graph()
    g.num_nodes, g.num_edges, g.num_graphs = nodes, edges, graphs
    g.max_graph_nodes, g.max_graph_edges, g.max_in_degree = 30, 120, 8
    g.intra_graph, g.valid, g.finalized = intra, 1, finalized
    return g


def test_lcgn_attention_rejects_bad_arguments_without_gpu():
    from graphvqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV, E_UNS = _lib.E_INVALID, _lib.E_UNSUPPORTED
    g = _graph()
    att = lambda g_, H, Cc, ldj=None, ldpc=None, ldo=None, J=None, pc=None, out=None: lib.gvqa_lcgn_attention(
        g_, H, Cc, 0, 0.2, J, 3 * H * Cc if ldj is None else ldj, pc, 2 * H * Cc if ldpc is None else ldpc, None, out,
        Cc if ldo is None else ldo, None, None)
    assert att(None, 2, 8) == E_INV and "null graph" in err()
    for H in (0, 9):
        assert att(C.byref(g), H, 8) == E_UNS and "heads" in err()
    assert att(C.byref(g), 2, 6) == E_UNS and "multiple of 4" in err()
    assert att(C.byref(g), 2, 2052) == E_UNS and "4096" in err()
    assert att(C.byref(g), 4, 1028) == E_UNS and "4096" in err()
    assert att(C.byref(g), 2, 8, ldj=47) == E_INV and "leading dimensions" in err()
    assert att(C.byref(_graph(finalized=0)), 2, 8) == E_INV and "finalized" in err()
    assert att(C.byref(g), 2, 8) == E_INV and "null tensor" in err()
    fake = 1 << 20                      # never dereferenced: the alignment check comes first
    assert att(C.byref(g), 2, 8, J=fake + 4, pc=fake, out=fake) == E_UNS and "aligned" in err()
    assert att(C.byref(g), 2, 8, ldj=50, J=fake, pc=fake, out=fake) == E_UNS and "aligned" in err()
    assert att(C.byref(_graph(nodes=0, edges=0)), 2, 8) == 0                     # an empty batch enqueues nothing


def test_gat_lcgn_forward_rejects_bad_arguments_without_gpu():
    from graphvqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV, E_WS, E_UNS = _lib.E_INVALID, _lib.E_WORKSPACE, _lib.E_UNSUPPORTED
    g, p = _graph(), _lib.LcgnParams()
    fwd = lambda g_, p_, H, Cc, ws_bytes=0, **kw: lib.gvqa_gat_lcgn_forward(
        g_, kw.get("in_c", 12), Cc, H, kw.get("cmd", 16), 1, 0.2, p_, None, None, None, None, None, ws_bytes, None)
    assert fwd(None, C.byref(p), 2, 8) == E_INV and "null" in err()
    assert fwd(C.byref(g), None, 2, 8) == E_INV and "null" in err()
    for H in (0, 9):
        assert fwd(C.byref(g), C.byref(p), H, 8) == E_UNS and "heads" in err()
    assert fwd(C.byref(g), C.byref(p), 2, 10) == E_UNS and "multiple of 4" in err()
    assert fwd(C.byref(g), C.byref(p), 8, 516) == E_UNS and "4096" in err()
    assert fwd(C.byref(g), C.byref(p), 2, 8, in_c=0) == E_INV and "bad dims" in err()
    need = lib.gvqa_gat_lcgn_workspace_bytes(C.byref(g), 12, 8, 2, 16)
    assert need >= 4 * (100 * 3 * 16 + 4 * 2 * 16)
    assert fwd(C.byref(g), C.byref(p), 2, 8) == E_WS and "workspace" in err()
    assert fwd(C.byref(g), C.byref(p), 2, 8, ws_bytes=need - 1) == E_WS
    # host-side queries: zero for what the layer does not take
    assert lib.gvqa_gat_lcgn_workspace_bytes(None, 12, 8, 2, 16) == 0
    assert lib.gvqa_gat_lcgn_workspace_bytes(C.byref(g), 12, 8, 9, 16) == 0
    assert lib.gvqa_gat_lcgn_workspace_bytes(C.byref(g), 12, 6, 2, 16) == 0
    # the one-call lcgn_seq stays the gat_heads = 1 model
    ld = _lib.LcgnDims(8, 8, 8, 4, 5, 4, 0.2, 0)
    assert lib.gvqa_lcgn_seq_forward(C.byref(g), C.byref(ld), C.byref(p), None, None, None, None, None, None, 0, None) == E_UNS


def _layer_oracle(x, edge_index, cmd, batch, p, H, concat, slope=0.2):
    """gat_lcgn.forward + message (lcgn.py:120-238) for either concat form: the oracle's lcgn_conv for concat=False; concat=True
    keeps the heads side by side instead of averaging them (lcgn.py:183-184), everything else as lcgn_conv states it."""
    if not concat:
        return R.lcgn_conv(x, edge_index, cmd, batch, p, prefix="", heads=H, negative_slope=slope, return_attention_weights=True)
    C_ = p["lin_l.weight"].shape[0] // H
    pm = dict(p)
    pm.pop("bias", None)
    # the per-head rows before the mean: lcgn_conv on each head's own weights with H = 1 (the softmax is per head anyway)
    outs, alphas = [], []
    for h in range(H):
        ph = {k: v[h * C_:(h + 1) * C_] for k, v in pm.items()}
        o, a = R.lcgn_conv(x, edge_index, cmd, batch, ph, prefix="", heads=1, negative_slope=slope, return_attention_weights=True)
        outs.append(o); alphas.append(a)
    out = torch.cat(outs, dim=1)
    if p.get("bias") is not None:
        out = out + p["bias"]
    return out, torch.cat(alphas, dim=1)


@pytest.mark.parametrize("H", [1, 2, 4, 8])
@pytest.mark.parametrize("concat", [False, True])
def test_layer_fixture_matches_the_oracle(H, concat):
    """The recorded reference layer (lcgn.py:63-238, several heads, both batches) is what the oracle states: this pins the oracle's
    lcgn_conv(heads=H) for H > 1 and the per-head form the concat check uses."""
    meta, g = load_golden("lcgn_heads_small")
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    s = meta["input_seeds"]
    x, cmd = t(synth.normal((N, meta["in_channels"]), s["x"])), t(synth.normal((B, meta["cmd_dim"]), s["cmd"]))
    p = tparams(synth.gat_lcgn_params(meta["in_channels"], meta["out_channels"], H, meta["param_seed"] + H, meta["cmd_dim"], concat=concat))
    for tag, ei in (("layer", g["edge_index"]), ("xlayer", g["x_edge_index"])):
        out, alpha = _layer_oracle(x, t(ei), cmd, t(g["batch"]), p, H, concat)
        assert maxabs(out, g[f"{tag}_h{H}_c{int(concat)}_out"]) < 1e-5, tag
        assert maxabs(alpha, g[f"{tag}_h{H}_c{int(concat)}_alpha"]) < 1e-5, tag
    # the batch's shape: multi-edges, an empty graph inside it, a node without in-edges (its output is the bias alone)
    ei = g["edge_index"]
    assert len(set(map(tuple, ei.T.tolist()))) < ei.shape[1]
    assert 1 not in set(g["batch"].tolist()) and B == 4
    assert 2 not in set(ei[1].tolist())
    bias = p["bias"]
    assert maxabs(t(g[f"layer_h{H}_c{int(concat)}_out"])[2], bias) == 0.0


@pytest.mark.parametrize("H", [2, 4])
def test_lcgn_seq_heads_fixture_matches_the_oracle(H):
    meta, g = load_golden("lcgn_heads_small")
    sq, s = meta["seq"], meta["input_seeds"]
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    O = sq["out_channels"]
    p = tparams(synth.lcgn_seq_params(sq["in_channels"], O, seed=sq["param_seed"] + H, cmd_dim=O, question_dim=O, heads=H))
    x, q, lstm = synth.normal((N, sq["in_channels"]), s["seq_x"]), synth.normal((B, O), s["q"]), synth.normal((sq["L"], B, O), s["lstm"])
    out = R.lcgn_seq(t(x), t(g["edge_index"]), t(g["batch"]), t(q), t(lstm), p, t(g["seq_x_ctx_init"]), heads=H)
    assert maxabs(out, g[f"seq_h{H}_out"]) < 1e-5
    torch.manual_seed(sq["torch_seed"])
    assert torch.equal(torch.randn(N, O), t(g["seq_x_ctx_init"]))


@pytest.mark.parametrize("H", [1, 2, 4, 8])
@pytest.mark.parametrize("concat", [False, True])
def test_gat_lcgn_state_dict_contract(H, concat):
    from graphvqa_amd.lcgn import gat_lcgn
    m = gat_lcgn(12, 8, 1, heads=H, concat=concat, cmd_dim=16)
    want = synth.gat_lcgn_params(12, 8, H, 1, 16, concat=concat)
    sd = m.state_dict()
    assert set(sd) == set(want)
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert float(sd["bias"].abs().max()) == 0.0                         # zeros(self.bias), lcgn.py:118
    assert "heads=%d" % H in repr(m)
    nb = gat_lcgn(12, 8, 1, heads=H, concat=concat, cmd_dim=16, bias=False)
    assert "bias" not in nb.state_dict()


def test_lcgn_seq_state_dict_contract_with_heads():
    from graphvqa_amd.lcgn import lcgn_seq
    m = lcgn_seq(300, 512, 300, 5, gat_cmd_dim=512, question_dim=512, gat_heads=4)
    want = synth.lcgn_seq_params(300, 512, seed=1, cmd_dim=512, question_dim=512, heads=4)
    sd = m.state_dict()
    assert set(sd) == set(want)
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert tuple(sd["lcgn.lin_l.weight"].shape) == (4 * 512, 3 * 512) and tuple(sd["lcgn.bias"].shape) == (512,)


def test_gat_lcgn_refuses_bipartite_forms():
    from graphvqa_amd.lcgn import gat_lcgn
    m = gat_lcgn(12, 8, 1, heads=2, cmd_dim=16)
    x = torch.zeros(3, 12)
    with pytest.raises(NotImplementedError):
        m((x, x), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(1, 16), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        m(x, torch.zeros(2, 1, dtype=torch.int64), torch.zeros(1, 16), torch.zeros(3, dtype=torch.int64), size=(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, torch.zeros(2, 1, dtype=torch.int64), torch.zeros(1, 16), torch.zeros(3, dtype=torch.int64))
