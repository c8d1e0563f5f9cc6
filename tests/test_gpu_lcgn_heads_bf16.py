"""GPU checks of lcgn_seq(gat_heads > 1, node_feature_dtype=bfloat16): the bf16-storage attention kernel (gvqa_lcgn_attention_bf16)
against the fp32 kernel on the same values, the eval road against a same-rounding CPU emulation and the oracle's model of bf16
storage (oracle/ref_torch.lcgn_seq(node_store=bf16_storage)), and the differentiable road against fp64 autograd."""
import pytest
import torch
import torch.nn.functional as F

from graphvqa_amd import synth
from oracle import ref_torch as R
from tests.util import load_golden, t, tparams, maxabs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rel(a, b, floor=0.0):
    b = b.detach().cpu().double()
    return maxabs(a, b) / max(float(b.abs().max()), floor, 1e-12)


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
def _kernel_case(dev, H, Cc, concat):
    """The operands of test_gpu_lcgn_heads.py::test_attention_kernel_matches_the_composition, J rounded to bf16; both batch kinds."""
    from graphvqa_amd.graph import SceneGraphBatch
    gb = synth.make_graph_batch(6, seed=0xA77, nodes_lo=1, nodes_hi=12, rel_per_node=1.5)
    N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
    J16 = (t(synth.normal((N, 3 * HC), 11), device=dev) * 0.3).bfloat16()
    pc = t(synth.normal((B, 2 * HC), 12), device=dev) * 0.3
    bias = t(synth.normal((HC if concat else Cc,), 13), device=dev)
    cross = gb.edge_index.copy()
    cross[0, ::7] = (cross[0, ::7] + 5) % N
    graphs = [SceneGraphBatch(t(ei, device=dev), t(gb.batch, device=dev), N, B) for ei in (gb.edge_index, cross)]
    assert graphs[0].c.intra_graph and not graphs[1].c.intra_graph
    return J16, pc, bias, graphs


def _check_kernel(dev, H, Cc, concat):
    from graphvqa_amd.lcgn import lcgn_attention, lcgn_attention_bf16
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, concat)
    for graph in graphs:
        with torch.no_grad():
            ref, ref_alpha = lcgn_attention(J16.float(), pc, graph, H, Cc, concat, 0.2, bias, want_alpha=True)
            o32, a32 = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, 0.2, bias, want_alpha=True, out_dtype=torch.float32)
            o16, a16 = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, 0.2, bias, want_alpha=True)
            o16b, _ = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, 0.2, bias)
            o32b, a32b = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, 0.2, bias, want_alpha=True, out_dtype=torch.float32)
        rmax = float(ref.abs().max())
        same = float((o16.float() == ref.bfloat16().float()).float().mean())
        print("lcgn_attention_bf16 H=%d C=%d concat=%d intra=%d: fp32 out %.3e, alpha %.3e, bf16 out %.3e (|ref| %.3e), bit-equal %.5f" %
              (H, Cc, concat, graph.c.intra_graph, maxabs(o32, ref), maxabs(a32, ref_alpha), maxabs(o16.float(), ref), rmax, same))
        assert o32.dtype == torch.float32 and o16.dtype == torch.bfloat16 and o32.shape == ref.shape == o16.shape
        assert maxabs(o32, ref) < 1e-5 * max(1.0, rmax)
        assert maxabs(a32, ref_alpha) < 1e-5 and maxabs(a16, ref_alpha) < 1e-5
        assert maxabs(o16.float(), ref) < 2.0 ** -8 * (rmax + 1.0)
        assert same > 0.99
        assert torch.equal(o16, o16b) and torch.equal(o32, o32b) and torch.equal(a32, a32b) and torch.equal(a32, a16)


@pytest.mark.parametrize("H,Cc,concat", [(1, 512, False), (4, 512, False), (4, 512, True), (3, 24, True), (8, 8, False),
                                         (2, 1032, False), (1, 2056, True)])
def test_bf16_attention_kernel_matches_the_fp32_kernel(dev, H, Cc, concat):
    """One wave for every head and one wave per head, an odd head count, 1 / 2 / 4 / 8 chunks per lane (C = 512 over 64 lanes: 1;
    1032: 3 -> 4; 2056: 5 -> 8; 24 over 16 lanes: 1; 8 over 8 lanes: 1), heads averaged and side by side."""
    from graphvqa_amd.lcgn import _attention_bf16_supported
    assert _attention_bf16_supported(H, Cc)
    _check_kernel(dev, H, Cc, concat)


@pytest.mark.parametrize("H,Cc,concat", [(3, 12, True), (2, 12, False)])
def test_bf16_attention_falls_back_to_the_fp32_kernel(dev, H, Cc, concat):
    """C % 8 != 0 is outside the entry point's limits (GVQA_E_UNSUPPORTED); the wrapper runs the fp32 kernel on the same values."""
    import ctypes as C
    from graphvqa_amd import _lib
    from graphvqa_amd.lcgn import _attention_bf16_supported
    assert not _attention_bf16_supported(H, Cc)
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, concat)
    out = torch.empty((J16.shape[0], ((H * Cc if concat else Cc) + 7) // 8 * 8), dtype=torch.bfloat16, device=dev)
    rc = _lib.load().gvqa_lcgn_attention_bf16(C.byref(graphs[0].c), H, Cc, int(concat), 0.2, J16.data_ptr(), J16.shape[1], pc.data_ptr(),
                                              pc.shape[1], bias.data_ptr(), out.data_ptr(), out.shape[1], 1, None, None)
    assert rc == _lib.E_UNSUPPORTED
    _check_kernel(dev, H, Cc, concat)


def test_bf16_attention_writes_into_a_column_block(dev):
    """`out` as the right half of an [N, 2 C] bf16 pair buffer (how lcgn_seq places the message): the left half is untouched."""
    from graphvqa_amd.lcgn import lcgn_attention_bf16
    H, Cc = 4, 16
    J16, pc, bias, graphs = _kernel_case(dev, H, Cc, False)
    N = J16.shape[0]
    pair = torch.full((N, 2 * Cc), 7.0, dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        want, _ = lcgn_attention_bf16(J16, pc, graphs[0], H, Cc, False, 0.2, bias)
        got, _ = lcgn_attention_bf16(J16, pc, graphs[0], H, Cc, False, 0.2, bias, out=pair[:, Cc:])
    assert got.data_ptr() == pair[:, Cc:].data_ptr()
    assert torch.equal(pair[:, Cc:], want) and bool((pair[:, :Cc] == 7.0).all())


# ---- lcgn_seq, eval ---------------------------------------------------------------------------------------------------------------
def _bf16_pieces(W, pieces):
    """The weight the bf16 matrix-core GEMM multiplies by: bf16(W) [+ bf16(W - bf16(W))]."""
    hi = W.bfloat16().float()
    return hi if pieces == 1 else hi + (W - hi).bfloat16().float()


def _storage_emulation(x, edge_index, batch, q, lstm, p, x_ctx_init, H, pieces, T=4, slope=0.2):
    """tests/test_gpu_gat.py::_lcgn_bf16_storage_emulation for H heads: lcgn_seq.forward on the CPU in fp32 with the per-node tensors
    rounded to bf16 exactly where the bf16 eval road stores them (x, x_loc, proj_x_loc, z_loc, x_ctx, prod, J -- once, after the
    sum of its three terms --, the message after the head mean and the bias) and the node products' weights replaced by the bf16
    pieces the matrix cores multiply by; the per-question path untouched."""
    rb = lambda v: v.bfloat16().float()
    p = dict(p)
    for k in ("init_sg_emb_input.0.weight", "proj_x_loc.1.weight", "lcgn.lin_l.weight", "lcgn.lin_r.weight", "lcgn.cal_x.weight",
              "proj_x_ctx.1.weight", "output_layer.weight", "fin_layer.weight"):
        p[k] = _bf16_pieces(p[k], pieces)
    O = p["fin_layer.weight"].shape[0]
    HO, N, B = H * O, x.shape[0], q.shape[0]
    Wcat = torch.cat([p["lcgn.lin_l.weight"], p["lcgn.lin_r.weight"], p["lcgn.cal_x.weight"]], 0)     # [3 H O, 3 O]
    x_loc = rb(F.linear(rb(x), p["init_sg_emb_input.0.weight"], p["init_sg_emb_input.0.bias"]))
    q_emb = F.relu(F.linear(q, p["qInput1.weight"], p["qInput1.bias"]))
    proj_x_loc = rb(F.linear(x_loc, p["proj_x_loc.1.weight"], p["proj_x_loc.1.bias"]))
    z_loc = rb(x_loc @ Wcat[:, :O].T)
    x_ctx = rb(x_ctx_init)
    src, dst = edge_index[0], edge_index[1]
    for t_ in range(T):
        cmd = R.lcgn_extract_command(q_emb, lstm, t_, p)
        proj_cmd = F.linear(cmd, p["lcgn.proj_cmd.weight"]).view(B, H, O)
        cal_cmd = F.linear(cmd, p["lcgn.cal_cmd.weight"]).view(B, H, O)
        prod = rb(F.linear(x_ctx, p["proj_x_ctx.1.weight"], p["proj_x_ctx.1.bias"]) * proj_x_loc)
        J = rb(x_ctx @ Wcat[:, O:2 * O].T + prod @ Wcat[:, 2 * O:].T + z_loc)
        x_l, x_r, x_val = J[:, :HO].view(N, H, O), J[:, HO:2 * HO].view(N, H, O), J[:, 2 * HO:].view(N, H, O)
        logit = (x_l[src] * (proj_cmd[batch[dst]] * x_r[dst])).sum(-1)                                # [E, H]
        alpha = R.segment_softmax(F.leaky_relu(logit, slope), dst, N)
        agg = R.scatter_add_rows(alpha.unsqueeze(-1) * (x_val[src] * cal_cmd[batch[src]]), dst, N).mean(dim=1)
        msg = rb(agg + p["lcgn.bias"])
        x_ctx = rb(F.linear(torch.cat([x_ctx, msg], 1), p["output_layer.weight"], p["output_layer.bias"]))
    return F.linear(torch.cat([x_loc, x_ctx], 1), p["fin_layer.weight"], p["fin_layer.bias"])


def _first_graphs(gb, n):
    N = int((gb.batch < n).sum())
    keep = gb.edge_index[1] < N
    assert bool((gb.edge_index[0][keep] < N).all())
    return synth.GraphBatch(edge_index=gb.edge_index[:, keep], batch=gb.batch[:N], num_graphs=n)


_SEQ = {}


def _seq_case(name):
    """Inputs, parameters and the CPU references of one case, computed once: the fp32 oracle, the fp64 oracle on bf16-stored node
    tensors, and the same-rounding emulation per number of weight pieces."""
    if name in _SEQ:
        return _SEQ[name]
    if name.startswith("small"):
        H = int(name[-1])
        meta, g = load_golden("lcgn_heads_small")
        sq, s = meta["seq"], meta["input_seeds"]
        N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
        Din, O, L = sq["in_channels"], sq["out_channels"], sq["L"]
        assert (N, Din, O) == (13, 12, 8)                     # in_channels = 12: the K padding
        ei, batch, xc = g["edge_index"], g["batch"], g["seq_x_ctx_init"]
        p = synth.lcgn_seq_params(Din, O, seed=sq["param_seed"] + H, cmd_dim=O, question_dim=O, heads=H)
        x, q, lstm = synth.normal((N, Din), s["seq_x"]), synth.normal((B, O), s["q"]), synth.normal((L, B, O), s["lstm"])
    else:
        Din, O, H = {"n390_40_64_8": (40, 64, 8), "n390_300_512_4": (300, 512, 4)}[name]
        gb = _first_graphs(synth.config2_batch(), 12)
        N, B, L = gb.num_nodes, gb.num_graphs, 10
        assert N == 390
        ei, batch = gb.edge_index, gb.batch
        p = synth.lcgn_seq_params(Din, O, seed=808, cmd_dim=O, question_dim=O, heads=H)
        x, q, lstm, xc = synth.normal((N, Din), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3), synth.normal((N, O), 4)
    tp = tparams(p)
    ref = R.lcgn_seq(t(x), t(ei), t(batch), t(q), t(lstm), tp, t(xc), heads=H)
    d64 = lambda v: t(v).double()
    ref_st = R.lcgn_seq(d64(x), t(ei), t(batch), d64(q), d64(lstm), {k: v.double() for k, v in tp.items()}, d64(xc), heads=H,
                        node_store=R.bf16_storage).float()
    emu = {pieces: _storage_emulation(t(x), t(ei), t(batch), t(q), t(lstm), tp, t(xc), H, pieces) for pieces in (2, 1)}
    _SEQ[name] = dict(H=H, Din=Din, O=O, p=p, inputs=(x, ei, batch, q, lstm), xc=xc, ref=ref, ref_st=ref_st, emu=emu)
    return _SEQ[name]


def _module(c, dev, dtype, pieces=2):
    from graphvqa_amd.lcgn import lcgn_seq
    m = lcgn_seq(c["Din"], c["O"], c["Din"], 5, gat_cmd_dim=c["O"], question_dim=c["O"], gat_heads=c["H"], node_feature_dtype=dtype,
                 bf16_weight_pieces=pieces)
    missing, unexpected = m.load_state_dict({k: t(v) for k, v in c["p"].items()}, strict=False)
    assert not unexpected and all(k.startswith("bns.") for k in missing), (missing, unexpected)
    return m.to(dev).eval()


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("case", ["small_h2", "small_h4", "n390_40_64_8", "n390_300_512_4"])
def test_lcgn_seq_bf16_heads_eval(dev, case, pieces):
    """Bounds of tests/test_gpu_gat.py::test_lcgn_bf16_node_features: <= 3e-3 of the output scale against the same-rounding
    emulation; with two weight pieces <= 2.5e-3 against the fp64 oracle on bf16-stored node tensors, and the storage is real: the
    output sits closer to that oracle than half the fp32 oracle's distance from it.  (Single-piece weights are not held to the
    storage oracle, as in that test: on the CPU the emulation itself sits 2.5e-3 .. 3.2e-3 of the scale from it, the fp32 oracle
    1.3e-3 .. 2.5e-3; two pieces: 2.8e-4 .. 3.7e-4.)  The fp32 mode's output differs."""
    c = _seq_case(case)
    m = _module(c, dev, torch.bfloat16, pieces)
    args = [t(a, device=dev) for a in c["inputs"]]
    with torch.no_grad():
        out = m(*args, x_ctx_init=t(c["xc"], device=dev))
        out2 = m(*args, x_ctx_init=t(c["xc"], device=dev))
        out32 = _module(c, dev, torch.float32)(*args, x_ctx_init=t(c["xc"], device=dev))
    ref, ref_st, emu = c["ref"], c["ref_st"], c["emu"][pieces]
    scale = float(ref.abs().max())
    storage_effect = maxabs(ref, ref_st)
    print("lcgn_seq bf16 heads %s pieces=%d: vs emulation %.3e, vs bf16-storage fp64 oracle %.3e, fp32 oracle vs storage oracle %.3e, "
          "vs fp32 mode %.3e, scale %.3e" % (case, pieces, maxabs(out, emu), maxabs(out, ref_st), storage_effect, maxabs(out, out32), scale))
    assert out.dtype == torch.float32 and out.shape == ref.shape and torch.equal(out, out2)
    assert maxabs(out, emu) < 3e-3 * max(scale, 1.0)
    if pieces == 2:         # (single-piece weights add 2^-9 to every product: 1.2 - 1.9 x the storage effect in the emulation itself)
        assert maxabs(out, ref_st) < 2.5e-3 * max(scale, 1.0)
        assert maxabs(out, ref_st) < 0.5 * storage_effect
    assert maxabs(out32, ref) < 1e-4
    assert maxabs(out, out32) > 1e-5


def test_lcgn_seq_bf16_heads_outside_the_bf16_kernels_shapes(dev):
    """out_channels = 12 (not a multiple of 8): the rounding road on the fp32 kernels, same rounding points."""
    from graphvqa_amd.lcgn import lcgn_seq
    H, Din, O, L = 2, 10, 12, 5
    gb = synth.make_graph_batch(4, seed=0x12C, nodes_lo=2, nodes_hi=9, rel_per_node=1.5)
    N, B = gb.num_nodes, gb.num_graphs
    p = synth.lcgn_seq_params(Din, O, seed=5, cmd_dim=O, question_dim=O, heads=H)
    c = dict(H=H, Din=Din, O=O, p=p)
    x, q, lstm, xc = synth.normal((N, Din), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3), synth.normal((N, O), 4)
    with torch.no_grad():
        out = _module(c, dev, torch.bfloat16)(*[t(a, device=dev) for a in (x, gb.edge_index, gb.batch, q, lstm)], x_ctx_init=t(xc, device=dev))
    tp = tparams(p)
    ref = R.lcgn_seq(t(x), t(gb.edge_index), t(gb.batch), t(q), t(lstm), tp, t(xc), heads=H)
    d64 = lambda v: t(v).double()
    ref_st = R.lcgn_seq(d64(x), t(gb.edge_index), t(gb.batch), d64(q), d64(lstm), {k: v.double() for k, v in tp.items()}, d64(xc), heads=H,
                        node_store=R.bf16_storage).float()
    scale = float(ref.abs().max())
    assert maxabs(out, ref_st) < 2.5e-3 * max(scale, 1.0)
    assert maxabs(out, ref) > 1e-5


# ---- lcgn_seq, differentiable -----------------------------------------------------------------------------------------------------
def test_lcgn_seq_bf16_heads_are_trainable(dev):
    """tests/test_gpu_backward.py::test_lcgn_bf16_node_features_are_trainable with two heads: the differentiable road rounds the
    per-node tensors where the eval road stores them (straight-through gradient).  Forward within 3e-3 of the output scale of the
    bf16 eval road; gradients within 5 % of each gradient's scale (floor: 1e-2 of the largest) of fp64 autograd through the oracle;
    the output really differs from the fp32 module's."""
    H = 2
    gb = synth.make_graph_batch(12, seed=0xBF16, nodes_lo=4, nodes_hi=20, rel_per_node=1.5)
    N, B, O, L, Din = gb.num_nodes, gb.num_graphs, 64, 6, 40
    p = synth.lcgn_seq_params(Din, O, seed=21, cmd_dim=O, question_dim=O, heads=H)
    c = dict(H=H, Din=Din, O=O, p=p)
    m, m32 = _module(c, dev, torch.bfloat16), _module(c, dev, torch.float32)
    x, q, lstm, xc, w = (synth.normal((N, Din), 1), synth.normal((B, O), 2), synth.normal((L, B, O), 3),
                         synth.normal((N, O), 4), synth.normal((N, O), 5))
    ei, b = t(gb.edge_index, device=dev), t(gb.batch, device=dev)
    grads = {}
    for name, mod in (("bf16", m), ("fp32", m32)):
        xs = [t(a, device=dev).requires_grad_(True) for a in (x, q, lstm)]
        out = mod(xs[0], ei, b, xs[1], xs[2], x_ctx_init=t(xc, device=dev))
        (out * t(w, device=dev)).sum().backward()
        grads[name] = (out.detach(), [v.grad for v in xs], {k: v.grad for k, v in mod.named_parameters() if not k.startswith("bns.")})
    rp = {k: v.double().requires_grad_(True) for k, v in tparams(p).items() if v.is_floating_point()}
    rs = [t(a).double().requires_grad_(True) for a in (x, q, lstm)]
    ref = R.lcgn_seq(rs[0], t(gb.edge_index), t(gb.batch), rs[1], rs[2], rp, t(xc).double(), heads=H)
    (ref * t(w).double()).sum().backward()
    scale = float(ref.detach().abs().max())
    with torch.no_grad():
        fused = m(t(x, device=dev), ei, b, t(q, device=dev), t(lstm, device=dev), x_ctx_init=t(xc, device=dev))
    out_b, gin_b, gp_b = grads["bf16"]
    print("lcgn_seq bf16 heads autograd: forward vs bf16 eval road %.3e, vs fp64 oracle %.3e, vs fp32 module %.3e (scale %.3e)" %
          (maxabs(out_b, fused), maxabs(out_b, ref), maxabs(out_b, grads["fp32"][0]), scale))
    assert maxabs(out_b, fused) < 3e-3 * max(scale, 1.0)
    assert maxabs(out_b, grads["fp32"][0]) > 1e-5
    floor = 1e-2 * max(float(v.grad.abs().max()) for v in list(rp.values()) + rs if v.grad is not None)
    bad = {}
    for got, r, name in zip(gin_b, rs, ("x", "q_encoding", "lstm_outputs")):
        bad[name] = _rel(got, r.grad, floor)
    for k, g in gp_b.items():
        rg = rp[k].grad if rp[k].grad is not None else torch.zeros_like(rp[k])
        bad[k] = _rel(g if g is not None else torch.zeros_like(rg), rg, floor)
    print("lcgn_seq bf16 heads autograd: worst gradient deviation from the fp64 oracle %.3e" % max(bad.values()))
    bad = {k: e for k, e in bad.items() if not e < 5e-2}
    assert not bad, bad
