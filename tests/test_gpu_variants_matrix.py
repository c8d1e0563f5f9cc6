"""GPU checks of the GINE / GCN execution modules (csrc/variants.hip, csrc/gine_mlp.hip) and the BatchNorm kernels (k_bn_relu_chain*
in variants.hip, csrc/bn_train.hip) over every kernel form their dispatch code can select, against the dense fp64 forms of
tests/variants_ref.py on its hard batch (in-degrees 0 .. 9, a 301-in-edge hub, a 301-out-edge source, repeated edges, duplicated self
loops, a node whose only in-edges are self loops, a one-node graph, an empty graph, with and without edges across graphs).  The
condition that selects each form is written beside its case; DESIGN.md ("GINE / GCN / BatchNorm: the test matrix") lists the kernels a
run of this file launches.

Bounds: products on the matrix cores TOL x max(1, |ref|max / 32), TOL = 1e-4; gradients 5e-4 relative with a floor of 1e-3 x the
largest gradient entry; the BatchNorm kernels 1e-5 x max(1, |ref|max), running statistics 1e-6 / 1e-5.  Ill-conditioned BatchNorm
inputs (column means up to 100 x the std, running_var = 0, batch columns with mean 1e4 at std 1 or std 1e-2 at mean 10): 8 x the
distance of the same operation in plain fp32 torch on the CPU from fp64, computed per case, never below the bounds above."""
import numpy as np
import pytest
import torch
from torch.nn import Linear, ReLU, Sequential

from tests import variants_ref as V
from tests.util import maxabs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(ei, batch, N, B, dev):
    from graphvqa_amd.graph import SceneGraphBatch
    return SceneGraphBatch(ei.to(dev), None if batch is None else batch.to(dev), N, B)


def _offset_view(a, dev):
    """`a` on the device as a contiguous view that starts 4 bytes into a fresh allocation: rows that are not 16-byte aligned."""
    flat = torch.empty(a.numel() + 1, dtype=a.dtype, device=dev)
    v = flat[1:].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class _Options:
    """Library options set for a block and restored after it."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        from graphvqa_amd import _lib
        self.old = {k: _lib.set_option(getattr(_lib, k), v) for k, v in self.values.items()}

    def __exit__(self, *exc):
        from graphvqa_amd import _lib
        for k, v in self.old.items():
            _lib.set_option(getattr(_lib, k), v)


# ---- GCN ----------------------------------------------------------------------------------------------------------------------------
def _gcn_conv(c, dev, bias=True):
    from graphvqa_amd.baseline_models import GCNConv
    conv = GCNConv(c["weight"].shape[0], c["weight"].shape[1], bias=bias).to(dev).eval()
    with torch.no_grad():
        conv.weight.copy_(c["weight"])
        if bias:
            conv.bias.copy_(c["bias"])
    return conv


@pytest.mark.parametrize("C", V.GCN_WIDTHS)
def test_gcn_every_aggregate_form_matches_fp64(dev, C):
    """gvqa_gcn_conv_forward: `v4 = C % 4 == 0 && out 16-byte aligned && (no bias || bias 16-byte aligned)`.  C = 1, 30: k_gcn_aggregate;
    C = 4 (one quad), 300 (75 quads: lanes 11 .. 63 of the second group idle), 512 (a full round of 128 quads), 520 (`q0 += 128`: a
    second round of two quads): k_gcn_aggregate_v4.  D = 24 and 36: k_transpose on partial 32-tiles.  The cross list with Di = 12 is the
    P[node_graph[src]] term.  Exact: k_gcn_dis and both aggregates skip every self loop (`src == i`) and add their own, so deleting all
    of them from the list, the duplicated ones included, leaves the order of the remaining edges and the output bits unchanged."""
    with torch.no_grad():
        for Di in (0, V.GCN_DI):
            c = V.gcn_case(C, Di)
            conv = _gcn_conv(c, dev)
            x, ins = c["x"].to(dev), None if Di == 0 else c["ins"].to(dev)
            for kind in (0, 1):
                ei = c["eis"][kind]
                ref = V.gcn_reference(c, kind)
                cpu = maxabs(V.gcn_reference(c, kind, torch.float32), ref)
                g = _graph(ei, c["batch"], c["N"], c["B"], dev)
                assert bool(g.intra_graph) == (kind == 0)
                out = conv(x, ei.to(dev), graph=g, ins=ins)
                d = maxabs(out, ref)
                print(f"gcn C={C} Di={Di} kind={kind}: gpu {d:.3g} cpu32 {cpu:.3g} bound {V.product_bound(ref):.3g}")
                assert bool(torch.isfinite(out).all()) and d < V.product_bound(ref), (Di, kind, d)
                bare = torch.from_numpy(V.without_self_loops(ei.numpy()))
                assert bare.shape[1] < ei.shape[1]
                assert torch.equal(conv(x, bare.to(dev), graph=_graph(bare, c["batch"], c["N"], c["B"], dev), ins=ins), out), (Di, kind)


def test_gcn_bias_forms_no_graph_and_no_edges(dev):
    """At C = 300: bias=None (the `bias ?` arms of both aggregates; v4 still selected); a bias 4 bytes into its allocation (`bias & 15`:
    k_gcn_aggregate at C % 4 == 0), which must agree with the aligned run to the bound; graph=None (one graph, built by the layer);
    E = 0 (every row is its own self loop: out = x W + b)."""
    from graphvqa_amd.baseline_models import GCNConv
    C = 300
    with torch.no_grad():
        for Di in (0, V.GCN_DI):
            c = V.gcn_case(C, Di)
            x, ins = c["x"].to(dev), None if Di == 0 else c["ins"].to(dev)
            aligned = _gcn_conv(c, dev)
            shifted = _gcn_conv(c, dev)
            shifted.bias = torch.nn.Parameter(_offset_view(c["bias"], dev))
            assert shifted.bias.data_ptr() % 16 == 4 and aligned.bias.data_ptr() % 16 == 0
            nobias = _gcn_conv(c, dev, bias=False)
            for kind in (0, 1):
                ei = c["eis"][kind]
                g = _graph(ei, c["batch"], c["N"], c["B"], dev)
                ref = V.gcn_reference(c, kind)
                a, s = aligned(x, ei.to(dev), graph=g, ins=ins), shifted(x, ei.to(dev), graph=g, ins=ins)
                ref0 = V.gcn_reference(c, kind, bias=False)
                n = nobias(x, ei.to(dev), graph=g, ins=ins)
                cpu, cpu0 = maxabs(V.gcn_reference(c, kind, torch.float32), ref), maxabs(V.gcn_reference(c, kind, torch.float32, bias=False), ref0)
                print(f"gcn C=300 Di={Di} kind={kind}: aligned {maxabs(a, ref):.3g} offset bias {maxabs(s, ref):.3g} scalar vs v4 {maxabs(a, s):.3g} "
                      f"cpu32 {cpu:.3g} no bias {maxabs(n, ref0):.3g} cpu32 {cpu0:.3g} bound {V.product_bound(ref):.3g}")
                assert maxabs(s, ref) < V.product_bound(ref) and maxabs(a, s) < V.product_bound(ref)
                assert maxabs(n, ref0) < V.product_bound(ref0)
            empty = torch.zeros((2, 0), dtype=torch.int64)
            c0 = dict(c, eis=(empty, empty))
            ref = V.gcn_reference(c0, 0)
            assert maxabs(ref, torch.cat((c["x"], c["ins"][c["batch"]]), 1).double() @ c["weight"].double() + c["bias"].double()
                          if Di else c["x"].double() @ c["weight"].double() + c["bias"].double()) < 1e-12
            out = aligned(x, empty.to(dev), graph=_graph(empty, c["batch"], c["N"], c["B"], dev), ins=ins)
            print(f"gcn C=300 Di={Di} E=0: gpu {maxabs(out, ref):.3g} cpu32 {maxabs(V.gcn_reference(c0, 0, torch.float32), ref):.3g} "
                  f"bound {V.product_bound(ref):.3g}")
            assert maxabs(out, ref) < V.product_bound(ref)
        c = V.gcn_case(C, 0)                                                  # graph=None: no instruction rows (they are per graph)
        for kind in (0, 1):
            out = _gcn_conv(c, dev)(c["x"].to(dev), c["eis"][kind].to(dev))
            ref = V.gcn_reference(c, kind)
            print(f"gcn C=300 graph=None kind={kind}: gpu {maxabs(out, ref):.3g} cpu32 {maxabs(V.gcn_reference(c, kind, torch.float32), ref):.3g} "
                  f"bound {V.product_bound(ref):.3g}")
            assert maxabs(out, ref) < V.product_bound(ref)


# ---- GINE ---------------------------------------------------------------------------------------------------------------------------
def _gine_conv(c, eps, dev, train_eps=False):
    from graphvqa_amd.baseline_models import GINEConv
    C, D = c["w1"].shape
    conv = GINEConv(Sequential(Linear(D, C), ReLU(), Linear(C, C)), eps=eps, train_eps=train_eps).to(dev).eval()
    conv.load_state_dict({"nn.0.weight": c["w1"], "nn.0.bias": c["b1"], "nn.2.weight": c["w2"], "nn.2.bias": c["b2"],
                          "eps": torch.tensor([eps], dtype=torch.float32)})
    return conv


# OPT_PROJECTION = F32, and SPLIT2H with every product on the library's kernels
GINE_OPTIONS = (dict(OPT_PROJECTION=1), dict(OPT_PROJECTION=2, OPT_SPLIT3_MIN_MFLOP=0))


@pytest.mark.parametrize("Dn", (10, 24, 300))
def test_gine_unfused_forms_match_fp64(dev, Dn):
    """gvqa_gine_conv_forward with N = 320 < 1024: the unfused products.  `vec = Dn % 4 == 0 && (h | edge_attr) 16-byte aligned`:
    Dn = 24, 300 take k_gine_aggregate<true> (in-degrees 0 .. 9: the two-edges-in-flight loop and its odd tail `if (s < hi)`; the hub:
    150 rounds and a tail), Dn = 10 and Dn = 24 on x / edge_attr 4 bytes into their allocations take k_gine_aggregate<false>.
    Di = 12: k_relu2 and k_gine_mid (`deg * P2 + (1 + eps) P1`, eps of either sign); Di = 0: the bias in the product's epilogue."""
    from graphvqa_amd import _lib
    assert (_lib.PROJECTION_F32, _lib.PROJECTION_SPLIT2H) == (1, 2)
    with torch.no_grad():
        for _, Di, C in (s for s in V.GINE_HARD if s[0] == Dn):
            c = V.gine_hard_case(Dn, Di, C)
            g = _graph(c["ei"], c["batch"], c["N"], c["B"], dev)
            ei, ins = c["ei"].to(dev), None if Di == 0 else c["ins"].to(dev)
            forms = [("aligned", c["x"].to(dev), c["ea"].to(dev))]
            if Dn == 24:
                forms.append(("offset", _offset_view(c["x"], dev), _offset_view(c["ea"], dev)))
            for eps in V.GINE_EPS:
                ref = V.gine_reference(c, eps)
                cpu = maxabs(V.gine_reference(c, eps, torch.float32), ref)
                conv = _gine_conv(c, eps, dev)
                for options in GINE_OPTIONS:
                    for name, x, ea in forms:
                        with _Options(**options):
                            out = conv(x, ei, ea, graph=g, ins=ins)
                        d = maxabs(out, ref)
                        print(f"gine Dn={Dn} Di={Di} C={C} eps={eps} {options} {name}: gpu {d:.3g} cpu32 {cpu:.3g} bound {V.product_bound(ref):.3g}")
                        assert bool(torch.isfinite(out).all()) and d < V.product_bound(ref), (Di, C, eps, options, name, d)


@pytest.mark.parametrize("N,Dn,C,Di", V.GINE_WIDE)
def test_gine_fused_mlp_thresholds_match_fp64(dev, N, Dn, C, Di):
    """`OPT_PROJECTION == SPLIT2H && N >= 1024 && gine_mlp_supported (8 <= C <= 320, C % 4 == 0, Dn >= 8, Dn % 4 == 0) && ld1 % 4 == 0`
    selects k_gine_pack_w + k_gine_mlp (with Di > 0: k_ins_cat and one [2 B, Di] product).  N = 1101 = 8 row tiles of 128 and a 77-row
    tail, at (24, 320, 12) the widest tile count, (300, 300, 0) the reference's widths, (8, 8, 8) the narrowest; N = 1023 and C = 324
    take the unfused form one row / one quad beyond the thresholds."""
    c = V.gine_wide_case(N, Dn, C, Di)
    with torch.no_grad():
        g = _graph(c["ei"], c["batch"], N, c["B"], dev)
        conv = _gine_conv(c, 0.25, dev)
        with _Options(OPT_PROJECTION=2, OPT_SPLIT3_MIN_MFLOP=0):
            out = conv(c["x"].to(dev), c["ei"].to(dev), c["ea"].to(dev), graph=g, ins=None if Di == 0 else c["ins"].to(dev))
    ref = V.gine_reference(c, 0.25)
    d, cpu = maxabs(out, ref), maxabs(V.gine_reference(c, 0.25, torch.float32), ref)
    print(f"gine wide N={N} Dn={Dn} C={C} Di={Di}: gpu {d:.3g} cpu32 {cpu:.3g} bound {V.product_bound(ref):.3g}")
    assert bool(torch.isfinite(out).all()) and d < V.product_bound(ref), d


@pytest.mark.parametrize("eps", V.GINE_EPS)
def test_gine_fused_mlp_instruction_share_with_either_sign_of_eps(dev, eps):
    """k_gine_mlp's `e1p * p1 + degp * p2` between the layers, at 1 + eps = 1.25 and 0.5, on wide_batch(1101) with its hub (deg = 301)."""
    N, Dn, C, Di = V.GINE_WIDE[0]
    c = V.gine_wide_case(N, Dn, C, Di)
    with torch.no_grad():
        g = _graph(c["ei"], c["batch"], N, c["B"], dev)
        with _Options(OPT_PROJECTION=2, OPT_SPLIT3_MIN_MFLOP=0):
            out = _gine_conv(c, eps, dev)(c["x"].to(dev), c["ei"].to(dev), c["ea"].to(dev), graph=g, ins=c["ins"].to(dev))
    ref = V.gine_reference(c, eps)
    cpu = maxabs(V.gine_reference(c, eps, torch.float32), ref)
    print(f"gine wide eps={eps}: gpu {maxabs(out, ref):.3g} cpu32 {cpu:.3g} bound {V.product_bound(ref):.3g}")
    assert maxabs(out, ref) < V.product_bound(ref)


def test_gine_fused_mlp_dead_rows_come_out_as_the_bias(dev):
    """Rows without in-edges whose x is 0 (`zmax = 0`: split2h_exponent's zero-row arm in layer 1) or 1e-20 (zmax > 0), under a negative
    nn.0.bias: the hidden row is relu(<= 0) = 0 (`ymax = 0`: the zero-row arm in layer 2), so the row is nn.2.bias to the bit."""
    N, Dn, C = 1101, 24, 320
    c = V.gine_wide_case(N, Dn, C, 0, dead=True)
    with torch.no_grad():
        g = _graph(c["ei"], c["batch"], N, c["B"], dev)
        with _Options(OPT_PROJECTION=2, OPT_SPLIT3_MIN_MFLOP=0):
            out = _gine_conv(c, 0.25, dev)(c["x"].to(dev), c["ei"].to(dev), c["ea"].to(dev), graph=g).cpu()
    ref = V.gine_reference(c, 0.25)
    rows = c["dead_rows"]
    assert torch.equal(out[rows], c["b2"].expand(len(rows), -1))
    live = torch.ones(N, dtype=torch.bool)
    live[rows] = False
    cpu = maxabs(V.gine_reference(c, 0.25, torch.float32)[live], ref[live])
    print(f"gine dead rows: the others gpu {maxabs(out[live], ref[live]):.3g} cpu32 {cpu:.3g} bound {V.product_bound(ref):.3g}")
    assert maxabs(out[live], ref[live]) < V.product_bound(ref)


# ---- the BN -> ReLU chain -----------------------------------------------------------------------------------------------------------
def _bns(stages, C, dev):
    bns = []
    for w, b, m, v in stages:
        bn = torch.nn.BatchNorm1d(C, eps=V.BN_EPS)
        bn.load_state_dict({"weight": w, "bias": b, "running_mean": m, "running_var": v, "num_batches_tracked": torch.tensor(0)})
        bns.append(bn.to(dev).eval())
    return bns


@pytest.mark.parametrize("N,C,offset", V.CHAIN_SHAPES)
def test_bn_relu_chain_forms_match_fp64(dev, N, C, offset):
    """gvqa_bn_relu_chain: `C % 4 == 0 && C <= 512 && (x | out) 16-byte aligned` selects k_bn_relu_chain_v4 on min(total4 / 256, 8 per
    CU) blocks, else k_bn_relu_chain on min(total / 256, 2048) blocks.  (322, 300): v4; (322, 30): scalar; (1101, 516): scalar at
    C > 512, 2220 blocks' worth on 2048; (4300, 512): v4, 2150 blocks' worth on 8 per CU; (322, 24) on an x 4 bytes into its
    allocation: scalar.  0, 1, 4 and 8 stages; nine raise.  Column means up to 100 x the std, one stage each with running_var = 0,
    negative and zero weights: the bound is 8 x the distance of torch's own fp32 eval BatchNorm on the CPU, never below the plain one."""
    from graphvqa_amd import _lib
    from graphvqa_amd.baseline_models import _bn_relu_chain
    with torch.no_grad():
        for S in V.CHAIN_STAGES:
            x, stages = V.chain_case(N, C, S)
            ref = V.bn_chain(x.double(), stages)
            cpu = maxabs(V.bn_chain_fp32(x, stages), ref)
            xd = _offset_view(x, dev) if offset else x.to(dev)
            assert xd.data_ptr() % 16 == (4 if offset else 0)
            out = _bn_relu_chain(xd, _bns(stages, C, dev))
            d, bound = maxabs(out, ref), max(V.MARGIN * cpu, V.plain_bound(ref))
            print(f"chain N={N} C={C} S={S}: gpu {d:.3g} cpu32 {cpu:.3g} bound {bound:.3g}")
            assert bool(torch.isfinite(out).all()) and d < bound, (S, d, cpu)
            if S == 0:
                assert torch.equal(out.cpu(), x)
        x, stages = V.chain_case(N, C, 8)
        with pytest.raises(_lib.GvqaError):
            _bn_relu_chain(x.to(dev), _bns(stages + stages[:1], C, dev))


# ---- train-mode BatchNorm + ReLU ------------------------------------------------------------------------------------------------------
def _bn_train_gpu(c, masked, dev):
    from graphvqa_amd.gat_skip import _BatchNormReluTrain, _bn_relu_train
    bn = torch.nn.BatchNorm1d(c["C"], eps=V.BN_EPS)
    with torch.no_grad():
        bn.weight.copy_(c["w"]); bn.bias.copy_(c["b"])
    bn = bn.to(dev).train()
    x = c["x"].detach().clone().to(dev).requires_grad_(True)
    if masked:          # the explicit keep mask, as test_bn_relu_with_feature_dropout_in_the_same_passes passes it
        y, mean, var = _BatchNormReluTrain.apply(x, bn.weight, bn.bias, V.BN_EPS, c["keep"].to(dev), 1.0 / 0.75)
        n = c["N"]
        stats = dict(running_mean=0.1 * mean, running_var=0.9 + 0.1 * var * (n / (n - 1)), mean=mean.detach(), var=var.detach())
    else:               # the module road: running statistics and num_batches_tracked updated by _bn_relu_train
        y = _bn_relu_train(bn, x)
        assert int(bn.num_batches_tracked) == 1
        stats = dict(running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())
    y.backward(c["dy"].to(dev))
    return dict(y=y.detach(), dx=x.grad, dweight=bn.weight.grad, dbias=bn.bias.grad, **stats)


@pytest.mark.parametrize("N,C", V.BN_TRAIN_SHAPES)
def test_bn_train_forms_and_block_m2_variance_match_fp64(dev, N, C):
    """bn_train.hip: `v4 = C % 4 == 0 && 16-byte aligned rows`, TPR = the power of two >= C / 4, at most 256.  (65, 4): TPR = 1 and a
    second row block of one row; (129, 1028): C / 4 = 257 > TPR = 256, the second column trip of k_bn_relu_apply_v4 /
    k_bn_relu_bwd_reduce_v4 / k_bn_relu_bwd_apply_v4, five 256-column blocks of k_bn_col_stats_fused, a last row block of one row;
    (64, 6): the scalar kernels; (2, 8): the smallest batch; (257, 300): TPR = 128, 53 idle column threads.  k_bn_col_stats_fused +
    k_bn_col_finish_m2 on columns with mean up to 1e4 at std 1, std 1e-2 at mean 10 and a constant column: E[x^2] - E[x]^2 in fp32 is
    off by more than the variance itself there; one column whose row 0 (bn_pivot's first probe row) is at 1e4 and the rest at 10 +- 1.
    Each kind of column is judged on its own.  Ordinary columns (mean 0.5, std 2): the plain bounds; every other kind: 8 x the distance
    of the two-pass fp32 form on the CPU on those columns, never below the plain bounds.  With a mask the batch mean and variance that
    _BatchNormReluTrain returns are compared too (plain bound 1e-5 x max(1, |ref|max)).  The constant column's variance is exactly 0."""
    c = V.bn_train_case(N, C)
    strata = V.bn_strata(c["kind"])
    for masked in (False, True):
        ref, nbt = V.bn_train_fp64(c, masked)
        cpu = V.bn_train_fp32(c, masked)
        got = _bn_train_gpu(c, masked, dev)
        assert nbt == 1 and all(bool(torch.isfinite(v).all()) for v in got.values())
        bad = {}
        for name, cols in strata.items():
            d, d32, plain = V.bn_distances(got, ref, cols), V.bn_distances(cpu, ref, cols), V.bn_plain_bounds(ref, cols)
            print(f"bn-train N={N} C={C} masked={masked} {name}: " + " ".join(f"{k} gpu {d[k]:.3g} cpu32 {d32[k]:.3g}" for k in d))
            for k in d:
                bound = plain[k] if name == "ordinary" else max(V.MARGIN * d32[k], plain[k])
                if not d[k] < bound:
                    bad[(name, k)] = (d[k], d32[k], bound)
        assert not bad, (masked, bad)
        const = V.BN_CONSTANT_COLUMN
        assert float(got["running_var"][const]) == pytest.approx(0.9, abs=1e-7)               # 0.9 x 1 + 0.1 x 0
        if not masked:                                                                         # (x - mean) is exactly 0: y = relu(bias)
            assert torch.equal(got["y"][:, const].cpu(), torch.relu(c["b"][const]).expand(N))


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
def _check_grads(name, got, ref):
    e = V.grad_errors(got, ref)
    print(f"{name}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
    bad = {k: v for k, v in e.items() if not v < V.GRAD_TOL}
    assert not bad, (name, bad)


def test_gine_gradients_with_trainable_eps_match_fp64_autograd(dev):
    """GINEConv(train_eps=True) called with graph= and ins= on both edge lists of the hard batch: every parameter, eps included, x,
    edge_attr and ins against autograd through the dense fp64 form; the same weights under no_grad (the inference kernels; on the
    cross list the concatenated form, as gine_seq calls it) agree with the training forward to the forward bound."""
    c = V.grad_case()
    for kind in (0, 1):
        ei = c["eis"][kind]
        g = _graph(ei, c["batch"], c["N"], c["B"], dev)
        conv = _gine_conv(c, float(c["eps"]), dev, train_eps=True)
        assert isinstance(conv.eps, torch.nn.Parameter)
        x, ea, ins = (c[k].detach().clone().to(dev).requires_grad_(True) for k in ("x", "ea", "ins"))
        out = conv(x, ei.to(dev), ea, graph=g, ins=ins)
        (out * c["w"].to(dev)).sum().backward()
        rout, ref = V.gine_grad_reference(c, kind)
        assert maxabs(out, rout) < V.product_bound(rout), kind
        got = {"x": x.grad, "ea": ea.grad, "ins": ins.grad, "w1": conv.nn[0].weight.grad, "b1": conv.nn[0].bias.grad,
               "w2": conv.nn[2].weight.grad, "b2": conv.nn[2].bias.grad, "eps": conv.eps.grad}
        assert all(v is not None for v in got.values()) and conv.eps.grad.shape == (1,)
        _check_grads(f"gine gradients kind={kind}", got, ref)
        with torch.no_grad():
            if kind == 0:
                fout = conv(x, ei.to(dev), ea, graph=g, ins=ins)
            else:
                b = c["batch"].to(dev)
                fout = conv(torch.cat((x, ins[b]), -1), ei.to(dev), torch.cat((ea, ins[b[ei.to(dev)[0]]]), -1), graph=g)
        assert maxabs(fout, out) < V.product_bound(rout), kind


@pytest.mark.parametrize("bias", (True, False))
def test_gcn_gradients_match_fp64_autograd(dev, bias):
    """GCNConv with and without bias, called with graph= and ins= on both edge lists: weight, bias, x and ins against autograd through
    the dense fp64 form; the same weights under no_grad (k_gcn_dis, k_gcn_aggregate_v4) agree with the training forward."""
    c = V.grad_case()
    for kind in (0, 1):
        ei = c["eis"][kind]
        g = _graph(ei, c["batch"], c["N"], c["B"], dev)
        conv = _gcn_conv(c, dev, bias=bias)
        x, ins = (c[k].detach().clone().to(dev).requires_grad_(True) for k in ("x", "ins"))
        out = conv(x, ei.to(dev), graph=g, ins=ins)
        (out * c["w"].to(dev)).sum().backward()
        rout, ref = V.gcn_grad_reference(c, kind, bias)
        assert maxabs(out, rout) < V.product_bound(rout), kind
        got = {"x": x.grad, "ins": ins.grad, "weight": conv.weight.grad}
        if bias:
            got["bias"] = conv.bias.grad
        _check_grads(f"gcn gradients kind={kind} bias={bias}", got, ref)
        with torch.no_grad():
            fout = conv(x, ei.to(dev), graph=g, ins=ins)
        assert maxabs(fout, out) < V.product_bound(rout), kind
