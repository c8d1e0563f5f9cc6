"""Shared pieces of the GINE / GCN / BatchNorm kernel tests (no GPU needed to import): the hard batch with the self-loop shapes GCN
needs on top of tests/lcgn_ref.py::hard_batch, a wider ragged batch cut to an exact node count, the dense fp64 references (written
from the formulas, independently of oracle/ref_torch.py), the same operations in plain fp32 torch on the CPU (the yardstick of the
scaled bounds: a kernel may be 8 x as far from fp64 as they are), and the inputs of every case of tests/test_gpu_variants_matrix.py,
which its CPU companion tests/test_variants_ref_host.py holds to a conditioning cap."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from graphvqa_amd import synth
from tests import lcgn_ref
from tests.util import t, maxabs

TOL = 1e-4                  # products on the matrix cores: TOL x max(1, |ref|max / 32)
GRAD_TOL = 5e-4             # gradients: relative, floor 1e-3 x the largest entry of any gradient
MARGIN = 8.0                # a kernel that sums in another order than the fp32 CPU form may be this many times as far from fp64
BN_EPS = 1e-5


def product_bound(ref):
    return TOL * max(1.0, float(ref.abs().max()) / 32.0)


def plain_bound(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


def well_conditioned(fp32_distance, ref):
    """The cap every scaled case is held to on the CPU: MARGIN x the fp32 form's distance stays below 1e-2 x |ref|max."""
    return MARGIN * fp32_distance < 1e-2 * float(ref.abs().max())


# ---- batches ------------------------------------------------------------------------------------------------------------------------
def _loop_counts(e, N):
    loop = e[0] == e[1]
    return np.bincount(e[1][loop], minlength=N), np.bincount(e[1][~loop], minlength=N)


@functools.lru_cache(maxsize=None)
def hard_batch():
    """lcgn_ref.hard_batch (320 nodes: in-degrees 0 .. 9, a 301-in-edge destination, a 301-out-edge source, repeated edges, a one-node
    graph with a self loop, an empty graph in the middle; a second edge list with cross-graph sources) plus two edges, appended to both
    lists, for GCN's add_remaining_self_loops: a second self loop on the one-node graph's node (`only_loops`: all its in-edges are self
    loops, so its degree is 1) and a second self loop on a node of the last graph that also has other in-edges (`double_loop`).  Every
    property is asserted here.  -> (GraphBatch, cross edge list, info)."""
    gb, cross, info = lcgn_ref.hard_batch()
    N, B = gb.num_nodes, gb.num_graphs
    only = int(np.flatnonzero(gb.batch == info["single_graph"])[0])
    double = None
    for n in np.flatnonzero(gb.batch == B - 1):
        counts = [(_loop_counts(e, N)[0][n], _loop_counts(e, N)[1][n]) for e in (gb.edge_index, cross)]
        if all(l == 1 and p >= 1 for l, p in counts):
            double = int(n)
            break
    assert double is not None
    extra = np.array([[only, double], [only, double]], dtype=np.int64)
    ei, cr = np.concatenate([gb.edge_index, extra], 1), np.concatenate([cross, extra], 1)
    info = dict(info, only_loops=only, double_loop=double)
    g0 = np.flatnonzero(gb.batch == 0)
    for name, e in (("intra", ei), ("cross", cr)):
        loops, plain = _loop_counts(e, N)
        indeg = np.bincount(e[1], minlength=N)
        assert loops[only] == 2 and plain[only] == 0, name                             # only self loops, two of them
        assert loops[double] == 2 and plain[double] >= 1, name                         # a duplicated self loop beside other in-edges
        assert bool(((loops == 1) & (plain >= 1)).any()), name                         # one self loop beside other in-edges
        assert bool(((loops == 0) & (plain >= 1)).any()), name                         # no self loop at all
        assert set(range(10)) <= set(indeg[g0].tolist()) and indeg[info["isolated"]] == 0, name
        assert indeg[info["hub_in"]] == lcgn_ref.HUB_DEGREE and plain[info["hub_in"]] == lcgn_ref.HUB_DEGREE, name
        assert np.bincount(e[0], minlength=N)[info["hub_out"]] == lcgn_ref.HUB_DEGREE, name
        assert int(np.bincount(e[0] * N + e[1], minlength=N * N).max()) >= 2, name
    assert bool((gb.batch[ei[0]] == gb.batch[ei[1]]).all()) and bool((gb.batch[cr[0]] != gb.batch[cr[1]]).any())
    assert np.bincount(gb.batch, minlength=B)[info["empty_graph"]] == 0
    ei.setflags(write=False); cr.setflags(write=False)
    return synth.GraphBatch(edge_index=ei, batch=gb.batch, num_graphs=B), cr, info


def without_self_loops(ei):
    return np.ascontiguousarray(ei[:, ei[0] != ei[1]])


@functools.lru_cache(maxsize=None)
def wide_batch(N):
    """hard_batch followed by generated ragged graphs (5 .. 40 nodes, about 1.5 relations per node, a self loop on every node), cut to
    exactly N nodes: the last graph keeps its first nodes and the edges among them.  Intra-graph edges only."""
    gb, _, _ = hard_batch()
    n0, b0 = gb.num_nodes, gb.num_graphs
    assert N > n0
    tail = synth.make_graph_batch((N - n0) // 5 + 1, seed=0x1101, nodes_lo=5, nodes_hi=40, rel_per_node=1.5)
    cut = N - n0
    assert tail.num_nodes >= cut
    keep = (tail.edge_index[0] < cut) & (tail.edge_index[1] < cut)
    ei = np.concatenate([gb.edge_index, tail.edge_index[:, keep] + n0], 1)
    batch = np.concatenate([gb.batch, tail.batch[:cut] + b0])
    B = int(batch[-1]) + 1
    assert batch.shape[0] == N and bool((np.diff(batch) >= 0).all()) and bool((batch[ei[0]] == batch[ei[1]]).all())
    sizes = np.bincount(batch, minlength=B)[b0:]
    assert sizes.min() >= 1 and sizes.max() <= 40 and len(set(sizes.tolist())) > 10                  # ragged
    ei.setflags(write=False); batch.setflags(write=False)
    return synth.GraphBatch(edge_index=ei, batch=batch, num_graphs=B)


# ---- GCN ----------------------------------------------------------------------------------------------------------------------------
def gcn_dense(x, weight, bias, ei, ins=None, batch=None):
    """out = D^-1/2 A D^-1/2 (x W) + b with A[dst, src] = the multiplicity of the edge, the diagonal (every self loop) replaced by 1,
    deg = A.sum(1); weight [in, out]; with `ins` the node rows are [x || ins[batch]].  Any dtype; differentiable."""
    N = x.shape[0]
    xc = x if ins is None else torch.cat((x, ins[batch]), 1)
    A = torch.zeros((N, N), dtype=x.dtype).index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=x.dtype), accumulate=True)
    A.fill_diagonal_(1.0)
    dis = A.sum(1).pow(-0.5)
    out = dis[:, None] * (A @ (dis[:, None] * (xc @ weight)))
    return out if bias is None else out + bias


GCN_WIDTHS = (1, 30, 4, 300, 512, 520)      # scalar aggregate: 1, 30; v4: one quad, a partial second lane group, a full round, a second round
GCN_DN, GCN_DI = 24, 12


@functools.lru_cache(maxsize=None)
def gcn_case(C, Di):
    """CPU fp32 tensors of one GCN case on hard_batch: x [N, 24], ins [B, Di] or None, weight [24 + Di, C], bias [C]."""
    gb, cross, _ = hard_batch()
    N, B, D = gb.num_nodes, gb.num_graphs, GCN_DN + Di
    return dict(x=t(synth.normal((N, GCN_DN), 21)), ins=t(synth.normal((B, Di), 22)) if Di else None,
                weight=t(synth.normal((D, C), 23 + C) / np.float32(np.sqrt(D))), bias=t(synth.normal((C,), 24) * np.float32(0.5)),
                eis=(t(gb.edge_index.copy()), t(cross.copy())), batch=t(gb.batch.copy()), N=N, B=B)


def gcn_reference(c, kind, dtype=torch.float64, bias=True):
    cast = lambda v: None if v is None else v.to(dtype)
    return gcn_dense(cast(c["x"]), cast(c["weight"]), cast(c["bias"]) if bias else None, c["eis"][kind], cast(c["ins"]), c["batch"])


# ---- GINE ---------------------------------------------------------------------------------------------------------------------------
def gine_dense(x, ea, ei, w1, b1, w2, b2, eps, ins=None, batch=None):
    """nn((1 + eps) x + sum over in-edges of relu(x_src + e)), nn = Lin(w1, b1) -> ReLU -> Lin(w2, b2); the sum as the product with the
    [N, E] incidence matrix; with `ins`, x and e are [x || ins[batch]] and [e || ins[batch[src]]].  Any dtype; differentiable."""
    N, E = x.shape[0], ei.shape[1]
    if ins is not None:
        x, ea = torch.cat((x, ins[batch]), 1), torch.cat((ea, ins[batch[ei[0]]]), 1)
    S = torch.zeros((N, E), dtype=x.dtype)
    S[ei[1], torch.arange(E)] = 1.0
    z = (1.0 + eps) * x + S @ torch.relu(x[ei[0]] + ea)
    return torch.relu(z @ w1.t() + b1) @ w2.t() + b2


GINE_EPS = (0.25, -0.5)
GINE_HARD = [(Dn, Di, C) for Dn in (10, 24, 300) for Di in (0, 12) for C in (8, 30, 300)]
# (N, Dn, C, Di) of the cases around the fused MLP's thresholds (N >= 1024, C <= 320): fused, fused, fused, one row short, one quad wide
GINE_WIDE = [(1101, 24, 320, 12), (1101, 300, 300, 0), (1101, 8, 8, 8), (1023, 24, 320, 12), (1101, 24, 324, 12)]


def _gine_weights(Dn, Di, C, seed):
    rng = np.random.default_rng(seed)
    w = lambda *shape: (rng.standard_normal(shape) / np.sqrt(shape[-1])).astype(np.float32)
    return dict(w1=t(w(C, Dn + Di)), b1=t(w(C)), w2=t(w(C, C)), b2=t(w(C)))


@functools.lru_cache(maxsize=None)
def gine_hard_case(Dn, Di, C):
    gb, _, _ = hard_batch()
    N, E, B = gb.num_nodes, gb.num_edges, gb.num_graphs
    return dict(x=t(synth.normal((N, Dn), 31)), ea=t(synth.normal((E, Dn), 32)), ins=t(synth.normal((B, Di), 33)) if Di else None,
                ei=t(gb.edge_index.copy()), batch=t(gb.batch.copy()), N=N, B=B, **_gine_weights(Dn, Di, C, 1000 * Dn + 10 * Di + C))


@functools.lru_cache(maxsize=None)
def gine_wide_case(N, Dn, C, Di, dead=False):
    """The fused test's inputs on wide_batch(N): a few rows far above and far below the rest (the row scales are per row), one output
    channel of layer 2 far below its neighbours.  dead: nn.0.bias = -(|b| + 0.01), the x rows of all but one node without in-edges 0
    (zmax = 0) and the last such node's 1e-20 x its row (zmax > 0, the hidden row still dead): `dead_rows` must come out as nn.2.bias."""
    gb = wide_batch(N)
    E, B = gb.num_edges, gb.num_graphs
    rng = np.random.default_rng(7 * Dn + C + N)
    x, ea = synth.normal((N, Dn), 41), synth.normal((E, Dn), 42)
    x[rng.integers(0, N, size=5)] *= 300.0
    x[rng.integers(0, N, size=5)] *= 1e-3
    c = dict(ea=t(ea), ins=t(synth.normal((B, Di), 43)) if Di else None, ei=t(gb.edge_index.copy()), batch=t(gb.batch.copy()), N=N, B=B,
             **_gine_weights(Dn, Di, C, 2000 * Dn + 10 * Di + C))
    c["w2"][C // 2] *= 1e-4
    if dead:
        assert Di == 0
        rows = np.flatnonzero(np.bincount(gb.edge_index[1], minlength=N) == 0)
        assert len(rows) >= 2 and hard_batch()[2]["isolated"] in rows
        x[rows[:-1]] = 0.0
        x[rows[-1]] = synth.normal((Dn,), 44) * np.float32(1e-20)
        c["b1"] = -(c["b1"].abs() + 0.01)
        c["dead_rows"] = t(rows)
    c["x"] = t(x)
    return c


def gine_reference(c, eps, dtype=torch.float64):
    cast = lambda v: None if v is None else v.to(dtype)
    return gine_dense(cast(c["x"]), cast(c["ea"]), c["ei"], cast(c["w1"]), cast(c["b1"]), cast(c["w2"]), cast(c["b2"]), eps, cast(c["ins"]),
                      c["batch"])


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
GRAD_DN, GRAD_DI, GRAD_C = 24, 12, 24


@functools.lru_cache(maxsize=None)
def grad_case():
    """Operands of the gradient checks on hard_batch (both edge lists): GINE and GCN weights at Dn = 24, Di = 12, C = 24, the loss
    weights w [N, C]."""
    gb, cross, _ = hard_batch()
    N, E, B = gb.num_nodes, gb.num_edges, gb.num_graphs
    D = GRAD_DN + GRAD_DI
    return dict(x=t(synth.normal((N, GRAD_DN), 51)), ea=t(synth.normal((E, GRAD_DN), 52)), ins=t(synth.normal((B, GRAD_DI), 53)),
                w=t(synth.normal((N, GRAD_C), 54)), eis=(t(gb.edge_index.copy()), t(cross.copy())), batch=t(gb.batch.copy()), N=N, B=B,
                eps=t(np.array([0.25], dtype=np.float32)), weight=t(synth.normal((D, GRAD_C), 55) / np.float32(np.sqrt(D))),
                bias=t(synth.normal((GRAD_C,), 56) * np.float32(0.5)), **_gine_weights(GRAD_DN, GRAD_DI, GRAD_C, 57))


GINE_GRAD_NAMES = ("x", "ea", "ins", "w1", "b1", "w2", "b2", "eps")
GCN_GRAD_NAMES = ("x", "ins", "weight", "bias")


def gine_grad_reference(c, kind, dtype=torch.float64):
    """(out, {name: gradient}) of gine_dense in `dtype`, loss (out * w).sum()."""
    leaves = {k: c[k].detach().clone().to(dtype).requires_grad_(True) for k in GINE_GRAD_NAMES}
    out = gine_dense(leaves["x"], leaves["ea"], c["eis"][kind], leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], leaves["eps"],
                     leaves["ins"], c["batch"])
    (out * c["w"].to(dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in leaves.items()}


def gcn_grad_reference(c, kind, bias, dtype=torch.float64):
    names = GCN_GRAD_NAMES if bias else GCN_GRAD_NAMES[:-1]
    leaves = {k: c[k].detach().clone().to(dtype).requires_grad_(True) for k in names}
    out = gcn_dense(leaves["x"], leaves["weight"], leaves.get("bias"), c["eis"][kind], leaves["ins"], c["batch"])
    (out * c["w"].to(dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in leaves.items()}


def grad_errors(got, ref):
    """{name: relative error} of each gradient, the floor 1e-3 x the largest entry of any of them (the measure of
    test_gine_gcn_tapped_convs_gradients_vs_oracle)."""
    floor = 1e-3 * max(float(r.abs().max()) for r in ref.values())
    return {k: maxabs(got[k], r) / max(float(r.abs().max()), floor, 1e-300) for k, r in ref.items()}


# ---- the BN -> ReLU chain (eval statistics) --------------------------------------------------------------------------------------------
# (N, C, x at a 4-byte offset): v4; scalar (C % 4 != 0); scalar past its 2048-block cap at C > 512; v4 past its cap of 8 blocks per CU;
# v4's width on a misaligned x, which takes the scalar form
CHAIN_SHAPES = [(322, 300, False), (322, 30, False), (1101, 516, False), (4300, 512, False), (322, 24, True)]
CHAIN_STAGES = (0, 1, 4, 8)


def bn_chain(x, stages, eps=BN_EPS):
    """relu(bn_{S-1}(... relu(bn_0(x)) ...)) from the definition, (h - mean) / sqrt(var + eps) * w + b, in x's dtype."""
    h = x
    for w, b, m, v in stages:
        h = torch.relu((h - m.to(h.dtype)) / torch.sqrt(v.to(h.dtype) + eps) * w.to(h.dtype) + b.to(h.dtype))
    return h


def bn_chain_fp32(x, stages, eps=BN_EPS):
    """The same chain as torch runs it in fp32 on the CPU: eval-mode F.batch_norm, then relu, per stage."""
    h = x.float()
    for w, b, m, v in stages:
        h = torch.relu(F.batch_norm(h, m, v, w, b, False, 0.0, eps))
    return h


@functools.lru_cache(maxsize=None)
def chain_case(N, C, S):
    """x [N, C] whose column means run from -100 to +100 x the column's std (std 1), and S stages whose running statistics are those of
    their actual input in fp64 (so every stage works where its input lives, the large means of stage 0 included) times a per-column
    jitter (the variance plus 0.25: a column that a stage has all but killed is not blown up 30 x by the next); on three disjoint column sets one stage each has running_var = 0 (its weight 0.01: the scale is w / sqrt(eps)), negative
    weights and zero weights.  -> (x, [(weight, bias, mean, var)] as fp32 CPU tensors)."""
    ratio = np.linspace(-100.0, 100.0, C)
    x = t((ratio[None, :] + synth.normal((N, C), 61).astype(np.float64)).astype(np.float32))
    col = np.arange(C)
    stages, h = [], x.double()
    for s in range(S):
        w = 0.5 + synth.uniform((C,), 62 + s).astype(np.float64)
        b = 0.3 * synth.normal((C,), 72 + s).astype(np.float64)
        m = h.mean(0).numpy() + 0.1 * h.std(0, unbiased=False).numpy() * synth.normal((C,), 82 + s)
        v = h.var(0, unbiased=False).numpy() * (0.5 + synth.uniform((C,), 92 + s)) + 0.25
        if s == min(1, S - 1):
            v[col % 7 == 1] = 0.0
            w[col % 7 == 1] = 0.01
        if s == min(2, S - 1):
            w[col % 7 == 2] *= -1.0
        if s == min(3, S - 1):
            w[col % 7 == 3] = 0.0
        st = tuple(t(a.astype(np.float32)) for a in (w, b, m, v))
        stages.append(st)
        h = bn_chain(h, [st])
    return x, stages


# ---- train-mode BatchNorm + ReLU (batch statistics) with gradients --------------------------------------------------------------------
# (N, C): TPR = 1 and a last row block of one row; the second column trip of the _v4 kernels (TPR = 256) and a last row block of one
# row; the scalar kernels (C % 4 != 0); the smallest batch; TPR = 128 with idle column threads
BN_TRAIN_SHAPES = [(65, 4), (129, 1028), (64, 6), (2, 8), (257, 300)]
BN_CONSTANT_COLUMN, BN_CONSTANT_VALUE = 1, 1000.5
BN_OUTLIER_COLUMN, BN_OUTLIER_VALUE = 3, 1e4      # row 0 of this column, the rest at mean 10, std 1: the statistics kernels' first probe row
BN_GATE_MARGIN = 0.05


def bn_column_kinds(C):
    """0: mean up to 1e4 with std 1; 1: std 1e-2 around mean 10; 2: ordinary (mean 0.5, std 2); 3: the constant column; 4: the column
    whose first row lies 1e4 stds from the rest."""
    kind = np.arange(C) % 3
    kind[BN_CONSTANT_COLUMN] = 3
    kind[BN_OUTLIER_COLUMN] = 4
    return kind


@functools.lru_cache(maxsize=None)
def bn_train_case(N, C):
    """x [N, C] by column kind, weight of either sign with 0.5 <= |w| <= 1.5, 0.1 <= |bias| <= 0.4 (the constant column's output is
    its bias: well away from the ReLU's edge; the outlier column has w = -1, b = 0.4: its outlier is gated off, the rest at about
    0.4 + 1 / sqrt(N) is not), dy, a keep mask at p = 0.25.  No element's pre-activation lies within BN_GATE_MARGIN
    of 0 in fp64: elements that did were moved by a fifth of their column's std, so that no correct fp32 result gates differently."""
    kind = bn_column_kinds(C)
    mean = np.select([kind == 0, kind == 1, kind == 2, kind == 4], [1e4 * (1.0 - 0.9 * synth.uniform((C,), 101)), 10.0, 0.5, 10.0],
                     BN_CONSTANT_VALUE)
    std = np.select([kind == 0, kind == 1, kind == 2, kind == 4], [1.0, 1e-2, 2.0, 1.0], 0.0)
    sign = np.where(synth.uniform((C,), 102) < 0.3, -1.0, 1.0)
    w = (sign * (0.5 + synth.uniform((C,), 103))).astype(np.float32)
    b = (np.where(synth.uniform((C,), 104) < 0.5, -1.0, 1.0) * (0.1 + 0.3 * synth.uniform((C,), 105))).astype(np.float32)
    w[BN_OUTLIER_COLUMN], b[BN_OUTLIER_COLUMN] = -1.0, 0.4
    x = (mean[None, :] + std[None, :] * synth.normal((N, C), 106).astype(np.float64)).astype(np.float32)
    x[0, BN_OUTLIER_COLUMN] = BN_OUTLIER_VALUE
    for _ in range(50):
        xd = x.astype(np.float64)
        pre = (xd - xd.mean(0)) / np.sqrt(xd.var(0) + BN_EPS) * w + b
        close = np.abs(pre) < BN_GATE_MARGIN
        if not close.any():
            break
        x = (xd + close * (0.2 * std[None, :]) * np.sign(w)[None, :]).astype(np.float32)
    else:
        raise AssertionError("bn_train_case: pre-activations stay at the ReLU's edge")
    assert float(np.ptp(x[:, BN_CONSTANT_COLUMN])) == 0.0 and x[0, BN_OUTLIER_COLUMN] == BN_OUTLIER_VALUE
    assert float(np.abs(x[1:, BN_OUTLIER_COLUMN] - 10.0).max()) < 6.0
    keep = (synth.uniform((N, C), 107) > 0.25).astype(np.uint8)
    return dict(x=t(x), w=t(w), b=t(b), dy=t(synth.normal((N, C), 108)), keep=t(keep), kind=kind, N=N, C=C)


# (mean, var: the batch statistics themselves, where the caller gets them -- _BatchNormReluTrain returns them)
BN_TRAIN_NAMES = ("y", "dx", "dweight", "dbias", "running_mean", "running_var", "mean", "var")


def bn_train_fp64(c, masked):
    """fp64 torch.nn.BatchNorm1d in training mode, relu, the keep mask at 1 / 0.75, backward with dy: {name: tensor} and
    num_batches_tracked."""
    bn = torch.nn.BatchNorm1d(c["C"], eps=BN_EPS).double()
    with torch.no_grad():
        bn.weight.copy_(c["w"]); bn.bias.copy_(c["b"])
    x = c["x"].double().requires_grad_(True)
    y = torch.relu(bn.train()(x))
    if masked:
        y = y * c["keep"].double() / 0.75
    y.backward(c["dy"].double())
    xd = c["x"].double()
    return dict(y=y.detach(), dx=x.grad, dweight=bn.weight.grad, dbias=bn.bias.grad, running_mean=bn.running_mean.clone(),
                running_var=bn.running_var.clone(), mean=xd.mean(0), var=xd.var(0, unbiased=False)), int(bn.num_batches_tracked)


def bn_train_fp32(c, masked):
    """The same in plain fp32 torch on the CPU: a two-pass mean, then the variance of the centred values; gradients by autograd."""
    x, w, b = (c[k].clone().requires_grad_(True) for k in ("x", "w", "b"))
    N = c["N"]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    y = torch.relu((x - mean) / torch.sqrt(var + BN_EPS) * w + b)
    if masked:
        y = y * c["keep"].float() / 0.75
    y.backward(c["dy"])
    with torch.no_grad():
        rm = 0.9 * torch.zeros_like(mean) + 0.1 * mean
        rv = 0.9 * torch.ones_like(var) + 0.1 * (var * (N / (N - 1)))
    return dict(y=y.detach(), dx=x.grad, dweight=w.grad, dbias=b.grad, running_mean=rm, running_var=rv, mean=mean.detach(), var=var.detach())


def bn_stats_in_kernel_order(x, pivot=True):
    """(mean, var) of x [N, C] with the roundings and the summation order of k_bn_col_stats_fused, k_bn_col_finish and k_bn_col_finish_m2,
    in numpy fp32 (without the kernels' fused multiply-adds): row blocks of 64, four interleaved accumulators per block, the block's
    M2 about its own rounded mean, the blocks combined over 64 interleaved thread rows and then in index order.  pivot: every value is
    taken relative to the median of the column's first, middle and last row, as the kernels do; False: the raw values (pivot 0), which is
    the arithmetic these kernels had before they shifted."""
    f = np.float32
    x = x.numpy()
    N, C = x.shape
    p = np.median(x[[0, N // 2, N - 1]], axis=0).astype(f) if pivot else np.zeros(C, f)
    nb = -(-N // 64)
    S, M2, n = np.zeros((nb, C), f), np.zeros((nb, C), f), [min(64, N - 64 * b) for b in range(nb)]
    for b in range(nb):
        v = np.zeros((64, C), f)
        v[:n[b]] = x[64 * b:64 * b + n[b]] - p
        a = [np.zeros(C, f) for _ in range(4)]
        for r in range(64):
            a[r % 4] = a[r % 4] + v[r]
        S[b] = (a[0] + a[1]) + (a[2] + a[3])
        mb = S[b] / f(n[b])
        a = [np.zeros(C, f) for _ in range(4)]
        for r in range(n[b]):
            d = v[r] - mb
            a[r % 4] = a[r % 4] + d * d
        M2[b] = (a[0] + a[1]) + (a[2] + a[3])

    def in_index_order(red):
        total = np.zeros(C, f)
        for k in range(64):
            total = total + red[k]
        return total

    red = np.zeros((64, C), f)
    for ry in range(64):
        a0, a1, b = np.zeros(C, f), np.zeros(C, f), ry
        while b + 64 < nb:
            a0, a1, b = a0 + S[b], a1 + S[b + 64], b + 128
        red[ry] = (a0 + S[b] if b < nb else a0) + a1
    mean = in_index_order(red) * (f(1.0) / f(N)) + p
    m = mean - p
    red = np.zeros((64, C), f)
    for ry in range(64):
        for b in range(ry, nb, 64):
            d = S[b] / f(n[b]) - m
            red[ry] = red[ry] + (M2[b] + f(n[b]) * d * d)
    var = in_index_order(red) / f(N)
    assert mean.dtype == f and var.dtype == f
    return torch.from_numpy(mean), torch.from_numpy(var)


BN_STRATA = ("ordinary", "large_mean", "small_std", "constant", "outlier_pivot")


def bn_strata(kind):
    """Column index sets by kind, each judged on its own (a shape without columns of a kind has no such entry): the ordinary columns
    are held to the plain bounds, every other kind to 8 x ITS fp32 form's distance, never below the plain bounds."""
    sets = dict(ordinary=kind == 2, large_mean=kind == 0, small_std=kind == 1, constant=kind == 3, outlier_pivot=kind == 4)
    return {k: np.flatnonzero(v) for k, v in sets.items() if v.any()}


def bn_distances(got, ref, cols):
    cols = torch.as_tensor(cols)
    return {k: maxabs(got[k].detach().cpu()[..., cols], ref[k][..., cols]) for k in BN_TRAIN_NAMES if k in got}


def bn_plain_bounds(ref, cols):
    """1e-5 x max(1, |ref|max) for y and the gradients, 1e-6 / 1e-5 for the running mean / variance, on the given columns."""
    cols = torch.as_tensor(cols)
    bounds = {k: 1e-5 * max(1.0, float(ref[k][..., cols].abs().max())) for k in ("y", "dx", "dweight", "dbias", "mean", "var")}
    bounds.update(running_mean=1e-6, running_var=1e-5)
    return bounds
