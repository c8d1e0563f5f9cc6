"""Shared pieces of the LCGN attention tests (no GPU needed to import): the dense restatement of include/gvqa.h's formulas that
serves as the reference in any precision, the dropout mask, the gradient error measure, and the hard batch (hard_batch) with the
operands, hub ordering and logit scaling that the matrix tests (tests/test_gpu_lcgn_attention_matrix*.py) and their CPU companion
(tests/test_lcgn_hard_batch.py) run on."""
import functools

import numpy as np
import torch

from graphvqa_amd import synth
from tests.util import t, maxabs

GRAD_TOL, SLOPE = 5e-4, 0.2
HUB_DEGREE = 301
BIG_LOGIT = 500.0
NAMES = ("dJ", "dpc", "dbias")

# (H, C) of the matrix; chunks per lane (KC) of the fp32 / bf16 kernels, re-derived by launch_plan below and pinned by
# tests/test_lcgn_hard_batch.py::test_shape_matrix_reaches_every_chunk_count
SHAPES = [(1, 8), (4, 256), (1, 1024), (2, 768), (5, 40), (7, 72), (6, 176), (8, 512), (2, 2048), (1, 4096), (3, 336)]
SHAPES_FP32_ODD = [(3, 20), (5, 44), (7, 76), (2, 1028), (1, 2052)]          # C % 8 != 0 at KC = 1, 2, 4, 8, 16 (fp32 only)
SHAPES_BIG = [(4, 256), (5, 40), (2, 2048), (1, 4096)]                       # the large-logit stratum


def launch_plan(H, Cc, per):
    """(one_wave, lanes per head, need, KC) as launch_lcgn_attention (per = 4 channels per lane and load) and
    launch_lcgn_attention_bf16 (per = 8) and the two backward entry points derive them."""
    one_wave = H * Cc <= 1024
    hpw = H if one_wave else 1
    lph = 64
    while lph * hpw > 64:
        lph >>= 1
    need = -(-(Cc // per) // lph)
    kc = next(k for k in (1, 2, 4, 8, 16) if need <= k)
    return one_wave, lph, need, kc


def with_concat(shapes):
    return [(H, Cc, concat) for H, Cc in shapes for concat in ((False, True) if H > 1 else (False,))]


def _dense_ref(J, pc, ei, batch, H, Cc, concat, bias, mask, slope=SLOPE):
    """The forward of include/gvqa.h's gvqa_lcgn_attention_train as plain torch ops in the operands' dtype; autograd through it is
    the reference for dJ, dpc and dbias."""
    N, HC = J.shape[0], H * Cc
    src, dst = ei[0], ei[1]
    x_l, x_r, x_val = (J[:, k * HC:(k + 1) * HC].view(N, H, Cc) for k in range(3))
    rows = pc[batch]
    y = rows[:, :HC].view(N, H, Cc) * x_r
    z = (x_l[src] * y[dst]).sum(-1)                                              # [E, H]
    l = torch.nn.functional.leaky_relu(z, slope)
    mx = torch.full((N, H), -float("inf"), dtype=J.dtype).scatter_reduce(0, dst[:, None].expand(-1, H), l.detach(), "amax")
    p = torch.exp(l - mx[dst])
    alpha = p / (torch.zeros((N, H), dtype=J.dtype).index_add(0, dst, p)[dst] + 1e-16)
    v = x_val * rows[:, HC:].view(N, H, Cc)                                      # cal_cmd of the SOURCE's graph
    w = alpha if mask is None else alpha * mask
    o = torch.zeros((N, H, Cc), dtype=J.dtype).index_add(0, dst, w[:, :, None] * v[src])
    out = o.reshape(N, HC) if concat else o.mean(dim=1)
    return (out if bias is None else out + bias), alpha


def _mask(E, H, seed, p=0.3):
    gen = torch.Generator().manual_seed(seed)
    return torch.bernoulli(torch.full((E, H), 1.0 - p), generator=gen) / (1.0 - p)


def _grad_errors(got, ref):
    """{name: relative error} of each gradient, the floor 1e-3 x the largest entry of any of them."""
    floor = 1e-3 * max(float(r.abs().max()) for r in ref.values())
    return {k: maxabs(got[k], r) / max(float(r.abs().max()), floor, 1e-300) for k, r in ref.items()}


# ---- the hard batch ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hard_batch():
    """One batch of five graphs, 320 nodes, built by hand so that it has what the generated fixtures lack; every property below is
    asserted here, with np.bincount, so an edit cannot lose one silently.  -> (GraphBatch with intra-graph edges, the same edge
    list with some sources moved into other graphs, info: the node and graph ids the tests look at).
      graph 0  10 nodes, node k with exactly k in-edges (k = 0 .. 9; no self-loops, so node 0 receives nothing)
      graph 1  one node with a self-loop
      graph 2  empty, inside the batch (its dpc row is exactly zero)
      graph 3  301 nodes: its first node receives 301 edges (300 sources, one of them twice), its second node sends 301 (300
               destinations, one of them twice); the edges in a fixed shuffled order, so a hub's edges are not contiguous in COO
      graph 4  8 nodes with self-loops and random edges, one of them repeated"""
    sizes = np.array([10, 1, 0, HUB_DEGREE, 8], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, B = int(off[-1]), len(sizes)
    batch = np.repeat(np.arange(B, dtype=np.int64), sizes)
    src, dst = [], []
    for k in range(10):
        src += [int(off[0]) + (k + 1 + j) % 10 for j in range(k)]
        dst += [int(off[0]) + k] * k
    src.append(int(off[1])); dst.append(int(off[1]))
    hub_in, hub_out = int(off[3]), int(off[3]) + 1
    s3 = list(range(hub_in + 1, hub_in + HUB_DEGREE)) + [hub_in + 5]             # 300 sources -> hub_in, one twice
    d3 = [hub_in] * HUB_DEGREE
    d3 += list(range(hub_in + 2, hub_in + HUB_DEGREE)) + [hub_in + 7]             # hub_out -> the 299 others (+ hub_in above), one twice
    s3 += [hub_out] * (HUB_DEGREE - 1)
    order = np.random.default_rng(0x301).permutation(len(s3))
    src += [s3[k] for k in order]; dst += [d3[k] for k in order]
    n4 = int(sizes[4])
    loops = list(range(int(off[4]), int(off[4]) + n4))
    rs = (off[4] + synth.randint(12, 0x4A, 0, n4, stream=5)).tolist()
    rd = (off[4] + synth.randint(12, 0x4A, 0, n4, stream=6)).tolist()
    src += loops + rs + [rs[0]]; dst += loops + rd + [rd[0]]
    ei = np.array([src, dst], dtype=np.int64)
    E = ei.shape[1]
    # the second list: every 7th edge takes its source 5 nodes further on (the existing tests' `cross`), the two hubs' edges
    # excepted so that the sender keeps its 301 and the receiver its 300 distinct logits (the batch-wide cross-graph kernel form
    # still serves both); destinations, and with them every in-degree, are those of the first list
    cross = ei.copy()
    idx = np.arange(0, E, 7)
    idx = idx[(cross[0, idx] != hub_out) & ((cross[0, idx] + 5) % N != hub_out) & (cross[1, idx] != hub_in)]
    cross[0, idx] = (cross[0, idx] + 5) % N
    info = dict(isolated=int(off[0]), hub_in=hub_in, hub_out=hub_out, empty_graph=2, single_graph=1)
    for name, e in (("intra", ei), ("cross", cross)):
        indeg, outdeg = np.bincount(e[1], minlength=N), np.bincount(e[0], minlength=N)
        assert set(range(10)) <= set(indeg[off[0]:off[1]].tolist()), name
        assert indeg[info["isolated"]] == 0 and not bool(((e[0] == e[1]) & (e[1] == info["isolated"])).any()), name
        assert indeg[hub_in] == HUB_DEGREE and int((indeg >= HUB_DEGREE).sum()) == 1, name
        assert outdeg[hub_out] == HUB_DEGREE and int((outdeg >= HUB_DEGREE).sum()) == 1, name
        pairs = np.bincount(e[0] * N + e[1], minlength=N * N)
        assert int(pairs.max()) >= 2, name                                                    # a repeated (src, dst)
        assert pairs[(hub_in + 5) * N + hub_in] == 2, name                                    # ... among the hub's own in-edges
        run = np.flatnonzero(e[1] == hub_in)
        assert int(run[-1] - run[0]) + 1 > HUB_DEGREE, name                                   # the hub's in-edges are spread out
    per_graph = np.bincount(batch, minlength=B)
    assert per_graph.tolist() == sizes.tolist() and per_graph[info["single_graph"]] == 1
    assert per_graph[info["empty_graph"]] == 0 and 0 < info["empty_graph"] < B - 1
    assert bool((batch[ei[0]] == batch[ei[1]]).all()) and bool((batch[cross[0]] != batch[cross[1]]).any())
    assert 200 <= N <= 400
    ei.setflags(write=False); cross.setflags(write=False); batch.setflags(write=False)
    return synth.GraphBatch(edge_index=ei, batch=batch, num_graphs=B), cross, info


def logits64(J, pc, ei, batch, H, Cc):
    """z [E, H] = x_l[src] . (proj_cmd[g(dst)] * x_r[dst]) in fp64 (numpy), before the leaky-relu."""
    N, HC = J.shape[0], H * Cc
    J, pc = np.asarray(J, dtype=np.float64), np.asarray(pc, dtype=np.float64)
    y = (pc[batch][:, :HC] * J[:, HC:2 * HC]).reshape(N, H, Cc)
    return np.einsum("ehc,ehc->eh", J[:, :HC].reshape(N, H, Cc)[ei[0]], y[ei[1]])


def order_hub(ei, z, hub):
    """The edge list with the hub's in-edges permuted among their COO positions so that head 0's logit ascends along them (CSR
    order within a row is COO order: the kernel's running maximum then moves at every step); every other edge stays put."""
    idx = np.flatnonzero(ei[1] == hub)
    out = ei.copy()
    out[:, idx] = ei[:, idx[np.argsort(z[idx, 0], kind="stable")]]
    return out


def _bf16_values(a):
    return t(a).bfloat16().float().numpy()


@functools.lru_cache(maxsize=2)
def hard_operands(H, Cc, bf16):
    """Operands of the existing kernel tests' scale (normal x 0.3, logits about +-1) on hard_batch; bf16: J holds bf16 values.  The
    hub ordering of each edge list is fixed here, from these logits.  -> (J [N, 3HC], pc [B, 2HC], bias [HC], (intra, cross))."""
    gb, cross, info = hard_batch()
    N, B, HC = gb.num_nodes, gb.num_graphs, H * Cc
    J, pc = synth.normal((N, 3 * HC), 11) * np.float32(0.3), synth.normal((B, 2 * HC), 12) * np.float32(0.3)
    bias = synth.normal((HC,), 13)
    if bf16:
        J = _bf16_values(J)
    eis = []
    for ei in (gb.edge_index, cross):
        e = order_hub(ei, logits64(J, pc, ei, gb.batch, H, Cc), info["hub_in"])
        z0 = logits64(J, pc, e, gb.batch, H, Cc)[e[1] == info["hub_in"], 0]
        assert z0.shape == (HUB_DEGREE,) and bool((np.diff(z0) >= 0).all()) and int((np.diff(z0) > 0).sum()) >= HUB_DEGREE - 2
        eis.append(e)
    return J, pc, bias, tuple(eis)


def big_logit_J(J, pc, ei, batch, H, Cc, bf16):
    """J with its x_l block rescaled so that max |z| over the batch is BIG_LOGIT (the factor in fp64), rounded to fp32, or to bf16
    values, before anyone sees it: leaky logits from -100 to +500, where an unshifted expf overflows on one side and flushes whole
    rows to zero on the other."""
    HC = H * Cc
    f = BIG_LOGIT / np.abs(logits64(J, pc, ei, batch, H, Cc)).max()
    big = np.asarray(J, dtype=np.float64).copy()
    big[:, :HC] *= f
    big = big.astype(np.float32)
    return _bf16_values(big) if bf16 else big


def hard_case(H, Cc, concat, bf16, kind, big, masked):
    """One case of the matrix as CPU tensors: dict(J, pc, bias, ei, batch, mask, w, N, B, info).  kind: 0 the intra-graph edge
    list, 1 the one with edges across graphs; big: the large-logit stratum; the mask is drawn after the edge order is fixed."""
    gb, _, info = hard_batch()
    J, pc, bias, eis = hard_operands(H, Cc, bf16)
    ei = eis[kind]
    if big:
        J = big_logit_J(J, pc, ei, gb.batch, H, Cc, bf16)
    HC = H * Cc
    cout = HC if concat else Cc
    return dict(J=t(J), pc=t(pc), bias=t(bias[:cout]), ei=t(ei), batch=t(gb.batch.copy()), N=gb.num_nodes, B=gb.num_graphs, info=info,
                mask=_mask(ei.shape[1], H, 77) if masked else None, w=t(synth.normal((gb.num_nodes, cout), 9)))


def dense_reference(c, H, Cc, concat, dtype=torch.float64, grads=True):
    """(out, alpha, {dJ, dpc, dbias}) of _dense_ref in `dtype` on the CPU on hard_case's operands, loss (out * w).sum()."""
    rs = [c[k].detach().clone().to(dtype).requires_grad_(grads) for k in ("J", "pc", "bias")]
    out, alpha = _dense_ref(rs[0], rs[1], c["ei"], c["batch"], H, Cc, concat, rs[2], None if c["mask"] is None else c["mask"].to(dtype))
    if not grads:
        return out.detach(), alpha.detach(), None
    (out * c["w"].to(dtype)).sum().backward()
    return out.detach(), alpha.detach(), dict(zip(NAMES, (r.grad for r in rs)))


def distances(got, ref):
    """{out, alpha, dJ, dpc, dbias} of (out, alpha, grads) from the fp64 (out, alpha, grads): absolute for out and alpha, _grad_errors'
    relative measure for the gradients."""
    d = dict(out=maxabs(got[0], ref[0]), alpha=maxabs(got[1], ref[1]))
    if got[2] is not None:
        d.update(_grad_errors(got[2], ref[2]))
    return d


# ---- column blocks of wider buffers (the leading-dimension tests) ---------------------------------------------------------------------
def column_block(rows, width, left, right, fill, device, dtype=torch.float32, guard_rows=1):
    """An [rows, width] column block inside a [rows + 2 guard_rows, left + width + right] buffer filled with `fill`:
    (buffer, view, leading dimension)."""
    buf = torch.full((rows + 2 * guard_rows, left + width + right), fill, dtype=dtype, device=device)
    return buf, buf[guard_rows:guard_rows + rows, left:left + width], left + width + right


def untouched(buf, view, fill):
    """Every element of buf outside its column block `view` still holds `fill` (NaN included)."""
    r0, c0 = divmod((view.data_ptr() - buf.data_ptr()) // buf.element_size(), buf.shape[1])
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    rest = buf[outside]
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())
