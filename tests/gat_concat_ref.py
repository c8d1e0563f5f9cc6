"""Shared pieces of the gat concat tests (no GPU needed to import): the two batches, the operands, the dense reference -- the bare
message passing of tests/test_gpu_backward.py::_mp_reference without its head mean, reshaped to [N, H*C], plus a bias -- in any
precision with autograd through it, and the bounds.  References are computed once per case (lru_cache) and handed out read-only."""
import functools

import numpy as np
import torch

from graphvqa_amd import synth
from tests.lcgn_ref import hard_batch
from tests.util import t, maxabs

SLOPE = 0.2
# the kernel family's own bounds (tests/test_gpu_backward.py::test_message_passing_backward_vs_autograd)
OUT_TOL, ALPHA_TOL, GRAD_TOL = 1e-5, 1e-6, 2e-5
MATRIX = [(4, 1, False), (12, 4, True), (32, 3, True), (30, 2, True), (300, 4, True), (512, 8, False), (516, 2, False), (128, 8, True)]   # (C, H, mask)
HARD = [(40, 4), (128, 8), (8, 1)]                                                                                                    # (C, H), masked
GRADS = ("dxp", "da_node", "da_edge", "dbias")


def rel(a, b):
    """max-abs error relative to the reference gradient's scale (tests/test_gpu_backward.py::_rel)."""
    b = b.detach().cpu().double()
    return maxabs(a, b) / max(float(b.abs().max()), 1e-12)


def dense_concat(xp, a_node, a_edge, mask, bias, edge_index, N, H, C, slope=SLOPE):
    """(out [N, H*C], alpha [E, H]) in the operands' dtype on the CPU, autograd-capable."""
    import torch.nn.functional as F
    from oracle import ref_torch as R
    src, dst = edge_index[0], edge_index[1]
    z = a_node[:, :H].index_select(0, src) + a_node[:, H:].index_select(0, dst) + a_edge
    alpha = R.segment_softmax(F.leaky_relu(z, slope), dst, N)
    am = alpha if mask is None else alpha * mask
    msg = xp.view(N, H, C).index_select(0, src) * am.unsqueeze(-1)
    out = R.scatter_add_rows(msg, dst, N).reshape(N, H * C)
    return (out if bias is None else out + bias), alpha


@functools.lru_cache(maxsize=None)
def generated_batch(C):
    """Six graphs of 5-40 nodes plus 70 edges into node 0 of the first graph (test_message_passing_backward_vs_autograd's batch):
    (edge_index [2, E], batch [N], num_graphs)."""
    gb = synth.make_graph_batch(6, seed=0xB00 + C, nodes_lo=5, nodes_hi=40, rel_per_node=2.0)
    n0 = int((gb.batch == 0).sum())
    extra = np.stack([np.arange(70) % n0, np.zeros(70, np.int64)])
    ei = np.concatenate([gb.edge_index, extra], axis=1)
    ei.setflags(write=False)
    return ei, gb.batch.copy(), gb.num_graphs


def _operands(ei, N, C, H, with_mask, seed):
    E = ei.shape[1]
    rng = np.random.default_rng(seed)
    c = dict(xp=rng.standard_normal((N, H * C)).astype(np.float32), a_node=rng.standard_normal((N, 2 * H)).astype(np.float32),
             a_edge=rng.standard_normal((E, H)).astype(np.float32),
             mask=((rng.random((E, H)) > 0.3) / 0.7).astype(np.float32) if with_mask else None,
             w=rng.standard_normal((N, H * C)).astype(np.float32), bias=rng.standard_normal((H * C,)).astype(np.float32))
    return {k: (None if v is None else t(v)) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def matrix_case(C, H, with_mask):
    ei, batch, B = generated_batch(C)
    N = batch.shape[0]
    return dict(_operands(ei, N, C, H, with_mask, C * 7 + H), ei=t(ei.copy()), batch=t(batch), N=N, B=B, C=C, H=H)


@functools.lru_cache(maxsize=None)
def hard_case(C, H, kind):
    """kind 0: the intra-graph edge list of tests/lcgn_ref.py::hard_batch, 1: the one with edges across graphs."""
    gb, cross, info = hard_batch()
    ei = (gb.edge_index, cross)[kind]
    return dict(_operands(ei, gb.num_nodes, C, H, True, 0x4A7 + C * 7 + H), ei=t(ei.copy()), batch=t(gb.batch.copy()), N=gb.num_nodes,
                B=gb.num_graphs, C=C, H=H, info=info)


def reference(c, dtype=torch.float64):
    """(out, alpha, {dxp, da_node, da_edge, dbias}) of dense_concat in `dtype`, loss (out * w).sum()."""
    rs = [c[k].detach().clone().to(dtype).requires_grad_(True) for k in ("xp", "a_node", "a_edge", "bias")]
    out, alpha = dense_concat(rs[0], rs[1], rs[2], None if c["mask"] is None else c["mask"].to(dtype), rs[3], c["ei"], c["N"], c["H"], c["C"])
    (out * c["w"].to(dtype)).sum().backward()
    return out.detach(), alpha.detach(), dict(zip(GRADS, (r.grad for r in rs)))


@functools.lru_cache(maxsize=None)
def matrix_reference(C, H, with_mask):
    return reference(matrix_case(C, H, with_mask))


@functools.lru_cache(maxsize=None)
def hard_reference(C, H, kind):
    return reference(hard_case(C, H, kind))


def distances(got, ref):
    """{out (relative to max(1, |ref|max)), alpha (absolute), each gradient (rel)} of (out, alpha, grads) from the fp64 triple."""
    d = dict(out=maxabs(got[0], ref[0]) / max(1.0, float(ref[0].abs().max())), alpha=maxabs(got[1], ref[1]))
    d.update({k: rel(got[2][k], ref[2][k]) for k in GRADS if k in got[2]})
    return d


def within_bounds(d, factor=1.0):
    return d["out"] < OUT_TOL * factor and d["alpha"] < ALPHA_TOL * factor and all(d[k] < GRAD_TOL * factor for k in GRADS if k in d)
