"""MI355X-native global attention pooling: `torch_geometric.utils.softmax(gate, batch)` followed by `scatter_add(gate * x, batch)`
(pipeline_model_gat.py:172-179 and :279-286, call site K13 of SURVEY 2.1).

`graph_attention_pool` is the differentiable op: the forward and the backward are one C call each (csrc/softmax_pool.hip), and the backward
keeps `x` and the `[N]` gate only.  `GlobalAttention` keeps PyG's class name, constructor, state_dict keys and `forward(x, batch, size=None)`;
its MLPs stay the caller's torch modules.  With `return_gate=True` it is the reference's `GlobalModel` (:279-286), which hands the gate back
as well.  The derivative takes the per-graph max as a constant, which differs from PyG's autograd by less than fp32 resolution (include/gvqa.h).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib
from .gat_skip import _f32c, _workspace
from .graph import SceneGraphBatch, _stream
from .graph_layernorm import _rows

FORM_AUTO, FORM_WORKGROUP, FORM_SPLIT = 0, 1, 2


def graph_attention_pool_form(graph: SceneGraphBatch, C_: int) -> int:
    """The kernel form the library's auto rule takes for this batch and width: 1 = one workgroup per graph, 2 = split."""
    rc = _lib.load().gvqa_graph_softmax_pool_form(C.byref(graph.c), int(C_))
    _lib.check(min(rc, 0))
    return rc


class _GraphAttentionPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, x, graph, form):
        lib = _lib.load()
        x = _rows(x, "x")
        score = _f32c(score, "score")
        N, Cw = x.shape
        B = graph.num_graphs
        dev = x.device
        # (a batch without nodes enqueues nothing and must still hand back zero rows)
        out = torch.empty((B, Cw), dtype=torch.float32, device=dev) if N > 0 else torch.zeros((B, Cw), dtype=torch.float32, device=dev)
        gate = torch.empty((N, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = _workspace(lib.gvqa_graph_softmax_pool_workspace_bytes(C.byref(graph.c), Cw), dev)
            _lib.check(lib.gvqa_graph_softmax_pool_forward(C.byref(graph.c), Cw, score.data_ptr(), 1, x.data_ptr(), x.stride(0) if N > 1 else Cw,
                                                           gate.data_ptr(), out.data_ptr(), Cw, form, ws.data_ptr(), ws.numel(), _stream(dev)))
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(x, gate)
            ctx.graph, ctx.form, ctx.score_shape = graph, form, score.shape
            ctx.set_materialize_grads(False)      # (an unused gate hands the backward dgate = None, not a tensor of zeros)
        return out, gate

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, dgate):
        lib = _lib.load()
        x, gate = ctx.saved_tensors
        graph = ctx.graph
        N, Cw = x.shape
        dev = x.device
        if dout is None:                           # only the gate was used downstream
            dout = torch.zeros((graph.num_graphs, Cw), dtype=torch.float32, device=dev)
        dout = _rows(dout, "dout")
        dgate = None if dgate is None else _f32c(dgate, "dgate")
        dscore = torch.empty(ctx.score_shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dx = torch.empty((N, Cw), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            ws = _workspace(lib.gvqa_graph_softmax_pool_workspace_bytes(C.byref(graph.c), Cw), dev)
            _lib.check(lib.gvqa_graph_softmax_pool_backward(C.byref(graph.c), Cw, x.data_ptr(), x.stride(0) if N > 1 else Cw, gate.data_ptr(),
                                                            dout.data_ptr(), dout.stride(0) if dout.shape[0] > 1 else Cw,
                                                            None if dgate is None else dgate.data_ptr(),
                                                            None if dscore is None else dscore.data_ptr(), None if dx is None else dx.data_ptr(),
                                                            Cw, ctx.form, ws.data_ptr(), ws.numel(), _stream(dev)))
        return dscore, dx, None, None


def graph_attention_pool(score: Tensor, x: Tensor, graph: SceneGraphBatch, return_gate: bool = False, _form: int | None = None):
    """out[b] = sum over the nodes i of graph b of gate_i x[i], gate = the softmax of `score` over the nodes of each graph (PyG semantics:
    max-shifted, denominator + 1e-16; a zero row for an empty graph).  score: fp32 [N] or [N, 1], x: fp32 [N, C] on the GPU.  Returns out
    [B, C], or (out, gate [N, 1]) with return_gate=True.  Differentiable in score and x (first order); a gradient arriving at the gate goes
    into the same backward call.  `_form` forces a kernel form (tests): 1 = one workgroup per graph, 2 = split; None = the auto rule."""
    if x.dim() != 2 or x.shape[0] != graph.num_nodes:
        raise ValueError("graph_attention_pool: x must be [N, C] with N = graph.num_nodes")
    if x.shape[1] < 1:
        raise ValueError("graph_attention_pool: x needs at least one channel")
    if not (score.dim() == 1 or (score.dim() == 2 and score.shape[1] == 1)) or score.shape[0] != x.shape[0]:
        raise ValueError("graph_attention_pool: score must be [N] or [N, 1]")
    out, gate = _GraphAttentionPoolFn.apply(score, x, graph, FORM_AUTO if _form is None else int(_form))
    return (out, gate) if return_gate else out


class GlobalAttention(torch.nn.Module):
    """torch_geometric.nn.GlobalAttention: out[b] = sum_i softmax_b(gate_nn(x))_i * nn(x)_i.  `gate_nn` maps [N, F] to [N, 1], `nn` (optional)
    [N, F] to [N, C]; both are the caller's torch modules (state_dict keys `gate_nn.*`, `nn.*`)."""

    def __init__(self, gate_nn, nn=None):
        super().__init__()
        _lib.load()
        self.gate_nn = gate_nn
        self.nn = nn
        self.reset_parameters()

    def reset_parameters(self):
        for m in (self.gate_nn, self.nn):
            if m is None:
                continue
            children = list(m.children())
            for item in (children if children else [m]):
                if hasattr(item, "reset_parameters"):
                    item.reset_parameters()

    def forward(self, x: Tensor, batch: Tensor | None, size: int | None = None, graph: SceneGraphBatch | None = None, return_gate: bool = False,
                _form: int | None = None):
        """size: the number of graphs (default batch.max() + 1, one host read; a larger size gives trailing zero rows).  graph: a prebuilt
        SceneGraphBatch of the same batch (no host read).  return_gate=True: (gate [N, 1], out), the order of the reference's GlobalModel."""
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        if not x.is_cuda:
            raise RuntimeError(f"x is on {x.device}: the MI355X execution path has no CPU fallback")
        if graph is None:
            N = x.shape[0]
            B = size if size is not None else (int(batch.max()) + 1 if N > 0 else 0)
            graph = SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=x.device), batch, N, int(B))
        score = self.gate_nn(x).view(-1, 1)
        x = self.nn(x) if self.nn is not None else x
        if score.dim() != x.dim() or score.shape[0] != x.shape[0]:
            raise ValueError("GlobalAttention: gate_nn must map [N, F] to [N, 1]")
        out, gate = graph_attention_pool(score, x, graph, return_gate=True, _form=_form)
        return (gate, out) if return_gate else out

    def __repr__(self):
        return "{}(gate_nn={}, nn={})".format(self.__class__.__name__, self.gate_nn, self.nn)
