"""MI355X-native counterpart of the reference's graph LayerNorm (graph_utils/my_graph_layernorm.py): one normalisation per graph over
its nodes x channels, 1-element `weight` / `bias`, eps outside the square root.

`LayerNorm` keeps the reference's class name, constructor, state_dict keys and `forward(x, batch=None)`; `graph_layernorm` is the
differentiable op underneath it: the forward and the backward are one C call each (csrc/graph_layernorm.hip), and the backward keeps
`x` and the per-graph `[B, 2]` (mean, sigma) rows only.  A graph with sigma == 0 gets `dx = (w dout - mean(w dout)) / eps` where the
reference's autograd yields NaN (the variance term is dropped; include/gvqa.h).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable
from torch.nn import Parameter

from . import _lib
from .gat_skip import _f32c, _workspace
from .graph import SceneGraphBatch, _stream

FORM_AUTO, FORM_WORKGROUP, FORM_SPLIT = 0, 1, 2


def _rows(t: Tensor, name: str) -> Tensor:
    """fp32 GPU rows with unit inner stride keep their row stride (a column block of a wider tensor); anything else is made contiguous."""
    if t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return _f32c(t, name)


def graph_layernorm_form(graph: SceneGraphBatch, D: int) -> int:
    """The kernel form the library's auto rule takes for this batch and width: 1 = one workgroup per graph, 2 = split."""
    rc = _lib.load().gvqa_graph_layernorm_form(C.byref(graph.c), int(D))
    _lib.check(min(rc, 0))
    return rc


class _GraphLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, graph, eps, form):
        lib = _lib.load()
        x = _rows(x, "x")
        w = None if weight is None else _f32c(weight, "weight")
        b = None if bias is None else _f32c(bias, "bias")
        N, D = x.shape
        need = any(ctx.needs_input_grad[:3])
        out = torch.empty((N, D), dtype=torch.float32, device=x.device)
        # (zeros: a batch without nodes enqueues nothing and must still hand the backward defined rows)
        stats = torch.zeros((graph.num_graphs, 2), dtype=torch.float32, device=x.device) if need else None
        with torch.cuda.device(x.device):
            ws = _workspace(lib.gvqa_graph_layernorm_workspace_bytes(C.byref(graph.c), D), x.device)
            _lib.check(lib.gvqa_graph_layernorm_forward(C.byref(graph.c), D, x.data_ptr(), x.stride(0) if N > 1 else D,
                                                        None if w is None else w.data_ptr(), None if b is None else b.data_ptr(), eps,
                                                        out.data_ptr(), D, None if stats is None else stats.data_ptr(), form,
                                                        ws.data_ptr(), ws.numel(), _stream(x.device)))
        if need:
            ctx.save_for_backward(x, w, stats)
            ctx.graph, ctx.eps, ctx.form = graph, eps, form
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        x, w, stats = ctx.saved_tensors
        graph = ctx.graph
        N, D = x.shape
        dout = _rows(dout, "dout")
        dev = x.device
        dx = torch.empty((N, D), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.zeros(1, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        db = torch.zeros(1, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(dev):
            ws = _workspace(lib.gvqa_graph_layernorm_workspace_bytes(C.byref(graph.c), D), dev)
            _lib.check(lib.gvqa_graph_layernorm_backward(C.byref(graph.c), D, x.data_ptr(), x.stride(0) if N > 1 else D, dout.data_ptr(),
                                                         dout.stride(0) if N > 1 else D, None if w is None else w.data_ptr(), ctx.eps,
                                                         stats.data_ptr(), None if dx is None else dx.data_ptr(), D,
                                                         None if dw is None else dw.data_ptr(), None if db is None else db.data_ptr(),
                                                         ctx.form, ws.data_ptr(), ws.numel(), _stream(dev)))
        return dx, dw, db, None, None, None


def graph_layernorm(x: Tensor, graph: SceneGraphBatch, weight: Tensor | None = None, bias: Tensor | None = None, eps: float = 1e-5,
                    _form: int | None = None) -> Tensor:
    """out = (x - mean_g) / (std_g + eps) * weight + bias, mean / std per graph of `graph` over its nodes x channels (biased, of the centred
    values).  x: fp32 [N, D] on the GPU; weight / bias: 1-element fp32 tensors or None (1 / 0).  Differentiable in x, weight and bias (first
    order).  `_form` forces a kernel form (tests): 1 = one workgroup per graph, 2 = split; None = the library's auto rule."""
    if x.dim() != 2 or x.shape[0] != graph.num_nodes:
        raise ValueError("graph_layernorm: x must be [N, D] with N = graph.num_nodes")
    if x.shape[1] < 1:
        raise ValueError("graph_layernorm: x needs at least one channel")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and t.numel() != 1:
            raise ValueError(f"graph_layernorm: {name} must have one element")
    return _GraphLayerNormFn.apply(x, weight, bias, graph, float(eps), FORM_AUTO if _form is None else int(_form))


class LayerNorm(torch.nn.Module):
    """graph_utils/my_graph_layernorm.LayerNorm: `weight` / `bias` are 1-element parameters (1 / 0), absent with affine=False."""

    def __init__(self, in_channels, eps=1e-5, affine=True):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps
        if affine:
            self.weight = Parameter(torch.ones(1))
            self.bias = Parameter(torch.zeros(1))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)

    def reset_parameters(self):
        if self.weight is not None:
            torch.nn.init.ones_(self.weight)
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, batch: Tensor | None = None, graph: SceneGraphBatch | None = None, _form: int | None = None) -> Tensor:
        """batch = None: one segment over all of x.  graph: a prebuilt SceneGraphBatch of the same batch (no host read of batch.max())."""
        if x.dim() != 2:
            raise ValueError("LayerNorm: x must be [N, D]")
        if not x.is_cuda:
            raise RuntimeError(f"x is on {x.device}: the MI355X execution path has no CPU fallback")
        if graph is None:
            N = x.shape[0]
            B = 1 if batch is None else (int(batch.max()) + 1 if N > 0 else 0)
            graph = SceneGraphBatch(torch.zeros((2, 0), dtype=torch.int64, device=x.device), batch, N, B)
        return graph_layernorm(x, graph, self.weight, self.bias, self.eps, _form)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels})"
