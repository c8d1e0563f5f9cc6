"""MI355X-native drop-in for the reference's `lcgn` module (baseline_and_test_models/lcgn.py).

`lcgn_seq` keeps the reference's constructor arguments (lcgn.py:255-256), forward signature
(:303) and state_dict keys (incl. the dead `bns.*` entries); the whole forward runs in one C-ABI
call (`gvqa_lcgn_seq_forward`).  `x_ctx` is initialised exactly like the reference:
`torch.randn(x_loc.size())` drawn on the CPU generator, then moved (lcgn.py:306), so the same
`torch.manual_seed` gives the same result.  `gat_heads > 1` runs as a sequence of the library's products around one
`gvqa_lcgn_attention` launch per iteration (eval) or the differentiable `lcgn_attention` (training: HIP forward and backward kernels);
with `node_feature_dtype=torch.bfloat16` the eval sequence is bf16 matrix-core products (`gvqa_linear_bf16`) around one
`gvqa_lcgn_attention_bf16` launch per iteration, every per-node tensor stored as bf16; training in that mode runs the bf16 attention
with gradients (`gvqa_lcgn_attention_bf16_train` / `_backward`), which saves J = [x_l | x_r | x_val] for the backward as bf16.

`gat_lcgn` is the reference's layer (lcgn.py:17-238) on its own: in eval without gradients one C-ABI call
(`gvqa_gat_lcgn_forward`), otherwise the library's differentiable products around the differentiable `lcgn_attention`.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable
from torch.nn import Linear, Parameter

from . import _lib
from .gat_skip import (_f32c, _workspace, _glorot, _ProjectionLinear, gat_message_passing, graph_rows,
                       edge_gather)
from .graph import SceneGraphBatch, _stream, _ptr

_ATT_MAX_HEADS, _ATT_MAX_HC = 8, 4096       # gvqa_lcgn_attention's limits (include/gvqa.h)


def _attention_supported(heads: int, channels: int) -> bool:
    return 1 <= heads <= _ATT_MAX_HEADS and channels > 0 and channels % 4 == 0 and heads * channels <= _ATT_MAX_HC


class _LcgnAttention(torch.autograd.Function):
    """lcgn_attention with gradients: gvqa_lcgn_attention_train forward (saves alpha), gvqa_lcgn_attention_backward (a walk by
    destination, a walk by source over the transposed graph, a per-graph sum: no [E, H C] array, no atomics).  Operands checked and
    made contiguous by the caller."""

    @staticmethod
    def forward(ctx, J, pc, bias, mask, graph, heads, channels, concat, slope):
        lib = _lib.load()
        HC = heads * channels
        cout = HC if concat else channels
        out = torch.empty((graph.num_nodes, cout), dtype=torch.float32, device=J.device)
        alpha = torch.empty((graph.num_edges, heads), dtype=torch.float32, device=J.device)
        with torch.cuda.device(J.device):
            _lib.check(lib.gvqa_lcgn_attention_train(C.byref(graph.c), heads, channels, int(bool(concat)), slope, J.data_ptr(), 3 * HC,
                                                     pc.data_ptr(), 2 * HC, _ptr(bias), _ptr(mask), out.data_ptr(), cout, alpha.data_ptr(),
                                                     _stream(J.device)))
        ctx.save_for_backward(J, pc, alpha, mask)
        ctx.graph, ctx.dims, ctx.has_bias = graph, (heads, channels, bool(concat), slope), bias is not None
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dalpha):
        lib = _lib.load()
        J, pc, alpha, mask = ctx.saved_tensors
        heads, channels, concat, slope = ctx.dims
        graph, HC = ctx.graph, heads * channels
        # a view, a broadcast or an unaligned slice as dout is copied, never refused
        dout = dout.to(torch.float32).contiguous()
        if dout.data_ptr() % 16:
            dout = dout.clone(memory_format=torch.contiguous_format)
        dJ, dpc = torch.empty_like(J), torch.empty_like(pc)
        with torch.cuda.device(J.device):
            gt = graph.transposed()
            ws = _workspace(lib.gvqa_lcgn_attention_backward_workspace_bytes(C.byref(graph.c), heads, channels), J.device)
            _lib.check(lib.gvqa_lcgn_attention_backward(C.byref(graph.c), C.byref(gt.c), heads, channels, int(concat), slope, J.data_ptr(),
                                                        3 * HC, pc.data_ptr(), 2 * HC, alpha.data_ptr(), _ptr(mask), dout.data_ptr(),
                                                        dout.shape[1], dJ.data_ptr(), 3 * HC, dpc.data_ptr(), 2 * HC, ws.data_ptr(),
                                                        ws.numel(), _stream(J.device)))
        dbias = dout.sum(dim=0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dJ, dpc, dbias, None, None, None, None, None, None


def lcgn_attention(J: torch.Tensor, pc: torch.Tensor, graph: SceneGraphBatch, heads: int, channels: int, concat: bool,
                   negative_slope: float = 0.2, bias: torch.Tensor | None = None, want_alpha: bool = False,
                   mask: torch.Tensor | None = None):
    """gat_lcgn's attention + aggregation for H heads as one HIP launch.
    J [N, 3HC] = [x_l | x_r | x_val], pc [B, 2HC] = [proj_cmd | cal_cmd] per graph -> (out [N, HC] (concat) or [N, C], alpha [E, H]
    or None).  mask [E, H] (COO order, optional): the attention dropout's keep factors, scaled by 1 / (1 - p); they multiply the
    messages after the softmax.  Differentiable in J, pc and bias (HIP backward kernels, deterministic); alpha is returned
    detached.  Without gradients and without a mask this is gvqa_lcgn_attention (inference)."""
    lib = _lib.load()
    HC = heads * channels
    J, pc = _f32c(J, "J"), _f32c(pc, "pc")
    if J.shape != (graph.num_nodes, 3 * HC) or pc.shape != (graph.num_graphs, 2 * HC):
        raise ValueError("lcgn_attention: J must be [N, 3 H C] and pc [B, 2 H C]")
    if bias is not None:
        bias = _f32c(bias, "bias")
    if mask is not None:
        mask = _f32c(mask, "mask")
        if mask.shape != (graph.num_edges, heads):
            raise ValueError("lcgn_attention: mask must be [E, H]")
    needs_grad = torch.is_grad_enabled() and (J.requires_grad or pc.requires_grad or (bias is not None and bias.requires_grad))
    if needs_grad or mask is not None:
        out, alpha = _LcgnAttention.apply(J, pc, bias, mask, graph, heads, channels, concat, negative_slope)
        return out, (alpha if want_alpha else None)
    cout = HC if concat else channels
    out = torch.empty((graph.num_nodes, cout), dtype=torch.float32, device=J.device)
    alpha = torch.empty((graph.num_edges, heads), dtype=torch.float32, device=J.device) if want_alpha else None
    with torch.cuda.device(J.device):
        _lib.check(lib.gvqa_lcgn_attention(C.byref(graph.c), heads, channels, int(bool(concat)), negative_slope, J.data_ptr(), 3 * HC,
                                           pc.data_ptr(), 2 * HC, _ptr(bias), out.data_ptr(), cout, _ptr(alpha), _stream(J.device)))
    return out, alpha


def _attention_bf16_supported(heads: int, channels: int) -> bool:
    return 1 <= heads <= _ATT_MAX_HEADS and channels > 0 and channels % 8 == 0 and heads * channels <= _ATT_MAX_HC


class _LcgnAttentionBf16(torch.autograd.Function):
    """_LcgnAttention on a J stored as bf16: gvqa_lcgn_attention_bf16_train forward, gvqa_lcgn_attention_bf16_backward.  J is bf16, or
    fp32 and rounded to bf16 (to nearest even) here with a straight-through gradient (_StoreBf16 fused with the attention).  Saved:
    J as bf16, pc, alpha and the mask -- never an fp32 [N, 3HC] tensor.  dJ comes back fp32 for an fp32 J, rounded once to bf16 for a
    bf16 J.  Operands checked and made contiguous by the caller."""

    @staticmethod
    def forward(ctx, J, pc, bias, mask, graph, heads, channels, concat, slope):
        lib = _lib.load()
        HC = heads * channels
        cout = HC if concat else channels
        J16 = J if J.dtype == torch.bfloat16 else J.to(torch.bfloat16)
        out = torch.empty((graph.num_nodes, cout), dtype=torch.float32, device=J.device)
        alpha = torch.empty((graph.num_edges, heads), dtype=torch.float32, device=J.device)
        with torch.cuda.device(J.device):
            _lib.check(lib.gvqa_lcgn_attention_bf16_train(C.byref(graph.c), heads, channels, int(bool(concat)), slope, J16.data_ptr(),
                                                          3 * HC, pc.data_ptr(), 2 * HC, _ptr(bias), _ptr(mask), out.data_ptr(), cout,
                                                          alpha.data_ptr(), _stream(J.device)))
        ctx.save_for_backward(J16, pc, alpha, mask)
        ctx.graph, ctx.dims, ctx.has_bias = graph, (heads, channels, bool(concat), slope), bias is not None
        ctx.j_dtype = J.dtype
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dalpha):
        lib = _lib.load()
        J16, pc, alpha, mask = ctx.saved_tensors
        heads, channels, concat, slope = ctx.dims
        graph, HC = ctx.graph, heads * channels
        # a view, a broadcast or an unaligned slice as dout is copied, never refused
        dout = dout.to(torch.float32).contiguous()
        if dout.data_ptr() % 16:
            dout = dout.clone(memory_format=torch.contiguous_format)
        dJ = torch.empty(J16.shape, dtype=torch.float32, device=J16.device)
        dpc = torch.empty_like(pc)
        with torch.cuda.device(J16.device):
            gt = graph.transposed()
            ws = _workspace(lib.gvqa_lcgn_attention_bf16_backward_workspace_bytes(C.byref(graph.c), heads, channels), J16.device)
            _lib.check(lib.gvqa_lcgn_attention_bf16_backward(C.byref(graph.c), C.byref(gt.c), heads, channels, int(concat), slope,
                                                             J16.data_ptr(), 3 * HC, pc.data_ptr(), 2 * HC, alpha.data_ptr(), _ptr(mask),
                                                             dout.data_ptr(), dout.shape[1], dJ.data_ptr(), 3 * HC, dpc.data_ptr(),
                                                             2 * HC, ws.data_ptr(), ws.numel(), _stream(J16.device)))
        if ctx.j_dtype == torch.bfloat16:
            dJ = dJ.to(torch.bfloat16)
        dbias = dout.sum(dim=0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dJ, dpc, dbias, None, None, None, None, None, None


def _lcgn_attention_store_bf16(J, pc, graph: SceneGraphBatch, heads: int, channels: int, concat: bool, negative_slope: float = 0.2,
                               bias=None, mask=None):
    """The differentiable bf16 attention on an fp32 J [N, 3HC]: J is rounded to bf16 inside the node (straight-through gradient,
    dJ fp32) and kept for the backward as bf16 only.  Shapes within _attention_bf16_supported.  -> (out fp32, alpha detached)."""
    HC = heads * channels
    J, pc = _f32c(J, "J"), _f32c(pc, "pc")
    if J.shape != (graph.num_nodes, 3 * HC) or pc.shape != (graph.num_graphs, 2 * HC):
        raise ValueError("lcgn_attention: J must be [N, 3 H C] and pc [B, 2 H C]")
    if bias is not None:
        bias = _f32c(bias, "bias")
    if mask is not None:
        mask = _f32c(mask, "mask")
        if mask.shape != (graph.num_edges, heads):
            raise ValueError("lcgn_attention: mask must be [E, H]")
    return _LcgnAttentionBf16.apply(J, pc, bias, mask, graph, heads, channels, concat, negative_slope)


def lcgn_attention_bf16(J16: torch.Tensor, pc: torch.Tensor, graph: SceneGraphBatch, heads: int, channels: int, concat: bool,
                        negative_slope: float = 0.2, bias: torch.Tensor | None = None, want_alpha: bool = False,
                        out_dtype: torch.dtype = torch.bfloat16, out: torch.Tensor | None = None, mask: torch.Tensor | None = None):
    """lcgn_attention on a J stored as bf16 (gvqa_lcgn_attention_bf16: one launch).  J16 [N, 3HC] bf16, pc [B, 2HC]
    and bias fp32 -> (out [N, HC] (concat) or [N, C] in `out_dtype` (bfloat16: rounded once, after the head mean and the bias; or
    float32), alpha [E, H] fp32 or None).  `out`: an [N, C_out] view of `out_dtype` with unit inner stride to write into (a column
    block of a wider buffer).  Shapes the entry point does not take (C % 8 != 0) run the fp32 kernel on J16.float(): the same
    values on a slower road.  mask [E, H] (COO order, optional): the attention dropout's keep factors, as lcgn_attention takes
    them.  Differentiable in J16, pc and bias (gvqa_lcgn_attention_bf16_train / _backward: J is saved as bf16, J16.grad is the fp32
    gradient rounded once to bf16, alpha is returned detached); when gradients are needed or a mask is given, out_dtype must be
    torch.float32 and out must be None."""
    lib = _lib.load()
    HC = heads * channels
    cout = HC if concat else channels
    if not J16.is_cuda:
        raise RuntimeError(f"J16 is on {J16.device}: the MI355X execution path has no CPU fallback")
    if J16.dtype != torch.bfloat16 or out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("lcgn_attention_bf16: J16 must be bfloat16 and out_dtype bfloat16 or float32")
    J16, pc = J16.contiguous(), _f32c(pc, "pc")
    if J16.shape != (graph.num_nodes, 3 * HC) or pc.shape != (graph.num_graphs, 2 * HC):
        raise ValueError("lcgn_attention_bf16: J16 must be [N, 3 H C] and pc [B, 2 H C]")
    if bias is not None:
        bias = _f32c(bias, "bias")
    if mask is not None:
        mask = _f32c(mask, "mask")
        if mask.shape != (graph.num_edges, heads):
            raise ValueError("lcgn_attention_bf16: mask must be [E, H]")
    needs_grad = torch.is_grad_enabled() and (J16.requires_grad or pc.requires_grad or (bias is not None and bias.requires_grad))
    if needs_grad or mask is not None:
        if out_dtype != torch.float32 or out is not None:
            raise ValueError("lcgn_attention_bf16: out_dtype must be torch.float32 and out must be None when gradients are needed or "
                             "a mask is given")
        if not _attention_bf16_supported(heads, channels):
            return lcgn_attention(J16.float(), pc, graph, heads, channels, concat, negative_slope, bias, want_alpha, mask=mask)
        res, alpha = _LcgnAttentionBf16.apply(J16, pc, bias, mask, graph, heads, channels, concat, negative_slope)
        return res, (alpha if want_alpha else None)
    if out is None:
        out = torch.empty((graph.num_nodes, cout), dtype=out_dtype, device=J16.device)
    elif out.shape != (graph.num_nodes, cout) or out.dtype != out_dtype or out.stride(1) != 1 or out.device != J16.device:
        raise ValueError("lcgn_attention_bf16: `out` must be an [N, C_out] view of out_dtype with unit inner stride")
    if not _attention_bf16_supported(heads, channels):
        res, alpha = lcgn_attention(J16.float(), pc, graph, heads, channels, concat, negative_slope, bias, want_alpha)
        out.copy_(res)
        return out, alpha
    alpha = torch.empty((graph.num_edges, heads), dtype=torch.float32, device=J16.device) if want_alpha else None
    with torch.cuda.device(J16.device):
        _lib.check(lib.gvqa_lcgn_attention_bf16(C.byref(graph.c), heads, channels, int(bool(concat)), negative_slope, J16.data_ptr(),
                                                3 * HC, pc.data_ptr(), 2 * HC, _ptr(bias), out.data_ptr(), out.stride(0),
                                                int(out_dtype == torch.bfloat16), _ptr(alpha), _stream(J16.device)))
    return out, alpha


def _lcgn_attention_autograd(J, pc, graph: SceneGraphBatch, heads: int, channels: int, concat: bool, negative_slope: float,
                             bias=None, p_att: float = 0.0):
    """Differentiable form of lcgn_attention (lcgn.py:148-238) on the library's building blocks: the dot-product logits
    x_l[src] . (proj_cmd[g(dst)] * x_r[dst]) per edge and head enter the GAT message passing as its per-edge term (leaky-relu,
    softmax, the alpha-weighted sum and their backward run there); x_val is scaled per node by its own graph's cal_cmd row first,
    which is the source's row of every message (lcgn.py:231) in any batch.  concat: one H = 1 message passing per head, the heads
    side by side (as gat._forward_autograd).  p_att > 0: attention dropout (lcgn.py:212) as a drawn mask."""
    H, Cc, HC = heads, channels, heads * channels
    N, E, dev = graph.num_nodes, graph.num_edges, J.device
    x_l, x_r, x_val = J[:, :HC], J[:, HC:2 * HC], J[:, 2 * HC:]
    y = graph_rows(pc[:, :HC], graph) * x_r                                                            # :152-154
    a_edge = (edge_gather(x_l, graph, "src") * edge_gather(y, graph, "dst")).view(E, H, Cc).sum(dim=-1)  # :207
    xv = x_val * graph_rows(pc[:, HC:], graph)                                                         # :153,230-231
    mask = torch.bernoulli(torch.full((E, H), 1.0 - p_att, device=dev)) / (1.0 - p_att) if p_att > 0 else None
    if not concat:
        out, alpha = gat_message_passing(xv, torch.zeros((N, 2 * H), device=dev), a_edge, graph, H, Cc, negative_slope, mask)
    else:
        outs, alphas = [], []
        zeros2 = torch.zeros((N, 2), device=dev)
        for h in range(H):
            o_h, al_h = gat_message_passing(xv[:, h * Cc:(h + 1) * Cc].contiguous(), zeros2, a_edge[:, h:h + 1].contiguous(), graph, 1, Cc,
                                            negative_slope, None if mask is None else mask[:, h:h + 1].contiguous())
            outs.append(o_h); alphas.append(al_h)
        out, alpha = torch.cat(outs, dim=1), torch.cat(alphas, dim=1)
    if bias is not None:
        out = out + bias
    return out, alpha


_FORCE_COMPOSITION = False      # tests and scripts/bench_lcgn_attention_train.py only: training takes _lcgn_attention_autograd


def _attention_train(J, pc, graph: SceneGraphBatch, heads: int, channels: int, concat: bool, negative_slope: float, bias=None,
                     p_att: float = 0.0, store_bf16: bool = False):
    """The attention of a training step: the differentiable lcgn_attention (HIP forward and backward kernels) for the shapes the
    kernels take, else the composition.  The dropout mask is drawn as _lcgn_attention_autograd draws it (same call, same shape,
    same place in the order of draws): one torch seed gives one mask on every road.  store_bf16: J is a per-node tensor of the
    bf16-node-feature mode, not yet rounded -- the bf16 attention node rounds it and saves it as bf16 (shapes within
    _attention_bf16_supported); on the other roads it is rounded first (_StoreBf16), the same values."""
    if _FORCE_COMPOSITION or not _attention_supported(heads, channels):
        J = _StoreBf16.apply(J) if store_bf16 else J
        return _lcgn_attention_autograd(J, pc, graph, heads, channels, concat, negative_slope, bias, p_att)
    mask = torch.bernoulli(torch.full((graph.num_edges, heads), 1.0 - p_att, device=J.device)) / (1.0 - p_att) if p_att > 0 else None
    if store_bf16 and _attention_bf16_supported(heads, channels):
        return _lcgn_attention_store_bf16(J, pc, graph, heads, channels, concat, negative_slope, bias, mask)
    J = _StoreBf16.apply(J) if store_bf16 else J
    return lcgn_attention(J, pc, graph, heads, channels, concat, negative_slope, bias, want_alpha=True, mask=mask)


def _stack_key(tensors, device):
    return (str(device),) + tuple((t.data_ptr(), t._version) for t in tensors)


class _StoreBf16(torch.autograd.Function):
    """A per-node tensor as the bf16-node-feature mode keeps it in HBM: rounded to bf16 (to nearest even) in the forward, the
    gradient passed straight through -- the rounding is a storage format, not part of the model."""

    @staticmethod
    def forward(ctx, v):
        return v.to(torch.bfloat16).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        return g


class gat_lcgn(nn.Module):
    """The reference's `gat_lcgn` layer (lcgn.py:17-238): command-conditioned dot-product attention over the in-edges.

    forward(x, edge_index, cmd, batch, edge_attr=None, size=None, return_attention_weights=None, graph=None) -> out [N, H C]
    (concat=True) / [N, C] (concat=False), or (out, (edge_index, alpha [E, H])).  `cmd` [B, cmd_dim] holds one command per graph of
    `batch`; `edge_attr` is ignored, as in the reference; `graph` takes a prebuilt SceneGraphBatch.  In eval without gradients the
    layer is one C-ABI call (gvqa_gat_lcgn_forward: one stacked node product, the per-graph command product, one attention launch);
    with gradients or in training with dropout it is the library's differentiable products around the differentiable
    lcgn_attention (gvqa_lcgn_attention_train / _backward); shapes outside the attention kernels' limits (H <= 8, C % 4 == 0,
    H C <= 4096) take a differentiable composition of the library's building blocks (_lcgn_attention_autograd).  Inside `lcgn_seq` the layer's weights are
    used by lcgn_seq's own forward."""

    def __init__(self, in_channels, out_channels, edge_in_channels, heads=1, concat=True, negative_slope=0.2,
                 dropout=0.0, cmd_dim=512, add_self_loops=True, bias=True, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.lin_l = Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = Linear(in_channels, heads * out_channels, bias=False)
        self.cal_x = Linear(in_channels, heads * out_channels, bias=False)
        self.proj_cmd = Linear(cmd_dim, heads * out_channels, False)
        self.cal_cmd = Linear(cmd_dim, heads * out_channels, False)
        if bias and concat:
            self.bias = Parameter(torch.empty(heads * out_channels))
        elif bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_l, self.lin_r, self.proj_cmd, self.cal_cmd, self.cal_x):
            _glorot(lin.weight)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def _stacked(self, device):
        """[lin_l; lin_r; cal_x] and [proj_cmd; cal_cmd] as contiguous fp32 stacks (the C call then reads them in place), rebuilt
        only when a weight tensor was replaced or modified in place (data_ptr / autograd version counter)."""
        ws = (self.lin_l.weight, self.lin_r.weight, self.cal_x.weight, self.proj_cmd.weight, self.cal_cmd.weight)
        key = _stack_key(ws, device)
        if getattr(self, "_stack_cache", None) is None or self._stack_cache[0] != key:
            with torch.no_grad():
                w3 = torch.cat([_f32c(w, "weight") for w in ws[:3]], dim=0).contiguous()
                wpc = torch.cat([_f32c(w, "weight") for w in ws[3:]], dim=0).contiguous()
            self._stack_cache = (key, w3, wpc)
        return self._stack_cache[1], self._stack_cache[2]

    def _forward_autograd(self, x, cmd, graph):
        proj = _ProjectionLinear.apply
        J = proj(x, torch.cat([self.lin_l.weight, self.lin_r.weight, self.cal_x.weight], dim=0))               # :144-145,230
        pc = proj(cmd, torch.cat([self.proj_cmd.weight, self.cal_cmd.weight], dim=0))                          # :148-149
        p_att = self.dropout if self.training else 0.0
        return _attention_train(J, pc, graph, self.heads, self.out_channels, self.concat, self.negative_slope, self.bias, p_att)

    def forward(self, x, edge_index, cmd, batch, edge_attr=None, size=None, return_attention_weights=None,
                graph: SceneGraphBatch | None = None):
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("gat_lcgn: a pair x (bipartite message passing) is not supported")
        if size is not None:
            raise NotImplementedError("gat_lcgn: bipartite `size` is not supported")
        assert x.dim() == 2, "Static graphs not supported in `GATConv`."                                       # lcgn.py:138
        lib = _lib.load()
        x, cmd = _f32c(x, "x"), _f32c(cmd, "cmd")
        H, Cc = self.heads, self.out_channels
        N, B = x.shape[0], cmd.shape[0]
        if x.shape[1] != self.lin_l.weight.shape[1] or cmd.dim() != 2 or cmd.shape[1] != self.proj_cmd.weight.shape[1]:
            raise ValueError("gat_lcgn: feature widths do not match the layer")
        if graph is None:
            if batch is None:
                batch = torch.zeros(N, dtype=torch.int64, device=x.device)
            graph = SceneGraphBatch(edge_index, batch, N, B)
        if graph.num_nodes != N or graph.num_graphs != B:
            raise ValueError("gat_lcgn: the graph does not match x / cmd (one command row per graph)")
        want_alpha = isinstance(return_attention_weights, bool)
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or cmd.requires_grad or any(w.requires_grad for w in self.parameters()))
        if needs_grad or (self.training and self.dropout > 0) or not _attention_supported(H, Cc):
            out, alpha = self._forward_autograd(x, cmd, graph)
        else:
            w3, wpc = self._stacked(x.device)
            HC, K = H * Cc, x.shape[1]
            p = _lib.LcgnParams()
            p.lin_l_weight, p.lin_r_weight, p.cal_x_weight = w3.data_ptr(), w3.data_ptr() + 4 * HC * K, w3.data_ptr() + 8 * HC * K
            p.proj_cmd_weight, p.cal_cmd_weight = wpc.data_ptr(), wpc.data_ptr() + 4 * HC * cmd.shape[1]
            bias = None if self.bias is None else _f32c(self.bias, "bias")
            p.bias = _ptr(bias)
            out = torch.empty((N, HC if self.concat else Cc), dtype=torch.float32, device=x.device)
            alpha = torch.empty((graph.num_edges, H), dtype=torch.float32, device=x.device) if want_alpha else None
            with torch.cuda.device(x.device):
                ws = _workspace(lib.gvqa_gat_lcgn_workspace_bytes(C.byref(graph.c), K, Cc, H, cmd.shape[1]), x.device)
                _lib.check(lib.gvqa_gat_lcgn_forward(C.byref(graph.c), K, Cc, H, cmd.shape[1], int(bool(self.concat)), self.negative_slope,
                                                     C.byref(p), x.data_ptr(), cmd.data_ptr(), out.data_ptr(), _ptr(alpha), ws.data_ptr(),
                                                     ws.numel(), _stream(x.device)))
        return (out, (edge_index, alpha)) if want_alpha else out

    def __repr__(self):
        return "{}({}, {}, heads={})".format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)


class lcgn_seq(nn.Module):
    def __init__(self, in_channels, out_channels, edge_attr_dim, num_ins, gat_cmd_dim=512, question_dim=512,
                 MAX_ITER_NUM=4, dropout=0.0, gat_heads=1, gat_negative_slope=0.2, gat_bias=True,
                 node_feature_dtype: torch.dtype = torch.float32, bf16_weight_pieces: int = 2):
        super().__init__()
        _lib.load()
        if node_feature_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("node_feature_dtype must be torch.float32 or torch.bfloat16")
        # build-side choice (BASELINE config 5): per-node tensors stored as bf16 in HBM, node GEMMs on the
        # bf16 matrix cores (fp32 accumulation) against the fp32 weights split into `bf16_weight_pieces`
        # bf16 pieces (2: the weights keep 16 significant bits; 1: weights rounded to bf16)
        if bf16_weight_pieces not in (1, 2):
            raise ValueError("bf16_weight_pieces must be 1 or 2")
        self.node_feature_dtype = node_feature_dtype
        self.bf16_weight_pieces = bf16_weight_pieces
        self._packed, self._packed_key = None, None
        self.init_sg_emb_input = nn.Sequential(Linear(in_channels, out_channels), nn.Dropout(dropout))
        self.MAX_ITER_NUM = MAX_ITER_NUM
        self.qInput1 = Linear(question_dim, out_channels)
        for t in range(MAX_ITER_NUM):
            setattr(self, "qInput2_%d" % t, Linear(out_channels, out_channels))
        self.cmd_inter2logits = Linear(out_channels, 1)
        self.dropout = dropout
        self.proj_x_loc = nn.Sequential(nn.Dropout(dropout), Linear(out_channels, out_channels))
        self.proj_x_ctx = nn.Sequential(nn.Dropout(dropout), Linear(out_channels, out_channels))
        self.output_layer = Linear(2 * out_channels, out_channels)
        self.fin_layer = Linear(2 * out_channels, out_channels)
        self.lcgn = gat_lcgn(in_channels=3 * out_channels, out_channels=out_channels, edge_in_channels=1,
                             heads=gat_heads, concat=False, negative_slope=gat_negative_slope, dropout=dropout,
                             bias=gat_bias, cmd_dim=gat_cmd_dim)
        self.bns = nn.ModuleList([nn.BatchNorm1d(out_channels) for _ in range(num_ins - 1)])   # dead in the reference too
        self.in_channels, self.out_channels, self.question_dim = in_channels, out_channels, question_dim
        self.gat_cmd_dim, self.gat_heads, self.negative_slope = gat_cmd_dim, gat_heads, gat_negative_slope

    def _forward_autograd(self, x, edge_index, q, lstm, graph, x_ctx_init):
        """Differentiable / training formulation of lcgn.py:303-323: the node-sized dense layers (with the module's
        dropouts) and their dx / dW run on the library's own products (_ProjectionLinear: the arithmetic
        GVQA_OPT_PROJECTION selects, as in the eval path), the per-question layers are torch ops; the per-graph command broadcasts, the softmax-weighted neighbour sum and their backward run on the HIP
        per-graph / message-passing kernels (the dot-product logit x_l[src] . (proj_cmd * x_r)[dst], lcgn.py:154,207,
        enters the message passing as its per-edge term).
        node_feature_dtype = bfloat16 (BASELINE config 5): the per-node tensors are rounded to bf16 at the points where the
        inference kernels store them (x, x_loc, proj_x_loc, the x_loc block of the joint projection, x_ctx, the gated product,
        x_l | x_r | x_val, the message), with a straight-through gradient; the fp32 master weights are used as they are (the
        inference path multiplies by their two bf16 pieces: 16 of their 24 bits) and gradients stay fp32."""
        rb = _StoreBf16.apply if self.node_feature_dtype == torch.bfloat16 else (lambda v: v)
        if self.gat_heads != 1:
            raise NotImplementedError("lcgn_seq: gat_heads != 1 is not implemented (reference default 1)")
        O, N, E = self.out_channels, x.shape[0], edge_index.shape[1]
        L = self.lcgn
        proj = _ProjectionLinear.apply              # node-sized products + their dx / dW on the library's own GEMMs
        init, p_loc, p_ctx = self.init_sg_emb_input, self.proj_x_loc, self.proj_x_ctx
        x_loc = init[1](rb(proj(rb(x), init[0].weight, init[0].bias)))                # :305
        x_ctx = rb(x_ctx_init)                                                        # :306
        plin = lambda m, v: proj(v, m.weight, m.bias)      # per-question Linears ([B, .]-sized): the library's f32-input kernel, not torch's vendor GEMM
        q_emb = torch.relu(plin(self.qInput1, q))                                     # :307
        proj_x_loc = rb(proj(p_loc[0](x_loc), p_loc[1].weight, p_loc[1].bias))        # :308
        lo = lstm.transpose(1, 0)                                                     # [B, L, O]
        zeros2 = torch.zeros((N, 2), device=x.device)
        p_att = L.dropout if self.training else 0.0
        # lin_l / lin_r / cal_x act on x_joint = [x_loc | x_ctx | proj_x_ctx(x_ctx) * proj_x_loc] (:312-313, :144-145, :230) as
        # one stacked [3O, 3O] weight; its x_loc column block multiplies an iteration-invariant operand: applied once
        w_joint = torch.cat([L.lin_l.weight, L.lin_r.weight, L.cal_x.weight], dim=0)
        z_loc = rb(proj(x_loc, w_joint[:, :O]))
        w_iter = w_joint[:, O:]
        for t in range(self.MAX_ITER_NUM):
            q_cmd = plin(getattr(self, "qInput2_%d" % t), q_emb)                      # :292-300
            # cmd_inter2logits is a [1, O] Linear: its product with q_cmd * lstm_out is a weighted sum over channels
            att = torch.softmax(((q_cmd * self.cmd_inter2logits.weight)[:, None, :] * lo).sum(dim=-1) + self.cmd_inter2logits.bias, dim=-1)
            cmd = (att[:, :, None] * lo).sum(dim=1)                                    # (a weighted sum over the L question tokens: no batched GEMM)
            x_pair = torch.cat([x_ctx, rb(proj(p_ctx[0](x_ctx), p_ctx[1].weight, p_ctx[1].bias) * proj_x_loc)], dim=-1)
            x_l, x_r, x_val = rb(proj(x_pair, w_iter) + z_loc).split(O, dim=1)
            y = graph_rows(plin(L.proj_cmd, cmd), graph) * x_r                        # :148-154
            a_edge = (edge_gather(x_l, graph, "src") * edge_gather(y, graph, "dst")).sum(dim=-1, keepdim=True)   # :207
            mask = torch.bernoulli(torch.full((E, 1), 1.0 - p_att, device=x.device)) / (1.0 - p_att) if p_att > 0 else None
            agg, _ = gat_message_passing(x_val, zeros2, a_edge, graph, 1, O, self.negative_slope, mask)   # :209-238
            msg = agg * graph_rows(plin(L.cal_cmd, cmd), graph)                       # :231 (edges are intra-graph)
            if L.bias is not None:
                msg = msg + L.bias
            x_ctx = rb(proj(torch.cat([x_ctx, rb(msg)], dim=-1), self.output_layer.weight, self.output_layer.bias))   # :316-319
        return proj(torch.cat([x_loc, x_ctx], dim=-1), self.fin_layer.weight, self.fin_layer.bias)           # :321-322

    def _forward_heads(self, x, q, lstm, graph, x_ctx_init, fused):
        """gat_heads = H > 1 (lcgn.py:303-323, the layer's heads averaged: concat=False): the formulation of _forward_autograd with
        lin_l / lin_r / cal_x as one stacked [3 H O, 3 O] weight (its x_loc column block applied once) and [proj_cmd; cal_cmd] as one
        [2 H O, O] product per iteration.  fused (eval without gradients): each iteration's attention + aggregation is one
        gvqa_lcgn_attention launch and the stacked weights are cached; otherwise the differentiable lcgn_attention
        (_attention_train, attention dropout in training).  node_feature_dtype = bfloat16 (fused=False only; the eval road is
        _forward_heads_bf16): the per-node tensors are rounded to bf16 where that road stores them, with a straight-through
        gradient; J is rounded inside the bf16 attention node (gvqa_lcgn_attention_bf16_train / _backward), which keeps it for the
        backward as bf16 -- for out_channels outside the bf16 kernels' shapes the fp32 attention kernels run on the rounded values."""
        H, O = self.gat_heads, self.out_channels
        L = self.lcgn
        proj = _ProjectionLinear.apply
        init, p_loc, p_ctx = self.init_sg_emb_input, self.proj_x_loc, self.proj_x_ctx
        plin = lambda m, v: proj(v, m.weight, m.bias)
        # node_feature_dtype = bfloat16 (never fused: that is _forward_heads_bf16): the roundings of _forward_autograd
        store16 = self.node_feature_dtype == torch.bfloat16
        rb = _StoreBf16.apply if store16 else (lambda v: v)
        if fused:
            ws = (L.lin_l.weight, L.lin_r.weight, L.cal_x.weight, L.proj_cmd.weight, L.cal_cmd.weight)
            key = _stack_key(ws, x.device)
            if getattr(self, "_heads_cache", None) is None or self._heads_cache[0] != key:
                with torch.no_grad():
                    self._heads_cache = (key, torch.cat(ws[:3], dim=0).contiguous(), torch.cat(ws[3:], dim=0).contiguous())
            w_joint, w_pc = self._heads_cache[1], self._heads_cache[2]
        else:
            w_joint = torch.cat([L.lin_l.weight, L.lin_r.weight, L.cal_x.weight], dim=0)
            w_pc = torch.cat([L.proj_cmd.weight, L.cal_cmd.weight], dim=0)
        x_loc = init[1](rb(proj(rb(x), init[0].weight, init[0].bias)))                            # :305
        x_ctx = rb(x_ctx_init)                                                                    # :306
        q_emb = torch.relu(plin(self.qInput1, q))                                                 # :307
        proj_x_loc = rb(proj(p_loc[0](x_loc), p_loc[1].weight, p_loc[1].bias))                    # :308
        lo = lstm.transpose(1, 0)
        p_att = L.dropout if self.training else 0.0
        z_loc = rb(proj(x_loc, w_joint[:, :O]))                # x_loc's column block of x_joint . [lin_l; lin_r; cal_x]^T, once
        w_iter = w_joint[:, O:]
        for t in range(self.MAX_ITER_NUM):
            q_cmd = plin(getattr(self, "qInput2_%d" % t), q_emb)                                  # :292-300
            att = torch.softmax(((q_cmd * self.cmd_inter2logits.weight)[:, None, :] * lo).sum(dim=-1) + self.cmd_inter2logits.bias, dim=-1)
            cmd = (att[:, :, None] * lo).sum(dim=1)
            x_pair = torch.cat([x_ctx, rb(proj(p_ctx[0](x_ctx), p_ctx[1].weight, p_ctx[1].bias) * proj_x_loc)], dim=-1)   # :312-313
            J = proj(x_pair, w_iter) + z_loc                                                      # [x_l | x_r | x_val]   :144-145,230
            pc = proj(cmd, w_pc)                                                                  # [proj_cmd | cal_cmd]  :148-149
            if fused:
                msg, _ = lcgn_attention(J, pc, graph, H, O, False, self.negative_slope, L.bias)   # :150-238
            else:           # bf16 mode: J is rounded where it is stored, inside the bf16 attention node or just ahead of the fp32 one
                msg, _ = _attention_train(J, pc, graph, H, O, False, self.negative_slope, L.bias, p_att, store_bf16=store16)
            x_ctx = rb(proj(torch.cat([x_ctx, rb(msg)], dim=-1), self.output_layer.weight, self.output_layer.bias))   # :316-319
        return proj(torch.cat([x_loc, x_ctx], dim=-1), self.fin_layer.weight, self.fin_layer.bias)           # :321-322

    def _bf16_heads_weights(self, device):
        """The node products' weights as gvqa_linear_bf16 reads them (gvqa_pack_weight_bf16: `bf16_weight_pieces` bf16 pieces side
        by side), the fp32 biases and [proj_cmd; cal_cmd]; rebuilt only when a weight was replaced or modified in place, or the
        number of pieces changed.  init's K is zero-padded to a multiple of 8 (the bf16 kernel's K step)."""
        L, O, P = self.lcgn, self.out_channels, self.bf16_weight_pieces
        ws = (self.init_sg_emb_input[0].weight, self.proj_x_loc[1].weight, self.proj_x_ctx[1].weight, L.lin_l.weight, L.lin_r.weight,
              L.cal_x.weight, self.output_layer.weight, self.fin_layer.weight, L.proj_cmd.weight, L.cal_cmd.weight)
        key = _stack_key(ws, device) + (P,)
        if getattr(self, "_heads16_cache", None) is not None and self._heads16_cache[0] == key:
            return self._heads16_cache[1]
        lib = _lib.load()

        def pack(W):                    # W [rows, K] fp32, unit inner stride (a column block of a wider weight passes its row stride)
            rows, K = W.shape
            Wpk = torch.empty((rows, P * K), dtype=torch.bfloat16, device=device)
            _lib.check(lib.gvqa_pack_weight_bf16(rows, K, P, W.data_ptr(), W.stride(0), Wpk.data_ptr(), _stream(device)))
            return Wpk

        with torch.no_grad(), torch.cuda.device(device):
            ws = [_f32c(w, "weight") for w in ws]
            K8 = (self.in_channels + 7) // 8 * 8
            w_init = ws[0] if K8 == self.in_channels else torch.nn.functional.pad(ws[0], (0, K8 - self.in_channels))
            w_joint = torch.cat(ws[3:6], dim=0)                 # [3 H O, 3 O]
            packed = dict(init=pack(w_init), p_loc=pack(ws[1]), p_ctx=pack(ws[2]), z_loc=pack(w_joint[:, :O]), iter=pack(w_joint[:, O:]),
                          output=pack(ws[6]), fin=pack(ws[7]), pc=torch.cat(ws[8:], dim=0).contiguous())
        self._heads16_cache = (key, packed)
        return packed

    def _forward_heads_bf16(self, x, q, lstm, graph, x_ctx_init):
        """gat_heads = H > 1 with node_feature_dtype = bfloat16, eval without gradients: every per-node tensor lives in HBM as bf16.
        The node products are gvqa_linear_bf16 (bf16 matrix cores, fp32 accumulation, bf16 C / addend / mul) against the packed
        weight pieces, writing through their leading dimension into [N, 2 O] pair buffers, so that [x_ctx | prod], [x_ctx | msg]
        and [x_loc | x_ctx] are each ONE product's A operand (no concatenation, one rounding of J); z_loc rides as the J product's
        addend and proj_x_loc as the proj_x_ctx product's mul; each iteration's attention is one gvqa_lcgn_attention_bf16 launch
        that writes the message (bf16) into its pair buffer.  The per-question path (q_emb, cmd, pc) is fp32; the output is fp32.
        Rounding points: those of the gat_heads = 1 bf16 kernels (x, x_loc, proj_x_loc, z_loc, x_ctx, prod, J, the message)."""
        lib = _lib.load()
        H, O, P = self.gat_heads, self.out_channels, self.bf16_weight_pieces
        L, N, dev = self.lcgn, x.shape[0], x.device
        bf = torch.bfloat16
        W = self._bf16_heads_weights(dev)
        proj = _ProjectionLinear.apply
        plin = lambda m, v: proj(v, m.weight, m.bias)
        st = _stream(dev)

        def lin(A, Wpk, n_out, Cv, bias=None, addend=None, mul=None, c_bf16=1):
            """Cv[N, n_out] = (A . Wpk^T + bias + addend) * mul; A, Cv, addend, mul: views with unit inner stride."""
            _lib.check(lib.gvqa_linear_bf16(N, n_out, A.shape[1], P, A.data_ptr(), A.stride(0), Wpk.data_ptr(), _ptr(bias), _ptr(addend),
                                            0 if addend is None else addend.stride(0), _ptr(mul), 0 if mul is None else mul.stride(0), 0,
                                            Cv.data_ptr(), Cv.stride(0), c_bf16, st))

        fb = lambda m: _f32c(m.bias, "bias")
        with torch.cuda.device(dev):
            K8 = (self.in_channels + 7) // 8 * 8
            x16 = torch.empty((N, K8), dtype=bf, device=dev)
            x16[:, :self.in_channels].copy_(x)
            if K8 != self.in_channels:
                x16[:, self.in_channels:].zero_()
            # pair[0] / pair[1]: [x_ctx | prod, then msg], the iterations alternate; fin_in: [x_loc | last x_ctx]
            pair = [torch.empty((N, 2 * O), dtype=bf, device=dev) for _ in range(2)]
            fin_in = torch.empty((N, 2 * O), dtype=bf, device=dev)
            x_loc = fin_in[:, :O]
            lin(x16, W["init"], O, x_loc, fb(self.init_sg_emb_input[0]))                         # :305
            pair[0][:, :O].copy_(x_ctx_init)                                                     # :306
            q_emb = torch.relu(plin(self.qInput1, q))                                            # :307
            proj_x_loc = torch.empty((N, O), dtype=bf, device=dev)
            lin(x_loc, W["p_loc"], O, proj_x_loc, fb(self.proj_x_loc[1]))                        # :308
            z_loc = torch.empty((N, 3 * H * O), dtype=bf, device=dev)
            lin(x_loc, W["z_loc"], 3 * H * O, z_loc)
            J = torch.empty((N, 3 * H * O), dtype=bf, device=dev)
            lo = lstm.transpose(1, 0)
            T = self.MAX_ITER_NUM
            for t in range(T):
                cur = pair[t % 2]
                q_cmd = plin(getattr(self, "qInput2_%d" % t), q_emb)                             # :292-300
                att = torch.softmax(((q_cmd * self.cmd_inter2logits.weight)[:, None, :] * lo).sum(dim=-1) + self.cmd_inter2logits.bias, dim=-1)
                cmd = (att[:, :, None] * lo).sum(dim=1)
                pc = proj(cmd, W["pc"])                                                          # [proj_cmd | cal_cmd]  :148-149
                lin(cur[:, :O], W["p_ctx"], O, cur[:, O:], fb(self.proj_x_ctx[1]), mul=proj_x_loc)   # prod              :312-313
                lin(cur, W["iter"], 3 * H * O, J, addend=z_loc)                                  # [x_l | x_r | x_val]   :144-145,230
                lcgn_attention_bf16(J, pc, graph, H, O, False, self.negative_slope, L.bias, out=cur[:, O:])   # msg over prod :150-238
                nxt = fin_in[:, O:] if t == T - 1 else pair[(t + 1) % 2][:, :O]
                lin(cur, W["output"], O, nxt, fb(self.output_layer))                             # :316-319
            if T == 0:
                fin_in[:, O:].copy_(pair[0][:, :O])
            out = torch.empty((N, O), dtype=torch.float32, device=dev)
            lin(fin_in, W["fin"], O, out, fb(self.fin_layer), c_bf16=0)                          # :321-322
        return out

    def forward(self, x, edge_index, batch, q_encoding, lstm_outputs, edge_attr=None, instr_vectors=None,
                graph: SceneGraphBatch | None = None, x_ctx_init: torch.Tensor | None = None):
        lib = _lib.load()
        x = _f32c(x, "x")
        q = _f32c(q_encoding, "q_encoding")
        lstm = _f32c(lstm_outputs, "lstm_outputs")
        N, O = x.shape[0], self.out_channels
        B, L = q.shape[0], lstm.shape[0]
        if self.gat_cmd_dim != O or lstm.shape[2] != O:
            raise ValueError("command width must equal out_channels (cmd is a weighted sum of lstm_outputs)")
        if lstm.shape[1] != B or x.shape[1] != self.in_channels or q.shape[1] != self.question_dim:
            raise ValueError("input shapes do not match the module")
        if x_ctx_init is None:
            x_ctx_init = torch.randn((N, O)).to(x.device)          # lcgn.py:306: CPU generator, then moved
        x_ctx_init = _f32c(x_ctx_init, "x_ctx_init")
        if graph is None:
            graph = SceneGraphBatch(edge_index, batch, N, B)
        differentiable = self.training or (torch.is_grad_enabled() and (x.requires_grad or q.requires_grad or lstm.requires_grad or
                                                                        any(w.requires_grad for w in self.parameters())))
        if self.gat_heads != 1:
            if self.node_feature_dtype == torch.bfloat16:
                # out_channels outside the bf16 kernels' shapes (O % 8 != 0, H O > 4096): the rounding road, on the fp32 kernels
                if not differentiable and _attention_bf16_supported(self.gat_heads, O):
                    return self._forward_heads_bf16(x, q, lstm, graph, x_ctx_init)
                return self._forward_heads(x, q, lstm, graph, x_ctx_init, fused=False)
            return self._forward_heads(x, q, lstm, graph, x_ctx_init, fused=not differentiable and _attention_supported(self.gat_heads, O))
        if differentiable:
            return self._forward_autograd(x, edge_index, q, lstm, graph, x_ctx_init)
        d = _lib.LcgnDims(self.in_channels, O, self.question_dim, self.MAX_ITER_NUM, L, self.gat_heads,
                          self.negative_slope,
                          (3 - self.bf16_weight_pieces) if self.node_feature_dtype == torch.bfloat16 else 0)
        p = _lib.LcgnParams()
        keep = []

        def ptr(t, name):
            t = _f32c(t, name)
            keep.append(t)
            return t.data_ptr()

        p.init_weight, p.init_bias = ptr(self.init_sg_emb_input[0].weight, "w"), ptr(self.init_sg_emb_input[0].bias, "b")
        p.qinput1_weight, p.qinput1_bias = ptr(self.qInput1.weight, "w"), ptr(self.qInput1.bias, "b")
        for t in range(self.MAX_ITER_NUM):
            lin = getattr(self, "qInput2_%d" % t)
            p.qinput2_weight[t], p.qinput2_bias[t] = ptr(lin.weight, "w"), ptr(lin.bias, "b")
        p.cmd_logit_weight, p.cmd_logit_bias = ptr(self.cmd_inter2logits.weight, "w"), ptr(self.cmd_inter2logits.bias, "b")
        p.proj_x_loc_weight, p.proj_x_loc_bias = ptr(self.proj_x_loc[1].weight, "w"), ptr(self.proj_x_loc[1].bias, "b")
        p.proj_x_ctx_weight, p.proj_x_ctx_bias = ptr(self.proj_x_ctx[1].weight, "w"), ptr(self.proj_x_ctx[1].bias, "b")
        p.output_weight, p.output_bias = ptr(self.output_layer.weight, "w"), ptr(self.output_layer.bias, "b")
        p.fin_weight, p.fin_bias = ptr(self.fin_layer.weight, "w"), ptr(self.fin_layer.bias, "b")
        p.lin_l_weight, p.lin_r_weight = ptr(self.lcgn.lin_l.weight, "w"), ptr(self.lcgn.lin_r.weight, "w")
        p.cal_x_weight = ptr(self.lcgn.cal_x.weight, "w")
        p.proj_cmd_weight, p.cal_cmd_weight = ptr(self.lcgn.proj_cmd.weight, "w"), ptr(self.lcgn.cal_cmd.weight, "w")
        p.bias = None if self.lcgn.bias is None else ptr(self.lcgn.bias, "b")
        out = torch.empty((N, O), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            # call-invariant weight forms (stacked blocks, bf16 pieces): rebuilt only when a weight tensor was
            # replaced or modified in place (data_ptr / autograd version counter) or the mode changed
            key = (d.node_bf16, str(x.device)) + tuple((t.data_ptr(), t._version) for t in keep)
            if self._packed is None or self._packed_key != key:
                nbytes = lib.gvqa_lcgn_pack_bytes(C.byref(d))
                packed = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
                _lib.check(lib.gvqa_lcgn_pack_weights(C.byref(d), C.byref(p), packed.data_ptr(), nbytes, _stream(x.device)))
                self._packed, self._packed_key = packed, key
            p.packed, p.packed_bytes = self._packed.data_ptr(), self._packed.numel()
            ws = _workspace(lib.gvqa_lcgn_seq_workspace_bytes(C.byref(graph.c), C.byref(d)), x.device)
            _lib.check(lib.gvqa_lcgn_seq_forward(C.byref(graph.c), C.byref(d), C.byref(p), x.data_ptr(), q.data_ptr(),
                                                 lstm.data_ptr(), x_ctx_init.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), _stream(x.device)))
        return out
