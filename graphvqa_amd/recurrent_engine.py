"""MI355X-native counterpart of the reference's `RecurrentExecutionEngine` (pipeline_model_gat.py:194-288): five instruction-conditioned
steps of a node cell over the scene graph, a graph LayerNorm, and a softmax "bitmap" over each graph's nodes that pools the history vector
of the next step.

`neighbor_mean` is the differentiable op under the cell: `scatter_mean(m[row], col, dim_size=N)` for a per-node `m` as one CSR gather-reduce
forward and one backward (csrc/neighbor_mean.hip), no `[E, F]` tensor.  `RecurrentExecutionEngine` keeps the reference's constructor,
attribute names and state_dict; its forward is one formulation for eval and training (the same kernels under `no_grad`):

  * the cell's first MLP acts on `[x[row] | h[batch[row]]]`, which depends on the SOURCE node only, so it is applied per node,
    `m = Lin2(relu(x Wa^T + (h Wb^T + b)[batch]))`, and the reference's `scatter_mean(mlp(...), col)` is `neighbor_mean(m, graph)`;
  * `x` is the same in every step (the reference never feeds a step's output to the next), so the two column blocks that act on it,
    `node_mlp_1[0].weight[:, :D]` and `node_mlp_2[0].weight[:, :D]`, are ONE `[N, D] x [D, 2D]` product per forward;
  * the instruction block of `node_mlp_2[0]` is one `[5B, Di]` product for all steps, broadcast to the nodes per step.

Node-sized products run on the library's GEMMs (`_ProjectionLinear`), the `D -> 1` gate on the tall-skinny kernels, LayerNorm and the
softmax pooling on their fused ops.  The output keeps `B = instr_vectors.shape[1]` history rows per step -- zero rows for graphs without
nodes -- where the reference's `dim_size=None` would drop TRAILING empty graphs.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable
from torch.nn import Linear as Lin, ReLU, Sequential as Seq

from . import _lib
from .gat_skip import _ProjectionLinear, add_graph_rows, edge_gather, edge_scatter_add, graph_rows, skinny_linear
from .global_attention import graph_attention_pool
from .graph import SceneGraphBatch, _stream
from .graph_layernorm import LayerNorm, _rows

MAX_EXECUTION_STEP = 5          # GQATorchDataset.MAX_EXECUTION_STEP (gqa_dataset_entry.py)
_FORCE_COMPOSED_MEAN = False    # tests and scripts/bench_recurrent_engine.py only: the mean by edge_gather + edge_scatter_add / bincount


class _NeighborMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph):
        lib = _lib.load()
        x = _rows(x, "x")
        N, F = x.shape
        out = torch.empty((N, F), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.gvqa_graph_neighbor_mean_forward(C.byref(graph.c), F, x.data_ptr(), x.stride(0) if N > 1 else F, out.data_ptr(), F,
                                                            _stream(x.device)))
        ctx.graph = graph
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        graph = ctx.graph
        dout = _rows(dout, "dout")
        N, F = dout.shape
        gt = graph.transposed()                    # (built on the first backward of this batch, cached on the handle)
        dx = torch.empty((N, F), dtype=torch.float32, device=dout.device)
        with torch.cuda.device(dout.device):
            _lib.check(lib.gvqa_graph_neighbor_mean_backward(C.byref(graph.c), C.byref(gt.c), F, dout.data_ptr(), dout.stride(0) if N > 1 else F,
                                                             dx.data_ptr(), F, _stream(dout.device)))
        return dx, None


def neighbor_mean(x: Tensor, graph: SceneGraphBatch) -> Tensor:
    """out[i] = the mean of x[j] over the in-edges (j -> i) of node i (torch_scatter.scatter_mean(x[row], col, dim_size=N): a zero row for a
    node without in-edges, a multi-edge counts once per occurrence, self-loops are ordinary edges).  x: fp32 [N, F] on the GPU; a column block
    of a wider tensor is read in place.  Differentiable in x (first order); the transposed CSR is built only when a gradient is asked for."""
    if x.dim() != 2 or x.shape[0] != graph.num_nodes:
        raise ValueError("neighbor_mean: x must be [N, F] with N = graph.num_nodes")
    if x.shape[1] < 1:
        raise ValueError("neighbor_mean: x needs at least one channel")
    return _NeighborMeanFn.apply(x, graph)


def _composed_mean(m: Tensor, graph: SceneGraphBatch, cnt: Tensor) -> Tensor:
    return edge_scatter_add(edge_gather(m, graph, "src"), graph) / cnt


class _NodeModel(torch.nn.Module):
    def __init__(self, d, di):
        super().__init__()
        self.node_mlp_1 = Seq(Lin(2 * d, d), ReLU(), Lin(d, d))
        self.node_mlp_2 = Seq(Lin(2 * d + di, d), ReLU(), Lin(d, d))


class _GlobalModel(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.node_mlp_1 = Seq(Lin(d, d), ReLU(), Lin(d, 1))


class RecurrentExecutionEngine(torch.nn.Module):
    """pipeline_model_gat.py:194-288.  `dropout` is unused, as in the reference."""

    def __init__(self, num_node_features, num_instr_features, dropout=0.1):
        super().__init__()
        _lib.load()
        self.num_node_features = num_node_features
        self.num_instr_features = num_instr_features
        self.engine_one_step_execution_cell = _NodeModel(num_node_features, num_instr_features)
        self.graph_layer_norm = LayerNorm(num_node_features)
        self.softmax_bitmap_predictor = _GlobalModel(num_node_features)
        self.history_vectors_mlp = Seq(Lin(num_node_features, num_instr_features), ReLU(), Lin(num_instr_features, num_instr_features))

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr, instr_vectors: Tensor, batch: Tensor, graph: SceneGraphBatch | None = None):
        """x [N, D], edge_index [2, E], instr_vectors [>= 5, B, Di], batch [N]; edge_attr is ignored (the reference never reads it) and may
        be None.  graph: a prebuilt SceneGraphBatch of (edge_index, batch) with B graphs.  Returns (x as passed in, execution_bitmap [N, 5],
        history_vectors [5, B, Di])."""
        D, Di, K = self.num_node_features, self.num_instr_features, MAX_EXECUTION_STEP
        for name, v in (("x", x), ("instr_vectors", instr_vectors)):
            if not v.is_cuda:
                raise RuntimeError(f"{name} is on {v.device}: the MI355X execution path has no CPU fallback")
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"RecurrentExecutionEngine: x must be [N, {D}] (got {tuple(x.shape)})")
        if instr_vectors.dim() != 3 or instr_vectors.shape[2] != Di:
            raise ValueError(f"RecurrentExecutionEngine: instr_vectors must be [steps, B, {Di}] (got {tuple(instr_vectors.shape)})")
        if instr_vectors.shape[0] < K:
            raise ValueError(f"RecurrentExecutionEngine: {K} execution steps need {K} instruction vectors (got {instr_vectors.shape[0]})")
        N, B = x.shape[0], instr_vectors.shape[1]
        if graph is None:
            graph = SceneGraphBatch(edge_index, batch, N, B)
        elif graph.num_nodes != N or graph.num_graphs != B:
            raise ValueError("RecurrentExecutionEngine: graph does not match x / instr_vectors")
        proj = _ProjectionLinear.apply
        cell, pred, ln = self.engine_one_step_execution_cell, self.softmax_bitmap_predictor.node_mlp_1, self.graph_layer_norm
        a0, a2, b0, b2 = cell.node_mlp_1[0], cell.node_mlp_1[2], cell.node_mlp_2[0], cell.node_mlp_2[2]
        # what does not change across the steps: both x column blocks as one product, the instruction block for all steps as one product
        xa, xt = proj(x, torch.cat((a0.weight[:, :D], b0.weight[:, :D]), 0), None).split(D, 1)
        ui = proj(instr_vectors[:K].reshape(K * B, Di), b0.weight[:, 2 * D:], b0.bias)
        cnt = None
        if _FORCE_COMPOSED_MEAN:
            cnt = torch.bincount(graph._keep[0][1], minlength=N).clamp(min=1).to(x.dtype).view(-1, 1)
        h = torch.zeros((B, D), dtype=torch.float32, device=x.device)
        bitmaps, hist = [], []
        for k in range(K):
            # NodeModel :250-259
            m = proj(torch.relu(xa + graph_rows(proj(h, a0.weight[:, D:], a0.bias), graph)), a2.weight, a2.bias)
            agg = _composed_mean(m, graph, cnt) if _FORCE_COMPOSED_MEAN else neighbor_mean(m, graph)
            z = add_graph_rows(proj(agg, b0.weight[:, D:2 * D], None), ui[k * B:(k + 1) * B], graph)
            xo = proj(torch.relu(z + xt), b2.weight, b2.bias) + x
            xo = ln(xo, batch, graph=graph)                                                      # :220
            # GlobalModel :279-286
            score = skinny_linear(torch.relu(proj(xo, pred[0].weight, pred[0].bias)), pred[2].weight.t()) + pred[2].bias
            h, gate = graph_attention_pool(score, xo, graph, return_gate=True)
            bitmaps.append(gate)
            hist.append(h)
        hm = self.history_vectors_mlp
        hv = proj(torch.relu(proj(torch.cat(hist, 0), hm[0].weight, hm[0].bias)), hm[2].weight, hm[2].bias)
        return x, torch.cat(bitmaps, dim=1), hv.view(K, B, Di)
