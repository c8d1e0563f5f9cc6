"""References for the RecurrentExecutionEngine tests (CPU): the neighbour mean and the whole module restated in plain torch -- indexing and
index_add_, the reference's own per-EDGE formulation (pipeline_model_gat.py:211-286), nothing from graphvqa_amd -- run in fp64 under torch
autograd (or in any other dtype)."""
import numpy as np
import torch

STEPS = 5
CELL, PRED, HIST = "engine_one_step_execution_cell.", "softmax_bitmap_predictor.", "history_vectors_mlp."


def tt(a, dtype=torch.float64):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.to(dtype) if x.is_floating_point() else x


def rows_sum(v, index, n):
    """out[k] = sum of v[e] over the e with index[e] == k (torch_scatter.scatter_add along dim 0)."""
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype).index_add_(0, index, v)


def neighbor_mean(x, edge_index, num_nodes):
    """torch_scatter.scatter_mean(x[row], col, dim=0, dim_size=N): the sum over the in-edges divided by max(in-degree, 1)."""
    row, col = edge_index[0], edge_index[1]
    cnt = rows_sum(torch.ones(col.shape[0], dtype=x.dtype), col, num_nodes).clamp(min=1)
    return rows_sum(x[row], col, num_nodes) / cnt.view(-1, 1)


def neighbor_mean_autograd(x, edge_index, dout, dtype=torch.float64):
    """out and dx of the op for loss = sum(out * dout).  numpy in, torch out."""
    xt = tt(x, dtype).requires_grad_(True)
    out = neighbor_mean(xt, tt(edge_index), x.shape[0])
    (out * tt(dout, dtype)).sum().backward()
    return out.detach(), xt.grad


def graph_layernorm(x, batch, num_graphs, weight, bias, eps=1e-5):
    """graph_utils/my_graph_layernorm.py:52-78: statistics per graph over nodes x channels, eps outside the square root."""
    norm = (rows_sum(torch.ones(batch.shape[0], dtype=x.dtype), batch, num_graphs).clamp(min=1) * x.shape[1]).view(-1, 1)
    mean = rows_sum(x, batch, num_graphs).sum(-1, keepdim=True) / norm
    xc = x - mean[batch]
    var = rows_sum(xc * xc, batch, num_graphs).sum(-1, keepdim=True) / norm
    return xc / (var.sqrt()[batch] + eps) * weight + bias


def graph_softmax(score, batch, num_graphs):
    """torch_geometric.utils.softmax: max-shifted per graph, denominator + 1e-16."""
    idx = batch.view(-1, 1).expand_as(score)
    mx = torch.full((num_graphs, score.shape[1]), float("-inf"), dtype=score.dtype).scatter_reduce(0, idx, score.detach(), reduce="amax")
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    ex = (score - mx[batch]).exp()
    return ex / (rows_sum(ex, batch, num_graphs)[batch] + 1e-16)


def _mlp(p, prefix, v):
    h = torch.relu(v @ p[prefix + "0.weight"].t() + p[prefix + "0.bias"])
    return h @ p[prefix + "2.weight"].t() + p[prefix + "2.bias"]


def engine(x, edge_index, instr_vectors, batch, p, num_graphs, ln_steps=None):
    """RecurrentExecutionEngine.forward as written in the reference: the per-edge concatenation, scatter_mean by destination, the residual,
    the graph LayerNorm, the softmax bitmap and its pooled history vector -- B = num_graphs history rows.  p: {state_dict key: tensor}.
    Returns (execution_bitmap [N, 5], history_vectors [5, B, Di]); ln_steps (a list) receives the per-step LayerNorm outputs."""
    row, col = edge_index[0], edge_index[1]
    N, D = x.shape
    h = torch.zeros((num_graphs, D), dtype=x.dtype)
    bitmaps, hist = [], []
    for k in range(STEPS):
        u = instr_vectors[k]
        out = _mlp(p, CELL + "node_mlp_1.", torch.cat([x[row], h[batch[row]]], dim=1))
        cnt = rows_sum(torch.ones(col.shape[0], dtype=x.dtype), col, N).clamp(min=1)
        out = rows_sum(out, col, N) / cnt.view(-1, 1)
        xo = _mlp(p, CELL + "node_mlp_2.", torch.cat([x, out, u[batch]], dim=1)) + x
        xo = graph_layernorm(xo, batch, num_graphs, p["graph_layer_norm.weight"], p["graph_layer_norm.bias"])
        if ln_steps is not None:
            ln_steps.append(xo)
        gate = graph_softmax(_mlp(p, PRED + "node_mlp_1.", xo), batch, num_graphs)
        h = rows_sum(gate * xo, batch, num_graphs)
        bitmaps.append(gate)
        hist.append(h)
    return torch.cat(bitmaps, dim=1), _mlp(p, HIST, torch.stack(hist, dim=0))


def engine_autograd(x, edge_index, instr_vectors, batch, params, num_graphs, dB, dH, dtype=torch.float64):
    """Outputs and every gradient for loss = sum(bitmap * dB) + sum(history_vectors * dH).  numpy in; returns
    dict(execution_bitmap, history_vectors, ln_steps [5, N, D], d_x, d_instr_vectors, d_<parameter key> ...) of torch tensors."""
    p = {k: tt(v, dtype).requires_grad_(True) for k, v in params.items()}
    xt, it = tt(x, dtype).requires_grad_(True), tt(instr_vectors, dtype).requires_grad_(True)
    ln = []
    bitmap, hv = engine(xt, tt(edge_index), it, tt(batch), p, num_graphs, ln)
    ((bitmap * tt(dB, dtype)).sum() + (hv * tt(dH, dtype)).sum()).backward()
    res = dict(execution_bitmap=bitmap.detach(), history_vectors=hv.detach(), ln_steps=torch.stack([v.detach() for v in ln]), d_x=xt.grad,
               d_instr_vectors=it.grad)
    res.update({"d_" + k: v.grad for k, v in p.items()})
    return res


def fixture_params(g):
    return {k[2:]: v for k, v in g.items() if k.startswith("p_")}


def maxabs(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max()) if a.numel() else 0.0


def rel(a, b, floor=0.0):
    """max-abs error relative to the reference's largest magnitude (`floor`: the scale below which a gradient counts as zero)."""
    b = torch.as_tensor(b).detach().cpu().double()
    return maxabs(a, b) / max(float(b.abs().max()) if b.numel() else 0.0, floor, 1e-12)
