"""References for the graph LayerNorm tests (CPU): the oracle's restatement under fp64 autograd, the closed-form backward the HIP kernels
implement, written out in fp64, and the fp32 composition (the oracle's op sequence in fp32) whose own error sets the offset test's bound."""
import numpy as np
import torch

from oracle import ref_torch as R

SHAPE_SIZES = [1, 6, 21, 40, 0, 129]          # the shape matrix's batch: a one-node graph, an empty graph in the middle, more than one row of 128


def batch_of(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def _scalar(v, dtype):
    return torch.tensor([1.0 if v is None else float(v)], dtype=dtype)


def autograd_reference(x, batch, num_graphs, weight, bias, dout, eps=1e-5, dtype=torch.float64):
    """out, dx, dweight, dbias of oracle.ref_torch.graph_layernorm under torch autograd, loss = sum(out * dout).  weight / bias: floats or
    None (1 / 0; their gradients are still returned).  numpy in, torch (dtype) out."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
    w = _scalar(weight, dtype).requires_grad_(True)
    b = torch.tensor([0.0 if bias is None else float(bias)], dtype=dtype, requires_grad=True)
    out = R.graph_layernorm(xt, torch.from_numpy(batch), num_graphs, w, b, eps)
    (out * torch.from_numpy(np.ascontiguousarray(dout)).to(dtype)).sum().backward()
    return out.detach(), xt.grad, w.grad, b.grad


def closed_form(x, batch, num_graphs, weight, bias, dout, eps=1e-5):
    """The same four results from the closed form (fp64), with the kernels' rule for sigma == 0: the variance term is dropped."""
    x, dout = torch.from_numpy(np.ascontiguousarray(x)).double(), torch.from_numpy(np.ascontiguousarray(dout)).double()
    w, b = (1.0 if weight is None else float(weight)), (0.0 if bias is None else float(bias))
    D = x.shape[1]
    out, dx = torch.zeros_like(x), torch.zeros_like(x)
    dw = db = 0.0
    for g in range(num_graphs):
        idx = torch.from_numpy(np.nonzero(batch == g)[0])
        if idx.numel() == 0:
            continue
        xs, gs = x[idx], dout[idx]
        M = xs.numel()
        xc = xs - xs.sum() / M
        sigma = float(torch.sqrt((xc * xc).sum() / M))
        y = xc / (sigma + eps)
        out[idx] = y * w + b
        gy = gs * w
        d = (gy - gy.sum() / M) / (sigma + eps)
        if sigma > 0:
            d = d - y * (gy * y).sum() / (M * sigma)
        dx[idx] = d
        dw += float((gs * y).sum())
        db += float(gs.sum())
    return out, dx, torch.tensor([dw], dtype=torch.float64), torch.tensor([db], dtype=torch.float64)


def fake_graph(nodes=100, edges=400, graphs=4, max_graph_nodes=30, finalized=1):
    """A gvqa_graph with hand-filled statistics and no device memory: enough for the host-side argument checks."""
    from graphvqa_amd import _lib
    g = _lib.Graph()
    g.num_nodes, g.num_edges, g.num_graphs = nodes, edges, graphs
    g.max_graph_nodes, g.max_graph_edges, g.max_in_degree = max_graph_nodes, 120, 8
    g.intra_graph, g.valid, g.finalized = 1, 1, finalized
    return g


def rel(a, b):
    """max-abs error relative to the largest reference magnitude."""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def maxabs(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max()) if a.numel() else 0.0
