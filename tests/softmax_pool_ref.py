"""References for the global attention pooling tests (CPU): the oracle's segment softmax and row scatter under torch autograd, in fp64 (the
reference) or fp32 (the composition whose own error the bounds are compared with)."""
import numpy as np
import torch

from oracle import ref_torch as R

# the shape matrix's batch: an empty graph in the middle, one-node graphs, 64 / 65 straddle a wave, 257 is one past a 256-thread block,
# 300 is more than one chunk of form 1
SHAPE_SIZES = [33, 1, 0, 300, 7, 128, 1, 64, 65, 257]


def batch_of(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def autograd_reference(score, x, batch, num_graphs, dout, dgate=None, dtype=torch.float64):
    """gate [N], out [B, C], dscore [N], dx [N, C] of oracle.ref_torch.segment_softmax + scatter_add_rows under torch autograd,
    loss = sum(out * dout) + sum(gate * dgate) (dgate None: the first term only).  numpy in, torch (dtype) out."""
    s = torch.from_numpy(np.ascontiguousarray(score)).to(dtype).reshape(-1, 1).requires_grad_(True)
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
    bt = torch.from_numpy(batch)
    gate = R.segment_softmax(s, bt, num_graphs)
    out = R.scatter_add_rows(gate * xt, bt, num_graphs)
    loss = (out * torch.from_numpy(np.ascontiguousarray(dout)).to(dtype)).sum()
    if dgate is not None:
        loss = loss + (gate * torch.from_numpy(np.ascontiguousarray(dgate)).to(dtype).reshape(-1, 1)).sum()
    loss.backward()
    return gate.detach().reshape(-1), out.detach(), s.grad.reshape(-1), xt.grad


def rel(a, b):
    """max-abs error relative to the largest reference magnitude."""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def maxabs(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max()) if a.numel() else 0.0
