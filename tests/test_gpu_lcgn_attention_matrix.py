"""GPU checks of the fp32 LCGN attention kernels (k_lcgn_attention, k_lcgn_att_bwd_dst, k_lcgn_att_bwd_src) over every chunk count
and both wave layouts their launchers can dispatch, on tests/lcgn_ref.py::hard_batch (in-degrees 0 .. 9, a destination with 301
in-edges whose head-0 logit ascends in CSR order, a source with 301 out-edges, repeated edges, a one-node graph, an empty graph in
the middle, with and without edges across graphs), against the dense fp64 form and autograd through it.

Bounds at the usual operand scale: those of tests/test_gpu_lcgn_attention_bwd.py (out 1e-5 x max(1, |ref|max), alpha 1e-5,
gradients GRAD_TOL under _grad_errors).  Large logits (max |z| = 500): 8 x the distance of the same dense form run in fp32 on the
CPU from fp64, never below the bounds above (the kernel sums in another order: a butterfly over lanes, CSR order over edges).
Leading dimensions: tests/test_gpu_lcgn_attention_ld.py."""
import pytest
import torch

from tests import lcgn_ref as L
from tests.lcgn_ref import GRAD_TOL, SLOPE

pytestmark = pytest.mark.gpu

CASES = L.with_concat(L.SHAPES + L.SHAPES_FP32_ODD)
BIG_CASES = L.with_concat(L.SHAPES_BIG)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(c, dev):
    from graphvqa_amd.graph import SceneGraphBatch
    return SceneGraphBatch(c["ei"].to(dev), c["batch"].to(dev), c["N"], c["B"])


def _gpu_run(c, graph, H, Cc, concat, dev):
    """lcgn_attention with gradients on the GPU, loss (out * w).sum(): (out, alpha, {dJ, dpc, dbias})."""
    from graphvqa_amd.lcgn import lcgn_attention
    ops = [c[k].detach().to(dev).requires_grad_(True) for k in ("J", "pc", "bias")]
    out, alpha = lcgn_attention(ops[0], ops[1], graph, H, Cc, concat, SLOPE, ops[2], want_alpha=True,
                                mask=None if c["mask"] is None else c["mask"].to(dev))
    assert out.requires_grad and not alpha.requires_grad
    (out * c["w"].to(dev)).sum().backward()
    return out.detach(), alpha, dict(zip(L.NAMES, (o.grad for o in ops)))


def _assert_exact_zeros(c, got, H, Cc):
    """What fp64 gives as an exact zero or an exact copy, the kernels give exactly: the node without in-edges gets the bias and no
    d x_r, the empty graph's dpc row is zero."""
    HC, info = H * Cc, c["info"]
    out, _, grads = got
    assert torch.equal(out[info["isolated"]].cpu(), c["bias"])
    assert float(grads["dJ"][info["isolated"], HC:2 * HC].abs().max()) == 0.0
    assert float(grads["dpc"][info["empty_graph"]].abs().max()) == 0.0
    assert int((grads["dpc"].abs().amax(dim=1) > 0).sum()) >= c["B"] - 2          # (the one-node graph's may be: its one edge masked)


def _inference_agrees(c, graph, got, H, Cc, concat, dev):
    """The inference kernel (no gradients, no mask), with and without alpha: bit for bit the training forward's out and alpha."""
    from graphvqa_amd.lcgn import lcgn_attention
    with torch.no_grad():
        J, pc, bias = (c[k].to(dev) for k in ("J", "pc", "bias"))
        out, alpha = lcgn_attention(J, pc, graph, H, Cc, concat, SLOPE, bias, want_alpha=True)
        plain, none = lcgn_attention(J, pc, graph, H, Cc, concat, SLOPE, bias)
    assert none is None and torch.equal(out, got[0]) and torch.equal(alpha, got[1]) and torch.equal(plain, out)


@pytest.mark.parametrize("H,Cc,concat", CASES)
def test_matrix_matches_fp64(dev, H, Cc, concat):
    for kind in (0, 1):
        graph = None
        for masked in (False, True):
            c = L.hard_case(H, Cc, concat, False, kind, False, masked)
            graph = graph or _graph(c, dev)
            assert bool(graph.c.intra_graph) == (kind == 0)
            ref = L.dense_reference(c, H, Cc, concat)
            got = _gpu_run(c, graph, H, Cc, concat, dev)
            d = L.distances(got, ref)
            print(f"H={H} C={Cc} concat={concat} kind={kind} masked={masked}: " + " ".join(f"{k} {v:.3g}" for k, v in d.items()))
            assert all(bool(torch.isfinite(v).all()) for v in (got[0], got[1], *got[2].values()))
            assert d["out"] < 1e-5 * max(1.0, float(ref[0].abs().max())), (kind, masked)
            assert d["alpha"] < 1e-5, (kind, masked)
            bad = {k: d[k] for k in L.NAMES if not d[k] < GRAD_TOL}
            assert not bad, (kind, masked, bad)
            _assert_exact_zeros(c, got, H, Cc)
            if not masked:
                _inference_agrees(c, graph, got, H, Cc, concat, dev)


@pytest.mark.parametrize("H,Cc,concat", BIG_CASES)
def test_large_logits_match_fp64(dev, H, Cc, concat):
    """max |z| = 500 (leaky logits -100 .. +500).  Measured on an MI355X, kernel / fp32 dense form on the CPU, worst of the four
    runs of a case: DESIGN.md section 4b, "LCGN attention: the test matrix"."""
    for kind in (0, 1):
        graph = None
        for masked in (False, True):
            c = L.hard_case(H, Cc, concat, False, kind, True, masked)
            graph = graph or _graph(c, dev)
            ref = L.dense_reference(c, H, Cc, concat)
            cpu = L.distances(L.dense_reference(c, H, Cc, concat, torch.float32), ref)
            got = _gpu_run(c, graph, H, Cc, concat, dev)
            assert all(bool(torch.isfinite(v).all()) for v in (got[0], got[1], *got[2].values())), (kind, masked)
            d = L.distances(got, ref)
            floor = dict(out=1e-5 * max(1.0, float(ref[0].abs().max())), alpha=1e-5, dJ=GRAD_TOL, dpc=GRAD_TOL, dbias=GRAD_TOL)
            print(f"big H={H} C={Cc} concat={concat} kind={kind} masked={masked}: " +
                  " ".join(f"{k} gpu {d[k]:.3g} cpu32 {cpu[k]:.3g}" for k in d))
            bad = {k: (d[k], cpu[k]) for k in d if not d[k] < max(8.0 * cpu[k], floor[k])}
            assert not bad, (kind, masked, bad)
            _assert_exact_zeros(c, got, H, Cc)
            if not masked:
                _inference_agrees(c, graph, got, H, Cc, concat, dev)
