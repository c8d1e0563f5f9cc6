"""GPU checks of the bf16 LCGN attention kernels (k_lcgn_attention_bf16 with fp32 and bf16 output, k_lcgn_att16_train,
k_lcgn_att16_bwd_dst, k_lcgn_att16_bwd_src) over every chunk count and both wave layouts their launchers can dispatch: the matrix
of tests/test_gpu_lcgn_attention_matrix.py on the same batch (tests/lcgn_ref.py::hard_batch), J rounded to bf16 before both sides
see it, against the dense fp64 form on J.bfloat16().double() and autograd through it.

Bounds: the fp32 matrix's (the kernels do fp32 arithmetic on values that are exact in fp32), large logits included; the bf16
output: those of tests/test_gpu_lcgn_heads_bf16.py::test_bf16_attention_kernel_matches_the_fp32_kernel (within 2^-8 (|ref|max + 1),
more than 99 % of the elements the reference's own rounding)."""
import pytest
import torch

from tests import lcgn_ref as L
from tests.lcgn_ref import GRAD_TOL, SLOPE
from tests.util import maxabs

pytestmark = pytest.mark.gpu

CASES = L.with_concat(L.SHAPES)
BIG_CASES = L.with_concat(L.SHAPES_BIG)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(c, dev):
    from graphvqa_amd.graph import SceneGraphBatch
    return SceneGraphBatch(c["ei"].to(dev), c["batch"].to(dev), c["N"], c["B"])


def _gpu_run(c, graph, H, Cc, concat, dev):
    """The bf16 attention node on an fp32 J that holds bf16 values (rounded inside: the same values; dJ stays fp32), loss
    (out * w).sum(): (out, alpha, {dJ, dpc, dbias})."""
    from graphvqa_amd.lcgn import _lcgn_attention_store_bf16
    ops = [c[k].detach().to(dev).requires_grad_(True) for k in ("J", "pc", "bias")]
    out, alpha = _lcgn_attention_store_bf16(ops[0], ops[1], graph, H, Cc, concat, SLOPE, ops[2],
                                            None if c["mask"] is None else c["mask"].to(dev))
    assert out.requires_grad and not alpha.requires_grad and out.dtype == torch.float32
    (out * c["w"].to(dev)).sum().backward()
    assert ops[0].grad.dtype == torch.float32
    return out.detach(), alpha, dict(zip(L.NAMES, (o.grad for o in ops)))


def _assert_exact_zeros(c, got, H, Cc):
    HC, info = H * Cc, c["info"]
    out, _, grads = got
    assert torch.equal(out[info["isolated"]].cpu(), c["bias"])
    assert float(grads["dJ"][info["isolated"], HC:2 * HC].abs().max()) == 0.0
    assert float(grads["dpc"][info["empty_graph"]].abs().max()) == 0.0
    assert int((grads["dpc"].abs().amax(dim=1) > 0).sum()) >= c["B"] - 2          # (the one-node graph's may be: its one edge masked)


def _inference_agrees(c, graph, got, ref, H, Cc, concat, dev, rounding=True):
    """The inference kernel (no gradients, no mask).  fp32 output, with and without alpha: bit for bit the training forward's (it
    is that launch).  bf16 output: the bounds of test_bf16_attention_kernel_matches_the_fp32_kernel, against the fp64 form
    (rounding: the share of elements that are the reference's own rounding is held at the usual operand scale only, where fp32's
    error is far below half a bf16 step; it is printed either way)."""
    from graphvqa_amd.lcgn import lcgn_attention_bf16
    with torch.no_grad():
        J16, pc, bias = c["J"].to(dev).bfloat16(), c["pc"].to(dev), c["bias"].to(dev)
        assert torch.equal(J16.float().cpu(), c["J"])
        o32, a32 = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, SLOPE, bias, want_alpha=True, out_dtype=torch.float32)
        p32, none = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, SLOPE, bias, out_dtype=torch.float32)
        o16, a16 = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, SLOPE, bias, want_alpha=True)
        p16, _ = lcgn_attention_bf16(J16, pc, graph, H, Cc, concat, SLOPE, bias)
    assert none is None and o32.dtype == torch.float32 and o16.dtype == torch.bfloat16
    assert torch.equal(o32, got[0]) and torch.equal(a32, got[1]) and torch.equal(p32, o32)
    assert torch.equal(a16, a32) and torch.equal(p16, o16)
    rmax = float(ref[0].abs().max())
    same = float((o16.float().cpu() == ref[0].float().bfloat16().float()).float().mean())
    print(f"    bf16 out: {maxabs(o16.float(), ref[0]):.3g} (|ref| {rmax:.3g}), the reference's rounding on {same:.5f}")
    assert maxabs(o16.float(), ref[0]) < 2.0 ** -8 * (rmax + 1.0)
    assert same > 0.99 or not rounding


@pytest.mark.parametrize("H,Cc,concat", CASES)
def test_matrix_matches_fp64(dev, H, Cc, concat):
    for kind in (0, 1):
        graph = None
        for masked in (False, True):
            c = L.hard_case(H, Cc, concat, True, kind, False, masked)
            graph = graph or _graph(c, dev)
            assert bool(graph.c.intra_graph) == (kind == 0)
            ref = L.dense_reference(c, H, Cc, concat)
            got = _gpu_run(c, graph, H, Cc, concat, dev)
            d = L.distances(got, ref)
            print(f"bf16 H={H} C={Cc} concat={concat} kind={kind} masked={masked}: " + " ".join(f"{k} {v:.3g}" for k, v in d.items()))
            assert all(bool(torch.isfinite(v).all()) for v in (got[0], got[1], *got[2].values()))
            assert d["out"] < 1e-5 * max(1.0, float(ref[0].abs().max())), (kind, masked)
            assert d["alpha"] < 1e-5, (kind, masked)
            bad = {k: d[k] for k in L.NAMES if not d[k] < GRAD_TOL}
            assert not bad, (kind, masked, bad)
            _assert_exact_zeros(c, got, H, Cc)
            if not masked:
                _inference_agrees(c, graph, got, ref, H, Cc, concat, dev)


@pytest.mark.parametrize("H,Cc,concat", BIG_CASES)
def test_large_logits_match_fp64(dev, H, Cc, concat):
    """max |z| = 500 (leaky logits -100 .. +500) on a J rounded to bf16 after the rescaling.  Bound: 8 x the distance of the dense form
    run in fp32 on the CPU from fp64, never below the matrix's bounds.  Measured on an MI355X, kernel / fp32 dense form on the CPU:
    DESIGN.md section 4b, "LCGN attention: the test matrix"."""
    for kind in (0, 1):
        graph = None
        for masked in (False, True):
            c = L.hard_case(H, Cc, concat, True, kind, True, masked)
            graph = graph or _graph(c, dev)
            ref = L.dense_reference(c, H, Cc, concat)
            cpu = L.distances(L.dense_reference(c, H, Cc, concat, torch.float32), ref)
            got = _gpu_run(c, graph, H, Cc, concat, dev)
            assert all(bool(torch.isfinite(v).all()) for v in (got[0], got[1], *got[2].values())), (kind, masked)
            d = L.distances(got, ref)
            floor = dict(out=1e-5 * max(1.0, float(ref[0].abs().max())), alpha=1e-5, dJ=GRAD_TOL, dpc=GRAD_TOL, dbias=GRAD_TOL)
            print(f"big bf16 H={H} C={Cc} concat={concat} kind={kind} masked={masked}: " +
                  " ".join(f"{k} gpu {d[k]:.3g} cpu32 {cpu[k]:.3g}" for k in d))
            bad = {k: (d[k], cpu[k]) for k in d if not d[k] < max(8.0 * cpu[k], floor[k])}
            assert not bad, (kind, masked, bad)
            _assert_exact_zeros(c, got, H, Cc)
            if not masked:
                _inference_agrees(c, graph, got, ref, H, Cc, concat, dev, rounding=False)
