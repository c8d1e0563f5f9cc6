"""GPU checks of the leading dimensions of the LCGN attention's C entry points, fp32 and bf16: gvqa_lcgn_attention[_bf16] (inference;
bf16 with fp32 and with bf16 output), gvqa_lcgn_attention[_bf16]_train with a mask, gvqa_lcgn_attention[_bf16]_backward, called
directly on J, pc, out, dout, dJ and dpc as column blocks of wider buffers.  The six leading dimensions differ from the widths and
from each other (multiples of 4, of 8 for bf16 rows; every block 16-byte aligned), and from the 2 H C stride of the backward's
per-node workspace rows.  Inputs are surrounded by NaN (a read outside a block poisons the result), outputs by a sentinel that
must survive, alpha and the workspace carry guards; every result is bit-identical to the same call on contiguous tensors.  Batch
and operands: tests/lcgn_ref.py::hard_batch, both edge lists."""
import ctypes as C

import pytest
import torch

from tests import lcgn_ref as L
from tests.lcgn_ref import SLOPE

pytestmark = pytest.mark.gpu

SENTINEL = -776.0               # (exact in bf16)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _written(*tensors):
    return all(bool(torch.isfinite(v.float()).all()) and not bool((v == SENTINEL).any()) for v in tensors)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("H,Cc,concat", [(5, 40, False), (5, 40, True), (4, 256, False), (4, 256, True)])
def test_entry_points_respect_every_leading_dimension(dev, H, Cc, concat, bf16):
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import SceneGraphBatch, _stream
    lib = _lib.load()
    sfx = "_bf16" if bf16 else ""
    infer, train_fn = getattr(lib, "gvqa_lcgn_attention" + sfx), getattr(lib, f"gvqa_lcgn_attention{sfx}_train")
    bwd_fn, ws_fn = getattr(lib, f"gvqa_lcgn_attention{sfx}_backward"), getattr(lib, f"gvqa_lcgn_attention{sfx}_backward_workspace_bytes")
    jdtype = torch.bfloat16 if bf16 else torch.float32
    HC = H * Cc
    cout = HC if concat else Cc
    for kind in (0, 1):
        c = L.hard_case(H, Cc, concat, bf16, kind, False, True)
        graph = SceneGraphBatch(c["ei"].to(dev), c["batch"].to(dev), c["N"], c["B"])
        gt = graph.transposed()
        N, B, E = c["N"], c["B"], graph.num_edges
        J, pc, bias, mask, dout = (c[k].to(dev) for k in ("J", "pc", "bias", "mask", "w"))
        J = J.to(jdtype)                                     # (bf16: the values are bf16 values already)
        Jb, Jv, ldJ = L.column_block(N, 3 * HC, 8, 8, NAN, dev, jdtype)
        pb, pv, ldpc = L.column_block(B, 2 * HC, 4, 8, NAN, dev)
        db, dv, lddo = L.column_block(N, cout, 12, 16, NAN, dev)
        Jv.copy_(J); pv.copy_(pc); dv.copy_(dout)
        lds = {"J": ldJ, "pc": ldpc, "dout": lddo, "out": 8 + cout + 24, "dJ": 4 + 3 * HC + 20, "dpc": 8 + 2 * HC + 12}
        assert len(set(lds.values())) == 6 and not set(lds.values()) & {3 * HC, 2 * HC, cout}
        assert all(v % 4 == 0 for v in lds.values()) and lds["J"] % 8 == 0 and lds["out"] % 8 == 0
        assert all(v.data_ptr() % 16 == 0 for v in (Jv, pv, dv))
        G = 3                                                # guard rows of alpha
        ws_bytes = ws_fn(C.byref(graph.c), H, Cc)
        assert ws_bytes > 0

        def forward(how, strided):
            odtype = torch.bfloat16 if how == "infer16" else torch.float32
            ob, ov, ldo = (L.column_block(N, cout, 8, 24, SENTINEL, dev, odtype) if strided else
                           L.column_block(N, cout, 0, 0, SENTINEL, dev, odtype, guard_rows=0))
            ab = torch.full((E + 2 * G, H), SENTINEL, device=dev)
            head = (C.byref(graph.c), H, Cc, int(concat), SLOPE) + ((Jv.data_ptr(), ldJ, pv.data_ptr(), ldpc) if strided else
                                                                    (J.data_ptr(), 3 * HC, pc.data_ptr(), 2 * HC))
            if how == "train":
                rc = train_fn(*head, bias.data_ptr(), mask.data_ptr(), ov.data_ptr(), ldo, ab[G:].data_ptr(), _stream(dev))
            elif bf16:
                rc = infer(*head, bias.data_ptr(), ov.data_ptr(), ldo, int(how == "infer16"), ab[G:].data_ptr(), _stream(dev))
            else:
                rc = infer(*head, bias.data_ptr(), ov.data_ptr(), ldo, ab[G:].data_ptr(), _stream(dev))
            _lib.check(rc)
            torch.cuda.synchronize()
            assert ldo == (lds["out"] if strided else cout) and ov.data_ptr() % 16 == 0
            assert L.untouched(ob, ov, SENTINEL) and bool((ab[:G] == SENTINEL).all()) and bool((ab[G + E:] == SENTINEL).all())
            return ov, ab[G:G + E]

        def backward(alpha, strided):
            jb, jv, lddj = (L.column_block(N, 3 * HC, 4, 20, SENTINEL, dev) if strided else
                            L.column_block(N, 3 * HC, 0, 0, SENTINEL, dev, guard_rows=0))
            qb, qv, lddp = (L.column_block(B, 2 * HC, 8, 12, SENTINEL, dev) if strided else
                            L.column_block(B, 2 * HC, 0, 0, SENTINEL, dev, guard_rows=0))
            ws = torch.full((ws_bytes + 256,), 0x5A, dtype=torch.uint8, device=dev)
            a = (Jv, ldJ, pv, ldpc, dv, lddo) if strided else (J, 3 * HC, pc, 2 * HC, dout, cout)
            _lib.check(bwd_fn(C.byref(graph.c), C.byref(gt.c), H, Cc, int(concat), SLOPE, a[0].data_ptr(), a[1], a[2].data_ptr(), a[3],
                              alpha.data_ptr(), mask.data_ptr(), a[4].data_ptr(), a[5], jv.data_ptr(), lddj, qv.data_ptr(), lddp,
                              ws.data_ptr(), ws_bytes, _stream(dev)))
            torch.cuda.synchronize()
            assert (lddj, lddp) == ((lds["dJ"], lds["dpc"]) if strided else (3 * HC, 2 * HC)) and jv.data_ptr() % 16 == 0
            assert L.untouched(jb, jv, SENTINEL) and L.untouched(qb, qv, SENTINEL) and bool((ws[ws_bytes:] == 0x5A).all())
            return jv, qv

        for how in ("infer", "infer16", "train") if bf16 else ("infer", "train"):
            (o1, a1), (o0, a0) = forward(how, True), forward(how, False)
            assert _written(o0, a0), (kind, how)
            assert torch.equal(o1, o0) and torch.equal(a1, a0), (kind, how)
        alpha = a0.contiguous()                              # of the masked training forward
        (dJ1, dpc1), (dJ0, dpc0) = backward(alpha, True), backward(alpha, False)
        assert _written(dJ0, dpc0) and float(dJ0.abs().max()) > 0 and float(dpc0.abs().max()) > 0, kind
        assert torch.equal(dJ1, dJ0) and torch.equal(dpc1, dpc0), kind
        assert float(dpc0[c["info"]["empty_graph"]].abs().max()) == 0.0
        assert L.untouched(Jb, Jv, NAN) and L.untouched(pb, pv, NAN) and L.untouched(db, dv, NAN)
