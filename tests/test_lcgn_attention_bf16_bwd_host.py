"""CPU-only checks of the bf16 LCGN attention's training surface: gvqa_lcgn_attention_bf16_train /
gvqa_lcgn_attention_bf16_backward (+ _workspace_bytes) exist, are bound, and validate their arguments (status codes and messages,
nothing enqueued); the new kernels' compiled resources."""
import ctypes as C
import json
import os

from tests.test_lcgn_heads_host import _graph

NAMES = {"gvqa_lcgn_attention_bf16_train": 15, "gvqa_lcgn_attention_bf16_backward_workspace_bytes": 3,
         "gvqa_lcgn_attention_bf16_backward": 21}


def _lib_and_err():
    from graphvqa_amd import _lib
    lib = _lib.load()
    return _lib, lib, (lambda: lib.gvqa_last_error().decode())


def test_new_entry_points_are_exported_and_bound():
    _lib, lib, _ = _lib_and_err()
    raw = C.CDLL(lib._name)
    for name, nargs in NAMES.items():
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    assert lib.gvqa_lcgn_attention_bf16_backward_workspace_bytes.restype is C.c_size_t


def test_attention_bf16_train_rejects_bad_arguments_without_gpu():
    _lib, lib, err = _lib_and_err()
    E_INV, E_UNS = _lib.E_INVALID, _lib.E_UNSUPPORTED
    g = _graph()
    fake = 1 << 20                      # never dereferenced: the checks come first

    def att(g_, H, Cc, ldj=None, ldpc=None, ldo=None, J=None, pc=None, out=None, alpha=None, bias=None):
        return lib.gvqa_lcgn_attention_bf16_train(g_, H, Cc, 0, 0.2, J, 3 * H * Cc if ldj is None else ldj, pc,
                                                  2 * H * Cc if ldpc is None else ldpc, bias, None, out, Cc if ldo is None else ldo, alpha,
                                                  None)

    assert att(None, 2, 8) == E_INV and "lcgn_attention_bf16_train: null graph" in err()
    for H in (0, 9):
        assert att(C.byref(g), H, 8) == E_UNS and "heads" in err()
    assert att(C.byref(g), 2, 12) == E_UNS and "multiple of 8" in err()
    assert att(C.byref(g), 2, 6) == E_UNS
    assert att(C.byref(g), 1, 4104) == E_UNS and "4096" in err()          # heads * C = 4104
    assert att(C.byref(g), 3, 1368) == E_UNS and "4096" in err()          # 4104 again, over three heads
    assert att(C.byref(g), 2, 8, ldj=47) == E_INV and "leading dimensions" in err()
    assert att(C.byref(g), 2, 8, ldpc=31) == E_INV and "leading dimensions" in err()
    assert att(C.byref(g), 2, 8, ldo=4) == E_INV and "leading dimensions" in err()
    assert att(C.byref(_graph(finalized=0)), 2, 8) == E_INV and "finalized" in err()
    assert att(C.byref(g), 2, 8) == E_INV and "null tensor" in err()
    for kw in (dict(pc=fake, out=fake), dict(J=fake, out=fake), dict(J=fake, pc=fake)):
        assert att(C.byref(g), 2, 8, alpha=fake, **kw) == E_INV and "null tensor" in err(), kw
    assert att(C.byref(g), 2, 8, J=fake, pc=fake, out=fake) == E_INV and "alpha_out is required" in err()
    ops = dict(J=fake, pc=fake, out=fake, alpha=fake)
    assert att(C.byref(g), 2, 8, ldj=3 * 16 + 4, **ops) == E_UNS and "aligned" in err()       # a bf16 row of 52: 104 bytes
    assert att(C.byref(g), 2, 8, ldpc=2 * 16 + 2, **ops) == E_UNS and "aligned" in err()
    assert att(C.byref(g), 2, 8, ldo=10, **ops) == E_UNS and "aligned" in err()
    for kw in (dict(J=fake + 8), dict(pc=fake + 4), dict(out=fake + 4), dict(bias=fake + 4)):
        assert att(C.byref(g), 2, 8, **{**ops, **kw}) == E_UNS and "aligned" in err(), kw
    assert att(C.byref(_graph(nodes=0, edges=0)), 2, 8) == 0                     # an empty batch enqueues nothing


def test_attention_bf16_backward_rejects_bad_arguments_without_gpu():
    _lib, lib, err = _lib_and_err()
    E_INV, E_WS, E_UNS = _lib.E_INVALID, _lib.E_WORKSPACE, _lib.E_UNSUPPORTED
    g, gt = _graph(), _graph()
    wsb = lib.gvqa_lcgn_attention_bf16_backward_workspace_bytes
    need = wsb(C.byref(g), 2, 8)
    assert need >= 4 * (400 * 2 + 100 * 2 * 16)                  # dz [E, H] and the per-node rows [N, 2 H C]
    assert wsb(None, 2, 8) == 0
    assert wsb(C.byref(g), 9, 8) == 0 and wsb(C.byref(g), 0, 8) == 0
    assert wsb(C.byref(g), 2, 12) == 0 and wsb(C.byref(g), 2, 6) == 0
    assert wsb(C.byref(g), 1, 4104) == 0
    assert wsb(C.byref(g), 1, 4096) >= 4 * (400 + 100 * 2 * 4096)
    fake = 1 << 20

    def bwd(g_, gt_, H, Cc, ws_bytes=need, ws=fake, **kw):
        HC = H * Cc
        return lib.gvqa_lcgn_attention_bf16_backward(
            g_, gt_, H, Cc, 0, 0.2, kw.get("J"), kw.get("ldj", 3 * HC), kw.get("pc"), kw.get("ldpc", 2 * HC), kw.get("alpha"), None,
            kw.get("dout"), kw.get("ldd", Cc), kw.get("dJ"), kw.get("lddj", 3 * HC), kw.get("dpc"), kw.get("lddpc", 2 * HC), ws, ws_bytes,
            None)

    assert bwd(None, C.byref(gt), 2, 8) == E_INV and "lcgn_attention_bf16_backward: null graph" in err()
    assert bwd(C.byref(g), None, 2, 8) == E_INV and "null graph" in err()
    for H in (0, 9):
        assert bwd(C.byref(g), C.byref(gt), H, 8) == E_UNS and "heads" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 12) == E_UNS and "multiple of 8" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 6) == E_UNS
    assert bwd(C.byref(g), C.byref(gt), 1, 4104) == E_UNS and "4096" in err()
    assert bwd(C.byref(_graph(finalized=0)), C.byref(gt), 2, 8) == E_INV and "finalized" in err()
    assert bwd(C.byref(g), C.byref(_graph(finalized=0)), 2, 8) == E_INV and "finalized" in err()
    assert bwd(C.byref(g), C.byref(_graph(nodes=99)), 2, 8) == E_INV and "transposed graph" in err()
    assert bwd(C.byref(g), C.byref(_graph(edges=401)), 2, 8) == E_INV and "transposed graph" in err()
    for kw in (dict(ldj=47), dict(lddj=47), dict(ldpc=31), dict(lddpc=31), dict(ldd=4)):
        assert bwd(C.byref(g), C.byref(gt), 2, 8, **kw) == E_INV and "leading dimensions" in err(), kw
    assert bwd(C.byref(g), C.byref(gt), 2, 8, ws_bytes=need - 1) == E_WS and "workspace" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, ws=None) == E_WS and "workspace" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8) == E_INV and "null dpc" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, dpc=fake) == E_INV and "null tensor" in err()
    ops = dict(J=fake, pc=fake, dout=fake, dJ=fake, dpc=fake)
    for k in ("J", "pc", "dout", "dJ"):
        assert bwd(C.byref(g), C.byref(gt), 2, 8, alpha=fake, **{**ops, k: None}) == E_INV and "null tensor" in err(), k
    assert bwd(C.byref(g), C.byref(gt), 2, 8, **ops) == E_INV and "null alpha" in err()
    for kw in (dict(J=fake + 8), dict(pc=fake + 4), dict(dout=fake + 8), dict(dJ=fake + 4)):
        assert bwd(C.byref(g), C.byref(gt), 2, 8, alpha=fake, **{**ops, **kw}) == E_UNS and "aligned" in err(), kw
    for kw in (dict(ldj=3 * 16 + 4), dict(ldpc=2 * 16 + 2), dict(ldd=10), dict(lddj=3 * 16 + 2)):
        assert bwd(C.byref(g), C.byref(gt), 2, 8, alpha=fake, **ops, **kw) == E_UNS and "aligned" in err(), kw
    empty = _graph(nodes=0, edges=0, graphs=0)
    assert bwd(C.byref(empty), C.byref(empty), 2, 8, ws_bytes=0, ws=None) == 0    # an empty batch enqueues nothing


def test_bf16_training_kernels_have_no_scratch_and_no_spills():
    from graphvqa_amd import build
    lib = build.build()
    res = json.load(open(os.path.join(os.path.dirname(lib), "kernel_resources.json")))
    want = {"k_lcgn_att16_train": 8,        # chunks per lane {1, 2, 4, 8} x {intra, cross-graph}
            "k_lcgn_att16_bwd_dst": 4,      # chunks per lane {1, 2, 4, 8}
            "k_lcgn_att16_bwd_src": 1}
    for name, count in want.items():
        hits = {k: v for k, v in res.items() if name in k}
        assert len(hits) == count, (name, sorted(hits))
        for k, v in hits.items():
            assert "k_lcgn_attention_bf16" not in k
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
