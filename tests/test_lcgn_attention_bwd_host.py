"""CPU-only checks of the LCGN attention's training surface: gvqa_lcgn_attention_train / gvqa_lcgn_attention_backward exist and
validate their arguments (status codes and messages, nothing enqueued), and the recorded reference gradients
(tests/golden/lcgn_heads_grads.npz) are what fp64 autograd through the oracle gives."""
import ctypes as C

import pytest
import torch

from graphvqa_amd import synth
from tests.test_lcgn_heads_host import _graph, _layer_oracle
from tests.util import load_golden, t, tparams, maxabs

PARAMS = ("lin_l.weight", "lin_r.weight", "cal_x.weight", "proj_cmd.weight", "cal_cmd.weight", "bias")


def _lib_and_err():
    from graphvqa_amd import _lib
    lib = _lib.load()
    return _lib, lib, (lambda: lib.gvqa_last_error().decode())


def test_new_entry_points_are_exported_and_bound():
    _lib, lib, _ = _lib_and_err()
    raw = C.CDLL(lib._name)
    for name in ("gvqa_lcgn_attention_train", "gvqa_lcgn_attention_backward_workspace_bytes", "gvqa_lcgn_attention_backward"):
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == {"gvqa_lcgn_attention_train": 15,
                                                                "gvqa_lcgn_attention_backward_workspace_bytes": 3,
                                                                "gvqa_lcgn_attention_backward": 21}[name]
    assert lib.gvqa_lcgn_attention_backward_workspace_bytes.restype is C.c_size_t


def test_attention_train_rejects_bad_arguments_without_gpu():
    _lib, lib, err = _lib_and_err()
    E_INV, E_UNS = _lib.E_INVALID, _lib.E_UNSUPPORTED
    g = _graph()
    att = lambda g_, H, Cc, ldj=None, ldpc=None, ldo=None, J=None, pc=None, out=None, alpha=None: lib.gvqa_lcgn_attention_train(
        g_, H, Cc, 0, 0.2, J, 3 * H * Cc if ldj is None else ldj, pc, 2 * H * Cc if ldpc is None else ldpc, None, None, out,
        Cc if ldo is None else ldo, alpha, None)
    assert att(None, 2, 8) == E_INV and "lcgn_attention_train: null graph" in err()
    for H in (0, 9):
        assert att(C.byref(g), H, 8) == E_UNS and "heads" in err()
    assert att(C.byref(g), 2, 6) == E_UNS and "multiple of 4" in err()
    assert att(C.byref(g), 4, 1028) == E_UNS and "4096" in err()
    assert att(C.byref(g), 2, 8, ldj=47) == E_INV and "leading dimensions" in err()
    assert att(C.byref(g), 2, 8, ldo=4) == E_INV and "leading dimensions" in err()
    assert att(C.byref(_graph(finalized=0)), 2, 8) == E_INV and "finalized" in err()
    assert att(C.byref(g), 2, 8) == E_INV and "null tensor" in err()
    fake = 1 << 20                      # never dereferenced: the checks come first
    assert att(C.byref(g), 2, 8, J=fake, pc=fake, out=fake) == E_INV and "alpha_out is required" in err()
    assert att(C.byref(g), 2, 8, J=fake + 4, pc=fake, out=fake, alpha=fake) == E_UNS and "aligned" in err()
    assert att(C.byref(g), 2, 8, ldj=50, J=fake, pc=fake, out=fake, alpha=fake) == E_UNS and "aligned" in err()
    assert att(C.byref(_graph(nodes=0, edges=0)), 2, 8) == 0                     # an empty batch enqueues nothing


def test_attention_backward_rejects_bad_arguments_without_gpu():
    _lib, lib, err = _lib_and_err()
    E_INV, E_WS, E_UNS = _lib.E_INVALID, _lib.E_WORKSPACE, _lib.E_UNSUPPORTED
    g, gt = _graph(), _graph()
    need = lib.gvqa_lcgn_attention_backward_workspace_bytes(C.byref(g), 2, 8)
    assert need >= 4 * (400 * 2 + 100 * 2 * 16)                  # dz [E, H] and the per-node rows [N, 2 H C]
    assert lib.gvqa_lcgn_attention_backward_workspace_bytes(None, 2, 8) == 0
    assert lib.gvqa_lcgn_attention_backward_workspace_bytes(C.byref(g), 9, 8) == 0
    assert lib.gvqa_lcgn_attention_backward_workspace_bytes(C.byref(g), 2, 6) == 0
    fake = 1 << 20

    def bwd(g_, gt_, H, Cc, ws_bytes=need, ws=fake, **kw):
        HC = H * Cc
        return lib.gvqa_lcgn_attention_backward(
            g_, gt_, H, Cc, 0, 0.2, kw.get("J"), kw.get("ldj", 3 * HC), kw.get("pc"), kw.get("ldpc", 2 * HC), kw.get("alpha"), None,
            kw.get("dout"), kw.get("ldd", Cc), kw.get("dJ"), kw.get("lddj", 3 * HC), kw.get("dpc"), kw.get("lddpc", 2 * HC), ws, ws_bytes,
            None)

    assert bwd(None, C.byref(gt), 2, 8) == E_INV and "lcgn_attention_backward: null graph" in err()
    assert bwd(C.byref(g), None, 2, 8) == E_INV and "null graph" in err()
    for H in (0, 9):
        assert bwd(C.byref(g), C.byref(gt), H, 8) == E_UNS and "heads" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 6) == E_UNS and "multiple of 4" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 2052) == E_UNS and "4096" in err()
    assert bwd(C.byref(_graph(finalized=0)), C.byref(gt), 2, 8) == E_INV and "finalized" in err()
    assert bwd(C.byref(g), C.byref(_graph(nodes=99)), 2, 8) == E_INV and "transposed graph" in err()
    assert bwd(C.byref(g), C.byref(_graph(edges=401)), 2, 8) == E_INV and "transposed graph" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, lddj=47) == E_INV and "leading dimensions" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, ldd=4) == E_INV and "leading dimensions" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, ws_bytes=need - 1) == E_WS and "workspace" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, ws=None) == E_WS and "workspace" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8) == E_INV and "null dpc" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, dpc=fake) == E_INV and "null tensor" in err()
    ops = dict(J=fake, pc=fake, dout=fake, dJ=fake, dpc=fake)
    assert bwd(C.byref(g), C.byref(gt), 2, 8, **ops) == E_INV and "null alpha" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, alpha=fake, **{**ops, "dout": fake + 8}) == E_UNS and "aligned" in err()
    assert bwd(C.byref(g), C.byref(gt), 2, 8, alpha=fake, ldd=10, **ops) == E_UNS and "aligned" in err()
    empty = _graph(nodes=0, edges=0, graphs=0)
    assert bwd(C.byref(empty), C.byref(empty), 2, 8, ws_bytes=0, ws=None) == 0    # an empty batch enqueues nothing


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("concat", [False, True])
def test_gradient_fixture_matches_fp64_autograd_through_the_oracle(H, concat):
    """The recorded reference gradients (lcgn.py:63-238, loss (out * w).sum()) against fp64 autograd through the oracle's
    lcgn_conv: outputs within 1e-4, gradients within 5e-4 relative with the floor 1e-3 x the largest gradient entry (the bound of
    tests/test_gpu_lcgn_heads.py::_grad_case_layer)."""
    meta, g = load_golden("lcgn_heads_grads")
    N, B = g["batch"].shape[0], int(g["batch"].max()) + 1
    s = meta["input_seeds"]
    p = synth.gat_lcgn_params(meta["in_channels"], meta["out_channels"], H, meta["param_seed"] + H, meta["cmd_dim"], concat=concat)
    assert set(p) == set(PARAMS)
    for tag, ei in (("layer", g["edge_index"]), ("xlayer", g["x_edge_index"])):
        key = f"{tag}_h{H}_c{int(concat)}"
        rp = {k: v.double().requires_grad_(True) for k, v in tparams(p).items()}
        x = t(synth.normal((N, meta["in_channels"]), s["x"])).double().requires_grad_(True)
        cmd = t(synth.normal((B, meta["cmd_dim"]), s["cmd"])).double().requires_grad_(True)
        out, _ = _layer_oracle(x, t(ei), cmd, t(g["batch"]), rp, H, concat, slope=meta["negative_slope"])
        (out * t(synth.normal(tuple(out.shape), meta["loss_seed"])).double()).sum().backward()
        assert maxabs(out, g[key + "_out"]) < 1e-4, key
        refs = {"dx": x.grad, "dcmd": cmd.grad, **{"d_" + k: rp[k].grad for k in PARAMS}}
        floor = 1e-3 * max(float(v.abs().max()) for v in refs.values())
        bad = {k: maxabs(g[f"{key}_{k}"], v) / max(float(v.abs().max()), floor) for k, v in refs.items()}
        bad = {k: e for k, e in bad.items() if not e < 5e-4}
        assert not bad, (key, bad)
