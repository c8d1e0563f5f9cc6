"""CPU-only checks of lcgn_seq(gat_heads > 1, node_feature_dtype=bfloat16): argument validation of gvqa_lcgn_attention_bf16
(status codes, nothing enqueued), the module's construction / state_dict contract, and the new kernel's compiled resources."""
import ctypes as C
import json
import os

import pytest
import torch

from graphvqa_amd import synth
from tests.test_lcgn_heads_host import _graph


def test_lcgn_attention_bf16_rejects_bad_arguments_without_gpu():
    from graphvqa_amd import _lib
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    E_INV, E_UNS = _lib.E_INVALID, _lib.E_UNSUPPORTED
    g = _graph()
    fake = 1 << 20                      # never dereferenced: every check comes before any device work

    def att(g_, H, Cc, ldj=None, ldpc=None, ldo=None, J=fake, pc=fake, out=fake, bias=None, out_bf16=1):
        return lib.gvqa_lcgn_attention_bf16(g_, H, Cc, 0, 0.2, J, 3 * H * Cc if ldj is None else ldj, pc,
                                            2 * H * Cc if ldpc is None else ldpc, bias, out, Cc if ldo is None else ldo, out_bf16, None, None)

    assert att(None, 2, 8) == E_INV and "null graph" in err()
    assert att(C.byref(_graph(finalized=0)), 2, 8) == E_INV and "finalized" in err()
    for kw in (dict(J=None), dict(pc=None), dict(out=None)):
        assert att(C.byref(g), 2, 8, **kw) == E_INV and "null tensor" in err(), kw
    assert att(C.byref(g), 2, 8, ldj=40) == E_INV and "leading dimensions" in err()
    for H in (0, 9):
        assert att(C.byref(g), H, 8) == E_UNS and "heads" in err()
    assert att(C.byref(g), 2, 12) == E_UNS and "multiple of 8" in err()
    assert att(C.byref(g), 2, 6) == E_UNS
    assert att(C.byref(g), 1, 4104) == E_UNS and "4096" in err()          # heads * C = 4104
    assert att(C.byref(g), 3, 1368) == E_UNS and "4096" in err()          # 4104 again, over three heads
    assert att(C.byref(g), 2, 8, ldj=3 * 16 + 4) == E_UNS and "aligned" in err()
    assert att(C.byref(g), 2, 8, ldpc=2 * 16 + 2) == E_UNS and "aligned" in err()
    assert att(C.byref(g), 2, 8, ldo=12) == E_UNS and "aligned" in err()              # a bf16 row of 12: 24 bytes
    assert att(C.byref(g), 2, 8, ldo=10, out_bf16=0) == E_UNS and "aligned" in err()  # an fp32 row of 10: 40 bytes
    for kw in (dict(J=fake + 8), dict(pc=fake + 4), dict(out=fake + 2), dict(bias=fake + 4)):
        assert att(C.byref(g), 2, 8, **kw) == E_UNS and "aligned" in err(), kw
    assert att(C.byref(_graph(nodes=0, edges=0)), 2, 8, J=None, pc=None, out=None) == 0      # an empty batch enqueues nothing


def test_lcgn_seq_bf16_heads_constructs_and_keeps_the_state_dict_contract():
    from graphvqa_amd.lcgn import lcgn_seq
    m = lcgn_seq(12, 8, 12, 5, gat_cmd_dim=8, question_dim=8, gat_heads=4, node_feature_dtype=torch.bfloat16)
    want = synth.lcgn_seq_params(12, 8, seed=1, cmd_dim=8, question_dim=8, heads=4)
    sd = m.state_dict()
    assert set(sd) == set(want)
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        assert sd[k].dtype == torch.float32 or not sd[k].is_floating_point(), k      # fp32 master weights: bf16 is a storage format of node tensors
    assert tuple(sd["lcgn.lin_l.weight"].shape) == (4 * 8, 3 * 8) and tuple(sd["lcgn.bias"].shape) == (8,)
    assert m.node_feature_dtype == torch.bfloat16 and m.gat_heads == 4 and m.bf16_weight_pieces == 2


@pytest.mark.parametrize("pieces", [2, 1])
def test_lcgn_seq_bf16_heads_has_no_cpu_fallback(pieces):
    """The combination is implemented (no NotImplementedError) and, like every other road, refuses CPU tensors."""
    from graphvqa_amd.lcgn import lcgn_seq
    m = lcgn_seq(12, 8, 12, 5, gat_cmd_dim=8, question_dim=8, gat_heads=4, node_feature_dtype=torch.bfloat16,
                 bf16_weight_pieces=pieces).eval()
    N, B, L = 5, 2, 3
    ei = torch.tensor([[0, 1, 3], [1, 2, 4]])
    batch = torch.tensor([0, 0, 0, 1, 1])
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(N, 12), ei, batch, torch.zeros(B, 8), torch.zeros(L, B, 8))


def test_lcgn_attention_bf16_wrapper_checks_its_operands_on_the_host():
    from graphvqa_amd.lcgn import lcgn_attention_bf16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lcgn_attention_bf16(torch.zeros(3, 48, dtype=torch.bfloat16), torch.zeros(1, 32), None, 2, 8, False)


def test_bf16_attention_kernel_has_no_scratch_and_no_spills():
    from graphvqa_amd import build
    lib = build.build()
    res = json.load(open(os.path.join(os.path.dirname(lib), "kernel_resources.json")))
    hits = {k: v for k, v in res.items() if "k_lcgn_attention_bf16" in k}
    assert len(hits) == 16, sorted(hits)            # chunks per lane {1, 2, 4, 8} x {intra, cross-graph} x {fp32, bf16 out}
    for k, v in hits.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
