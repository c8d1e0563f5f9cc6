"""CPU companion of tests/test_gpu_lcgn_attention_matrix.py and tests/test_gpu_lcgn_attention_matrix_bf16.py: the hard batch has the
structure it promises, the shape matrix lands on every chunk count of the launchers, and the large-logit inputs are fair -- the
plain fp32 dense reference stays finite on them and close to fp64, so a correct fp32 kernel can meet the bounds held on the GPU."""
import numpy as np
import pytest
import torch

from tests import lcgn_ref as L


def test_hard_batch_has_the_structure():
    gb, cross, info = L.hard_batch()                # (its own assertions run here)
    N = gb.num_nodes
    for ei in (gb.edge_index, cross):
        indeg, outdeg = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
        assert sorted(set(indeg.tolist()) & set(range(10))) == list(range(10))
        assert indeg.max() == indeg[info["hub_in"]] == L.HUB_DEGREE and outdeg.max() == outdeg[info["hub_out"]] == L.HUB_DEGREE
        assert indeg[info["isolated"]] == 0
        assert len({(int(s), int(d)) for s, d in ei.T}) < ei.shape[1]
    sizes = np.bincount(gb.batch, minlength=gb.num_graphs)
    assert sizes[info["empty_graph"]] == 0 and sizes[info["single_graph"]] == 1 and 0 < info["empty_graph"] < gb.num_graphs - 1
    assert bool((gb.batch[cross[0]] != gb.batch[cross[1]]).any()) and bool((gb.batch[gb.edge_index[0]] == gb.batch[gb.edge_index[1]]).all())
    assert bool((cross[1] == gb.edge_index[1]).all())


@pytest.mark.parametrize("bf16", [False, True])
def test_hub_logits_ascend_in_coo_order(bf16):
    """Head 0's logit ascends along the hub's in-edges in both edge lists (the running maximum moves at every step), and stays
    ascending, up to near-ties that the rounding of the rescaled J reorders, in the large-logit stratum; the other heads do not."""
    H, Cc = 4, 256
    gb, _, info = L.hard_batch()
    J, pc, _, eis = L.hard_operands(H, Cc, bf16)
    for ei in eis:
        hub = ei[1] == info["hub_in"]
        z = L.logits64(J, pc, ei, gb.batch, H, Cc)[hub]
        assert bool((np.diff(z[:, 0]) >= 0).all()) and int((np.diff(z[:, 0]) > 0).sum()) >= L.HUB_DEGREE - 2
        assert all(int((np.diff(z[:, h]) < 0).sum()) > 50 for h in range(1, H))
        zb = L.logits64(L.big_logit_J(J, pc, ei, gb.batch, H, Cc, bf16), pc, ei, gb.batch, H, Cc)
        assert abs(np.abs(zb).max() - L.BIG_LOGIT) < (4.0 if bf16 else 1e-3)
        # (rounding the rescaled x_l to bf16 again moves z by about 2^-9 of its scale: near-ties swap)
        assert int((np.diff(zb[hub, 0]) > 0).sum()) >= (L.HUB_DEGREE - 1) * (0.8 if bf16 else 0.99)


def test_shape_matrix_reaches_every_chunk_count():
    """launch_plan restates the launchers' rule; the matrix must land on every chunk count (KC) the templates are instantiated for,
    in the one-wave layout (H C <= 1024) and in the one-wave-per-head layout, with full lanes (need == KC) and idle head segments."""
    fp32 = {L.launch_plan(H, Cc, 4)[::3] for H, Cc in L.SHAPES}
    bf16 = {L.launch_plan(H, Cc, 8)[::3] for H, Cc in L.SHAPES}
    # KC = 16 (fp32) and KC = 8 (bf16) need C > 2048, so H = 1 and H C > 1024: they exist in the second layout only
    assert fp32 == {(True, 1), (True, 2), (True, 4), (True, 8), (False, 1), (False, 2), (False, 4), (False, 8), (False, 16)}
    assert bf16 == {(True, 1), (True, 2), (True, 4), (False, 1), (False, 2), (False, 4), (False, 8)}
    assert [L.launch_plan(H, Cc, 4)[3] for H, Cc in L.SHAPES] == [1, 4, 4, 4, 2, 4, 1, 2, 8, 16, 8]
    assert [L.launch_plan(H, Cc, 8)[3] for H, Cc in L.SHAPES] == [1, 2, 2, 2, 1, 2, 1, 1, 4, 8, 4]
    assert [L.launch_plan(H, Cc, 4)[3] for H, Cc in L.SHAPES_FP32_ODD] == [1, 2, 4, 8, 16]
    assert all(Cc % 8 == 4 for _, Cc in L.SHAPES_FP32_ODD) and all(Cc % 8 == 0 for _, Cc in L.SHAPES)
    full = {per: {kc for H, Cc in L.SHAPES for _, _, need, kc in [L.launch_plan(H, Cc, per)] if need == kc} for per in (4, 8)}
    assert full[4] == {1, 2, 4, 8, 16} and full[8] == {1, 2, 4, 8}
    assert {H for H, _ in L.SHAPES} >= {5, 6, 7} and max(H * Cc for H, Cc in L.SHAPES) == 4096
    assert set(L.SHAPES_BIG) <= set(L.SHAPES) and {(4, 256), (5, 40), (2, 2048)} <= set(L.SHAPES_BIG)
    assert {L.launch_plan(H, Cc, 8)[3] for H, Cc in L.SHAPES_BIG} == {1, 2, 4, 8}


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("H,Cc", L.SHAPES_BIG)
def test_large_logit_inputs_are_fair_to_fp32(H, Cc, bf16):
    """At max |z| = 500 the dense reference in fp32 is finite and within 2e-5 of fp64 in out and alpha, with and without the mask,
    on both edge lists; the leaky logits reach past +400 (an unshifted expf overflows) and below -88 (it underflows)."""
    concat = H > 1
    worst = dict(out=0.0, alpha=0.0)
    for kind in (0, 1):
        for masked in (False, True):
            c = L.hard_case(H, Cc, concat, bf16, kind, True, masked)
            ref = L.dense_reference(c, H, Cc, concat, torch.float64, grads=False)
            got = L.dense_reference(c, H, Cc, concat, torch.float32, grads=False)
            assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
            d = L.distances(got, ref)
            worst = {k: max(worst[k], d[k]) for k in worst}
        z = torch.from_numpy(L.logits64(c["J"].numpy(), c["pc"].numpy(), c["ei"].numpy(), c["batch"].numpy(), H, Cc))
        l = torch.nn.functional.leaky_relu(z, L.SLOPE)
        assert float(l.max()) > 400 and float(l.min()) < -88
    print(f"H={H} C={Cc} bf16={bf16}: fp32 dense reference from fp64 at max |z| = 500: out {worst['out']:.3g} alpha {worst['alpha']:.3g}")
    assert worst["out"] < 2e-5 and worst["alpha"] < 2e-5
