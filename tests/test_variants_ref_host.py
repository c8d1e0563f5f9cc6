"""CPU companion of tests/test_gpu_variants_matrix.py: the dense references of tests/variants_ref.py agree with the oracle's
restatement in fp64 and with the recorded fixtures, the batches have the structure they promise, and every case the GPU file runs
is fair -- its fp32 CPU form stays so close to fp64 that 8 x its distance is below 1e-2 x |ref|max, so a scaled bound proves
something and a correct fp32 kernel can meet it."""
import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from oracle import ref_torch as R
from tests import variants_ref as V
from tests.util import load_golden, t, tparams, maxabs

GOLDEN_TOL = 2e-5           # tests/test_oracle_golden.py's bounds on these fixtures: TOL for out and gcn_conv_small, 5e-5 for the convs


def _seq_by_dense(kind, x, ei, ea, ins, batch, p):
    """gine_seq / gcn_seq with return_convs as written from the dense forms: hop i sees x after i BN -> ReLU stages."""
    K, h, convs = ins.shape[0], x, []
    for i in range(K):
        if kind == "gine":
            q = [p[f"convs.{i}.nn.{k}"] for k in ("0.weight", "0.bias", "2.weight", "2.bias")]
            convs.append(V.gine_dense(h, ea, ei, *q, float(p[f"convs.{i}.eps"]), ins[i], batch))
        else:
            convs.append(V.gcn_dense(h, p[f"convs.{i}.weight"], p[f"convs.{i}.bias"], ei, ins[i], batch))
        if i != K - 1:
            h = V.bn_chain(h, [tuple(p[f"bns.{i}.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))])
    return h, convs


def test_hard_and_wide_batches_have_the_structure():
    gb, cross, info = V.hard_batch()                              # (its own assertions run here)
    N = gb.num_nodes
    for e in (gb.edge_index, cross):
        loops, plain = V._loop_counts(e, N)
        assert loops[info["only_loops"]] == 2 and plain[info["only_loops"]] == 0
        assert loops[info["double_loop"]] == 2 and plain[info["double_loop"]] >= 1
        indeg = np.bincount(e[1], minlength=N)
        assert sorted(set(indeg.tolist()) & set(range(10))) == list(range(10)) and indeg.max() == 301
        assert V.without_self_loops(e).shape[1] == e.shape[1] - int(loops.sum())
    assert bool((cross[1] == gb.edge_index[1]).all()) and bool((gb.batch[cross[0]] != gb.batch[cross[1]]).any())
    for n in (1101, 1023):
        wb = V.wide_batch(n)
        assert wb.num_nodes == n and bool((wb.edge_index[:, :gb.num_edges] == gb.edge_index).all())
        assert bool((wb.batch[wb.edge_index[0]] == wb.batch[wb.edge_index[1]]).all()) and wb.edge_index.max() < n
        assert int((np.bincount(wb.edge_index[1], minlength=n) == 0).sum()) >= 2          # the dead-rows case has rows to set
    assert 1101 == 8 * 128 + 77


def test_dense_references_equal_the_oracle_in_fp64():
    gb, cross, _ = V.hard_batch()
    N, B, Dn, Di = gb.num_nodes, gb.num_graphs, 24, 12
    x, ins = t(synth.normal((N, Dn), 1)).double(), t(synth.normal((5, B, Di), 3)).double()
    batch = t(gb.batch.copy())
    pg, pc = (tparams(f(Dn, Dn, Di, 77), torch.float64) for f in (synth.gine_seq_params, synth.gcn_seq_params))
    for i in range(5):
        pg[f"convs.{i}.eps"] = torch.tensor([0.25 - 0.2 * i], dtype=torch.float64)
    for e in (gb.edge_index, cross):
        ei = t(e.copy())
        ea = t(synth.normal((e.shape[1], Dn), 2)).double()
        xc, ec = torch.cat((x, ins[0][batch]), 1), torch.cat((ea, ins[0][batch[ei[0]]]), 1)
        ref = R.gcn_conv(xc, ei, {"weight": pc["convs.0.weight"], "bias": pc["convs.0.bias"]})
        assert maxabs(V.gcn_dense(x, pc["convs.0.weight"], pc["convs.0.bias"], ei, ins[0], batch), ref) < 1e-12
        assert maxabs(V.gcn_dense(xc, pc["convs.0.weight"], pc["convs.0.bias"], ei), ref) < 1e-12
        q = {k[len("convs.0."):]: v for k, v in pg.items() if k.startswith("convs.0.nn")}
        for eps in V.GINE_EPS:
            ref = R.gine_conv(xc, ei, ec, q, eps=eps)
            got = V.gine_dense(x, ea, ei, q["nn.0.weight"], q["nn.0.bias"], q["nn.2.weight"], q["nn.2.bias"], eps, ins[0], batch)
            assert maxabs(got, ref) < 1e-12
        # the oracle's gine_seq takes eps = 0 (its default); compare the sequences with it
        p0 = dict(pg, **{f"convs.{i}.eps": torch.zeros(1, dtype=torch.float64) for i in range(5)})
        for kind, p, args in (("gine", p0, (x, ei, ea, ins, batch)), ("gcn", pc, (x, ei, ins, batch))):
            rout, rconvs = (R.gine_seq if kind == "gine" else R.gcn_seq)(*args, p, return_convs=True)
            out, convs = _seq_by_dense(kind, x, ei, ea, ins, batch, p)
            assert maxabs(out, rout) < 1e-12 and maxabs(torch.stack(convs), torch.stack(rconvs)) < 1e-12, kind


def test_dense_references_reproduce_the_recorded_fixtures():
    meta, g = load_golden("gcn_conv_small")
    p = tparams(synth.gcn_seq_params(20, 8, 4, meta["param_seed"], num_layers=1))
    assert maxabs(V.gcn_dense(t(g["x"]), p["convs.0.weight"], p["convs.0.bias"], t(g["edge_index"])), g["out"]) < GOLDEN_TOL
    for kind, f in (("gcn", synth.gcn_seq_params), ("gine", synth.gine_seq_params)):
        meta, g = load_golden(kind + "_seq_small")
        p = tparams(f(meta["dn"], meta["dn"], meta["di"], meta["param_seed"]))
        ea = t(g["edge_attr"]) if kind == "gine" else None
        out, convs = _seq_by_dense(kind, t(g["x"]), t(g["edge_index"]), ea, t(g["instr"]), t(g["batch"]), p)
        assert maxabs(out, g["out"]) < GOLDEN_TOL and maxabs(torch.stack(convs), g["convs"]) < 5e-5, kind


# ---- the conditioning cap: every case of the GPU file ---------------------------------------------------------------------------------
def _fair(name, got32, ref):
    d = maxabs(got32, ref)
    print(f"{name}: fp32 CPU form from fp64 {d:.3g}, |ref|max {float(ref.abs().max()):.3g}")
    assert bool(torch.isfinite(got32).all()) and V.well_conditioned(d, ref), (name, d, float(ref.abs().max()))
    return d


@pytest.mark.parametrize("C", V.GCN_WIDTHS)
def test_gcn_cases_are_fair_to_fp32(C):
    for Di in (0, V.GCN_DI):
        c = V.gcn_case(C, Di)
        for kind in (0, 1):
            _fair(f"gcn C={C} Di={Di} kind={kind}", V.gcn_reference(c, kind, torch.float32), V.gcn_reference(c, kind))
            if C == 300:                  # test_gcn_bias_forms_no_graph_and_no_edges (graph=None is the same arithmetic as graph=)
                _fair(f"gcn C=300 Di={Di} kind={kind} no bias", V.gcn_reference(c, kind, torch.float32, bias=False),
                      V.gcn_reference(c, kind, bias=False))
        if C == 300:
            empty = torch.zeros((2, 0), dtype=torch.int64)
            c0 = dict(c, eis=(empty, empty))
            _fair(f"gcn C=300 Di={Di} E=0", V.gcn_reference(c0, 0, torch.float32), V.gcn_reference(c0, 0))


def test_gine_cases_are_fair_to_fp32():
    for Dn, Di, C in V.GINE_HARD:
        c = V.gine_hard_case(Dn, Di, C)
        for eps in V.GINE_EPS:
            _fair(f"gine Dn={Dn} Di={Di} C={C} eps={eps}", V.gine_reference(c, eps, torch.float32), V.gine_reference(c, eps))
    for N, Dn, C, Di in V.GINE_WIDE:
        c = V.gine_wide_case(N, Dn, C, Di)
        for eps in V.GINE_EPS if (N, Dn, C, Di) == V.GINE_WIDE[0] else V.GINE_EPS[:1]:      # (the instruction-share test runs both signs at the first)
            _fair(f"gine wide N={N} Dn={Dn} C={C} Di={Di} eps={eps}", V.gine_reference(c, eps, torch.float32), V.gine_reference(c, eps))
    c = V.gine_wide_case(1101, 24, 320, 0, dead=True)
    ref = V.gine_reference(c, 0.25)
    _fair("gine dead rows", V.gine_reference(c, 0.25, torch.float32), ref)
    assert torch.equal(ref[c["dead_rows"]], c["b2"].double().expand(len(c["dead_rows"]), -1))
    assert float(c["x"][c["dead_rows"][-1]].abs().max()) > 0 and float(c["x"][c["dead_rows"][:-1]].abs().max()) == 0


def test_gradient_cases_are_fair_to_fp32():
    c = V.grad_case()
    for kind in (0, 1):
        ref = V.gine_grad_reference(c, kind)
        e = V.grad_errors(V.gine_grad_reference(c, kind, torch.float32)[1], ref[1])
        print(f"gine gradients kind={kind}: fp32 CPU form " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
        assert set(e) == set(V.GINE_GRAD_NAMES) and V.MARGIN * max(e.values()) < 1e-2
        for bias in (True, False):
            ref = V.gcn_grad_reference(c, kind, bias)
            e = V.grad_errors(V.gcn_grad_reference(c, kind, bias, torch.float32)[1], ref[1])
            print(f"gcn gradients kind={kind} bias={bias}: fp32 CPU form " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
            assert V.MARGIN * max(e.values()) < 1e-2


@pytest.mark.parametrize("N,C,offset", V.CHAIN_SHAPES)
def test_bn_chain_cases_are_fair_to_fp32(N, C, offset):
    for S in V.CHAIN_STAGES:
        x, stages = V.chain_case(N, C, S)
        ref = V.bn_chain(x.double(), stages)
        _fair(f"chain N={N} C={C} S={S}", V.bn_chain_fp32(x, stages), ref)
        col = np.arange(C)
        if S:
            assert float(stages[min(1, S - 1)][3][col % 7 == 1].abs().max()) == 0.0                  # running_var = 0
            assert float(stages[min(2, S - 1)][0][col % 7 == 2].max()) < 0.0                         # negative weights
            assert float(stages[min(3, S - 1)][0][col % 7 == 3].abs().max()) == 0.0                  # zero weights
            assert float((ref > 0).double().mean()) > 0.2                                            # the chain does not die out
        else:
            assert torch.equal(ref, x.double())
    x, _ = V.chain_case(N, C, 1)
    ratio = (x.double().mean(0) / x.double().std(0)).abs()
    assert 80 < float(ratio.max()) < 125


@pytest.mark.parametrize("N,C", V.BN_TRAIN_SHAPES)
def test_bn_train_cases_are_fair_to_fp32(N, C):
    c = V.bn_train_case(N, C)
    kind, x = c["kind"], c["x"].double()
    assert kind[V.BN_CONSTANT_COLUMN] == 3 and float(x[:, V.BN_CONSTANT_COLUMN].var(unbiased=False)) == 0.0
    out = x[:, V.BN_OUTLIER_COLUMN]
    assert kind[V.BN_OUTLIER_COLUMN] == 4 and float(out[0]) == 1e4 and float((out[0] - out[1:].mean()) / out[1:].std(unbiased=False).clamp(min=1)) > 5e3
    assert set(V.bn_strata(kind)) <= set(V.BN_STRATA) and {"ordinary", "large_mean", "constant", "outlier_pivot"} <= set(V.bn_strata(kind))
    assert sum(len(v) for v in V.bn_strata(kind).values()) == C
    big, small = np.flatnonzero(kind == 0), np.flatnonzero(kind == 1)
    assert float(x[:, big].mean(0).max()) > 5e3 and (N == 2 or 0.5 < float(x[:, big].std(0).mean()) < 1.5)
    if len(small):
        assert abs(float(x[:, small].mean()) - 10.0) < 0.05 and float(x[:, small].std(0).max()) < 3e-2
    pre = (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + V.BN_EPS) * c["w"].double() + c["b"].double()
    assert float(pre.abs().min()) >= V.BN_GATE_MARGIN and 0.2 < float((pre > 0).double().mean()) < 0.8
    # E[x^2] - E[x]^2 in fp32 is useless on these columns: this is what the inputs are for
    naive = (c["x"] ** 2).mean(0) - c["x"].mean(0) ** 2
    assert N == 2 or float((naive - x.var(0, unbiased=False)).abs()[big].max()) > 1.0
    for masked in (False, True):
        ref, nbt = V.bn_train_fp64(c, masked)
        got = V.bn_train_fp32(c, masked)
        assert nbt == 1
        for name, cols in V.bn_strata(kind).items():
            d = V.bn_distances(got, ref, cols)
            print(f"bn-train N={N} C={C} masked={masked} {name}: fp32 CPU form " + " ".join(f"{k} {v:.3g}" for k, v in d.items()))
            for k, v in d.items():
                # (the cap is per case, over all its columns: at N = 2 the two rows' xhat is +-1 and dx is of order eps / var in every column)
                assert V.MARGIN * v < 1e-2 * max(float(ref[k].abs().max()), 1e-300), (name, k, v)


@pytest.mark.parametrize("N,C", V.BN_TRAIN_SHAPES)
def test_bn_statistics_in_the_kernels_summation_order(N, C):
    """k_bn_col_stats_fused / k_bn_col_finish / k_bn_col_finish_m2 restated in numpy fp32 (V.bn_stats_in_kernel_order): with the
    median-of-three pivot the batch mean and variance meet the bounds the GPU test sets, per kind of column; on the raw values (the
    kernels before the pivot) the variance of the large-mean columns misses them at the two shapes with more than one full row block:
    every block's rounded mean enters n_b (mean_b - mean)^2 in first order."""
    c = V.bn_train_case(N, C)
    ref, _ = V.bn_train_fp64(c, True)
    two_pass = V.bn_train_fp32(c, True)
    strata = V.bn_strata(c["kind"])
    missed = {}
    for pivot in (True, False):
        mean, var = V.bn_stats_in_kernel_order(c["x"], pivot)
        got = dict(mean=mean, var=var, running_mean=0.1 * mean, running_var=0.9 + 0.1 * var * (N / (N - 1)))
        for name, cols in strata.items():
            d, d32, plain = V.bn_distances(got, ref, cols), V.bn_distances(two_pass, ref, cols), V.bn_plain_bounds(ref, cols)
            print(f"bn statistics N={N} C={C} pivot={pivot} {name}: " + " ".join(f"{k} restated {d[k]:.3g} two-pass {d32[k]:.3g}" for k in d))
            for k in d:
                if not d[k] < (plain[k] if name == "ordinary" else max(V.MARGIN * d32[k], plain[k])):
                    missed[(pivot, name, k)] = (d[k], d32[k])
    assert not [k for k in missed if k[0]], missed
    if N > 128:
        assert (False, "large_mean", "var") in missed, missed
