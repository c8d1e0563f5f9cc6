"""The gat_seq hop-kernel decision, pinned on the CPU: which hop form runs, which weight layout it needs and how much workspace /
weight cache it takes are pure host code over the scalar statistics of a graph handle, the dims and the process options.

tests/golden/seq_plan_table.json is that decision recorded from the commit named in its header (the parent of the change that
moved the rule into one plan function); the test replays every row against the built library and requires the four values equal.

    python -m tests.test_seq_plan --record      # re-record (only on purpose: a changed row is a behaviour change)
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests.util import GOLDEN, ROOT

TABLE = os.path.join(GOLDEN, "seq_plan_table.json")
_KEEP = []          # dummy buffers that stand in for device arrays (the queries test the pointers for NULL only)

# ---- fabricated handles: name -> (graphs, row groups, largest row group's edges, extras) ---------------------------------
# nodes = 128 per row group unless given, edges = 4 per node; pk = (packed row groups, their largest edge count)
_HANDLES = {
    "cfg3":        dict(graphs=2048, nodes=65536, edges=262144, groups=512, rg_edges=512),
    "cfg2_pk":     dict(graphs=1000, nodes=29785, edges=59570, groups=262, rg_edges=256, pk=(246, 270)),
    "shard256":    dict(graphs=256, nodes=8192, edges=32768, groups=64, rg_edges=512),
    "g550":        dict(graphs=2200, groups=550, rg_edges=512),
    # the default rule's fill thresholds on 256 CUs, both sides: one round 0.85, two 0.76, three 0.82, four 0.85
    "g217":        dict(graphs=868, groups=217, rg_edges=512),
    "g218":        dict(graphs=872, groups=218, rg_edges=512),
    "g389":        dict(graphs=1556, groups=389, rg_edges=512),
    "g390":        dict(graphs=1560, groups=390, rg_edges=512),
    "g629":        dict(graphs=2516, groups=629, rg_edges=512),
    "g630":        dict(graphs=2520, groups=630, rg_edges=512),
    "g870":        dict(graphs=3480, groups=870, rg_edges=512),
    "g871":        dict(graphs=3484, groups=871, rg_edges=512),
    # the 128-row-group boundary of HOP_COEFFS = 2, inside and outside the in-kernel coefficients' 522-edge capacity
    "g127_e512":   dict(graphs=508, groups=127, rg_edges=512),
    "g128_e512":   dict(graphs=512, groups=128, rg_edges=512),
    "g127_e600":   dict(graphs=508, groups=127, rg_edges=600),
    "g128_e600":   dict(graphs=512, groups=128, rg_edges=600),
    "g64_e522":    dict(graphs=256, groups=64, rg_edges=522),
    "g64_e523":    dict(graphs=256, groups=64, rg_edges=523),
    # LDS edge capacities: persistent chained <= 614 < persistent <= 716; aggregate-first <= 1024; chained 8-wave <= 1420 < 8-wave <= 1574
    "e614":        dict(graphs=2048, groups=512, rg_edges=614),
    "e650":        dict(graphs=2048, groups=512, rg_edges=650),
    "e717":        dict(graphs=2048, groups=512, rg_edges=717),
    "e1024":       dict(graphs=2048, groups=512, rg_edges=1024),
    "e1025":       dict(graphs=2048, groups=512, rg_edges=1025),
    "e1500":       dict(graphs=2048, groups=512, rg_edges=1500),
    "e2000":       dict(graphs=2048, groups=512, rg_edges=2000),
    # H = 8: persistent chained <= 341 < persistent <= 398
    "e300":        dict(graphs=2048, groups=512, rg_edges=300),
    "e380":        dict(graphs=2048, groups=512, rg_edges=380),
    "no_groups":   dict(graphs=16, nodes=65536, edges=262144, groups=0, rg_edges=0),
    "cross_graph": dict(graphs=2048, groups=512, rg_edges=512, intra=0),
    "unfinalized": dict(graphs=2048, groups=512, rg_edges=512, finalized=0),
    "pk_only_fits": dict(graphs=2048, groups=512, rg_edges=1100, pk=(470, 1000)),
}

# name -> (node_dim == out_channels, edge_dim, ins_dim, heads, num_hops)
_DIMS = {
    "d512":     (512, 512, 512, 4, 5),
    "d300":     (300, 300, 512, 4, 5),
    "d256":     (256, 256, 512, 4, 5),      # the C <= 256 exclusion of the default rule ...
    "d260":     (260, 260, 512, 4, 5),      # ... and the first width past it
    "d384":     (384, 384, 512, 4, 5),      # column parts need C > 384
    "d388":     (388, 388, 512, 4, 5),
    "d516":     (516, 516, 512, 4, 5),      # beyond the aggregate-first kernel's 512 columns
    "d64":      (64, 48, 40, 4, 5),         # too small a product for the split projection on a shard
    "d512_h8":  (512, 512, 512, 8, 5),
    "d512_h2":  (512, 512, 512, 2, 5),
    "d512_h1":  (512, 512, 512, 1, 5),
    "d512_k1":  (512, 512, 512, 4, 1),      # one hop: no one-launch form
    "d512_k8":  (512, 512, 512, 4, 8),
    "d512_noins": (512, 512, 0, 4, 5),
    "d510":     (510, 510, 512, 4, 5),      # C % 4 != 0
    "bad_skip": (512, 512, 512, 4, 5),      # node_dim != out_channels (out_channels = 256 below): the error returns
}

COLUMNS = ["handle", "dims", "hop_fusion", "projection", "hop_coeffs", "packed_groups",
           "hop_kernel", "weight_layout", "workspace_bytes", "weight_cache_bytes"]


def _cases():
    """(handle, dims, hop_fusion override or None, projection override or None, HOP_COEFFS, PACKED_GROUPS)"""
    modes = [None, 0, 1, 2, 3, 4, 5, 6]
    rows = []
    # every mode on the main batches
    main = [("cfg3", "d512"), ("cfg2_pk", "d300"), ("cfg2_pk", "d512"), ("shard256", "d512"), ("shard256", "d64"), ("g550", "d512"),
            ("e650", "d512"), ("e1025", "d512"), ("e1500", "d512"), ("e2000", "d512"), ("no_groups", "d512"),
            ("cross_graph", "d512"), ("unfinalized", "d512"), ("cfg3", "bad_skip"), ("cfg3", "d512_h8"), ("e300", "d512_h8"),
            ("e380", "d512_h8"), ("cfg3", "d512_h2"), ("pk_only_fits", "d512")]
    rows += [(h, d, m, None, 2, 1) for h, d in main for m in modes]
    # fill thresholds and capacities: default rule and the explicit aggregate-first / persistent modes
    for h in ("g217", "g218", "g389", "g390", "g629", "g630", "g870", "g871", "e614", "e717", "e1024"):
        rows += [(h, "d512", m, None, 2, 1) for m in (None, 2, 4)]
    # widths
    for d in ("d256", "d260", "d384", "d388", "d516", "d510", "d512_h1", "d512_k1", "d512_k8", "d512_noins"):
        rows += [("cfg3", d, m, None, 2, 1) for m in (None, 1, 5, 6)]
    # the process options
    for h, d in (("cfg3", "d512"), ("cfg2_pk", "d300"), ("shard256", "d512"), ("g127_e512", "d512"), ("g128_e512", "d512"),
                 ("g127_e600", "d512"), ("g128_e600", "d512"), ("g64_e522", "d512"), ("g64_e523", "d512"), ("pk_only_fits", "d512")):
        rows += [(h, d, m, None, hc, pg) for hc in (0, 1, 2) for pg in (0, 1) for m in (None, 1) if (hc, pg) != (2, 1) or h.startswith("g1") or h.startswith("g64")]
    # the projection override (value + 1: split3, f32, split2h)
    for h, d in (("cfg3", "d512"), ("cfg2_pk", "d300"), ("shard256", "d512")):
        rows += [(h, d, m, p, 2, 1) for p in (1, 2, 3) for m in (None, 0, 1, 2, 4)]
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def _handle(spec):
    from graphvqa_amd import _lib
    g = _lib.Graph()
    groups = spec["groups"]
    g.num_graphs = spec["graphs"]
    g.num_nodes = spec.get("nodes", groups * 128)
    g.num_edges = spec.get("edges", 4 * g.num_nodes)
    g.max_graph_nodes, g.max_graph_edges, g.max_in_degree = 32, 128, 8
    g.intra_graph, g.valid, g.finalized = spec.get("intra", 1), 1, spec.get("finalized", 1)
    dummy = C.create_string_buffer(64)
    _KEEP.append(dummy)
    g.num_row_groups, g.max_row_group_edges = groups, spec["rg_edges"]
    g.row_group_ptr = C.addressof(dummy) if groups > 0 else None
    if "pk" in spec:
        g.pk_num_row_groups, g.pk_max_row_group_edges = spec["pk"]
        g.pk_row_group_ptr = C.addressof(dummy)
    return g


def _dims(name, spec, hop_fusion, projection):
    from graphvqa_amd import _lib
    dn, de, di, heads, hops = spec
    d = _lib.GatDims(dn, de, di, 256 if name == "bad_skip" else dn, heads, hops, 0.2, 1e-5)
    d.hop_fusion = 0 if hop_fusion is None else hop_fusion + 1
    d.projection = 0 if projection is None else projection
    return d


def _answer(lib, handles, dims, case):
    """The four recorded values of one row, under that row's process options (restored afterwards)."""
    from graphvqa_amd import _lib
    h, dname, hop_fusion, projection, hop_coeffs, packed_groups = case
    g, d = _handle(handles[h]), _dims(dname, dims[dname], hop_fusion, projection)
    old = (_lib.set_option(_lib.OPT_HOP_COEFFS, hop_coeffs), _lib.set_option(_lib.OPT_PACKED_GROUPS, packed_groups))
    try:
        kernel = lib.gvqa_gat_seq_hop_kernel(C.byref(g), C.byref(d))
        layout = lib.gvqa_gat_seq_weight_layout(C.byref(g), C.byref(d))
        ws = lib.gvqa_gat_seq_workspace_bytes(C.byref(g), C.byref(d))
        cache = lib.gvqa_gat_seq_weight_cache_bytes(C.byref(d), layout)
    finally:
        _lib.set_option(_lib.OPT_HOP_COEFFS, old[0])
        _lib.set_option(_lib.OPT_PACKED_GROUPS, old[1])
    return [int(kernel), int(layout), int(ws), int(cache)]


def _gpu_cu_count():
    """CUs of the visible GPU, or None without one (the library then plans for 256)."""
    import torch
    if not torch.cuda.is_available():
        return None
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_seq_plan_table_matches_the_recorded_decisions():
    """Replays tests/golden/seq_plan_table.json (recorded from the commit its header names, on 256 CUs) and requires the hop kernel,
    the weight layout id, the workspace size and the weight-cache size of that layout to be EQUAL in every row.

    Coverage of the table (asserted below, so that a re-recorded table cannot lose it): every GVQA_HOP_* value 0 .. 7; the weight
    layout ids -1, 0, 1, 2, 3, 7 and 10; both error returns (GVQA_E_INVALID: handle not finalized, node_dim != out_channels;
    GVQA_E_UNSUPPORTED: cross-graph edges); the default rule's fill thresholds on both sides (217 | 218 groups = 0.85 of one round,
    389 | 390 = 0.76 of two, 629 | 630 = 0.82 of three, 870 | 871 = 0.85 of four); the C <= 256 exclusion (256 | 260); the
    128-row-group boundary of HOP_COEFFS = 2 (127 | 128 groups, within and beyond the in-kernel coefficients' 522 edges); the LDS
    edge capacities of every kernel (persistent 614 / 716 and, H = 8, 341 / 398; aggregate-first 1024; 8-wave 1420 / 1574);
    packed row groups on and off; every hop_fusion override 0 .. 6 and unset; the three projection overrides; HOP_COEFFS 0 / 1 / 2.
    Skips only when a GPU with a CU count other than 256 is visible (the thresholds scale with it)."""
    from graphvqa_amd import _lib, build
    build.build()
    cus = _gpu_cu_count()
    if cus is not None and cus != 256:
        pytest.skip(f"the table was recorded for 256 CUs, this GPU has {cus}")
    lib = _lib.load()
    table = json.load(open(TABLE))
    assert table["columns"] == COLUMNS
    rows = table["rows"]
    assert 200 <= len(rows) <= 600
    bad = []
    for row in rows:
        case = tuple(row[:6])
        got = _answer(lib, table["handles"], {k: tuple(v) for k, v in table["dims"].items()}, case)
        if got != row[6:]:
            bad.append((case, row[6:], got))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ (case, recorded, got): {bad[:8]}"
    kernels, layouts = {r[6] for r in rows}, {r[7] for r in rows}
    assert kernels == {0, 1, 2, 3, 4, 5, 6, 7, _lib.E_INVALID, _lib.E_UNSUPPORTED}, kernels
    assert layouts == {-1, 0, 1, 2, 3, 7, 10}, layouts
    by_handle = lambda h, d="d512": [r[6] for r in rows if r[0] == h and r[1] == d and r[2] is None and r[3] is None and (r[4], r[5]) == (2, 1)]
    for below, above in (("g217", "g218"), ("g389", "g390"), ("g629", "g630"), ("g870", "g871")):
        assert by_handle(below) == [3] and by_handle(above) == [6], (below, above)
    assert by_handle("cfg3", "d256") == [3] and by_handle("cfg3", "d260") == [6]
    ws = lambda h: [r[8] for r in rows if r[0] == h and r[1] == "d512" and r[2] is None and (r[4], r[5]) == (2, 1)]
    assert by_handle("g127_e600") == [1] and by_handle("g128_e600") == [3]          # no in-kernel coefficients: chained from 128 groups on
    assert by_handle("g127_e512") == [3] and by_handle("g128_e512") == [3] and ws("g127_e512")[0] * 128 > ws("g128_e512")[0] * 127   # (the partial-logit buffers)


def _record():
    from graphvqa_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert _gpu_cu_count() in (None, 256)
    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "graphvqa_amd/csrc", "include"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    assert not dirty, "record from a clean csrc/ and include/"
    rows = [list(c) + _answer(lib, _HANDLES, _DIMS, c) for c in _cases()]
    table = {"header": f"gat_seq plan decisions of this project's commit {commit} (256 CUs), recorded by `python -m tests.test_seq_plan --record`; "
                       "hop_fusion: the per-call override's option value or null, projection: the override field as passed (value + 1) or null",
             "columns": COLUMNS, "handles": _HANDLES, "dims": _DIMS, "rows": rows}
    with open(TABLE, "w") as f:
        f.write("{\n")
        for k in ("header", "columns", "handles", "dims"):
            f.write(f" {json.dumps(k)}: {json.dumps(table[k])},\n")
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]\n}\n")
    print(f"{len(rows)} rows -> {TABLE}")
    print("hop kernels:", sorted({r[6] for r in rows}), "layouts:", sorted({r[7] for r in rows}))


if __name__ == "__main__":
    if "--record" in sys.argv:
        _record()
