"""CPU-only checks: the C-ABI library loads and exports every declared symbol, host logic."""
import json
import os
import re

import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from graphvqa_amd.scene_graph import scene_graph_topology, batch_scene_graphs
from tests.util import ROOT, load_golden, integration_md_stub, header_struct_members


def test_library_exports_every_declared_symbol():
    from graphvqa_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gvqa.h")).read()
    declared = set(re.findall(r"\b(gvqa_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.gvqa_version()
    # pure host-side entry points can be called without a GPU
    assert lib.gvqa_graph_workspace_bytes(10, 20, 2) > (11 + 20 + 20 + 10 + 3) * 4


def test_struct_layouts_match_header():
    import ctypes as C
    from graphvqa_amd import _lib
    assert C.sizeof(_lib.Graph) == 3 * 8 + 6 * 8 + 6 * 4 + 8 + 2 * 4 + 8 + 2 * 4 + 7 * 8     # + row_group_ptr, num_row_groups, max_row_group_edges, row_group_order, + the packed plan (2 ints, 7 pointers)
    assert _lib.Graph.row_group_ptr.offset == 96 and _lib.Graph.max_row_group_edges.offset == 108 and _lib.Graph.row_group_order.offset == 112
    assert C.sizeof(_lib.GatConvParams) == 10 * 8
    assert C.sizeof(_lib.GatDims) == 10 * 4 and _lib.GatDims.projection.offset == 32 and _lib.GatDims.hop_fusion.offset == 36
    assert C.sizeof(_lib.LcgnDims) == 8 * 4
    assert C.sizeof(_lib.GatMpBwdDesc) == 16 + 15 * 8 and _lib.GatMpBwdDesc.dalpha_node.offset == 120 and _lib.GatMpBwdDesc.dxp_absmax.offset == 128


def _ctypes_members(cls):
    import ctypes as C
    kinds = {C.c_void_p: "ptr", C.c_char_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_float: "f32", C.c_size_t: "size"}
    out = []
    for name, typ in cls._fields_:
        if hasattr(typ, "_length_"):
            out.append((name, kinds[typ._type_], typ._length_))
        else:
            out.append((name, kinds[typ], 0))
    return out


_HEADER_STRUCTS = {"Graph": "gvqa_graph", "GatConvParams": "gvqa_gat_conv_params", "GatDims": "gvqa_gat_dims",
                   "GatMpDesc": "gvqa_gat_mp_desc", "GatMpBwdDesc": "gvqa_gat_mp_bwd_desc", "MpPlan": "gvqa_mp_plan",
                   "BnParams": "gvqa_bn_params", "GineParams": "gvqa_gine_params", "GcnParams": "gvqa_gcn_params",
                   "LcgnDims": "gvqa_lcgn_dims", "LcgnParams": "gvqa_lcgn_params", "PoolParams": "gvqa_pool_params",
                   "ClassifierParams": "gvqa_classifier_params", "EncoderParams": "gvqa_encoder_params"}


def test_every_ctypes_structure_matches_the_header_member_for_member():
    """Parsed from include/gvqa.h, not from hand-kept offsets: names, kinds (pointer / int32 / int64 / float / size_t), array
    lengths and order of every structure the binding mirrors."""
    import ctypes as C
    from graphvqa_amd import _lib
    mirrored = {n for n in dir(_lib) if isinstance(getattr(_lib, n), type) and issubclass(getattr(_lib, n), C.Structure)
                and getattr(_lib, n) is not C.Structure}
    assert mirrored == set(_HEADER_STRUCTS), mirrored ^ set(_HEADER_STRUCTS)
    for cls, cname in _HEADER_STRUCTS.items():
        assert _ctypes_members(getattr(_lib, cls)) == header_struct_members(cname), cname


def test_integration_stub_structs_match_the_header():
    """INTEGRATION.md section 2 is the binding a maintainer copies: its fenced block is EXECUTED here (it dlopens the library
    and defines the structures; the forward itself runs on the GPU tier) and its three structures are held to the header."""
    import subprocess, sys
    code = integration_md_stub() + """
import json, ctypes as C
kinds = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int64: "i64", C.c_float: "f32", C.c_size_t: "size"}
print(json.dumps({n: [(f, kinds[t], 0) for f, t in c._fields_] for n, c in (("gvqa_graph", Graph),
      ("gvqa_gat_conv_params", HopParams), ("gvqa_gat_dims", Dims))}))
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for cname, members in got.items():
        assert [tuple(m) for m in members] == header_struct_members(cname), cname


def test_dynamic_symbols_are_the_c_abi_only():
    """-fvisibility=hidden + GVQA_API + the linker's version script: `nm -D` shows gvqa_* and nothing else defined."""
    import shutil, subprocess
    from graphvqa_amd import _lib, build
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-D", "--defined-only", build.build()], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = [l.split()[-1] for l in r.stdout.splitlines() if l.strip()]
    assert syms and all(s.startswith("gvqa_") for s in syms), [s for s in syms if not s.startswith("gvqa_")][:10]
    assert set(syms) == set(_lib.PROTOTYPES), set(syms) ^ set(_lib.PROTOTYPES)


def test_kernels_with_counted_dma_waits_keep_their_register_budget():
    """The LDS-DMA kernels order their asm-issued DMAs with hand-counted `s_waitcnt vmcnt(N)`; the compiler's own counter knows nothing of those DMAs, so a
    spill it re-loads inside a K loop comes with a `vmcnt(0)` that drains every DMA in flight (round 6 found two per step in the one-launch hop kernel), and
    a large scratch frame doubles a short kernel's dispatch time (round 6: the GINE MLP).  build.py keeps the compiler's per-kernel resource remarks
    (lib/kernel_resources.json); this pins what the shipped kernels were measured with: no scratch at all in the GEMM-class kernels, a bounded frame --
    outside the K loop, checked in the ISA when it was set -- in the hop kernels, and the occupancy each was designed for."""
    from graphvqa_amd import build
    lib = build.build()
    res = json.load(open(os.path.join(os.path.dirname(lib), "kernel_resources.json")))
    def of(sub):
        hits = {k: v for k, v in res.items() if sub in k}
        assert hits, sub
        return hits
    for sub in ("k_linear_bf16_big", "k_linear_bf16_wide", "k_linear_bf16_dma", "k_gine_mlp", "k_linear_nn_direct", "k_linear_tn_direct", "k_linear_f32_dma"):
        for k, v in of(sub).items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)          # (SGPR spills go to VGPR lanes: no memory traffic)
    for k, v in of("k_linear_split3").items():          # (the six-product bf16 x 3 epilogue variants keep a 12-byte frame)
        assert v["ScratchSize"] <= 16, (k, v)
    for k, v in of("k_hopagg4").items():                # 8 waves x 256 registers; the one-launch forms spill a few hop-invariant values outside the K loop
        assert v["Occupancy"] == 2 and v["ScratchSize"] <= 160 and v["LDS Size"] <= 160 * 1024, (k, v)
    for k, v in of("k_gine_mlp").items():               # 4 waves x 512 registers (accumulators in AGPRs)
        assert v["Occupancy"] == 1 and v["AGPRs"] >= 160, (k, v)
    for k, v in of("k_linear_bf16_big").items():
        assert v["Occupancy"] == 2 and v["LDS Size"] == 3 * 48 * 1024, (k, v)


def test_argument_validation_without_gpu():
    import ctypes as C
    from graphvqa_amd import _lib
    lib = _lib.load()
    g = _lib.Graph()
    assert lib.gvqa_graph_build(-1, 0, 0, None, None, None, 0, None, C.byref(g)) == _lib.E_INVALID
    assert b"negative" in lib.gvqa_last_error()
    assert lib.gvqa_graph_build(4, 2, 1, None, None, None, 0, None, C.byref(g)) == _lib.E_INVALID
    d = _lib.GatDims(8, 8, 4, 16, 4, 5, 0.2, 1e-5)     # node_dim != out_channels
    assert lib.gvqa_gat_seq_forward(C.byref(g), C.byref(d), (_lib.GatConvParams * 5)(), None, None, None, None,
                                    None, None, None, 0, None) == _lib.E_INVALID
    assert b"skip connection" in lib.gvqa_last_error()


def test_module_state_dict_contract():
    """Key names and shapes of SURVEY 8a-5c (pipeline_model_gat.py:823-836 loads by name+shape)."""
    from graphvqa_amd.gat_skip import gat_seq
    m = gat_seq(300, 300, 300, 512, 5, dropout=0.1, gat_heads=4)
    sd = m.state_dict()
    want = synth.gat_seq_params(300, 300, 300, 512, 5, 4, seed=1)
    assert set(sd) == set(want)
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert sum(p.numel() for p in m.parameters()) == 9765900
    assert sd["convs.0.lin_r.weight"].data_ptr() == sd["convs.0.lin_l.weight"].data_ptr()
    # reference init rule: glorot bound, zero bias
    a = np.sqrt(6.0 / (1200 + 812))
    w = sd["convs.3.lin_l.weight"]
    assert float(w.abs().max()) <= a * (1 + 1e-6) and float(w.abs().max()) > 0.99 * a   # fp32 rounding of the bound
    assert float(sd["convs.0.bias"].abs().max()) == 0.0


def test_cpu_tensors_raise_no_fallback():
    from graphvqa_amd.gat_skip import gat_seq
    m = gat_seq(8, 8, 8, 8, 2, gat_heads=4).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(3, 8), torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 8), torch.zeros(2, 1, 8),
          torch.zeros(3, dtype=torch.int64))


def test_synth_is_deterministic_and_shaped():
    a, b = synth.normal((1000,), 5), synth.normal((1000,), 5)
    assert np.array_equal(a, b) and abs(a.mean()) < 0.15 and 0.9 < a.std() < 1.1
    gb = synth.config3_batch()
    assert (gb.num_nodes, gb.num_edges, gb.num_graphs) == (65536, 262144, 2048)
    assert np.all(np.diff(gb.batch) >= 0)
    assert np.array_equal(gb.batch[gb.edge_index[0]], gb.batch[gb.edge_index[1]])   # block diagonal
    gb2 = synth.config2_batch()
    assert gb2.num_graphs == 1000 and 28000 < gb2.num_nodes < 32000 and gb2.num_edges == 2 * gb2.num_nodes
    # every node has its self loop first among its outgoing edges
    first = np.unique(gb2.edge_index[0], return_index=True)[1]
    assert np.array_equal(gb2.edge_index[0][first], gb2.edge_index[1][first])


def test_scene_graph_builder_matches_pinned_topology():
    meta, g = load_golden("debug_topology")
    # rebuild from a tiny hand-written scene graph exercising every rule
    sg = {"objects": {"b": {"relations": [{"object": "a", "name": "on"}, {"object": "a", "name": "near"}]},
                      "a": {"relations": [{"object": "b", "name": "under"}]},
                      "c": {"relations": [{"object": "a", "name": "left of"}]}}}
    n, ei, added = scene_graph_topology(sg)
    # nodes sorted: a=0, b=1, c=2.  a: self, a->b (reverse exists) ; b: self, b->a, b->a ; c: self, c->a, +a->c
    assert n == 3
    assert ei.T.tolist() == [[0, 0], [0, 1], [1, 1], [1, 0], [1, 0], [2, 2], [2, 0], [0, 2]]
    assert added.tolist() == [7]
    n0, ei0, _ = scene_graph_topology({"objects": {}})      # empty graph -> 2-node dummy
    assert n0 == 2 and ei0.shape[1] == 4
    gb = batch_scene_graphs([sg, sg])
    assert gb.num_nodes == 6 and gb.edge_index[:, 8:].min() == 3


def _fake_graph(nodes, edges, graphs, max_nodes, max_edges, intra=1):
    """A finalized gvqa_graph with hand-filled statistics (no device memory): enough for host-side planning."""
    from graphvqa_amd import _lib
    g = _lib.Graph()
    g.num_nodes, g.num_edges, g.num_graphs = nodes, edges, graphs
    g.max_graph_nodes, g.max_graph_edges, g.max_in_degree = max_nodes, max_edges, 8
    g.intra_graph, g.valid, g.finalized = intra, 1, 1
    return g


def test_mp_tiling_plan_host_logic():
    """The LDS-tiling decision of the message-passing kernel is pure host code: check it without a GPU."""
    import ctypes as C
    from graphvqa_amd import _lib
    lib = _lib.load()

    def plan(g, Cc, H):
        p = _lib.MpPlan()
        assert lib.gvqa_gat_mp_plan(C.byref(g), Cc, H, C.byref(p)) == 0
        return p

    p = plan(_fake_graph(65536, 262144, 2048, 32, 128), 512, 4)          # BASELINE config 3
    assert p.tiled == 1 and p.channel_range == 128 and p.stage_buffers == 2 and p.blocks_per_cu == 3
    assert p.stages_per_graph == 4 * 5 and p.accumulators == 2 and p.lds_bytes <= 160 * 1024 // 3
    assert p.blocks_per_graph == 1                                          # a full batch: one block per graph
    small = plan(_fake_graph(2048, 8192, 64, 32, 128), 512, 4)              # 64 graphs cannot fill 256 CUs
    assert small.tiled == 1 and small.blocks_per_graph == 4 and small.channel_range == 128
    assert plan(_fake_graph(8192, 32768, 256, 32, 128), 512, 4).blocks_per_graph == 2
    p = plan(_fake_graph(29785, 59570, 1000, 40, 80), 300, 4)            # BASELINE config 2
    assert p.tiled == 1 and p.channel_range == 100 and p.blocks_per_cu >= 3 and p.channel_range % 4 == 0
    p = plan(_fake_graph(5000, 20000, 1, 5000, 20000), 32, 4)            # one huge graph: no LDS tile
    assert p.tiled == 0
    assert plan(_fake_graph(100, 400, 4, 30, 120), 30, 4).tiled == 0     # C % 4 != 0 -> scalar general kernels
    assert plan(_fake_graph(100, 400, 4, 30, 120, intra=0), 32, 4).tiled == 0   # cross-graph edges
    assert plan(_fake_graph(100, 400, 4, 30, 120), 32, 3).tiled == 0     # H not in {1,2,4,8}
    g = _fake_graph(100, 400, 4, 30, 120)
    g.finalized = 0
    assert plan(g, 32, 4).tiled == 0                                      # statistics not available yet
    big = plan(_fake_graph(4000, 16000, 10, 400, 1600), 512, 4)          # 400-node graphs: narrower ranges, fewer per CU
    assert big.tiled == 1 and big.lds_bytes <= 160 * 1024 and big.channel_range < 128


def test_every_entry_point_rejects_bad_arguments_without_gpu():
    """Status codes + messages, never a crash: null structs, non-positive dims, missing weights,
    undersized workspaces (all checked before any device work is enqueued)."""
    import ctypes as C
    from graphvqa_amd import _lib
    lib = _lib.load()
    g = _fake_graph(100, 400, 4, 30, 120)
    E_INV, E_WS, E_UNS = _lib.E_INVALID, _lib.E_WORKSPACE, _lib.E_UNSUPPORTED
    err = lambda: lib.gvqa_last_error().decode()

    # linear
    assert lib.gvqa_linear_f32(4, 4, 4, None, 4, None, 4, None, 0, None, 4, None) == E_INV and "null" in err()
    assert lib.gvqa_linear_f32(-1, 4, 4, None, 4, None, 4, None, 0, None, 4, None) == E_INV
    assert lib.gvqa_linear_f32(0, 4, 4, None, 4, None, 4, None, 0, None, 4, None) == 0          # empty product is fine
    # gat conv / seq
    d = _lib.GatDims(8, 8, 0, 8, 4, 1, 0.2, 1e-5)
    p = _lib.GatConvParams()
    assert lib.gvqa_gat_conv_forward(C.byref(g), C.byref(d), C.byref(p), None, None, None, None, None, 0, None) == E_WS
    assert lib.gvqa_gat_conv_forward(None, C.byref(d), C.byref(p), None, None, None, None, None, 0, None) == E_INV
    d9 = _lib.GatDims(8, 8, 4, 8, 4, 9, 0.2, 1e-5)
    assert lib.gvqa_gat_seq_forward(C.byref(g), C.byref(d9), (_lib.GatConvParams * 9)(), None, None, None, None, None,
                                    None, None, 0, None) == E_INV and "num_hops" in err()
    gx = _fake_graph(100, 400, 4, 30, 120, intra=0)
    d2 = _lib.GatDims(8, 8, 4, 8, 4, 2, 0.2, 1e-5)
    assert lib.gvqa_gat_seq_forward(C.byref(gx), C.byref(d2), (_lib.GatConvParams * 2)(), None, None, None, None, None,
                                    None, None, 0, None) == E_UNS and "joins two graphs" in err()
    assert lib.gvqa_gat_seq_workspace_bytes(C.byref(g), C.byref(d2)) > 0
    assert lib.gvqa_gat_seq_forward_trainbn(C.byref(g), C.byref(d2), (_lib.GatConvParams * 2)(), None, None, None, None,
                                            None, None, 0, None) == E_INV
    # message passing descriptor
    m = _lib.GatMpDesc()
    assert lib.gvqa_gat_message_passing(C.byref(g), C.byref(m), None, 0, None) == E_INV
    # variants
    assert lib.gvqa_bn_relu_chain(10, 8, 9, None, 1e-5, None, None, None) == E_INV and "stages" in err()
    gp = _lib.GineParams()
    assert lib.gvqa_gine_conv_forward(C.byref(g), 8, 0, 8, C.byref(gp), None, None, None, None, None, 0, None) == E_INV
    assert lib.gvqa_gine_conv_forward(C.byref(gx), 8, 4, 8, C.byref(gp), None, None, None, None, None, 0, None) == E_INV
    cp = _lib.GcnParams()
    assert lib.gvqa_gcn_conv_forward(C.byref(g), 8, 0, 8, C.byref(cp), None, None, None, None, 0, None) == E_INV
    ld = _lib.LcgnDims(8, 8, 8, 4, 5, 2, 0.2, 0)                                   # heads != 1
    assert lib.gvqa_lcgn_seq_forward(C.byref(g), C.byref(ld), C.byref(_lib.LcgnParams()), None, None, None, None, None,
                                     None, 0, None) == E_UNS
    ld1 = _lib.LcgnDims(8, 8, 8, 4, 5, 1, 0.2, 0)
    assert lib.gvqa_lcgn_seq_forward(C.byref(g), C.byref(ld1), C.byref(_lib.LcgnParams()), None, None, None, None, None,
                                     None, 0, None) == E_WS
    assert lib.gvqa_lcgn_pack_bytes(C.byref(ld1)) > 15 * 64 * 4 and lib.gvqa_lcgn_pack_bytes(None) == 0
    ld16 = _lib.LcgnDims(8, 8, 8, 4, 5, 1, 0.2, 1)
    # both modes carry packed node-GEMM weights on top of the stacked fp32 forms: bf16 pieces (bf16 node features) or two-piece
    # fp16 images with their row scales (fp32 mode)
    stacks = (3 * 64 + 3 * 128 + 2 * 64 + 4 * 64 + 4 * 8) * 4
    assert lib.gvqa_lcgn_pack_bytes(C.byref(ld16)) > stacks and lib.gvqa_lcgn_pack_bytes(C.byref(ld1)) > stacks
    assert lib.gvqa_lcgn_pack_weights(C.byref(ld1), C.byref(_lib.LcgnParams()), None, 0, None) == E_INV
    assert lib.gvqa_linear_bf16(4, 4, 12, 2, None, 12, None, None, None, 0, None, 0, 0, None, 4, 0, None) == E_INV
    assert lib.gvqa_pack_weight_bf16(4, 4, 3, None, 4, None, None) == E_INV
    assert lib.gvqa_attention_pool_forward(C.byref(g), 8, 8, C.byref(_lib.PoolParams()), None, None, None, None, 0, None) == E_INV
    assert lib.gvqa_answer_logits_forward(4, 8, 8, 10, C.byref(_lib.ClassifierParams()), None, None, None, None, 0, None) == E_INV
    assert lib.gvqa_sg_encoder_forward(C.byref(g), 50, 8, 12, 1, C.byref(_lib.EncoderParams()), None, None, None, 0, None,
                                       1e-5, None, None, None, 0, None) == E_INV
    # differentiable path
    assert lib.gvqa_gat_mp_backward(C.byref(g), None, C.byref(_lib.GatMpBwdDesc()), None) == E_INV
    bd = _lib.GatMpBwdDesc(); bd.C, bd.H = 8, 9
    assert lib.gvqa_gat_mp_backward(C.byref(g), C.byref(g), C.byref(bd), None) == E_UNS and "H <=" in err()
    bd.H = 4
    assert lib.gvqa_gat_mp_backward(C.byref(g), C.byref(g), C.byref(bd), None) == E_INV and "null tensor" in err()
    assert lib.gvqa_bn_train_workspace_bytes(1000, 32) >= 4 * 2 * 32 * 4 and lib.gvqa_bn_train_workspace_bytes(10, 0) == 0
    assert lib.gvqa_bn_relu_train_forward(10, 0, None, None, None, 1e-5, None, None, None, None, 0, None) == E_INV
    assert lib.gvqa_bn_relu_train_forward(10, 8, None, None, None, 1e-5, None, None, None, None, 0, None) == E_INV
    assert lib.gvqa_bn_relu_train_backward(10, 8, None, None, None, None, None, 1e-5, None, None, None, None, None, 0, None) == E_INV
    assert lib.gvqa_graph_rows_to_nodes(C.byref(g), 8, None, 4, None, 8, 0, None) == E_INV       # ld_rows < F
    assert lib.gvqa_graph_segment_sum(C.byref(g), 8, None, 8, None, 8, None) == E_INV
    assert lib.gvqa_graph_edge_rows_sum(C.byref(g), 8, None, 8, None, 4, None) == E_INV      # ld_out < F
    assert lib.gvqa_graph_finalize(C.byref(_lib.Graph()), None) == E_INV
    assert lib.gvqa_prof_collect(None, None) == E_INV


def test_package_all_lists_every_module():
    import graphvqa_amd
    here = os.path.dirname(graphvqa_amd.__file__)
    mods = {f[:-3] for f in os.listdir(here) if f.endswith(".py") and f != "__init__.py"}
    assert set(graphvqa_amd.__all__) == mods, set(graphvqa_amd.__all__) ^ mods


def _product_source(text):
    """`text` without the lines that only the measurement build (-DGVQA_PROBES) compiles: the `#ifdef GVQA_PROBES` half of every
    conditional on it and the `#else` half of every `#ifndef GVQA_PROBES`, nested conditionals included."""
    kept, stack = [], []        # stack: per open conditional, whether its current half is probes-only
    for line in text.splitlines():
        d = re.match(r"\s*#\s*(ifdef|ifndef|if|elif|else|endif)\b\s*(\S*)", line)
        if d and d.group(1) in ("ifdef", "ifndef", "if"):
            probes = d.group(2) == "GVQA_PROBES" and d.group(1) != "if"
            stack.append([probes and d.group(1) == "ifdef", probes])
        elif d and d.group(1) in ("elif", "else"):
            if stack[-1][1]:
                stack[-1][0] = not stack[-1][0]
        elif d:
            stack.pop()
        elif not any(half for half, _ in stack):
            kept.append(line)
    assert not stack, "unbalanced preprocessor conditionals"
    return "\n".join(kept)


def test_product_library_reads_only_the_documented_option_variables():
    header = open(os.path.join(ROOT, "include", "gvqa.h")).read()
    comment = re.search(r"/\* Process-wide run-time options\..*?\*/", header, re.S).group(0)
    documented = set(re.findall(r"\bGVQA_[A-Z0-9_]+", comment)) - set(re.findall(r"\bGVQA_OPT_[A-Z0-9_]+", comment))
    assert len(documented) == 9, sorted(documented)
    csrc = os.path.join(ROOT, "graphvqa_amd", "csrc")
    read, indirect = set(), []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        src = _product_source(open(os.path.join(csrc, f)).read())
        read |= set(re.findall(r"\b(?:getenv|env_int)\(\s*\"(GVQA_[A-Z0-9_]+)\"", src))
        indirect += [f"{f}: {m}" for m in re.findall(r"\bgetenv\(\s*([^\"\s)][^)]*)\)", src)]
    assert indirect == ["capi.hip: name"], indirect          # options_init's env_int helper, fed the literal names above
    assert read == documented, sorted(read ^ documented)


def test_python_package_reads_only_the_documented_environment_variables():
    """The same for graphvqa_amd/*.py: the GVQA_* names read through os.environ / os.getenv are GVQA_LIB (a second build of the library) and
    GVQA_ALLGATHER (the multi-chip gather), each named in DESIGN.md or INTEGRATION.md; nothing else in the package is switched from outside."""
    pkg = os.path.join(ROOT, "graphvqa_amd")
    read = set()
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            read |= set(re.findall(r"\b(?:environ(?:\.get\(|\[)|getenv\()\s*[\"'](GVQA_[A-Z0-9_]+)[\"']", src))
            assert not re.findall(r"\b(?:environ(?:\.get\(|\[)|getenv\()\s*[^\"'\s]", src), f"{f}: an environment name that is not a literal"
    assert read == {"GVQA_LIB", "GVQA_ALLGATHER"}, sorted(read)
    docs = open(os.path.join(ROOT, "DESIGN.md")).read() + open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in read:
        assert re.search(r"\b%s\b" % name, docs), name
