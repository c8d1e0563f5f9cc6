"""Host tier of gvqa_embed_sum_backward (no GPU): argument validation and error strings, the Python mirrors of the header's constants,
the workspace size at the config-3 node call, and the fairness of the GPU tier's bound on a numpy restatement of the algorithm."""
import os
import re

import numpy as np
import pytest

from tests import embed_sum_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from graphvqa_amd import _lib, build
    build.build()
    return _lib.load()


def _header_constant(name):
    header = open(os.path.join(ROOT, "include", "gvqa.h")).read()
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", header)
    assert m, name
    return int(m.group(1))


def test_constants_mirror_the_header():
    from graphvqa_amd import _lib
    assert _lib.EMBED_BWD_SLICE == _header_constant("GVQA_EMBED_BWD_SLICE")
    assert _lib.EMBED_BWD_CHUNK == _header_constant("GVQA_EMBED_BWD_CHUNK")
    assert _lib.EMBED_BWD_MAX_V == _header_constant("GVQA_EMBED_BWD_MAX_V") >= 8192


def test_workspace_holds_no_expansion(lib):
    """config-3 node call: far below the [rows T, D] array the torch road builds (943 MB); the plan's arrays are two histograms of
    V x slices ints, 8 bytes per occurrence and two partial rows per chunk."""
    rows, T, V, D = 65536, 12, 3000, 300
    need = lib.gvqa_embed_sum_backward_workspace_bytes(rows, T, V, D)
    assert 0 < need <= rows * T * D * 4 // 10
    from graphvqa_amd import _lib
    n = rows * T
    plan = 2 * (V * (n // _lib.EMBED_BWD_SLICE) + 1) * 4 + n * 8 + (n // _lib.EMBED_BWD_CHUNK) * 2 * D * 4
    assert need <= plan + (1 << 20)
    # it grows with the occurrences, not with occurrences x D x T
    assert lib.gvqa_embed_sum_backward_workspace_bytes(4 * rows, 1, V, D) < need
    assert lib.gvqa_embed_sum_backward_workspace_bytes(0, 1, V, D) > 0


def test_unsupported_shapes_have_no_workspace(lib):
    from graphvqa_amd import _lib
    assert lib.gvqa_embed_sum_backward_workspace_bytes(10, 1, _lib.EMBED_BWD_MAX_V, 8) > 0
    assert lib.gvqa_embed_sum_backward_workspace_bytes(10, 1, _lib.EMBED_BWD_MAX_V + 1, 8) == 0
    assert lib.gvqa_embed_sum_backward_workspace_bytes(1 << 30, 2, 16, 8) == 0          # rows T = 2^31
    for bad in ((-1, 1, 4, 4), (4, 0, 4, 4), (4, 1, 0, 4), (4, 1, 4, 0)):
        assert lib.gvqa_embed_sum_backward_workspace_bytes(*bad) == 0


def test_argument_validation_and_error_strings(lib):
    """Every refusal comes before any device work: these calls run without a GPU (the pointers are never dereferenced)."""
    from graphvqa_amd import _lib
    err = lambda: lib.gvqa_last_error().decode()
    P = 0x1000                                                          # a non-null address that is never read
    need = lib.gvqa_embed_sum_backward_workspace_bytes(8, 2, 10, 4)
    call = lambda rows=8, T=2, V=10, D=4, tok=P, neg=None, ign=-1, dout=P, ldd=4, dt=P, ws=P, nb=need: lib.gvqa_embed_sum_backward(
        rows, T, V, D, tok, neg, ign, dout, ldd, dt, ws, nb, None)
    for kw in (dict(rows=-1), dict(T=0), dict(V=0), dict(D=0)):
        assert call(**kw) == _lib.E_INVALID and "bad dims" in err()
    for ign in (-2, 10, 1 << 40):
        assert call(ign=ign) == _lib.E_INVALID and "ignore_index" in err()
    assert call(V=_lib.EMBED_BWD_MAX_V + 1) == _lib.E_UNSUPPORTED and str(_lib.EMBED_BWD_MAX_V) in err()
    assert call(rows=1 << 30, T=2) == _lib.E_UNSUPPORTED
    assert call(dt=None) == _lib.E_INVALID and "null" in err()
    assert call(tok=None) == _lib.E_INVALID and "null" in err()
    assert call(dout=None) == _lib.E_INVALID and "null" in err()
    assert call(ldd=3) == _lib.E_INVALID and "ldd" in err()
    assert call(nb=need - 1) == _lib.E_WORKSPACE and "workspace" in err()
    assert call(ws=None) == _lib.E_WORKSPACE and "workspace" in err()


def test_numpy_restatement_meets_the_bound_on_counts_around_the_chunk():
    """The bound of the GPU tier is fair: counting sort + chunked fp32 sum, restated in numpy at the library's chunk and slice sizes,
    meets it on the 'counts around the chunk' inputs -- and at a chunk size that cuts the runs elsewhere."""
    L, S = _header_constant("GVQA_EMBED_BWD_CHUNK"), _header_constant("GVQA_EMBED_BWD_SLICE")
    # (the fp64 reference itself first, on a case small enough to write out)
    tok = np.array([[1, 1, 0], [2, 9, -4]], dtype=np.int64)              # 9 clamps to 2, -4 to 0
    dout = np.array([[1.0, 2.0], [10.0, 20.0]], dtype=np.float32)
    ref, bound, cnt = ER.reference(tok, dout, 3, np.array([0, 1], dtype=np.uint8), -1)
    assert ref.tolist() == [[1 - 10, 2 - 20], [2, 4], [-20, -40]] and cnt.tolist() == [2, 2, 2]
    ref, bound, cnt = ER.reference(tok, dout, 3, None, 0)
    assert ref.tolist() == [[0, 0], [2, 4], [20, 40]] and cnt.tolist() == [0, 2, 2]
    tok, dout, negate, V = ER.counts_around_chunk(L)
    ref, bound, cnt = ER.reference(tok, dout, V, negate, -1)
    assert list(cnt[:9]) == [0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, 4 * L + 3]
    for chunk, slice_ in ((L, S), (L, 300), (37, 64)):
        got = ER.counting_sort_chunked_sum(tok, dout, V, negate, -1, slice_, chunk)
        ER.check(got, ref, bound, cnt, f"L={chunk} S={slice_}")
    # ignoring a token drops its occurrences and zeroes its row; the others keep their bits
    got = ER.counting_sort_chunked_sum(tok, dout, V, negate, 8, S, L)
    ref8, bound8, cnt8 = ER.reference(tok, dout, V, negate, 8)
    assert cnt8[8] == 0 and not got[8].any()
    ER.check(got, ref8, bound8, cnt8, "ignore 8")
