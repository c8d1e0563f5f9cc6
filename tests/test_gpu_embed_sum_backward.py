"""GPU tier of the table gradient of the token-embedding sums: gvqa_embed_sum_backward through the C ABI, the differentiable op
`sg_encoder.embed_sum`, and the encoder on both roads of its embedding backward.  Reference: fp64 index_add_ on the CPU over the fp32
inputs; bound per element cnt_v * 2^-23 * sum|terms| (tests/embed_sum_ref.py: the a-priori bound of an fp32 sum in any order), exact
zeros for unused / ignored rows, exact values for rows with one occurrence."""
import functools

import numpy as np
import pytest
import torch

from graphvqa_amd import synth
from tests.util import t
from tests import embed_sum_ref as ER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _consts():
    from graphvqa_amd import _lib
    return _lib.EMBED_BWD_CHUNK, _lib.EMBED_BWD_SLICE


def _backward(dev, tok, dout, V, negate=None, ignore=-1, dtable=None, ws=None):
    """One call of the entry point.  tok: numpy int64 [rows, T]; dout: a numpy array or a CUDA view [rows, D] with unit inner stride."""
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream
    lib = _lib.load()
    rows, T = tok.shape
    g = dout if isinstance(dout, torch.Tensor) else t(dout, device=dev)
    D = g.shape[1]
    tk = t(tok, device=dev)
    ng = None if negate is None else t(negate, device=dev)
    need = lib.gvqa_embed_sum_backward_workspace_bytes(rows, T, V, D)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    if dtable is None:
        dtable = torch.empty((V, D), dtype=torch.float32, device=dev)
    _lib.check(lib.gvqa_embed_sum_backward(rows, T, V, D, tk.data_ptr() if rows else None, None if ng is None else ng.data_ptr(), ignore,
                                           g.data_ptr() if rows else None, g.stride(0) if rows else D, dtable.data_ptr(), ws.data_ptr(),
                                           ws.numel(), _stream(dev)))
    torch.cuda.synchronize(dev)
    return dtable.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _chunk_case():
    L, S = _consts()
    tok, dout, negate, V = ER.counts_around_chunk(L)
    return (tok, dout, negate, V) + ER.reference(tok, dout, V, negate, -1)


def test_counts_around_the_chunk(dev):
    L, S = _consts()
    tok, dout, negate, V, ref, bound, cnt = _chunk_case()
    assert list(cnt[:9]) == [0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, 4 * L + 3] and tok.shape[1] == 1 and dout.shape[1] == 300
    assert (np.diff(tok[:, 0]) != 0).sum() > tok.shape[0] // 2                   # interleaved, not sorted
    ER.check(_backward(dev, tok, dout, V, negate), ref, bound, cnt)


@pytest.mark.parametrize("ignore", [0, -1])
def test_pad_heavy_node_form(dev, ignore):
    tok, dout, V = ER.pad_heavy()
    assert ((tok != 0).sum(1) >= 1).all() and ((tok != 0).sum(1) <= 4).all() and tok[5, 0] == tok[5, 1]
    ref, bound, cnt = ER.reference(tok, dout, V, None, ignore)
    assert cnt[0] == (0 if ignore == 0 else (tok == 0).sum())
    got = _backward(dev, tok, dout, V, None, ignore)
    ER.check(got, ref, bound, cnt, f"ignore={ignore}")
    if ignore == 0:
        assert not got[0].any()


def test_across_slices_at_the_vocabulary_limit(dev):
    from graphvqa_amd import _lib
    L, S = _consts()
    tok, dout, negate, V = ER.across_slices(S)
    assert V == _lib.EMBED_BWD_MAX_V == 8192 and tok.size > 3 * S
    flat = np.clip(tok.reshape(-1), 0, V - 1)
    ns = -(-flat.size // S)
    assert all((flat[s * S:(s + 1) * S] == 5).any() for s in range(ns))
    assert (flat[(ns - 1) * S:] == 8191).sum() == 2 and not (flat[:(ns - 1) * S] == 8191).any()
    ref, bound, cnt = ER.reference(tok, dout, V, negate, -1)
    assert (cnt == 0).sum() > 8000
    ER.check(_backward(dev, tok, dout, V, negate), ref, bound, cnt)


@pytest.mark.parametrize("D", [4, 6, 300, 512])
@pytest.mark.parametrize("layout", ["plain", "column_block", "one_float_off"])
def test_widths_and_alignment(dev, D, layout):
    rng = np.random.default_rng(100 + D)
    rows, T, V = 70, 3, 9
    tok = rng.integers(0, V, (rows, T)).astype(np.int64)
    tok[tok == 7] = 2                                                            # token 7 unused
    negate = (rng.random(rows) < 0.25).astype(np.uint8)
    dout = rng.standard_normal((rows, D)).astype(np.float32)
    if layout == "plain":
        g = t(dout, device=dev)
    elif layout == "column_block":
        wide = torch.full((rows, D + 8), float("nan"), device=dev)
        wide[:, 4:4 + D] = t(dout, device=dev)
        g = wide[:, 4:4 + D]
        assert g.stride(0) == D + 8 > D
    else:
        flat = torch.full((rows * D + 1,), float("nan"), device=dev)
        flat[1:] = t(dout, device=dev).reshape(-1)
        g = flat[1:].view(rows, D)
        assert g.data_ptr() % 16 == 4
    ref, bound, cnt = ER.reference(tok, dout, V, negate, -1)
    ER.check(_backward(dev, tok, g, V, negate), ref, bound, cnt, f"D={D} {layout}")


def test_one_token_vocabulary_and_no_rows(dev):
    rng = np.random.default_rng(11)
    rows, T, D = 300, 2, 20
    tok = np.zeros((rows, T), dtype=np.int64)
    dout = rng.standard_normal((rows, D)).astype(np.float32)
    ref, bound, cnt = ER.reference(tok, dout, 1, None, -1)
    assert cnt.tolist() == [rows * T]
    ER.check(_backward(dev, tok, dout, 1), ref, bound, cnt, "V=1")
    assert not _backward(dev, tok, dout, 1, None, 0).any()                       # the only token ignored
    nan = torch.full((5, D), float("nan"), device=dev)
    got = _backward(dev, np.zeros((0, T), dtype=np.int64), np.zeros((0, D), dtype=np.float32), 5, dtable=nan)
    assert got.shape == (5, D) and not got.any()


def test_same_bits_on_every_call(dev):
    tok, dout, negate, V, ref, bound, cnt = _chunk_case()
    from graphvqa_amd import _lib
    need = _lib.load().gvqa_embed_sum_backward_workspace_bytes(tok.shape[0], 1, V, dout.shape[1])
    a = _backward(dev, tok, dout, V, negate)
    b = _backward(dev, tok, dout, V, negate)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    c = _backward(dev, tok, dout, V, negate, dtable=torch.full((V, dout.shape[1]), float("nan"), device=dev), ws=ws)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    tok2, dout2, negate2, V2 = ER.across_slices(_consts()[1])
    need2 = _lib.load().gvqa_embed_sum_backward_workspace_bytes(tok2.shape[0], tok2.shape[1], V2, dout2.shape[1])
    a2 = _backward(dev, tok2, dout2, V2, negate2, 4097)
    c2 = _backward(dev, tok2, dout2, V2, negate2, 4097, dtable=torch.full((V2, dout2.shape[1]), float("nan"), device=dev),
                   ws=torch.full((need2,), 0xFF, dtype=torch.uint8, device=dev))
    assert a2.tobytes() == c2.tobytes() and not a2[4097].any()


def test_error_codes_and_the_torch_road_past_the_limit(dev):
    from graphvqa_amd import _lib
    from graphvqa_amd.graph import _stream
    from graphvqa_amd.sg_encoder import embed_sum
    lib = _lib.load()
    err = lambda: lib.gvqa_last_error().decode()
    rows, T, V, D = 40, 2, 10, 8
    tok = torch.zeros((rows, T), dtype=torch.int64, device=dev)
    g, dt = torch.zeros((rows, D), device=dev), torch.zeros((V, D), device=dev)
    need = lib.gvqa_embed_sum_backward_workspace_bytes(rows, T, V, D)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda V_, nb: lib.gvqa_embed_sum_backward(rows, T, V_, D, tok.data_ptr(), None, -1, g.data_ptr(), D, dt.data_ptr(), ws.data_ptr(), nb,
                                                      _stream(dev))
    assert call(V, need - 1) == _lib.E_WORKSPACE and "workspace" in err()
    big = _lib.EMBED_BWD_MAX_V + 1
    assert lib.gvqa_embed_sum_backward_workspace_bytes(rows, T, big, D) == 0
    assert call(big, need) == _lib.E_UNSUPPORTED
    # the op past the limit: the torch road, the same gradient
    rng = np.random.default_rng(12)
    tk = rng.integers(0, big, (rows, T)).astype(np.int64)
    tk[:, 1] = 3
    negate = (rng.random(rows) < 0.5).astype(np.uint8)
    w = rng.standard_normal((rows, D)).astype(np.float32)
    table = torch.zeros((big, D), device=dev, requires_grad=True)
    (embed_sum(t(tk, device=dev), table, t(negate, device=dev), 3) * t(w, device=dev)).sum().backward()
    ref, bound, cnt = ER.reference(tk, w, big, negate, 3)
    ER.check(table.grad.cpu().numpy(), ref, bound, cnt, "torch road")
    assert not table.grad[3].any()


@pytest.mark.parametrize("ignore", [None, 0])
def test_op_against_fp64_autograd(dev, ignore):
    """embed_sum(...).backward against fp64 autograd through table[tokens].sum(1) * sign; forward bits are gvqa_embed_sum's."""
    from graphvqa_amd.sg_encoder import embed_sum
    rng = np.random.default_rng(13)
    rows, T, V, D = 500, 5, 40, 36
    tk = rng.integers(0, V, (rows, T)).astype(np.int64)
    tk[:, 3:] = 0
    negate = (rng.random(rows) < 0.3).astype(np.uint8)
    tab = rng.standard_normal((V, D)).astype(np.float32)
    w = rng.standard_normal((rows, D)).astype(np.float32)
    table = t(tab, device=dev).requires_grad_(True)
    tokens = t(tk, device=dev)
    out = embed_sum(tokens, table, t(negate, device=dev), ignore)
    (out * t(w, device=dev)).sum().backward()
    assert tokens.grad is None and not tokens.requires_grad
    rt = t(tab).double().requires_grad_(True)
    sign = 1.0 - 2.0 * t(negate).double()
    rout = rt[t(tk)].sum(1) * sign.view(-1, 1)
    (rout * t(w).double()).sum().backward()
    assert float((out.detach().cpu().double() - rout.detach()).abs().max()) < 1e-5
    rg = rt.grad.clone()
    if ignore is not None:
        rg[ignore] = 0
    ref, bound, cnt = ER.reference(tk, w, V, negate, -1 if ignore is None else ignore)
    assert np.allclose(ref, rg.numpy(), rtol=0, atol=1e-9)
    ER.check(table.grad.cpu().numpy(), ref, bound, cnt, f"op ignore={ignore}")
    # negate as bool, no negate, and a table that needs no gradient
    out2 = embed_sum(tokens, table.detach(), t(negate, device=dev).bool(), ignore)
    assert not out2.requires_grad and torch.equal(out2, out.detach())
    with pytest.raises(ValueError):
        embed_sum(tokens, table, None, V)


def _gqa_like_batch(seed=21):
    """~300 nodes in four ragged graphs; every node has a self-loop edge with the token SELF (a quarter of all edges), the other edges
    random inside their graph; 1-4 real tokens per node, then pad 0; some edges in added_sym_edge."""
    rng = np.random.default_rng(seed)
    sizes, V, SELF = [120, 7, 93, 80], 50, 3
    N = sum(sizes)
    batch = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    src, dst, etok = [], [], []
    for b, n in enumerate(sizes):
        m = 3 * n
        src.append(first[b] + rng.integers(0, n, m)); dst.append(first[b] + rng.integers(0, n, m)); etok.append(rng.integers(4, V, m))
        src.append(first[b] + np.arange(n)); dst.append(first[b] + np.arange(n)); etok.append(np.full(n, SELF))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    e_tok = np.concatenate(etok).astype(np.int64).reshape(-1, 1)
    perm = rng.permutation(ei.shape[1])
    ei, e_tok = ei[:, perm], e_tok[perm]
    x_tok = np.zeros((N, 12), dtype=np.int64)
    for r in range(N):
        k = 1 + int(rng.integers(0, 4))
        x_tok[r, :k] = rng.integers(1, V, k)
    added = np.sort(rng.choice(ei.shape[1], 37, replace=False)).astype(np.int64)
    assert (e_tok[:, 0] == SELF).sum() * 4 == e_tok.shape[0]
    return x_tok, e_tok, ei, batch, added, len(sizes), V


@functools.lru_cache(maxsize=None)
def _encoder_reference():
    from oracle import ref_torch as R
    from tests.util import tparams
    x_tok, e_tok, ei, batch, added, B, V = _gqa_like_batch()
    D = 64
    N, E = x_tok.shape[0], ei.shape[1]
    w1, w2 = synth.normal((N, D), 86), synth.normal((E, D), 87)
    pe = synth.encoder_params(V, D, seed=3)
    rp = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in tparams(pe).items()}
    rxe, ree = R.scene_graph_encoder(t(x_tok), t(ei), t(e_tok), t(added), t(batch), B, rp)
    ((rxe * t(w1).double()).sum() + (ree * t(w2).double()).sum()).backward()
    grads = {k: v.grad.clone() for k, v in rp.items() if isinstance(v, torch.Tensor) and v.requires_grad and v.grad is not None}
    grads["sg_vocab_embedding.weight"][0] = 0                                   # nn.Embedding(padding_idx=0)
    return pe, w1, w2, rxe.detach(), ree.detach(), grads


@pytest.mark.parametrize("road", ["hip", "torch"])
def test_encoder_gradients_on_both_roads(dev, road, monkeypatch):
    """Every parameter gradient of the encoder on a GQA-shaped batch against fp64 autograd through the oracle, with the bound of
    test_config1_pipeline_end_to_end_gradients (5e-4 of the gradient's scale with its floor); the pad row exactly zero."""
    import types
    from graphvqa_amd import sg_encoder
    x_tok, e_tok, ei, batch, added, B, V = _gqa_like_batch()
    pe, w1, w2, rxe, ree, rgrads = _encoder_reference()
    D = 64
    monkeypatch.setattr(sg_encoder, "_FORCE_TORCH_EMBED_BACKWARD", road == "torch")
    calls = []
    real = sg_encoder._lib.load().gvqa_embed_sum_backward
    monkeypatch.setattr(sg_encoder._lib.load(), "gvqa_embed_sum_backward", lambda *a: (calls.append(a[6]), real(*a))[1])
    enc = sg_encoder.GroundTruth_SceneGraph_Encoder(V, 0, D)
    enc.load_state_dict({k: t(v) for k, v in pe.items()})
    enc.to(dev).eval()
    data = types.SimpleNamespace(x=t(x_tok, device=dev), edge_attr=t(e_tok, device=dev), edge_index=t(ei, device=dev),
                                 batch=t(batch, device=dev), added_sym_edge=t(added, device=dev))
    xe, ee, _ = enc(data)
    ((xe * t(w1, device=dev)).sum() + (ee * t(w2, device=dev)).sum()).backward()
    assert sorted(calls) == ([] if road == "torch" else [-1, 0])                 # node call ignores the pad id, the edge call nothing
    assert float((xe.detach().cpu().double() - rxe).abs().max()) < 1e-4 and float((ee.detach().cpu().double() - ree).abs().max()) < 1e-4
    floor = 1e-3 * max(float(g.abs().max()) for g in rgrads.values())
    bad = {}
    for k, v in enc.named_parameters():
        rg = rgrads[k]
        e = float((v.grad.detach().cpu().double() - rg).abs().max()) / max(float(rg.abs().max()), floor, 1e-12)
        if not e < 5e-4:
            bad[k] = e
    assert not bad, bad
    assert not enc.sg_vocab_embedding.weight.grad[0].any()
