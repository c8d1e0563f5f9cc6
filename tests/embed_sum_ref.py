"""Shared by tests/test_embed_sum_backward_host.py and tests/test_gpu_embed_sum_backward.py: the inputs of the table-gradient cases, the
fp64 reference with its a-priori bound, and a numpy restatement of the counting sort + chunked sum (a reference written from the
contract in include/gvqa.h; nothing here imports the package).

The bound: an fp32 sum of n terms in ANY order is within gamma_(n-1) * sum|terms| < n * 2^-23 * sum|terms| of the exact sum (while
n * 2^-24 << 1), so every element obeys |kernel - fp64| <= cnt_v * 2^-23 * sum|terms|, whatever the chunking; rows without occurrences
(and the ignored row) are exactly zero and rows with one occurrence are exact."""
from __future__ import annotations

import numpy as np
import torch


def reference(tokens, dout, V, negate=None, ignore=-1):
    """fp64 index_add_ over the fp32 inputs.  Returns (ref [V, D] fp64, bound [V, D] fp64, cnt [V])."""
    tokens = np.asarray(tokens, dtype=np.int64)
    rows, T = tokens.shape
    D = dout.shape[1]
    ids = torch.from_numpy(np.clip(tokens, 0, V - 1).reshape(-1))
    r = torch.arange(rows).repeat_interleave(T)
    keep = ids != ignore
    ids, r = ids[keep], r[keep]
    g = torch.from_numpy(np.ascontiguousarray(dout)).double()
    if negate is not None:
        g = g * (1.0 - 2.0 * torch.from_numpy(np.asarray(negate).astype(np.float64))).view(-1, 1)      # exact
    terms = g.index_select(0, r)
    ref = torch.zeros((V, D), dtype=torch.float64).index_add_(0, ids, terms)
    absum = torch.zeros((V, D), dtype=torch.float64).index_add_(0, ids, terms.abs())
    cnt = torch.bincount(ids, minlength=V).double()
    bound = cnt.view(-1, 1) * 2.0 ** -23 * absum
    return ref.numpy(), bound.numpy(), cnt.numpy().astype(np.int64)


def check(got, ref, bound, cnt, what=""):
    """got [V, D] fp32 against the reference: within the bound everywhere, exact zeros for cnt = 0, exact for cnt = 1."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - ref)
    over = err > bound
    assert not over.any(), (what, "rows over the bound", np.unique(np.nonzero(over)[0])[:8], float(err[over].max()), float(bound[over].min()))
    assert not got[cnt == 0].any(), (what, "a row without occurrences is not zero")
    one = cnt == 1
    assert np.array_equal(got[one].astype(np.float64), ref[one]), (what, "a row with one occurrence is not exact")


def counts_around_chunk(L, seed=5):
    """T = 1, V = 12, D = 300: token counts exactly 0, 1, 2, L - 1, L, L + 1, 2 L, 2 L + 1, 4 L + 3 (tokens 0 .. 8) and the rest spread over
    tokens 9 .. 11; rows interleaved (a fixed permutation), a quarter negated.  rows = 11 L + 64: the nine counts alone add up to
    11 L + 7, so the 9 L + 64 rows first planned for this case cannot hold them; the counts are kept, the row number follows."""
    rng = np.random.default_rng(seed)
    rows, V, D = 11 * L + 64, 12, 300
    counts = [0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, 4 * L + 3]
    ids = np.concatenate([np.full(c, v, dtype=np.int64) for v, c in enumerate(counts)])
    rest = rows - ids.size
    assert rest > 0
    ids = np.concatenate([ids, rng.integers(9, 12, rest).astype(np.int64)])
    ids = ids[rng.permutation(rows)]
    negate = (rng.random(rows) < 0.25).astype(np.uint8)
    dout = rng.standard_normal((rows, D)).astype(np.float32)
    got = np.bincount(ids, minlength=V)
    assert list(got[:9]) == counts
    return ids.reshape(rows, 1), dout, negate, V


def pad_heavy(seed=6):
    """rows = 37, T = 12, V = 50, D = 300: 1-4 real tokens per row, then pad 0; row 5 repeats a token."""
    rng = np.random.default_rng(seed)
    rows, T, V, D = 37, 12, 50, 300
    tok = np.zeros((rows, T), dtype=np.int64)
    for r in range(rows):
        k = 1 + r % 4
        tok[r, :k] = rng.integers(1, V, k)
    tok[5, :2] = 17
    dout = rng.standard_normal((rows, D)).astype(np.float32)
    return tok, dout, V


def across_slices(S, seed=7):
    """rows T > 3 S at the vocabulary limit V = 8192: token 5 once in every slice, ids past the table (clamped to 8191) only in the last
    slice, a negative id (clamped to 0), everything else from 40 ids: most rows of the table are unused."""
    rng = np.random.default_rng(seed)
    T, V, D = 6, 8192, 68
    rows = (3 * S) // T + 40
    n = rows * T
    assert n > 3 * S
    pool = np.concatenate([rng.integers(6, 8000, 39), [4097]]).astype(np.int64)
    flat = pool[rng.integers(0, pool.size, n)]
    flat[flat == 5] = 6
    ns = -(-n // S)
    for s in range(ns):
        flat[min(s * S + 11 + 3 * s, n - 1)] = 5
    flat[n - 9] = 9000
    flat[n - 2] = 8191
    flat[3] = -7
    assert (flat[: (ns - 1) * S] < 8191).all()
    negate = (rng.random(rows) < 0.3).astype(np.uint8)
    dout = rng.standard_normal((rows, D)).astype(np.float32)
    return flat.reshape(rows, T), dout, negate, V


def counting_sort_chunked_sum(tokens, dout, V, negate, ignore, S, L):
    """The contract's algorithm in numpy, fp32: stable counting sort of the kept occurrences by token through per-slice histograms and a
    scan over (token, slice); chunks of L sorted positions summed in order; runs inside a chunk written directly, a chunk's head / tail
    runs kept as partial rows; a spanning token = tail of its first chunk + heads of the following ones, in chunk order."""
    tokens = np.asarray(tokens, dtype=np.int64)
    rows, T = tokens.shape
    D = dout.shape[1]
    ids = np.clip(tokens, 0, V - 1).reshape(-1)
    n = ids.size
    ns = -(-n // S)
    hist = np.zeros((V, ns), dtype=np.int64)
    for o in range(n):
        if ids[o] != ignore:
            hist[ids[o], o // S] += 1
    base = np.concatenate([[0], np.cumsum(hist.reshape(-1))])
    M = int(base[-1])
    cursor = base[:-1].reshape(V, ns).copy()
    srow, stok = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for o in range(n):
        if ids[o] != ignore:
            p = cursor[ids[o], o // S]
            cursor[ids[o], o // S] += 1
            srow[p], stok[p] = o // T, ids[o]
    start_of = base[:-1].reshape(V, ns)[:, 0]
    end_of = np.concatenate([start_of[1:], [M]])
    sign = np.ones(rows, dtype=np.float32) if negate is None else (1 - 2 * np.asarray(negate).astype(np.float32))
    out = np.full((V, D), np.nan, dtype=np.float32)
    nc = -(-M // L) if M else 0
    head, tail = np.full((max(nc, 1), D), np.nan, dtype=np.float32), np.full((max(nc, 1), D), np.nan, dtype=np.float32)
    for c in range(nc):
        lo, hi = c * L, min((c + 1) * L, M)
        p = lo
        while p < hi:
            q = p
            acc = np.zeros(D, dtype=np.float32)
            while q < hi and stok[q] == stok[p]:
                acc = acc + sign[srow[q]] * dout[srow[q]]
                q += 1
            v = stok[p]
            if p == lo and start_of[v] < lo:
                head[c] = acc
            elif q == hi and end_of[v] > hi:
                tail[c] = acc
            else:
                out[v] = acc
            p = q
    for v in range(V):
        s, e = int(start_of[v]), int(end_of[v])
        if e == s:
            out[v] = 0
        elif s // L != (e - 1) // L:
            acc = tail[s // L].copy()
            for c in range(s // L + 1, (e - 1) // L + 1):
                acc = acc + head[c]
            out[v] = acc
    return out
