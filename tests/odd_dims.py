"""Shared by test_oracle_odd_dims.py (CPU) and test_gpu_odd_dims.py (GPU): the dimensions off the vector-aligned case, the corpora,
and a second opinion that does not pass through the oracle — the float64 cosine of the raw vectors in numpy."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests import helpers as H

# odd, below 16, one off a power of two / off a 64-byte chunk: every dim % 8 in 1..7, dim % 16, % 32, % 64, % 128 != 0
D = [1, 2, 3, 5, 7, 9, 13, 15, 17, 31, 33, 63, 65, 127, 129, 255, 257, 769, 1023]
WALK_DIMS = [2, 3, 5, 7, 9, 13, 15, 17, 31, 33, 63, 65, 127, 129, 255, 257]

STORAGES = [("u8", O.STORAGE_U8, 0), ("bin", O.STORAGE_SUBBYTE, 1), ("q2", O.STORAGE_SUBBYTE, 2), ("oct", O.STORAGE_SUBBYTE, 3),
            ("f16", O.STORAGE_F16, 0), ("f32", O.STORAGE_F32, 0)]

U = 2.0 ** -24  # unit roundoff of f32

# cos_bruteforce_topk (n, dim, B, k): the last three go past the 16384-candidate seed chunk (the fused epilogue)
BRUTE_CASES = [(3000, 3, 37, 10), (5001, 13, 5, 32), (700, 33, 300, 1), (20000, 65, 130, 10), (70000, 97, 37, 10), (40000, 769, 70, 10)]
BRUTE_BORROWED = (20000, 96, 37, 10)     # dim % 4 == 0 on a table whose base is 4 bytes off a 16-byte boundary


def scale_of(storage):
    return 0.9 if storage == O.STORAGE_SUBBYTE else 1.0      # SubByte levels are hard-wired to [-1, 1): keep the corpus inside


def walk_corpus(kind, n, dim, storage):
    X = H.uniform_corpus(n, dim, seed=7 + dim) if kind == "uniform" else H.clustered_corpus(n, dim, n_centers=24, seed=5 + dim)
    return X * np.float32(scale_of(storage))


def walk_queries(X, dim, storage, nq=12):
    return np.concatenate([H.queries_from(X, nq - 4, seed=3), H.uniform_corpus(4, dim, seed=99) * np.float32(scale_of(storage))])


def brute_corpus(n, dim, B):
    X = H.clustered_corpus(n, dim, n_centers=20, seed=3)
    return X, H.queries_from(X, B, noise=0.05, seed=8)


def cos64(X, Q):
    """[B][n] float64 cosine of the raw f32 vectors"""
    x, q = X.astype(np.float64), Q.astype(np.float64)
    return (q @ x.T) / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None, :])


def bound_a(x, q):
    """|s - cos64| <= (dim/8 + 16) u * sum|x_i q_i| / (|x||q|) + 4u for ONE pair of f32 vectors: the 8-chain f32 dot
    (dim/8 fused steps per chain, a 3-deep tree, the scalar tail), two norms and a divide; u = 2^-24.  Derived, not tuned."""
    x, q = x.astype(np.float64), q.astype(np.float64)
    dim = x.shape[-1]
    return (dim / 8 + 16) * U * np.abs(x * q).sum(axis=-1) / (np.linalg.norm(x, axis=-1) * np.linalg.norm(q, axis=-1)) + 4 * U


def assert_scores_within_bound(X, Q, ids, scores, counts=None, what=""):
    """(a): every returned score is the float64 cosine of (raw row, raw query) within bound_a; returns the worst error / bound"""
    worst = 0.0
    n = X.shape[0]
    for b in range(Q.shape[0]):
        c = ids.shape[1] if counts is None else int(counts[b])
        if c == 0:
            continue
        rows = ids[b, :c].astype(np.int64)
        assert (rows < n).all(), f"{what}: query {b}: an id outside the corpus"
        x = X[rows]
        ref = (x.astype(np.float64) @ Q[b].astype(np.float64)) / (np.linalg.norm(x.astype(np.float64), axis=1) * np.linalg.norm(Q[b].astype(np.float64)))
        bnd = bound_a(x, Q[b][None, :])
        err = np.abs(scores[b, :c].astype(np.float64) - ref)
        assert (err <= bnd).all(), f"{what}: query {b}: score off the float64 cosine by {err.max():.3e}, bound {bnd[err.argmax()]:.3e}"
        worst = max(worst, float((err / bnd).max()))
    return worst


def float64_topk_excused(X, Q, ids, k):
    """(b): ids [B][k] must be the float64 top k (cosine descending, larger id first).  A query whose list differs is excused only
    when two float64 scores next to each other among ranks 0 .. k (the k returned and the first one left out) are closer than
    bound_a of either; anything else fails.  Returns the number of excused queries."""
    c = cos64(X, Q)
    n = X.shape[0]
    excused = 0
    for b in range(Q.shape[0]):
        order = np.lexsort((-np.arange(n), -c[b]))[:k + 1]            # cosine descending, then id descending
        if np.array_equal(order[:k].astype(np.uint32), ids[b]):
            continue
        s = c[b, order]
        bnd = bound_a(X[order], Q[b][None, :])
        gap = s[:-1] - s[1:]
        near = gap < np.maximum(bnd[:-1], bnd[1:])
        assert near.any(), (f"query {b}: ids {ids[b].tolist()} are not the float64 top {k} {order[:k].tolist()} and no two scores "
                            f"around the returned ranks are within the bound (smallest gap {gap.min():.3e}, bound {bnd.max():.3e})")
        excused += 1
    return excused
