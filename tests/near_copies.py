"""Shared by test_oracle_near_copies.py (CPU) and test_gpu_brute_near_copies.py (GPU): corpora that hold hundreds of copies and
near-copies of one row, the cases the brute force is given on them, and the conditions that make such a corpus a test — more rows
within the scores' error of the k-th score than the survivor pool holds, so that a pool cut by the GEMM's order cannot be trusted.
References (the oracle's answers) are computed once per process and never changed."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from tests import helpers as H
from tests import odd_dims as OD

KINDS = ("exact", "pow2", "scaled", "mixed")
AIMED = 8           # the first eight queries look at the copied row
NQ = 12


def pool_width(k):
    """flat_plan.h brute_pool: the smallest of 64, 128, ..., 1024 keys that holds 2k"""
    return next(p for p in (64, 128, 256, 512, 1024) if 2 * k <= p)


def margin_bound(dim):
    """flat_plan.h brute_margin_bound, restated (tests/cxx/flat_plan_check.cpp pins the header to the same numbers): what the library
    takes for |GEMM score - exact score|"""
    return 2.0 * ((dim + dim // 8 + 32) + 8) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def near_copy_corpus(n, dim, copies, kind, seed=5, lo_row=0):
    """-> X [n][dim], Q [12][dim], rows: `copies` rows at or past lo_row replaced by base * s, base = row 17 of the clustered corpus"""
    assert kind in KINDS
    X = H.clustered_corpus(n, dim, n_centers=20, seed=3)
    base = X[17].copy()
    rng = np.random.default_rng(seed)
    rows = lo_row + rng.choice(n - lo_row, copies, replace=False)
    if kind == "exact":
        s = np.ones(copies, np.float32)
    elif kind == "pow2":
        s = (2.0 ** rng.integers(-3, 4, copies)).astype(np.float32)
    elif kind == "scaled":
        s = rng.uniform(0.5, 2.0, copies).astype(np.float32)
    else:
        s = np.concatenate([np.ones(copies // 2, np.float32), rng.uniform(0.5, 2.0, copies - copies // 2).astype(np.float32)])
    X[rows] = base[None, :] * s[:, None]
    Q = np.concatenate([base[None, :] + np.float32(0.02) * rng.standard_normal((6, dim)).astype(np.float32), base[None, :],
                        np.float32(2.0) * base[None, :], H.queries_from(X, 4, noise=0.05, seed=8)]).astype(np.float32)
    X.setflags(write=False)
    Q.setflags(write=False)
    rows.setflags(write=False)
    return X, Q, rows


# (n, dim, copies, kind, lo_row, k)
UNFUSED = [(3000, 96, 200, kind, 0, k) for kind in KINDS for k in (1, 10, 32)]          # P = 64, one score-matrix chunk
NO_FLOAT4 = [(3000, 97, 200, "scaled", 0, 10)]                                          # rows that are not 16-byte aligned
WIDE = [(3000, 100, 400, "scaled", 0, 33), (3000, 100, 400, "scaled", 0, 64), (4000, 96, 1500, "scaled", 0, 512)]   # P = 128, 128, 1024
FUSED = [(20000, 64, 300, "scaled", 16000, 10), (20000, 64, 300, "mixed", 16000, 32),   # every copy arrives through the fused epilogue
         (20000, 64, 300, "scaled", 0, 10)]                                             # copies on both sides of the seed
ALL_TIE = [(20000, 64, 20000, "exact", 0, 10), (20000, 64, 20000, "exact", 0, 64), (5000, 64, 5000, "scaled", 0, 10)]
MASKED = (3000, 96, 200, "scaled", 0, 10)
SHARDED = (3000, 96, 200, "mixed", 0, 10)
SHARD_SIZES = [1033, 1100, 867]
CASES = UNFUSED + NO_FLOAT4 + WIDE + FUSED + ALL_TIE        # MASKED and SHARDED are UNFUSED corpora at k = 10: among them already


# The recipe's seed is 5.  With EVERY row a scaled copy, seed 5 leaves only 5 of the 8 aimed queries with two score bit patterns in their
# top 10 (test_oracle_near_copies.py asks for 6): that corpus takes another seed, the first that meets the condition
SEED_OF = {(5000, 64, 5000, "scaled", 0): 6}


def corpus(case):
    """the corpus of a case, or of its first five entries (n, dim, copies, kind, lo_row) -> X, Q, rows"""
    n, dim, copies, kind, lo_row = case[:5]
    return near_copy_corpus(n, dim, copies, kind, seed=SEED_OF.get(tuple(case[:5]), 5), lo_row=lo_row)


def case_id(c):
    n, dim, copies, kind, lo_row, k = c
    return f"{n}x{dim}-{copies}{kind}{'-from%d' % lo_row if lo_row else ''}-k{k}"


@functools.lru_cache(maxsize=None)
def _oracle_at_widest(n, dim, copies, kind, lo_row):
    X, Q, _ = corpus((n, dim, copies, kind, lo_row))
    kmax = max(c[5] for c in CASES if c[:5] == (n, dim, copies, kind, lo_row))
    return O.bruteforce_topk(X, Q, kmax, threads=8)


def oracle_topk(case):
    """the oracle sorts every exact score and cuts at k: its answer at k is the first k columns of its answer at a larger k"""
    ids, sc = _oracle_at_widest(*case[:5])
    return ids[:, :case[5]], sc[:, :case[5]]


def masks_for(case):
    """two masks over the MASKED corpus: [0] removes every second copy, [1] leaves at most k - 3 rows in all (k - 5 copies and rows 3 and n - 1)"""
    n, _, copies, _, _, k = case
    _, _, rows = corpus(case)
    half = np.ones(n, bool)
    half[np.sort(rows)[::2]] = False
    few = np.zeros(n, bool)
    few[np.sort(rows)[:k - 5]] = True
    few[[3, n - 1]] = True
    return np.stack([half, few])


def rows_near_kth(X, Q, k, live=None):
    """per query: how many (live) rows have a float64 cosine within 2 * bound_a (odd_dims.py) of the query's k-th best"""
    c = OD.cos64(X, Q)
    out = []
    for b in range(Q.shape[0]):
        cb = c[b] if live is None else c[b][live]
        xb = X if live is None else X[live]
        kth = np.sort(cb)[-k]
        out.append(int((np.abs(cb - kth) <= 2.0 * OD.bound_a(xb, Q[b][None, :])).sum()))
    return np.array(out)


def kth_to_pth_gap(X, Q, k):
    """per query: float64 score of rank k minus that of rank P = pool_width(k) (1-based ranks; n >= P)"""
    c = -np.sort(-OD.cos64(X, Q), axis=1)
    return c[:, k - 1] - c[:, pool_width(k) - 1]


# the ordinary corpora (Gaussian mixtures) on which no query may leave the MFMA path: (n, dim, B) and the k's that fit
ORDINARY = [((3000, 96, 37), (10, 33, 512)), ((5001, 100, 5), (10, 33, 512)), ((20000, 65, 130), (10, 33, 512))]
