"""GPU: cos_flat_search_f16_batch, the exhaustive scan over HalfPrecisionFP rows.  Every assertion is bit-exact against the oracle's
flat_search_batch on the same index — counts, ids, score bits.  The oracle scores every row with dot_product_f16's sequential chain; the
device generates candidates on the f16 MFMA and re-scores them in that order (kernels_flat_f16.hip)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import near_copies as NC

pytestmark = pytest.mark.gpu


def _index(X, storage=O.STORAGE_F16):
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType(ca.StorageKind(storage), 0))
    return ix.upload_vectors(X)


def _oracle(X, Q, top_k):
    p = O.HNSWParams(dim=X.shape[1], storage=O.STORAGE_F16, num_layers=3)
    ref = O.OracleIndex(p).set_vectors(X).flat_search_batch(Q, top_k, threads=8)
    assert (ref[2] == min(top_k, X.shape[0])).all()
    return ref


def _same(got, ref, what=None):
    for g, r in zip(got[:3], ref):
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(r).view(np.uint32)), what


@functools.lru_cache(maxsize=None)
def _mixture(n, dim, B):
    X = H.clustered_corpus(n, dim, n_centers=20, seed=3)
    return X, H.queries_from(X, B, noise=0.05, seed=8)


# (dim, n, B, top_k): dim 8 less than one MFMA k step | 72 a k tail of 8 on the x8 form, a row stride that is not 2 * dim | 136 a tail
# after whole steps | 1024 the workload's width, four resident panels | 1100 fragments re-read per step.  n 100: the pool is not full |
# 3000 unfused only | 20000 past FLAT_SEED: thresholds, fused appends, a partial last row tile.  B 70: a partial query tile.
# top_k 1, 12, 13, 102: P = 64, 128, 256, 1024
SHAPES = [(8, 100, 1, 13), (72, 3000, 70, 102), (136, 20000, 70, 12), (1024, 20000, 1, 1), (1024, 3000, 70, 13), (1100, 20000, 5, 12)]


@pytest.mark.parametrize("dim,n,B,top_k", SHAPES)
def test_scan_matches_oracle(dim, n, B, top_k):
    X, Q = _mixture(n, dim, B)
    got = _index(X).flat_search_f16(Q, top_k, with_stats=True)
    _same(got, _oracle(X, Q, top_k))
    st = got[3]
    assert (st.queries, st.pool) == (B, next(p for p in (64, 128, 256, 512, 1024) if 10 * top_k <= p))
    assert st.gemm_launches >= (2 if n > 16384 else 1) and st.gemm_ms > 0


def f16_margin_bound(dim):
    """flat_plan.h f16_margin_bound, restated"""
    return 2.0 * (2 * dim + 2) * 2.0 ** -24


def test_modes_agree_and_ordinary_data_stays_on_the_mfma():
    n, dim, B, top_k = 20000, 64, 70, 10
    X, Q = _mixture(n, dim, B)
    # the premise: the N-th and P-th of the oracle's own quantized scores lie more than four bounds apart for every query
    xh, qh = X.astype(np.float16).astype(np.float64), Q.astype(np.float16).astype(np.float64)
    s = -np.sort(-(qh @ xh.T) / (np.linalg.norm(Q.astype(np.float64), axis=1)[:, None] * np.linalg.norm(X.astype(np.float64), axis=1)[None, :]), axis=1)
    assert (s[:, 5 * top_k - 1] - s[:, 127] > 4 * f16_margin_bound(dim)).all()
    ref, ix = _oracle(X, Q, top_k), _index(X)
    for mode in (0, 1, 2):
        got = ix.flat_search_f16(Q, top_k, exact_mode=mode, with_stats=True)
        _same(got, ref, mode)
        assert got[3].exact_queries == (B if mode == 2 else 0), mode


# more than P - N = 78 scaled copies of one row: unfused, and (scaled by powers of two) every copy arriving through the fused epilogue
@pytest.mark.parametrize("case", [(3000, 96, 200, "scaled", 0), (20000, 64, 300, "pow2", 16000)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_near_copies_take_the_exact_path(case):
    X, Q, _ = NC.corpus(case)
    ref, ix = _oracle(X, Q, 10), _index(X)
    for mode in (1, 2):
        got = ix.flat_search_f16(Q, 10, exact_mode=mode, with_stats=True)
        _same(got, ref, mode)
        assert 0 < got[3].exact_queries <= NC.NQ and (mode == 1 or got[3].exact_queries == NC.NQ), mode


def test_refusals_leave_the_handle_usable():
    import cosdata_amd as ca
    X, Q = _mixture(3000, 72, 70)
    with pytest.raises(ca.CosdataError) as ei:
        _index(X, O.STORAGE_U8).flat_search_f16(Q, 5)
    assert ei.value.status == 1
    ix = _index(X)
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search_f16(Q, 103)
    assert ei.value.status == 4
    Z = X.copy()
    Z[1234] = 0
    with pytest.raises(ca.CosdataError) as ei:
        _index(Z).flat_search_f16(Q, 5)
    assert ei.value.status == 2
    Qz = Q.copy()
    Qz[3] = 0
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search_f16(Qz, 5)
    assert ei.value.status == 2
    _same(ix.flat_search_f16(Q, 5), _oracle(X, Q, 5))


def test_warm_handle_equals_a_cold_one():
    """a wide call, a narrow one, then new vectors on the same handle: each the answer of a cold handle (the oracle's)"""
    X, Q = _mixture(3000, 72, 70)
    ix = _index(X)
    _same(ix.flat_search_f16(Q, 102), _oracle(X, Q, 102))
    _same(ix.flat_search_f16(Q[:5], 3), _oracle(X, Q[:5], 3))
    Y = H.clustered_corpus(5000, 72, n_centers=20, seed=9)
    ix.upload_vectors(Y)
    _same(ix.flat_search_f16(Q, 12), _oracle(Y, Q, 12))
