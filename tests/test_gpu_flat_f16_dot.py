"""GPU: cos_flat_search_f16_dot_batch, the exhaustive scan of a HalfPrecisionFP collection with the dot-product metric, masked or not.
The yardstick is the oracle's exhaustive mode under METRIC_DOT (on the sub-corpus of live rows for a mask, tests/flat_masked.py):
counts, ids and score bits are compared for equality.  The rows carry their own scales, so the f16 dot ranking is not the cosine one."""
import functools
from unittest import mock

import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_masked as FM
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _index(X, storage=O.STORAGE_F16, metric=O.METRIC_DOT, built=False):
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3, ef_construction=32, ef_search=32), ca.DistanceMetric(metric),
                      ca.StorageType(ca.StorageKind(storage), 0), seed=11).upload_vectors(X)
    return ix.build(1024) if built else ix               # delete() wants the graph


def _oracle(X, Q, top_k, metric=O.METRIC_DOT):
    p = O.HNSWParams(dim=X.shape[1], metric=metric, storage=O.STORAGE_F16, num_layers=3)
    return O.OracleIndex(p).set_vectors(X).flat_search_batch(Q, top_k, threads=8)


@functools.lru_cache(maxsize=None)
def _world(dim, n, B):
    """a clustered mixture, every row scaled by its own factor in [0.5, 2].  Tight clusters of about 1000 rows: among a query's cluster
    mates the dot ranks by scale and the cosine does not, so the best 5 * top_k rows by dot leave out rows that the cosine ranks first"""
    X = H.clustered_corpus(n, dim, n_centers=max(1, n // 1000), sigma=0.3 / np.sqrt(dim), seed=3)
    X = X * np.random.default_rng(4).uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    Q = H.queries_from(X, B, noise=0.5 / np.sqrt(dim), seed=8)
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


@functools.lru_cache(maxsize=None)
def _ref(dim, n, B, top_k):
    return _oracle(*_world(dim, n, B), top_k)


def _pool(top_k):
    return next(p for p in (64, 128, 256, 512, 1024) if 10 * top_k <= p)


def _f16_dots(X, Q):
    """float64 dots of the f16 codes, |q^| and X^max: what the margin rule is about"""
    X16, Q16 = X.astype(np.float16).astype(np.float64), Q.astype(np.float16).astype(np.float64)
    return Q16 @ X16.T, np.linalg.norm(Q16, axis=1), np.linalg.norm(X16, axis=1).max()


def _bound(dim, qn, xmax):
    """flat_plan.h f16_dot_margin_bound, restated"""
    return 4.0 * dim * 2.0 ** -24 * qn * xmax


# (8, 100, 1, 13): under one k step, pool not full | (72, 3000, 70, 102): x8 tail, stride != 2 dim, P = 1024, partial query tile |
# (136, 20000, 70, 12): tail after whole steps, past the seed chunk: thresholds, fused appends, a partial last row tile |
# (1024, 20000, 1, 1): four resident panels | (1100, 20000, 5, 12): fragments re-read per step
SHAPES = [(8, 100, 1, 13), (72, 3000, 70, 102), (136, 20000, 70, 12), (1024, 20000, 1, 1), (1100, 20000, 5, 12)]


@pytest.mark.parametrize("dim,n,B,top_k", SHAPES)
def test_parity_with_the_oracle(dim, n, B, top_k):
    X, Q = _world(dim, n, B)
    ref = _ref(dim, n, B, top_k)
    assert not np.array_equal(ref[0], _oracle(X, Q, top_k, O.METRIC_COSINE)[0]), "the dot ranking must differ from the cosine one"
    got = _index(X).flat_search_f16_dot(Q, top_k, with_stats=True)
    FM.same(got, ref)
    st = got[3]
    assert st.pool == _pool(top_k) and st.queries == B and st.tiles_scanned == st.tiles_total == (n + 63) // 64 * ((B + 127) // 128)
    assert st.gemm_launches >= 2 if n > 16384 else st.gemm_launches == 1


def _masked_ref(X, Q, masks, qm, top_k):
    """query b's answer: the oracle over X[masks[qm[b]]].  subset_flat's storage table gets its HalfPrecisionFP row for these calls only:
    other test files are parametrised over the table"""
    with mock.patch.dict(FM.STORAGES, {"f16": (O.STORAGE_F16, 0)}):
        per = {g: FM.subset_flat(X, Q, "f16", masks[g], top_k, metric=O.METRIC_DOT) for g in np.unique(qm)}
    return tuple(np.stack([per[qm[b]][i][b] for b in range(Q.shape[0])]) for i in range(3))


@pytest.mark.parametrize("kind", ["one_percent", "four_masks", "deleted", "few_and_none"])
@pytest.mark.parametrize("dim,n,B,top_k", [SHAPES[2], SHAPES[3]])
def test_masked_parity_with_the_oracle_on_the_live_rows(dim, n, B, top_k, kind):
    X, Q = _world(dim, n, B)
    rng = np.random.default_rng(5)
    masks, qm, skip, dele = (rng.random((1, n)) < 0.01), np.zeros(B, int), False, None
    if kind == "four_masks":
        masks, qm = np.stack([rng.random(n) < k for k in (0.5, 0.9, 0.02, 2.0)]), np.arange(B) % 4
    elif kind == "deleted":
        dele = np.unique(np.concatenate([rng.integers(0, n, 300), [0, n - 1]])).astype(np.uint32)
        masks = np.ones((1, n), bool)
        masks[0, dele] = False
    elif kind == "few_and_none":                          # fewer live rows than top_k (where top_k allows it), none, every row
        masks = np.zeros((3, n), bool)
        masks[0, rng.choice(n, top_k - 1, replace=False)] = True
        masks[2] = True
        qm = np.arange(B) % 3 if B > 1 else np.ones(B, int)
    ref = _masked_ref(X, Q, masks, qm, top_k)
    ix = _index(X, built=dele is not None)
    if dele is not None:
        ix.delete(dele)
    got = ix.flat_search_f16_dot(Q, top_k, None if dele is not None else masks, None if dele is not None else qm, skip_deleted=dele is not None,
                                 with_stats=True)
    FM.same(got, ref, what=kind)
    live = masks.sum(axis=1)[qm]
    assert np.array_equal(got[2], np.minimum(top_k, live)), kind
    st = got[3]
    assert st.tiles_total == (n + 63) // 64 * ((B + 127) // 128) and st.tiles_scanned <= st.tiles_total
    if kind == "one_percent":
        assert 0 < st.tiles_scanned < st.tiles_total


def test_ordinary_data_stays_on_the_mfma_path():
    dim, n, B, top_k = 64, 20000, 70, 10
    X, Q = _world(dim, n, B)
    N, P = 5 * top_k, _pool(top_k)
    d, qn, xmax = _f16_dots(X, Q)
    d = -np.sort(-d, axis=1)
    assert (d[:, N - 1] - d[:, P - 1] > 4.0 * _bound(dim, qn, xmax)).all(), "premise: ranks N and P lie four bounds apart"
    ref, ix = _ref(dim, n, B, top_k), _index(X)
    for mode in (0, 1, 2):
        got = ix.flat_search_f16_dot(Q, top_k, exact_mode=mode, with_stats=True)
        FM.same(got, ref, what=mode)
        assert got[3].exact_queries == (B if mode == 2 else 0), mode


@pytest.mark.parametrize("n,lo_row", [(3000, 0), (20000, 16384)])   # one score-matrix chunk | every copy arrives through the fused epilogue
def test_near_copies_around_the_cut_take_the_exact_path(n, lo_row):
    dim, B, top_k, copies = 64, 12, 10, 200
    N, P = 5 * top_k, _pool(top_k)
    X, Q = _world(dim, n, B)
    X, rng = X.copy(), np.random.default_rng(6)
    best = int(np.argmax(_f16_dots(X, Q[:1])[0][0]))      # the row with query 0's largest dot ...
    C = np.repeat(X[best].astype(np.float16)[None, :], copies, axis=0)
    j, cols = rng.integers(0, dim, copies), np.arange(copies)
    C[cols, j] = np.nextafter(C[cols, j], np.where(rng.random(copies) < 0.5, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    X[lo_row + rng.choice(n - lo_row, copies, replace=False)] = C.astype(np.float32)   # ... 200 times, one coordinate one f16 ulp away
    d, qn, xmax = _f16_dots(X, Q)
    near = (np.abs(d[0] - np.sort(d[0])[-N]) <= _bound(dim, qn[0], xmax)).sum()
    assert near > P - N, "premise: more rows within the bound of the cut than the pool has to spare"
    ref, ix = _oracle(X, Q, top_k), _index(X)
    for mode in (1, 2):
        got = ix.flat_search_f16_dot(Q, top_k, exact_mode=mode, with_stats=True)
        FM.same(got, ref, what=mode)
        assert 0 < got[3].exact_queries <= B if mode == 1 else got[3].exact_queries == B


def test_refusals_leave_the_handle_usable():
    import cosdata_amd as ca
    dim, n, B, top_k = 72, 3000, 70, 5
    X, Q = _world(dim, n, B)
    ref, ix = _ref(dim, n, B, top_k), _index(X)
    refusals = [(lambda: _index(X, O.STORAGE_U8).flat_search_f16_dot(Q, top_k), 1),
                (lambda: _index(X, metric=O.METRIC_COSINE).flat_search_f16_dot(Q, top_k), 4),
                (lambda: ix.flat_search_f16_dot(Q, 103), 4),
                (lambda: ix.flat_search_f16_dot(Q, top_k, exact_mode=3), 3),
                (lambda: ix.flat_search_f16(Q, top_k), 4),                          # the cosine calls keep refusing the dot metric
                (lambda: ix.flat_search_f16_masked(Q, top_k, np.ones(n, bool)), 4)]
    for call, status in refusals:
        with pytest.raises(ca.CosdataError) as ei:
            call()
        assert ei.value.status == status
        FM.same(ix.flat_search_f16_dot(Q, top_k), ref, what=status)
