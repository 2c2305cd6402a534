"""GPU: cos_flat_search_f32_batch, the exhaustive scan of a FullPrecisionFP collection, masked or not.  The yardstick is the oracle's
exhaustive mode over STORAGE_F32 (on the sub-corpus of live rows for a mask, tests/flat_masked.py): counts, ids and score bits are
compared for equality.  The device generates candidates on the f32 MFMA and re-scores them in the reference's order
(kernels_flat_f32.hip): a k step is 8 dims, a panel 128, the query fragments stay in registers up to 512."""
import ctypes as C
import functools
from unittest import mock

import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_masked as FM
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _index(X, storage=O.STORAGE_F32, built=False):
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3, ef_construction=32, ef_search=32), ca.DistanceMetric.Cosine,
                      ca.StorageType(ca.StorageKind(storage), 0), seed=11).upload_vectors(X)
    return ix.build(1024) if built else ix               # delete() wants the graph


def _oracle(X, Q, top_k):
    p = O.HNSWParams(dim=X.shape[1], metric=O.METRIC_COSINE, storage=O.STORAGE_F32, num_layers=3)
    return O.OracleIndex(p).set_vectors(X).flat_search_batch(Q, top_k, threads=8)


@functools.lru_cache(maxsize=None)
def _world(dim, n, B):
    """a clustered mixture with tight clusters of about 1000 rows, every row scaled by its own factor: the norms matter"""
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


def _bound(dim):
    """flat_plan.h f32_margin_bound, restated"""
    return 2.0 * ((dim + dim // 8 + 32) + 8) * 2.0 ** -24


# (5, 100, 1, 13): under one k step, pool not full | (75, 3000, 70, 102): a tail that is no whole step, stride != 4 dim, P = 1024,
# partial query tile | (139, 20000, 70, 12): a second panel, past the seed chunk: thresholds, fused appends, a partial last row tile |
# (512, 20000, 1, 1): four resident panels, the widest resident row | (513, 20000, 5, 12): one dim past it, fragments re-read per step
SHAPES = [(5, 100, 1, 13), (75, 3000, 70, 102), (139, 20000, 70, 12), (512, 20000, 1, 1), (513, 20000, 5, 12)]


@pytest.mark.parametrize("dim,n,B,top_k", SHAPES)
def test_parity_with_the_oracle(dim, n, B, top_k):
    X, Q = _world(dim, n, B)
    got = _index(X).flat_search_f32(Q, top_k, with_stats=True)
    FM.same(got, _ref(dim, n, B, top_k))
    st = got[3]
    assert st.pool == _pool(top_k) and st.queries == B and st.tiles_scanned == st.tiles_total == (n + 63) // 64 * ((B + 127) // 128)
    assert st.gemm_launches >= 2 if n > 16384 else st.gemm_launches == 1


def _masked_ref(X, Q, masks, qm, top_k):
    """query b's answer: the oracle over X[masks[qm[b]]].  subset_flat's storage table gets its FullPrecisionFP row for these calls only:
    other test files are parametrised over the table"""
    with mock.patch.dict(FM.STORAGES, {"f32": (O.STORAGE_F32, 0)}):
        per = {g: FM.subset_flat(X, Q, "f32", masks[g], top_k) for g in np.unique(qm)}
    return tuple(np.stack([per[qm[b]][i][b] for b in range(Q.shape[0])]) for i in range(3))


@pytest.mark.parametrize("kind", ["one_percent", "four_masks", "deleted", "few_and_none"])
@pytest.mark.parametrize("dim,n,B,top_k", [SHAPES[2], SHAPES[4]])
def test_masked_parity_with_the_oracle_on_the_live_rows(dim, n, B, top_k, kind):
    X, Q = _world(dim, n, B)
    rng = np.random.default_rng(5)
    masks, qm, dele = (rng.random((1, n)) < 0.01), np.zeros(B, int), None
    if kind == "four_masks":
        masks, qm = np.stack([rng.random(n) < k for k in (0.5, 0.9, 0.02, 2.0)]), np.arange(B) % 4
    elif kind == "deleted":
        dele = np.unique(np.concatenate([rng.integers(0, n, 300), [0, n - 1]])).astype(np.uint32)
        masks = np.ones((1, n), bool)
        masks[0, dele] = False
    elif kind == "few_and_none":                          # fewer live rows than top_k, none, every row
        masks = np.zeros((3, n), bool)
        masks[0, rng.choice(n, top_k - 1, replace=False)] = True
        masks[2] = True
        qm = np.arange(B) % 3
    ref = _masked_ref(X, Q, masks, qm, top_k)
    ix = _index(X, built=dele is not None)
    if dele is not None:
        ix.delete(dele)
    got = ix.flat_search_f32(Q, top_k, None if dele is not None else masks, None if dele is not None else qm, skip_deleted=dele is not None,
                             with_stats=True)
    FM.same(got, ref, what=kind)
    assert np.array_equal(got[2], np.minimum(top_k, masks.sum(axis=1)[qm])), kind
    st = got[3]
    assert st.tiles_total == (n + 63) // 64 * ((B + 127) // 128) and st.tiles_scanned <= st.tiles_total
    if kind == "one_percent":
        assert 0 < st.tiles_scanned < st.tiles_total


@pytest.mark.parametrize("n,lo_row", [(3000, 0), (20000, 16384)])   # one score-matrix chunk | every copy arrives through the fused epilogue
def test_copies_around_the_cut_and_only_they_take_the_exact_path(n, lo_row):
    dim, B, top_k, copies = 64, 12, 10, 200
    N, P = 5 * top_k, _pool(top_k)
    X, Q = _world(dim, n, B)
    X, rng = X.copy(), np.random.default_rng(6)

    def cosines(X):                                       # float64: what the margin rule is about
        X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
        return (Q64 @ X64.T) / (np.linalg.norm(Q64, axis=1)[:, None] * np.linalg.norm(X64, axis=1)[None, :])
    nth = int(np.argsort(-cosines(X)[0])[N - 1])          # the row at query 0's cut ...
    X[lo_row + rng.choice(n - lo_row, copies, replace=False)] = X[nth]   # ... 200 times: more copies than the P - N the pool has to spare
    s = -np.sort(-cosines(X), axis=1)
    flagged = (s >= s[:, N - 1:N] - _bound(dim)).sum(axis=1) > P   # more rows within the bound of the N-th than the pool holds
    assert flagged[0] and not flagged.all(), "premise: query 0's cut lies among the copies, another query's does not"
    # soundness: a query the rule must trust has no row outside the best P within the bound of its N-th — by twice the rule's own margin
    assert (s[~flagged, N - 1] - s[~flagged, P - 1] > 4.0 * _bound(dim)).all(), "premise"
    ref, ix = _oracle(X, Q, top_k), _index(X)
    for mode in (1, 2):
        got = ix.flat_search_f32(Q, top_k, exact_mode=mode, with_stats=True)
        FM.same(got, ref, what=mode)
        assert got[3].exact_queries == (flagged.sum() if mode == 1 else B), mode
    assert ix.flat_search_f32(Q, top_k, exact_mode=0, with_stats=True)[3].exact_queries == 0


def test_refusals_leave_the_handle_usable():
    import cosdata_amd as ca
    from cosdata_amd import _lib
    dim, n, B, top_k = 75, 3000, 70, 5
    X, Q = _world(dim, n, B)
    ref, ix = _ref(dim, n, B, top_k), _index(X)
    Z, Qz, live = X.copy(), Q.copy(), np.ones(n, bool)
    Z[1234], Qz[3], live[1234] = 0, 0, False
    zix = _index(Z)

    def bad_struct_size():
        ids, sc, cnt = np.zeros((B, top_k), np.uint32), np.zeros((B, top_k), np.float32), np.zeros(B, np.uint32)
        opts = _lib.CosFlatF16Opts(struct_size=4, exact_mode=1)
        _lib.check(_lib.lib().cos_flat_search_f32_batch(ix._h, Q.ctypes.data, B, top_k, None, C.byref(opts), ids.ctypes.data, sc.ctypes.data,
                                                        cnt.ctypes.data, None))
    refusals = [(lambda: _index(X, O.STORAGE_U8).flat_search_f32(Q, top_k), 1),
                (lambda: _index(X, O.STORAGE_F16).flat_search_f32(Q, top_k), 1),
                (lambda: ix.flat_search_f32(Q, 0), 3),
                (lambda: ix.flat_search_f32(Q, top_k, exact_mode=3), 3),
                (bad_struct_size, 3),
                (lambda: ix.flat_search_f32(Q, top_k, live, np.full(B, 1)), 3),          # a query names a mask that is not there
                (lambda: ix.flat_search_f32(Q, 103), 4),
                (lambda: ix.flat_search_f32(Qz, top_k), 2),
                (lambda: zix.flat_search_f32(Q, top_k), 2),
                (lambda: zix.flat_search_f32(Q, top_k, np.ones(n, bool)), 2),
                (lambda: ix.flat_search(Q, top_k), 4)]                                    # the code scan keeps refusing f32 rows
    for call, status in refusals:
        with pytest.raises(ca.CosdataError) as ei:
            call()
        assert ei.value.status == status
        FM.same(ix.flat_search_f32(Q, top_k), ref, what=status)
    # a zero-norm row that no query of the call can see is no error
    FM.same(zix.flat_search_f32(Q, top_k, live), _masked_ref(Z, Q, live[None, :], np.zeros(B, int), top_k), what="dead zero row")
