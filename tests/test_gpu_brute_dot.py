"""GPU: cos_bruteforce_topk_dot — the exact top k by inner product over the raw f32 rows — against numpy in float64.

Exact data: integer entries in -8 .. 8, every corpus row times a power of two from 2^-3 .. 2^3.  Every product and partial sum is a
multiple of 2^-3 below 2^24 (dim <= 1100), so the f32 dot is exact in any summation order and equals the float64 one: ids, score bits
and counts are compared for equality.  The row scales make the inner-product ranking differ from the cosine ranking, and integer data
is full of ties: the tie rule (larger id first) and the margin rule's exact pass are both exercised."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def bound_c(dim):
    """flat_plan.h brute_margin_bound: |MFMA dot - reference-order dot| <= c |q| |x|"""
    return 2.0 * ((dim + dim // 8 + 32) + 8) * U


def exact_data(dim, n, B, seed, negative=False):
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, (n, dim)).astype(np.float64)
    Q = rng.integers(-8, 9, (B, dim)).astype(np.float64)
    if negative:                                                      # every score <= 0: the best is the least negative
        X, Q = -np.abs(X), np.abs(Q)
    X *= 2.0 ** rng.integers(-3, 4, (n, 1))
    return X.astype(np.float32), Q.astype(np.float32)


def expected(X, Q, k, live=None):
    """float64 top k per query by (score descending, larger id first) over the live rows -> ids, scores (f32), counts"""
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    B, n = S.shape
    ids, sc, cnt = np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32), np.zeros(B, np.uint32)
    for b in range(B):
        rows = np.arange(n) if live is None else np.flatnonzero(live[b])
        order = rows[np.lexsort((-rows, -S[b, rows]))][:k]
        cnt[b] = order.size
        ids[b, :order.size], sc[b, :order.size] = order, S[b, order]
    return ids, sc, cnt


def same(got, ref):
    ids, sc, cnt = ref
    assert np.array_equal(got[2], cnt)
    for b in range(ids.shape[0]):
        c = int(cnt[b])
        assert np.array_equal(got[0][b, :c], ids[b, :c]), b
        assert np.array_equal(got[1][b, :c].view(np.uint32), sc[b, :c].view(np.uint32)), b


def index(X, lo=-64.0, hi=64.0):
    import cosdata_amd as ca
    return ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=2), ca.DistanceMetric.DotProduct, values_range=(lo, hi)).upload_vectors(X)


@pytest.mark.parametrize("dim,n,B,k,negative", [
    (8, 100, 1, 1, False),          # less than one K panel; pool not full
    (70, 3000, 70, 33, False),      # dim % 4 != 0; partial query tile; unfused only; P = 128
    (136, 20000, 70, 12, False),    # past the seed chunk: thresholds, fused appends, partial last row tile; P = 64
    (1100, 20000, 5, 512, False),   # P = 1024; many panels
    (136, 20000, 70, 12, True),     # pools whose every score is negative
])
def test_matches_float64(dim, n, B, k, negative):
    X, Q = exact_data(dim, n, B, 3, negative)
    ix = index(X)
    got = ix.bruteforce_topk_dot(Q, k)
    same(got, expected(X, Q, k))
    assert not np.array_equal(ix.bruteforce_topk(Q, k)[0], got[0])    # a call wired to the cosine kernels fails here


@pytest.mark.parametrize("dim,n,B,k", [(70, 3000, 70, 33), (136, 20000, 70, 12)])
def test_masks_and_deleted_rows(dim, n, B, k):
    X, Q = exact_data(dim, n, B, 5)
    rng = np.random.default_rng(6)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.02, np.zeros(n, bool)])
    masks[2, rng.choice(n, k - 3, replace=False)] = True              # fewer than k live rows
    qm = rng.integers(0, 3, B).astype(np.uint32)
    qm[:3] = (0, 1, 2)
    ix = index(X).build(1024)
    full = expected(X, Q, k)
    dele = np.unique(np.concatenate([full[0][:20, 0], rng.integers(0, n, 20).astype(np.uint32)]))
    ix.delete(dele)
    gone = np.zeros(n, bool)
    gone[dele] = True
    same(ix.bruteforce_topk_dot(Q, k, masks, qm, skip_deleted=True), expected(X, Q, k, masks[qm] & ~gone))
    same(ix.bruteforce_topk_dot(Q, k, skip_deleted=True), expected(X, Q, k, np.broadcast_to(~gone, (B, n))))
    same(ix.bruteforce_topk_dot(Q, k), full)                          # the unmasked call still sees the deleted rows


def real_data(dim, n, B, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, dim)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    return X, rng.standard_normal((B, dim)).astype(np.float32)


def check_real(got, X, Q, k):
    """ids = the float64 top k; scores within c |q| |x| of the float64 dot"""
    ids, sc, _ = expected(X, Q, k)
    assert np.array_equal(got[0], ids)
    S = np.take_along_axis(Q.astype(np.float64) @ X.astype(np.float64).T, ids.astype(np.int64), 1)
    tol = bound_c(X.shape[1]) * np.linalg.norm(Q.astype(np.float64), axis=1)[:, None] * np.linalg.norm(X.astype(np.float64), axis=1)[ids]
    assert np.all(np.abs(got[1].astype(np.float64) - S) <= tol)


def test_exact_knob_and_a_stale_row_norm_maximum():
    from cosdata_amd import _lib
    dim, n, B, k, P = 136, 20000, 8, 12, 64
    X, Q = real_data(dim, n, B, 11)
    Q[:, 0] = 0.0
    S = np.sort(Q.astype(np.float64) @ X.astype(np.float64).T, axis=1)[:, ::-1]
    qn, xn = np.linalg.norm(Q.astype(np.float64), axis=1), np.linalg.norm(X.astype(np.float64), axis=1)
    # the premises, from float64 alone: the rule passes every query (rank k and rank P lie twice its gap apart), and neighbouring
    # ranks of the answer lie further apart than the errors of two reference-order dots together ((dim / 8 + 16) u |q| |x| each:
    # flat_plan.h), so the order of the returned f32 scores is the float64 order
    assert np.all(S[:, k - 1] - S[:, P - 1] > 4 * bound_c(dim) * qn * xn.max())
    assert np.all(S[:, :k] - S[:, 1:k + 1] > 2 * (dim // 8 + 16) * U * qn[:, None] * xn.max())
    ix = index(X, -8.0, 8.0)
    for mode, exact_queries in ((0, 0), (1, 0), (2, B)):
        with _lib.tuning(flat_brute_exact=mode):
            check_real(ix.bruteforce_topk_dot(Q, k), X, Q, k)
        st = ix.last_brute_stats()
        assert (st.queries, st.exact_queries, st.pool) == (B, exact_queries, P)
    # warm handle: one row of the next corpus is huge (and orthogonal to every query: it scores 0), so with ITS maximum the rule
    # trusts no pool.  A maximum kept from the first corpus would still pass them all.
    X2 = X.copy()
    X2[7] = 0.0
    X2[7, 0] = 2.0 ** 30
    ix.upload_vectors(X2)
    check_real(ix.bruteforce_topk_dot(Q, k), X2, Q, k)
    assert ix.last_brute_stats().exact_queries == B


def test_near_copies_take_the_exact_pass():
    dim, n, B, k = 136, 20000, 70, 12                                 # P = 64: more than P - k rows tie with the k-th score
    X, Q = exact_data(dim, n, B, 7)
    rng = np.random.default_rng(8)
    base = rng.integers(-8, 9, dim).astype(np.float32)
    where = rng.choice(np.arange(1, n), 100, replace=False)
    X[where[:70]] = base * 4                                          # 70 rows with one score, the best for the query `base`
    X[where[70:]] = base * 2
    Q[:4] = base
    ix = index(X)
    same(ix.bruteforce_topk_dot(Q, k), expected(X, Q, k))
    assert ix.last_brute_stats().exact_queries >= 4


def test_refusals_leave_the_handle_usable():
    from cosdata_amd import _lib
    X, Q = exact_data(70, 3000, 4, 9)
    ix = index(X)
    for k in (0, 3001, 513):
        with pytest.raises(_lib.CosdataError) as err:
            ix.bruteforce_topk_dot(Q, k)
        assert err.value.status == _lib.ERR_INVALID
    ids, sc = np.zeros((4, 5), np.uint32), np.zeros((4, 5), np.float32)
    sm = _lib.CosScanMask(C.sizeof(_lib.CosScanMask), _lib.SCAN_SKIP_DELETED, 0, None, None)
    rc = _lib.lib().cos_bruteforce_topk_dot(ix._h, Q.ctypes.data, 4, 5, C.byref(sm), ids.ctypes.data, sc.ctypes.data, None)
    assert rc == _lib.ERR_INVALID
    same(ix.bruteforce_topk_dot(Q, 5), expected(X, Q, 5))
