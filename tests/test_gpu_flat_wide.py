"""Exhaustive scans with survivor pools wider than 64 keys: cos_flat_search_batch at top_k 13 .. 204 (pools of 128 .. 1024 keys,
the smallest that holds the 5 * top_k rerank candidates) and cos_bruteforce_topk at k 33 .. 512 (the smallest that holds 2k).  Every
answer must equal the oracle's (O.OracleIndex.flat_search_batch / O.bruteforce_topk) bit for bit: counts, and the first `count`
ids and scores of every row (scores as uint32 views)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

STORAGES = [(O.STORAGE_U8, 0), (O.STORAGE_SUBBYTE, 2)]
SEED = 16384   # candidates that go through the score matrix (the unfused first chunk)


def pool_width(need):
    """the documented rule: the smallest of 64, 128, ..., 1024 keys that holds `need`"""
    return next(p for p in (64, 128, 256, 512, 1024) if need <= p)


def fused_launches(n, P):
    """scan launches of the documented fused schedule: the seed chunk, then chunks `growth` times everything seen
    (8 for the 64-key pool, 4 for the wider ones), capped at 4 M candidates by the tile kernel only (nothing here comes near it)"""
    if n <= SEED:
        return 1
    growth, seen, launches = (8 if P == 64 else 4), SEED, 1
    while seen < n:
        seen += min(seen * growth, n - seen)
        launches += 1
    return launches


def same(got, ref):
    """counts equal, and the first `count` entries of every row equal (scores bit for bit)"""
    gi, gs, gc = got[:3]
    ri, rs, rc = ref[:3]
    if not np.array_equal(gc, rc):
        return False
    k = gi.shape[1]
    live = np.arange(k)[None, :] < np.asarray(rc)[:, None]
    return np.array_equal(gi[live], ri[live]) and np.array_equal(gs.view(np.uint32)[live], rs.view(np.uint32)[live])


def device_index(X, storage, res, metric=None):
    import cosdata_amd as ca
    kw = {} if metric is None else {"distance_metric": metric}
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType(ca.StorageKind(storage), res), **kw)
    ix.upload_vectors(X)
    return ix


def oracle_index(X, storage, res, metric=O.METRIC_COSINE):
    return O.OracleIndex(O.HNSWParams(dim=X.shape[1], metric=metric, storage=storage, resolution=res, num_layers=3)).set_vectors(X)


def mixed_queries(X, B, seed=8):
    return np.concatenate([H.queries_from(X, B - 2, noise=0.05, seed=seed), H.uniform_corpus(2, X.shape[1], seed=77)])


@functools.lru_cache(maxsize=2)
def _small(storage, res):
    """n = 3001, dim = 100, B = 37 (one ragged query block), n below the seed: the unfused path only"""
    X = H.uniform_corpus(3001, 100, seed=13) * 0.9
    return X, mixed_queries(X, 37), device_index(X, storage, res), oracle_index(X, storage, res)


def test_gate_wide_calls_answer_and_the_limits_refuse():
    import cosdata_amd as ca
    X, Q, ix, oix = _small(O.STORAGE_U8, 0)
    ref10 = oix.flat_search_batch(Q, 10, threads=4)
    assert same(ix.flat_search(Q, 13), oix.flat_search_batch(Q, 13, threads=4))      # refused before wide pools existed
    assert same(ix.flat_search(Q, 204), oix.flat_search_batch(Q, 204, threads=4))
    obi, obs = O.bruteforce_topk(X, Q, 512, threads=4)
    for k in (33, 512):                                                              # refused before wide pools existed
        ids, sc = ix.bruteforce_topk(Q, k)
        assert np.array_equal(ids, obi[:, :k]) and np.array_equal(sc.view(np.uint32), obs[:, :k].view(np.uint32))
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Q, 205)
    assert ei.value.status == 4 and "204" in str(ei.value)
    assert same(ix.flat_search(Q, 10), ref10)
    with pytest.raises(ca.CosdataError) as ei:
        ix.bruteforce_topk(Q, 513)
    assert ei.value.status == 3
    assert same(ix.flat_search(Q, 10), ref10)


@pytest.mark.parametrize("storage,res", STORAGES)
@pytest.mark.parametrize("top_k", [13, 25, 26, 51, 52, 102, 103, 204])
def test_both_edges_of_every_pool_width_unfused(storage, res, top_k):
    """5 * top_k = 65 / 125 | 130 / 255 | 260 / 510 | 515 / 1020: the first and the last top_k of the 128, 256, 512 and 1024 pools"""
    X, Q, ix, oix = _small(storage, res)
    got = ix.flat_search(Q, top_k, with_stats=True)
    assert same(got, oix.flat_search_batch(Q, top_k, threads=4))
    assert got[3].gemm_launches == 1


@functools.lru_cache(maxsize=1)
def _fused(storage, res, dim):
    X = H.clustered_corpus(40000, dim, n_centers=40, sigma=0.2, seed=23)
    return X, device_index(X, storage, res), oracle_index(X, storage, res)


@pytest.mark.parametrize("top_k", [13, 51, 204])
@pytest.mark.parametrize("B", [70, 261])
@pytest.mark.parametrize("dim", [96, 768])
@pytest.mark.parametrize("storage,res", STORAGES)
def test_fused_path_matches_oracle_and_does_not_fall_back(storage, res, dim, B, top_k):
    """n = 40000 > the seed chunk: the rest runs the threshold-filtered scan (at 768 dims the query-resident kernels) and the wide
    append fold.  The launch count is the fused schedule's: a fallback to the unfused path would add its own launches."""
    X, ix, oix = _fused(storage, res, dim)
    Q = mixed_queries(X, B)
    got = ix.flat_search(Q, top_k, with_stats=True)
    assert same(got, oix.flat_search_batch(Q, top_k, threads=8))
    assert got[3].gemm_launches == fused_launches(40000, pool_width(5 * top_k)) == 2


@functools.lru_cache(maxsize=1)
def _rows_once_corpus():
    return H.clustered_corpus(40000, 128, n_centers=40, sigma=0.2, seed=41)


@pytest.mark.parametrize("knobs", [{}, {"flat_tile_kernel": 1}], ids=["default", "tile_kernel"])
@pytest.mark.parametrize("n,launches", [(16384, 1), (16385, 2), (40000, 2)])
@pytest.mark.parametrize("storage,res,row_bytes", [(O.STORAGE_U8, 0, 128), (O.STORAGE_SUBBYTE, 2, 32)])
def test_a_scan_reads_every_row_once(storage, res, row_bytes, n, launches, knobs):
    """The chunks of a scan that does not overflow cover [0, n) exactly once: the code bytes streamed are n rows for the one block of
    256 queries (B = 3; a u8 row of 128 dims is 128 bytes, a quaternary one 2 chunks of 16 = 32; the products are exact in a double),
    and the launches are the schedule's (tests/golden/flat_plan_cases.txt): n = 16384 is the seed chunk alone and not fused, one row
    more is a fused chunk of one row, 40000 = 16384 + 23616.  Query-resident kernels (128 dims has an instantiation) and the tile kernel."""
    from cosdata_amd import _lib
    X = _rows_once_corpus()[:n]
    Q = mixed_queries(X, 3)
    ix = device_index(X, storage, res)
    with _lib.tuning(**knobs):
        got = ix.flat_search(Q, 10, with_stats=True)
    assert got[3].code_bytes == float(n * row_bytes * 1)
    assert got[3].gemm_launches == launches
    assert same(got, oracle_index(X, storage, res).flat_search_batch(Q, 10, threads=4))


@pytest.mark.parametrize("n", [30, 100, 700])
@pytest.mark.parametrize("top_k", [50, 204])
def test_fewer_vectors_than_the_pool(n, top_k):
    X = H.uniform_corpus(n, 48, seed=5) * 0.9
    Q = mixed_queries(X, 9)
    ix, oix = device_index(X, O.STORAGE_U8, 0), oracle_index(X, O.STORAGE_U8, 0)
    got, ref = ix.flat_search(Q, top_k), oix.flat_search_batch(Q, top_k, threads=2)
    assert np.array_equal(got[2], np.full(9, min(n, top_k), np.uint32))
    assert same(got, ref)


@pytest.mark.parametrize("storage,res", STORAGES)
def test_ties_across_both_cuts(storage, res):
    """500 distinct rows, 40 copies each, at shuffled positions: in every ranking the entries come in runs of 40 equal keys, so
    position 5 * top_k of the quantized ranking (65, 510) and position top_k of the reranked one (13, 102) fall inside a run — larger
    id first decides at the pool's boundary, inside the merges (n = 20000: a seed chunk of several segments and a fused chunk) and
    at the output"""
    rng = np.random.default_rng(19)
    base = H.clustered_corpus(500, 64, n_centers=6, sigma=0.3, seed=29) * 0.9
    X = np.ascontiguousarray(base[rng.permutation(np.repeat(np.arange(500), 40))])
    Q = np.concatenate([H.queries_from(base, 7, noise=0.05, seed=3), base[:2]])
    ix, oix = device_index(X, storage, res), oracle_index(X, storage, res)
    for top_k in (13, 102):
        assert same(ix.flat_search(Q, top_k), oix.flat_search_batch(Q, top_k, threads=4)), top_k


@pytest.mark.parametrize("storage,res", STORAGES)
def test_adversarial_order_overflow_or_not_same_answer(storage, res):
    """the corpus of test_flat_code_scan_fused_overflow_falls_back_exactly: every later vector is closer to the query than all
    earlier ones, so everything beats the running threshold; whether or not the append buffer overflows, the answer is the oracle's"""
    n, dim = 60000, 64
    rng = np.random.default_rng(4)
    q = rng.standard_normal(dim).astype(np.float32)
    q /= np.linalg.norm(q)
    noise = rng.standard_normal((n, dim)).astype(np.float32)
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    w = np.linspace(0.0, 1.0, n, dtype=np.float32)[:, None]
    X = (w * q[None, :] + (1.0 - w) * noise).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X *= 0.9
    Q = np.stack([q * 0.9, -q * 0.9, X[100], X[59000]]).astype(np.float32)
    ix, oix = device_index(X, storage, res), oracle_index(X, storage, res)
    for top_k in (50, 204):
        assert same(ix.flat_search(Q, top_k), oix.flat_search_batch(Q, top_k, threads=8)), top_k


@pytest.mark.parametrize("storage,res", STORAGES)
def test_dot_product_metric_wide(storage, res):
    import cosdata_amd as ca
    X = H.clustered_corpus(45000, 384, n_centers=25, sigma=0.25, seed=37) * 0.8
    Q = H.queries_from(X, 70, noise=0.05, seed=5)
    ix = device_index(X, storage, res, metric=ca.DistanceMetric.DotProduct)
    oix = oracle_index(X, storage, res, metric=O.METRIC_DOT)
    assert same(ix.flat_search(Q, 60), oix.flat_search_batch(Q, 60, threads=8))


@pytest.mark.parametrize("storage,res,dim", [(O.STORAGE_SUBBYTE, 2, 768), (O.STORAGE_U8, 0, 512)])
def test_implementations_agree_at_a_wide_width(storage, res, dim):
    """top_k = 102 (512-key pool): the query-resident kernels, the 256 x 128 tile kernel, the score-matrix path and (quaternary) the
    i8-digit kernel feed the same wide selection and return the same arrays"""
    from cosdata_amd import _lib
    X = H.clustered_corpus(50000, dim, n_centers=30, sigma=0.25, seed=31)
    Q = H.queries_from(X, 64, noise=0.05, seed=9)
    ix = device_index(X, storage, res)
    ref = ix.flat_search(Q, 102)
    assert np.array_equal(ref[2], np.full(64, 102, np.uint32))
    knobs = [("flat_tile_kernel", 1), ("flat_unfused", 1)] + ([("flat_fp4", 0)] if storage == O.STORAGE_SUBBYTE else [])
    for name, val in knobs:
        with _lib.tuning(**{name: val}):
            got = ix.flat_search(Q, 102)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)) and np.array_equal(got[2], ref[2]), name


@pytest.mark.parametrize("storage,res", STORAGES)
@pytest.mark.parametrize("dim", [97, 1001])
def test_odd_rows_through_the_wide_rerank(storage, res, dim):
    """rows that are not a multiple of four floats (and so only 4-byte aligned) through the wide rerank kernel"""
    X = H.uniform_corpus(2500, dim, seed=13) * 0.9
    Q = mixed_queries(X, 33)
    ix, oix = device_index(X, storage, res), oracle_index(X, storage, res)
    assert same(ix.flat_search(Q, 51), oix.flat_search_batch(Q, 51, threads=4))


def test_zero_norm_is_still_a_calculation_error_at_a_wide_width():
    import cosdata_amd as ca
    X = H.uniform_corpus(20000, 64, seed=3)
    Q = H.queries_from(X, 6, seed=1)
    ix = device_index(X, O.STORAGE_U8, 0)
    ok = ix.flat_search(Q, 60)
    Qz = Q.copy()
    Qz[3] = -1.0                                               # all-zero u8 code -> |q| = 0
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Qz, 60)
    assert ei.value.status == 2
    again = ix.flat_search(Q, 60)                              # the handle answers afterwards
    assert all(np.array_equal(a, b) for a, b in zip(ok, again))
    X2 = X.copy()
    X2[1234] = -1.0                                            # a zero-norm stored vector
    ix.upload_vectors(X2)
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Q, 60)
    assert ei.value.status == 2
    ix.upload_vectors(X)
    again = ix.flat_search(Q, 60)
    assert all(np.array_equal(a, b) for a, b in zip(ok, again))


@pytest.mark.parametrize("storage,res", STORAGES)
def test_narrow_after_wide_returns_the_same_bits(storage, res):
    """the workspace only grows: a 64-key call on a handle that has served a 1024-key call must index it by its own width"""
    X, ix, oix = _fused(storage, res, 96)
    Q = mixed_queries(X, 70)
    first = ix.flat_search(Q, 10)
    wide = ix.flat_search(Q, 204)
    third = ix.flat_search(Q, 10)
    assert all(np.array_equal(a, b) for a, b in zip(first, third))
    assert same(first, oix.flat_search_batch(Q, 10, threads=8))
    assert same(wide, oix.flat_search_batch(Q, 204, threads=8))


BRUTE_SHAPES = {"unfused": (3000, 96, 37), "fused": (70000, 96, 37), "fused768": (20000, 768, 130), "odd_dim": (5001, 100, 5)}


@functools.lru_cache(maxsize=1)
def _brute(shape):
    import cosdata_amd as ca
    n, dim, B = BRUTE_SHAPES[shape]
    X = H.clustered_corpus(n, dim, n_centers=20, seed=3)
    Q = H.queries_from(X, B, noise=0.05, seed=8)
    ix = ca.HNSWIndex(dim, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType.UnsignedByte())
    ix.upload_vectors(X)
    # the oracle sorts every exact score and cuts at k: its answer at k is the first k columns of its answer at 512
    return Q, ix, O.bruteforce_topk(X, Q, 512, threads=8)


@pytest.mark.parametrize("k", [33, 64, 65, 128, 129, 256, 257, 512])
@pytest.mark.parametrize("shape", list(BRUTE_SHAPES))
def test_bruteforce_wide_matches_oracle(shape, k):
    """both edges of the 128, 256, 512 and 1024 pools (2k = 66 / 128 | 130 / 256 | 258 / 512 | 514 / 1024).  Continuous random data:
    a candidate's GEMM score differs from its reference-order score by a few ulps, so only entries within a few ulps of the k-th exact
    score can change sides, and here the k-th and the P-th score lie thousands of error bounds apart: the pool of P >= 2k holds the
    answer and the margin rule (flat_plan.h brute_margin_safe) flags no query.  Corpora where that is NOT so — more than P - k copies
    or scaled copies of one row — take the library's exact path and are the subject of test_gpu_brute_near_copies.py."""
    Q, ix, (oids, osc) = _brute(shape)
    ids, sc = ix.bruteforce_topk(Q, k)
    assert np.array_equal(ids, oids[:, :k])
    assert np.array_equal(sc.view(np.uint32), osc[:, :k].view(np.uint32))


def test_bruteforce_wide_transpose_detecting():
    """asymmetric inputs (the corpus of test_bruteforce_transpose_detecting) at k = 64: a 128-key pool"""
    import cosdata_amd as ca
    n, dim = 512, 64
    X = np.zeros((n, dim), np.float32)
    for i in range(n):
        X[i, i % dim] = 1.0
        X[i, (i * 7 + 3) % dim] += 0.25 + (i // dim) * 0.01
    Q = np.zeros((200, dim), np.float32)
    for b in range(200):
        Q[b, (b * 5) % dim] = 1.0
        Q[b, (b * 11 + 1) % dim] = 0.1 + 0.001 * b
    ix = ca.HNSWIndex(dim, ca.HNSWHyperParams(num_layers=3))
    ix.upload_vectors(X)
    ids, sc = ix.bruteforce_topk(Q, 64)
    oids, osc = O.bruteforce_topk(X, Q, 64, threads=2)
    assert np.array_equal(ids, oids) and np.array_equal(sc.view(np.uint32), osc.view(np.uint32))
