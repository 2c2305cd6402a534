"""Learned-sparse search that keeps up to 1024 candidates per query (cos_sparse_set_max_candidates; kernels_sparse.hip: the wide
instantiations R = 2, 4, 8, 16 of the scan kernels and sparse_wide_finish_kernel).

Every comparison is on ids, score BITS and counts of every query against the C oracle (oracle.sparse_search + sparse_rerank): the
sums are exact u32, so there is no tolerance anywhere.  The shapes are the ones of tests/test_sparse.py and
tests/test_gpu_sparse_update.py (their helpers are imported, their corpora are built once per module and never changed)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_sparse import _assert_like_oracle, _corpus, _index_with_layout, _queries

pytestmark = pytest.mark.gpu

UPPER = 3.0


def _flat(qs):
    qo = np.cumsum([0] + [len(q[0]) for q in qs]).astype(np.uint32)
    qd = np.concatenate([q[0] for q in qs] + [np.zeros(1, np.uint32)])[:max(int(qo[-1]), 1)]
    qv = np.concatenate([q[1] for q in qs] + [np.zeros(1, np.float32)])[:max(int(qo[-1]), 1)]
    return qd.astype(np.uint32), qv.astype(np.float32), qo


@functools.lru_cache(maxsize=None)
def _parity_corpus(bits):
    """three accumulator tiles (the last one ragged) and several splits per query at 70 queries"""
    return _corpus(n=20000, vocab=600, bits=bits, upper=UPPER, seed=10 + bits)


@functools.lru_cache(maxsize=None)
def _parity_queries():
    return _queries(70, 600, seed=3)


@functools.lru_cache(maxsize=None)
def _parity_ranking(bits, thr):
    """per query EVERY touched vector in the oracle's order (k_with_reranking = 0); its first k entries are what the oracle returns
    for k_with_reranking = k (tests/test_sparse.py::test_oracle_matches_python_restatement holds the oracle to that)"""
    _, dims, key_off, vec_ids, *_ = _parity_corpus(bits)
    return [O.sparse_search(dims, key_off, vec_ids, 20000, bits, UPPER, thr, q[0], q[1]) for q in _parity_queries()]


@pytest.fixture(scope="module")
def parity_index():
    """one handle at 1024 per (layout, bits), shared by the parity cases; closed when the module is done"""
    made = {}

    def get(layout, bits):
        if (layout, bits) not in made:
            _, dims, key_off, vec_ids, row_off, raw_dims, raw_vals = _parity_corpus(bits)
            ix = _index_with_layout(layout, bits, UPPER, dims, key_off, vec_ids, 20000, row_off, raw_dims, raw_vals)
            ix.set_max_candidates(1024)
            made[(layout, bits)] = ix
        return made[(layout, bits)]

    yield get
    for ix in made.values():
        ix.close()


def _refused(ix, args, status):
    import cosdata_amd as ca
    with pytest.raises(ca.CosdataError) as ei:
        ix.search_batch(*args)
    assert ei.value.status == status, ei.value


# ---- 1. the gate ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_gate_default_64_widened_rounded_and_narrowed_again(layout):
    import cosdata_amd as ca
    bits, thr, n = 6, 0.0, 20000
    _, dims, key_off, vec_ids, row_off, raw_dims, raw_vals = _parity_corpus(bits)
    ix = _index_with_layout(layout, bits, UPPER, dims, key_off, vec_ids, n, row_off, raw_dims, raw_vals)
    qs = _parity_queries()
    qd, qv, qo = _flat(qs)
    assert ix.max_candidates == 64
    _refused(ix, (qd, qv, qo, 20, thr, 5), 4)                                  # COS_ERR_UNIMPLEMENTED: 100 candidates > 64
    ix.set_max_candidates(100)
    assert ix.max_candidates == 128
    _assert_like_oracle(ix, dims, key_off, vec_ids, n, bits, UPPER, thr, qs, 20, row_off, raw_dims, raw_vals, 5)
    _refused(ix, (qd, qv, qo, 26, thr, 5), 4)                                  # 130 > 128; the handle stays usable:
    _assert_like_oracle(ix, dims, key_off, vec_ids, n, bits, UPPER, thr, qs, 128)
    for bad in (0, 1025):
        with pytest.raises(ca.CosdataError) as ei:
            ix.set_max_candidates(bad)
        assert ei.value.status == 3                                            # COS_ERR_INVALID
        assert ix.max_candidates == 128
    _assert_like_oracle(ix, dims, key_off, vec_ids, n, bits, UPPER, thr, qs, 20, row_off, raw_dims, raw_vals, 5)
    ix.set_max_candidates(64)
    assert ix.max_candidates == 64
    _refused(ix, (qd, qv, qo, 20, thr, 5), 4)
    _assert_like_oracle(ix, dims, key_off, vec_ids, n, bits, UPPER, thr, qs, 64)
    for want, ask in ((64, 1), (128, 65), (256, 129), (512, 257), (1024, 513), (1024, 1024)):
        assert ix.set_max_candidates(ask).max_candidates == want
    ix.close()


# ---- 2. parity at both edges of every instantiation ------------------------------------------------------------------------------
# (32 R, 64 R] candidates run the instantiation R: 65 | 128 | 129 | 256 | 257 | 512 | 513 | 1024, and widths inside.  With the
# oracle on these corpora: at (6, 0.0) 62 of the 70 queries touch more than 1024 vectors (the cut is exercised) and 8 touch
# 869 .. 1024 (count < top_k is exercised); at (4, 0.5) the split is 30 / 40; at every cut listed most queries have
# equal similarities on both sides of the cut (22 .. 68 over all three corpora), so the larger-id rule decides what is kept.

WIDE_K_RF = [(65, 0), (100, 0), (128, 0), (129, 0), (256, 0), (257, 0), (512, 0), (513, 0), (1000, 0), (1024, 0), (13, 5), (20, 5), (200, 5),
             (1024, 1)]


@pytest.mark.parametrize("k,rf", WIDE_K_RF)
@pytest.mark.parametrize("bits,thr", [(6, 0.0), (4, 0.5), (8, 0.3)])
@pytest.mark.parametrize("layout", [0, 1])
def test_wide_search_matches_oracle(parity_index, layout, bits, thr, k, rf):
    _, dims, key_off, vec_ids, row_off, raw_dims, raw_vals = _parity_corpus(bits)
    ix = parity_index(layout, bits)
    qs = _parity_queries()
    ids, sc, cnt = ix.search_batch(*_flat(qs), k, thr, rf)
    full = _parity_ranking(bits, thr)
    cut = short = 0
    for b, q in enumerate(qs):
        cand, sims = full[b][0][:k * max(rf, 1)], full[b][1][:k * max(rf, 1)]
        if rf == 0:
            eid, esc = cand[:k], sims[:k].astype(np.float32)
        else:
            eid, esc = O.sparse_rerank(row_off, raw_dims, raw_vals, cand, q[0], q[1], top_k=k)
        c = int(cnt[b])
        assert c == len(eid), (b, c, len(eid))
        assert np.array_equal(ids[b, :c], eid), (b, ids[b, :c][:8], eid[:8])
        assert np.array_equal(sc[b, :c].view(np.uint32), np.asarray(esc, np.float32).view(np.uint32)), b
        cut += len(full[b][0]) > k * max(rf, 1)
        short += len(eid) < k
    assert cut > 0, "no query of this case has more candidates than it keeps"
    if k >= 1000:
        assert short > 0, "no query of this case returns fewer than top_k"


# ---- 3. narrow calls on a widened handle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_narrow_calls_do_not_change_on_a_widened_handle(parity_index, layout):
    bits, thr = 6, 0.0
    _, dims, key_off, vec_ids, row_off, raw_dims, raw_vals = _parity_corpus(bits)
    plain = _index_with_layout(layout, bits, UPPER, dims, key_off, vec_ids, 20000, row_off, raw_dims, raw_vals)
    wide = parity_index(layout, bits)
    assert plain.max_candidates == 64 and wide.max_candidates == 1024
    args = _flat(_parity_queries())
    wide.search_batch(*args, 1000, thr, 0)                                     # the wide workspace exists before the narrow calls
    for k, rf in ((10, 0), (64, 0), (12, 5)):
        a = plain.search_batch(*args, k, thr, rf)
        blocks = plain.last_stats().blocks
        b = wide.search_batch(*args, k, thr, rf)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]), (k, rf)
        assert wide.last_stats().blocks == blocks and a[2].max() == k
    plain.close()


# ---- 4. edge cases -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _edge_corpus():
    """tests/test_sparse.py::test_packed_layout_edge_cases_and_repeated_ids: n = 16411 (two full tiles + 27 ids), vocab 90, and the
    ids of dimension 3's key list 10 named again in its key list 12 (the packed accumulator's touch bound fails: flag-word blocks)"""
    bits, n = 6, 16411
    _, dims, key_off, vec_ids, *_ = _corpus(n=n, vocab=90, nnz=10, bits=bits, upper=UPPER, seed=77)
    ko = np.asarray(key_off).reshape(len(dims), (1 << bits) + 1).copy()
    lo, hi = int(ko[3, 10]), int(ko[3, 11])
    extra = vec_ids[lo:hi].copy()
    at = int(ko[3, 13])
    vec_ids = np.concatenate([vec_ids[:at], extra, vec_ids[at:]])
    flat = ko.ravel()
    flat[3 * ((1 << bits) + 1) + 13:] += len(extra)
    d0, d1, d3 = int(dims[0]), int(dims[1]), int(dims[3])
    queries = [(np.array([d0], np.uint32), np.array([0.0], np.float32)),                       # quantizes to 0: every visited vector, similarity 0, order by id alone
               (np.array([100000, 100001], np.uint32), np.array([1.0, 2.0], np.float32)),      # unknown dimensions only
               (np.array([], np.uint32), np.array([], np.float32)),                             # no terms at all
               (np.array([d0, d1, d0], np.uint32), np.array([1.5, 0.7, 0.2], np.float32)),      # the same dimension twice
               (np.array([d3, d1], np.uint32), np.array([2.9, 0.3], np.float32)),               # the repeated ids
               (np.array([d3], np.uint32), np.array([0.001], np.float32))]
    return bits, n, dims, flat.astype(np.uint64), vec_ids, queries


@pytest.mark.parametrize("k", [300, 1000])
@pytest.mark.parametrize("layout", [0, 1])
def test_wide_edge_cases_single_query_launches_zero_weights_repeated_ids(layout, k):
    bits, n, dims, key_off, vec_ids, queries = _edge_corpus()
    ix = _index_with_layout(layout, bits, UPPER, dims, key_off, vec_ids, n)
    ix.set_max_candidates(1024)
    zero = O.sparse_search(dims, key_off, vec_ids, n, bits, UPPER, 0.0, *queries[0], k_with_reranking=k)
    assert len(zero[0]) == k and not zero[1].any() and np.array_equal(zero[0], np.sort(zero[0])[::-1])   # what the first query is for
    for thr in (0.0, 0.6):
        for batch in ([0], [1], [2], [3], [4], [5], [0, 1, 2, 3, 4, 5]):      # one query per launch: a block per tile (splits = n_tiles)
            _assert_like_oracle(ix, dims, key_off, vec_ids, n, bits, UPPER, thr, [queries[i] for i in batch], k)
    ix.close()


# ---- 5. long queries ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _long_corpus():
    """tests/test_sparse.py::test_packed_layout_long_queries_and_table_windows: n = 70000, 8-bit keys, queries of 65 .. 300 terms
    (term groups of 64, table windows, counted and flag-word blocks in one launch; the unpacked kernel's block-wide path)"""
    bits, n, vocab = 8, 70000, 500
    _, dims, key_off, vec_ids, *_ = _corpus(n=n, vocab=vocab, nnz=12, bits=bits, upper=UPPER, seed=5)
    rng = np.random.default_rng(1)
    qs = []
    for m, scale in ((65, 0.05), (130, 2.9), (257, 0.02), (300, 2.5), (64, 2.9), (7, 0.4), (200, 0.0)):
        d = rng.choice(vocab, size=m, replace=False).astype(np.uint32)
        qs.append((d, (scale * (0.5 + rng.random(m))).astype(np.float32)))
    return bits, n, dims, key_off, vec_ids, qs


@pytest.mark.parametrize("k", [200, 1000])
@pytest.mark.parametrize("layout", [0, 1])
def test_wide_long_queries_term_groups_and_table_windows(layout, k):
    bits, n, dims, key_off, vec_ids, qs = _long_corpus()
    ix = _index_with_layout(layout, bits, UPPER, dims, key_off, vec_ids, n)
    ix.set_max_candidates(1024)
    batches = ([0, 1, 2, 3, 4, 5, 6], [3], [1, 5]) if layout else ([0, 1, 2, 3, 4, 5, 6],)
    for thr in (0.0, 0.4):
        for batch in batches:
            _assert_like_oracle(ix, dims, key_off, vec_ids, n, bits, UPPER, thr, [qs[i] for i in batch], k)
    ix.close()


# ---- 6. the setting survives updates -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_wide_search_after_insert_and_delete(layout):
    import cosdata_amd as ca
    from tests.test_sparse_update_model import SparseModel, queries, rows_of, vectors
    bits, n0, m, vocab = 6, 6000, 500, 120
    n = n0 + m
    raw = vectors(n, vocab, 24, seed=31)
    base = rows_of(raw, range(n0))
    csr0 = ca.sparse_build_csr(bits, UPPER, *base)
    ix = _index_with_layout(layout, bits, UPPER, csr0[0], csr0[1], csr0[2], n0, *base)
    ix.set_max_candidates(1024)
    assert ix.insert(*rows_of(raw, range(n0, n))) == n0
    dele = np.random.default_rng(7).choice(n, 300, replace=False)
    gone = rows_of(raw, dele)
    assert ix.delete(dele, *gone) == int(gone[0][-1])
    assert ix.max_candidates == 1024
    # the surviving rows: the deleted vectors keep their ids and hold no pairs
    ro, rd, rv = raw
    lens = np.diff(ro.astype(np.int64))
    keep = np.repeat(~np.isin(np.arange(n), dele), lens)
    lens[dele] = 0
    alive = (np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), rd[keep], rv[keep])
    csr = ca.sparse_build_csr(bits, UPPER, *alive)
    qs = queries(SparseModel.from_csr(bits, UPPER, *csr, n), 32, vocab, seed=9)
    for thr in (0.0, 0.5):
        full = [O.sparse_search(csr[0], csr[1], csr[2], n, bits, UPPER, thr, q[0], q[1]) for q in qs]
        assert sum(len(f[0]) > 1000 for f in full) >= 8 and not any(np.isin(f[0], dele).any() for f in full)
        _assert_like_oracle(ix, csr[0], csr[1], csr[2], n, bits, UPPER, thr, qs, 1000)
        _assert_like_oracle(ix, csr[0], csr[1], csr[2], n, bits, UPPER, thr, qs, 100, alive[0], alive[1], alive[2], 5)
    ix.close()
