"""GPU: BM25 search on a shard set (cos_shardset_attach_bm25, cos_shardset_bm25_search_batch), every shard on device 0.

Shard s holds the postings of its own documents under LOCAL ids.  The set's answer must be, bit for bit (counts, ids, score bits),
the answer of ONE index over the whole collection: oracle.bm25_search on the collection's CSR and one cos_bm25 handle created from
it.  The corpus, the expected answers and the CPU restatements of the two inexact schemes are tests/shardset_text_world.py; the
preconditions (per-shard search + merge differs for >= 30 of the 37 queries at top_k 10: measured 37; the collection's idf with
per-shard buckets for >= 20 at top_k 60: measured 26) are asserted on the CPU at the top of the first test."""
import threading

import numpy as np
import pytest

from tests import shardset_text_world as W

pytestmark = pytest.mark.gpu

OK, INVALID, UNIMPLEMENTED, NOT_READY = 0, 3, 4, 6
_cache = {}


def _set(bounds, bm, doc_bases=None):
    from cosdata_amd.shardset import ShardSet
    return ShardSet(W.dense_stubs(bounds)).attach_bm25(bm, doc_bases)


def _shared():
    """the pristine 3-shard set and the whole-collection handle (no test updates them)"""
    if "shared" not in _cache:
        bm = W.bm_shards(W.BOUNDS3)
        _cache["shared"] = (_set(W.BOUNDS3, bm), bm, W.whole_handle())
    return _cache["shared"]


# ---- 1. the collection's answer at every top_k ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [10, 60, 200, 512])
def test_set_equals_the_whole_collection(top_k):
    W.assert_world_shape()
    W.assert_preconditions()
    w = W.world()
    ss, _, whole = _shared()
    exp = W.whole_expected(top_k)
    got = ss.bm25_search(w.q_terms, w.q_off, top_k)
    W.same(got, exp, f"set vs oracle, top_k {top_k}")
    one = whole.search_batch(w.q_terms, w.q_off, top_k)
    W.same(one, exp, f"single handle vs oracle, top_k {top_k}")
    W.same_arrays(got, one, f"set vs single handle, top_k {top_k}")
    if top_k >= 60:                                       # a top_k above a query's number of non-empty buckets: the count is the buckets'
        assert (got[2] < top_k).any() and got[2].max() == min(top_k, max(e[0].size for e in W.whole_expected(512)))
    found = np.concatenate([got[0][i, :got[2][i]] for i in range(W.NQ)])      # (slots past the count hold whatever the buffer held)
    assert {int(np.searchsorted(W.BOUNDS3, i, side="right")) for i in found} == {1, 2, 3}          # every shard contributes


# ---- 2. edge queries ------------------------------------------------------------------------------------------------------------------------
def test_edge_queries():
    w = W.world()
    ss, _, whole = _shared()
    tables = [set(w.csr(W.BOUNDS3[s], W.BOUNDS3[s + 1])[0].tolist()) for s in range(3)]
    only_one = [t for t in w.terms.tolist() if sum(t in tb for tb in tables) == 1]
    assert only_one, "no term lives in exactly one shard"
    common = next(t for t in w.terms.tolist() if all(t in tb for tb in tables))
    queries = [[only_one[0]],                                   # a term present in exactly one shard
               [only_one[-1], common],
               [common, int(W.UNKNOWN)],                        # a term hash in no shard, beside a known one
               [int(W.UNKNOWN), int(W.UNKNOWN) - 2],            # none of the terms exists: count 0
               [common, only_one[0], common]]                   # a term repeated inside one query: applied twice
    qt = np.array([t for q in queries for t in q], np.uint32)
    qo = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.uint32)
    for top_k in (10, 512):
        exp = W.expected(w.csr(0, W.N), W.N, qt, qo, top_k)
        got = ss.bm25_search(qt, qo, top_k)
        W.same(got, exp, f"edge queries vs oracle, top_k {top_k}")
        W.same_arrays(got, whole.search_batch(qt, qo, top_k), f"edge queries vs single handle, top_k {top_k}")
        assert got[2][3] == 0 and got[2][0] > 0


# ---- 3. a second layout: 8 shards, bases multiples of 512; B = 1 -----------------------------------------------------------------------------
def test_eight_shards_and_a_single_query():
    w = W.world()
    bm = W.bm_shards(W.BOUNDS8)
    ss = _set(W.BOUNDS8, bm, doc_bases=np.array(W.BOUNDS8[:-1], np.uint32))       # explicit bases (equal to the dense shards' id_base)
    for top_k in (10, 200):
        W.same(ss.bm25_search(w.q_terms, w.q_off, top_k), W.whole_expected(top_k), f"8 shards, top_k {top_k}")
    for i in (0, 17, 36):
        got = ss.bm25_search(w.query(i), np.array([0, w.query(i).size], np.uint32), 60)
        W.same(got, [W.whole_expected(60)[i]], f"8 shards, B = 1, query {i}")
    ss.close()


# ---- 4. updates on the shard handles ---------------------------------------------------------------------------------------------------------
def test_inserts_and_deletes_on_the_shard_handles():
    bm, whole = W.bm_shards(W.BOUNDS3), W.whole_handle()
    ss = _set(W.BOUNDS3, bm)
    qt, qo = W.update_queries()
    n_before = whole.stats()["documents_count"]
    W.apply_updates(bm, whole, 0)
    assert whole.stats()["documents_count"] == n_before + W.N_EXTRA
    th, off, di, tf, tomb = whole.download()
    assert not tomb.any()
    for top_k in (10, 60, 512):
        got = ss.bm25_search(qt, qo, top_k)
        W.same_arrays(got, whole.search_batch(qt, qo, top_k), f"after the insert, top_k {top_k}")
        W.same(got, W.expected((th, off, di, tf), W.N + W.N_EXTRA, qt, qo, top_k), f"after the insert vs oracle, top_k {top_k}")
    assert (got[0][got[2] > 0, 0] >= W.N).any()           # the inserted documents are found
    W.apply_updates(bm, whole, 1)
    st = whole.stats()
    assert st["documents_count"] == W.N + W.N_EXTRA - 350 and st["tombstones"] > 0      # N falls, the tombstones stay in the lists
    assert sum(b.stats()["postings"] for b in bm) == st["postings"]                    # ... and still count in len
    for top_k in (10, 60, 512):
        W.same_arrays(ss.bm25_search(qt, qo, top_k), whole.search_batch(qt, qo, top_k), f"after the deletes, top_k {top_k}")
    ss.close()


# ---- 5. the 64-term rule ----------------------------------------------------------------------------------------------------------------------
def test_more_than_64_matching_terms_over_the_shards():
    """65 distinct known terms, no shard holding more than 40 of them: the set refuses like the whole index, and answers afterwards"""
    import cosdata_amd as ca
    terms = (np.arange(90, dtype=np.uint32) * 7 + 11)
    held = [terms[0:40], terms[25:65], terms[50:90]]              # shard s holds these terms; every term of [0, 65) is in some shard
    rng = np.random.default_rng(9)
    bounds, per_doc = [0, 600, 1300, 2000], []
    for s in range(3):
        for d in range(bounds[s], bounds[s + 1]):
            per_doc.append(np.sort(rng.choice(held[s], 3, replace=False)))
    doc = np.repeat(np.arange(2000, dtype=np.uint32), 3)
    hs = np.concatenate(per_doc).astype(np.uint32)
    tf = rng.uniform(0.2, 2.2, doc.size).astype(np.float32)

    def csr(lo, hi):
        m = (doc >= lo) & (doc < hi)
        o = np.argsort(hs[m], kind="stable")
        t, c = np.unique(hs[m][o], return_counts=True)
        off = np.zeros(t.size + 1, np.uint64)
        off[1:] = np.cumsum(c)
        return t, off, (doc[m][o] - np.uint32(lo)).astype(np.uint32), tf[m][o]

    bm = [ca.BM25Index(*csr(bounds[s], bounds[s + 1]), bounds[s + 1] - bounds[s]) for s in range(3)]
    whole = ca.BM25Index(*csr(0, 2000), 2000)
    from cosdata_amd.shardset import ShardSet
    ss = ShardSet(W.dense_stubs(bounds)).attach_bm25(bm, np.array(bounds[:-1], np.uint32))
    q65, q64 = terms[:65].copy(), terms[:64].copy()
    assert all(np.isin(q65, h).sum() <= 40 for h in held) and np.isin(q65, np.concatenate(held)).all()
    off = lambda q: np.array([0, q.size], np.uint32)
    before = ss.bm25_search(q64, off(q64), 100)                                     # 64 matching terms: the most that is answered
    W.same_arrays(before, whole.search_batch(q64, off(q64), 100), "64 terms")
    W.same(before, W.expected(csr(0, 2000), 2000, q64, off(q64), 100), "64 terms vs oracle")
    s_set, s_one = W.status(ss.bm25_search, q65, off(q65), 100), W.status(whole.search_batch, q65, off(q65), 100)
    assert s_set == s_one == UNIMPLEMENTED, (s_set, s_one)
    W.same_arrays(ss.bm25_search(q64, off(q64), 100), before, "the call after the refusal")
    ss.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_set_answering():
    from cosdata_amd.shardset import ShardSet
    w = W.world()
    _, bm, whole = _shared()
    ss = ShardSet(W.dense_stubs(W.BOUNDS3))
    assert W.status(ss.bm25_search, w.q_terms, w.q_off, 10) == NOT_READY             # nothing attached
    assert W.status(ss.hybrid_search, np.ones((W.NQ, 8), np.float32), w.q_terms, w.q_off, 10) == NOT_READY
    assert W.status(ss.attach_bm25, bm[:2]) == INVALID                               # wrong n_shards
    assert W.status(ss.attach_bm25, bm, np.array([0, 9000, 9000], np.uint32)) == INVALID          # bases do not strictly increase
    assert W.status(ss.attach_bm25, bm, np.array([0, 10000, 9000], np.uint32)) == INVALID
    assert W.status(ss.attach_bm25, bm, np.array([0, 9000, 0xFFFFFFFF - 1999], np.uint32)) == INVALID   # base + largest id (1999) = u32::MAX
    assert W.status(ss.bm25_search, w.q_terms, w.q_off, 10) == NOT_READY             # a refused attach attaches nothing
    ss.attach_bm25(bm, np.array([0, 9000, 0xFFFFFFFF - 2000], np.uint32))           # ... one below fits
    ss.attach_bm25(bm)
    good = ss.bm25_search(w.q_terms, w.q_off, 10)
    W.same(good, W.whole_expected(10), "after the refused attaches")
    for top_k in (0, 513):                                                          # the single handle's statuses, whatever they are
        s_set, s_one = W.status(ss.bm25_search, w.q_terms, w.q_off, top_k), W.status(whole.search_batch, w.q_terms, w.q_off, top_k)
        assert s_set == s_one, (top_k, s_set, s_one)
        if s_set == OK and top_k:
            W.same_arrays(ss.bm25_search(w.q_terms, w.q_off, top_k), whole.search_batch(w.q_terms, w.q_off, top_k), f"top_k {top_k}")
        W.same_arrays(ss.bm25_search(w.q_terms, w.q_off, 10), good, f"after top_k {top_k}")
    ss.attach_bm25(None)                                                            # detach
    assert W.status(ss.bm25_search, w.q_terms, w.q_off, 10) == NOT_READY
    ss.close()


def test_an_insert_past_a_shards_id_range_is_refused_by_every_search():
    """a global id names one document: the middle shard holds local ids 0 .. 999 (global 9000 .. 9999); a document inserted under local
    id 1000 would be global id 10000, shard 2's first.  Every search of the set then says so, until the bases leave room."""
    w = W.world()
    bm = W.bm_shards(W.BOUNDS3)
    ss = _set(W.BOUNDS3, bm)
    good = ss.bm25_search(w.q_terms, w.q_off, 10)
    u = w.update([W.N])
    bm[1].insert(np.array([W.BOUNDS3[2] - W.BOUNDS3[1]], np.uint32), u[1], u[2], u[3])
    assert W.status(ss.bm25_search, w.q_terms, w.q_off, 10) == INVALID
    assert W.status(ss.hybrid_search, np.ones((W.NQ, 8), np.float32), w.q_terms, w.q_off, 10) == INVALID
    assert W.status(ss.attach_bm25, bm) == INVALID                                  # ... and so does attaching with the same bases
    ss.attach_bm25(bm, np.array([0, 9000, 10001], np.uint32))                       # room for the new document: the set answers again
    moved = ss.bm25_search(w.q_terms, w.q_off, 10)
    assert (good[2] > 0).all() and (moved[2] > 0).all()
    ss.close()


# ---- 7. a search beside an insert ------------------------------------------------------------------------------------------------------------
def test_search_beside_an_insert_sees_before_or_after():
    w = W.world()
    bm, whole = W.bm_shards(W.BOUNDS3), W.whole_handle()
    ss = _set(W.BOUNDS3, bm)
    qt, qo = W.update_queries()
    before = whole.search_batch(qt, qo, 60)
    ids = np.arange(W.N, W.N + W.N_EXTRA)
    whole.insert(*w.update(ids))
    after = whole.search_batch(qt, qo, 60)
    assert not np.array_equal(before[0], after[0])
    answers, errors = [], []

    def searcher():
        try:
            for _ in range(20):
                answers.append(ss.bm25_search(qt, qo, 60))
        except Exception as e:                                                      # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=searcher)
    t.start()
    bm[2].insert(*w.update(ids, W.BOUNDS3[2]))
    t.join()
    assert not errors, errors
    assert len(answers) == 20

    def equal(a, b):
        try:
            W.same_arrays(a, b)
            return True
        except AssertionError:
            return False

    kinds = [equal(a, before) or (2 if equal(a, after) else 0) for a in answers]
    assert all(kinds), kinds                                                       # every answer is the before or the after expectation
    W.same_arrays(ss.bm25_search(qt, qo, 60), after, "after the insert")
    ss.close()
