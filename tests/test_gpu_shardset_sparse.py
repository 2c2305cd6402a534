"""GPU: learned-sparse search on a shard set (cos_shardset_attach_sparse, cos_shardset_sparse_search_batch), every shard on device 0.

Shard s holds the postings and raw vectors of its own vectors under LOCAL ids.  The set's answer must be, bit for bit (counts, ids,
score bits), the answer of ONE index over the whole collection: oracle.sparse_search + oracle.sparse_rerank on the collection's CSR,
and one cos_sparse handle created from it.  The corpus, the expected answers and the CPU restatement of the inexact scheme are
tests/shardset_sparse_world.py; its preconditions are asserted on the CPU at the top of the first test."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import shardset_sparse_world as W
from tests.shardset_text_world import dense_stubs, status
from tests.test_sparse import _corpus

pytestmark = pytest.mark.gpu

OK, INVALID, UNIMPLEMENTED, NOT_READY = 0, 3, 4, 6
_cache = {}


def _set(bounds, sp, bases=None):
    from cosdata_amd.shardset import ShardSet
    return ShardSet(dense_stubs(bounds)).attach_sparse(sp, bases)


def _shared(bits, bounds, layout=None, max_cand=None):
    """a pristine set and the whole-collection handle per (bits, layout, width) — no test updates them"""
    key = (bits, tuple(bounds), layout, max_cand)
    if key not in _cache:
        w = W.world(bits)
        sp = W.sparse_shards(w, bounds, layout=layout)
        whole = _cache.get(("whole", bits)) or W.whole_handle(w)
        _cache["whole", bits] = whole
        if max_cand:
            for h in sp:
                h.set_max_candidates(max_cand)
        _cache[key] = (_set(bounds, sp), sp, whole)
    ss, sp, whole = _cache[key]
    whole.set_max_candidates(max_cand or 64)
    return ss, sp, whole


def _expected(w, thr, top_k, factor, queries=None):
    return [w.expected(thr, q, top_k, factor) for q in (w.queries if queries is None else queries)]


def _check(ss, whole, w, thr, top_k, factor, what, queries=None):
    qd, qv, qo = w.query_csr(queries)
    got = ss.sparse_search(qd, qv, qo, top_k, thr, factor)
    W.same(got, _expected(w, thr, top_k, factor, queries), f"set vs oracle, {what}")
    if whole is not None:
        qd1, qv1 = (qd, qv) if qd.size else (np.zeros(1, np.uint32), np.zeros(1, np.float32))
        W.same_arrays(got, whole.search_batch(qd1, qv1, qo, top_k, thr, factor), f"set vs single handle, {what}")
    return got


# ---- 1. three shards: the collection's answer at every width of the narrow path --------------------------------------------------------------
@pytest.mark.parametrize("bits,thr,layout", [(6, 0.0, 1), (6, 0.0, 0), (4, 0.5, 1), (8, 0.3, 1)])
def test_three_shards_equal_the_whole_collection(bits, thr, layout):
    W.assert_preconditions()
    w = W.world(bits)
    ss, _, whole = _shared(bits, W.BOUNDS3, layout=layout)
    for top_k, factor in [(10, 0), (10, 5), (1, 0), (12, 5), (64, 0)]:
        got = _check(ss, whole, w, thr, top_k, factor, f"bits {bits} thr {thr} layout {layout} top_k {top_k} factor {factor}")
    found = np.concatenate([got[0][i, :got[2][i]] for i in range(W.NQ)])
    assert {int(np.searchsorted(W.BOUNDS3, i, side="right")) for i in found} == {1, 2, 3}          # every shard contributes


# ---- 2. eight shards, the wide paths -----------------------------------------------------------------------------------------------------------
def test_eight_shards_wide():
    """C = 250: records of 256 slots (R = 4), 2048 gathered keys; some queries have fewer than C candidates in the whole collection"""
    w = W.world(4)
    ss, _, whole = _shared(4, W.BOUNDS8, max_cand=256)
    got = _check(ss, whole, w, 0.5, 50, 5, "8 shards, (50, 5)")
    assert sum(w.touched(0.5, q)[0].size < 250 for q in w.queries) >= 1 and (got[2] == 50).any()
    _check(ss, whole, w, 0.5, 12, 5, "8 shards, (12, 5)")                               # the narrow record behind the same set


@pytest.mark.parametrize("top_k,factor", [(1024, 0), (200, 5)])
def test_eight_shards_widest(top_k, factor):
    """records of 1024 slots (R = 16), 8192 gathered keys: the widest fold"""
    w = W.world(6)
    ss, _, whole = _shared(6, W.BOUNDS8, max_cand=1024)
    _check(ss, whole, w, 0.0, top_k, factor, f"8 shards, ({top_k}, {factor})", queries=w.queries[:4])


# ---- 3. edge queries -----------------------------------------------------------------------------------------------------------------------------
def test_edge_queries():
    w = W.world(6)
    ss, _, whole = _shared(6, W.BOUNDS3)
    f32, u32 = np.float32, np.uint32
    rare = (np.array([7], u32), np.array([0.004], f32))                                # quantizes to 0: every similarity is 0
    edge = [w.queries[5],
            (np.zeros(0, u32), np.zeros(0, f32)),                                       # no pairs: count 0
            (np.array([VOC + 3, VOC + 11], u32), np.array([1.0, 2.0], f32)),           # unknown dimensions only: count 0
            rare,
            (np.array([7, 7], u32), np.array([1.5, 0.5], f32))]                        # a dimension twice in one query
    for top_k, factor in [(10, 0), (10, 5), (64, 0)]:
        got = _check(ss, whole, w, 0.0, top_k, factor, f"edge queries ({top_k}, {factor})", queries=edge)
        assert got[2][1] == 0 and got[2][2] == 0 and got[2][0] > 0
    for i in (0, 17, 39):                                                              # a single query
        _check(ss, whole, w, 0.0, 10, 5, f"B = 1, query {i}", queries=[w.queries[i]])
    _check(ss, whole, w, 0.0, 10, 5, "empty query alone", queries=[edge[1]])


VOC = W.VOCAB + 1000


def test_dimensions_of_one_small_shard_and_top_k_above_the_touched_vectors():
    """a collection of 600 vectors in shards of 200 / 50 / 350: the dimensions 5000 .. 5004 exist in the small middle shard only, in 30
    of its vectors — a query of those dimensions touches 30 vectors, fewer than top_k and than C, all in one shard"""
    bits = 6
    _, _, _, _, ro, rd, rv = _corpus(n=600, vocab=W.VOCAB, bits=bits, upper=W.UPPER, seed=13)
    rng = np.random.default_rng(2)
    rows = [(rd[int(ro[i]):int(ro[i + 1])], rv[int(ro[i]):int(ro[i + 1])]) for i in range(600)]
    for v in range(210, 240):                                                           # (appended dims are larger: rows stay ascending)
        extra = np.sort(rng.choice(np.arange(5000, 5005), 2, replace=False)).astype(np.uint32)
        rows[v] = (np.concatenate([rows[v][0], extra]), np.concatenate([rows[v][1], rng.gamma(1.2, 0.7, 2).astype(np.float32)]))
    raw = (np.cumsum([0] + [d.size for d, _ in rows]), np.concatenate([d for d, _ in rows]), np.concatenate([x for _, x in rows]))
    small = [(np.array([5000, 5003, 5004], np.uint32), np.array([1.0, 0.7, 2.0], np.float32)),
             (np.array([5001, 12, 5002], np.uint32), np.array([0.5, 1.1, 0.9], np.float32))]
    w = W.World(bits, raw=raw, queries=small + W.world(bits).queries[:6])
    bounds = [0, 200, 250, 600]
    sp, whole = W.sparse_shards(w, bounds), W.whole_handle(w)
    ss = _set(bounds, sp)
    for top_k, factor in [(40, 0), (10, 5), (64, 0), (12, 5)]:
        got = _check(ss, whole, w, 0.0, top_k, factor, f"small shard ({top_k}, {factor})")
        ids0 = got[0][0, :got[2][0]]
        assert ((ids0 >= 210) & (ids0 < 240)).all() and got[2][0] == min(top_k, w.touched(0.0, small[0])[0].size)
    assert w.touched(0.0, small[0])[0].size < 40
    ss.close()


# ---- 4. updates on the shard handles -----------------------------------------------------------------------------------------------------------
def _extra(bits, m=300):
    _, _, _, _, ro, rd, rv = _corpus(n=m, vocab=W.VOCAB, bits=bits, upper=W.UPPER, seed=21)
    return ro, rd, rv


def test_inserts_and_deletes_on_the_shard_handles():
    bits, thr = 6, 0.0
    w = W.world(bits)
    sp, whole = W.sparse_shards(w, W.BOUNDS3), W.whole_handle(w)
    ss = _set(W.BOUNDS3, sp)
    qd, qv, qo = w.query_csr()
    before = ss.sparse_search(qd, qv, qo, 10, thr, 5)
    ro, rd, rv = _extra(bits)
    assert sp[2].insert(ro, rd, rv) == W.BOUNDS3[3] - W.BOUNDS3[2]                       # local ids in the last shard
    assert whole.insert(ro, rd, rv) == W.N                                               # ... global ids 6000 .. in the whole handle
    dele = np.arange(1100, 4100, 7)                                                      # global ids of the middle shard
    dro, drd, drv = w.rows_csr(dele)
    assert sp[1].delete(dele - W.BOUNDS3[1], dro, drd, drv) == whole.delete(dele, dro, drd, drv) > 0
    # the collection after the updates, for the oracle: the deleted vectors keep their ids and hold no pairs
    keep = np.ones(W.N, bool)
    keep[dele] = False
    lens = np.concatenate([np.diff(w.row_off).astype(np.int64) * keep, np.diff(ro).astype(np.int64)])
    pair_keep = np.repeat(keep, np.diff(w.row_off).astype(np.int64))
    after = W.World(bits, raw=(np.cumsum(np.concatenate([[0], lens])), np.concatenate([w.raw_dims[pair_keep], rd]), np.concatenate([w.raw_vals[pair_keep], rv])))
    changed = 0
    for top_k, factor in [(10, 0), (10, 5), (64, 0), (12, 5)]:
        got = ss.sparse_search(qd, qv, qo, top_k, thr, factor)
        W.same_arrays(got, whole.search_batch(qd, qv, qo, top_k, thr, factor), f"after the updates ({top_k}, {factor})")
        W.same(got, _expected(after, thr, top_k, factor), f"after the updates vs oracle ({top_k}, {factor})")
        if (top_k, factor) == (10, 5):
            changed = sum(not np.array_equal(got[0][i], before[0][i]) for i in range(W.NQ))
            found = np.concatenate([got[0][i, :got[2][i]] for i in range(W.NQ)])
            assert (found >= W.N).any() and not np.isin(found, dele).any()
    assert changed > 0
    ss.close()


def test_an_insert_past_the_next_base_is_refused_by_every_search():
    """the middle shard holds local ids 0 .. 3199 (global 1000 .. 4199): one more vector would be global id 4200, the last shard's first"""
    w = W.world(6)
    sp = W.sparse_shards(w, W.BOUNDS3)
    ss = _set(W.BOUNDS3, sp)
    qd, qv, qo = w.query_csr()
    good = ss.sparse_search(qd, qv, qo, 10, 0.0, 5)
    ro, rd, rv = _extra(6, m=40)
    sp[1].insert(ro[:2], rd[:int(ro[1])], rv[:int(ro[1])])
    assert status(ss.sparse_search, qd, qv, qo, 10, 0.0, 5) == INVALID
    assert status(ss.sparse_search, qd, qv, qo, 10, 0.0, 0) == INVALID
    arms = np.zeros(W.NQ, np.uint8)                                                      # DENSE_SPARSE: refused before the dense half is enqueued
    assert status(ss.hybrid_search_mixed, arms, np.ones((W.NQ, 8), np.float32), (qd, qv, qo), None, 10) == INVALID
    assert status(ss.attach_sparse, sp) == INVALID                                      # ... and so does attaching with the same bases
    one = sp[1].search_batch(qd, qv, qo, 10, 0.0, 5)                                     # the shard handle itself still answers
    assert (one[2] > 0).any()
    ss.attach_sparse(sp, np.array([0, 1000, 4201], np.uint32))                           # room for the new vector: the set answers again
    moved = ss.sparse_search(qd, qv, qo, 10, 0.0, 5)
    assert (good[2] > 0).any() and np.array_equal(moved[2], good[2])
    ss.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_set_answering():
    from cosdata_amd import _lib
    from cosdata_amd.shardset import ShardSet
    w = W.world(6)
    _, sp, whole = _shared(6, W.BOUNDS3)
    qd, qv, qo = w.query_csr()
    ss = ShardSet(dense_stubs(W.BOUNDS3))
    assert status(ss.sparse_search, qd, qv, qo, 10) == NOT_READY                         # nothing attached
    assert status(ss.attach_sparse, sp[:2]) == INVALID                                   # wrong n_shards
    assert status(ss.attach_sparse, [sp[0], sp[1], sp[1]]) == INVALID                    # a handle twice
    assert status(ss.attach_sparse, sp, np.array([0, 1000, 1000], np.uint32)) == INVALID  # bases do not strictly increase
    assert status(ss.attach_sparse, sp, np.array([0, 999, 4200], np.uint32)) == INVALID   # shard 0's 1000 vectors reach into shard 1
    assert status(ss.attach_sparse, sp, np.array([0, 1000, 0xFFFFFFFF - 1800], np.uint32)) == INVALID   # base + n = u32::MAX
    other_bits = W.sparse_shards(W.world(4), W.BOUNDS3)
    assert status(ss.attach_sparse, [sp[0], other_bits[1], sp[2]]) == INVALID            # quantization_bits differ
    assert status(ss.sparse_search, qd, qv, qo, 10) == NOT_READY                         # a refused attach attaches nothing
    ss.attach_sparse(sp, np.array([0, 1000, 0xFFFFFFFF - 1801], np.uint32))              # ... one below fits
    ss.attach_sparse(sp)
    good = ss.sparse_search(qd, qv, qo, 10, 0.0, 5)
    W.same(good, _expected(w, 0.0, 10, 5), "after the refused attaches")

    def still_answers(what):
        W.same_arrays(ss.sparse_search(qd, qv, qo, 10, 0.0, 5), good, what)

    # C above a shard's cos_sparse_set_max_candidates (64 unless set), as the single handle refuses it
    for top_k, factor in [(13, 5), (65, 0)]:
        assert status(ss.sparse_search, qd, qv, qo, top_k, 0.0, factor) == status(whole.search_batch, qd, qv, qo, top_k, 0.0, factor) == UNIMPLEMENTED
        still_answers(f"after ({top_k}, {factor})")
    sp[0].set_max_candidates(256)
    sp[2].set_max_candidates(256)                                                        # the narrowest shard decides
    assert status(ss.sparse_search, qd, qv, qo, 50, 0.0, 5) == UNIMPLEMENTED
    sp[0].set_max_candidates(64)
    sp[2].set_max_candidates(64)
    still_answers("after the narrowest shard refused")
    # decreasing offsets; top_k 0; B at the single handle's bound (refused before an offset is read)
    bad = qo.copy()
    bad[3], bad[4] = bad[4], bad[3]
    assert status(ss.sparse_search, qd, qv, bad, 10) == INVALID
    assert status(ss.sparse_search, qd, qv, qo, 0) == INVALID
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = (np.zeros(16, np.uint32), np.zeros(16, np.float32), np.zeros(16, np.uint32))
    assert _lib.lib().cos_shardset_sparse_search_batch(ss._h, p(qd), p(qv), p(qo), 0x80000000, 10, 0.0, 0, p(out[0]), p(out[1]), p(out[2])) == INVALID
    still_answers("after the invalid arguments")
    # a rerank while one shard holds no raw vectors
    no_raw = W.sparse_shards(w, W.BOUNDS3, keep_raw=False)
    ss.attach_sparse([sp[0], no_raw[1], sp[2]])
    assert status(ss.sparse_search, qd, qv, qo, 10, 0.0, 5) == NOT_READY
    W.same(ss.sparse_search(qd, qv, qo, 10, 0.0, 0), _expected(w, 0.0, 10, 0), "no rerank needs no raw vectors")
    ss.attach_sparse(sp)
    still_answers("after the missing raw vectors")
    ss.attach_sparse(None)                                                               # detach
    assert status(ss.sparse_search, qd, qv, qo, 10) == NOT_READY
    ss.close()


def test_nine_shards_at_1024_candidates_are_above_the_fold():
    """9 x 1024 gathered keys per query: refused before anything runs; 512 candidates (9 x 512 = 4608 keys) are answered"""
    bounds = [0, 60, 120, 180, 240, 300, 360, 420, 480, 600]
    _, _, _, _, ro, rd, rv = _corpus(n=600, vocab=W.VOCAB, bits=6, upper=W.UPPER, seed=13)
    w = W.World(6, raw=(ro, rd, rv), queries=W.world(6).queries[:5])
    sp, whole = W.sparse_shards(w, bounds), W.whole_handle(w)
    for h in sp + [whole]:
        h.set_max_candidates(1024)
    ss = _set(bounds, sp)
    qd, qv, qo = w.query_csr()
    assert status(ss.sparse_search, qd, qv, qo, 1024, 0.0, 0) == UNIMPLEMENTED
    assert status(ss.sparse_search, qd, qv, qo, 205, 0.0, 5) == UNIMPLEMENTED            # C = 1025 is above every handle's width
    assert status(ss.sparse_search, qd, qv, qo, 103, 0.0, 5) == UNIMPLEMENTED            # C = 515: records of 1024 slots
    _check(ss, whole, w, 0.0, 512, 0, "9 shards, (512, 0)")
    _check(ss, whole, w, 0.0, 100, 5, "9 shards, (100, 5)")
    ss.close()


# ---- 6. a search beside an insert ------------------------------------------------------------------------------------------------------------------
def test_search_beside_an_insert_sees_before_or_after():
    bits, thr = 6, 0.0
    w = W.world(bits)
    sp, whole = W.sparse_shards(w, W.BOUNDS3), W.whole_handle(w)
    ss = _set(W.BOUNDS3, sp)
    qd, qv, qo = w.query_csr()
    ro, rd, rv = _extra(bits)
    before = whole.search_batch(qd, qv, qo, 10, thr, 5)
    whole.insert(ro, rd, rv)
    after = whole.search_batch(qd, qv, qo, 10, thr, 5)
    assert not np.array_equal(before[0], after[0])
    answers, errors = [], []

    def searcher():
        try:
            for _ in range(20):
                answers.append(ss.sparse_search(qd, qv, qo, 10, thr, 5))
        except Exception as e:                                                          # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=searcher)
    t.start()
    sp[2].insert(ro, rd, rv)
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
    assert all(kinds), kinds                                                           # every answer is the before or the after expectation
    W.same_arrays(ss.sparse_search(qd, qv, qo, 10, thr, 5), after, "after the insert")
    ss.close()
