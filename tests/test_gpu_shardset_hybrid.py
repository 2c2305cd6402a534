"""GPU: dense + BM25 hybrid search on a shard set (cos_shardset_hybrid_search_batch), every shard on device 0.

Three dense u8 shards of the 12 000 ids of tests/shardset_text_world.py (built on the device, id_base = the shard bounds) and the three
BM25 shards of that world, attached with doc_bases=None.  The expected answer is cos_rrf_fuse_batch — and
oracle.rrf_fuse per query — over the set's own dense lists (ShardSet.batch_search for 3 x top_k) and the whole-collection BM25
handle's lists for 3 x top_k; ids, score bits and counts must be equal."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import shardset_text_world as W

pytestmark = pytest.mark.gpu

DIM, KC = 32, 60.0
UNIMPLEMENTED, CALCULATION = 4, 2
_cache = {}


def _dense():
    """(the three dense shards, the 37 dense queries)"""
    import cosdata_amd as ca
    if "dense" not in _cache:
        X = H.clustered_corpus(W.N, DIM, n_centers=24, sigma=0.2, seed=31) * np.float32(0.9)
        hp = ca.HNSWHyperParams(num_layers=3, ef_construction=32, ef_search=32)
        shards = []
        for s in range(3):
            ix = ca.HNSWIndex(DIM, hp, id_base=W.BOUNDS3[s])
            ix.upload_vectors(np.ascontiguousarray(X[W.BOUNDS3[s]:W.BOUNDS3[s + 1]])).build(256)
            shards.append(ix)
        _cache["dense"] = (shards, H.queries_from(X, W.NQ, noise=0.03, seed=8))
    return _cache["dense"]


def _check(ss, whole, Q, qt, qo, top_k, what):
    import cosdata_amd as ca
    k3 = 3 * top_k
    d_ids, _, d_cnt = ss.batch_search(Q, k3)
    t_ids, _, t_cnt = whole.search_batch(qt, qo, k3)
    exp = ca.rrf_fuse_batch(d_ids, d_cnt, t_ids, t_cnt, KC, top_k)
    got = ss.hybrid_search(Q, qt, qo, top_k, KC)
    W.same_arrays(got, exp, what)
    W.same(got, [O.rrf_fuse(d_ids[i, :d_cnt[i]], t_ids[i, :t_cnt[i]], KC, top_k) for i in range(np.atleast_2d(Q).shape[0])], what + " vs oracle")
    assert (got[2] > 0).all()
    return got


def test_hybrid_on_the_set_is_rrf_over_the_two_merged_lists():
    from cosdata_amd.shardset import ShardSet
    W.assert_preconditions()
    w = W.world()
    shards, Q = _dense()
    bm, whole = W.bm_shards(W.BOUNDS3), W.whole_handle()
    ss = ShardSet(shards).attach_bm25(bm)                              # doc_bases=None: the dense shards' id_base
    for top_k in (5, 20, 170):
        got = _check(ss, whole, Q, w.q_terms, w.q_off, top_k, f"top_k {top_k}, 37 queries")
        one = _check(ss, whole, Q[3:4], w.query(3), np.array([0, w.query(3).size], np.uint32), top_k, f"top_k {top_k}, 1 query")
        assert np.array_equal(one[0][0, :one[2][0]], got[0][3, :got[2][3]])
    # the text half alone, on a set with real dense shards
    W.same(ss.bm25_search(w.q_terms, w.q_off, 60), W.whole_expected(60), "bm25_search beside dense shards")
    # refusals; the set answers afterwards
    good = ss.hybrid_search(Q, w.q_terms, w.q_off, 20, KC)
    assert W.status(ss.hybrid_search, Q, w.q_terms, w.q_off, 171) == UNIMPLEMENTED
    Qz = Q.copy()
    Qz[5] = -1.0                                                       # zero quantized norm (u8 codes all 0): the dense call's status
    assert W.status(ss.batch_search, Qz, 60) == CALCULATION
    assert W.status(ss.hybrid_search, Qz, w.q_terms, w.q_off, 20) == CALCULATION
    W.same_arrays(ss.hybrid_search(Q, w.q_terms, w.q_off, 20, KC), good, "the call after the failing one")
    # the same call after the inserts and deletes of the BM25 test
    for step in (0, 1):
        W.apply_updates(bm, whole, step)
        _check(ss, whole, Q, w.q_terms, w.q_off, 20, f"after update step {step}")
    assert not np.array_equal(ss.hybrid_search(Q, w.q_terms, w.q_off, 20, KC)[0], good[0])      # the updates are visible in the fused lists
    ss.close()
