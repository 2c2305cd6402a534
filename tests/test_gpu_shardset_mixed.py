"""GPU: the mixed hybrid call on a shard set (cos_shardset_hybrid_search_mixed), every shard on device 0.

Three dense u8 shards of 6000 vectors at the bounds of tests/shardset_sparse_world.py, the three learned-sparse shards of that world
(vec_bases = the dense shards' id_base) and the three BM25 shards of tests/shardset_text_world.py (their own doc_bases).  A batch mixes
the three arms in interleaved order.  The expected fusion is oracle.rrf_fuse over per-arm lists: the sparse and BM25 lists from the
oracle over the whole collection, the dense list the set's own cos_shardset_search_batch answer for 3 x top_k (a sharded walk is not
the unsharded walk; other tests hold it to the oracle)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import shardset_sparse_world as SW
from tests import shardset_text_world as TW

pytestmark = pytest.mark.gpu

DIM, KC, BITS, THR = 32, 60.0, 6, 0.0
INVALID, UNIMPLEMENTED, NOT_READY, CALCULATION = 3, 4, 6, 2
DS, DB, SB = 0, 1, 2                                                     # COS_HYBRID_DENSE_SPARSE, _DENSE_BM25, _SPARSE_BM25
TEXT_BASES = np.array(TW.BOUNDS3[:-1], np.uint32)
_cache = {}


def _world():
    """(dense shards, sparse shards, BM25 shards) — built once; no test updates them"""
    import cosdata_amd as ca
    if "w" not in _cache:
        X = H.clustered_corpus(SW.N, DIM, n_centers=24, sigma=0.2, seed=31) * np.float32(0.9)
        hp = ca.HNSWHyperParams(num_layers=3, ef_construction=32, ef_search=32)
        dense = []
        for s in range(3):
            ix = ca.HNSWIndex(DIM, hp, id_base=SW.BOUNDS3[s])
            ix.upload_vectors(np.ascontiguousarray(X[SW.BOUNDS3[s]:SW.BOUNDS3[s + 1]])).build(256)
            dense.append(ix)
        sp = SW.sparse_shards(SW.world(BITS), SW.BOUNDS3)
        for h in sp:
            h.set_max_candidates(1024)
        _cache["w"] = (dense, sp, TW.bm_shards(TW.BOUNDS3), H.queries_from(X, SW.NQ, noise=0.03, seed=8))
    return _cache["w"]


def _full_set():
    from cosdata_amd.shardset import ShardSet
    dense, sp, bm, Q = _world()
    if "ss" not in _cache:
        _cache["ss"] = ShardSet(dense).attach_sparse(sp).attach_bm25(bm, TEXT_BASES)
    return _cache["ss"], Q


def _batch(arms, Q):
    """query i of the batch uses dense query i, sparse query i and BM25 query i of the three worlds -> the request's three sub-batches"""
    sw, tw = SW.world(BITS), TW.world()
    arms = np.asarray(arms, np.uint8)
    idx = np.arange(arms.size)
    di, si, bi = idx[arms != SB], idx[arms != DB], idx[arms != DS]
    dense = np.ascontiguousarray(Q[di]) if di.size else None
    sparse = sw.query_csr([sw.queries[i] for i in si]) if si.size else None
    text = None
    if bi.size:
        terms = [tw.query(int(i)) for i in bi]
        text = (np.concatenate(terms).astype(np.uint32), np.cumsum([0] + [t.size for t in terms]).astype(np.uint32))
    return arms, dense, sparse, text


def _expected(ss, arms, Q, top_k, factor):
    sw, tw = SW.world(BITS), TW.world()
    k3 = 3 * top_k
    arms = np.asarray(arms, np.uint8)
    di = np.arange(arms.size)[arms != SB]
    dense = {}
    if di.size:
        d_ids, _, d_cnt = ss.batch_search(np.ascontiguousarray(Q[di]), k3)
        dense = {int(q): d_ids[j, :d_cnt[j]] for j, q in enumerate(di)}
    csr = tw.csr(0, TW.N)
    out = []
    for q, a in enumerate(arms.tolist()):
        sparse = sw.expected(THR, sw.queries[q], k3, factor)[0] if a != DB else None
        text = O.bm25_search(csr[0], csr[1], csr[2], csr[3], TW.N, tw.query(q), k3)[0] if a != DS else None
        first, second = (dense[q], sparse) if a == DS else (dense[q], text) if a == DB else (sparse, text)
        out.append(O.rrf_fuse(first, second, KC, top_k))
    return out


def _check(ss, arms, Q, top_k, factor, what):
    a, dense, sparse, text = _batch(arms, Q)
    got = ss.hybrid_search_mixed(a, dense, sparse, text, top_k, KC, THR, factor)
    TW.same(got, _expected(ss, a, Q, top_k, factor), what)
    return got


MIXED = np.array([DS, DB, SB, SB, DS, DB, DB, SB, DS, DS, SB, DB] * 3 + [SB], np.uint8)     # 37 queries, every arm, interleaved


@pytest.mark.parametrize("top_k,factor", [(10, 0), (10, 5), (20, 5), (170, 0)])
def test_mixed_batch_is_rrf_over_the_per_arm_lists(top_k, factor):
    SW.assert_preconditions()
    ss, Q = _full_set()
    got = _check(ss, MIXED, Q, top_k, factor, f"mixed, top_k {top_k} factor {factor}")
    assert (got[2] > 0).all()


def test_all_dense_bm25_equals_the_sets_hybrid_call():
    ss, Q = _full_set()
    tw = TW.world()
    arms = np.full(TW.NQ, DB, np.uint8)
    a, dense, _, text = _batch(arms, Q)
    for top_k in (5, 20):
        got = ss.hybrid_search_mixed(a, dense, None, text, top_k, KC)
        TW.same_arrays(got, ss.hybrid_search(Q[:TW.NQ], tw.q_terms, tw.q_off, top_k, KC), f"all DENSE_BM25, top_k {top_k}")
        assert np.array_equal(text[0], tw.q_terms) and np.array_equal(text[1], tw.q_off)


def test_single_queries_and_batches_that_lack_an_arm():
    from cosdata_amd.shardset import ShardSet
    dense, sp, bm, Q = _world()
    ss, _ = _full_set()
    for arm in (DS, DB, SB):
        for q in (0, 11):
            arms = np.full(q + 1, arm, np.uint8)                           # (query q of every world: a batch of q + 1, compared on its last)
            one = _check(ss, arms, Q, 10, 5, f"arm {arm}, {q + 1} queries")
            assert one[2][q] > 0
    single = ss.hybrid_search_mixed(*_batch([SB], Q), 10, KC, THR, 5)
    TW.same(single, _expected(ss, [SB], Q, 10, 5), "B = 1")
    # a half without queries needs nothing attached
    lacks = {"no sparse half": (np.array([DB, DB, DB, DB], np.uint8), lambda s: s.attach_bm25(bm, TEXT_BASES)),
             "no BM25 half": (np.array([DS, DS, DS], np.uint8), lambda s: s.attach_sparse(sp)),
             "no dense queries": (np.array([SB, SB, SB, SB, SB], np.uint8), lambda s: s.attach_sparse(sp).attach_bm25(bm, TEXT_BASES))}
    for what, (arms, attach) in lacks.items():
        part = attach(ShardSet(dense))
        _check(part, arms, Q, 10, 5, what)
        part.close()


def test_failing_dense_query_and_refusals_leave_the_set_answering():
    from cosdata_amd.shardset import ShardSet
    dense, sp, bm, Q = _world()
    ss, _ = _full_set()
    a, dq, sparse, text = _batch(MIXED, Q)
    good = ss.hybrid_search_mixed(a, dq, sparse, text, 10, KC, THR, 5)

    def still_answers(what):
        TW.same_arrays(ss.hybrid_search_mixed(a, dq, sparse, text, 10, KC, THR, 5), good, what)

    dz = dq.copy()
    dz[4] = -1.0                                                           # zero quantized norm (u8 codes all 0): the dense call's status
    assert TW.status(ss.hybrid_search_mixed, a, dz, sparse, text, 10, KC, THR, 5) == CALCULATION
    still_answers("the call after the failing dense query")
    assert TW.status(ss.hybrid_search_mixed, a, dq, sparse, text, 171, KC, THR, 0) == UNIMPLEMENTED        # top_k 171
    assert TW.status(ss.hybrid_search_mixed, a, dq, sparse, text, 70, KC, THR, 5) == UNIMPLEMENTED         # 3 x 70 x 5 = 1050 candidates
    sp[1].set_max_candidates(64)
    assert TW.status(ss.hybrid_search_mixed, a, dq, sparse, text, 10, KC, THR, 5) == UNIMPLEMENTED         # 150 > the narrowest shard's 64
    sp[1].set_max_candidates(1024)
    bad = a.copy()
    bad[7] = 3
    assert TW.status(ss.hybrid_search_mixed, bad, dq, sparse, text, 10, KC, THR, 5) == INVALID             # an arm above 2
    still_answers("after the refusals")
    # a rerank while a shard holds no raw vectors; a needed half that is not attached
    no_raw = SW.sparse_shards(SW.world(BITS), SW.BOUNDS3, keep_raw=False)
    part = ShardSet(dense).attach_sparse([sp[0], no_raw[1], sp[2]]).attach_bm25(bm, TEXT_BASES)
    assert TW.status(part.hybrid_search_mixed, a, dq, sparse, text, 10, KC, THR, 5) == NOT_READY
    TW.same(part.hybrid_search_mixed(a, dq, sparse, text, 10, KC, THR, 0), _expected(part, a, Q, 10, 0), "no rerank needs no raw vectors")
    part.attach_sparse(None)
    assert TW.status(part.hybrid_search_mixed, a, dq, sparse, text, 10, KC, THR, 0) == NOT_READY           # sparse half not attached
    part.attach_sparse(sp).attach_bm25(None)
    assert TW.status(part.hybrid_search_mixed, a, dq, sparse, text, 10, KC, THR, 0) == NOT_READY           # BM25 half not attached
    part.attach_bm25(bm, TEXT_BASES)
    TW.same_arrays(part.hybrid_search_mixed(a, dq, sparse, text, 10, KC, THR, 5), good, "attached again")
    part.close()
    still_answers("at the end")
