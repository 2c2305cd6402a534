"""cos_bruteforce_topk on corpora with hundreds of copies and near-copies of one row (tests/near_copies.py; the conditions that make
them a test are asserted without a GPU by test_oracle_near_copies.py).  More rows lie within the scores' error of the k-th score than
the survivor pool holds, so the f32 MFMA's ranking cannot decide which of them survive: the call has to notice (flat_plan.h
brute_margin_safe) and score such a query's rows in the reference's order.  Every answer must equal O.bruteforce_topk bit for bit —
ids and scores as uint32 views — on the unfused and the fused schedule, at every pool width, under masks and on a shard set; on the
ordinary corpora no query may leave the MFMA path."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_masked as FM
from tests import near_copies as NC
from tests import odd_dims as OD

pytestmark = pytest.mark.gpu


def plain_index(X, id_base=0):
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType.UnsignedByte(), id_base=id_base)
    ix.upload_vectors(np.ascontiguousarray(X))
    return ix


@functools.lru_cache(maxsize=2)
def _index(corpus_key):
    return plain_index(NC.corpus(corpus_key)[0])


def assert_same(got, ref, what):
    ids, sc = got[:2]
    oids, osc = ref
    wrong = [b for b in range(ids.shape[0]) if not (np.array_equal(ids[b], oids[b]) and np.array_equal(sc[b].view(np.uint32), osc[b].view(np.uint32)))]
    missed = [int(len(set(oids[b].tolist()) - set(ids[b].tolist()))) for b in wrong]
    assert not wrong, f"{what}: queries {wrong} differ from the oracle; oracle ids missing from the answer per such query: {missed}"


def run_case(case, **knobs):
    from cosdata_amd import _lib
    _, Q, _ = NC.corpus(case)
    ix = _index(case[:5])
    with _lib.tuning(**knobs):
        got = ix.bruteforce_topk(Q, case[5])
    assert_same(got, NC.oracle_topk(case), NC.case_id(case))
    return ix


@pytest.mark.parametrize("case", NC.UNFUSED + NC.NO_FLOAT4 + NC.WIDE, ids=NC.case_id)
def test_one_score_matrix_chunk(case):
    """n below the seed: the GEMM writes its scores, the selection cuts the pool of 64 (k 1, 10, 32), 128 (k 33, 64) or 1024 (k 512) keys;
    dim 97 stages its rows without float4"""
    run_case(case)


@pytest.mark.parametrize("unfused", [0, 1], ids=["fused", "flat_unfused"])
@pytest.mark.parametrize("case", NC.FUSED, ids=NC.case_id)
def test_copies_through_the_fused_epilogue(case, unfused):
    """n = 20000: rows from 16384 on reach the pool through the GEMM's threshold filter and the append fold.  Copies only there, or on both
    sides of the seed; the same on the score-matrix path alone"""
    run_case(case, flat_unfused=unfused)


@pytest.mark.parametrize("case", NC.ALL_TIE, ids=NC.case_id)
def test_every_row_is_a_copy(case):
    """all rows equal: the answer is ids n-1, n-2, ... with one score.  All rows scaled copies: every query is near every row"""
    n, k = case[0], case[5]
    ix = run_case(case)
    if case[3] == "exact":
        _, Q, _ = NC.corpus(case)
        ids, _ = ix.bruteforce_topk(Q, k)
        assert np.array_equal(ids, np.tile(np.arange(n - 1, n - 1 - k, -1, dtype=np.uint32), (Q.shape[0], 1)))


def test_masked_half_of_the_copies_and_fewer_rows_than_k():
    """two masks share the queries (query b takes mask b % 2): one removes every second copy, the other leaves fewer than k rows; the
    reference is the oracle on the live rows with the ids mapped back (tests/flat_masked.py)"""
    case = NC.MASKED
    k = case[5]
    X, Q, _ = NC.corpus(case)
    masks = NC.masks_for(case)
    qm = (np.arange(Q.shape[0]) % 2).astype(np.uint32)
    ix = _index(case[:5])
    got = ix.bruteforce_topk_masked(Q, k, masks, qm)
    for g in range(2):
        sel = np.flatnonzero(qm == g)
        ref = FM.subset_brute(X, Q, masks[g], k)
        FM.same(tuple(a[sel] for a in got), ref, rows=sel, what=f"mask {g}")
        assert (got[2][sel] == min(k, int(masks[g].sum()))).all()
    assert (got[2][qm == 1] < k).all()


def test_shard_set_of_three():
    """the mixed corpus cut into three id-range shards on one device: the set's answer is the oracle's on the whole corpus"""
    from cosdata_amd.shardset import ShardSet
    case = NC.SHARDED
    X, Q, _ = NC.corpus(case)
    bounds = np.concatenate([[0], np.cumsum(NC.SHARD_SIZES)])
    shards = [plain_index(X[bounds[s]:bounds[s + 1]], id_base=int(bounds[s])) for s in range(3)]
    ss = ShardSet(shards)
    try:
        got = ss.bruteforce_topk(Q, case[5])
        assert (got[2] == case[5]).all()
        assert_same(got, NC.oracle_topk(case), "shard set")
    finally:
        ss.close()


# ---- the exact path by knob, and who took it ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _ordinary(shape):
    n, dim, B = shape
    X, Q = OD.brute_corpus(n, dim, B)
    return Q, plain_index(X), O.bruteforce_topk(X, Q, min(512, n), threads=8)


@pytest.mark.parametrize("shape,ks", NC.ORDINARY, ids=[f"{s[0]}x{s[1]}" for s, _ in NC.ORDINARY])
def test_ordinary_corpora_exact_path_by_knob_equals_default_and_nobody_takes_it_unasked(shape, ks):
    """flat_brute_exact = 2 sends every query down the exact path: the oracle's answer and the default path's, bit for bit.  With default
    knobs these corpora (k-th to P-th gap above four times the bound, test_oracle_near_copies.py) send none"""
    from cosdata_amd import _lib
    Q, ix, (oids, osc) = _ordinary(shape)
    for k in ks:
        ids, sc = ix.bruteforce_topk(Q, k)
        st = ix.last_brute_stats()
        assert (st.queries, st.exact_queries, st.pool) == (Q.shape[0], 0, NC.pool_width(k)), (k, st.queries, st.exact_queries, st.pool)
        with _lib.tuning(flat_brute_exact=2):
            eids, esc = ix.bruteforce_topk(Q, k)
            assert ix.last_brute_stats().exact_queries == Q.shape[0]
        assert_same((ids, sc), (oids[:, :k], osc[:, :k]), f"default k {k}")
        assert_same((eids, esc), (oids[:, :k], osc[:, :k]), f"exact k {k}")
        assert np.array_equal(ids, eids) and np.array_equal(sc.view(np.uint32), esc.view(np.uint32))


def test_last_brute_stats_contract():
    """zero before the first call; a wrong struct_size is refused (status 3) and the handle answers afterwards"""
    import ctypes as C
    import cosdata_amd as ca
    from cosdata_amd import _lib
    case = NC.UNFUSED[0]
    ix = plain_index(NC.corpus(case)[0])
    st = ix.last_brute_stats()
    assert (st.queries, st.exact_queries, st.pool) == (0, 0, 0)
    bad = _lib.CosBruteStats(struct_size=12)
    assert _lib.lib().cos_index_last_brute_stats(ix._h, C.byref(bad)) == 3
    ix.bruteforce_topk_masked(NC.corpus(case)[1], 10, skip_deleted=True)
    st = ix.last_brute_stats()
    assert st.queries == NC.NQ and st.pool == 64 and st.exact_queries >= NC.AIMED
    with pytest.raises(ca.CosdataError):
        ix.bruteforce_topk(NC.corpus(case)[1], 513)
    assert ix.last_brute_stats().queries == NC.NQ                  # a refused call leaves the last answer's figures


@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_id)
def test_aimed_queries_take_the_exact_path(case):
    """at least the eight queries aimed at the copied row are flagged; flat_brute_exact = 0 (the margin rule off) reports none"""
    from cosdata_amd import _lib
    ix = run_case(case)
    st = ix.last_brute_stats()
    assert NC.AIMED <= st.exact_queries <= NC.NQ and st.queries == NC.NQ, (st.queries, st.exact_queries)
    _, Q, _ = NC.corpus(case)
    with _lib.tuning(flat_brute_exact=0):
        ix.bruteforce_topk(Q, case[5])
        assert ix.last_brute_stats().exact_queries == 0
