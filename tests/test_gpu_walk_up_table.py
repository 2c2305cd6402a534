"""GPU: the row level directly under the level table reads table columns for the neighbours that have a node one level up
(LevelDev::adj_up, WalkPlan::up_table_level, tuning knob walk_up_table).  The level-table GEMM has already computed the integer dot
of the query with every node of the table's lowest level; a neighbour of the level below that also has a node there is taken from
that column instead of from its code row.  Same integer, so every per-level list and every result must keep its bits: knob 0 (never)
against knob 2 (at every launch size), and both against the oracle where tests/test_gpu_walk_table.py compares to it.

Shapes: levels shrink by four, so 20 000 vectors give 1 250 nodes on level 2 and about 312 on level 3; the table is pinned to the
levels >= 3, which leaves the row levels 2, 1, 0 under the table levels 3, 4, 5.  The other cases use 6 000 vectors (375 / 94)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_gpu_walk_table import _check_against_oracle, _same

pytestmark = pytest.mark.gpu

LAYERS, TAB_MIN = 5, 3   # table levels 3..5, the level under the table is 2
KNOBS_ON = dict(walk_up_table=2, walk_adj_mag=2)
KNOBS_OFF = dict(walk_up_table=0, walk_adj_mag=2)


@functools.lru_cache(maxsize=None)
def _oracle(dim, metric, n, m0, m):
    X = H.clustered_corpus(n, dim, n_centers=24, seed=900 + dim)
    X.setflags(write=False)
    oix = H.oracle_index(X, O.STORAGE_U8, 0, num_layers=LAYERS, ef_construction=40, ef_search=112, metric=metric,
                         level0_neighbors_count=m0, neighbors_count=m)
    return X, oix


def _device(oix, X, visited=0, cut=0):
    """a device index over the oracle's graph, throughput kernel at every launch size, table pinned to the levels >= TAB_MIN;
    cut: 0 = one launch, l = split walk cut after level l (the order's key level is chosen when the graph is committed)"""
    from cosdata_amd import _lib
    knobs = {"walk_split_levels": 1 << cut} if cut else {}
    with _lib.tuning(**knobs):
        dix = H.device_index_from_oracle(oix, X, visited_mode=visited)
    _pin(dix, cut)
    return dix


def _pin(dix, cut=0, tab_min=TAB_MIN):
    dix.set_latency_mode(0)
    dix.set_latency_waves(0)
    dix.set_walk_order(1 if cut else 0)
    dix.set_walk_table(sum(dix.level_count(l) for l in range(tab_min, LAYERS + 1)), 1)
    assert dix.walk_table_info()[0] == tab_min


def _run(dix, Q, knobs, top_k=10):
    """-> (final results with statuses, per-level lists of the queries that did not fail, table evaluations of the ann launch)"""
    from cosdata_amd import _lib
    with _lib.tuning(**knobs):
        ids, sc, cnt, rc, status = dix.batch_search(Q, top_k, return_status=True)
        walk = dix.ann_search_batch(Q[status == 0])
        sp = dix.last_walk_split()
    return (ids, sc, cnt, status), rc, walk, sp


def _compare(dix, Q, cut=0):
    off, rc0, walk0, sp0 = _run(dix, Q, KNOBS_OFF)
    on, rc2, walk2, sp2 = _run(dix, Q, KNOBS_ON)
    assert rc0 == rc2 and _same(on, off) and _same(walk2, walk0)            # ids, similarities as bit patterns, counts, statuses
    assert sp0.table_level_min == TAB_MIN and sp2.table_level_min == TAB_MIN and sp0.cut_after_level == cut and sp2.cut_after_level == cut
    assert sp2.upper_evals + sp2.lower_evals == sp0.upper_evals + sp0.lower_evals   # the same walk, evaluation for evaluation
    assert int(sp2.table_evals) - int(sp0.table_evals) > 0                  # ... of which some came from the table on the level under it
    return on, sp0, sp2


def test_base_case_every_bit_and_the_share_of_table_winners():
    from cosdata_amd import _lib
    X, oix = _oracle(768, O.METRIC_COSINE, 20000, 64, 32)
    dix = _device(oix, X)
    Q = H.queries_from(X, 384, noise=0.05, seed=21)
    Q[7] = oix.params.range_lo                                # the all-zero code: CalculationError at the entry node, same on both sides
    on, sp0, sp2 = _compare(dix, Q)
    assert on[3][7] == 2 and np.count_nonzero(on[3]) == 1
    ok = np.array([b for b in range(0, 384, 17) if b != 7])
    _check_against_oracle(oix, on[:3], Q, 10, ok)
    # A quarter of level 2's nodes have a node on level 3; so has about a quarter of its neighbour slots (checked here on the
    # graph itself), and so should have 15..35 % of the level's winners.  The level's evaluations: the table evaluations with the
    # table moved one level down minus those with the table where it is (knob 0 both times: the same walk either way).
    lv2_ids, lv2_nbr = dix.download_graph()[TAB_MIN - 1]
    lv3_ids = dix.download_graph()[TAB_MIN][0]
    live = lv2_nbr[lv2_nbr != 0xFFFFFFFF]
    assert 0.15 < np.isin(live, lv3_ids).mean() < 0.35 and 0.15 < np.isin(lv2_ids, lv3_ids).mean() < 0.35
    Qok = np.delete(Q, 7, axis=0)
    _pin(dix, tab_min=TAB_MIN - 1)                            # (the table rule moves: adj_up follows it to level 1)
    with _lib.tuning(**KNOBS_OFF):
        dix.ann_search_batch(Qok)
        level2 = int(dix.last_walk_split().table_evals) - int(sp0.table_evals)
    _pin(dix)
    share = (int(sp2.table_evals) - int(sp0.table_evals)) / level2
    print(f"level {TAB_MIN - 1}: {level2} evaluations, {share:.3f} of them from table columns")
    assert 0.15 < share < 0.35
    # the table one level down: level 1 is the level under the table now, and the launch after the move is still bit-exact
    _pin(dix, tab_min=TAB_MIN - 1)
    off1, _, walk_off1, s0 = _run(dix, Qok, KNOBS_OFF)
    on1, _, walk_on1, s1 = _run(dix, Qok, KNOBS_ON)
    assert _same(on1, off1) and _same(walk_on1, walk_off1) and int(s1.table_evals) > int(s0.table_evals)
    assert _same(on1[:3], tuple(np.delete(a, 7, axis=0) for a in on[:3]))


# dims 520 (33 chunks: a tail chunk on the one-row-per-pass path), 768, 1024 (one chunk pass), 1536 (two); both metrics; both
# filters; ef 48 (one key per lane), 112 (two), 200 (four); one launch, a split walk with the level under the table in its lower
# range (cut after 3, the flagship's arrangement) and in its upper range, next to the table levels (cut after 1)
CASES = [
    (520, O.METRIC_COSINE, 0, 48, 0, 64, 32),
    (520, O.METRIC_DOT, 1, 112, 3, 64, 32),
    (768, O.METRIC_COSINE, 1, 112, 0, 64, 32),
    (768, O.METRIC_DOT, 0, 200, 1, 64, 32),
    (1024, O.METRIC_COSINE, 0, 112, 3, 128, 64),
    (1024, O.METRIC_DOT, 0, 48, 1, 128, 64),
    (1024, O.METRIC_COSINE, 1, 200, 3, 128, 64),
    (1536, O.METRIC_COSINE, 0, 200, 0, 64, 32),
    (1536, O.METRIC_COSINE, 1, 48, 3, 64, 32),
    (1536, O.METRIC_DOT, 0, 112, 1, 64, 32),
]


@pytest.mark.parametrize("dim,metric,visited,ef,cut,m0,m", CASES)
def test_every_path_keeps_every_bit(dim, metric, visited, ef, cut, m0, m):
    X, oix = _oracle(dim, metric, 6000, m0, m)
    dix = _device(oix, X, visited, cut)
    dix.set_ef_search(ef)
    oix.set_ef_search(ef)
    oix.set_visited_mode(O.VISITED_EXACT if visited else 0)
    try:
        Q = H.queries_from(X, 300, noise=0.05, seed=ef + dim)
        on, _, _ = _compare(dix, Q, cut)
        assert np.count_nonzero(on[3]) == 0
        _check_against_oracle(oix, on[:3], Q, 10, np.arange(0, 300, 19))
    finally:
        oix.set_ef_search(112)
        oix.set_visited_mode(0)


def test_a_root_replaced_on_a_live_graph():
    """cos_index_set_root invalidates the norms beside the adjacency and adj_up with them; the first launch big enough refills both"""
    X, oix0 = _oracle(520, O.METRIC_COSINE, 6000, 64, 32)
    oix = O.OracleIndex(oix0.params).set_vectors(X).import_graph(oix0.export_graph(), oix0.root_raw())
    dix = _device(oix, X)
    Q = H.queries_from(X, 1024, noise=0.05, seed=5)           # ADJ_MAG_REFILL_MIN_B queries: the launch that pays for the refill
    _compare(dix, Q[:300])
    root2 = np.ascontiguousarray(X[7] * 0.5 + X[11] * 0.5)
    dix.set_root(root2)
    oix.set_root_raw(root2)
    on, _, _ = _compare(dix, Q)
    _check_against_oracle(oix, on[:3], Q, 10, np.arange(0, 1024, 41))


def test_append_and_delete_on_the_resident_graph():
    """adj_up follows the graph: 500 vectors appended, then 8 ids deleted, a search after each"""
    import cosdata_amd as ca
    n, dim = 5000, 520
    Xall = H.clustered_corpus(n + 500, dim, n_centers=24, seed=77)
    hp = ca.HNSWHyperParams(num_layers=LAYERS, ef_construction=40, ef_search=112, level_0_neighbors_count=64, neighbors_count=32)
    dix = ca.HNSWIndex(dim, hp, ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), seed=3)
    dix.upload_vectors(Xall[:n]).build(256)
    op = O.HNSWParams(dim=dim, num_layers=LAYERS, ef_construction=40, ef_search=112, level0_neighbors_count=64, neighbors_count=32, seed=3)
    Q = H.queries_from(Xall, 300, noise=0.05, seed=8)

    def check(Xnow):
        _pin(dix)
        on, _, _ = _compare(dix, Q)
        oix = O.OracleIndex(op).set_vectors(Xnow).import_graph(dix.download_graph(), dix.download_root())
        _check_against_oracle(oix, on[:3], Q, 10, np.arange(0, 300, 19))
        return on

    check(Xall[:n])
    dix.append(Xall[n:], 256)
    check(Xall)
    dele = np.arange(40, 5400, 700, dtype=np.uint32)
    assert dele.size == 8
    dix.delete(dele)
    on = check(Xall)
    assert not np.isin(on[0], dele).any()
