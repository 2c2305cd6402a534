"""GPU: the nested level table of the throughput walk (cosdata_amd/csrc/table_nested.h, LevelDev::adj_tab, WalkPlan::table_nested, tuning
knob walk_table_nested).  The table has one GEMM column per vector of its lowest level instead of one per (level, node); a table level's
walk loads node | column in the word where it loaded the node.  The integer dot in a column is the one the per-level table held, so
every per-level list and every result keeps its bits: knob 2 (every graph) against knob 0 (never) and against the oracle.

Shapes: levels shrink by four, so 20 000 vectors give about 5 000 / 1 250 / 313 / 79 nodes on levels 1 .. 4; with ten layers the top
levels hold a handful of nodes down to the root alone."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_gpu_walk_table import _check_against_oracle, _same

pytestmark = pytest.mark.gpu

N = 20000
NEST, FLAT = dict(walk_table_nested=2), dict(walk_table_nested=0)
UP_ON, UP_OFF = dict(walk_up_table=2, walk_adj_mag=2), dict(walk_up_table=0, walk_adj_mag=2)


@functools.lru_cache(maxsize=None)
def _oracle(dim, metric, layers, n=N):
    X = H.clustered_corpus(n, dim, n_centers=24, seed=700 + dim)
    X.setflags(write=False)
    oix = H.oracle_index(X, O.STORAGE_U8, 0, num_layers=layers, ef_construction=32, ef_search=112, metric=metric,
                         level0_neighbors_count=32, neighbors_count=16)
    return X, oix


def _pin(dix, tab_min):
    """throughput kernel at every launch size, one launch, table pinned to the levels >= tab_min"""
    dix.set_latency_mode(0)
    dix.set_latency_waves(0)
    dix.set_walk_order(0)
    top = _top(dix)
    dix.set_walk_table(sum(dix.level_count(l) for l in range(tab_min, top + 1)), 1)
    assert dix.walk_table_info()[0] == tab_min


def _top(dix):
    return dix.hnsw_params.num_layers


def _run(dix, Q, knobs, top_k=10):
    from cosdata_amd import _lib
    with _lib.tuning(**knobs):
        info = dix.walk_table_info()
        ids, sc, cnt, rc, status = dix.batch_search(Q, top_k, return_status=True)
        sp_search = dix.last_walk_split()
        walk = dix.ann_search_batch(Q[status == 0])
        sp = dix.last_walk_split()
    return (ids, sc, cnt, status), rc, walk, sp, sp_search, info


def _compare(dix, Q, tab_min, up=UP_OFF):
    """knob 2 against knob 0 on final answers, statuses and per-level lists; what each launch reports"""
    top = _top(dix)
    n_min, n_all = dix.level_count(tab_min), sum(dix.level_count(l) for l in range(tab_min, top + 1))
    flat, rc0, walk0, sp0, sps0, info0 = _run(dix, Q, dict(FLAT, **up))
    nest, rc2, walk2, sp2, sps2, info2 = _run(dix, Q, dict(NEST, **up))
    assert rc0 == rc2 and _same(nest, flat) and _same(walk2, walk0)
    assert info0 == (tab_min, n_all) and info2 == (tab_min, n_min)
    for sp, cols in ((sp0, n_all), (sps0, n_all), (sp2, n_min), (sps2, n_min)):
        assert sp.table_level_min == tab_min and sp.table_cols == cols and sp.table_evals > 0
    assert sp2.table_evals == sp0.table_evals and sp2.upper_evals + sp2.lower_evals == sp0.upper_evals + sp0.lower_evals
    assert sp2.table_int8_ops * n_all == sp0.table_int8_ops * n_min
    return nest, sp0, sp2


# dims 64 / 80 / 100 (four / five / seven 16-byte chunks, the last two with a tail); both metrics; both filters; ef 16 / 64 / 112 (one
# key per lane, and two); launches of 1 / 255 / 256 / 300 queries around the GEMM's 256-query row group; table ranges of one level, two
# levels, and every level up to levels of a single node (ten layers); the level under the table with and without its table columns
CASES = [
    # dim, metric, layers, tab_min, visited, ef, B, up
    (64, O.METRIC_COSINE, 10, 1, 0, 112, 300, UP_OFF),
    (64, O.METRIC_COSINE, 10, 3, 1, 64, 256, UP_ON),
    (64, O.METRIC_COSINE, 10, 2, 0, 16, 1, UP_ON),
    (80, O.METRIC_DOT, 4, 4, 0, 16, 255, UP_ON),
    (80, O.METRIC_DOT, 4, 3, 1, 112, 1, UP_OFF),
    (100, O.METRIC_COSINE, 4, 2, 0, 64, 300, UP_ON),
    (100, O.METRIC_COSINE, 4, 3, 1, 16, 256, UP_OFF),
    (100, O.METRIC_DOT, 4, 1, 0, 112, 255, UP_OFF),
    (100, O.METRIC_DOT, 4, 4, 1, 64, 300, UP_ON),
    # 1024 dims (6 000 vectors): the one-row-per-pass path, the only one on which the level under the table reads table columns —
    # of the nested table here, by the COLUMN of the node one level up
    (1024, O.METRIC_COSINE, 5, 3, 0, 112, 300, UP_ON),
    (1024, O.METRIC_DOT, 5, 2, 1, 64, 255, UP_ON),
]


@pytest.mark.parametrize("dim,metric,layers,tab_min,visited,ef,B,up", CASES)
def test_every_path_keeps_every_bit(dim, metric, layers, tab_min, visited, ef, B, up):
    X, oix = _oracle(dim, metric, layers, 6000 if dim == 1024 else N)
    dix = H.device_index_from_oracle(oix, X, visited_mode=visited)
    _pin(dix, tab_min)
    if layers == 10:
        assert dix.level_count(10) == 1 and dix.level_count(4) > 1      # levels of the root alone at the top of the table
    dix.set_ef_search(ef)
    oix.set_ef_search(ef)
    oix.set_visited_mode(O.VISITED_EXACT if visited else 0)
    try:
        Q = H.queries_from(X, B, noise=0.05, seed=ef + dim)
        nest, sp0, sp2 = _compare(dix, Q, tab_min, up)
        assert np.count_nonzero(nest[3]) == 0
        if up is UP_ON and tab_min >= 2:
            _, sp_off, _ = _compare(dix, Q, tab_min, UP_OFF)
            if dim == 1024:
                assert int(sp2.table_evals) > int(sp_off.table_evals)  # the level under the table read table columns, of either table
            else:
                assert int(sp2.table_evals) == int(sp_off.table_evals) # (rows of fewer than 64 chunks: that level keeps its code rows)
        _check_against_oracle(oix, nest[:3], Q, 10, np.arange(0, B, 19))
    finally:
        oix.set_ef_search(112)
        oix.set_visited_mode(0)


def test_a_zero_norm_query_fails_the_same_way():
    X, oix = _oracle(100, O.METRIC_COSINE, 4)
    dix = H.device_index_from_oracle(oix, X)
    _pin(dix, 2)
    Q = H.queries_from(X, 300, noise=0.05, seed=3)
    Q[7] = oix.params.range_lo          # the all-zero code: CalculationError at the start node's table entry
    Q[299] = oix.params.range_lo
    nest, _, _ = _compare(dix, Q, 2, UP_ON)
    assert nest[3][7] == 2 and nest[3][299] == 2 and np.count_nonzero(nest[3]) == 2


def test_a_root_replaced_on_a_live_graph():
    """cos_index_set_root invalidates the table's operands and the side arrays: the next launch regathers and refills"""
    X, oix0 = _oracle(1024, O.METRIC_COSINE, 5, 6000)     # (1024 dims: the level under the table reads table columns too)
    oix = O.OracleIndex(oix0.params).set_vectors(X).import_graph(oix0.export_graph(), oix0.root_raw())
    dix = H.device_index_from_oracle(oix, X)
    _pin(dix, 3)
    Q = H.queries_from(X, 1024, noise=0.05, seed=5)       # (1 024 queries: the launch that pays for the refill of the norms)
    _compare(dix, Q[:300], 3, UP_ON)
    root2 = np.ascontiguousarray(X[7] * 0.5 + X[11] * 0.5)
    dix.set_root(root2)
    oix.set_root_raw(root2)
    nest, sp0, sp2 = _compare(dix, Q, 3, UP_ON)
    _, sp_off, _ = _compare(dix, Q, 3, UP_OFF)
    assert int(sp2.table_evals) > int(sp_off.table_evals)   # adj_up was refilled, with columns
    _check_against_oracle(oix, nest[:3], Q, 10, np.arange(0, 1024, 41))


def test_append_and_delete_on_the_resident_graph():
    """adj_tab follows the graph: vectors appended (new nodes on the table levels: new operands), then ids deleted (the adjacency changes
    under a table that stays: the side array alone is refilled); after each the answers equal the walk without a table"""
    import cosdata_amd as ca
    from cosdata_amd import _lib
    n, dim, layers = 18000, 64, 4
    Xall = H.clustered_corpus(n + 2000, dim, n_centers=24, seed=78)
    hp = ca.HNSWHyperParams(num_layers=layers, ef_construction=32, ef_search=64, level_0_neighbors_count=32, neighbors_count=16)
    dix = ca.HNSWIndex(dim, hp, ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), seed=3)
    dix.upload_vectors(Xall[:n]).build(1024)
    Q = H.queries_from(Xall, 300, noise=0.05, seed=8)

    def check():
        _pin(dix, 2)
        nest, _, sp2 = _compare(dix, Q, 2, UP_ON)
        with _lib.tuning(**NEST):
            walk = dix.ann_search_batch(Q)
            dix.set_walk_table(0, 0)
            plain_res, plain_walk = dix.batch_search(Q, 10), dix.ann_search_batch(Q)
            assert dix.last_walk_split().table_cols == 0
        assert _same(nest[:3], plain_res) and _same(walk, plain_walk)
        return nest

    check()
    dix.append(Xall[n:], 1024)
    check()
    dele = np.arange(40, 19000, 900, dtype=np.uint32)
    dix.delete(dele)
    nest = check()
    assert not np.isin(nest[0], dele).any()


def _auto_level_min(counts, ef, M, c=None):
    """the automatic table rule (walk_operands.h, table_rule) over the nodes of levels 0 .. top: level by level from the top while a level
    holds at most c x ef x M nodes (c = 10 up to ef = 1.5 M, 8 up to 2 M, 6 above, or knob walk_table_rule_c; 2^20 at most, alone and
    together)"""
    if c is None:
        c = 10 if 2 * ef <= 3 * M else 8 if ef <= 2 * M else 6
    lmin = cols = 0
    for l in range(len(counts) - 1, 0, -1):
        if counts[l] > min(c * ef * M, 1 << 20) or cols + counts[l] > 1 << 20:
            break
        lmin, cols = l, cols + counts[l]
    return lmin


# 20 000 x 64, ten layers (levels near 5 000 / 1 250 / 313): ef 16 -> 112 -> 16 moves the table from level 2 to level 1 and back; rows of
# four chunks, so no level wants adj_up under either key.
# 6 000 x 1024, five layers (levels near 1 500 / 375 / 94), walk_table_rule_c = 1: ef 16 -> 64 -> 16 moves it from level 3 (bound 256) to
# level 2 (bound 1 024) and back; rows of one pass, so adj_up is filled for level 2, freed and filled for level 1, and filled for level 2
# again, every time with columns of the nested table.
@pytest.mark.parametrize("dim,layers,n,efs,rule_c", [(64, 10, N, (16, 112), None), (1024, 5, 6000, (16, 64), 1)])
def test_the_table_key_changes_and_comes_back(dim, layers, n, efs, rule_c):
    """ef_search moves the automatic rule to another key and back on one handle: the nested set, adj_tab and adj_up of the level under
    the table are settled for the second key beside the first key's sets, which are found again afterwards.  Every step reports the
    rule's level and the columns of the nested set, equals the same handle without nested table and up-table columns, and equals the
    oracle; the level under the table reads table columns at every step where it can (1024 dims); the third step gives the first
    step's bits."""
    import cosdata_amd as ca
    X, oix = _oracle(dim, O.METRIC_COSINE, layers, n)
    dix = H.device_index_from_oracle(oix, X)
    dix.set_latency_mode(0)
    dix.set_latency_waves(0)
    dix.set_walk_order(0)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, 1)
    counts = [dix.level_count(l) for l in range(_top(dix) + 1)]
    want = {ef: _auto_level_min(counts, ef, 16, rule_c) for ef in efs}
    assert want[efs[0]] != want[efs[1]] and min(want.values()) >= (2 if dim == 1024 else 1), (counts, want)
    Q = H.queries_from(X, 300, noise=0.05, seed=21)
    rule = {} if rule_c is None else dict(walk_table_rule_c=rule_c)
    on, off = dict(NEST, **UP_ON, **rule), dict(FLAT, **UP_OFF, **rule)
    steps = []
    try:
        for ef in (efs[0], efs[1], efs[0]):
            dix.set_ef_search(ef)
            oix.set_ef_search(ef)
            lmin, n_min, n_all = want[ef], counts[want[ef]], sum(counts[want[ef]:])
            nest, rc2, walk2, sp2, sps2, info2 = _run(dix, Q, on)
            flat, rc0, walk0, sp0, sps0, info0 = _run(dix, Q, off)
            assert info2 == (lmin, n_min) and info0 == (lmin, n_all)
            for sp, cols in ((sp2, n_min), (sps2, n_min), (sp0, n_all), (sps0, n_all)):
                assert sp.table_level_min == lmin and sp.table_cols == cols and sp.table_evals > 0
            if dim == 1024:     # adj_up of level lmin - 1 is there, in the nested table's columns: a stale or missing array reads no column
                assert int(sp2.table_evals) > int(sp0.table_evals) and int(sps2.table_evals) > int(sps0.table_evals)
            else:
                assert int(sp2.table_evals) == int(sp0.table_evals)
            assert rc2 == rc0 and _same(nest, flat) and _same(walk2, walk0) and np.count_nonzero(nest[3]) == 0
            _check_against_oracle(oix, nest[:3], Q, 10, np.arange(0, 300, 19))
            steps.append((nest, walk2))
        assert _same(steps[2][0], steps[0][0])
        # ... and the per-level lists, up to their counts (the workspace keeps step two's longer lists behind them)
        (ids0, sims0, cnt0), (ids2, sims2, cnt2) = steps[0][1], steps[2][1]
        live = np.arange(ids0.shape[2])[None, None, :] < cnt0[:, :, None]
        assert np.array_equal(cnt2, cnt0) and np.array_equal(ids2[live], ids0[live])
        assert np.array_equal(sims2[live].view(np.uint32), sims0[live].view(np.uint32))
    finally:
        oix.set_ef_search(112)


def test_one_client_batch_keeps_the_per_level_table():
    """a 256-query batch above ef 128 takes the four-wave kernel, whose source knows nothing of the nested table: on a handle whose big
    launches read the nested set it reads the per-level one, and answers as it did"""
    from cosdata_amd import _lib
    X, oix = _oracle(100, O.METRIC_COSINE, 4)
    dix = H.device_index_from_oracle(oix, X)
    dix.set_ef_search(160)
    dix.set_latency_waves(256)                                       # one client batch; 300 queries walk on the throughput kernel
    top = _top(dix)
    n_all, n_min = sum(dix.level_count(l) for l in range(1, top + 1)), dix.level_count(1)
    Q = H.queries_from(X, 300, noise=0.05, seed=2)
    res = {}
    for name, knobs in (("flat", FLAT), ("nest", NEST)):
        with _lib.tuning(**knobs):
            assert dix.walk_table_info()[0] == 1
            one = dix.batch_search(Q[:256], 10, return_status=True)
            sp_one = dix.last_walk_split()
            big = dix.batch_search(Q, 10, return_status=True)
            sp_big = dix.last_walk_split()
            res[name] = (one, big)
            assert sp_one.table_cols == n_all            # (the four-wave kernel does not count its table evaluations)
            assert sp_big.table_cols == (n_min if name == "nest" else n_all) and sp_big.table_evals > 0
            assert dix.walk_table_info() == (1, sp_big.table_cols)
    for a, b in zip(res["flat"], res["nest"]):
        assert a[3] == b[3] and np.array_equal(a[4], b[4]) and _same(a[:3], b[:3])
    dix.set_latency_waves(0)                                         # the same batch on the throughput kernel: the nested table, same answers
    with _lib.tuning(**NEST):
        tk = dix.batch_search(Q[:256], 10, return_status=True)
        assert dix.last_walk_split().table_cols == n_min
    assert _same(tk[:3], res["flat"][0][:3])


def test_small_graphs_keep_the_per_level_table_by_default():
    """knob 1 (the default) builds the nested set only where it saves 4 096 columns or more: a graph of 20 000 vectors saves about
    1 650, so its launches run exactly what they ran before"""
    X, oix = _oracle(64, O.METRIC_COSINE, 10)
    dix = H.device_index_from_oracle(oix, X)
    _pin(dix, 1)
    n_all = sum(dix.level_count(l) for l in range(1, 11))
    assert 0 < n_all - dix.level_count(1) < 4096
    Q = H.queries_from(X, 300, noise=0.05, seed=4)
    dix.batch_search(Q, 10)
    assert dix.walk_table_info() == (1, n_all) and dix.last_walk_split().table_cols == n_all
