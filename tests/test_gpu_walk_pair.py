"""GPU: the pair walk (kernels_walk_pair.hip, walk_pair_plan.h, tuning knobs walk_pair / walk_pair_cache).  The last range of an
ordered launch is walked by workgroups of two waves, neighbours in the sorted order, and every code row a wave fetches is dotted with
both queries; the partner's integer dot goes into the partner's LDS cache, where its winners look before they fetch a row.  The
cached integer is the one the row block computes, so ids, score bits, counts, statuses and every per-level list must be what the same
launch returns with walk_pair = 0, and what the oracle returns.

Shapes: 20 000 vectors in 24 clusters, six levels that shrink by four (5 000 / 1 250 / 312 / 78 / 20 nodes); the table is pinned to the
levels >= 4 and the walk is cut after level 4, so the pair kernel walks the levels 3..0, level 3 being the level under the table — the
flagship's arrangement.  The mixed launch holds identical pairs, pairs from one cluster and unrelated queries, 301 queries in all, one
of them with a zero norm: that one fails above the cut, sorts last and takes the one place without a partner, so the two edge cases —
a wave that walks alone, a live wave beside a failed one — have launches of their own (121 queries, none failing; 120 queries, one
failing), in which every query is compared with the oracle."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_gpu_walk_table import _check_against_oracle, _same

pytestmark = pytest.mark.gpu

LAYERS, TAB_MIN, CUT, N = 5, 4, 4, 20000
BASE = dict(walk_up_table=2, walk_adj_mag=2)


@functools.lru_cache(maxsize=None)
def _corpus(dim):
    X = H.clustered_corpus(N, dim, n_centers=24, seed=1300 + dim)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _graph(dim, m0, m, values_range=(-1.0, 1.0)):
    """corpus, oracle index over a graph the device builder made, and the device index the tests search (same graph, uploaded)"""
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X = _corpus(dim)
    lo, hi = values_range
    hp = ca.HNSWHyperParams(num_layers=LAYERS, ef_construction=64, ef_search=112, level_0_neighbors_count=m0, neighbors_count=m)
    bix = ca.HNSWIndex(dim, hp, ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), (lo, hi), seed=5)
    bix.upload_vectors(X).build(512)
    op = O.HNSWParams(dim=dim, num_layers=LAYERS, ef_construction=64, ef_search=112, level0_neighbors_count=m0, neighbors_count=m, seed=5,
                      range_lo=lo, range_hi=hi)
    oix = O.OracleIndex(op).set_vectors(X).import_graph(bix.download_graph(), bix.download_root())
    del bix
    with _lib.tuning(walk_split_levels=1 << CUT):
        dix = H.device_index_from_oracle(oix, X)
    _pin(dix)
    return X, oix, dix


def _pin(dix):
    dix.set_latency_mode(0)
    dix.set_latency_waves(0)
    dix.set_walk_order(1)
    dix.set_walk_table(sum(dix.level_count(l) for l in range(TAB_MIN, LAYERS + 1)), 1)
    assert dix.walk_table_info()[0] == TAB_MIN and dix.walk_order_cuts() == [CUT]


def _make_queries(X, dim, m0, range_lo):
    rng = np.random.default_rng(dim + m0)
    noise = lambda k: 0.05 * rng.standard_normal((k, dim)).astype(np.float32)
    base = X[rng.integers(0, N, 60)] + noise(60)
    same = np.repeat(base, 2, axis=0)                                     # 60 identical pairs, neighbours in arrival order
    rows = rng.integers(0, N, 60)
    mates = np.argsort(-(X[rows] @ X.T), axis=1)[:, 1 + rng.integers(0, 20)]   # one of the 20 nearest rows: the same cluster
    cluster = np.empty((120, dim), np.float32)
    cluster[0::2], cluster[1::2] = X[rows] + noise(60), X[mates] + noise(60)
    other = X[rng.integers(0, N, 61)] + noise(61)
    Q = np.ascontiguousarray(np.concatenate([same, cluster, other]).astype(np.float32))
    Q[150] = range_lo                                                     # the all-zero code: |q| = 0, CalculationError at the top level
    assert Q.shape[0] == 301
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=None)
def _queries(dim, m0, m, values_range=(-1.0, 1.0)):
    return _make_queries(_corpus(dim), dim, m0, values_range[0])


def _run(dix, Q, pair, cache=512, top_k=10, taken=True):
    """taken = False: the plan must leave the launch to walk_kernel although the knob asks for pairs"""
    from cosdata_amd import _lib
    with _lib.tuning(walk_pair=pair, walk_pair_cache=cache, **BASE):
        ids, sc, cnt, rc, status = dix.batch_search(Q, top_k, return_status=True)
        ps = dix.last_pair_stats()
        sp = dix.last_walk_split()
        walk = dix.ann_search_batch(Q[status == 0])
        ps_walk = dix.last_pair_stats()
    assert sp.cut_after_level == CUT and sp.table_level_min == TAB_MIN
    for p in (ps, ps_walk):
        assert p.cache_entries == (cache if pair and taken else 0)        # the launch really walked in pairs / really did not
        if not (pair and taken):
            assert p.cache_hits == 0 and p.row_evals == 0
    return (ids, sc, cnt, status), rc, walk, ps, sp


def _check_lists_against_oracle(oix, walk, Qok, sample):
    ids, sims, counts = walk
    for b in sample:
        oi, osim, olc = oix.ann_search(Qok[b])
        assert np.array_equal(counts[b], olc), f"query {b}"
        off = 0
        for s, c in enumerate(int(c) for c in olc):
            assert np.array_equal(ids[b, s, :c], oi[off:off + c]), f"query {b} slot {s}"
            assert np.array_equal(sims[b, s, :c].view(np.uint32), osim[off:off + c].view(np.uint32)), f"query {b} slot {s}"
            off += c


def _compare(dix, oix, Q, cache, zero=(), every=False):
    """every: all queries that did not fail are compared with the oracle, results and per-level lists, not a sample of them"""
    off, rc0, walk0, _, sp0 = _run(dix, Q, 0)
    on, rc2, walk2, ps, sp2 = _run(dix, Q, 2, cache)
    assert rc0 == rc2 and _same(on, off) and _same(walk2, walk0)          # ids, score bits, counts, statuses; every per-level list
    assert sp2.lower_evals == sp0.lower_evals and sp2.upper_evals == sp0.upper_evals   # the same walk, evaluation for evaluation
    assert ps.cache_hits + ps.row_evals > 0 and ps.cache_hits + ps.row_evals <= sp2.lower_evals
    status = on[3]
    assert sorted(np.flatnonzero(status)) == sorted(zero) and all(status[z] == 2 for z in zero)
    ok = np.flatnonzero(status == 0)
    _check_against_oracle(oix, on[:3], Q, 10, ok if every else ok[::7])
    _check_lists_against_oracle(oix, walk2, Q[ok], range(0, ok.size, 1 if every else 23))
    print(f"pair walk: {ps.cache_hits} hits, {ps.row_evals} rows fetched, {sp2.lower_evals} evaluations below the cut")
    return on, walk2, ps


# dims 1024 (64 chunks: every lane holds one) and 1000 (63 chunks, the last one half padding); M0 256 / M 64 and M0 64 / M 32; ef 64 (one
# key per lane), 112 (two), 256 (four); caches of 256 and 1024 entries
CASES = [
    (1024, 256, 64, 112, 256),
    (1024, 256, 64, 64, 1024),
    (1024, 256, 64, 256, 1024),
    (1000, 64, 32, 64, 256),
    (1000, 64, 32, 112, 1024),
    (1000, 64, 32, 256, 256),
]


@pytest.mark.parametrize("dim,m0,m,ef,cache", CASES)
def test_pairs_keep_every_bit(dim, m0, m, ef, cache):
    X, oix, dix = _graph(dim, m0, m)
    Q = _queries(dim, m0, m)
    dix.set_ef_search(ef)
    oix.set_ef_search(ef)
    try:
        _pin(dix)
        _compare(dix, oix, Q, cache, zero=(150,))                         # (query 150 fails above the cut and takes the place without a partner)
    finally:
        dix.set_ef_search(112)
        oix.set_ef_search(112)


def test_identical_pairs_hit_the_cache_and_repeats_return_the_same_bytes():
    X, oix, dix = _graph(1024, 256, 64)
    _pin(dix)
    Q = np.ascontiguousarray(_queries(1024, 256, 64)[:120])               # the 60 identical pairs
    on, walk, ps = _compare(dix, oix, Q, 512)
    assert ps.cache_hits > 0                                              # the path cannot pass unused
    assert _same(tuple(a[0::2] for a in on), tuple(a[1::2] for a in on))
    for _ in range(2):                                                    # hit counts may differ from run to run, results may not
        again, _, walk_again, ps_again, _ = _run(dix, Q, 2, 512)
        assert _same(again, on) and _same(walk_again, walk) and ps_again.cache_hits > 0


def test_odd_launch_without_a_failing_query_the_last_wave_walks_alone():
    """121 queries, none fails: the query at the last place of the sorted order goes to wave 0 of workgroup 60, which has no partner
    (zero partner chunk, no inserts, an own cache nobody fills) and walks all four levels.  Which query that is is not known here, so
    every query's result and every per-level list is compared with the oracle's."""
    X, oix, dix = _graph(1000, 64, 32)
    _pin(dix)
    Q = np.ascontiguousarray(_queries(1000, 64, 32)[:121])               # (the zero-norm query is number 150)
    on, _, ps = _compare(dix, oix, Q, 256, every=True)
    assert np.count_nonzero(on[3]) == 0 and ps.cache_hits > 0


def test_the_partner_of_a_zero_norm_query_answers_like_the_oracle():
    """120 queries, one of them with a zero norm.  It fails above the cut, takes the largest order key and sorts to place 119; the
    deal in twos gives places 118 and 119 to one workgroup, so the query at place 118 is a live wave whose partner returned at once.
    Every one of the 119 others must answer COS_OK with the oracle's result and the oracle's per-level lists."""
    X, oix, dix = _graph(1024, 256, 64)
    _pin(dix)
    Q = np.array(_queries(1024, 256, 64)[:120])
    Q[37] = oix.params.range_lo
    on, _, ps = _compare(dix, oix, Q, 512, zero=(37,), every=True)
    assert np.count_nonzero(on[3] == 0) == 119


def test_a_cache_that_does_not_fit_leaves_the_launch_to_walk_kernel():
    """walk_pair_cache values outside walk_pair_plan.h's domain (4096 entries: two waves of 39 KB; 500: no power of two) are no error:
    the launch runs walk_kernel and returns the same bytes"""
    X, oix, dix = _graph(1024, 256, 64)
    _pin(dix)
    Q = np.ascontiguousarray(_queries(1024, 256, 64)[:120])
    off, rc0, walk0, _, _ = _run(dix, Q, 0)
    for cache in (4096, 500):
        got, rc, walk, ps, _ = _run(dix, Q, 2, cache, taken=False)
        assert rc == rc0 and _same(got, off) and _same(walk, walk0) and ps.cache_hits == 0
    got, rc, walk, ps, _ = _run(dix, Q, 2, 2048)                          # the largest cache: 2 x 22.5 KB
    assert rc == rc0 and _same(got, off) and _same(walk, walk0) and ps.cache_entries == 2048


def test_id_base_other_than_zero():
    from cosdata_amd import _lib
    X, oix, _ = _graph(1000, 64, 32)
    with _lib.tuning(walk_split_levels=1 << CUT):
        dix = H.device_index_from_oracle(oix, X, id_base=7001)
    _pin(dix)
    Q = _queries(1000, 64, 32)
    off, _, walk0, _, _ = _run(dix, Q, 0)
    on, _, walk2, ps, _ = _run(dix, Q, 2, 256)
    assert _same(on, off) and _same(walk2, walk0) and ps.cache_hits + ps.row_evals > 0
    ok = np.flatnonzero(on[3] == 0)[::9]
    oids, osc, ocnt = oix.search_batch(Q[ok], 10, threads=4)[:3]
    assert np.array_equal(on[2][ok], ocnt) and np.array_equal(on[1][ok].view(np.uint32), osc.view(np.uint32))
    assert np.array_equal(on[0][ok], np.where(np.arange(10)[None, :] < ocnt[:, None], oids + 7001, oids).astype(np.uint32))
