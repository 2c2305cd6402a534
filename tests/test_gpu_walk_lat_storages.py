"""Both latency kernels over binary / octal codes and f16 / f32 rows (walk_latency_storages_domain, walk_plan.h): the oracle's ids,
score bits, counts and statuses, and — through cos_index_last_walk_kernel — the kernel that the setters asked for really walked.
The evaluation blocks themselves are held to the oracle value by value by tests/test_gpu_lat_dots.py; here is what only a walk shows:
the kernels' own LDS offsets at the row-width limit, the pool switch of the launchers, a zero-norm row met in the middle of a walk, and
the kernel a handle picks when nobody told it."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

N = 3000
N_LIMIT = 1000  # rows of 2048 dims: the oracle's build of f16 rows is a scalar loop
F32, F16, BIN, OCT = (O.STORAGE_F32, 0), (O.STORAGE_F16, 0), (O.STORAGE_SUBBYTE, 1), (O.STORAGE_SUBBYTE, 3)
# the smallest rows that can break each path: f32 tail only / 9 chain steps / tail of 4 / 128 steps + tail; f16 one element / not a
# multiple of 8 halves / across LDS tiles of the dimension; a partial chunk, several chunk passes and the 64-chunk limit of the codes
SHAPES = [(F32, d) for d in (7, 72, 100, 1027)] + [(F16, d) for d in (1, 72, 100, 1027)] + [(BIN, d) for d in (100, 1000, 8192)] + [(OCT, d) for d in (100, 2048)]
WIDE = [(F32, 100), (F16, 100), (BIN, 1000), (OCT, 100)]          # level-0 rows of 128 slots
OVER = [(F32, 2049), (F16, 2049), (BIN, 8193), (OCT, 2049)]       # one dimension (one chunk) over each row-width limit
CASES = [(st, d, m) for st, d in SHAPES for m in (O.METRIC_COSINE, O.METRIC_DOT) if not (st == F32 and m == O.METRIC_DOT)]  # f32 + dot: create refuses
# WALK_LAT_FLOAT_MAX_DIM: 8 KB of query in LDS behind each kernel's own arrays, where the kernels' hand-written offsets (s_q, s_tile,
# my_tile) must agree with walk_lat_lds_bytes / walk_lat4_lds_bytes — at ef 256, each kernel's largest layout
LIMIT = [(F32, O.METRIC_COSINE), (F16, O.METRIC_COSINE), (F16, O.METRIC_DOT)]
F16_TILE_EDGES = (64, 65, 128, 129)                               # one tile of the four-wave kernel (64 dims) and of the one-wave kernel (128), and one element more
ONE_PER_STORAGE = [(F32, 72), (F16, 72), (BIN, 1000), (OCT, 100)]  # shapes of SHAPES: their graphs are built once
POOL_EFS = (1, 64, 65)                                            # launch_lat_r / launch_lat4_r: pools of 64 keys up to ef 64, of 256 above
N_DRAWN_ZEROED = 2


@functools.lru_cache(maxsize=None)
def _graph(st, dim, m0, n=N):
    """corpus and the oracle's cosine graph over it — built once per shape (the oracle's f16 build at 1027 dims takes seconds)"""
    sub = st[0] == O.STORAGE_SUBBYTE
    X = H.uniform_corpus(n, dim, seed=dim) * np.float32(0.9) if sub else H.clustered_corpus(n, dim, n_centers=12, seed=dim)
    return X, H.oracle_index(X, st[0], st[1], num_layers=4, ef_construction=24, ef_search=16, neighbors_count=m0 // 2, level0_neighbors_count=m0)


def _queries(X):
    """33 queries: 24 near corpus rows, 9 anywhere, one of them all zero"""
    Q = np.concatenate([H.queries_from(X, 24, seed=3), H.uniform_corpus(9, X.shape[1], seed=99) * np.float32(0.9)])
    Q[5] = 0.0
    return Q


@functools.lru_cache(maxsize=None)
def _oracle_pair(st, dim, metric, m0, n=N, zeroed=False):
    """corpus, queries and the oracle index.  The dot-product twin walks the cosine graph.  zeroed: the same graph over the corpus with
    a few rows set to zero (norm 0: cosine against them is a CalculationError) — the row nearest to query 0 and N_DRAWN_ZEROED drawn,
    all of level 0 only: a zero row on an upper level, or more of them, fails every walk of a 3000-row graph with rows of 64 slots"""
    X, oix = _graph(st, dim, m0, n)
    Q = _queries(X)
    if zeroed:
        upper = oix.export_graph()[1][0]
        rows = np.setdiff1d(np.arange(n), upper)
        near = int(np.argmax(X @ Q[0]))
        drawn = np.random.default_rng(17).choice(rows[rows != near], N_DRAWN_ZEROED, replace=False)
        X = X.copy()
        X[np.concatenate([drawn, [near] if near in rows else []]).astype(np.int64)] = 0.0
    if metric != O.METRIC_COSINE or zeroed:
        p = dict(metric=metric, storage=st[0], resolution=st[1], num_layers=4, ef_search=16, neighbors_count=m0 // 2, level0_neighbors_count=m0)
        oix = O.OracleIndex(O.HNSWParams(dim=dim, **p)).set_vectors(X).import_graph(oix.export_graph(), oix.root_raw())
    return X, Q, oix


@functools.lru_cache(maxsize=None)
def _pair(st, dim, metric, m0, n=N, zeroed=False):
    """queries, oracle index and the device index loaded with its graph"""
    X, Q, oix = _oracle_pair(st, dim, metric, m0, n, zeroed)
    return Q, oix, H.device_index_from_oracle(oix, X)


def _assert_same(dix, got, want, kernel):
    (ids, sc, cnt, rc, status), (oids, osc, ocnt, orc, ostatus) = got, want
    assert dix.last_walk_kernel() == kernel
    assert rc == orc and np.array_equal(status, ostatus)
    ok = ostatus == 0
    assert np.array_equal(cnt[ok], ocnt[ok])
    # a call promises the first `count` entries of a list (ef 1 pops the start node alone: level 0 returns nothing)
    held = ok[:, None] & (np.arange(ids.shape[1])[None, :] < ocnt.reshape(-1, 1))
    assert np.array_equal(ids[held], oids[held])
    assert np.array_equal(sc.view(np.uint32)[held], osc.view(np.uint32)[held])


def _assert_walk(st, dim, metric, m0, waves, ef, B, kernel, n=N, zeroed=False):
    Q, oix, dix = _pair(st, dim, metric, m0, n, zeroed)
    Q = Q[:1] if B == 1 else Q
    oix.set_ef_search(ef)
    dix.set_ef_search(ef)
    dix.set_latency_mode(2048)
    dix.set_latency_waves(2048 if waves else 0)
    want = oix.search_batch(Q, 10, threads=4, raise_on_error=False)
    _assert_same(dix, dix.batch_search(Q, 10, return_status=True), want, kernel)
    return want


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("ef", [16, 256])
@pytest.mark.parametrize("waves", [0, 1])
@pytest.mark.parametrize("st,dim,metric", CASES)
def test_latency_kernels_match_oracle(st, dim, metric, waves, ef, B):
    _assert_walk(st, dim, metric, 64, waves, ef, B, "latency_waves" if waves else "latency")


@pytest.mark.parametrize("waves", [0, 1])
@pytest.mark.parametrize("st,dim", WIDE)
def test_rows_of_128_slots_stay_on_the_one_wave_kernel(st, dim, waves):
    """the four-wave kernel's claim table is sized for rows of <= 64 slots: it declines, the one-wave kernel walks"""
    _assert_walk(st, dim, O.METRIC_COSINE, 128, waves, 256, 33, "latency")


@pytest.mark.parametrize("st,dim", OVER)
def test_rows_over_the_limit_keep_their_kernel(st, dim):
    """float rows over 2048 dimensions stay on the throughput kernel; code rows over 64 chunks on walk_general_kernel, as before"""
    _assert_walk(st, dim, O.METRIC_COSINE, 16, 1, 16, 33, "general" if st[0] == O.STORAGE_SUBBYTE else "throughput")  # (narrow rows: a cheap oracle build)


@pytest.mark.parametrize("waves", [0, 1])
@pytest.mark.parametrize("st,metric", LIMIT)
def test_float_rows_at_the_width_limit(st, metric, waves):
    """2048 dims, ef 256, 33 queries: each kernel at its largest LDS (one wave 33 040 B with rows of 256 slots, four waves 54 320 B)"""
    _assert_walk(st, 2048, metric, 64, waves, 256, 33, "latency_waves" if waves else "latency", n=N_LIMIT)


@pytest.mark.parametrize("st", [F32, F16])
def test_float_rows_at_the_width_limit_under_rows_of_128_slots(st):
    """... and the one-wave kernel's filter of a 128-slot level in front of the query"""
    _assert_walk(st, 2048, O.METRIC_COSINE, 128, 1, 256, 33, "latency", n=N_LIMIT)


@pytest.mark.parametrize("waves", [0, 1])
@pytest.mark.parametrize("dim", F16_TILE_EDGES)
def test_f16_rows_at_the_tile_edges(dim, waves):
    _assert_walk(F16, dim, O.METRIC_COSINE, 64, waves, 256, 33, "latency_waves" if waves else "latency", n=N // 2)


@pytest.mark.parametrize("ef", POOL_EFS)
@pytest.mark.parametrize("waves", [0, 1])
@pytest.mark.parametrize("st,dim", ONE_PER_STORAGE)
def test_both_sides_of_the_pool_switch(st, dim, waves, ef):
    _assert_walk(st, dim, O.METRIC_COSINE, 64, waves, ef, 33, "latency_waves" if waves else "latency")


@pytest.mark.parametrize("waves", [0, 1])
@pytest.mark.parametrize("st,dim", ONE_PER_STORAGE)
def test_one_zero_norm_row_among_good_candidates(st, dim, waves):
    """the oracle's graph over the corpus, imported over the corpus with two or three rows zeroed: a walk that wins one of them is a
    CalculationError, the others succeed — one flagged word among good ones, where the zero query Q[5] flags every candidate"""
    want = _assert_walk(st, dim, O.METRIC_COSINE, 64, waves, 16, 33, "latency_waves" if waves else "latency", zeroed=True)
    status = np.delete(want[4], 5)
    assert (status == O.ERR_CALCULATION).sum() >= 4 and (status == O.OK).sum() >= 4, status


# walk_latency_default_max_B (walk_plan.h) read off the code: (launch sizes at the handle's ef 16 | at ef 257) -> kernel
DEFAULTS = [(F16, 72, {256: "latency_waves", 257: "latency", 2048: "latency", 2049: "throughput"}), (OCT, 100, {256: "latency_waves", 257: "latency", 2048: "latency", 2049: "throughput"}),
            (F32, 72, {256: "latency_waves", 257: "throughput"}), (BIN, 1000, {256: "throughput"})]


@pytest.mark.parametrize("st,dim,expect", DEFAULTS)
def test_a_fresh_handle_takes_the_measured_kernel(st, dim, expect):
    """no latency setter, no tuning override, rows of 64 slots: the defaults that route real traffic"""
    X, _, oix = _oracle_pair(st, dim, O.METRIC_COSINE, 64)
    Q = H.queries_from(X, max(expect), seed=7)
    dix = H.device_index_from_oracle(oix, X)
    try:
        for ef, sizes in ((16, expect), (257, {256: "throughput"} if st in (F16, OCT) else {})):
            if not sizes:
                continue
            oix.set_ef_search(ef)
            dix.set_ef_search(ef)
            want = oix.search_batch(Q[:max(sizes)], 10, threads=4, raise_on_error=False)
            for B, kernel in sizes.items():
                _assert_same(dix, dix.batch_search(Q[:B], 10, return_status=True), tuple(w[:B] if isinstance(w, np.ndarray) else w for w in want), kernel)
    finally:
        dix.close()
