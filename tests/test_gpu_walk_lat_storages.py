"""Both latency kernels over binary / octal codes and f16 / f32 rows (walk_latency_storages_domain, walk_plan.h): the oracle's ids,
score bits, counts and statuses, and — through cos_index_last_walk_kernel — the kernel that the setters asked for really walked."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

N = 3000
F32, F16, BIN, OCT = (O.STORAGE_F32, 0), (O.STORAGE_F16, 0), (O.STORAGE_SUBBYTE, 1), (O.STORAGE_SUBBYTE, 3)
# the smallest rows that can break each path: f32 tail only / 9 chain steps / tail of 4 / 128 steps + tail; f16 one element / not a
# multiple of 8 halves / across LDS tiles of the dimension; a partial chunk, several chunk passes and the 64-chunk limit of the codes
SHAPES = [(F32, d) for d in (7, 72, 100, 1027)] + [(F16, d) for d in (1, 72, 100, 1027)] + [(BIN, d) for d in (100, 1000, 8192)] + [(OCT, d) for d in (100, 2048)]
WIDE = [(F32, 100), (F16, 100), (BIN, 1000), (OCT, 100)]          # level-0 rows of 128 slots
OVER = [(F32, 2049), (F16, 2049), (BIN, 8193), (OCT, 2049)]       # one dimension (one chunk) over each row-width limit
CASES = [(st, d, m) for st, d in SHAPES for m in (O.METRIC_COSINE, O.METRIC_DOT) if not (st == F32 and m == O.METRIC_DOT)]  # f32 + dot: create refuses


@functools.lru_cache(maxsize=None)
def _graph(st, dim, m0):
    """corpus and the oracle's cosine graph over it — built once per shape (the oracle's f16 build at 1027 dims takes seconds)"""
    sub = st[0] == O.STORAGE_SUBBYTE
    X = H.uniform_corpus(N, dim, seed=dim) * np.float32(0.9) if sub else H.clustered_corpus(N, dim, n_centers=12, seed=dim)
    return X, H.oracle_index(X, st[0], st[1], num_layers=4, ef_construction=24, ef_search=16, neighbors_count=m0 // 2, level0_neighbors_count=m0)


@functools.lru_cache(maxsize=None)
def _pair(st, dim, metric, m0):
    """queries (33: one of zeros), oracle index and the device index loaded with its graph; the dot-product twin walks the cosine graph"""
    X, oix = _graph(st, dim, m0)
    if metric != O.METRIC_COSINE:
        p = dict(metric=metric, storage=st[0], resolution=st[1], num_layers=4, ef_search=16, neighbors_count=m0 // 2, level0_neighbors_count=m0)
        oix = O.OracleIndex(O.HNSWParams(dim=dim, **p)).set_vectors(X).import_graph(oix.export_graph(), oix.root_raw())
    Q = np.concatenate([H.queries_from(X, 24, seed=3), H.uniform_corpus(9, dim, seed=99) * np.float32(0.9)])
    Q[5] = 0.0
    return Q, oix, H.device_index_from_oracle(oix, X)


def _assert_walk(st, dim, metric, m0, waves, ef, B, kernel):
    Q, oix, dix = _pair(st, dim, metric, m0)
    Q = Q[:1] if B == 1 else Q
    oix.set_ef_search(ef)
    dix.set_ef_search(ef)
    dix.set_latency_mode(2048)
    dix.set_latency_waves(2048 if waves else 0)
    oids, osc, ocnt, orc, ostatus = oix.search_batch(Q, 10, threads=4, raise_on_error=False)
    ids, sc, cnt, rc, status = dix.batch_search(Q, 10, return_status=True)
    assert dix.last_walk_kernel() == kernel
    assert rc == orc and np.array_equal(status, ostatus)
    ok = ostatus == 0
    assert np.array_equal(cnt[ok], ocnt[ok]) and np.array_equal(ids[ok], oids[ok])
    assert np.array_equal(sc[ok].view(np.uint32), osc[ok].view(np.uint32))


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
