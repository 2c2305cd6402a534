"""GPU: the level-table GEMM as a queue of work items shared by two launches (kernels_scan.hip level_table_areg, walk_plan.h
table_early_wgs).  A chained, ordered, gated launch issues the GEMM as an early part of `walk_table_early_wgs` workgroups behind the
previous chained walk's upper range and a full-width late part behind that walk's end; both claim (row group, column stripe) items
from one counter.  However the items are split between the parts, every result keeps its bits; the queries' code sums now come out
of the quantize kernel, and a wrong sum would shift every table entry."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

B, TOP_K = 300, 10        # two row groups of 256 queries, the last with 44 rows
EARLY = (0, 1, 3, 1000)   # one launch | nearly everything left to the late part | both parts work | clamped: the late part finds the queue empty


def _index(storage, dim):
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X = H.clustered_corpus(3000, dim, n_centers=16, seed=40 + dim)
    scale = 0.9 if storage == O.STORAGE_SUBBYTE else 1.0
    X = (X * scale).astype(np.float32)
    oix = H.oracle_index(X, storage, 2 if storage == O.STORAGE_SUBBYTE else 0, num_layers=5, ef_construction=32, ef_search=32,
                         level0_neighbors_count=32, neighbors_count=16)
    with _lib.tuning(walk_chain_min_b=0):             # read at create: every launch takes its place in the walk chain
        dix = H.device_index_from_oracle(oix, X)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, 1)
    dix.set_walk_order(1)
    Q = (H.queries_from(X, B, noise=0.05, seed=7) * scale).astype(np.float32)
    return oix, dix, Q


def _search_two_streams(dix, Q):
    """the same queries on two streams back to back: the second launch's GEMM waits on events of the first one's walk"""
    import torch
    dev = torch.device("cuda:0")
    q = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    outs = [(torch.zeros(B, TOP_K, dtype=torch.int32, device=dev), torch.zeros(B, TOP_K, dtype=torch.float32, device=dev),
             torch.zeros(B, dtype=torch.int32, device=dev), torch.full((B,), -1, dtype=torch.int32, device=dev)) for _ in streams]
    torch.cuda.synchronize()
    for s, (ids, sc, cnt, st) in zip(streams, outs):
        dix.batch_search_device(q.data_ptr(), B, TOP_K, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), st.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    splits = [dix.last_walk_split(s.cuda_stream) for s in streams]
    return [tuple(t.cpu().numpy().view(np.uint32) for t in o) for o in outs], splits


def _items(cols):
    """work items of the GEMM's queue for B queries x cols columns (walk_plan.h table_gemm_items): a table this small has stripes of the
    minimum of 2 column tiles on any device"""
    tiles, row_groups = (cols + 63) // 64, (B + 255) // 256
    assert tiles * row_groups < 2 * 24 * 2
    return (tiles + 1) // 2 * row_groups


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_against_oracle(oix, res, Q, sample):
    ids, sc, cnt, status = res
    oids, osc, ocnt = oix.search_batch(Q[sample], TOP_K, threads=4)[:3]
    assert not status.any()
    assert np.array_equal(cnt[sample], ocnt)
    for j, b in enumerate(sample):
        c = int(ocnt[j])
        assert np.array_equal(ids[b, :c], oids[j, :c].view(np.uint32)), f"query {b}"
        assert np.array_equal(sc[b, :c], osc[j, :c].view(np.uint32)), f"query {b}"


@pytest.mark.parametrize("storage,dim", [(O.STORAGE_U8, 128), (O.STORAGE_U8, 1024), (O.STORAGE_SUBBYTE, 128)])
def test_every_split_of_the_queue_keeps_the_bits(storage, dim):
    from cosdata_amd import _lib
    oix, dix, Q = _index(storage, dim)
    lmin, cols = dix.walk_table_info()
    assert lmin >= 1 and cols > 128 and 3 < _items(cols) < 1000   # several stripes per row group; setting 3 leaves work, 1000 is clamped
    dix.enable_timing(True)
    ref = None
    for early in EARLY:
        with _lib.tuning(walk_table_after_sort=2, walk_table_early_wgs=early):
            runs, splits = _search_two_streams(dix, Q)
        for sp in splits:                             # chained + ordered + table: the gated path, the early part as planned
            assert sp.queries == B and sp.table_cols == cols and sp.cut_after_level >= 1 and sp.table_evals > 0 and sp.table_ms > 0
            assert sp.table_early_wgs == min(early, _items(cols)), early
        if ref is None:
            ref = runs[0]
        for r in runs:
            assert _same(r, ref), early
    _check_against_oracle(oix, ref, Q, np.arange(0, B, 7))
    # without the table the walk dots the code rows itself: a wrong query sum in the GEMM's recentring term would show here
    import cosdata_amd as ca
    dix.set_walk_table(0, 0)
    with _lib.tuning(walk_table_after_sort=2, walk_table_early_wgs=0):
        runs, splits = _search_two_streams(dix, Q)
    assert all(sp.table_cols == 0 and sp.table_evals == 0 and sp.table_early_wgs == 0 for sp in splits)
    assert _same(runs[0], ref) and _same(runs[1], ref)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, 1)


def test_tile_gemm_path_takes_the_sums_from_the_quantizer_too():
    """96 dims: code rows that are no whole 64-byte chunks take the 256 x 128 tile GEMM, which has no queue — one launch whatever
    the knob says — and reads the same query sums"""
    from cosdata_amd import _lib
    oix, dix, Q = _index(O.STORAGE_U8, 96)
    assert dix.walk_table_info()[1] > 128
    res = {}
    for early in (0, 3):
        with _lib.tuning(walk_table_after_sort=2, walk_table_early_wgs=early):
            runs, splits = _search_two_streams(dix, Q)
        assert all(sp.table_evals > 0 and sp.cut_after_level >= 1 and sp.table_early_wgs == 0 for sp in splits)
        assert _same(runs[0], runs[1])
        res[early] = runs[0]
    assert _same(res[0], res[3])
    _check_against_oracle(oix, res[0], Q, np.arange(0, B, 7))
