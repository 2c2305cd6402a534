"""GPU: one launch plan per search (cosdata_amd/csrc/walk_plan.h).  With every threshold pulled down to a few queries one small index
crosses them all — four-wave / one-wave latency kernel, level table, locality order, walk chain, side stream, the refill and the use of
the norms beside the adjacency: every launch keeps the bits of a handle over the same graph with every feature off, and reports the
table and the cut exactly where the recorded decisions (tests/golden/walk_plan_cases.txt) put them."""
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, TOP_K = 96, 10
LAT4, LAT, TABLE_MIN, ORDER_MIN, CHAIN_SIDE_MIN = 4, 16, 64, 128, 256


def _recorded(B, ef):
    """(use_table, ordered) of the fixture's case with this test's handle: u8 x 96, 3 layers, M 16 / 32, the knobs above"""
    want = [0, 0, 6, 8, 3, 16, 32, 64, 0, 0, B, ef, 1, 0, LAT, LAT4, 1, 1, TABLE_MIN, ORDER_MIN, CHAIN_SIDE_MIN, CHAIN_SIDE_MIN, 1, 1, 1]
    hits = []
    for line in open(os.path.join(ROOT, "tests", "golden", "walk_plan_cases.txt")):
        if line.startswith("#"):
            continue
        v = [int(x) for x in line.split()]
        if v[:25] == want and v[25] != 0 and v[27:31] == [1, 1, 1, 1]:      # a table operand, its buffer, one key level, order buffers
            hits.append((v[33], v[32]))
    assert len(hits) == 1, (B, ef, hits)
    return hits[0]


@pytest.fixture(scope="module")
def handles():
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X = H.clustered_corpus(3000, DIM, n_centers=16, seed=11)
    hp = dict(num_layers=3, ef_construction=32, ef_search=32, level_0_neighbors_count=32, neighbors_count=16)
    with _lib.tuning(walk_chain_min_b=CHAIN_SIDE_MIN, walk_side_min_b=CHAIN_SIDE_MIN):   # read at create
        dix = ca.HNSWIndex(DIM, ca.HNSWHyperParams(**hp), ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), seed=5)
    dix.upload_vectors(X).build(256)
    dix.set_latency_waves(LAT4)
    dix.set_latency_mode(LAT)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, TABLE_MIN)
    dix.set_walk_order(ORDER_MIN)
    off = ca.HNSWIndex(DIM, ca.HNSWHyperParams(**hp), ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), seed=5)
    off.upload_vectors(X).upload_graph(dix.download_graph(), dix.download_root())
    off.set_walk_order(0)
    off.set_walk_table(0, 0)
    off.set_latency_mode(0)
    off.set_latency_waves(0)
    Q = H.queries_from(X, 4096, noise=0.05, seed=3)
    return dix, off, X, Q


def _search(ix, Q):
    import torch
    dev = torch.device("cuda:0")
    B = Q.shape[0]
    q = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    ids = torch.zeros(B, TOP_K, dtype=torch.int32, device=dev)
    sc = torch.zeros(B, TOP_K, dtype=torch.float32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ix.batch_search_device(q.data_ptr(), B, TOP_K, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(np.uint32) for t in (ids, sc, cnt)) + (st.cpu().numpy(),)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_split(dix, B, ef):
    lmin, cols = dix.walk_table_info()
    cuts = dix.walk_order_cuts()
    assert lmin >= 1 and cols > 0 and cuts
    use_table, ordered = _recorded(B, ef)
    sp = dix.last_walk_split()
    assert sp.queries == B
    assert (sp.table_level_min, sp.table_cols) == ((lmin, cols) if use_table else (0, 0)), (B, ef)
    assert sp.cut_after_level == (cuts[0] if ordered else 0), (B, ef)
    assert (sp.table_evals > 0) == bool(use_table), (B, ef)
    return use_table, ordered


@pytest.mark.parametrize("B", [1, 4, 5, 16, 17, 63, 64, 127, 128, 255, 256, 300])
def test_every_threshold_keeps_the_bits_and_reports_its_plan(handles, B):
    dix, off, X, Q = handles
    q = Q[:B].copy()
    if B == 128:
        q[17] = -1.0                 # quantizes to the all-zero code: |q| = 0 -> CalculationError at the first evaluation
    got, ref = _search(dix, q), _search(off, q)
    use_table, ordered = _check_split(dix, B, 32)
    assert use_table == (B <= LAT4 or B >= TABLE_MIN) and ordered == (B >= ORDER_MIN)
    assert off.last_walk_split().table_level_min == 0 and off.last_walk_split().cut_after_level == 0
    assert _same(got, ref)
    bad = np.flatnonzero(ref[3])
    assert list(bad) == ([17] if B == 128 else []) and (B != 128 or ref[3][17] == 2)


def test_wide_beam_keeps_the_single_launch(handles):
    dix, off, X, Q = handles
    try:
        dix.set_ef_search(257)
        off.set_ef_search(257)
        got, ref = _search(dix, Q[:300]), _search(off, Q[:300])
        use_table, ordered = _check_split(dix, 300, 257)
        assert use_table and not ordered and dix.last_walk_split().cut_after_level == 0
        assert _same(got, ref) and not ref[3].any()
    finally:
        dix.set_ef_search(32)
        off.set_ef_search(32)


def test_norms_beside_the_adjacency_across_refill_and_use_thresholds(handles):
    """a root replaced on a live graph invalidates the norms: launches below the refill threshold gather, the first one at it refills,
    launches from the use threshold on read them — same bits throughout"""
    dix, off, X, Q = handles
    root = np.ascontiguousarray(X[7] * 0.5 + X[11] * 0.5)
    dix.set_root(root)
    off.set_root(root)
    for B in (1023, 1024, 4095, 4096):
        got, ref = _search(dix, Q[:B]), _search(off, Q[:B])
        _check_split(dix, B, 32)
        assert _same(got, ref) and not ref[3].any(), B
