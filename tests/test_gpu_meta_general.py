"""Metadata collections beyond walk_meta_kernel's domain (walk_meta_general_kernel, kernels_meta_general.hip): rows of more 16-byte
chunks than the fast kernel's registers hold, more than 64 scanned neighbour slots per node.  Every case is the device against the
oracle, list for list and bit for bit (tests/test_gpu_meta.py: _assert_same_filtered), on schema "A" over 300 embeddings and 12
queries; the guards computed from the ORACLE's output keep a case from passing because nothing happened."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import meta_append as MA
from tests import meta_helpers as MH
from tests.test_gpu_meta import _assert_same_filtered
from tests.test_gpu_meta_schemas import _cosine_guards, _nonempty

pytestmark = pytest.mark.gpu

N, NQ, TOP_K = 300, 12, 10
WIDE = dict(neighbors_count=128, level0_neighbors_count=128)     # two passes of 64 slots on every level


def _scenario(storage, res, dim, seed=4, **kw):
    return MH.Scenario(n=N, dim=dim, seed=seed, storage=storage, res=res, **MH.SCHEMAS["A"], **kw)


def _empty_handle(sc):
    """Scenario.device_index without its enable_metadata"""
    import cosdata_amd as ca
    p = sc.params
    hp = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                            level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
    dix = ca.HNSWIndex(sc.dim, hp, ca.DistanceMetric(p.metric), ca.StorageType(ca.StorageKind(p.storage), p.resolution),
                       (p.range_lo, p.range_hi), p.shortlist_size)
    return dix.upload_vectors(sc.X)


@pytest.mark.parametrize("storage,res,dim,kw", [
    (O.STORAGE_U8, 0, 2112, {}),                                   # 132 chunks: three passes of 64
    (O.STORAGE_U8, 0, 4114, {}),                                   # past four passes; a partial last chunk, a dim that is no multiple of four
    (O.STORAGE_SUBBYTE, 1, 8320, {}),                              # 65 chunks
    (O.STORAGE_SUBBYTE, 2, 4160, {}),
    (O.STORAGE_SUBBYTE, 3, 2080, {}),
    (O.STORAGE_U8, 0, 64, dict(shortlist_size=100, **WIDE)),       # a partial second pass of slots
    (O.STORAGE_U8, 0, 64, dict(shortlist_size=128, **WIDE)),       # two full passes
    (O.STORAGE_U8, 0, 2112, dict(metric=O.METRIC_DOT)),            # the vector distance decides for every node; nothing is dropped
])
def test_filtered_search_on_uploaded_oracle_graphs(storage, res, dim, kw):
    """every row was COS_ERR_UNIMPLEMENTED at enable_metadata before the general kernel"""
    sc = _scenario(storage, res, dim, **kw)
    oix = sc.oracle()
    dix = sc.device(oix)
    Q, off, rows, _ = sc.queries(nq=NQ, seed=7)
    if kw.get("metric") == O.METRIC_DOT:                           # (no -1.0 is dropped under the dot product: no level ever falls back)
        assert _nonempty(oix, Q, off, rows) * 2 >= NQ
    else:
        _cosine_guards(oix, Q, off, rows)                          # half of the queries find replicas, a level falls back to its entry node
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


@pytest.mark.parametrize("storage,res", [(O.STORAGE_U8, 0), (O.STORAGE_SUBBYTE, 1), (O.STORAGE_SUBBYTE, 2), (O.STORAGE_SUBBYTE, 3),
                                         (O.STORAGE_F16, 0), (O.STORAGE_F32, 0)])
def test_forced_general_kernel_on_what_the_fast_kernel_serves(storage, res):
    """meta_walk_general = 1 at dim 64: one chunk pass, one pass of slots, and ef_search at the edges of the pool widths"""
    from cosdata_amd import _lib
    sc = _scenario(storage, res, 64)
    oix = sc.oracle()
    dix = sc.device(oix)
    Q, off, rows, _ = sc.queries(nq=NQ, seed=7)
    with _lib.tuning(meta_walk_general=1):
        for ef in (1, 4, 5, 64, 257, 1024):
            oix.set_ef_search(ef)
            dix.set_ef_search(ef)
            _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


def _oracle_rounds(sc, bs):
    oix = O.OracleIndex(sc.params).set_vectors(sc.X)
    oix.meta_enable(sc.mdim, sc.replicas)
    oix.build()
    oix.meta_set_nodes(sc.node_ids, sc.mbits).meta_build_rounds(sc.max_levels, bs)
    return oix


@pytest.mark.parametrize("dim,kw", [(2112, {}), (64, dict(shortlist_size=100, **WIDE))])
def test_component_builder_equals_the_oracle_rounds_builder(dim, kw):
    """cos_index_build_meta == coso_meta_build_rounds slot for slot on every level (walk_meta_general_kernel<.., INDEXING>)"""
    sc = _scenario(O.STORAGE_U8, 0, dim, seed=11, **kw)
    oix = _oracle_rounds(sc, 48)
    dix = sc.device_index()
    dix.upload_graph(oix.export_graph(), oix.root_raw())
    dix.build_meta(sc.node_ids, sc.mbits, sc.max_levels, 48)
    MA.assert_same_levels(dix.download_meta_graph(), oix.meta_export_graph())
    Q, off, rows, _ = sc.queries(nq=NQ, seed=5)
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


def test_append_meta_continues_a_component_of_wide_rows():
    """build_meta(first 29 embeddings: 188 inserted nodes, a boundary of the batch-48 schedule) + append + append_meta == ONE oracle
    meta_build_rounds over the whole table"""
    sc = _scenario(O.STORAGE_U8, 0, 2112, seed=21)
    sp = MA.Split(sc, (29, N), 48)
    dix = sp.device_step(sp.device_old(48), 0, 48)
    oix = sp.oracle_whole(48)
    MA.assert_same_levels(dix.download_meta_graph(), oix.meta_export_graph())
    Q, off, rows, _ = sc.queries(nq=NQ, seed=5)
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


def test_a_row_beyond_one_workgroups_lds_is_refused_at_enable_time():
    """f32 x 38 000 dims, 128 slots: the general kernel would need 1 024 (filter) + 8 192 (popped list at ef 1024) + 1 024 (level list)
    + 1 024 (winner lists, filter dims) + 5 120 (pass window) + 152 000 (query row) + 16 = 168 400 bytes > 163 840; the plain walk
    (walk_general_kernel: 153.6 KB) still serves the handle"""
    import cosdata_amd as ca
    sc = MH.Scenario(n=40, dim=38000, seed=4, storage=O.STORAGE_F32, shortlist_size=128, **MH.SCHEMAS["A"], **WIDE)
    dix = _empty_handle(sc)
    with pytest.raises(ca.CosdataError) as ei:
        dix.enable_metadata(sc.mdim, sc.replicas)
    assert ei.value.status == O.ERR_UNIMPLEMENTED and "LDS" in str(ei.value)
    oix = O.OracleIndex(sc.params).set_vectors(sc.X)
    oix.build()
    dix.upload_graph(oix.export_graph(), oix.root_raw())
    Q = sc.queries(nq=4, seed=7)[0]
    ids, sims, counts = dix.ann_search_batch(Q)
    for b in range(Q.shape[0]):
        oi, osim, olc = oix.ann_search(Q[b])
        assert np.array_equal(counts[b], olc)
        got = np.concatenate([ids[b, s, :int(c)] for s, c in enumerate(olc)])
        assert np.array_equal(got, oi) and np.array_equal(np.concatenate([sims[b, s, :int(c)] for s, c in enumerate(olc)]).view(np.uint32), osim.view(np.uint32))


def test_ef_construction_beyond_the_register_pools_stays_refused():
    import cosdata_amd as ca
    sc = _scenario(O.STORAGE_U8, 0, 64, ef_construction=1025)
    with pytest.raises(ca.CosdataError) as ei:
        _empty_handle(sc).enable_metadata(sc.mdim, sc.replicas)
    assert ei.value.status == O.ERR_UNIMPLEMENTED
