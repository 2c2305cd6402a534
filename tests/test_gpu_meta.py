"""Metadata-filtered search on the device vs the oracle on the same collection: per-level lists of the
filtered ann_search, final results (replica ids + exact scores), error behaviour, and the BASE graph of a metadata collection
(ids = vector row x max_replicas) for unfiltered search and for the device builder."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import meta_helpers as MH
from tests.test_gpu_parity import _assert_same_search, _assert_same_walk

pytestmark = pytest.mark.gpu


def _assert_same_filtered(sc, oix, dix, Q, off, rows, top_k):
    ids, sims, counts = dix.ann_search_filtered(Q, off, rows.astype(np.int8))
    for b in range(Q.shape[0]):
        oi, osim, olc = oix.ann_search_filtered(Q[b], rows[off[b]:off[b + 1]])
        assert np.array_equal(counts[b], olc), f"query {b}: level counts {counts[b]} vs {olc}"
        o = 0
        for s, c in enumerate(olc):
            c = int(c)
            assert np.array_equal(ids[b, s, :c], oi[o:o + c]), f"query {b} slot {s}: ids differ\n{ids[b, s, :c]}\n{oi[o:o + c]}"
            assert np.array_equal(sims[b, s, :c].view(np.uint32), osim[o:o + c].view(np.uint32)), f"query {b} slot {s}: sims differ"
            o += c
    gi, gs, gc = dix.search_filtered(Q, off, rows.astype(np.int8), top_k)
    ei, es, ec = oix.search_filtered_batch(Q, off, rows, top_k, threads=4)
    assert np.array_equal(gc, ec)
    for b in range(Q.shape[0]):
        c = int(gc[b])
        assert np.array_equal(gi[b, :c], ei[b, :c]), f"query {b}: final ids differ"
        assert np.array_equal(gs[b, :c].view(np.uint32), es[b, :c].view(np.uint32)), f"query {b}: final scores differ"
    return gi, gc


@pytest.mark.parametrize("storage,res,dim", [(O.STORAGE_U8, 0, 64), (O.STORAGE_U8, 0, 1024), (O.STORAGE_SUBBYTE, 2, 128), (O.STORAGE_F32, 0, 96),
                                             (O.STORAGE_F16, 0, 72)])
def test_filtered_search_matches_oracle(storage, res, dim):
    sc = MH.Scenario(n=1500, dim=dim, seed=4, storage=storage, res=res)
    oix = sc.oracle()
    dix = sc.device(oix)
    Q, off, rows, desc = sc.queries(nq=36, seed=7)
    gi, gc = _assert_same_filtered(sc, oix, dix, Q, off, rows, 10)
    assert (gc > 0).sum() >= 18                                   # is / and / or filters do find their replicas
    for ef in (16, 200, 400, 900):                                # (900: the 64 x 16-key pool of round 5)
        oix.set_ef_search(ef)
        dix.set_ef_search(ef)
        _assert_same_filtered(sc, oix, dix, Q[:12], off[:13], rows[:off[12]], 5)


def test_unfiltered_search_and_builder_on_a_metadata_collection():
    """the Base replicas: ids are vector row x 4 in the visited filter, the lists and the results"""
    import cosdata_amd as ca
    sc = MH.Scenario(n=2500, dim=96, seed=8)
    oix = sc.oracle()
    dix = sc.device(oix)
    Q, *_ = sc.queries(nq=32, seed=2)
    _assert_same_walk(oix, dix, Q)
    _assert_same_search(oix, dix, Q, 10)
    assert (dix.batch_search(Q, 10)[0] % 4 == 0).all()
    # device builder on the same collection == the oracle's rounds builder (both number the nodes row x 4)
    p = sc.params
    o2 = O.OracleIndex(p).set_vectors(sc.X)
    o2.meta_enable(MH.MDIM, MH.REPLICAS)
    o2.build_rounds(256, greedy=False)
    hp = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                            level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
    d2 = ca.HNSWIndex(sc.dim, hp, seed=p.seed)
    d2.upload_vectors(sc.X).enable_metadata(MH.MDIM, MH.REPLICAS)
    d2.build(256)
    for (di, dn), (oi, on) in zip(d2.download_graph(), o2.export_graph()):
        assert np.array_equal(di, oi) and np.array_equal(dn, on)


def test_filtered_search_argument_and_error_contract():
    import cosdata_amd as ca
    sc = MH.Scenario(n=600, dim=32, seed=1)
    oix = sc.oracle()
    dix = sc.device(oix)
    Q, off, rows, _ = sc.queries(nq=6, seed=1)
    with pytest.raises(ca.CosdataError) as ei:                     # a query without a filter belongs to cos_search_batch
        dix.search_filtered(Q[:2], np.array([0, 1, 1], np.uint32), rows[:1].astype(np.int8), 5)
    assert ei.value.status == 3
    Qz = Q.copy()
    Qz[1] = -1.0                                                   # zero quantized norm: CalculationError once a vector cosine is needed
    g = dix.search_filtered(Qz, off, rows.astype(np.int8), 5, return_status=True)
    e = oix.search_filtered_batch(Qz, off, rows, 5, threads=2, raise_on_error=False)
    assert g[3] == e[3] and np.array_equal(g[4], e[4])
    plain = ca.HNSWIndex(32, ca.HNSWHyperParams(num_layers=2))
    plain.upload_vectors(sc.X)
    with pytest.raises(ca.CosdataError) as ei:
        plain.mdim = MH.MDIM
        plain.search_filtered(Q[:1], off[:2], rows[:off[1]].astype(np.int8), 5)
    assert ei.value.status == 6                                    # NotReady: no metadata component


def test_reuploading_vectors_resets_the_whole_metadata_component():
    """cos_index_upload_vectors freed the metadata LEVELS but kept id_stride, mdim, the node table and the metadata
    dimensions, so a later cos_index_upload_meta_graph_level passed its checks and mapped stale replica ids to rows beyond the new n.
    Now the handle is a plain collection again after a re-upload, and a node table with out-of-range replicas is refused."""
    import ctypes as C
    import cosdata_amd as ca
    sc = MH.Scenario(n=1200, dim=64, seed=3)
    oix = sc.oracle()
    dix = sc.device(oix)
    levels = oix.meta_export_graph()
    X_small = sc.X[:300]
    dix.upload_vectors(X_small)                              # fewer vectors than the stale replica ids refer to
    lid, nbr = np.ascontiguousarray(levels[0][0], np.uint32), np.ascontiguousarray(levels[0][1], np.uint32)
    rc = ca._lib.lib().cos_index_upload_meta_graph_level(dix._h, 0, lid.size, lid.ctypes.data_as(C.c_void_p), nbr.ctypes.data_as(C.c_void_p))
    assert rc == 6                                           # no schema any more: NotReady, not an out-of-bounds walk
    with pytest.raises(ca.CosdataError) as ei:
        dix.mdim = MH.MDIM
        dix.upload_meta_graph(sc.node_ids, sc.mbits, levels)
    assert ei.value.status == 6
    # the handle works as a plain (stride-1) collection: ids are rows again
    dix.build(64)
    ids = dix.batch_search(X_small[:8], 3)[0]
    assert (ids[:, 0] == np.arange(8)).all()
    # with the schema enabled again, the stale node table (replicas of rows >= 300) is refused by its range check
    dix.upload_vectors(X_small).enable_metadata(MH.MDIM, MH.REPLICAS)
    with pytest.raises(ca.CosdataError) as ei:
        dix.upload_meta_graph(sc.node_ids, sc.mbits, levels)
    assert ei.value.status == 3


@pytest.mark.parametrize("storage,res,dim,bs", [(O.STORAGE_U8, 0, 64, 1), (O.STORAGE_U8, 0, 64, 48), (O.STORAGE_U8, 0, 96, 4096), (O.STORAGE_SUBBYTE, 2, 128, 256),
                                                (O.STORAGE_F32, 0, 48, 200), (O.STORAGE_F16, 0, 72, 128)])
def test_component_built_on_the_device_equals_the_oracle_rounds_builder(storage, res, dim, bs):
    """cos_index_build_meta (index-mode walk_meta_kernel + the link kernels with the refusal rules of vector_store.rs:1017-1041) ==
    coso_meta_build_rounds with the same batch size, slot for slot on every level; batches of one == the sequential reference
    order; filtered search on the device-built component == the oracle on its own"""
    import cosdata_amd as ca
    sc = MH.Scenario(n=1300, dim=dim, seed=11, storage=storage, res=res)
    oix = O.OracleIndex(sc.params).set_vectors(sc.X)
    oix.meta_enable(MH.MDIM, MH.REPLICAS)
    oix.build()
    oix.meta_set_nodes(sc.node_ids, sc.mbits).meta_build_rounds(sc.max_levels, bs)
    p = sc.params
    hp = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                            level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
    dix = ca.HNSWIndex(sc.dim, hp, ca.DistanceMetric(p.metric), ca.StorageType(ca.StorageKind(p.storage), p.resolution), (p.range_lo, p.range_hi),
                       p.shortlist_size)
    dix.upload_vectors(sc.X).enable_metadata(MH.MDIM, MH.REPLICAS)
    dix.upload_graph(oix.export_graph(), oix.root_raw())
    dix.build_meta(sc.node_ids, sc.mbits, sc.max_levels, bs)
    want = oix.meta_export_graph()
    got = dix.download_meta_graph()
    for l, ((gi, gn), (ei, en)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, ei), f"level {l}: node sets differ"
        assert np.array_equal(gn, en), f"level {l}: adjacency differs in {np.count_nonzero((gn != en).any(axis=1))} of {len(en)} rows"
    Q, off, rows, desc = sc.queries(nq=24, seed=5)
    _assert_same_filtered(sc, oix, dix, Q, off, rows, 10)


def test_filtered_search_on_two_shards_of_a_metadata_collection():
    """round 6: a metadata collection may be sharded by embedding range — shard s holds embeddings [e0, e0 + n) and returns replica ids
    id_base + row x max_replicas + i with id_base = e0 x max_replicas.  Two shards, the same filtered queries on both, merged with the
    shard-exchange merge rule == the oracle's two filtered searches (ids shifted) under the same rule."""
    import cosdata_amd as ca
    from tests.test_sharded_merge import _merge_numpy
    A = MH.Scenario(n=900, dim=64, seed=4)
    Bs = MH.Scenario(n=700, dim=64, seed=9)
    oa, ob = A.oracle(), Bs.oracle()
    base_b = 900 * MH.REPLICAS
    da, db = A.device(oa), Bs.device(ob, id_base=base_b)
    Q, off, rows, _ = A.queries(nq=30, seed=5)
    k = 10
    parts_d, parts_o = [], []
    for dix, oix, base in ((da, oa, 0), (db, ob, base_b)):
        gi, gs, gc = dix.search_filtered(Q, off, rows.astype(np.int8), k)
        ei, es, ec = oix.search_filtered_batch(Q, off, rows, k, threads=4)
        assert np.array_equal(gc, ec)
        for b in range(Q.shape[0]):
            c = int(gc[b])
            assert np.array_equal(gi[b, :c], ei[b, :c] + base) and np.array_equal(gs[b, :c].view(np.uint32), es[b, :c].view(np.uint32)), f"shard base {base}, query {b}"
        parts_d.append((gi, gs, gc))
        parts_o.append((np.where(np.arange(k)[None, :] < ec[:, None], ei + base, ei).astype(np.uint32), es, ec))
    md = _merge_numpy(np.stack([p[0] for p in parts_d]), np.stack([p[1] for p in parts_d]), np.stack([p[2] for p in parts_d]), k)
    mo = _merge_numpy(np.stack([p[0] for p in parts_o]), np.stack([p[1] for p in parts_o]), np.stack([p[2] for p in parts_o]), k)
    assert np.array_equal(md[2], mo[2])
    for b in range(Q.shape[0]):
        c = int(md[2][b])
        assert np.array_equal(md[0][b, :c], mo[0][b, :c]) and np.array_equal(md[1][b, :c].view(np.uint32), mo[1][b, :c].view(np.uint32))
    owners = {int(i) >= base_b for b in range(Q.shape[0]) for i in md[0][b, :int(md[2][b])]}
    assert owners == {False, True}                               # both shards contribute to merged answers
    with pytest.raises(ca.CosdataError):                         # a base that is not a whole number of embeddings is refused
        Bs.device(ob, id_base=base_b + 1)


def test_failed_component_build_leaves_no_component():
    """a replica whose vector has zero norm aborts its insertion walk with CalculationError (cosine.rs:228-232), as on the base graph
    (tests/test_gpu_builder.py::test_failed_build_leaves_no_graph): the handle must come out of the failed cos_index_build_meta without
    the component (filtered search -> NotReady), not half-linked, and a build on repaired vectors succeeds"""
    import cosdata_amd as ca
    sc = MH.Scenario(n=400, dim=32, seed=31)
    good = sc.X.copy()
    sc.X[250] = -1.0                                              # quantizes to all-zero bytes -> |v| = 0
    dix = sc.device_index()
    sc.X = good                                                   # (the queries below come from the repaired rows)
    with pytest.raises(ca.CosdataError) as ei:
        dix.build_meta(sc.node_ids, sc.mbits, sc.max_levels, 16)
    assert ei.value.status == ca._lib.ERR_CALCULATION
    Q, off, rows, _ = sc.queries(nq=4, seed=1)
    with pytest.raises(ca.CosdataError) as ei:
        dix.search_filtered(Q, off, rows.astype(np.int8), 5)
    assert ei.value.status == ca._lib.ERR_NOT_READY
    dix.upload_vectors(good).enable_metadata(sc.mdim, sc.replicas)
    dix.build_meta(sc.node_ids, sc.mbits, sc.max_levels, 16)
    _, _, counts = dix.search_filtered(Q, off, rows.astype(np.int8), 5)
    assert (counts > 0).any()                                     # the component answers again
