"""Filtered search on the device vs the oracle beyond the one scenario of tests/test_gpu_meta.py (5 metadata dims, 4 replicas per
embedding, cosine, default shortlist): other schemas (9, 16, 1 and 64 dims; replica strides 5, 6, 2 and 7), the binary / octal /
two-chunk u8 instances of walk_meta_kernel, the dot-product metric, a shortlist shorter than a node's slots, ef_search at the pool
widths' boundaries and below the lookahead window, the component builder on those schemas, two shards, and the error contract.
Every case is the device against the oracle, list for list and bit for bit (_assert_same_filtered); the guards computed from the
ORACLE's output keep a case from passing because nothing happened: queries do find replicas, levels do fall back to the entry
node, and the keep-100 cut does cut."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import meta_helpers as MH
from tests.test_gpu_meta import _assert_same_filtered

pytestmark = pytest.mark.gpu

NQ, TOP_K = 24, 10


def _oracle_lists(oix, Q, off, rows):
    """per query: the per-level lists [(ids, sims), ...], top level first"""
    out = []
    for b in range(Q.shape[0]):
        ids, sims, lc = oix.ann_search_filtered(Q[b], rows[off[b]:off[b + 1]])
        e = np.concatenate([[0], np.cumsum(lc)]).astype(int)
        out.append([(ids[e[i]:e[i + 1]], sims[e[i]:e[i + 1]]) for i in range(lc.size)])
    return out


def _fallback_levels(lists):
    """level lists that are the empty-list fallback: the entry node alone, with similarity exactly -1.0"""
    return sum(1 for q in lists for ids, sims in q if ids.size == 1 and sims[0] == -1.0)


def _nonempty(oix, Q, off, rows, top_k=TOP_K):
    return int((oix.search_filtered_batch(Q, off, rows, top_k, threads=4)[2] > 0).sum())


def _cut_queries(lists, off):
    """queries with two or more filters one of whose level lists is exactly 100 long (the keep-100 cut over several walks)"""
    return sum(1 for b, q in enumerate(lists) if off[b + 1] - off[b] >= 2 and any(ids.size == 100 for ids, _ in q))


def _cosine_guards(oix, Q, off, rows):
    assert _nonempty(oix, Q, off, rows) * 2 >= Q.shape[0]
    assert _fallback_levels(_oracle_lists(oix, Q, off, rows)) >= 1


def _case(schema, n=900, dim=64, seed=4, storage=O.STORAGE_U8, res=0, **kw):
    sc = MH.Scenario(n=n, dim=dim, seed=seed, storage=storage, res=res, **MH.SCHEMAS[schema], **kw)
    return sc, sc.oracle()


@pytest.mark.parametrize("schema,n,storage,res,dim", [
    ("A", 900, O.STORAGE_U8, 0, 64), ("B", 900, O.STORAGE_U8, 0, 64), ("C", 600, O.STORAGE_U8, 0, 64), ("D", 600, O.STORAGE_U8, 0, 64),
    ("A", 900, O.STORAGE_F32, 0, 96), ("A", 900, O.STORAGE_F16, 0, 72),
    # walk_meta_kernel<ENG_Q1>, <ENG_Q3>, <ENG_U8, CH = 2> (1025 .. 2048 dims) and the last dimension that instance takes
    ("A", 900, O.STORAGE_SUBBYTE, 1, 256), ("A", 900, O.STORAGE_SUBBYTE, 3, 96), ("A", 600, O.STORAGE_U8, 0, 1536), ("A", 300, O.STORAGE_U8, 0, 2048),
])
def test_schemas_and_engines_match_oracle(schema, n, storage, res, dim):
    sc, oix = _case(schema, n=n, dim=dim, storage=storage, res=res)
    dix = sc.device(oix)
    Q, off, rows, _ = sc.queries(nq=NQ, seed=7)
    _cosine_guards(oix, Q, off, rows)
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


def test_dot_product_metric_has_no_f32_arm_on_a_metadata_collection_either():
    """DotProductDistance::calculate has no FullPrecisionFP arm (dotproduct.rs:20-64): the oracle cannot even build the base graph of
    schema A in f32 and the device refuses the handle, both with StorageMismatch — the float engine's dot-product walk is the f16 case
    below"""
    import cosdata_amd as ca
    sc = MH.Scenario(n=900, dim=64, seed=4, storage=O.STORAGE_F32, metric=O.METRIC_DOT, **MH.SCHEMAS["A"])
    with pytest.raises(ValueError, match=f"status {O.ERR_STORAGE_MISMATCH}"):
        sc.oracle()
    with pytest.raises(ca.CosdataError) as ei:
        sc.device_index()
    assert ei.value.status == O.ERR_STORAGE_MISMATCH


@pytest.mark.parametrize("storage,dim", [(O.STORAGE_U8, 64), (O.STORAGE_F16, 64)])
def test_dot_product_metric_ignores_the_node_kinds(storage, dim):
    """metric != cosine: the vector distance decides for every node, pseudo nodes included, and nothing is dropped for being -1.0"""
    sc, oix = _case("A", dim=dim, storage=storage, metric=O.METRIC_DOT)
    dix = sc.device(oix)
    Q, off, rows, _ = sc.queries(nq=NQ, seed=7)
    assert (oix.search_filtered_batch(Q, off, rows, TOP_K, threads=4)[2] == TOP_K).all()
    assert _fallback_levels(_oracle_lists(oix, Q, off, rows)) == 0
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


@pytest.mark.parametrize("shortlist,seed", [(20, 4), (8, 4), (1, 7)])
def test_shortlist_shorter_than_the_neighbour_slots(shortlist, seed):
    """slots = min(M, shortlist_size) < M on every level (M = 32, 64): the scan stops at the shortlist, lanes beyond it read slot
    slots - 1 of the lookahead rows and drop it.  With a shortlist of 1 the builder's own walks scan one slot per node as well, the
    component is a bundle of chains and no seed lets half of the queries find a replica (the oracle gives 0 .. 4 of 24 over seeds
    0 .. 7): what that case has to show instead is that walks leave the entry node and that some query still ends on a replica."""
    sc, oix = _case("A", shortlist_size=shortlist, seed=seed)
    dix = sc.device(oix)
    Q, off, rows, _ = sc.queries(nq=NQ, seed=7)
    if shortlist > 1:
        _cosine_guards(oix, Q, off, rows)
    else:
        lists = _oracle_lists(oix, Q, off, rows)
        assert _fallback_levels(lists) >= 1 and any(ids.size >= 2 for q in lists for ids, _ in q) and _nonempty(oix, Q, off, rows) >= 1
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


EF_EDGES = [1, 2, 3, 4, 5, 65, 256, 257, 512, 513, 1024]     # below / at the lookahead window of 4; R = 1|4, 4|8, 8|16 and the last ef


@pytest.fixture(scope="module")
def edge_world():
    sc, oix = _case("A")
    return sc, oix, sc.device(oix), sc.queries(nq=12, seed=7)


@pytest.mark.parametrize("ef", EF_EDGES)
def test_ef_search_at_the_pool_width_boundaries(edge_world, ef):
    sc, oix, dix, (Q, off, rows, _) = edge_world
    oix.set_ef_search(ef)
    dix.set_ef_search(ef)
    lists = _oracle_lists(oix, Q, off, rows)
    if ef >= 64:
        assert _nonempty(oix, Q, off, rows) * 2 >= Q.shape[0] and _fallback_levels(lists) >= 1
    if ef >= 256:
        assert _cut_queries(lists, off) >= 1
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


def test_ef_search_beyond_the_walk_is_refused_and_the_handle_survives(edge_world):
    import cosdata_amd as ca
    sc, oix, dix, (Q, off, rows, _) = edge_world
    dix.set_ef_search(1025)
    with pytest.raises(ca.CosdataError) as ei:
        dix.search_filtered(Q, off, rows.astype(np.int8), TOP_K)
    assert ei.value.status == O.ERR_UNIMPLEMENTED
    oix.set_ef_search(64)
    dix.set_ef_search(64)
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


@pytest.mark.parametrize("schema,storage,res,dim,bs", [("A", O.STORAGE_U8, 0, 64, 1), ("A", O.STORAGE_U8, 0, 64, 256), ("D", O.STORAGE_U8, 0, 64, 48),
                                                       ("B", O.STORAGE_SUBBYTE, 2, 128, 128)])
def test_component_builder_on_other_schemas_equals_the_oracle_rounds_builder(schema, storage, res, dim, bs):
    """cos_index_build_meta == coso_meta_build_rounds slot for slot on every level: at index time the pseudo x pseudo cosine (its bits
    order the pseudo nodes' neighbours) and the Metadata x Metadata > 0.99 decision run the 8-chain metadata dot at 9, 16 and 64 dims"""
    sc = MH.Scenario(n=600 if schema == "D" else 900, dim=dim, seed=11, storage=storage, res=res, **MH.SCHEMAS[schema])
    oix = O.OracleIndex(sc.params).set_vectors(sc.X)
    oix.meta_enable(sc.mdim, sc.replicas)
    oix.build()
    oix.meta_set_nodes(sc.node_ids, sc.mbits).meta_build_rounds(sc.max_levels, bs)
    dix = sc.device_index()
    dix.upload_graph(oix.export_graph(), oix.root_raw())
    dix.build_meta(sc.node_ids, sc.mbits, sc.max_levels, bs)
    for l, ((gi, gn), (ei, en)) in enumerate(zip(dix.download_meta_graph(), oix.meta_export_graph())):
        assert np.array_equal(gi, ei), f"level {l}: node sets differ"
        assert np.array_equal(gn, en), f"level {l}: adjacency differs in {np.count_nonzero((gn != en).any(axis=1))} of {len(en)} rows"
    Q, off, rows, _ = sc.queries(nq=NQ, seed=5)
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)


def test_two_shards_with_a_replica_stride_of_five():
    """shard s returns id_base + row x 5 + i with id_base = first embedding x 5; merged like test_filtered_search_on_two_shards_of_a_
    metadata_collection"""
    import cosdata_amd as ca
    from tests.test_sharded_merge import _merge_numpy
    A, oa = _case("A", n=500, seed=4)
    Bs, ob = _case("A", n=400, seed=9)
    base_b = 500 * A.replicas
    da, db = A.device(oa), Bs.device(ob, id_base=base_b)
    Q, off, rows, _ = A.queries(nq=NQ, seed=5)
    parts_d, parts_o = [], []
    for dix, oix, base in ((da, oa, 0), (db, ob, base_b)):
        gi, gs, gc = dix.search_filtered(Q, off, rows.astype(np.int8), TOP_K)
        ei, es, ec = oix.search_filtered_batch(Q, off, rows, TOP_K, threads=4)
        assert np.array_equal(gc, ec) and (ec > 0).sum() * 2 >= NQ
        for b in range(NQ):
            c = int(gc[b])
            assert np.array_equal(gi[b, :c], ei[b, :c] + base) and np.array_equal(gs[b, :c].view(np.uint32), es[b, :c].view(np.uint32)), f"shard base {base}, query {b}"
        parts_d.append((gi, gs, gc))
        parts_o.append((np.where(np.arange(TOP_K)[None, :] < ec[:, None], ei + base, ei).astype(np.uint32), es, ec))
    md = _merge_numpy(*[np.stack([p[i] for p in parts_d]) for i in range(3)], TOP_K)
    mo = _merge_numpy(*[np.stack([p[i] for p in parts_o]) for i in range(3)], TOP_K)
    assert np.array_equal(md[2], mo[2])
    for b in range(NQ):
        c = int(md[2][b])
        assert np.array_equal(md[0][b, :c], mo[0][b, :c]) and np.array_equal(md[1][b, :c].view(np.uint32), mo[1][b, :c].view(np.uint32))
    owners = {int(i) >= base_b for b in range(NQ) for i in md[0][b, :int(md[2][b])]}
    assert owners == {False, True}                               # both shards contribute to merged answers
    with pytest.raises(ca.CosdataError) as ei:                   # 3 replicas into an embedding: not a whole number of embeddings
        Bs.device(ob, id_base=base_b + 3)
    assert ei.value.status == O.ERR_INVALID


@pytest.fixture(scope="module")
def contract_world():
    sc, oix = _case("A")
    return sc, oix, sc.device(oix), sc.queries(nq=6, seed=7)


def test_an_all_zero_filter_row_is_the_oracles_unimplemented(contract_world):
    """a filter without any dimension is a Base-kind query under the pseudo root: one of the reference's unreachable!() arms"""
    sc, oix, dix, (Q, off, rows, _) = contract_world
    bad = rows.copy()
    bad[off[2]] = 0
    g = dix.search_filtered(Q, off, bad.astype(np.int8), TOP_K, return_status=True)
    e = oix.search_filtered_batch(Q, off, bad, TOP_K, threads=2, raise_on_error=False)
    assert e[3] == O.ERR_UNIMPLEMENTED and e[4].tolist() == [0, 0, O.ERR_UNIMPLEMENTED, 0, 0, 0]
    assert g[3] == e[3] and np.array_equal(g[4], e[4])
    _assert_same_filtered(sc, oix, dix, Q, off, rows, TOP_K)     # the next call on the handle


def test_a_value_no_node_has_finds_nothing(contract_world):
    sc, oix, dix, (Q, off, rows, _) = contract_world
    assert sc.fields[0] == (6, 3)                                # value 7 fits the field's 3 digits and is beyond its cardinality
    f = np.zeros((1, sc.mdim), np.int32)
    f[0, :3] = MH.bits(7, 3)
    o1 = np.array([0, 1], np.uint32)
    e = oix.search_filtered_batch(Q[:1], o1, f, TOP_K, raise_on_error=False)
    g = dix.search_filtered(Q[:1], o1, f.astype(np.int8), TOP_K, return_status=True)
    assert e[3] == O.OK and e[2][0] == 0 and e[4][0] == O.OK
    assert g[3] == O.OK and g[2][0] == 0 and g[4][0] == O.OK
    _assert_same_filtered(sc, oix, dix, Q[:1], o1, f, TOP_K)


def test_six_or_filters_are_cut_to_the_best_hundred(contract_world):
    sc, oix, dix, (Q, off, rows, _) = contract_world
    f = np.array([sc.dims({0: v}) for v in range(1, 7)], np.int32)   # field 0 is any of its six values
    o1 = np.array([0, 6], np.uint32)
    oix.set_ef_search(200)
    dix.set_ef_search(200)
    try:
        lists = _oracle_lists(oix, Q[:1], o1, f)
        assert lists[0][-1][0].size == 100                       # level 0: 6 walks x up to 100 survivors, the best 100 kept
        _assert_same_filtered(sc, oix, dix, Q[:1], o1, f, TOP_K)
        # a matching pseudo node leads the list at cosine 1.0 and is dropped from the results: the 5k candidates of the rerank
        # are the 5k replicas behind it, however short 5k is
        assert lists[0][-1][0][0] >= MH.PSEUDO_ROOT
        for k in (1, 2):
            _assert_same_filtered(sc, oix, dix, Q[:1], o1, f, k)
            assert oix.search_filtered_batch(Q[:1], o1, f, k)[2][0] == k
    finally:
        oix.set_ef_search(64)
        dix.set_ef_search(64)


def test_metadata_dimensions_outside_1_to_64_are_refused(contract_world):
    import cosdata_amd as ca
    sc = contract_world[0]
    dix = ca.HNSWIndex(sc.dim, ca.HNSWHyperParams(num_layers=2))
    dix.upload_vectors(sc.X[:50])
    for mdim in (65, 0):
        with pytest.raises(ca.CosdataError) as ei:
            dix.enable_metadata(mdim, 4)
        assert ei.value.status == O.ERR_INVALID
