"""Embeddings appended to a collection with a metadata schema on the device: cos_index_append (the base graph continues, ids = row x
max_replicas, the resident component follows the vector table) and cos_index_append_meta (the new replica nodes join the component by
the schedule of cos_index_build_meta continued).  Held to the oracle: the base graph to build_rounds + append, the component to ONE
meta_build_rounds over the whole node table — tests/meta_append.py cuts the table and asserts that every cut is admissible."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import meta_append as MA
from tests import meta_helpers as MH
from tests.test_gpu_meta import _assert_same_filtered
from tests.test_gpu_parity import _assert_same_search, _assert_same_walk

pytestmark = pytest.mark.gpu


def _filtered_answers(sc, dix, nq=12):
    Q, off, rows, _ = sc.queries(nq=nq, seed=5)
    return dix.search_filtered(Q, off, rows.astype(np.int8), 10)


def _found(ids, counts):
    """the ids a search returned (entries past a query's count are unspecified)"""
    return np.concatenate([ids[b, :int(c)] for b, c in enumerate(counts)])


def _assert_answers_unchanged(before, after):
    (bi, bs, bc), (ai, as_, ac) = before, after
    assert np.array_equal(bc, ac)
    assert np.array_equal(_found(bi, bc), _found(ai, ac)) and np.array_equal(_found(bs, bc).view(np.uint32), _found(as_, ac).view(np.uint32))


def test_append_is_accepted_on_a_device_built_metadata_collection():
    """refused with COS_ERR_UNIMPLEMENTED (status 4) before cos_index_append carried the component"""
    sc = MH.Scenario(n=MA.N, dim=32, seed=20)
    dix = MA.device_base(sc,302, 8)
    dix.append(sc.X[302:310], 8)
    assert dix.n == 310
    ids, _, counts = dix.batch_search(sc.X[302:310], 3)
    assert (counts == 3).all() and (ids % sc.replicas == 0).all()
    assert (ids[:, 0] == np.arange(302, 310) * sc.replicas).all()     # every new embedding finds itself, under its Base id


@pytest.mark.parametrize("n0,b", [(305, 8), (417, 16)])
def test_base_graph_continues_like_the_oracle_s(n0, b):
    """build(b) on X[:n0] + append(X[n0:], b) == the oracle's build_rounds(b) + append on every level, for a cut on a boundary of the base
    schedule and for one that is not (the oracle continues from wherever the earlier build ended)"""
    sc = MH.Scenario(n=MA.N, dim=48, seed=27)
    assert (n0 in MA.boundaries(MA.N, b)) == (n0 == 305)
    sp = MA.Split(sc, (n0, MA.N), 1)
    oix = sp.oracle_base(b)
    dix = MA.device_base(sc,n0, b)
    dix.append(sc.X[n0:], b)
    MA.assert_same_levels(dix.download_graph(), oix.export_graph())
    Q, *_ = sc.queries(nq=16, seed=2)
    ids, _, counts = dix.batch_search(Q, 10)
    ids = _found(ids, counts)
    assert ids.size and (ids % sc.replicas == 0).all() and (ids // sc.replicas >= n0).any()


def test_between_the_two_calls_the_component_answers_over_the_old_replicas():
    sc, sp, batch, base_batch = MA.case("default-b8")
    dix = sp.device_old(base_batch)
    before = dix.download_meta_graph()
    dix.append(sc.X[sp.cuts[0]:], base_batch)
    # slot for slot what it was: only the pseudo nodes' vector row was renumbered, which the id form does not show
    MA.assert_same_levels(dix.download_meta_graph(), before, "after append: ")
    oix = sp.oracle_base(base_batch)
    oix.meta_set_nodes(*sp.table(sp.old)[:2]).meta_build_rounds(sp.table(sp.old)[2], sp.batch)
    MA.assert_same_levels(before, oix.meta_export_graph(), "old table: ")
    Q, off, rows, _ = sc.queries(nq=24, seed=5)
    gi, gc = _assert_same_filtered(sc, oix, dix, Q, off, rows, 10)
    assert (gc > 0).sum() >= 12 and (_found(gi, gc) // sc.replicas < sp.cuts[0]).all()


@pytest.mark.parametrize("name", ["default-b8", "default-b0", "schemaD-b8", "schemaC-q2-b48", "schemaA-f16-b1"])
def test_appended_component_equals_one_oracle_build_over_the_whole_table(name):
    """build_meta(old table) + append + append_meta(new nodes) == ONE meta_build_rounds over the whole table, row for row on every level;
    filtered search and its per-level lists equal the oracle's"""
    sc, sp, batch, base_batch = MA.case(name)
    dix = sp.device_old(base_batch)
    sp.device_step(dix, 0, base_batch, batch)
    oix = sp.oracle_whole(base_batch)
    MA.assert_same_levels(dix.download_meta_graph(), oix.meta_export_graph())
    Q, off, rows, _ = sc.queries(nq=24, seed=5)
    gi, gc = _assert_same_filtered(sc, oix, dix, Q, off, rows, 10)
    assert (_found(gi, gc) // sc.replicas >= sp.cuts[0]).any()         # the appended replicas are found


def test_two_appends_in_a_row_and_unfiltered_search_afterwards():
    sc, sp, batch, base_batch = MA.case("default-b8-twice")
    assert [int(m.sum()) for m in sp.steps] == [24, 870]
    assert any((sp.table(m)[2] > 0).any() for m in sp.steps)           # a new node above level 0: its child link is exercised
    dix = sp.device_old(base_batch)
    sp.device_step(dix, 0, base_batch)
    sp.device_step(dix, 1, base_batch)
    oix = sp.oracle_whole(base_batch)
    MA.assert_same_levels(dix.download_meta_graph(), oix.meta_export_graph())
    MA.assert_same_levels(dix.download_graph(), oix.export_graph(), "base graph: ")
    Q, off, rows, _ = sc.queries(nq=24, seed=5)
    _assert_same_filtered(sc, oix, dix, Q, off, rows, 10)
    _assert_same_walk(oix, dix, Q)                                     # the Base replicas: batch_search and ann_search on the grown collection
    _assert_same_search(oix, dix, Q, 10)


def test_new_rows_with_all_zero_metadata_are_in_the_table_and_on_no_level():
    """Metadata::from: a row whose dimensions are all zero is a Base replica — recorded, inserted nowhere, as in the build"""
    sc = MH.Scenario(n=MA.N, dim=32, seed=28)
    n0 = 417
    mb = sc.mbits.copy()
    zero = [int(np.searchsorted(sc.node_ids, sc.replicas * 450 + 2)), int(np.searchsorted(sc.node_ids, sc.replicas * 599 + 3))]
    mb[zero] = 0
    sp = MA.Split(sc, (n0, MA.N), 1, mbits=mb)                         # batches of one: every cut is admissible
    dix = sp.device_old(64)
    sp.device_step(dix, 0, 64)
    oix = sp.oracle_whole(64)
    got = dix.download_meta_graph()
    MA.assert_same_levels(got, oix.meta_export_graph())
    assert not np.isin(sc.node_ids[zero], got[0][0]).any() and got[0][0].size == sc.node_ids.size - 2
    import cosdata_amd as ca
    with pytest.raises(ca.CosdataError) as ei:                         # the last row IS in the table: nothing may be appended at or below it
        dix.append_meta(sc.node_ids[zero[1]:zero[1] + 1], mb[zero[1]:zero[1] + 1], [0], 1)
    assert ei.value.status == 3


def test_append_meta_contract():
    import cosdata_amd as ca
    sc, sp, batch, base_batch = MA.case("default-b8")
    ids, mb, ml = sp.table(sp.steps[0])
    dix = sp.device_old(base_batch)
    before = _filtered_answers(sc, dix)

    def refused(status, ids_, mb_, ml_):
        with pytest.raises(ca.CosdataError) as ei:
            dix.append_meta(ids_, mb_, ml_, batch)
        assert ei.value.status == status, str(ei.value)
        _assert_answers_unchanged(before, _filtered_answers(sc, dix))  # unchanged and searchable

    refused(3, ids, mb, ml)                                            # id / id_stride >= n: cos_index_append comes first
    dix.append(sc.X[sp.cuts[0]:], base_batch)
    before = _filtered_answers(sc, dix)
    swapped = ids.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    refused(3, swapped, mb, ml)                                        # not strictly ascending
    refused(3, np.append(ids[:5], MH.PSEUDO_ROOT + 1).astype(np.uint32), mb[:6], ml[:6])   # an id in the pseudo range
    old_ids = sp.table(sp.old)[0]
    refused(3, np.append(old_ids[old_ids < MH.PSEUDO_ROOT][-1:], ids).astype(np.uint32), np.vstack([mb[:1], mb]), np.append(ml[:1], ml))   # not above every resident replica
    refused(3, np.append(ids, sc.replicas * MA.N + 1).astype(np.uint32), np.vstack([mb, mb[:1]]), np.append(ml, 0))   # no resident vector
    high = ml.copy()
    high[7] = sc.params.num_layers + 1
    refused(3, ids, mb, high)                                          # a level above num_layers
    dix.set_visited_mode(ca.VISITED_EXACT)
    with pytest.raises(ca.CosdataError) as ei:
        dix.append_meta(ids, mb, ml, batch)
    assert ei.value.status == 3
    dix.set_visited_mode(ca.VISITED_REF)
    _assert_answers_unchanged(before, _filtered_answers(sc, dix))
    with pytest.raises(ca.CosdataError) as ei:                         # delete stays refused on a metadata collection
        dix.delete([4])
    assert ei.value.status == 4
    dix.release_link_state()                                           # ... frees the component's link state too
    with pytest.raises(ca.CosdataError) as ei:
        dix.append_meta(ids, mb, ml, batch)
    assert ei.value.status == 6
    with pytest.raises(ca.CosdataError) as ei:
        dix.append(sc.X[:4], base_batch)
    assert ei.value.status == 6
    _assert_answers_unchanged(before, _filtered_answers(sc, dix))
    # an UPLOADED component has no link state either
    oix = sc.oracle()
    up = sc.device(oix)
    with pytest.raises(ca.CosdataError) as ei:
        up.append_meta(ids, mb, ml, batch)
    assert ei.value.status == 6
