"""GPU: the filtered and the exhaustive searches on a shard set (cos_shardset_search_filtered_batch, cos_shardset_flat_search_batch,
cos_shardset_bruteforce_topk) and the walk with more than 1024 merged keys, shards on one device.  Every answer is compared bit for bit
(counts, ids, score bits) with the per-shard single-index calls merged by the checker of the merge rule
(tests/test_sharded_merge.py::_merge_numpy); the brute force also with one index holding the whole corpus, the filtered and the
walk also with the oracle's per-shard searches."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import meta_helpers as MH
from tests.test_sharded_merge import _merge_numpy

pytestmark = pytest.mark.gpu

N, DIM, NQ = 1900, 96, 9
SIZES3 = [633, 700, 567]                                  # ragged: no boundary is a multiple of 32
SIZES8 = [237, 240, 231, 250, 236, 229, 242, 235]
_cache = {}


def _world():
    if "world" not in _cache:
        X = H.clustered_corpus(N, DIM, n_centers=12, sigma=0.2, seed=17) * np.float32(0.9)
        _cache["world"] = (X, H.queries_from(X, NQ, noise=0.03, seed=5))
    return _cache["world"]


def _plain_index(X, storage=O.STORAGE_U8, res=0, id_base=0):
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType(ca.StorageKind(storage), res), id_base=id_base)
    ix.upload_vectors(np.ascontiguousarray(X))
    return ix


def _shards(sizes, storage=O.STORAGE_U8, res=0):
    """graph-less id-range shards of the common corpus (one list per sizes / storage for the whole module)"""
    key = (tuple(sizes), storage, res)
    if key not in _cache:
        X, _ = _world()
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        assert bounds[-1] == N
        _cache[key] = [_plain_index(X[bounds[s]:bounds[s + 1]], storage, res, id_base=int(bounds[s])) for s in range(len(sizes))]
    return _cache[key]


def _merged(parts, k):
    return _merge_numpy(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]).astype(np.uint32), k)


def _same(got, exp, what=""):
    assert np.array_equal(got[2], exp[2]), (what, got[2], exp[2])
    for b in range(got[0].shape[0]):
        c = int(got[2][b])
        assert np.array_equal(got[0][b, :c], exp[0][b, :c]), (what, b)
        assert np.array_equal(got[1][b, :c].view(np.uint32), exp[1][b, :c].view(np.uint32)), (what, b)


# ---- (a) brute force: the exact global top-k ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 200, 512])
def test_bruteforce_is_the_exact_global_topk(k):
    """3 x 512 = 1536 keys: the LDS merge; 3 x 200 and 3 x 10: the wave kernel"""
    from cosdata_amd.shardset import ShardSet
    X, Q = _world()
    shards = _shards(SIZES3)
    ss = ShardSet(shards)
    got = ss.bruteforce_topk(Q, k)
    parts = [s.bruteforce_topk(Q, k) + (np.full(NQ, k, np.uint32),) for s in shards]
    _same(got, _merged(parts, k), "per-shard merged")
    assert (got[2] == k).all()
    if "whole" not in _cache:
        _cache["whole"] = _plain_index(X)
    w_i, w_s = _cache["whole"].bruteforce_topk(Q, k)
    assert np.array_equal(got[0], w_i) and np.array_equal(got[1].view(np.uint32), w_s.view(np.uint32))
    assert len({int(np.searchsorted(np.cumsum(SIZES3), i, side="right")) for i in got[0].ravel()}) == 3      # every shard contributes
    ss.close()


# ---- (b) flat search ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,top_k", [(SIZES3, 10), (SIZES3, 204), (SIZES8, 204)], ids=["3x10", "3x204", "8x204"])
@pytest.mark.parametrize("storage,res", [(O.STORAGE_U8, 0), (O.STORAGE_SUBBYTE, 2)], ids=["u8", "quaternary"])
def test_flat_search_is_the_per_shard_scan_merged(storage, res, sizes, top_k):
    """3 x 204 = 612 keys take the wave kernel, 8 x 204 = 1632 the LDS merge"""
    from cosdata_amd.shardset import ShardSet
    _, Q = _world()
    shards = _shards(sizes, storage, res)
    ss = ShardSet(shards)
    got = ss.flat_search(Q, top_k)
    exp = _merged([s.flat_search(Q, top_k) for s in shards], top_k)
    _same(got, exp, (storage, len(sizes), top_k))
    assert (got[2] == top_k).all() and got[0].max() < N and got[0][:, 0].min() >= 0
    ss.close()


# ---- (c) masks over global rows, deleted rows -------------------------------------------------------------------------------------------
def test_masked_scans_cut_global_masks_at_the_shard_boundaries():
    import cosdata_amd as ca
    from cosdata_amd.shardset import ShardSet
    X, Q = _world()
    bounds = np.concatenate([[0], np.cumsum(SIZES3)])
    # shard 1 gets a graph of its own, so that rows of it can be deleted
    hp = ca.HNSWHyperParams(num_layers=3, ef_construction=32, ef_search=32)
    mid = ca.HNSWIndex(DIM, hp, id_base=int(bounds[1]))
    mid.upload_vectors(np.ascontiguousarray(X[bounds[1]:bounds[2]])).build(256)
    dele_rows = np.array([0, 5, 31, 32, 33, 100, 699], np.uint32)      # cos_index_delete takes the shard's own rows
    mid.delete(dele_rows)
    dele = (bounds[1] + dele_rows).astype(np.uint32)                   # ... which are these global ids
    assert mid.deleted_count() == dele.size
    base = _shards(SIZES3)
    shards = [base[0], mid, base[2]]
    rng = np.random.default_rng(21)
    masks = np.zeros((4, N), bool)
    masks[0] = rng.random(N) < 0.5                        # two allow-lists over the whole collection, cut inside words
    masks[1] = rng.random(N) < 0.1
    masks[2, bounds[1] + 3:bounds[1] + 420] = True        # live rows in shard 1 only (some of them deleted)
    masks[3, [2, 640, 641, 1899]] = True                  # four live rows, some in every shard: fewer than top_k
    masks[3, bounds[1] + 5] = True                        # ... and a deleted one, which must not come back
    qm = np.array([0, 1, 0, 2, 1, 3, 0, 1, 2], np.uint32)
    ss = ShardSet(shards)
    for top_k in (10, 60):
        exp = _merged([s.flat_search_masked(Q, top_k, masks[:, bounds[i]:bounds[i + 1]], qm, skip_deleted=True) for i, s in enumerate(shards)], top_k)
        got = ss.flat_search(Q, top_k, masks=masks, query_mask=qm, skip_deleted=True)
        _same(got, exp, ("flat", top_k))
        assert got[2][5] == 4 and set(got[0][5, :4].tolist()) == {2, 640, 641, 1899}
        assert ((got[0][3, :got[2][3]] >= bounds[1]) & (got[0][3, :got[2][3]] < bounds[2])).all()        # the query that lives in one shard
        for b in range(NQ):
            ids = got[0][b, :got[2][b]]
            assert masks[qm[b]][ids].all() and not np.isin(ids, dele).any()
    for k in (10, 300):
        exp = _merged([s.bruteforce_topk_masked(Q, k, masks[:, bounds[i]:bounds[i + 1]], qm, skip_deleted=True) for i, s in enumerate(shards)], k)
        got = ss.bruteforce_topk(Q, k, masks=masks, query_mask=qm, skip_deleted=True)
        _same(got, exp, ("brute", k))
        assert got[2][5] == 4
    # skip_deleted alone (no masks): every shard reads its own deleted set; a packed global mask gives the bool one's answer
    got = ss.flat_search(Q, 10, skip_deleted=True)
    _same(got, _merged([s.flat_search_masked(Q, 10, skip_deleted=True) for s in shards], 10), "deleted only")
    assert not np.isin(got[0], dele).any()
    from cosdata_amd.index import pack_row_masks
    a = ss.flat_search(Q, 10, masks=pack_row_masks(masks), query_mask=qm)
    _same(a, ss.flat_search(Q, 10, masks=masks, query_mask=qm), "packed")
    ss.close()


def _meta():
    """two shards of a metadata collection, oracle and device (once for the module)"""
    if "meta" not in _cache:
        A = MH.Scenario(n=900, dim=64, seed=4)
        Bs = MH.Scenario(n=700, dim=64, seed=9)
        oa, ob = A.oracle(), Bs.oracle()
        Q, off, rows, _ = A.queries(nq=30, seed=5)
        _cache["meta"] = (A, oa, ob, A.device(oa), Bs.device(ob, id_base=900 * MH.REPLICAS), Q, off, rows)
    return _cache["meta"]


# ---- (d) filtered search --------------------------------------------------------------------------------------------------------------------
def test_filtered_search_on_a_shard_set_of_a_metadata_collection():
    """the construction of tests/test_gpu_meta.py::test_filtered_search_on_two_shards_of_a_metadata_collection, behind one call"""
    from cosdata_amd.shardset import ShardSet
    A, oa, ob, da, db, Q, off, rows = _meta()
    base_b = 900 * MH.REPLICAS
    k = 10
    ss = ShardSet([da, db])
    got = ss.search_filtered(Q, off, rows.astype(np.int8), k)
    parts_d, parts_o = [], []
    for dix, oix, base in ((da, oa, 0), (db, ob, base_b)):
        parts_d.append(dix.search_filtered(Q, off, rows.astype(np.int8), k))
        ei, es, ec = oix.search_filtered_batch(Q, off, rows, k, threads=4)
        parts_o.append((np.where(np.arange(k)[None, :] < ec[:, None], ei + base, ei).astype(np.uint32), es, ec))
    _same(got, _merged(parts_o, k), "oracle")
    _same(got, _merged(parts_d, k), "per-shard")
    owners = {int(i) >= base_b for b in range(Q.shape[0]) for i in got[0][b, :int(got[2][b])]}
    assert owners == {False, True} and (got[2] > 0).sum() >= 15
    ss.close()


# ---- (e) refusals leave the set usable --------------------------------------------------------------------------------------------------
def test_refusals_carry_the_single_index_status_and_leave_the_set_usable():
    import cosdata_amd as ca
    from cosdata_amd.shardset import ShardSet
    X, Q = _world()
    shards = _shards(SIZES3)
    ss = ShardSet(shards)
    good = ss.flat_search(Q, 10)
    Qz = Q.copy()
    Qz[1] = -1.0                                                   # zero quantized norm: CalculationError for the call, as on one index
    with pytest.raises(ca.CosdataError) as ei:
        ss.flat_search(Qz, 10)
    assert ei.value.status == 2 and "shard 0" in str(ei.value)
    with pytest.raises(ca.CosdataError) as ei:
        shards[0].flat_search(Qz, 10)
    assert ei.value.status == 2
    for call in (ss.flat_search, ss.bruteforce_topk, ss.batch_search):      # 3 x 2731 = 8193 merged keys
        with pytest.raises(ca.CosdataError) as ei:
            call(Q, 2731)
        assert ei.value.status == 4
    with pytest.raises(ca.CosdataError) as ei:                     # the smallest shard holds 567 rows; 513 is past the operator's own limit
        ss.bruteforce_topk(Q, 513)
    assert ei.value.status == 3
    small = ShardSet([shards[0], _plain_index(X[633:933], id_base=633)])
    with pytest.raises(ca.CosdataError) as ei:                     # k above the smallest shard (300 rows), though shard 0 could serve it
        small.bruteforce_topk(Q, 301)
    assert ei.value.status == 3 and "shard 1" in str(ei.value)
    with pytest.raises(ca.CosdataError) as ei:
        shards[0].bruteforce_topk(Q, 634)
    assert ei.value.status == 3
    _same(small.bruteforce_topk(Q, 300), _merged([s.bruteforce_topk(Q, 300) + (np.full(NQ, 300, np.uint32),) for s in small.shards], 300), "small")
    small.close()
    f32 = _shards(SIZES3, O.STORAGE_F32, 0)
    sf = ShardSet(f32)
    with pytest.raises(ca.CosdataError) as ei:                     # the flat scan has no f32 form
        sf.flat_search(Q, 10)
    assert ei.value.status == 4 and "shard 0" in str(ei.value)
    with pytest.raises(ca.CosdataError) as ei:
        f32[0].flat_search(Q, 10)
    assert ei.value.status == 4
    _same(sf.bruteforce_topk(Q, 10), ss.bruteforce_topk(Q, 10), "f32 shards still serve the brute force")
    sf.close()
    # a correct call afterwards still answers, with the bits from before
    again = ss.flat_search(Q, 10)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(good, again))
    ss.close()


def test_a_plain_shard_in_a_filtered_call_is_not_ready():
    import cosdata_amd as ca
    from cosdata_amd.shardset import ShardSet
    A, _, _, da, db, Q, off, rows = _meta()
    plain = _plain_index(A.X[:300], id_base=900 * MH.REPLICAS)
    mixed = ShardSet([da, plain])
    with pytest.raises(ca.CosdataError) as ei:
        mixed.search_filtered(Q, off, rows.astype(np.int8), 5)
    assert ei.value.status == 6 and "shard 1" in str(ei.value)        # NotReady, the single-index status
    mixed.close()
    ss = ShardSet([da, db])
    Qz = Q.copy()
    Qz[:] = -1.0                                                       # every query zero-norm: whatever the walk needs first fails
    with pytest.raises(ca.CosdataError) as ei:
        ss.search_filtered(Qz, off, rows.astype(np.int8), 5)
    rc = da.search_filtered(Qz, off, rows.astype(np.int8), 5, return_status=True)[3]
    assert ei.value.status == rc == 2
    got = ss.search_filtered(Q, off, rows.astype(np.int8), 5)          # ... and the set still answers
    _same(got, _merged([d.search_filtered(Q, off, rows.astype(np.int8), 5) for d in (da, db)], 5), "after refusals")
    ss.close()


# ---- (f) the walk with more than 1024 merged keys ---------------------------------------------------------------------------------------
def test_walk_on_eight_shards_with_1600_merged_keys_matches_oracle():
    """cos_shardset_search_batch at 8 x 200 keys, refused before the wide merge; built as
    tests/test_gpu_shardset.py::test_shardset_eight_shards_one_device_match_oracle builds its set, on a smaller corpus"""
    from cosdata_amd.shardset import ShardSet
    dim, sizes = 64, [260, 250, 270, 240, 255, 265, 245, 258]
    X = H.clustered_corpus(sum(sizes), dim, n_centers=20, sigma=0.03, seed=88)
    hp = dict(num_layers=3, ef_construction=40, ef_search=48)
    shards, oracles, base = [], [], 0
    for s, n_s in enumerate(sizes):
        Xs = np.ascontiguousarray(X[base:base + n_s])
        oix = H.oracle_index(Xs, O.STORAGE_U8, 0, seed=11 + s, **hp)
        shards.append(H.device_index_from_oracle(oix, Xs, id_base=base))
        oracles.append((base, oix))
        base += n_s
    ss = ShardSet(shards)
    B, k = 12, 200
    Q = H.queries_from(X, B, noise=0.004, seed=100 + B)
    got = ss.batch_search(Q, k)
    parts = []
    for b0, oix in oracles:
        oi, osc, oc = oix.search_batch(Q, k, threads=4)[:3]
        parts.append((np.where(np.arange(k)[None, :] < oc[:, None], oi + b0, oi).astype(np.uint32), osc, oc))
    _same(got, _merged(parts, k), "walk")
    assert (got[2] > 0).all()
    ss.close()
