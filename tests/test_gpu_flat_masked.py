"""GPU: the exhaustive scans over a subset of the rows — cos_flat_search_masked_batch, cos_bruteforce_topk_masked, the handle's deleted
set.  Every assertion is bit-exact (counts, ids, score bits) against the oracle ON THE SUBSET (tests/flat_masked.py): the oracle's own
scan over the live rows with the ids mapped back.  The mask test sits where the kernels keep a candidate, so every kernel family is run:
the query-resident kernels (default), the 256 x 128 tile kernel (flat_tile_kernel = 1), the score-matrix path (flat_unfused = 1) and the i8
digits (flat_fp4 = 0)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_masked as FM
from tests import helpers as H
from tests.flat_masked import KEEPS, N, TOP_K, same
from tests.test_gpu_append import _device

pytestmark = pytest.mark.gpu

KNOBS = (dict(flat_tile_kernel=1), dict(flat_unfused=1), dict(flat_fp4=0))
STORAGE_IDS = list(FM.STORAGES)
_indexes = {}


def _index(storage, dim=FM.DIM, metric=None, X=None, cache=True):
    """a device index over the common corpus (one per storage, dim and metric for the whole module) or over `X`"""
    import cosdata_amd as ca
    key = (storage, dim, int(metric or 0))
    if X is None and cache and key in _indexes:
        return _indexes[key]
    kind, res = FM.STORAGES[storage]
    ix = ca.HNSWIndex(dim, ca.HNSWHyperParams(num_layers=3), distance_metric=metric or ca.DistanceMetric.Cosine,
                      storage_type=ca.StorageType(ca.StorageKind(kind), res))
    ix.upload_vectors(FM.world(dim)[0] if X is None else X)
    if X is None and cache:
        _indexes[key] = ix
    return ix


def _all(n=N):
    return np.ones(n, bool)


# ---- 1. storages x kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("storage", STORAGE_IDS)
def test_shared_mask_every_storage_and_kernel(storage, keep):
    from cosdata_amd import _lib
    X, Q = FM.world()
    live = FM.keep_mask(keep)
    full = FM.subset_flat(X, Q, storage, _all(), TOP_K, key="all")
    hit = FM.mask_matters(full[0], live)                              # from the oracle alone: the mask changes the answer
    assert hit == FM.NQ if keep != 0.9 else hit * 3 >= FM.NQ, hit
    ref = FM.subset_flat(X, Q, storage, live, TOP_K, key=keep)
    ix = _index(storage)
    same(ix.flat_search_masked(Q, TOP_K, live), ref, what="default")
    for knob in KNOBS:
        with _lib.tuning(**knob):
            same(ix.flat_search_masked(Q, TOP_K, live), ref, what=knob)


def test_u8_rows_that_are_no_64_byte_chunks():
    """72 dims: the u8 rows have no query-resident instantiation, the fused chunk runs on the tile kernel by default"""
    from cosdata_amd import _lib
    X, Q = FM.world(72)
    ix = _index("u8", 72)
    for keep in KEEPS:
        live = FM.keep_mask(keep)
        ref = FM.subset_flat(X, Q, "u8", live, TOP_K, key=("d72", keep))
        same(ix.flat_search_masked(Q, TOP_K, live), ref, what=keep)
        with _lib.tuning(flat_unfused=1):
            same(ix.flat_search_masked(Q, TOP_K, live), ref, what=(keep, "unfused"))


# ---- 2. per-query masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGE_IDS)
def test_per_query_masks(storage):
    """four masks, query b under mask b % 4: the tile kernel's 256-row blocks and the query-resident kernels' 64-row waves mix them"""
    from cosdata_amd import _lib
    X, Q = FM.world(nq=261)
    masks = FM.four_masks()
    refs = [FM.subset_flat(X, Q, storage, masks[g], TOP_K, key=("q261", g)) for g in range(4)]
    qm = np.arange(261, dtype=np.uint32) % 4
    ref = tuple(np.stack([refs[qm[b]][a][b] for b in range(261)]) for a in range(3))
    ix = _index(storage)
    for B in (5, 70, 261):
        got = ix.flat_search_masked(Q[:B], TOP_K, masks, qm[:B])
        same(got, ref, what=B)
        plain = ix.flat_search(Q[:B], TOP_K)
        ones = np.flatnonzero(qm[:B] == 3)                            # the all-ones queries: the unmasked call's bits
        assert all(np.array_equal(np.asarray(g)[ones].view(np.uint32), np.asarray(p)[ones].view(np.uint32)) for g, p in zip(got, plain))
        with _lib.tuning(flat_tile_kernel=1):
            same(ix.flat_search_masked(Q[:B], TOP_K, masks, qm[:B]), ref, what=(B, "tile"))
    with _lib.tuning(flat_unfused=1):
        same(ix.flat_search_masked(Q, TOP_K, masks, qm), ref, what="unfused")


# ---- 3. pool widths and short lists ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [13, 204])
@pytest.mark.parametrize("storage", ["u8", "quaternary"])
def test_wide_pools_with_fewer_live_rows_than_candidates(storage, top_k):
    """P = 128 and P = 1024 at keep 0.02: ~400 live rows, fewer than the 1020 rerank candidates of top_k 204 — the pool never fills and
    its threshold stays 0 through the fused chunk"""
    from cosdata_amd import _lib
    X, Q = FM.world()
    live = FM.keep_mask(0.02)
    assert 204 < np.count_nonzero(live) < 1020
    ref = FM.subset_flat(X, Q, storage, live, top_k, key=0.02)
    ix = _index(storage)
    same(ix.flat_search_masked(Q, top_k, live), ref)
    for knob in (dict(flat_tile_kernel=1), dict(flat_unfused=1)):
        with _lib.tuning(**knob):
            same(ix.flat_search_masked(Q, top_k, live), ref, what=knob)


@pytest.mark.parametrize("storage", ["u8", "binary"])
def test_short_lists_and_padding_bits(storage):
    """7 live rows -> counts 7; none -> counts 0; the bits at and past n in the last word are set and must be ignored"""
    from cosdata_amd.index import pack_row_masks
    X, Q = FM.world()
    seven = np.zeros(N, bool)
    seven[[3, 999, 16383, 16384, 16385, 19000, N - 1]] = True
    masks = np.stack([seven, np.zeros(N, bool), FM.keep_mask(0.5)])
    bits = pack_row_masks(masks)
    assert N % 32 != 0
    bits[:, -1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)  # rows N .. 32 * words - 1 do not exist
    qm = np.arange(FM.NQ, dtype=np.uint32) % 3
    refs = [FM.subset_flat(X, Q, storage, masks[g], TOP_K, key=("short", g) if g < 2 else 0.5) for g in range(3)]
    ref = tuple(np.stack([refs[qm[b]][a][b] for b in range(FM.NQ)]) for a in range(3))
    assert set(ref[2]) == {7, 0, TOP_K}
    got = _index(storage).flat_search_masked(Q, TOP_K, bits, qm)
    same(got, ref)
    assert sorted(got[0][0][:7]) == sorted(np.flatnonzero(seven))


# ---- 4. dot-product metric -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["binary", "u8"])
def test_dot_product_metric(storage):
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X, Q = FM.world()
    live = FM.keep_mask(0.5)
    ref = FM.subset_flat(X, Q, storage, live, TOP_K, metric=O.METRIC_DOT, key=0.5)
    ix = _index(storage, metric=ca.DistanceMetric.DotProduct)
    same(ix.flat_search_masked(Q, TOP_K, live), ref)
    for knob in KNOBS:
        with _lib.tuning(**knob):
            same(ix.flat_search_masked(Q, TOP_K, live), ref, what=knob)


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["u8", "quaternary"])
def test_ties_keep_the_oracles_order(storage):
    """row 100 copied into rows 5000, 15000 and 19000 (both sides of the seed chunk's end): equal scores, larger id first, among the
    copies a mask keeps"""
    from cosdata_amd import _lib
    X = FM.world()[0].copy()
    copies = [100, 5000, 15000, 19000]
    X[copies[1:]] = X[100]
    Q = np.ascontiguousarray(np.concatenate([X[100][None, :] * np.float32(0.99), FM.world()[1][:19]]))
    masks = np.ones((4, N), bool)
    masks[0, [5000, 19000]] = False
    masks[1, [100]] = False
    masks[2, [15000, 19000, 100]] = False
    qm = np.arange(20, dtype=np.uint32) % 4
    qm[0] = 0
    ix = _index(storage, X=X)
    refs = [FM.subset_flat(X, Q, storage, masks[g], TOP_K) for g in range(4)]
    for shift in range(4):                                            # query 0 (the copies' own vector) under each mask in turn
        q = qm.copy()
        q[0] = shift
        ref = tuple(np.stack([refs[q[b]][a][b] for b in range(20)]) for a in range(3))
        kept = [c for c in copies if masks[shift, c]]
        assert list(ref[0][0][:len(kept)]) == sorted(kept, reverse=True), "the copies do not lead the list: the corpus is no test"
        same(ix.flat_search_masked(Q, TOP_K, masks, q), ref, what=shift)
        with _lib.tuning(flat_tile_kernel=1):
            same(ix.flat_search_masked(Q, TOP_K, masks, q), ref, what=(shift, "tile"))


# ---- 6. zero norm ----------------------------------------------------------------------------------------------------------------
def test_zero_norm_counts_only_where_a_query_can_see_it():
    """quaternary (SubByte norms are the raw vector's): row 777 is all zero.  Masked out for every query the call answers with the
    oracle's bits; live for one query it is CalculationError; the unmasked call on the handle stays CalculationError"""
    import cosdata_amd as ca
    X = FM.world()[0].copy()
    Q = FM.world()[1]
    X[777] = 0.0
    ix = _index("quaternary", X=X)
    live = FM.keep_mask(0.5).copy()
    live[777] = False
    ref = FM.subset_flat(X, Q, "quaternary", live, TOP_K)
    same(ix.flat_search_masked(Q, TOP_K, live), ref, what="masked out")
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Q, TOP_K)
    assert ei.value.status == 2
    seen = live.copy()
    seen[777] = True
    qm = np.zeros(FM.NQ, np.uint32)
    qm[41] = 1
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search_masked(Q, TOP_K, np.stack([live, seen]), qm)
    assert ei.value.status == 2
    same(ix.flat_search_masked(Q, TOP_K, np.stack([live, seen]), np.zeros(FM.NQ, np.uint32)), ref, what="mask 1 unused")   # no query names the mask that sees it
    same(ix.flat_search_masked(Q, TOP_K, live), ref, what="after the refusal")
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Q, TOP_K)
    assert ei.value.status == 2
    Qz = Q.copy()
    Qz[5] = 0.0
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search_masked(Qz, TOP_K, live)
    assert ei.value.status == 2


# ---- 7. deleted set (and 8: the brute force on the same handle) ------------------------------------------------------------------
def test_deleted_set_through_delete_append_and_upload():
    X, Q = FM.world()
    p = O.HNSWParams(dim=FM.DIM, storage=O.STORAGE_SUBBYTE, resolution=1, num_layers=3, ef_construction=32, ef_search=32, seed=11)
    dix = _device(X, p).build(1024)
    full = FM.subset_flat(X, Q, "binary", _all(), TOP_K, key="all")
    assert dix.deleted_count() == 0 and dix.deleted_rows().size == 0
    rng = np.random.default_rng(9)
    dele = np.unique(np.concatenate([full[0][:40, 0], rng.integers(0, 16384, 50), rng.integers(16384, N, 50)])).astype(np.uint32)
    dix.delete(np.concatenate([dele, dele[:1]]))                      # one id twice
    gone = np.zeros(N, bool)
    gone[dele] = True
    assert dix.deleted_count() == dele.size and np.array_equal(dix.deleted_rows(), dele)
    plain = dix.flat_search(Q, TOP_K)
    same(plain, full, what="the plain scan still sees deleted rows")
    assert gone[plain[0][:40, 0]].all()
    same(dix.flat_search_masked(Q, TOP_K, skip_deleted=True), FM.subset_flat(X, Q, "binary", ~gone, TOP_K), what="skip_deleted")
    half = FM.keep_mask(0.5)
    same(dix.flat_search_masked(Q, TOP_K, half, skip_deleted=True), FM.subset_flat(X, Q, "binary", half & ~gone, TOP_K), what="mask and skip_deleted")
    same(dix.flat_search_masked(Q, TOP_K, half), FM.subset_flat(X, Q, "binary", half, TOP_K, key=0.5), what="mask alone")
    for k in (10, 40):
        same(dix.bruteforce_topk_masked(Q, k, skip_deleted=True), FM.subset_brute(X, Q, ~gone, k), what=("brute", k))
    same(dix.flat_search(Q, TOP_K), full, what="plain after masked")
    # 500 more rows: live, the bitmap grows with the tables, the earlier deletions stay
    X2 = np.concatenate([X, H.clustered_corpus(500, FM.DIM, n_centers=10, sigma=0.25, seed=4) * np.float32(0.9)])
    dix.append(X2[N:], 1024)
    gone2 = np.concatenate([gone, np.zeros(500, bool)])
    assert dix.deleted_count() == dele.size and np.array_equal(dix.deleted_rows(), dele)
    got = dix.flat_search_masked(Q, TOP_K, skip_deleted=True)
    same(got, FM.subset_flat(X2, Q, "binary", ~gone2, TOP_K), what="after append")
    cold = _index("binary", X=X2).flat_search(Q, TOP_K)
    warm = dix.flat_search(Q, TOP_K)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(warm, cold))
    dix.delete(np.array([N + 3], np.uint32))
    assert dix.deleted_count() == dele.size + 1 and dix.deleted_rows()[-1] == N + 3
    dix.upload_vectors(X)
    assert dix.deleted_count() == 0
    same(dix.flat_search_masked(Q, TOP_K, skip_deleted=True), full, what="after a new upload")


# ---- 8. brute force --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 130])
def test_bruteforce_masked(dim):
    """130 dims: rows are not 16-byte aligned, the GEMM stages scalars.  k 10 keeps 64 survivors, k 40 a pool of 128"""
    from cosdata_amd import _lib
    X, Q = FM.world(dim, 261)
    ix = _index("u8", dim)
    masks = FM.four_masks()
    qm = np.arange(261, dtype=np.uint32) % 4
    for k in (10, 40):
        refs = [FM.subset_brute(X, Q, masks[g], k, key=(dim, g)) for g in range(4)]
        for g, keep in enumerate(KEEPS):
            same(ix.bruteforce_topk_masked(Q[:70], k, masks[g]), refs[g], what=(k, keep))
        ref = tuple(np.stack([refs[qm[b]][a][b] for b in range(261)]) for a in range(3))
        for B in (5, 261):
            got = ix.bruteforce_topk_masked(Q[:B], k, masks, qm[:B])
            same(got, ref, what=(k, B))
        with _lib.tuning(flat_unfused=1):
            same(ix.bruteforce_topk_masked(Q, k, masks, qm), ref, what=(k, "unfused"))
        few = np.zeros(N, bool)
        few[[5, 16000, 17000, 19999, N - 1, 42, 77]] = True           # fewer live rows than k
        got = ix.bruteforce_topk_masked(Q[:70], k, few)
        same(got, FM.subset_brute(X, Q[:70], few, k), what=(k, "few"))
        assert (got[2] == 7).all()
        plain = ix.bruteforce_topk(Q[:70], k)
        none = ix.bruteforce_topk_masked(Q[:70], k)                   # no mask: the unmasked call's bits, full counts
        assert np.array_equal(none[0], plain[0]) and np.array_equal(none[1].view(np.uint32), plain[1].view(np.uint32)) and (none[2] == k).all()


# ---- 9. contract -----------------------------------------------------------------------------------------------------------------
def _raw_flat(ix, Q, top_k, sm):
    from cosdata_amd import _lib
    B = Q.shape[0]
    ids, sc, cnt = np.zeros((B, top_k), np.uint32), np.zeros((B, top_k), np.float32), np.zeros(B, np.uint32)
    rc = _lib.lib().cos_flat_search_masked_batch(ix._h, Q.ctypes.data, B, top_k, C.byref(sm) if sm is not None else None, ids.ctypes.data, sc.ctypes.data,
                                                 cnt.ctypes.data, None)
    return rc, (ids, sc, cnt)


def _raw_brute(ix, Q, k, sm, counts=True):
    from cosdata_amd import _lib
    B = Q.shape[0]
    ids, sc, cnt = np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32), np.zeros(B, np.uint32)
    rc = _lib.lib().cos_bruteforce_topk_masked(ix._h, Q.ctypes.data, B, k, C.byref(sm) if sm is not None else None, ids.ctypes.data, sc.ctypes.data,
                                               cnt.ctypes.data if counts else None)
    return rc, (ids, sc, cnt)


def test_refusals_and_the_unmasked_forms():
    import cosdata_amd as ca
    from cosdata_amd import _lib
    from cosdata_amd.index import pack_row_masks
    X, Q = FM.world()
    Q = np.ascontiguousarray(Q)
    ix = _index("quaternary")
    plain = ix.flat_search(Q, TOP_K)
    bits = pack_row_masks(np.stack([FM.keep_mask(0.5), FM.keep_mask(0.9)]))
    qm = (np.arange(FM.NQ, dtype=np.uint32) % 2)
    size = C.sizeof(_lib.CosScanMask)
    bad_q = qm.copy()
    bad_q[17] = 2
    refused = {
        "struct_size": _lib.CosScanMask(size - 4, 0, 1, bits.ctypes.data, None),
        "bits NULL": _lib.CosScanMask(size, 0, 1, None, None),
        "query_mask NULL": _lib.CosScanMask(size, 0, 2, bits.ctypes.data, None),
        "index out of range": _lib.CosScanMask(size, 0, 2, bits.ctypes.data, bad_q.ctypes.data),
    }
    for what, sm in refused.items():
        assert _raw_flat(ix, Q, TOP_K, sm)[0] == _lib.ERR_INVALID, what
        assert _raw_brute(ix, Q, TOP_K, sm)[0] == _lib.ERR_INVALID, what
        rc, got = _raw_flat(ix, Q, TOP_K, None)                       # the handle answers after every refusal; NULL = the unmasked call
        assert rc == 0 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, plain)), what
    ok = _lib.CosScanMask(size, 0, 2, bits.ctypes.data, qm.ctypes.data)
    assert _raw_flat(ix, Q, 205, ok)[0] == _lib.ERR_UNIMPLEMENTED
    assert _raw_brute(ix, Q, TOP_K, ok, counts=False)[0] == _lib.ERR_INVALID          # out_counts is required
    assert _raw_brute(ix, Q, 513, ok)[0] == _lib.ERR_INVALID
    rc, got = _raw_flat(ix, Q, TOP_K, _lib.CosScanMask(size, 0, 0, None, None))       # no allow-list, no flag: the unmasked call
    assert rc == 0 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, plain))
    got = ix.flat_search_masked(Q, TOP_K)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, plain))
    rc, got = _raw_flat(ix, Q, TOP_K, ok)
    assert rc == 0
    same(got, ix.flat_search_masked(Q, TOP_K, np.stack([FM.keep_mask(0.5), FM.keep_mask(0.9)]), qm))


@pytest.mark.parametrize("kind", [O.STORAGE_F16, O.STORAGE_F32])
def test_float_storages_are_refused_by_the_code_scan_and_served_by_the_brute_force(kind):
    import cosdata_amd as ca
    X, Q = FM.world()
    ix = ca.HNSWIndex(FM.DIM, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType(ca.StorageKind(kind), 0))
    ix.upload_vectors(X)
    live = FM.keep_mask(0.5)
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search_masked(Q, TOP_K, live)
    assert ei.value.status == 4
    same(ix.bruteforce_topk_masked(Q, TOP_K, live), FM.subset_brute(X, Q, live, TOP_K, key=(FM.DIM, "half70")))
