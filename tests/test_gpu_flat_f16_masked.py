"""GPU: cos_flat_search_f16_masked_batch, the exhaustive f16 scan over each query's live rows.  The yardstick is the oracle's exhaustive
f16 finalisation on the sub-corpus of live rows with the ids mapped back (tests/flat_masked.py: the oracle on the subset): counts, ids
and score bits are compared for equality."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_masked as FM
from tests import helpers as H
from tests import near_copies as NC

pytestmark = pytest.mark.gpu
TOP_K = 5                                                # N = 25, P = 64


def _index(X, storage=O.STORAGE_F16, metric=None, built=False):
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3, ef_construction=32, ef_search=32), metric or ca.DistanceMetric.Cosine,
                      ca.StorageType(ca.StorageKind(storage), 0), seed=11).upload_vectors(X)
    return ix.build(1024) if built else ix               # delete() wants the graph


@functools.lru_cache(maxsize=None)
def _world(n, dim, B):
    X = H.clustered_corpus(n, dim, n_centers=20, seed=3)
    Q = H.queries_from(X, B, noise=0.05, seed=8)
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


def _subset(X, Q, live, top_k):
    """FM.subset_flat for f16 storage: the oracle's flat search over X[live], ids mapped back"""
    rows, B = np.flatnonzero(live).astype(np.uint32), Q.shape[0]
    out = np.full((B, top_k), 0xFFFFFFFF, np.uint32), np.zeros((B, top_k), np.float32), np.zeros(B, np.uint32)
    if rows.size:
        p = O.HNSWParams(dim=X.shape[1], storage=O.STORAGE_F16, num_layers=3)
        ids, sc, cnt = O.OracleIndex(p).set_vectors(np.ascontiguousarray(X[rows])).flat_search_batch(Q, top_k, threads=8)
        assert (cnt == min(top_k, rows.size)).all()
        out[0][:, :cnt[0]], out[1][:], out[2][:] = rows[ids[:, :cnt[0]]], sc, cnt
    return out


def _ref(X, Q, masks, qm, top_k=TOP_K):
    """query b's answer: the oracle over X[masks[qm[b]]]"""
    masks, qm = np.atleast_2d(masks), np.zeros(Q.shape[0], int) if qm is None else np.asarray(qm)
    per = {g: _subset(X, Q, masks[g], top_k) for g in np.unique(qm)}
    return tuple(np.stack([per[qm[b]][i][b] for b in range(Q.shape[0])]) for i in range(3))


def _rows(n, rows):
    m = np.zeros(n, bool)
    m[np.asarray(rows)] = True
    return m


# dim 8: only the x8 tail step | 40: x16 steps and an x8 tail | 264: past the 256-dim panel.  n 200: three tiles and a partial one;
# 16584: 200 rows past the seed chunk, which arrive through the fused epilogue.  B 130 crosses the 128-query block
SHAPES = [(8, 200, 3), (40, 200, 130), (264, 200, 3), (40, 16584, 130)]
KINDS = ["half", "three_masks", "deleted", "allow_and_deleted", "one_tile", "dead_tile", "bits_past_n"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,n,B", SHAPES)
def test_parity_with_the_oracle_on_the_live_rows(dim, n, B, kind):
    X, Q = _world(n, dim, B)
    rng = np.random.default_rng(5)
    half = rng.random(n) < 0.5
    dele = np.unique(np.concatenate([rng.integers(0, n, 9), [0, n - 1]])).astype(np.uint32)
    last = (n - 1) // 64                                  # the partial tile; the big shape's lies in the fused chunk
    masks, qm, skip, live = half, None, False, None
    if kind == "three_masks":
        masks, qm = np.stack([half, rng.random(n) < 0.1, np.ones(n, bool)]), np.arange(B) % 3
    elif kind == "deleted":
        masks, skip, live = None, True, ~_rows(n, dele)
    elif kind == "allow_and_deleted":
        skip, live = True, half & ~_rows(n, dele)
    elif kind == "one_tile":
        masks = _rows(n, np.arange(64 * (last - 1), 64 * last))
    elif kind == "dead_tile":
        masks = half & ~_rows(n, np.arange(64, 128)) & ~_rows(n, np.arange(64 * last, n))
    ref = _ref(X, Q, masks if live is None else live, qm)
    if kind == "bits_past_n":                             # packed words with every padding bit set
        from cosdata_amd.index import pack_row_masks
        masks = pack_row_masks(masks)
        masks[:, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF if n % 32 else 0)
    ix = _index(X, built=skip)
    if skip:
        ix.delete(dele)
    got = ix.flat_search_f16_masked(Q, TOP_K, masks, qm, skip_deleted=skip, with_stats=True)
    FM.same(got, ref, what=kind)
    st, blocks, tiles = got[3], (B + 127) // 128, (n + 63) // 64
    assert st.tiles_total == blocks * tiles and 0 < st.tiles_scanned <= st.tiles_total
    if kind == "one_tile":
        assert st.tiles_scanned == blocks
    if kind == "dead_tile":
        assert st.tiles_scanned == blocks * (tiles - 2)


def test_few_live_rows():
    """30 live rows: fewer than P, more than N | 12: fewer than N | 3: fewer than top_k | none, beside a neighbour that sees every row"""
    X, Q = _world(200, 40, 130)
    rng = np.random.default_rng(6)
    masks = np.stack([_rows(200, rng.choice(200, c, replace=False)) if c else np.zeros(200, bool) for c in (30, 12, 3, 0)] + [np.ones(200, bool)])
    qm = np.arange(130) % 5
    got = _index(X).flat_search_f16_masked(Q, TOP_K, masks, qm, with_stats=True)
    FM.same(got, _ref(X, Q, masks, qm))
    assert np.array_equal(got[2], np.array([5, 5, 3, 0, 5], np.uint32)[qm])


def test_near_copies_flag_a_query_only_while_they_are_live():
    case = (3000, 96, 200, "scaled", 0)
    X, Q, rows = NC.corpus(case)
    half = np.random.default_rng(5).random(3000) < 0.5
    copies_live, copies_dead = half | _rows(3000, rows), half & ~_rows(3000, rows)
    ix = _index(X)
    for live, flagged in ((copies_live, True), (copies_dead, False)):
        ref = _ref(X, Q, live, None, 10)
        got = ix.flat_search_f16_masked(Q, 10, live, exact_mode=1, with_stats=True)
        FM.same(got, ref, what=flagged)
        assert (got[3].exact_queries > 0) == flagged
        FM.same(ix.flat_search_f16_masked(Q, 10, live, exact_mode=2), ref, what=(flagged, 2))
    # ordinary data past the seed chunk: the three modes agree, and only mode 2 leaves the MFMA path
    X, Q = _world(16584, 40, 130)
    masks, qm = np.random.default_rng(7).random((2, 16584)) < 0.5, np.arange(130) % 2
    ref, ix = _ref(X, Q, masks, qm), _index(X)
    for mode in (0, 1, 2):
        got = ix.flat_search_f16_masked(Q, TOP_K, masks, qm, exact_mode=mode, with_stats=True)
        FM.same(got, ref, what=mode)
        assert got[3].exact_queries == (130 if mode == 2 else 0), mode


def test_refusals_and_forwarding():
    import ctypes as C
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X, Q = _world(200, 40, 3)
    half = np.random.default_rng(5).random(200) < 0.5
    ix = _index(X)
    ref = _ref(X, Q, half, None)
    refusals = [(lambda: _index(X, O.STORAGE_U8).flat_search_f16_masked(Q, TOP_K, half), 1),
                (lambda: _index(X, metric=ca.DistanceMetric.DotProduct).flat_search_f16_masked(Q, TOP_K, half), 4),
                (lambda: ix.flat_search_f16_masked(Q, 103, half), 4),
                (lambda: ix.flat_search_f16_masked(Q, TOP_K, np.stack([half, half]), [0, 2, 1]), 3)]
    for call, status in refusals:
        with pytest.raises(ca.CosdataError) as ei:
            call()
        assert ei.value.status == status
        FM.same(ix.flat_search_f16_masked(Q, TOP_K, half), ref, what=status)
    out = np.zeros((3, TOP_K), np.uint32), np.zeros((3, TOP_K), np.float32), np.zeros(3, np.uint32)
    sm, keep = ix._scan_mask(half, None, False, 3)
    opts = _lib.CosFlatF16Opts(struct_size=4, exact_mode=1)                       # a struct_size that is not the struct's
    args = [Q.ctypes.data, 3, TOP_K, C.byref(sm), C.byref(opts)] + [a.ctypes.data for a in out] + [None]
    assert _lib.lib().cos_flat_search_f16_masked_batch(ix._h, *args) == 3
    FM.same(ix.flat_search_f16_masked(Q, TOP_K, half), ref, what="struct_size")
    # a zero-norm row fails the call only while some query can be given it
    Z = X.copy()
    Z[77] = 0
    zix = _index(Z)
    with pytest.raises(ca.CosdataError) as ei:
        zix.flat_search_f16_masked(Q, TOP_K, half | _rows(200, [77]))
    assert ei.value.status == 2
    FM.same(zix.flat_search_f16_masked(Q, TOP_K, half & ~_rows(200, [77])), _ref(X, Q, half & ~_rows(200, [77]), None), what="dead zero row")
    # no mask is the unmasked call; a warm handle (masked, unmasked, masked with another n_masks) equals a cold one
    plain = ix.flat_search_f16(Q, TOP_K)
    FM.same(ix.flat_search_f16_masked(Q, TOP_K), plain, what="mask=None")
    two = np.stack([~half, half])
    FM.same(ix.flat_search_f16_masked(Q, TOP_K, two, [1, 0, 1]), _index(X).flat_search_f16_masked(Q, TOP_K, two, [1, 0, 1]), what="warm")
    FM.same(ix.flat_search_f16_masked(Q, TOP_K, two, [1, 0, 1]), _ref(X, Q, two, [1, 0, 1]), what="warm against the oracle")
