"""cos_sparse_bruteforce_topk (kernels_sparse_brute.hip): the exact top k of a learned-sparse query over the raw rows.

The reference is the rule restated in numpy: per (query, row) the f32 sum in QUERY order, one multiply and one add per shared
dimension; candidates share a dimension and are live; order by (simkey(score), id) descending.  Ids, counts and score bits must be
equal: the rule fixes the order of operations, so there is no tolerance.  A float64 dot bounds the f32 scores as a sanity check.

Shapes: a tile of the scan is up to 8188 nonzeros and up to 1024 rows.  "main" (3000 rows, 0 .. 40 nonzeros) has several chunks and
tiles, rows cut by tile boundaries, a 450-nonzero row placed across the first boundary (the wave-wide path), 1200 rows of 0 .. 3
nonzeros (tiles ended by the row limit), empty rows and 61 copies of one heavy row (ties at every cut).  "n1023/1024/1025" are 0 .. 3
nonzeros per row: one row-limited tile exactly, one row less, one more."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB, BITS, UPPER = 500, 6, 3.0


def _rows(lens, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for ln in lens:
        d = np.sort(rng.choice(VOCAB, int(ln), replace=False)).astype(np.uint32)
        rows.append((d, (rng.integers(1, 13, int(ln)) / 4).astype(np.float32)))  # few distinct values: ties and sums of exactly 0
    return rows


@functools.lru_cache(maxsize=None)
def _corpus(name):
    rng = np.random.default_rng(5)
    if name != "main":
        return _rows(rng.integers(0, 4, int(name[1:])), 7)
    lens = rng.integers(0, 41, 3000)
    lens[rng.random(3000) < 0.05] = 0
    lens[1500:2700] = rng.integers(0, 4, 1200)
    start = np.concatenate([[0], np.cumsum(lens)])
    lens[np.searchsorted(start, 8188 - 100) - 1] = 450  # begins under nonzero 8088 and ends behind 8188
    rows = _rows(lens, 6)
    rows[599] = (rows[599][0], np.full(rows[599][0].size, 3.0, np.float32))
    for r in range(600, 661):
        rows[r] = rows[599]
    return rows


def _csr(rows):
    ro = np.cumsum([0] + [r[0].size for r in rows]).astype(np.uint64)
    return ro, np.concatenate([r[0] for r in rows] + [np.zeros(0, np.uint32)]), np.concatenate([r[1] for r in rows] + [np.zeros(0, np.float32)])


@functools.lru_cache(maxsize=None)
def _queries():
    """17 = one more than a block of 16: 13 fast ones, then unsorted, repeated dimension, 200 pairs, no shared dimension"""
    rng = np.random.default_rng(11)
    qs = []
    for i in range(13):
        d = np.sort(rng.choice(VOCAB, int(rng.integers(1, 31)), replace=False)).astype(np.uint32)
        v = (rng.integers(1, 13, d.size) / 4).astype(np.float32)
        if i % 3 == 1:
            v[::2] *= -1  # scores of both signs, and +0.0 where equal values cancel
        qs.append((d, v))
    d = rng.permutation(VOCAB)[:12].astype(np.uint32)
    qs.append((d, np.linspace(-1, 2, 12).astype(np.float32)))
    qs.append((np.array([3, 9, 9, 40], np.uint32), np.array([1.5, 0.25, 0.75, -2], np.float32)))
    qs.append((np.sort(rng.choice(VOCAB, 200, replace=False)).astype(np.uint32), rng.random(200).astype(np.float32)))
    qs.append((np.array([100000, 100001], np.uint32), np.ones(2, np.float32)))
    return qs


N_SLOW = 3


def _flat(qs):
    qo = np.cumsum([0] + [q[0].size for q in qs]).astype(np.uint32)
    return np.concatenate([q[0] for q in qs]), np.concatenate([q[1] for q in qs]), qo


def _dense(rows):
    val, has = np.zeros((len(rows), VOCAB), np.float32), np.zeros((len(rows), VOCAB), bool)
    for r, (d, v) in enumerate(rows):
        val[r, d], has[r, d] = v, True
    return val, has


def _reference(val, has, live, q):
    """-> ids and f32 scores of every candidate, in the call's order"""
    n = val.shape[0]
    dp, dp64, mag, hit = np.zeros(n, np.float32), np.zeros(n), np.zeros(n), np.zeros(n, bool)
    for d, qv in zip(*q):
        if d < VOCAB:
            m = has[:, d]
            dp[m] = dp[m] + val[m, d] * np.float32(qv)  # f32 multiply, then f32 add
            dp64[m] += val[m, d].astype(np.float64) * float(qv)
            mag[m] += np.abs(val[m, d].astype(np.float64) * float(qv))
            hit |= m
    assert np.all(np.abs(dp - dp64) <= q[0].size * 2.0 ** -23 * mag)
    cand = np.flatnonzero(hit & live)
    b = dp[cand].view(np.uint32)
    key = np.where(b >> 31, ~b, b ^ np.uint32(0x80000000)).astype(np.uint64) << np.uint64(32) | cand.astype(np.uint64)
    order = np.argsort(key)[::-1]
    return cand[order].astype(np.uint32), dp[cand][order]


def _check(ix, rows, live, qs, k):
    ids, scores, counts = ix.bruteforce_topk(*_flat(qs), k)
    val, has = _dense(rows)
    for i, q in enumerate(qs):
        rid, rsc = _reference(val, has, live, q)
        c = min(k, rid.size)
        assert counts[i] == c, (i, counts[i], c)
        assert np.array_equal(ids[i, :c], rid[:c]), i
        assert np.array_equal(scores[i, :c].view(np.uint32), rsc[:c].view(np.uint32)), i
    return ids, scores, counts


@pytest.fixture(scope="module")
def index():
    import cosdata_amd as ca
    made = {}

    def get(name):
        if name not in made:
            made[name] = ca.InvertedIndex.from_vectors(BITS, UPPER, *_csr(_corpus(name)))
        return made[name]

    yield get
    for ix in made.values():
        ix.close()


@pytest.mark.parametrize("name,k,B", [("main", 1, 17), ("main", 10, 17), ("main", 64, 17), ("main", 65, 17), ("main", 1024, 17), ("main", 10, 1),
                                      ("n1023", 10, 17), ("n1024", 10, 17), ("n1025", 10, 17)])
def test_equals_the_rule(index, name, k, B):
    rows, ix = _corpus(name), index(name)
    _, _, counts = _check(ix, rows, np.ones(len(rows), bool), _queries()[:B], k)
    st = ix.last_brute_stats()
    assert (st["queries"], st["slow_queries"], st["pool"]) == (B, N_SLOW if B == 17 else 0, 64 if k <= 64 else 128 if k == 65 else 1024)
    if B == 17:
        assert counts[16] == 0  # shares no dimension with any row


def test_limits_refused_and_handle_usable(index):
    import cosdata_amd as ca
    from cosdata_amd import _lib
    rows, ix = _corpus("n1023"), index("n1023")
    with pytest.raises(ca.CosdataError) as ei:
        ix.bruteforce_topk(*_flat(_queries()), 1025)
    assert ei.value.status == _lib.ERR_UNIMPLEMENTED
    _check(ix, rows, np.ones(len(rows), bool), _queries(), 10)
    bare = ca.InvertedIndex.from_vectors(BITS, UPPER, *_csr(rows), keep_raw=False)
    with pytest.raises(ca.CosdataError) as ei:
        bare.bruteforce_topk(*_flat(_queries()), 10)
    assert ei.value.status == _lib.ERR_NOT_READY
    bare.close()


def test_warm_handle_after_insert_and_delete():
    import cosdata_amd as ca
    rows = list(_corpus("main"))
    ix = ca.InvertedIndex.from_vectors(BITS, UPPER, *_csr(rows))
    more = _rows(np.random.default_rng(2).integers(0, 41, 50), 8)
    assert ix.insert(*_csr(more)) == len(rows)
    rows += more
    gone = np.array([0, 599, 600, 630, 660, 1499, 2999, 3001, 3049], np.uint32)
    ix.delete(gone, *_csr([rows[g] for g in gone]))
    live = np.ones(len(rows), bool)
    live[gone] = False
    ids, _, counts = _check(ix, rows, live, _queries(), 64)
    assert not np.isin(ids[np.arange(64)[None, :] < counts[:, None]], gone).any()
    ix.close()


def test_every_reranked_result_carries_the_brute_force_score(index):
    ix = index("n1023").set_max_candidates(1024)
    qd, qv, qo = _flat(_queries()[:13])
    sid, ssc, scn = ix.search_batch(qd, qv, qo, 10, 0.0, 5)
    bid, bsc, bcn = ix.bruteforce_topk(qd, qv, qo, 1024)
    assert bcn.max() < 1024 and scn.sum() > 0  # k >= candidates: the full list
    for i in range(13):
        full = dict(zip(bid[i, :bcn[i]].tolist(), bsc[i, :bcn[i]].view(np.uint32).tolist()))
        assert all(full[v] == b for v, b in zip(sid[i, :scn[i]].tolist(), ssc[i, :scn[i]].view(np.uint32).tolist()))
