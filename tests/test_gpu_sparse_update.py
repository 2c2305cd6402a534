"""cos_sparse_insert / cos_sparse_delete / cos_sparse_stats / cos_sparse_download on the resident postings, through the C ABI.

Every comparison is on ids, score BITS and counts of every query.  An updated handle is held to three things at once: the
C oracle (oracle.sparse_search + sparse_rerank) on the CSR the state should have (cos_sparse_build_csr of the union after inserts,
the Python model of tests/test_sparse_update_model.py after deletes), a fresh InvertedIndex created from that CSR with the same
n_vectors and raw rows, and download() array for array.

Inputs: every generated query holds a dimension from the five longest lists that still hold a posting, with a value that does
not quantize to 0; early-termination thresholds are 0.0 and 0.5 (<= 0.75); the expected answer of every such query is asserted
non-empty.  The only queries expected to be empty are the ones built to be."""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_sparse_update_model import SparseModel, np_quantize, queries, rows_of, vectors

pytestmark = pytest.mark.gpu

UPPER = 3.0
THRS = (0.0, 0.5)
K_RF = ((10, 0), (64, 0), (12, 5))
SPK_MAX_N = (1 << 24) - 2 * 8192
LAYOUT_BITS = [(0, 4), (0, 6), (0, 8), (1, 4), (1, 6), (1, 8)]


def create(layout, bits, csr, n, raw=None):
    import cosdata_amd as ca
    from cosdata_amd import _lib
    with _lib.tuning(sparse_layout=layout):
        ix = ca.InvertedIndex(bits, UPPER, csr[0], csr[1], csr[2], n, *(raw if raw is not None else ()))
    assert ix.packed == bool(layout)
    return ix


def flat(qs):
    qo = np.cumsum([0] + [len(q[0]) for q in qs]).astype(np.uint32)
    qd = np.concatenate([q[0] for q in qs] + [np.zeros(1, np.uint32)])[:max(int(qo[-1]), 1)]
    qv = np.concatenate([q[1] for q in qs] + [np.zeros(1, np.float32)])[:max(int(qo[-1]), 1)]
    return qd.astype(np.uint32), qv.astype(np.float32), qo


def expected(csr, n, bits, thr, qs, k, rf, raw):
    out = []
    for q in qs:
        cand, sims = O.sparse_search(csr[0], csr[1], csr[2], n, bits, UPPER, thr, q[0], q[1], k_with_reranking=k * max(rf, 1))
        if rf == 0:
            out.append((cand[:k], sims[:k].astype(np.float32)))
        else:
            out.append(tuple(np.asarray(a) for a in O.sparse_rerank(raw[0], raw[1], raw[2], cand, q[0], q[1], top_k=k)))
    return out


def mismatches(got, exp, label):
    ids, sc, cnt = got
    bad = 0
    for i, (ei, es) in enumerate(exp):
        c = int(cnt[i])
        ok = c == len(ei) and np.array_equal(ids[i, :c], ei) and np.array_equal(sc[i, :c].view(np.uint32), np.asarray(es, np.float32).view(np.uint32))
        if not ok:
            if label is not None and bad < 3:
                print(f"MISMATCH {label} query {i}: got {c} {ids[i, :c][:6]} want {len(ei)} {ei[:6]}")
            bad += 1
    return bad


def assert_state(ix, layout, bits, csr, n, raw, qs, label, expect_nonempty=True, fresh_stats=True):
    """ix == the oracle on `csr` == a fresh handle created from `csr` (search bits, stats, postings_visited) == download()"""
    fresh = create(layout, bits, csr, n, raw)
    qd, qv, qo = flat(qs)
    for thr in THRS:
        for k, rf in K_RF:
            if rf and raw is None:
                continue
            exp = expected(csr, n, bits, thr, qs, k, rf, raw)
            if expect_nonempty:
                assert all(len(e[0]) > 0 for e in exp), (label, "a query's expected answer is empty")
            got = ix.search_batch(qd, qv, qo, k, thr, rf)
            visited = ix.last_stats().postings_visited
            assert mismatches(got, exp, f"{label} thr={thr} k={k} rf={rf}") == 0
            fgot = fresh.search_batch(qd, qv, qo, k, thr, rf)
            assert mismatches(fgot, exp, f"{label} (fresh create) thr={thr} k={k} rf={rf}") == 0
            assert fresh.last_stats().postings_visited == visited, (label, thr, k, rf)
    dl = ix.download()
    assert np.array_equal(dl[0], csr[0]) and np.array_equal(dl[1], csr[1]) and np.array_equal(dl[2], csr[2]), label
    sa, sb = ix.stats(), fresh.stats()
    for key in ("n_vectors", "n_dims", "postings", "dir_rows", "dir_tiles", "packed", "have_raw", "raw_pairs"):
        assert sa[key] == sb[key], (label, key, sa, sb)
    assert sa["n_vectors"] == n and sa["postings"] == csr[2].size and sa["device_bytes"] >= 4 * csr[2].size
    fresh.close()


# ---- 1. insert ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,bits", LAYOUT_BITS)
def test_insert_grows_the_index_like_a_fresh_create(layout, bits):
    import cosdata_amd as ca
    n0, vocab = 8000, 500
    steps = (1, 7, 3000)                                                # 8008 -> 11008 crosses 8192
    n_all = n0 + sum(steps)
    raw = vectors(n_all, vocab, 24, seed=40 + bits, lo_vocab=vocab - 6, lo_until=n0 + 8)   # the last batch brings 6 dimensions
    base = rows_of(raw, range(n0))
    csr = ca.sparse_build_csr(bits, UPPER, *base)
    ix = create(layout, bits, csr, n0, base)
    model = SparseModel.from_csr(bits, UPPER, *csr, n0)
    qs = queries(model, 40, vocab, seed=3)
    assert_state(ix, layout, bits, csr, n0, base, qs, "before")
    st0 = ix.stats()
    assert st0["dir_tiles"] == 1 and st0["removed"] == 0
    cur = n0
    for step in steps:
        assert ix.insert(*rows_of(raw, range(cur, cur + step))) == cur
        cur += step
        union = rows_of(raw, range(cur))
        csr = ca.sparse_build_csr(bits, UPPER, *union)
        assert_state(ix, layout, bits, csr, cur, union, qs, f"after +{step}")
    st = ix.stats()
    assert st["dir_tiles"] == 2                                         # a batch crossed a multiple of 8192 ids
    assert st["n_dims"] > st0["n_dims"]                                 # a dimension the index did not have
    assert st["dir_rows"] > st0["dir_rows"]                             # a list grew past 256 postings
    assert st["raw_pairs"] == int(raw[0][-1])
    # vectors without pairs still take ids; m == 0 does nothing
    before = ix.stats()
    assert ix.insert(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32)) == cur
    assert ix.stats() == before
    assert ix.insert(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32)) == cur
    empty_rows = (np.concatenate([union[0], np.full(2, union[0][-1], np.uint64)]), union[1], union[2])
    assert_state(ix, layout, bits, csr, cur + 2, empty_rows, qs, "after two vectors without pairs")
    ix.close()


@pytest.mark.parametrize("layout", [0, 1])
def test_insert_without_raw_vectors_and_with_edge_values(layout):
    import cosdata_amd as ca
    bits, n0, n_all, vocab = 6, 3000, 3400, 400
    ro, rd, rv = vectors(n_all, vocab, 24, seed=9)
    rv = rv.copy()
    rv[int(ro[n0]):int(ro[n0]) + 7] = [0.0, -1.0, 3.0, 2.9999, 1e30, np.nan, 1e-30]
    raw = (ro, rd, rv)
    csr = ca.sparse_build_csr(bits, UPPER, *rows_of(raw, range(n0)))
    ix = create(layout, bits, csr, n0)
    assert ix.insert(*rows_of(raw, range(n0, n_all))) == n0
    csr = ca.sparse_build_csr(bits, UPPER, *raw)
    model = SparseModel.from_csr(bits, UPPER, *csr, n_all)
    assert_state(ix, layout, bits, csr, n_all, None, queries(model, 32, vocab, seed=4), "no raw vectors")
    ix.close()


# ---- 2. delete ----------------------------------------------------------------------------------------------------------------

def _model_state(ix, layout, bits, model, raw, qs, label, **kw):
    assert_state(ix, layout, bits, model.csr(), model.n, raw, qs, label, **kw)


@pytest.mark.parametrize("layout,bits", LAYOUT_BITS)
def test_delete_equals_the_model(layout, bits):
    import cosdata_amd as ca
    n, vocab = 11000, 500
    raw = vectors(n, vocab, 24, seed=60 + bits)
    csr = ca.sparse_build_csr(bits, UPPER, *raw)
    ix = create(layout, bits, csr, n, raw)
    model = SparseModel.from_csr(bits, UPPER, *csr, n)
    rng = np.random.default_rng(bits)
    rows0 = ix.stats()["dir_rows"]

    def both(ids, ro, rd, rv):
        want = model.delete(ids, ro, rd, rv)
        assert ix.delete(ids, ro, rd, rv) == want
        return want

    # a quarter of the vectors with their pairs, in a shuffled order
    quarter = rng.permutation(rng.choice(n, n // 4, replace=False))
    args = rows_of(raw, quarter)
    assert both(quarter, *args) == int(args[0][-1])
    qs = queries(model, 40, vocab, seed=5)
    _model_state(ix, layout, bits, model, raw, qs, "a quarter deleted")
    assert ix.stats()["removed"] == int(args[0][-1])
    # the same call again removes nothing and swaps nothing
    dl = ix.download()
    assert both(quarter, *args) == 0
    assert all(np.array_equal(a, b) for a, b in zip(dl, ix.download()))
    # values that quantize to another key: the postings stay
    alive = np.setdiff1d(np.arange(n), quarter)
    some = alive[:300]
    ro, rd, rv = rows_of(raw, some)
    key = np_quantize(rv, UPPER, bits)
    other = np.where(key < (1 << bits) - 1, key + 1, key - 1)
    moved = ((other + 0.5) / ((1 << bits) - 1) * UPPER).astype(np.float32)
    assert not np.any(np_quantize(moved, UPPER, bits) == key)
    # (a vector may hold the moved key in the same dimension only if it names the dimension twice: these rows do not)
    assert both(some, ro, rd, moved) == 0
    assert all(np.array_equal(a, b) for a, b in zip(dl, ix.download()))
    # a subset of a vector's pairs; ids the index never held; unknown dimensions
    sub = alive[300:900]
    ro, rd, rv = rows_of(raw, sub)
    keep = np.concatenate([np.arange(int(ro[i]), int(ro[i + 1]))[i % 2::2] for i in range(sub.size)])
    sro = np.concatenate([[0], np.cumsum([len(np.arange(int(ro[i]), int(ro[i + 1]))[i % 2::2]) for i in range(sub.size)])]).astype(np.uint64)
    assert both(sub, sro, rd[keep], rv[keep]) == keep.size
    assert both(np.array([n, n + 5, 0xFFFFFFFF], np.uint32), np.array([0, 1, 2, 3], np.uint64), rd[:3], rv[:3]) == 0
    assert both(alive[:2], np.array([0, 1, 2], np.uint64), np.array([100000, 100001], np.uint32), np.array([1.0, 2.0], np.float32)) == 0
    _model_state(ix, layout, bits, model, raw, qs, "subset of pairs")
    # enough of one list that it falls back to 256 postings or fewer: it loses its directory row
    lens = {d: sum(len(l) for l in node) for d, node in model.lists.items()}
    d_fall = min((d for d in lens if lens[d] > 256), key=lambda d: lens[d])
    pairs = [(v, k) for k, l in enumerate(model.lists[d_fall]) for v in l][: lens[d_fall] - 250]
    centre = lambda k: np.float32((k + 0.5) / ((1 << bits) - 1) * UPPER) if k < (1 << bits) - 1 else np.float32(UPPER)
    assert all(int(np_quantize([centre(k)], UPPER, bits)[0]) == k for k in range(1 << bits))
    rows_before = ix.stats()["dir_rows"]
    assert both(np.array([v for v, _ in pairs], np.uint32), np.arange(len(pairs) + 1).astype(np.uint64), np.full(len(pairs), d_fall, np.uint32),
                np.array([centre(k) for _, k in pairs], np.float32)) == len(pairs)
    assert ix.stats()["dir_rows"] == rows_before - 1
    # every posting of one dimension: a query on it alone returns nothing; the dimension stays in the table
    d_gone = min(lens, key=lambda d: lens[d])
    pairs = [(v, k) for k, l in enumerate(model.lists[d_gone]) for v in l]
    n_dims = ix.stats()["n_dims"]
    assert both(np.array([v for v, _ in pairs], np.uint32), np.arange(len(pairs) + 1).astype(np.uint64), np.full(len(pairs), d_gone, np.uint32),
                np.array([centre(k) for _, k in pairs], np.float32)) == len(pairs)
    assert ix.stats()["n_dims"] == n_dims
    qs = queries(model, 40, vocab, seed=6)
    _model_state(ix, layout, bits, model, raw, qs, "a list below the threshold, a dimension emptied")
    alone = [(np.array([d_gone], np.uint32), np.array([2.0], np.float32))]
    for thr in THRS:
        ids, sc, cnt = ix.search_batch(*flat(alone), 10, thr, 0)
        assert cnt[0] == 0
    # a later insert revives the dimension (and goes behind the survivors of every list)
    more = vectors(600, vocab, 24, seed=99)
    row0 = more[1][:int(more[0][1])]                                    # its first vector names the emptied dimension (dims stay ascending)
    if d_gone not in row0.tolist():
        row0[0] = d_gone
        row0.sort()
    first = model.insert(*more)
    assert ix.insert(*more) == first == n
    raw2 = (np.concatenate([raw[0], raw[0][-1] + more[0][1:]]), np.concatenate([raw[1], more[1]]), np.concatenate([raw[2], more[2]]))
    _model_state(ix, layout, bits, model, raw2, qs, "insert after the deletes")
    ids, sc, cnt = ix.search_batch(*flat(alone), 10, 0.0, 0)
    assert cnt[0] >= 1 and ids[0, :cnt[0]].min() >= n                   # only vectors of the later insert
    ix.close()


# ---- 3. a vector that names one dimension twice ---------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_vector_that_names_a_dimension_twice(layout):
    import cosdata_amd as ca
    bits, n, vocab = 8, 3000, 400
    raw = vectors(n, vocab, 24, seed=7)
    csr = ca.sparse_build_csr(bits, UPPER, *raw)
    ix = create(layout, bits, csr, n)
    model = SparseModel.from_csr(bits, UPPER, *csr, n)
    heavy = model.longest()
    da, db = int(heavy[0]), int(heavy[1])
    # vector n: dimension da twice with one key; vector n + 1: dimension db with two keys and da four times
    upd = (np.array([0, 2, 8], np.uint64), np.array([da, da, db, da, db, da, da, da], np.uint32),
           np.array([2.9, 2.9, 2.9, 2.99, 1.0, 2.99, 2.99, 2.99], np.float32))
    assert ix.insert(*upd) == model.insert(*upd) == n
    # large query values on 8-bit keys: 255 * 255 * 4 = 260100 per term; with the multiplicity the sum passes 2^22 only if the
    # bound sees it — either way the answer is the model's
    qs = queries(model, 24, vocab, seed=8)
    qs += [(np.array([da, db] + [int(d) for d in heavy[2:]], np.uint32), np.full(len(heavy), 3.0, np.float32)),
           (np.array([da] * 16 + [db] * 16, np.uint32), np.full(32, 3.0, np.float32)),
           (np.array([da], np.uint32), np.array([3.0], np.float32))]
    _model_state(ix, layout, bits, model, None, qs, "repeated dimension")
    ids, sc, cnt = ix.search_batch(*flat(qs[-1:]), 10, 0.0, 0)
    assert ids[0, 0] == n + 1 and sc[0, 0] == float(4 * 255 * int(np_quantize([2.99], UPPER, bits)[0]))
    one = (np.array([n], np.uint32), np.array([0, 1], np.uint64), np.array([da], np.uint32), np.array([2.9], np.float32))
    assert ix.delete(*one) == model.delete(*one) == 1                   # one of the two
    _model_state(ix, layout, bits, model, None, qs, "one of two removed")
    both = (np.array([n, n + 1], np.uint32), np.array([0, 2, 5], np.uint64), np.array([da, da, da, da, db], np.uint32),
            np.array([2.9, 2.9, 2.99, 2.99, 1.0], np.float32))
    assert ix.delete(*both) == model.delete(*both) == 4                 # the second 2.9 of vector n is already gone
    _model_state(ix, layout, bits, model, None, qs, "more removed")
    ix.close()


# ---- 4. random interleavings ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,bits,seed", [(0, 6, 1), (1, 6, 2), (1, 8, 3), (0, 4, 4), (1, 4, 5)])
def test_random_interleaving_of_inserts_deletes_and_searches(layout, bits, seed):
    import cosdata_amd as ca
    n0, n_all, vocab = 2500, 5000, 400
    raw = vectors(n_all, vocab, 24, seed=80 + seed, lo_vocab=vocab - 10, lo_until=n0)
    base = rows_of(raw, range(n0))
    csr = ca.sparse_build_csr(bits, UPPER, *base)
    ix = create(layout, bits, csr, n0, base)
    model = SparseModel.from_csr(bits, UPPER, *csr, n0)
    rng = np.random.default_rng(seed)
    cur, deleted = n0, set()
    for step in range(10):
        if rng.random() < 0.5 and cur < n_all:
            m = int(rng.choice([1, 7, 150, 400]))
            m = min(m, n_all - cur)
            upd = rows_of(raw, range(cur, cur + m))
            assert ix.insert(*upd) == model.insert(*upd) == cur
            cur += m
        else:
            ids = rng.choice(cur, int(rng.integers(1, 300)), replace=False)     # some of them deleted before: nothing to find
            args = rows_of(raw, ids)
            assert ix.delete(ids, *args) == model.delete(ids, *args)
            deleted |= set(ids.tolist())
        if step % 3 == 2 or step == 9:
            _model_state(ix, layout, bits, model, rows_of(raw, range(cur)), queries(model, 24, vocab, seed=seed * 100 + step), f"step {step}")
    ix.close()


# ---- 5. failure leaves the handle as it was ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_rejected_updates_leave_the_handle_unchanged(layout):
    import cosdata_amd as ca
    bits, n, vocab = 6, 3000, 400
    raw = vectors(n + 20, vocab, 24, seed=11)
    base = rows_of(raw, range(n))
    csr = ca.sparse_build_csr(bits, UPPER, *base)
    ix = create(layout, bits, csr, n, base)
    model = SparseModel.from_csr(bits, UPPER, *csr, n)
    qs = queries(model, 24, vocab, seed=12)
    qd, qv, qo = flat(qs)
    want = {(thr, k, rf): ix.search_batch(qd, qv, qo, k, thr, rf) for thr in THRS for k, rf in K_RF}
    want_dl, want_st = ix.download(), ix.stats()
    good = rows_of(raw, range(n, n + 20))

    def rejected(fn, status):
        with pytest.raises(ca.CosdataError) as ei:
            fn()
        assert ei.value.status == status
        for (thr, k, rf), w in want.items():
            got = ix.search_batch(qd, qv, qo, k, thr, rf)
            assert np.array_equal(got[2], w[2])
            assert mismatches(got, [(w[0][i, :int(w[2][i])], w[1][i, :int(w[2][i])]) for i in range(len(qs))], "after a rejected call") == 0
        assert all(np.array_equal(a, b) for a, b in zip(want_dl, ix.download()))
        assert ix.stats() == want_st

    ro = good[0].copy(); ro[5] = ro[4] - 1
    rejected(lambda: ix.insert(ro, good[1], good[2]), 3)                 # decreasing row_offsets
    ro = good[0].copy(); ro[0] = 1
    rejected(lambda: ix.insert(ro, good[1], good[2]), 3)                 # row_offsets[0] != 0
    rd = good[1].copy(); a = int(good[0][3]); rd[a], rd[a + 1] = rd[a + 1], rd[a]
    rejected(lambda: ix.insert(good[0], rd, good[2]), 3)                 # descending dims in a row, raw vectors kept
    rejected(lambda: ix.delete(np.arange(20, dtype=np.uint32), ro, good[1], good[2]), 3)
    assert ix.insert(*good) == n                                         # and the handle still takes the good update
    union = rows_of(raw, range(n + 20))
    assert_state(ix, layout, bits, ca.sparse_build_csr(bits, UPPER, *union), n + 20, union, qs, "after the rejected calls")
    ix.close()


def test_insert_past_the_packed_limit_is_refused():
    import cosdata_amd as ca
    bits, n = 6, SPK_MAX_N - 3
    ids = np.array([5, n - 1, 70000, 8191, 8192], np.uint32)
    ro = np.array([0, 2, 3, 5], np.uint64)                              # three vectors' worth of pairs ...
    rd, rv = np.array([3, 9, 3, 3, 9], np.uint32), np.array([1.0, 2.0, 1.0, 2.5, 0.2], np.float32)
    dims = np.array([3, 9], np.uint32)
    w = (1 << bits) + 1
    ko = np.zeros(2 * w, np.uint64)
    ko[1:w] = 3; ko[w:] = 3; ko[w + 1:] = 5                              # ... filed as a handful of postings at key 0 of two dimensions
    csr = (dims, ko, ids)
    ix = create(1, bits, csr, n)
    qs = [(np.array([3, 9], np.uint32), np.array([1.0, 1.0], np.float32)), (np.array([9], np.uint32), np.array([2.0], np.float32))]
    qd, qv, qo = flat(qs)
    want, want_st, want_dl = ix.search_batch(qd, qv, qo, 10, 0.0, 0), ix.stats(), ix.download()
    assert want[2].tolist() == [5, 2]
    with pytest.raises(ca.CosdataError) as ei:
        ix.insert(np.array([0, 1, 2, 3, 4], np.uint64), rd[:4], rv[:4])  # n + 4 > SPK_MAX_N
    assert ei.value.status == 4                                          # COS_ERR_UNIMPLEMENTED
    got = ix.search_batch(qd, qv, qo, 10, 0.0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and ix.stats() == want_st
    assert all(np.array_equal(a, b) for a, b in zip(want_dl, ix.download()))
    assert ix.insert(ro, rd, rv) == n                                    # exactly up to the limit is taken
    assert ix.stats()["n_vectors"] == SPK_MAX_N
    got = ix.search_batch(qd, qv, qo, 10, 0.0, 0)
    assert got[2].tolist() == [8, 4] and got[0][1, 0] == n
    ix.close()


# ---- 6. a search thread beside the updates ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 1])
def test_search_thread_sees_the_index_before_or_after_an_update(layout):
    import cosdata_amd as ca
    bits, n0, step, rounds, vocab, k = 6, 6000, 400, 6, 400, 10
    raw = vectors(n0 + rounds * step, vocab, 24, seed=13)
    base = rows_of(raw, range(n0))
    csr = ca.sparse_build_csr(bits, UPPER, *base)
    ix = create(layout, bits, csr, n0, base)
    model = SparseModel.from_csr(bits, UPPER, *csr, n0)
    qs = queries(model, 16, vocab, seed=14)
    qd, qv, qo = flat(qs)
    # the states the index goes through: insert, delete, insert, delete, ...
    ops, states = [], [expected(model.csr(), model.n, bits, 0.0, qs, k, 0, None)]
    cur = n0
    for r in range(rounds):
        if r % 2 == 0:
            upd = rows_of(raw, range(cur, cur + step))
            model.insert(*upd)
            ops.append(("insert", upd))
            cur += step
        else:
            ids = np.arange(r * 97, r * 97 + 500, dtype=np.uint32)
            args = (ids,) + rows_of(raw, ids)
            model.delete(*args)
            ops.append(("delete", args))
        states.append(expected(model.csr(), model.n, bits, 0.0, qs, k, 0, None))
        assert all(len(e[0]) > 0 for e in states[-1])
    state, stop, seen, errs = [0], threading.Event(), [], []

    def searcher():
        try:
            while not stop.is_set():
                lo = state[0]
                got = ix.search_batch(qd, qv, qo, k, 0.0, 0)
                seen.append((lo, min(state[0] + 1, rounds), got))        # an update that began after `lo` was read may have finished
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    t = threading.Thread(target=searcher)
    t.start()
    try:
        for r, (what, args) in enumerate(ops):
            getattr(ix, what)(*args)
            state[0] = r + 1
    finally:
        stop.set()
        t.join()
    assert not errs, errs
    assert seen
    bad = sum(not any(mismatches(got, states[s], None) == 0 for s in range(lo, hi + 1)) for lo, hi, got in seen)
    assert bad == 0, (bad, len(seen))
    assert mismatches(ix.search_batch(qd, qv, qo, k, 0.0, 0), states[rounds], "final") == 0
    ix.close()
