"""The mixed hybrid call (cos_hybrid_search_mixed: repo::batch_hybrid_search, api/vectordb/search/repo.rs:343-555): every query names
its arm, the dense / learned-sparse / BM25 searches run for top_k * 3 over their own sub-batches and RRF fuses each query's two lists on
the device.  Everything is compared on ids, score bits and counts, with no tolerance, against the oracle's composition (dense
search, sparse_search [+ sparse_rerank], bm25_search, rrf_fuse), against a dict restatement of the fusion rule written here, and
against the same batch taken through the separate entry points of the C ABI.

One id space of n = 6000 is shared by the three indexes.  The base batch has 48 queries, arms cycling 0, 1, 2.  Half of them are
TARGETED: all halves of the query are derived from the same document, so that the two lists share ids (the fusion's add path); the
others come from the generators of tests/test_gpu_hybrid.py and tests/test_sparse.py; three are built to leave a list empty."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_gpu_hybrid import _postings, _queries as _bm25_queries
from tests.test_sparse import _corpus, _queries as _sparse_queries

pytestmark = pytest.mark.gpu

N, DIM, VOCAB, BITS, UPPER, B0 = 6000, 96, 300, 6, 3.0, 48
UNKNOWN_TERM = 12345                      # (the generator of tests/test_gpu_hybrid.py uses it too: no posting list)
EMPTY_SECOND = {3: "sparse", 4: "bm25"}   # base queries whose SECOND list is empty; query 5 (SPARSE_BM25) has both lists empty


class Data:
    """corpora, oracle-side indexes and the 48 base queries: everything the CPU needs (no device)"""

    def __init__(self):
        self.X = H.clustered_corpus(N, DIM, n_centers=12, seed=6)
        self.oix = H.oracle_index(self.X, O.STORAGE_U8, 0, num_layers=4, ef_construction=48, ef_search=96)
        self.bm = _postings(N, VOCAB, 9)                                   # terms, offsets, docs, tfs
        self.rows, self.dims, self.key_off, self.vec_ids, self.row_off, self.raw_dims, self.raw_vals = _corpus(n=N, vocab=VOCAB, bits=BITS, upper=UPPER, seed=4)
        terms, offsets, docs, _ = self.bm
        term_of = np.repeat(terms, np.diff(offsets).astype(np.int64))
        rng = np.random.default_rng(77)
        target = rng.integers(0, N, B0)
        gen_bm = _bm25_queries(terms, B0, 5)
        gen_sp = _sparse_queries(B0, VOCAB, seed=3)
        self.arm = np.arange(B0, dtype=np.uint8) % 3
        self.dense, self.sparse, self.bm25 = [None] * B0, [None] * B0, [None] * B0
        for q in range(B0):
            a, v = int(self.arm[q]), int(target[q])
            targeted = (q // 3) % 2 == 0
            if a != 2:                                                     # dense half: a noisy copy of a document (of the target when targeted)
                src = v if targeted else int(rng.integers(0, N))
                self.dense[q] = (self.X[src] + 0.02 * rng.standard_normal(DIM)).astype(np.float32)
            if a != 1:                                                     # sparse half: the target's own pairs (some dropped), or a generator query
                if targeted:
                    d, x = self.rows[v]
                    keep = rng.random(d.size) < 0.8
                    keep[0] = True
                    self.sparse[q] = (d[keep].copy(), x[keep].copy())
                else:
                    self.sparse[q] = gen_sp[q]
            if a != 0:                                                     # BM25 half: every term that holds the target, or a generator query
                if targeted:
                    t = np.unique(term_of[docs == v])
                    self.bm25[q] = (t if t.size else np.array([UNKNOWN_TERM], np.uint32)).astype(np.uint32)
                else:
                    self.bm25[q] = gen_bm[0][gen_bm[1][q]:gen_bm[1][q + 1]].copy()
        unknown_dims = (np.array([VOCAB + 500, VOCAB + 501], np.uint32), np.array([1.0, 2.0], np.float32))
        self.sparse[3] = unknown_dims                                      # DENSE_SPARSE with an empty second list
        self.bm25[4] = np.array([UNKNOWN_TERM, UNKNOWN_TERM + 1], np.uint32)   # DENSE_BM25 with an empty second list
        self.sparse[5] = unknown_dims                                      # SPARSE_BM25 with both lists empty: fused count 0
        self.bm25[5] = np.array([UNKNOWN_TERM], np.uint32)
        self._lists = {}

    # ---- the oracle's lists, computed once per (kind, query, width, threshold, rerank) ----
    def dense_lists(self, k3):
        key = ("dense", k3)
        if key not in self._lists:
            idx = [q for q in range(B0) if self.dense[q] is not None]
            ids, _, cnt = self.oix.search_batch(np.stack([self.dense[q] for q in idx]), k3, threads=4)[:3]
            self._lists[key] = {q: ids[i, :cnt[i]].copy() for i, q in enumerate(idx)}
        return self._lists[key]

    def sparse_list(self, q, k3, thr, rf, csr=None, raw=None, n=N):
        key = ("sparse", q, k3, thr, rf, id(csr))
        if key not in self._lists:
            dims, key_off, vec_ids = csr if csr is not None else (self.dims, self.key_off, self.vec_ids)
            row_off, raw_dims, raw_vals = raw if raw is not None else (self.row_off, self.raw_dims, self.raw_vals)
            d, x = self.sparse[q]
            cand, _ = O.sparse_search(dims, key_off, vec_ids, n, BITS, UPPER, thr, d, x, k_with_reranking=k3 * max(rf, 1))
            self._lists[key] = cand[:k3] if rf == 0 else O.sparse_rerank(row_off, raw_dims, raw_vals, cand, d, x, top_k=k3)[0]
        return self._lists[key]

    def bm25_list(self, q, k3):
        key = ("bm25", q, k3)
        if key not in self._lists:
            self._lists[key] = O.bm25_search(*self.bm, N, self.bm25[q], k3)[0]
        return self._lists[key]

    def two_lists(self, q, k, thr=0.0, rf=0):
        a, k3 = int(self.arm[q]), 3 * k
        first = self.dense_lists(k3)[q] if a != 2 else self.sparse_list(q, k3, thr, rf)
        second = self.sparse_list(q, k3, thr, rf) if a == 0 else self.bm25_list(q, k3)
        return first, second

    # ---- a request over the base queries `idx` (any order, repeats allowed) ----
    def request(self, idx):
        arms = self.arm[idx]
        dq = [self.dense[q] for q in idx if self.dense[q] is not None]
        sq = [self.sparse[q] for q in idx if self.sparse[q] is not None]
        bq = [self.bm25[q] for q in idx if self.bm25[q] is not None]
        dense = np.stack(dq) if dq else None
        sparse = flat_sparse(sq) if sq else None
        bm25 = (np.concatenate(bq).astype(np.uint32), np.cumsum([0] + [t.size for t in bq]).astype(np.uint32)) if bq else None
        return arms, dense, sparse, bm25


def flat_sparse(qs):
    return (np.concatenate([q[0] for q in qs]).astype(np.uint32), np.concatenate([q[1] for q in qs]).astype(np.float32),
            np.cumsum([0] + [len(q[0]) for q in qs]).astype(np.uint32))


def rrf_restated(first, second, kc, top_k):
    """repo.rs:524-549 with a dict and np.float32 arithmetic: the first list INSERTS 1 / (rank + k + EPSILON), so a later occurrence
    of an id overwrites; the second list ADDS; then fused score descending (all positive: total_cmp is <), larger id first, top_k"""
    eps, one, kc = np.float32(1.1920929e-07), np.float32(1.0), np.float32(kc)
    final = {}
    for rank, i in enumerate(np.asarray(first).tolist()):
        final[i] = one / ((np.float32(rank) + kc) + eps)
    for rank, i in enumerate(np.asarray(second).tolist()):
        final[i] = np.float32(final.get(i, np.float32(0.0)) + one / ((np.float32(rank) + kc) + eps))
    order = sorted(final.items(), key=lambda t: (-float(t[1]), -t[0]))[:top_k]
    return np.array([i for i, _ in order], np.uint32), np.array([s for _, s in order], np.float32)


_data = None


def data() -> Data:
    global _data
    if _data is None:
        _data = Data()
    return _data


def expected(q, k, thr=0.0, rf=0, kc=60.0):
    """(ids, scores) of base query q: O.rrf_fuse of the oracle's two lists — and the dict restatement agrees with it"""
    d = data()
    key = ("fused", q, k, thr, rf, kc)
    if key not in d._lists:
        first, second = d.two_lists(q, k, thr, rf)
        fi, fs = O.rrf_fuse(first, second, kc, k)
        ri, rs = rrf_restated(first, second, kc, k)
        assert np.array_equal(fi, ri) and np.array_equal(fs.view(np.uint32), rs.view(np.uint32)), (q, k, fi[:5], ri[:5])
        d._lists[key] = (fi, fs)
    return d._lists[key]


def overlap_conditions(k, thr=0.0, rf=0):
    """what the base batch must exercise at this top_k, counted on the oracle's lists alone"""
    d = data()
    both = {0: 0, 1: 0, 2: 0}
    short = empty_second = below = 0
    for q in range(B0):
        first, second = d.two_lists(q, k, thr, rf)
        both[int(d.arm[q])] += bool(np.intersect1d(first, second).size)
        short += first.size < 3 * k or second.size < 3 * k
        empty_second += second.size == 0
        below += expected(q, k, thr, rf)[0].size < k
    return both, short, empty_second, below


class Handles:
    def __init__(self):
        import cosdata_amd as ca
        from cosdata_amd import _lib
        d = data()
        self.ctx = ca.HybridContext()
        self.dix = H.device_index_from_oracle(d.oix, d.X)
        self.bm = ca.BM25Index(*d.bm, N)
        args = (BITS, UPPER, d.dims, d.key_off, d.vec_ids, N, d.row_off, d.raw_dims, d.raw_vals)
        self.sp = {}
        for layout in (0, 1):                                              # 1 = packed, the default at this size
            with _lib.tuning(sparse_layout=layout):
                self.sp[layout] = ca.InvertedIndex(*args)
            assert self.sp[layout].packed == bool(layout)
            self.sp[layout].set_max_candidates(1024)
        self.sp_narrow = ca.InvertedIndex(*args)                           # left at the default of 64 candidates
        self.sp_no_raw = ca.InvertedIndex(*args[:6]).set_max_candidates(1024)

    def close(self):
        for x in [self.ctx, self.bm, self.sp_narrow, self.sp_no_raw] + list(self.sp.values()):
            x.close()


@pytest.fixture(scope="module")
def hx():
    h = Handles()
    yield h
    h.close()


def mixed(hx, idx, k, thr=0.0, rf=0, sp="default", ix="default", bm="default", ctx=None, kc=60.0):
    import cosdata_amd as ca
    arms, dense, sparse, bm25 = data().request(idx)
    return ca.hybrid_search_mixed(ctx or hx.ctx, hx.dix if ix == "default" else ix, hx.sp[1] if sp == "default" else sp, hx.bm if bm == "default" else bm,
                                  arms, dense, sparse, bm25, k, kc, thr, rf)


def assert_equals_expected(got, idx, k, thr=0.0, rf=0):
    ids, sc, cnt = got
    bad = []
    for i, q in enumerate(idx):
        fi, fs = expected(int(q), k, thr, rf)
        c = int(cnt[i])
        if not (c == fi.size and np.array_equal(ids[i, :c], fi) and np.array_equal(sc[i, :c].view(np.uint32), fs.view(np.uint32))):
            bad.append((i, int(q), c, fi.size, ids[i, :min(c, 4)].tolist(), fi[:4].tolist()))
        assert np.all(ids[i, c:] == 0xFFFFFFFF) and np.all(sc[i, c:] == 0), ("entries past the count were written", i)
    assert not bad, bad[:5]


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


ALL = np.arange(B0)


# ---- 1. parity of a mixed batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,rf,thr,layout", [
    (10, 0, 0.0, 1),     # narrow sparse path (30 candidates), RRF R = 1
    (30, 0, 0.0, 1),     # sparse R = 2 (90), RRF R = 4 (180 ids)
    (30, 0, 0.0, 0),     # ... on the unpacked sparse layout
    (170, 0, 0.0, 1),    # the limit: 510 of BM25's 512 buckets, sparse R = 8, RRF R = 16, a dense side shorter than 510
    (30, 2, 0.0, 1),     # raw-value rerank of 180 candidates
    (10, 0, 0.3, 1),     # early termination
])
def test_mixed_batch_matches_oracle_composition(hx, k, rf, thr, layout):
    both, short, empty_second, below = overlap_conditions(k, thr, rf)
    print("queries with an id on both lists per arm", both, "| a short side", short, "| empty second list", empty_second, "| fused count below top_k", below)
    assert all(v >= 4 for v in both.values()), both                        # a quarter of the 16 queries of every arm
    assert short >= 1 and empty_second >= 1 and below >= 1
    if k == 170:
        assert all(l.size < 510 for l in data().dense_lists(510).values())  # ef_search 96 bounds what the dense half returns
    got = mixed(hx, ALL, k, thr, rf, sp=hx.sp[layout])
    assert_equals_expected(got, ALL, k, thr, rf)


# ---- 2. the same batch through the separate entry points ---------------------------------------------------------------------
@pytest.mark.parametrize("k,rf", [(10, 0), (30, 2)])
def test_composition_through_the_abi_gives_the_same_bits(hx, k, rf):
    import cosdata_amd as ca
    d = data()
    arms, dense, sparse, bm25 = d.request(ALL)
    k3 = 3 * k
    di, _, dc = hx.dix.batch_search(dense, k3)[:3]
    si, _, sc_ = hx.sp[1].search_batch(*sparse, k3, 0.0, rf)
    bi, _, bc = hx.bm.search_batch(*bm25, k3)
    first = np.zeros((B0, k3), np.uint32); second = np.zeros((B0, k3), np.uint32)
    fc = np.zeros(B0, np.uint32); sc2 = np.zeros(B0, np.uint32)
    nd = ns = nb = 0                                                       # the running counts of the request's query_mapping
    for q in range(B0):
        a = int(arms[q])
        if a == 0:
            first[q], fc[q], second[q], sc2[q] = di[nd], dc[nd], si[ns], sc_[ns]; nd += 1; ns += 1
        elif a == 1:
            first[q], fc[q], second[q], sc2[q] = di[nd], dc[nd], bi[nb], bc[nb]; nd += 1; nb += 1
        else:
            first[q], fc[q], second[q], sc2[q] = si[ns], sc_[ns], bi[nb], bc[nb]; ns += 1; nb += 1
    want = ca.rrf_fuse_batch(first, fc, second, sc2, 60.0, k)
    got = mixed(hx, ALL, k, 0.0, rf)
    assert np.array_equal(got[2], want[2])
    for q in range(B0):
        c = int(want[2][q])
        assert np.array_equal(got[0][q, :c], want[0][q, :c]) and np.array_equal(got[1][q, :c].view(np.uint32), want[1][q, :c].view(np.uint32)), q


def test_all_dense_bm25_batch_equals_cos_hybrid_search_batch(hx):
    import cosdata_amd as ca
    idx = np.array([q for q in range(B0) if data().arm[q] == 1] * 2)
    arms, dense, _, bm25 = data().request(idx)
    for k in (10, 170):
        want = ca.hybrid_search_batch(hx.dix, hx.bm, dense, bm25[0], bm25[1], k, 60.0)
        got = mixed(hx, idx, k, sp=None)
        assert np.array_equal(got[2], want[2])
        for i in range(idx.size):
            c = int(want[2][i])
            assert np.array_equal(got[0][i, :c], want[0][i, :c]) and np.array_equal(got[1][i, :c].view(np.uint32), want[1][i, :c].view(np.uint32)), (k, i)
        assert_equals_expected(got, idx, k)


# ---- 3. shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [0, 1, 2, 3, 4, 5])
def test_single_query_of_each_arm(hx, q):
    """B = 1 (the single-query hybrid_search): a targeted query of every arm, and the three with an empty list"""
    assert_equals_expected(mixed(hx, np.array([q]), 10), [q], 10)


@pytest.mark.parametrize("absent", [0, 1, 2])
def test_batch_without_one_arm(hx, absent):
    """no query of one arm: all three halves still run; and a batch of ONE arm only, with the handle it does not need NULL"""
    idx = np.array([q for q in range(B0) if data().arm[q] != absent])
    assert_equals_expected(mixed(hx, idx, 10), idx, 10)
    only = np.array([q for q in range(B0) if data().arm[q] == absent])
    null = {0: dict(bm=None), 1: dict(sp=None), 2: dict(ix=None)}[absent]
    assert_equals_expected(mixed(hx, only, 10, **null), only, 10)
    assert_equals_expected(mixed(hx, only, 10), only, 10)                  # a handle that is not needed may also be there


def test_batch_larger_than_a_client_batch(hx):
    """B = 300: more than one 256-query batch of the host, base queries repeated in a shuffled order"""
    idx = np.random.default_rng(1).permutation(np.arange(300) % B0)
    assert_equals_expected(mixed(hx, idx, 10), idx, 10)


# ---- 4. refusals and recovery --------------------------------------------------------------------------------------------------
def test_refusals_report_their_status_and_leave_the_handles_as_they_were(hx):
    import cosdata_amd as ca
    good = mixed(hx, ALL, 10)
    assert_equals_expected(good, ALL, 10)

    def refused(status, **kw):
        with pytest.raises(ca.CosdataError) as ei:
            mixed(hx, kw.pop("idx", ALL), kw.pop("k", 10), **kw)
        assert ei.value.status == status, (status, str(ei.value))
        assert same_bits(good, mixed(hx, ALL, 10)), "the call after the refusal differs"

    refused(4, k=171)                                                      # 3 * 171 > 512: Unimplemented
    good_narrow = mixed(hx, ALL, 10, sp=hx.sp_narrow)                      # 30 candidates fit the default of 64
    assert same_bits(good, good_narrow)
    refused(4, k=30, sp=hx.sp_narrow)                                      # 90 candidates on a handle left at 64
    refused(4, k=10, rf=3, sp=hx.sp_narrow)
    assert same_bits(good, mixed(hx, ALL, 10, sp=hx.sp_narrow))
    assert same_bits(good, mixed(hx, ALL, 10, sp=hx.sp_no_raw))            # no rerank asked: no raw vectors needed
    refused(6, k=10, rf=2, sp=hx.sp_no_raw)                                # NotReady
    assert same_bits(good, mixed(hx, ALL, 10, sp=hx.sp_no_raw))
    refused(3, sp=None)                                                    # a needed handle is NULL
    refused(3, bm=None)
    refused(3, ix=None)
    refused(3, k=0)
    # an arm value of 3
    arms, dense, sparse, bm25 = data().request(ALL)
    bad = arms.copy()
    bad[7] = 3
    with pytest.raises(ca.CosdataError) as ei:
        ca.hybrid_search_mixed(hx.ctx, hx.dix, hx.sp[1], hx.bm, bad, dense, sparse, bm25, 10)
    assert ei.value.status == 3
    # decreasing offsets, a small struct_size, B == 0
    for which in ("sparse", "bm25"):
        off = (sparse[2] if which == "sparse" else bm25[1]).copy()
        off[5] = off[6] + 1                                                # offsets[6] < offsets[5]
        with pytest.raises(ca.CosdataError) as ei:
            ca.hybrid_search_mixed(hx.ctx, hx.dix, hx.sp[1], hx.bm, arms, dense, (sparse[0], sparse[1], off) if which == "sparse" else sparse,
                                   (bm25[0], off) if which == "bm25" else bm25, 10)
        assert ei.value.status == 3, which
    from cosdata_amd import _lib
    rq = _lib.CosHybridRequest()
    rq.struct_size = C.sizeof(_lib.CosHybridRequest) - 4
    out = np.zeros(16, np.uint32)
    p = out.ctypes.data_as(C.c_void_p)
    assert _lib.lib().cos_hybrid_search_mixed(hx.ctx._h, hx.dix._h, hx.sp[1]._h, hx.bm._h, C.byref(rq), p, p, p) == 3
    rq.struct_size = C.sizeof(_lib.CosHybridRequest)
    assert _lib.lib().cos_hybrid_search_mixed(hx.ctx._h, hx.dix._h, hx.sp[1]._h, hx.bm._h, C.byref(rq), p, p, p) == 3   # B == 0
    assert same_bits(good, mixed(hx, ALL, 10))


def test_zero_norm_dense_query_fails_the_call_and_the_next_call_answers(hx):
    import cosdata_amd as ca
    good = mixed(hx, ALL, 10)
    arms, dense, sparse, bm25 = data().request(ALL)
    dz = dense.copy()
    dz[9] = -1.0                                                           # quantizes to all-zero bytes -> |q| = 0
    with pytest.raises(ca.CosdataError) as ei:
        ca.hybrid_search_mixed(hx.ctx, hx.dix, hx.sp[1], hx.bm, arms, dz, sparse, bm25, 10)
    assert ei.value.status == 2
    assert "query 13" in str(ei.value)                                     # dense row 9 is request query 13 (rows 0, 1 | 3, 4 | ...: two per three queries)
    assert same_bits(good, mixed(hx, ALL, 10))


# ---- 5. the sparse search on a stream, results left on the device ---------------------------------------------------------------
@pytest.mark.parametrize("k,rf,thr,layout", [(10, 0, 0.0, 1), (30, 2, 0.0, 1), (64, 0, 0.3, 0), (170, 3, 0.0, 1)])
def test_sparse_search_batch_device_equals_search_batch(hx, k, rf, thr, layout):
    import torch
    sp = hx.sp[layout]
    qd, qv, qo = flat_sparse([q for q in data().sparse if q is not None])
    B = qo.size - 1
    ids, sc, cnt = sp.search_batch(qd, qv, qo, k, thr, rf)
    visited = int(sp.last_stats().postings_visited)
    assert visited > 0
    dev = torch.device("cuda:0")
    for stream in (torch.cuda.Stream(device=dev), None):                   # a stream of the caller's, and the default stream
        o_i = torch.zeros(B, k, dtype=torch.int32, device=dev); o_s = torch.zeros(B, k, device=dev); o_c = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        sp.search_batch_device(qd, qv, qo, k, o_i.data_ptr(), o_s.data_ptr(), o_c.data_ptr(), thr, rf, stream.cuda_stream if stream else 0)
        st = sp.last_stats()                                               # waits for the batch
        assert int(st.postings_visited) == visited and st.kernel_ms > 0
        torch.cuda.synchronize()
        gc = o_c.cpu().numpy().view(np.uint32)
        assert np.array_equal(gc, cnt)
        gi, gs = o_i.cpu().numpy().view(np.uint32), o_s.cpu().numpy()
        for b in range(B):
            c = int(cnt[b])
            assert np.array_equal(gi[b, :c], ids[b, :c]) and np.array_equal(gs[b, :c].view(np.uint32), sc[b, :c].view(np.uint32)), b
    again = sp.search_batch(qd, qv, qo, k, thr, rf)
    assert same_bits((ids, sc, cnt), again)


# ---- 6. after an update of both postings indexes -------------------------------------------------------------------------------
def test_mixed_call_after_insert_and_delete(hx):
    """the sparse and the BM25 index start with ids 0 .. 5799, get 5800 .. 5999 inserted and 50 ids deleted; the dense index is
    untouched.  Expected: the oracle's sparse search on the updated CSR (the model of tests/test_sparse_update_model.py keeps it),
    the BM25 model of tests/test_bm25_update_model.py (tombstones stay in a list's length), the oracle's dense search and RRF."""
    import cosdata_amd as ca
    from tests.test_bm25_update_model import ModelIndex
    from tests.test_sparse_update_model import SparseModel, rows_of
    d = data()
    n0, k, k3 = 5800, 10, 30
    # 50 ids to delete: 20 that the fused lists of the base batch hold (oracle lists only), 30 spread over the id space
    hot = np.unique(np.concatenate([expected(q, k)[0] for q in range(B0)]))[::5][:20]
    spread = np.setdiff1d(np.arange(7, N, 97, dtype=np.uint32), hot)[:50 - hot.size]
    dele = np.sort(np.concatenate([hot, spread])).astype(np.uint32)
    assert dele.size == 50 and hot.size == 20
    raw = (d.row_off, d.raw_dims, d.raw_vals)
    # learned-sparse
    base = rows_of(raw, np.arange(n0))
    sp = ca.InvertedIndex.from_vectors(BITS, UPPER, *base, keep_raw=True).set_max_candidates(1024)
    sm = SparseModel(BITS, UPPER)
    sm.insert(*base)
    upd = rows_of(raw, np.arange(n0, N))
    assert sp.insert(*upd) == n0 and sm.insert(*upd) == n0
    dr = rows_of(raw, dele)
    assert sp.delete(dele, *dr) == sm.delete(dele, *dr) > 0
    csr = sm.csr()
    # BM25: the term-major postings split by document id
    terms, offsets, docs, tfs = d.bm
    term_of = np.repeat(terms, np.diff(offsets).astype(np.int64))
    old = docs < n0
    t0, c0 = np.unique(term_of[old], return_counts=True)
    base_csr = (t0.astype(np.uint32), np.concatenate([[0], np.cumsum(c0)]).astype(np.uint64), docs[old], tfs[old])
    bm = ca.BM25Index(*base_csr, n0)
    model = ModelIndex(*base_csr, n0)

    def doc_major(ids):
        sel = np.flatnonzero(np.isin(docs, ids))
        o = sel[np.lexsort((term_of[sel], docs[sel]))]
        off = np.searchsorted(docs[o], np.concatenate([ids, [np.uint32(0xFFFFFFFF)]])).astype(np.uint64)
        off[-1] = o.size
        return np.asarray(ids, np.uint32), off, term_of[o].astype(np.uint32), tfs[o].astype(np.float32)

    u = doc_major(np.arange(n0, N, dtype=np.uint32))
    bm.insert(*u); model.insert(*u)
    u = doc_major(dele)
    bm.delete(*u[:3]); model.delete(*u[:3])
    got = mixed(hx, ALL, k, sp=sp, bm=bm)
    dense = d.dense_lists(k3)
    bad = []
    for q in range(B0):
        a = int(d.arm[q])
        sl = d.sparse_list(q, k3, 0.0, 0, csr=csr, n=N) if a != 1 else None
        bl = model.search(d.bm25[q], k3)[0] if a != 0 else None
        first, second = (dense[q], sl) if a == 0 else (dense[q], bl) if a == 1 else (sl, bl)
        fi, fs = O.rrf_fuse(first, second, 60.0, k)
        c = int(got[2][q])
        if not (c == fi.size and np.array_equal(got[0][q, :c], fi) and np.array_equal(got[1][q, :c].view(np.uint32), fs.view(np.uint32))):
            bad.append((q, a, c, fi.size))
        if a != 1:
            assert not np.isin(sl, dele).any()
    assert not bad, bad
    sp.close(); bm.close()
