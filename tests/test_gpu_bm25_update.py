"""cos_bm25_insert / cos_bm25_delete / cos_bm25_stats / cos_bm25_download on the resident postings, through the C ABI.

Every comparison is on ids, score BITS and counts, for cos_bm25_search_batch and cos_bm25_search_batch_device (and
cos_hybrid_search_batch where named).  Insert-only states are held to a fresh cos_bm25_create from the merged CSR and to
oracle.bm25_search on it; states with tombstones to the Python model of tests/test_bm25_update_model.py (the oracle takes a
plain CSR and cannot express a tombstone).

Inputs: posting lists at most n_docs // 3 long (the bound asked for is n_docs // 2; the tighter one keeps
documents_count >= len for every list even after the SAME quarter of the documents is deleted twice, which lowers
documents_count twice), at most a quarter of the documents deleted, every query with at least one term that keeps a live
posting (asserted) except in the test of the tombstones-only list."""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_bm25_update_model import ModelIndex

pytestmark = pytest.mark.gpu

N, N0, VOCAB = 30000, 22000, 3000
_TF = np.array([[O.bm25_tf(c, dl, 100.0, 1.5, 0.75) for dl in range(20, 301)] for c in range(1, 6)], np.float32)


class Corpus:
    """document-major postings (ids 0 .. n-1, term hashes ascending inside a document) and their term-major slices"""

    def __init__(self, n, vocab, seed, cap=None):
        rng = np.random.default_rng(seed)
        self.n = n
        self.terms = np.sort(rng.choice(1 << 31, vocab, replace=False)).astype(np.uint32)
        df = np.clip((n / (1.0 + np.arange(vocab)) ** 1.05).astype(np.int64), 1, cap if cap is not None else n // 3)
        self.heavy = None
        rng.shuffle(df)
        self.heavy = self.terms[np.argsort(-df)[:5]]
        d = np.concatenate([rng.choice(n, int(x), replace=False) for x in df]).astype(np.uint32)
        h = np.repeat(self.terms, df)
        tf = _TF[rng.integers(0, 5, d.size), rng.integers(0, 281, d.size)]
        o = np.lexsort((h, d))
        self.doc, self.hash, self.tf = d[o], h[o], tf[o]
        self.doc_off = np.searchsorted(self.doc, np.arange(n + 1)).astype(np.uint64)

    def csr(self, lo, hi):
        """term-major CSR of documents [lo, hi): terms with a posting there, ascending; doc ids ascending inside a list"""
        a, b = int(self.doc_off[lo]), int(self.doc_off[hi])
        o = np.argsort(self.hash[a:b], kind="stable")
        h = self.hash[a:b][o]
        terms, counts = np.unique(h, return_counts=True)
        off = np.zeros(terms.size + 1, np.uint64)
        off[1:] = np.cumsum(counts)
        return terms.astype(np.uint32), off, self.doc[a:b][o], self.tf[a:b][o]

    def update(self, ids, subset=None):
        """(doc_ids, doc_offsets, term_hashes, tfs) of the documents `ids`; subset(i, n_terms) -> indices kept of document i's terms"""
        th, tf, off = [], [], [0]
        for i in np.asarray(ids).tolist():
            a, b = int(self.doc_off[i]), int(self.doc_off[i + 1])
            sel = np.arange(b - a) if subset is None else subset(i, b - a)
            th.append(self.hash[a:b][sel]); tf.append(self.tf[a:b][sel])
            off.append(off[-1] + len(sel))
        return (np.asarray(ids, np.uint32), np.array(off, np.uint64), np.concatenate(th).astype(np.uint32) if th else np.zeros(0, np.uint32),
                np.concatenate(tf).astype(np.float32) if tf else np.zeros(0, np.float32))


_corpora = {}


def corpus(n=N, vocab=VOCAB, seed=21):
    key = (n, vocab, seed)
    if key not in _corpora:
        _corpora[key] = Corpus(n, vocab, seed)
    return _corpora[key]


def queries(c: Corpus, B, seed, pool=None):
    """each query: one of the five longest lists (a term that keeps live postings) + up to 7 others, sometimes an unknown term"""
    rng = np.random.default_rng(seed)
    pool = c.terms if pool is None else pool
    qt, qo = [], [0]
    for _ in range(B):
        t = np.unique(np.concatenate([rng.choice(c.heavy, 1), rng.choice(pool, int(rng.integers(0, 8)), replace=False)]))
        rng.shuffle(t)
        if rng.random() < 0.3:
            t = np.concatenate([t, np.array([12345], np.uint32)])
        qt.append(t.astype(np.uint32)); qo.append(qo[-1] + t.size)
    return np.concatenate(qt), np.array(qo, np.uint32)


def device_search(bm, qt, qo, k):
    import torch
    B = qo.size - 1
    dev = torch.device("cuda:0")
    o_i = torch.zeros(B, k, dtype=torch.int32, device=dev); o_s = torch.zeros(B, k, device=dev); o_c = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    bm.search_batch_device(qt, qo, k, o_i.data_ptr(), o_s.data_ptr(), o_c.data_ptr(), st.cuda_stream)
    st.synchronize()
    return o_i.cpu().numpy().view(np.uint32), o_s.cpu().numpy(), o_c.cpu().numpy().view(np.uint32)


def mismatches(got, expected, label=""):
    """got = (ids [B][k], scores, counts); expected = list of (ids, scores) per query -> number of queries that differ in any bit"""
    ids, sc, cnt = got
    bad = 0
    for i, (ei, es) in enumerate(expected):
        c = int(cnt[i])
        ok = c == ei.size and np.array_equal(ids[i, :c], ei) and np.array_equal(sc[i, :c].view(np.uint32), es.view(np.uint32))
        if not ok:
            if label is not None and bad < 3:
                print(f"MISMATCH {label} query {i}: got {c} {ids[i, :c][:6]} want {ei.size} {ei[:6]}")
            bad += 1
    return bad


def check_against(bm, expected, qt, qo, k, label):
    assert mismatches(bm.search_batch(qt, qo, k), expected, label + " host-out") == 0
    assert mismatches(device_search(bm, qt, qo, k), expected, label + " device-out") == 0


def oracle_expected(csr, n_docs, qt, qo, k):
    return [O.bm25_search(csr[0], csr[1], csr[2], csr[3], n_docs, qt[qo[i]:qo[i + 1]], k) for i in range(qo.size - 1)]


def model_expected(model, qt, qo, k):
    return [model.search(qt[qo[i]:qo[i + 1]], k) for i in range(qo.size - 1)]


def assert_download_equals(bm, csr, tomb=None):
    th, off, di, tf, tb = bm.download()
    assert np.array_equal(th, csr[0]) and np.array_equal(off, csr[1]) and np.array_equal(di, csr[2])
    assert np.array_equal(tf.view(np.uint32), np.asarray(csr[3], np.float32).view(np.uint32))
    assert np.array_equal(tb, np.zeros(di.size, bool) if tomb is None else tomb)


def assert_same_as_fresh(bm, csr, n_docs, qt, qo, k, label):
    """the updated handle == a fresh cos_bm25_create from the merged CSR == oracle.bm25_search on it (tile directory included:
    the fresh handle's comes from the host pass of create, the updated one's from bm25_tile_dir_kernel)"""
    import cosdata_amd as ca
    exp = oracle_expected(csr, n_docs, qt, qo, k)
    check_against(bm, exp, qt, qo, k, label)
    fresh = ca.BM25Index(csr[0], csr[1], csr[2], csr[3], n_docs)
    check_against(fresh, exp, qt, qo, k, label + " (fresh create)")
    fi, fs, fc = fresh.search_batch(qt, qo, k)                        # (entries past a query's count are not written: compare up to it)
    assert mismatches(bm.search_batch(qt, qo, k), [(fi[i, :int(fc[i])], fs[i, :int(fc[i])]) for i in range(qo.size - 1)], label + " vs fresh") == 0
    sa, sb = bm.stats(), fresh.stats()
    for key in ("documents_count", "n_terms", "postings", "tombstones", "dir_rows", "dir_tiles"):
        assert sa[key] == sb[key], (key, sa, sb)
    fresh.close()


# ---- 1. insert only ---------------------------------------------------------------------------------------------------------

def test_insert_grows_the_index_like_a_fresh_create():
    import cosdata_amd as ca
    c = corpus()
    base = c.csr(0, N0)
    bm = ca.BM25Index(*base, N0)
    qt, qo = queries(c, 48, 5)
    assert_same_as_fresh(bm, base, N0, qt, qo, 20, "before")
    cur = N0
    for step in (1, 7, 3000):
        bm.insert(*c.update(np.arange(cur, cur + step)))
        cur += step
        merged = c.csr(0, cur)
        assert_same_as_fresh(bm, merged, cur, qt, qo, 20, f"after +{step}")
        assert_download_equals(bm, merged)
        st = bm.stats()
        assert st["documents_count"] == cur and st["n_terms"] == merged[0].size and st["postings"] == merged[2].size
        assert st["tombstones"] == 0 and st["largest_doc_id"] == cur - 1
        assert st["device_bytes"] >= 8 * merged[2].size
    bm.close()


# ---- 2. directory transitions -------------------------------------------------------------------------------------------------

def _lists_case(lists, split, n_total):
    """lists: {term hash: ascending doc ids}.  Index of the documents < split, grown by the documents >= split in ONE insert,
    against a fresh create of everything and the oracle.  Queries: every term alone, and mixes."""
    import cosdata_amd as ca
    d = np.concatenate([np.asarray(v, np.uint32) for v in lists.values()])
    h = np.concatenate([np.full(len(v), t, np.uint32) for t, v in lists.items()])
    tf = (0.25 + ((d.astype(np.uint64) * 7 + h) % 13).astype(np.float32) / 8).astype(np.float32)
    o = np.lexsort((h, d))
    c = Corpus.__new__(Corpus)
    c.n, c.doc, c.hash, c.tf = n_total, d[o], h[o], tf[o]
    c.doc_off = np.searchsorted(c.doc, np.arange(n_total + 1)).astype(np.uint64)
    c.terms = np.array(sorted(lists), np.uint32)
    base, merged = c.csr(0, split), c.csr(0, n_total)
    bm = ca.BM25Index(*base, split)
    rng = np.random.default_rng(len(lists))
    qs = [np.array([t], np.uint32) for t in c.terms] + [rng.choice(c.terms, min(c.terms.size, int(rng.integers(2, 7))), replace=False) for _ in range(24)]
    qt, qo = np.concatenate(qs).astype(np.uint32), np.concatenate([[0], np.cumsum([q.size for q in qs])]).astype(np.uint32)
    assert_same_as_fresh(bm, base, split, qt, qo, 15, "base")
    bm.insert(*c.update(np.arange(split, n_total)))
    assert_same_as_fresh(bm, merged, n_total, qt, qo, 15, "grown")
    assert_download_equals(bm, merged)
    return bm, c, merged, (qt, qo)


def _spread(rng, n, lo, hi):
    return np.sort(rng.choice(np.arange(lo, hi), n, replace=False)).astype(np.uint32)


def _background(rng, split, n_total):
    """two long lists (directory rows before and after) and a short one, over the whole id range"""
    return {50: np.concatenate([_spread(rng, split // 3, 0, split), _spread(rng, (n_total - split) // 3, split, n_total)]),
            4000000000: np.concatenate([_spread(rng, split // 4, 0, split), _spread(rng, (n_total - split) // 4, split, n_total)]),
            777: np.concatenate([_spread(rng, 40, 0, split), _spread(rng, 9, split, n_total)])}


@pytest.mark.parametrize("before,after", [(250, 255), (250, 256), (250, 257), (255, 257), (256, 257), (257, 300), (1, 257), (256, 256)])
def test_list_pushed_across_the_directory_threshold(before, after):
    rng = np.random.default_rng(before * 1000 + after)
    split, n_total = 20000, 21000
    lists = _background(rng, split, n_total)
    lists[123456] = np.concatenate([_spread(rng, before, 0, split), _spread(rng, after - before, split, n_total)])
    bm, _, merged, _ = _lists_case(lists, split, n_total)
    assert bm.stats()["dir_rows"] == 2 + (after > 256)
    bm.close()


def test_largest_id_moves_from_8191_to_8192():
    rng = np.random.default_rng(1)
    lists = {50: _spread(rng, 3000, 0, 8192), 60: np.concatenate([_spread(rng, 300, 0, 8191), [8191, 8192]]).astype(np.uint32),
             70: np.array([5, 8192], np.uint32), 80: _spread(rng, 100, 0, 8192)}
    lists[50] = np.unique(np.concatenate([lists[50], [8191]])).astype(np.uint32)
    bm, _, _, _ = _lists_case(lists, 8192, 8193)
    assert bm.stats()["dir_tiles"] == 2 and bm.stats()["largest_doc_id"] == 8192
    bm.close()


def test_one_tile_becomes_five():
    rng = np.random.default_rng(2)
    split, n_total = 5000, 5 * 8192 - 100
    lists = _background(rng, split, n_total)
    lists[60] = np.concatenate([_spread(rng, 200, 0, split), np.array([8192, 16383, 16384, 3 * 8192, n_total - 1], np.uint32)])
    bm, _, _, _ = _lists_case(lists, split, n_total)
    assert bm.stats()["dir_tiles"] == 5
    bm.close()


@pytest.mark.parametrize("where", ["before_first", "between", "after_last", "all_three"])
def test_term_that_exists_only_in_the_update(where):
    rng = np.random.default_rng(3)
    split, n_total = 12000, 14000
    lists = _background(rng, split, n_total)             # existing hashes: 50, 777, 4000000000
    new = {"before_first": [7], "between": [900], "after_last": [4100000000], "all_three": [7, 900, 4100000000]}[where]
    for j, t in enumerate(new):
        lists[t] = _spread(rng, (3, 300, 40)[j % 3] if where == "all_three" else 300, split, n_total)
    bm, _, merged, _ = _lists_case(lists, split, n_total)
    assert bm.stats()["n_terms"] == 3 + len(new)
    bm.close()


def test_update_that_touches_no_existing_term():
    rng = np.random.default_rng(4)
    split, n_total = 9000, 9500
    lists = {50: _spread(rng, 3000, 0, split), 777: _spread(rng, 40, 0, split), 4000000000: _spread(rng, 257, 0, split),
             60: _spread(rng, 10, split, n_total), 3000000000: _spread(rng, 260, split, n_total)}
    bm, _, _, _ = _lists_case(lists, split, n_total)
    bm.close()


def test_insert_of_no_documents_is_a_no_op():
    import cosdata_amd as ca
    c = corpus()
    base = c.csr(0, N0)
    bm = ca.BM25Index(*base, N0)
    z32, z64 = np.zeros(0, np.uint32), np.zeros(1, np.uint64)
    before = bm.stats()
    bm.insert(z32, z64, z32, np.zeros(0, np.float32))
    bm.delete(z32, z64, z32)
    assert bm.stats() == before
    assert_download_equals(bm, base)
    bm.close()


# ---- 3. delete --------------------------------------------------------------------------------------------------------------

def _assert_state(bm, model, c, qt, qo, k, label):
    for i in range(qo.size - 1):                            # the inputs' own condition: a live posting for every query
        assert any(t in model.lists and not all(model.lists[t][2]) for t in qt[qo[i]:qo[i + 1]].tolist()), (label, i)
    check_against(bm, model_expected(model, qt, qo, k), qt, qo, k, label)
    mt, mo, md, mf, mtomb = model.csr()
    assert_download_equals(bm, (mt, mo, md, mf), mtomb)
    st = bm.stats()
    assert st["documents_count"] == model.documents_count and st["tombstones"] == int(mtomb.sum()) and st["postings"] == md.size


def test_delete_then_insert_equals_the_model():
    import cosdata_amd as ca
    c = corpus()
    base = c.csr(0, N0)
    bm = ca.BM25Index(*base, N0)
    model = ModelIndex(*base, N0)
    qt, qo = queries(c, 32, 6)
    rng = np.random.default_rng(8)
    _assert_state(bm, model, c, qt, qo, 20, "fresh")
    one = np.array([4321], np.uint32)
    u = c.update(one)
    bm.delete(*u[:3]); model.delete(*u[:3])
    _assert_state(bm, model, c, qt, qo, 20, "one deleted")
    quarter = np.sort(rng.choice(np.setdiff1d(np.arange(N0), one), N0 // 4 - 1, replace=False)).astype(np.uint32)
    u = c.update(quarter)
    bm.delete(*u[:3]); model.delete(*u[:3])
    _assert_state(bm, model, c, qt, qo, 20, "a quarter deleted")
    assert bm.stats()["documents_count"] == N0 - N0 // 4
    # the same ids again: lists unchanged, documents_count lower again (the reference's behaviour)
    lists_before = bm.download()
    bm.delete(*u[:3]); model.delete(*u[:3])
    again = bm.download()
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(lists_before, again))
    assert bm.stats()["documents_count"] == N0 - N0 // 4 - quarter.size
    _assert_state(bm, model, c, qt, qo, 20, "deleted twice")
    # an insert AFTER the deletes: tombstones travel through the merge, new postings go behind them
    u = c.update(np.arange(N0, N0 + 2500))
    bm.insert(*u); model.insert(*u)
    _assert_state(bm, model, c, qt, qo, 20, "insert after deletes")
    u = c.update(np.arange(N0 + 100, N0 + 900, 3))
    bm.delete(*u[:3]); model.delete(*u[:3])
    _assert_state(bm, model, c, qt, qo, 20, "delete of inserted documents")
    bm.close()


def test_delete_with_a_subset_of_the_terms_and_with_unknown_terms():
    import cosdata_amd as ca
    c = corpus()
    base = c.csr(0, N0)
    bm = ca.BM25Index(*base, N0)
    model = ModelIndex(*base, N0)
    qt, qo = queries(c, 32, 9)
    rng = np.random.default_rng(10)
    ids = np.sort(rng.choice(N0, 1500, replace=False)).astype(np.uint32)
    di, do, th, _ = c.update(ids, subset=lambda i, n: np.arange(n)[i % 2::2])      # every other term of each document
    bm.delete(di, do, th); model.delete(di, do, th)
    _assert_state(bm, model, c, qt, qo, 20, "subset of terms")
    # terms the index does not hold, mixed with terms it holds but the document does not have
    ids2 = np.sort(rng.choice(N0, 300, replace=False)).astype(np.uint32)
    th2 = np.tile(np.array([3, 12345, int(c.heavy[0]), 4294967295], np.uint32), ids2.size)
    do2 = (np.arange(ids2.size + 1) * 4).astype(np.uint64)
    bm.delete(ids2, do2, th2); model.delete(ids2, do2, th2)
    _assert_state(bm, model, c, qt, qo, 20, "unknown terms")
    bm.close()


def test_list_that_holds_tombstones_only_contributes_nothing():
    import cosdata_amd as ca
    rng = np.random.default_rng(11)
    lists = {50: _spread(rng, 3000, 0, 9000), 60: np.array([17, 4000, 8500], np.uint32), 70: _spread(rng, 300, 0, 9000)}
    d = np.concatenate(list(lists.values())); h = np.concatenate([np.full(len(v), t, np.uint32) for t, v in lists.items()])
    o = np.lexsort((d, h))
    terms = np.array([50, 60, 70], np.uint32)
    off = np.array([0, 3000, 3003, 3303], np.uint64)
    docs = d[o].astype(np.uint32)
    tfs = (0.25 + (docs % 11).astype(np.float32) / 4).astype(np.float32)
    bm = ca.BM25Index(terms, off, docs, tfs, 9000)
    model = ModelIndex(terms, off, docs, tfs, 9000)
    args = (np.array([17, 4000, 8500], np.uint32), np.array([0, 1, 2, 3], np.uint64), np.array([60, 60, 60], np.uint32))
    bm.delete(*args); model.delete(*args)
    qs = [np.array([60], np.uint32), np.array([60, 50], np.uint32), np.array([70, 60], np.uint32), np.array([50, 70, 60], np.uint32)]
    qt, qo = np.concatenate(qs), np.concatenate([[0], np.cumsum([q.size for q in qs])]).astype(np.uint32)
    ids, sc, cnt = bm.search_batch(qt, qo, 10)
    assert cnt[0] == 0
    check_against(bm, model_expected(model, qt, qo, 10), qt, qo, 10, "tombstones only")
    assert bm.stats()["tombstones"] == 3 and bm.stats()["documents_count"] == 8997
    bm.close()


# ---- 4. hybrid --------------------------------------------------------------------------------------------------------------

def test_hybrid_search_on_an_updated_bm25_index():
    import cosdata_amd as ca
    n, n0, d, B, k = 6000, 5000, 96, 40, 10
    X = H.clustered_corpus(n, d, n_centers=12, seed=6)
    oix = H.oracle_index(X, O.STORAGE_U8, 0, num_layers=4, ef_construction=48, ef_search=96)
    dix = H.device_index_from_oracle(oix, X)
    c = corpus(n, 400, 33)
    base = c.csr(0, n0)
    bm = ca.BM25Index(*base, n0)
    model = ModelIndex(*base, n0)
    u = c.update(np.arange(n0, n))
    bm.insert(*u); model.insert(*u)
    dele = np.arange(3, n, 5, dtype=np.uint32)                        # a fifth of the documents
    u = c.update(dele)
    bm.delete(*u[:3]); model.delete(*u[:3])
    Q = H.queries_from(X, B, seed=2)
    qt, qo = queries(c, B, 5)
    ids, sc, cnt = ca.hybrid_search_batch(dix, bm, Q, qt, qo, k, 60.0)
    od = oix.search_batch(Q, 3 * k, threads=4)
    bad = 0
    for i in range(B):
        oi, _ = model.search(qt[qo[i]:qo[i + 1]], 3 * k)
        fi, fs = O.rrf_fuse(od[0][i, :od[2][i]], oi, 60.0, k)
        cc = int(cnt[i])
        bad += not (cc == fi.size and np.array_equal(ids[i, :cc], fi) and np.array_equal(sc[i, :cc].view(np.uint32), fs.view(np.uint32)))
    assert bad == 0
    bm.close()


# ---- 5. errors leave the handle as it was -----------------------------------------------------------------------------------

def test_rejected_updates_leave_the_handle_unchanged():
    import cosdata_amd as ca
    c = corpus()
    base = c.csr(0, N0)
    bm = ca.BM25Index(*base, N0)
    bm.insert(*c.update(np.arange(N0, N0 + 50)))                      # an updated handle: largest id ever held = N0 + 49
    qt, qo = queries(c, 24, 12)
    want_search = bm.search_batch(qt, qo, 10)
    want_dl, want_st = bm.download(), bm.stats()
    good = c.update(np.arange(N0 + 50, N0 + 60))

    def rejected(fn):
        with pytest.raises(ca.CosdataError) as ei:
            fn()
        assert ei.value.status == 3                                    # COS_ERR_INVALID
        wi, ws, wc = want_search
        assert mismatches(bm.search_batch(qt, qo, 10), [(wi[i, :int(wc[i])], ws[i, :int(wc[i])]) for i in range(qo.size - 1)], "after a rejected call") == 0
        assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(want_dl, bm.download()))
        assert bm.stats() == want_st

    ids = good[0].copy(); ids[3], ids[4] = ids[4], ids[3]
    rejected(lambda: bm.insert(ids, *good[1:]))                        # ids not ascending
    ids = good[0].copy(); ids[5] = ids[4]
    rejected(lambda: bm.insert(ids, *good[1:]))                        # ... not strictly
    low = c.update(np.arange(N0 + 49, N0 + 59))
    rejected(lambda: bm.insert(*low))                                  # an id not above the largest ever held
    th = good[2].copy()
    a = int(good[1][int(np.argmax(np.diff(good[1].astype(np.int64)) >= 2))])   # a document with two terms or more
    th[a + 1] = th[a]
    rejected(lambda: bm.insert(good[0], good[1], th, good[3]))         # a term hash repeated inside a document
    tf = good[3].copy(); tf[7] = np.nan
    rejected(lambda: bm.insert(good[0], good[1], good[2], tf))         # a NaN tf
    tf = good[3].copy(); tf[0] = np.inf
    rejected(lambda: bm.insert(good[0], good[1], good[2], tf))
    bm.insert(*good)                                                   # and the handle still takes the good update
    merged = c.csr(0, N0 + 60)
    assert_same_as_fresh(bm, merged, N0 + 60, qt, qo, 10, "after the rejected calls")
    bm.close()
    # documents_count < m on delete
    small = ca.BM25Index(*base, 3)
    want_dl, want_st = small.download(), small.stats()
    u = c.update(np.arange(10, 14))
    with pytest.raises(ca.CosdataError) as ei:
        small.delete(*u[:3])
    assert ei.value.status == 3
    assert small.stats() == want_st
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(want_dl, small.download()))
    small.close()


# ---- 6. a search thread beside the inserts ----------------------------------------------------------------------------------

def test_search_thread_sees_the_index_before_or_after_an_insert():
    import cosdata_amd as ca
    c = corpus()
    rounds, step, k = 6, 500, 10
    qt, qo = queries(c, 16, 13)
    states = [oracle_expected(c.csr(0, N0 + r * step), N0 + r * step, qt, qo, k) for r in range(rounds + 1)]
    bm = ca.BM25Index(*c.csr(0, N0), N0)
    state = [0]                                                        # inserts completed so far (written by the main thread)
    stop = threading.Event()
    seen, errs = [], []

    def searcher():
        try:
            while not stop.is_set():
                lo = state[0]
                got = bm.search_batch(qt, qo, k)
                hi = state[0] + 1                                      # an insert that began after `lo` was read may have finished
                seen.append((lo, min(hi, rounds), got))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    t = threading.Thread(target=searcher)
    t.start()
    try:
        for r in range(rounds):
            bm.insert(*c.update(np.arange(N0 + r * step, N0 + (r + 1) * step)))
            state[0] = r + 1
    finally:
        stop.set()
        t.join()
    assert not errs, errs
    assert seen
    bad = 0
    for lo, hi, got in seen:                                           # every answer is the answer of ONE whole state
        bad += not any(mismatches(got, states[s], None) == 0 for s in range(lo, hi + 1))
    assert bad == 0, (bad, len(seen))
    check_against(bm, states[rounds], qt, qo, k, "final")
    bm.close()
