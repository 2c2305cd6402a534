"""The text collection of the shard-set BM25 / hybrid tests (test_gpu_shardset_bm25.py, test_gpu_shardset_hybrid.py), the expected
answers from the oracle, and CPU restatements of the two sharding schemes that are NOT exact — asserted to differ from the expected
answer before anything runs on the device, so that the tests cannot pass on a scheme that is wrong.

The collection: N documents (global ids 0 .. N - 1) over VOCAB term hashes with Zipf weights, 3-12 distinct terms per document, stored
tf uniform in (0.2, 2.2); N_EXTRA further documents (ids N ..) for the insert tests, some with terms no document below N has."""
import ctypes
import ctypes.util

import numpy as np

from oracle import oracle as O

N, VOCAB, NQ = 12000, 300, 37
N_EXTRA, N_NEW_TERMS = 500, 20
BOUNDS3 = [0, 9000, 10000, 12000]                  # shard 0 spans two 8192-id tiles; 9000 and 10000 are no multiples of 512
BOUNDS8 = [1536 * s for s in range(8)] + [N]       # 8 x 1536 (bases multiples of 512; the last shard is 1248 documents)
SEED = 5
ALPHA = 1.8                                        # Zipf exponent of the term weights
UNKNOWN = np.uint32(0x7FFFFFF1)                    # a term hash no document has

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.log1pf.restype = ctypes.c_float
_libm.log1pf.argtypes = [ctypes.c_float]


def idf(n_docs, length):
    """get_idf with the reference's u32 wrap, on the host libm (what bm25_prepare computes)"""
    num = np.float32(np.uint32((int(n_docs) - int(length)) & 0xFFFFFFFF)) + np.float32(0.5)
    return np.float32(_libm.log1pf(np.float32(num / (np.float32(length) + np.float32(0.5)))))


class World:
    def __init__(self, seed=SEED, alpha=ALPHA):
        rng = np.random.default_rng(seed)
        n_all = N + N_EXTRA
        hashes = np.sort(rng.choice(1 << 31, VOCAB + N_NEW_TERMS, replace=False)).astype(np.uint32)
        pick = rng.permutation(VOCAB + N_NEW_TERMS)
        self.terms = np.sort(hashes[pick[:VOCAB]])                 # the collection's vocabulary
        self.new_terms = np.sort(hashes[pick[VOCAB:]])             # terms only the extra documents have
        w = 1.0 / (1.0 + np.arange(VOCAB)) ** alpha
        w = w[rng.permutation(VOCAB)]                              # (weight and hash order are unrelated)
        n_t = rng.integers(3, 13, n_all)
        keys = np.log(w)[None, :] + rng.gumbel(size=(n_all, VOCAB))   # Gumbel top-k: n_t distinct terms, probability by weight
        order = np.argsort(-keys, axis=1)
        docs, hs = [], []
        for d in range(n_all):
            t = self.terms[order[d, :n_t[d]]]
            if d >= N and rng.random() < 0.3:
                t = np.concatenate([t, rng.choice(self.new_terms, 1)])
            docs.append(np.full(t.size, d, np.uint32)); hs.append(np.sort(t))
        self.doc, self.hash = np.concatenate(docs), np.concatenate(hs).astype(np.uint32)
        self.tf = rng.uniform(0.2, 2.2, self.doc.size).astype(np.float32)
        self.doc_off = np.searchsorted(self.doc, np.arange(n_all + 1)).astype(np.uint64)
        # 37 queries of 1-6 distinct terms of the vocabulary, uniform over it (rare terms are the ones a small shard lacks)
        qt, qo = [], [0]
        for _ in range(NQ):
            t = rng.choice(self.terms, int(rng.integers(1, 7)), replace=False).astype(np.uint32)
            qt.append(t); qo.append(qo[-1] + t.size)
        self.q_terms, self.q_off = np.concatenate(qt), np.array(qo, np.uint32)

    def csr(self, lo, hi, base=0):
        """term-major CSR (terms, offsets, doc ids - base, tfs) of the documents [lo, hi)"""
        a, b = int(self.doc_off[lo]), int(self.doc_off[hi])
        o = np.argsort(self.hash[a:b], kind="stable")
        terms, counts = np.unique(self.hash[a:b][o], return_counts=True)
        off = np.zeros(terms.size + 1, np.uint64)
        off[1:] = np.cumsum(counts)
        return terms.astype(np.uint32), off, (self.doc[a:b][o] - np.uint32(base)).astype(np.uint32), self.tf[a:b][o]

    def update(self, ids, base=0):
        """document-major (doc ids - base, doc_offsets, term hashes, tfs) of the documents `ids` (ascending)"""
        th, tf, off = [], [], [0]
        for i in np.asarray(ids).tolist():
            a, b = int(self.doc_off[i]), int(self.doc_off[i + 1])
            th.append(self.hash[a:b]); tf.append(self.tf[a:b]); off.append(off[-1] + b - a)
        return ((np.asarray(ids, np.int64) - base).astype(np.uint32), np.array(off, np.uint64), np.concatenate(th).astype(np.uint32),
                np.concatenate(tf).astype(np.float32))

    def query(self, i):
        return self.q_terms[self.q_off[i]:self.q_off[i + 1]]


_cache = {}


def world():
    if "w" not in _cache:
        _cache["w"] = World()
    return _cache["w"]


def expected(csr, n_docs, q_terms, q_off, k):
    """oracle.bm25_search per query over ONE CSR -> [(ids, scores)]"""
    return [O.bm25_search(csr[0], csr[1], csr[2], csr[3], n_docs, q_terms[q_off[i]:q_off[i + 1]], k) for i in range(q_off.size - 1)]


def whole_expected(k):
    """the collection's answer to the world's 37 queries (computed once per k)"""
    if ("exp", k) not in _cache:
        w = world()
        _cache["exp", k] = expected(w.csr(0, N), N, w.q_terms, w.q_off, k)
    return _cache["exp", k]


def merge_lists(parts, k):
    """lists [(ids, scores)] -> one list by (score descending, larger id first), cut at k"""
    ids = np.concatenate([p[0] for p in parts]).astype(np.uint32)
    sc = np.concatenate([p[1] for p in parts]).astype(np.float32)
    o = np.lexsort((ids, sc.view(np.uint32)))[::-1][:k]       # scores are positive: their bits order like their values
    return ids[o], sc[o]


def per_shard_search_merged(bounds, k):
    """scheme A (wrong): every shard answers from its own statistics (idf of its own count and lists), the lists are merged"""
    w = world()
    out = []
    csrs = [w.csr(bounds[s], bounds[s + 1], bounds[s]) for s in range(len(bounds) - 1)]
    for i in range(NQ):
        parts = []
        for s, c in enumerate(csrs):
            ids, sc = O.bm25_search(c[0], c[1], c[2], c[3], bounds[s + 1] - bounds[s], w.query(i), k)
            parts.append((ids + np.uint32(bounds[s]), sc))
        out.append(merge_lists(parts, k))
    return out


def collection_idf_shard_buckets(bounds, k):
    """scheme B (wrong): the collection's idf, but every shard keeps its own 512 buckets (over its local ids) and cuts at k before the
    merge.  f32 arithmetic in the kernel's order: p0, + p1, ... over the query's sorted terms."""
    w = world()
    terms, off, docs, tfs = w.csr(0, N)
    out = []
    for i in range(NQ):
        score, touched = np.zeros(N, np.float32), np.zeros(N, bool)
        for h in np.sort(w.query(i)):
            j = int(np.searchsorted(terms, h))
            if j >= terms.size or terms[j] != h:
                continue
            lo, hi = int(off[j]), int(off[j + 1])
            p = tfs[lo:hi] * idf(N, hi - lo)
            d = docs[lo:hi]
            score[d] = np.where(touched[d], score[d] + p, p).astype(np.float32)
            touched[d] = True
        parts = []
        for s in range(len(bounds) - 1):
            g = np.flatnonzero(touched[bounds[s]:bounds[s + 1]]) + bounds[s]
            best = {}
            for d in g.tolist():                                   # ascending: a strictly greater score wins, the smallest id keeps a tie
                b = (d - bounds[s]) % 512
                if b not in best or score[d] > score[best[b]]:
                    best[b] = d
            ids = np.array(sorted(best.values()), np.uint32)
            parts.append(merge_lists([(ids, score[ids])], k))
        out.append(merge_lists(parts, k))
    return out


def n_differing(lists, exp):
    return sum(1 for (gi, gs), (ei, es) in zip(lists, exp)
               if not (np.array_equal(gi, ei) and np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(es, np.float32).view(np.uint32))))


def assert_preconditions():
    """the two inexact schemes do differ from the collection's answer on this corpus (issue: at least 30 and 20 of the 37 queries)"""
    if "pre" not in _cache:
        a = n_differing(per_shard_search_merged(BOUNDS3, 10), whole_expected(10))
        b = n_differing(collection_idf_shard_buckets(BOUNDS3, 60), whole_expected(60))
        _cache["pre"] = (a, b)
    a, b = _cache["pre"]
    assert a >= 30, f"per-shard search + merge differs for only {a} of {NQ} queries at top_k 10"
    assert b >= 20, f"collection idf + per-shard buckets differs for only {b} of {NQ} queries at top_k 60"
    return a, b


def assert_world_shape():
    """the three properties the 3-shard layout was chosen for"""
    w = world()
    t0, o0, _, _ = w.csr(BOUNDS3[0], BOUNDS3[1], BOUNDS3[0])
    assert BOUNDS3[1] > 8192 and int(np.diff(o0.astype(np.int64)).max()) > 256          # two tiles, the tile-directory path
    assert BOUNDS3[1] % 512 and BOUNDS3[2] % 512
    t1 = w.csr(BOUNDS3[1], BOUNDS3[2], BOUNDS3[1])[0]
    assert VOCAB - t1.size >= 40, t1.size                                                # the smallest shard lacks many terms


def same(got, exp_lists, what=""):
    """(ids [B][k], scores, counts) == [(ids, scores)] per query: counts, ids and score BITS; slots past the count are not compared"""
    ids, sc, cnt = got
    assert len(exp_lists) == ids.shape[0], what
    for i, (ei, es) in enumerate(exp_lists):
        c = int(cnt[i])
        assert c == ei.size, (what, i, c, ei.size)
        assert np.array_equal(ids[i, :c], ei), (what, i, ids[i, :c][:8], ei[:8])
        assert np.array_equal(sc[i, :c].view(np.uint32), np.asarray(es, np.float32).view(np.uint32)), (what, i)


def same_arrays(got, exp, what=""):
    """two (ids, scores, counts) results: counts, and ids / score bits up to the count"""
    assert np.array_equal(got[2], exp[2]), (what, got[2], exp[2])
    for i in range(got[0].shape[0]):
        c = int(got[2][i])
        assert np.array_equal(got[0][i, :c], exp[0][i, :c]), (what, i)
        assert np.array_equal(got[1][i, :c].view(np.uint32), exp[1][i, :c].view(np.uint32)), (what, i)


# ---- device-side helpers of both test files (they import cosdata_amd when called, so this module stays importable without a GPU) -------
def dense_stubs(bounds):
    """the set's dense shards: tiny graph-less indexes whose id_base is the shard's first document (the text calls never search them)"""
    import cosdata_amd as ca
    key = ("dense", tuple(bounds))
    if key not in _cache:
        X = np.random.default_rng(1).standard_normal((4, 8)).astype(np.float32)
        _cache[key] = [ca.HNSWIndex(8, ca.HNSWHyperParams(num_layers=3), id_base=int(b)).upload_vectors(X) for b in bounds[:-1]]
    return _cache[key]


def bm_shards(bounds):
    """fresh cos_bm25 handles, shard s = the documents [bounds[s], bounds[s + 1]) under local ids"""
    import cosdata_amd as ca
    w = world()
    return [ca.BM25Index(*w.csr(bounds[s], bounds[s + 1], bounds[s]), bounds[s + 1] - bounds[s]) for s in range(len(bounds) - 1)]


def whole_handle():
    import cosdata_amd as ca
    return ca.BM25Index(*world().csr(0, N), N)


def status(fn, *a):
    import cosdata_amd as ca
    try:
        fn(*a)
    except ca.CosdataError as e:
        return e.status
    return 0


def apply_updates(bm, whole, step):
    """step 0: 500 documents into the last shard (local ids), some with terms new to every shard; step 1: 300 documents of the middle
    shard and 50 of shard 0 deleted.  The whole-collection handle receives the same under global ids."""
    w = world()
    if step == 0:
        ids = np.arange(N, N + N_EXTRA)
        assert np.isin(w.update(ids)[2], w.new_terms).any()
        bm[2].insert(*w.update(ids, BOUNDS3[2]))
        whole.insert(*w.update(ids))
    else:
        rng = np.random.default_rng(3)
        mid = np.sort(rng.choice(np.arange(BOUNDS3[1], BOUNDS3[2]), 300, replace=False))
        first = np.sort(rng.choice(BOUNDS3[1], 50, replace=False))
        bm[1].delete(*w.update(mid, BOUNDS3[1])[:3])
        bm[0].delete(*w.update(first)[:3])
        whole.delete(*w.update(np.concatenate([first, mid]))[:3])


def update_queries():
    """the world's queries + some that name the new terms"""
    w = world()
    extra = [[int(w.new_terms[0])], [int(w.new_terms[3]), int(w.terms[5])], [int(w.new_terms[7]), int(w.new_terms[9]), int(w.terms[100])]]
    qt = np.concatenate([w.q_terms, np.array([t for q in extra for t in q], np.uint32)])
    qo = np.concatenate([w.q_off, w.q_off[-1] + np.cumsum([len(q) for q in extra])]).astype(np.uint32)
    return qt, qo
