"""Plain-Python model of a BM25 index that is updated in place, written from the reference source, and its pins.

    TFIDFIndex::insert                     src/indexes/tf_idf/mod.rs:85-110
    TFIDFIndex::mark_embedding_as_deleted  src/indexes/tf_idf/mod.rs:112-141
    VersionedVec::push_sorted / delete     src/models/versioned_vec.rs:205-222, :131-150 (the tombstone), iterator :251-275
    SparseAnnQueryBasic::search_bm25       src/models/sparse_ann_query.rs:149-233, get_idf :298-302

`oracle.bm25_search` takes a plain CSR and computes the idf from the list length it is given, so it cannot say what a search
over tombstones returns; `model_search` can: the posting iterator skips a tombstone (it adds nothing to any score), the idf of
a list uses its length INCLUDING tombstones and the decremented documents_count.  Head order as in tests/test_oracle_pybm25.py:
document id, then term hash, then query position; np.float32 arithmetic.  The GPU tests (tests/test_gpu_bm25_update.py)
hold the device to this model.  A query term whose list holds tombstones only contributes nothing."""
import bisect
import heapq

import numpy as np
import pytest

from oracle import oracle as O


class ModelIndex:
    """term hash -> [doc ids], [stored tfs], [tombstone flags], in list order; documents_count like TFIDFIndexRoot's"""

    def __init__(self, terms, offsets, docs, tfs, documents_count):
        self.lists = {}
        for i, t in enumerate(np.asarray(terms).tolist()):
            lo, hi = int(offsets[i]), int(offsets[i + 1])
            self.lists[int(t)] = (np.asarray(docs[lo:hi]).tolist(), [np.float32(x) for x in tfs[lo:hi]], [False] * (hi - lo))
        self.documents_count = int(documents_count)

    def insert(self, doc_ids, doc_offsets, term_hashes, tfs):
        for i, d in enumerate(np.asarray(doc_ids).tolist()):
            self.documents_count += 1                                   # mod.rs:91
            for j in range(int(doc_offsets[i]), int(doc_offsets[i + 1])):
                l = self.lists.setdefault(int(term_hashes[j]), ([], [], []))
                l[0].append(int(d)); l[1].append(np.float32(tfs[j])); l[2].append(False)   # push_sorted: ids only grow -> the end
        return self

    def delete(self, doc_ids, doc_offsets, term_hashes):
        for i, d in enumerate(np.asarray(doc_ids).tolist()):
            self.documents_count -= 1                                   # once per call, found or not (mod.rs:117-119)
            for j in range(int(doc_offsets[i]), int(doc_offsets[i + 1])):
                l = self.lists.get(int(term_hashes[j]))
                if l is None:
                    continue                                            # no list: left alone
                p = bisect.bisect_left(l[0], d)                         # ids ascend and are distinct inside a list: this IS the first entry with the id
                if p < len(l[0]) and l[0][p] == d and not l[2][p]:      # ... that still EQUALS it (a tombstone does not, versioned_vec.rs:141-150)
                    l[2][p] = True
        return self

    def csr(self):
        """-> terms, offsets, docs, tfs, tomb (tombstoned tfs reported as 0, like cos_bm25_download)"""
        terms = np.array(sorted(self.lists), np.uint32)
        offsets = np.zeros(terms.size + 1, np.uint64)
        docs, tfs, tomb = [], [], []
        for i, t in enumerate(terms.tolist()):
            l = self.lists[t]
            offsets[i + 1] = offsets[i] + np.uint64(len(l[0]))
            docs += l[0]; tomb += l[2]
            tfs += [np.float32(0) if dead else x for x, dead in zip(l[1], l[2])]
        return terms, offsets, np.array(docs, np.uint32), np.array(tfs, np.float32), np.array(tomb, bool)

    def search(self, q_terms, k):
        return model_search(self, q_terms, k)


def _next_live(l, cur):
    while cur < len(l[0]) and l[2][cur]:
        cur += 1                                                        # versioned_vec.rs:251-275: the iterator skips tombstones
    return cur


def model_search(ix: ModelIndex, q_terms, k):
    heads = []                                                          # (next doc id, term hash, entry order, cursor, idf)
    for order, th in enumerate(np.asarray(q_terms).tolist()):
        l = ix.lists.get(int(th))
        if l is None or not l[0]:
            continue
        idf = O.bm25_idf(ix.documents_count, len(l[0]))                 # get_idf(documents_count, documents.len()): tombstones count
        cur = _next_live(l, 0)
        if cur == len(l[0]):
            continue                                                    # tombstones only: contributes nothing
        heapq.heappush(heads, (l[0][cur], int(th), order, cur, idf))
    buckets = [(0xFFFFFFFF, np.float32(-np.inf))] * 512

    def advance(th, order, cur, idf):
        l = ix.lists[th]
        nxt = _next_live(l, cur + 1)
        if nxt < len(l[0]):
            heapq.heappush(heads, (l[0][nxt], th, order, nxt, idf))

    while heads:
        doc, th, order, cur, idf = heapq.heappop(heads)
        score = np.float32(ix.lists[th][1][cur]) * idf
        advance(th, order, cur, idf)
        while heads and heads[0][0] == doc:
            _, th2, o2, c2, idf2 = heapq.heappop(heads)
            score = np.float32(score + np.float32(ix.lists[th2][1][c2]) * idf2)
            advance(th2, o2, c2, idf2)
        b = doc % 512
        if score > buckets[b][1]:
            buckets[b] = (doc, score)
    res = [(s, d) for d, s in buckets if d != 0xFFFFFFFF]
    res.sort(key=lambda t: (float(t[0]), t[1]), reverse=True)
    res = res[:k]
    return np.array([d for _, d in res], np.uint32), np.array([s for s, _ in res], np.float32)


def _corpus(seed):
    """the generator of tests/test_oracle_pybm25.py (same seeds, same draws)"""
    rng = np.random.default_rng(seed)
    n_docs, T = int(rng.integers(600, 3000)), 120
    terms = np.sort(rng.choice(1 << 31, T, replace=False).astype(np.uint32))
    lens = np.minimum(rng.zipf(1.4, T) * 2, n_docs // 2).astype(np.int64)
    offsets = np.zeros(T + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    docs = np.concatenate([np.sort(rng.choice(n_docs, int(l), replace=False)) for l in lens]).astype(np.uint32)
    tfs = np.array([O.bm25_tf(int(c), int(dl), 120.0, 1.5, 0.75) for c, dl in
                    zip(rng.integers(1, 6, docs.size), rng.integers(40, 260, docs.size))], np.float32)
    return rng, n_docs, terms, offsets, docs, tfs


def _doc_terms(terms, offsets, docs, d):
    """the term hashes of document d (what the host gets from process_text of its text)"""
    out = []
    for i, t in enumerate(terms.tolist()):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        p = lo + int(np.searchsorted(docs[lo:hi], d))
        if p < hi and docs[p] == d:
            out.append(t)
    return np.array(out, np.uint32)


@pytest.mark.parametrize("seed", range(6))
def test_model_without_tombstones_equals_c_oracle(seed):
    rng, n_docs, terms, offsets, docs, tfs = _corpus(seed)
    ix = ModelIndex(terms, offsets, docs, tfs, n_docs)
    for _ in range(12):
        m = int(rng.integers(1, 9))
        q = rng.choice(terms, m, replace=True).astype(np.uint32)
        if rng.random() < 0.3:
            q[0] = 7
        for k in (1, 10, 30):
            pi, ps = ix.search(q, k)
            ci, cs = O.bm25_search(terms, offsets, docs, tfs, n_docs, q, k)
            assert np.array_equal(pi, ci), (q, k)
            assert np.array_equal(ps.view(np.uint32), cs.view(np.uint32)), (q, k)


@pytest.mark.parametrize("seed", range(3))
def test_model_insert_equals_c_oracle_on_the_merged_csr(seed):
    """an index grown document by document answers like the C oracle on the CSR of the whole corpus, and csr() is that CSR"""
    rng, n_docs, terms, offsets, docs, tfs = _corpus(seed)
    n0 = n_docs * 2 // 3
    keep = docs < n0
    off0 = np.zeros(terms.size + 1, np.uint64)
    off0[1:] = np.cumsum([int(keep[int(offsets[i]):int(offsets[i + 1])].sum()) for i in range(terms.size)])
    ix = ModelIndex(terms, off0, docs[keep], tfs[keep], n0)
    by_doc = {}
    for i, t in enumerate(terms.tolist()):
        for p in range(int(offsets[i]), int(offsets[i + 1])):
            if docs[p] >= n0:
                by_doc.setdefault(int(docs[p]), []).append((t, tfs[p]))
    ids = np.arange(n0, n_docs, dtype=np.uint32)
    doff = np.zeros(ids.size + 1, np.uint64)
    doff[1:] = np.cumsum([len(by_doc.get(int(d), [])) for d in ids])
    th = np.array([t for d in ids for t, _ in by_doc.get(int(d), [])], np.uint32)
    tf = np.array([f for d in ids for _, f in by_doc.get(int(d), [])], np.float32)
    ix.insert(ids, doff, th, tf)
    assert ix.documents_count == n_docs
    mt, mo, md, mf, mtomb = ix.csr()
    assert np.array_equal(mt, terms) and np.array_equal(mo, offsets) and np.array_equal(md, docs)
    assert np.array_equal(mf.view(np.uint32), tfs.view(np.uint32)) and not mtomb.any()
    for _ in range(8):
        q = rng.choice(terms, int(rng.integers(1, 9)), replace=True).astype(np.uint32)
        pi, ps = ix.search(q, 10)
        ci, cs = O.bm25_search(terms, offsets, docs, tfs, n_docs, q, 10)
        assert np.array_equal(pi, ci) and np.array_equal(ps.view(np.uint32), cs.view(np.uint32))


@pytest.mark.parametrize("seed", range(3))
def test_fully_deleted_document_is_never_returned(seed):
    rng, n_docs, terms, offsets, docs, tfs = _corpus(seed)
    ix = ModelIndex(terms, offsets, docs, tfs, n_docs)
    long_terms = terms[np.argsort(-np.diff(offsets.astype(np.int64)))[:6]]
    q = long_terms[:4]
    before, _ = ix.search(q, 30)
    victims = before[:5]
    dt = [_doc_terms(terms, offsets, docs, int(d)) for d in victims]
    doff = np.zeros(victims.size + 1, np.uint64)
    doff[1:] = np.cumsum([t.size for t in dt])
    ix.delete(victims, doff, np.concatenate(dt))
    assert ix.documents_count == n_docs - victims.size
    _, _, _, _, tomb = ix.csr()
    assert int(tomb.sum()) == int(doff[-1])
    for qq in (q, long_terms, terms[:40]):
        after, _ = ix.search(qq, 30)
        assert not np.isin(after, victims).any()
    # a second delete of the same documents marks nothing more, but counts again (the reference's behaviour)
    ix.delete(victims, doff, np.concatenate(dt))
    assert ix.documents_count == n_docs - 2 * victims.size and int(ix.csr()[4].sum()) == int(doff[-1])


def test_partly_deleted_document_scores_with_its_remaining_terms():
    terms = np.array([10, 20, 30], np.uint32)
    offsets = np.array([0, 3, 6, 8], np.uint64)
    docs = np.array([1, 5, 9, 1, 5, 7, 5, 9], np.uint32)
    tfs = np.array([0.5, 0.75, 1.0, 1.25, 1.5, 0.25, 2.0, 0.125], np.float32)
    ix = ModelIndex(terms, offsets, docs, tfs, 12)
    ix.delete([5], [0, 1], [20])                                      # delete called with a subset of document 5's terms
    assert ix.documents_count == 11
    ids, sc = ix.search(np.array([10, 20, 30], np.uint32), 10)
    idf = {t: O.bm25_idf(11, n) for t, n in ((10, 3), (20, 3), (30, 2))}   # lengths include the tombstone
    want5 = np.float32(np.float32(0.75) * idf[10] + np.float32(2.0) * idf[30])
    got = dict(zip(ids.tolist(), sc.tolist()))
    assert np.float32(got[5]).view(np.uint32) == want5.view(np.uint32)
    want1 = np.float32(np.float32(0.5) * idf[10] + np.float32(1.25) * idf[20])
    assert np.float32(got[1]).view(np.uint32) == want1.view(np.uint32)
    # a list that holds tombstones only contributes nothing; a term the index does not hold is left alone
    ix.delete([5, 9], [0, 1, 3], [30, 30, 99])
    assert ix.documents_count == 9
    ids2, _ = ix.search(np.array([30], np.uint32), 10)
    assert ids2.size == 0
    ids3, sc3 = ix.search(np.array([30, 10], np.uint32), 10)
    assert sorted(ids3.tolist()) == [1, 5, 9]
    assert np.float32(dict(zip(ids3.tolist(), sc3.tolist()))[5]).view(np.uint32) == np.float32(np.float32(0.75) * O.bm25_idf(9, 3)).view(np.uint32)
