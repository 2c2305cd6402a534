"""Insert / delete on the learned-sparse inverted index: a plain-Python model written from the reference, and what pins it.

    InvertedIndexNode::insert   models/inverted_index.rs:176-201   every (dim, value) pair pushes the id to the END of the list of
                                                                   (dim, quantize(value)); a dimension never seen gets a node
    InvertedIndexNode::delete   models/inverted_index.rs:205-222   look ONLY in the list of (dim, quantize(value)) ...
    VersionedVec::delete        models/versioned_vec.rs:131-154    ... and turn the FIRST entry that equals the id into a tombstone
    VersionedVec::iter          models/versioned_vec.rs:251-275    readers skip tombstones: a deleted posting is an absent one

The model keeps `dim -> [list per key]`; a delete removes the entry (nothing else of a list enters a score, so that is the
tombstone's whole effect).  Search = tests/test_sparse.py::_py_sequential_search over the lists.  tests/test_gpu_sparse_update.py
holds the device to this model; the tests here hold the model to cos_sparse_build_csr and to the C oracle, and check the
argument handling of the new entry points that needs no device."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_sparse import _py_sequential_search


def np_quantize(vals, upper, bits):
    """InvertedIndexNode::quantize on an array (pinned against the oracle's scalar below)"""
    one_q = np.float32((1 << bits) - 1)
    with np.errstate(all="ignore"):
        t = (np.asarray(vals, np.float32) / np.float32(upper)) * one_q
        t = np.where(t < 0, np.float32(0), np.where(t > one_q, one_q, t))        # f32::clamp keeps NaN
        q = np.where(np.isnan(t) | (t <= 0), 0, np.minimum(t, np.float32(255.0))).astype(np.int64)   # `as u8`
    return np.minimum(q, (1 << bits) - 1).astype(np.int64)


class SparseModel:
    """InvertedIndexRoot as dim -> [list of ids per key]; ids are handed out sequentially"""

    def __init__(self, bits, upper, n=0):
        self.bits, self.upper, self.Q, self.n = bits, float(upper), 1 << bits, n
        self.lists = {}

    @classmethod
    def from_csr(cls, bits, upper, dims, key_off, vec_ids, n):
        m = cls(bits, upper, n)
        w = m.Q + 1
        for t, d in enumerate(np.asarray(dims).tolist()):
            m.lists[d] = [np.asarray(vec_ids[int(key_off[t * w + k]):int(key_off[t * w + k + 1])]).tolist() for k in range(m.Q)]
        return m

    def insert(self, row_off, dims, vals):
        first = self.n
        keys = np_quantize(vals, self.upper, self.bits).tolist()
        dims = np.asarray(dims).tolist()
        for i in range(len(row_off) - 1):
            for p in range(int(row_off[i]), int(row_off[i + 1])):      # every pair, zero values included
                self.lists.setdefault(dims[p], [[] for _ in range(self.Q)])[keys[p]].append(self.n)
            self.n += 1
        return first

    def delete(self, ids, row_off, dims, vals):
        removed = 0
        keys = np_quantize(vals, self.upper, self.bits).tolist()
        dims = np.asarray(dims).tolist()
        for i, v in enumerate(np.asarray(ids).tolist()):
            for p in range(int(row_off[i]), int(row_off[i + 1])):
                node = self.lists.get(dims[p])
                if node is None:
                    continue                                           # no node for the dimension: nothing happens
                lst = node[keys[p]]                                    # ONLY the list of the quantized value
                if v in lst:
                    lst.remove(v)                                      # the first entry that equals the id
                    removed += 1
        return removed

    def csr(self):
        dims = np.array(sorted(self.lists), np.uint32)
        ko, ids = [], []
        for d in dims.tolist():
            for k in range(self.Q):
                ko.append(len(ids))
                ids += self.lists[d][k]
            ko.append(len(ids))
        return dims, np.array(ko, np.uint64), np.array(ids, np.uint32)

    def postings(self):
        return sum(len(l) for node in self.lists.values() for l in node)

    def longest(self, count=5):
        """the `count` dimensions with the longest lists that still hold a posting"""
        lens = sorted(((sum(len(l) for l in node), d) for d, node in self.lists.items()), reverse=True)
        return [d for ln, d in lens[:count] if ln > 0]

    def search(self, q_dims, q_vals, thr, limit=0):
        """sequential_search -> (ids, similarities), similarity descending, larger id first"""
        dots = _py_sequential_search(self.lists, self.bits, self.upper, thr, (np.asarray(q_dims), np.asarray(q_vals)))
        order = sorted(dots.items(), key=lambda kv: (-kv[1], -kv[0]))
        if limit:
            order = order[:limit]
        return np.array([v for v, _ in order], np.uint32), np.array([s for _, s in order], np.uint32)


def vectors(n, vocab, nnz, seed, lo_vocab=None, lo_until=0):
    """sparse vectors of tests/test_sparse.py::_corpus's kind as a raw CSR: 4 .. nnz-1 ascending dimensions per vector, values
    gamma(1.2, 0.7), a twentieth of them times 5 (above the upper bound 3.0).  Vectors below `lo_until` draw from the first
    `lo_vocab` dimensions only, so that later ones bring dimensions an index of the first part does not have."""
    rng = np.random.default_rng(seed)
    ds, xs, off = [], [], [0]
    for v in range(n):
        voc = lo_vocab if (lo_vocab and v < lo_until) else vocab
        d = np.sort(rng.choice(voc, size=int(rng.integers(4, nnz)), replace=False)).astype(np.uint32)
        x = rng.gamma(1.2, 0.7, d.size).astype(np.float32)
        x[rng.random(d.size) < 0.05] *= 5.0
        ds.append(d); xs.append(x); off.append(off[-1] + d.size)
    return np.array(off, np.uint64), np.concatenate(ds), np.concatenate(xs)


def rows_of(raw, ids):
    """(row_offsets, dims, vals) of the vectors `ids` of a raw CSR"""
    ro, rd, rv = raw
    ids = np.asarray(ids, np.int64)
    if ids.size == 0:
        return np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32)
    sel = np.concatenate([np.arange(int(ro[i]), int(ro[i + 1])) for i in ids]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum([int(ro[i + 1]) - int(ro[i]) for i in ids])]).astype(np.uint64)
    return off, rd[sel], rv[sel]


def queries(model, nq, vocab, seed):
    """each query: one of the five longest lists that still hold a posting + up to 9 other dimensions (some unknown), values
    gamma(1.5, 0.8), a tenth of them tiny (quantize to 0); the heavy dimension gets a value that does not quantize to 0"""
    rng = np.random.default_rng(seed)
    heavy = model.longest()
    out = []
    for _ in range(nq):
        h = int(rng.choice(heavy))
        others = [int(d) for d in rng.choice(vocab + 20, size=int(rng.integers(1, 10)), replace=False) if int(d) != h]
        d = np.array([h] + others, np.uint32)
        x = rng.gamma(1.5, 0.8, d.size).astype(np.float32)
        x[rng.random(d.size) < 0.1] = 0.01
        x[0] = max(float(x[0]), 0.5)
        o = rng.permutation(d.size)
        out.append((d[o], x[o]))
    return out


def drop_from_csr(bits, dims, key_off, vec_ids, pairs):
    """the CSR without the postings `pairs` = [(id, dim, key)] name — written on the arrays, independently of the model: per pair
    the first position of the id inside the (dim, key) list that an earlier pair has not taken"""
    w = (1 << bits) + 1
    ko = np.asarray(key_off).reshape(len(dims), w).astype(np.int64)
    keep = np.ones(len(vec_ids), bool)
    pos_of = {int(d): t for t, d in enumerate(dims)}
    for v, d, k in pairs:
        t = pos_of.get(int(d))
        if t is None:
            continue
        lo, hi = ko[t, k], ko[t, k + 1]
        hit = np.nonzero((vec_ids[lo:hi] == v) & keep[lo:hi])[0]
        if hit.size:
            keep[lo + hit[0]] = False
    gone = np.concatenate([[0], np.cumsum(~keep)])
    return dims, (ko - gone[ko]).ravel().astype(np.uint64), vec_ids[keep]


def test_numpy_quantizer_is_the_oracles():
    vals = np.array([0.0, -1.0, 3.0, 2.9999, 1e30, np.nan, 1e-30, 1.49, 0.7, np.inf, -np.inf, 2.0], np.float32)
    for bits in (1, 4, 6, 8):
        for upper in (3.0, 2.5, 2.0):
            assert np_quantize(vals, upper, bits).tolist() == [O.sparse_quantize(v, upper, bits) for v in vals]


@pytest.mark.parametrize("bits", [4, 6, 8])
def test_model_after_inserts_is_the_csr_of_the_union(bits):
    import cosdata_amd as ca
    raw = vectors(1500, 300, 24, seed=bits, lo_vocab=280, lo_until=900)
    m = SparseModel(bits, 3.0)
    cur = 0
    for step in (900, 1, 7, 592):
        assert m.insert(*rows_of(raw, range(cur, cur + step))) == cur
        cur += step
        d, ko, ids = ca.sparse_build_csr(bits, 3.0, *rows_of(raw, range(cur)))
        md, mko, mids = m.csr()
        assert np.array_equal(md, d) and np.array_equal(mko, ko) and np.array_equal(mids, ids)
    assert m.n == 1500 and m.postings() == int(raw[0][-1])


@pytest.mark.parametrize("bits,thr", [(4, 0.5), (6, 0.0), (8, 0.3), (6, 0.75)])
def test_model_after_deletes_is_the_oracle_on_the_csr_without_those_postings(bits, thr):
    import cosdata_amd as ca
    n, vocab = 3000, 400
    raw = vectors(n, vocab, 24, seed=10 + bits)
    d, ko, ids = ca.sparse_build_csr(bits, 3.0, *raw)
    m = SparseModel.from_csr(bits, 3.0, d, ko, ids, n)
    rng = np.random.default_rng(bits)
    dele = np.sort(rng.choice(n, n // 4, replace=False))
    args = rows_of(raw, dele)
    pairs = [(int(dele[i]), int(args[1][p]), int(k)) for i in range(dele.size) for p, k in
             zip(range(int(args[0][i]), int(args[0][i + 1])), np_quantize(args[2][int(args[0][i]):int(args[0][i + 1])], 3.0, bits))]
    removed = m.delete(dele, *args)
    assert removed == int(args[0][-1]) == len(pairs)
    want = drop_from_csr(bits, d, ko, ids, pairs)
    got = m.csr()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert m.delete(dele, *args) == 0                                   # the second delete finds nothing
    assert all(np.array_equal(a, b) for a, b in zip(m.csr(), want))
    for q in queries(m, 24, vocab, seed=bits + 1):
        oi, os_ = O.sparse_search(want[0], want[1], want[2], n, bits, 3.0, thr, q[0], q[1])
        mi, ms = m.search(q[0], q[1], thr)
        assert oi.size > 0                                               # a heavy dimension: never an empty answer
        assert np.array_equal(mi, oi) and np.array_equal(ms, os_)
        assert not np.isin(oi, dele).any()                               # every pair of a deleted vector was handed in


def test_wrong_value_second_delete_unknown_dimension_and_repeated_dimension():
    bits, upper = 6, 3.0
    m = SparseModel(bits, upper)
    ro = np.array([0, 3, 5, 8], np.uint64)
    dims = np.array([5, 9, 11, 5, 9, 7, 7, 7], np.uint32)                # vector 2 names dimension 7 three times
    vals = np.array([1.0, 2.0, 0.0, 1.0, 2.9, 0.5, 0.5, 1.5], np.float32)
    assert m.insert(ro, dims, vals) == 0 and m.n == 3
    k = lambda x: int(np_quantize([x], upper, bits)[0])
    assert m.lists[5][k(1.0)] == [0, 1] and m.lists[11][0] == [0]        # a zero value is inserted too (key 0)
    assert m.lists[7][k(0.5)] == [2, 2] and m.lists[7][k(1.5)] == [2]    # pushed once per pair
    one = np.array([0, 1], np.uint64)
    # a value that quantizes to another key than the stored one: nothing happens
    assert k(1.2) != k(1.0)
    assert m.delete([0], one, [5], [1.2]) == 0 and m.lists[5][k(1.0)] == [0, 1]
    # unknown dimension, id the index never held: nothing happens, no error
    assert m.delete([0], one, [1234], [1.0]) == 0
    assert m.delete([77], one, [5], [1.0]) == 0
    # the right value: the first entry that equals the id; again: nothing
    assert m.delete([0], one, [5], [1.0]) == 1 and m.lists[5][k(1.0)] == [1]
    assert m.delete([0], one, [5], [1.0]) == 0
    # k pairs naming the same (id, dim, key) remove k postings; the other key's posting stays
    assert m.delete([2], np.array([0, 1], np.uint64), [7], [0.5]) == 1 and m.lists[7][k(0.5)] == [2]
    assert m.insert(np.array([0, 2], np.uint64), [7, 7], [0.5, 0.5]) == 3 and m.lists[7][k(0.5)] == [2, 3, 3]
    assert m.delete([3], np.array([0, 3], np.uint64), [7, 7, 7], [0.5, 0.5, 0.5]) == 2 and m.lists[7][k(0.5)] == [2]
    # a dimension whose lists are all empty stays in the table and answers nothing; an insert revives it
    assert m.delete([0], one, [11], [0.0]) == 1
    assert 11 in m.csr()[0].tolist() and m.search([11], [1.0], 0.0)[0].size == 0
    assert m.insert(one, [11], [2.0]) == 4 and m.search([11], [1.0], 0.0)[0].tolist() == [4]
    # the search over a repeated dimension adds once per posting
    ids, sims = m.search([7], [3.0], 0.0)
    assert ids.tolist() == [2] and sims.tolist() == [63 * k(0.5) + 63 * k(1.5)]


def test_entry_points_check_their_arguments_without_a_device():
    from cosdata_amd import _lib
    L = _lib.lib()
    ro = (C.c_uint64 * 2)(0, 1)
    d, v, i = (C.c_uint32 * 1)(3), (C.c_float * 1)(1.0), (C.c_uint32 * 1)(0)
    assert L.cos_sparse_insert(None, 1, ro, d, v, None) == _lib.ERR_INVALID
    assert L.cos_sparse_delete(None, i, ro, 1, d, v, None) == _lib.ERR_INVALID
    st = _lib.CosSparseIndexStats()
    st.struct_size = C.sizeof(_lib.CosSparseIndexStats) - 8
    assert L.cos_sparse_stats(None, C.byref(st)) == _lib.ERR_INVALID
    nt, nnz = C.c_uint32(0), C.c_uint64(0)
    assert L.cos_sparse_download(None, C.byref(nt), C.byref(nnz), None, None, None) == _lib.ERR_INVALID
    assert C.sizeof(_lib.CosSparseIndexStats) == 64
