"""postings_merge_kernel (csrc/postings_update.h) through its three posting formats — BM25Index.insert, InvertedIndex.insert in
the unpacked and in the packed layout — at the smallest shape that reaches every path of the kernel.

Three lists in key order, one insert:
  A  4090 + s old postings, 5 new ones     B  only in the update, 3 postings     C  6 old postings, 2 new ones
so the new array is  A old | A new | B | C old | C new  = 4106 + s postings in two 4096-posting pieces.  With s = 0 .. 4, A's
old/delta seam (4090 + s), the A/B boundary (4095 + s), the B/C boundary (4098 + s), C's seam (4104 + s) and the piece
boundary (4096) each land on every offset inside a thread's group of four, and the array ends on and off a multiple of four.

The expected arrays come from numpy (BM25) and cos_sparse_build_csr over all vectors (sparse), never from the device;
test_inputs_are_well_formed checks them without one."""
import numpy as np
import pytest

from tests.test_gpu_bm25_update import assert_download_equals, mismatches as bm25_mismatches, oracle_expected
from tests.test_gpu_sparse_update import UPPER, create, expected as sparse_expected, flat, mismatches as sparse_mismatches

N0, NEW = 13000, 5                     # ids before the insert, ids it brings: every list stays under (N0 + NEW) // 3 postings
KEYS = (1000, 2000, 3000)              # term hashes / dimensions of A, B, C
BITS = 6
S = range(5)


def shape(s):
    """per list (old ids, new ids), both strictly ascending, every new id above every old one"""
    rng = np.random.default_rng(70 + s)
    new = N0 + np.arange(NEW, dtype=np.uint32)
    pick = lambda k: np.sort(rng.choice(N0, k, replace=False)).astype(np.uint32)
    return [(pick(4090 + s), new), (np.zeros(0, np.uint32), new[1:4]), (pick(6), new[[0, 4]])]


def by_id(s):
    """the postings of all three lists as (id, key) in id-major order (keys ascending inside an id) + where each id starts"""
    lists = shape(s)
    ids = np.concatenate([np.concatenate(l) for l in lists])
    keys = np.concatenate([np.full(l[0].size + l[1].size, k, np.uint32) for k, l in zip(KEYS, lists)])
    o = np.lexsort((keys, ids))
    ids, keys = ids[o], keys[o]
    return ids, keys, np.searchsorted(ids, np.arange(N0 + NEW + 1)).astype(np.uint64)


def bm25_inputs(s):
    """(base CSR of the documents < N0, update of the documents >= N0, merged CSR of all of them), the merged one list by list"""
    tf_of = lambda d, k: (0.25 + ((d.astype(np.uint64) * 7 + k) % 13).astype(np.float32) / 8).astype(np.float32)

    def csr(part):                     # part 0: old postings only, part 1: old then new
        rows = [(k, np.concatenate(l[:part + 1])) for k, l in zip(KEYS, shape(s))]
        rows = [(k, d) for k, d in rows if d.size]
        off = np.cumsum([0] + [d.size for _, d in rows]).astype(np.uint64)
        return (np.array([k for k, _ in rows], np.uint32), off, np.concatenate([d for _, d in rows]),
                np.concatenate([tf_of(d, k) for k, d in rows]))

    ids, keys, start = by_id(s)
    a = int(start[N0])
    update = (np.arange(N0, N0 + NEW, dtype=np.uint32), start[N0:] - start[N0], keys[a:], tf_of(ids[a:], keys[a:]))
    return csr(0), update, csr(1)


def sparse_rows(s, lo, hi):
    """the raw vectors [lo, hi) as (row_offsets, dims, values); the values spread over every key of 6 bits and past the upper bound"""
    ids, keys, start = by_id(s)
    a, b = int(start[lo]), int(start[hi])
    vals = (0.05 + ((ids[a:b].astype(np.uint64) * 7 + keys[a:b]) % 61).astype(np.float32) / 20).astype(np.float32)
    return start[lo:hi + 1] - start[lo], keys[a:b], vals


@pytest.mark.parametrize("s", S)
def test_inputs_are_well_formed(s):
    import cosdata_amd as ca
    want = [(4090 + s, 5), (0, 3), (6, 2)]
    for (old, new), (n_old, n_new) in zip(shape(s), want):
        assert (old.size, new.size) == (n_old, n_new)
        assert np.all(np.diff(old.astype(np.int64)) > 0) and np.all(np.diff(new.astype(np.int64)) > 0)
        assert old.size == 0 or int(new.min()) > int(old.max())
        assert old.size + new.size <= (N0 + NEW) // 3
    bounds = [0, 4095 + s, 4098 + s, 4106 + s]
    base, update, merged = bm25_inputs(s)
    assert base[0].tolist() == [KEYS[0], KEYS[2]] and base[1].tolist() == [0, 4090 + s, 4096 + s]
    assert merged[0].tolist() == list(KEYS) and merged[1].tolist() == bounds
    assert update[1].tolist() == [0, 2, 4, 6, 8, 10] and update[2].size == update[3].size == 10
    for t in range(3):                                                  # ids strictly ascending inside every merged list
        assert np.all(np.diff(merged[2][bounds[t]:bounds[t + 1]].astype(np.int64)) > 0)
    assert np.isfinite(merged[3]).all() and np.unique(merged[3]).size == 13
    w = (1 << BITS) + 1
    dims, ko, ids = ca.sparse_build_csr(BITS, UPPER, *sparse_rows(s, 0, N0 + NEW))
    assert dims.tolist() == list(KEYS) and ko[::w].tolist() == bounds[:3] and ko[w - 1::w].tolist() == bounds[1:] and ids.size == bounds[3]
    assert (np.diff(ko.reshape(3, w)[0]) > 0).sum() > 32             # A's postings spread over most of the 64 keys
    dims0, ko0, _ = ca.sparse_build_csr(BITS, UPPER, *sparse_rows(s, 0, N0))
    assert dims0.tolist() == [KEYS[0], KEYS[2]] and ko0[w - 1::w].tolist() == [4090 + s, 4096 + s]


@pytest.mark.gpu
@pytest.mark.parametrize("s", S)
def test_bm25_merge(s):
    import cosdata_amd as ca
    base, update, merged = bm25_inputs(s)
    bm = ca.BM25Index(*base, N0)
    bm.insert(*update)
    assert_download_equals(bm, merged)
    fresh = ca.BM25Index(*merged, N0 + NEW)
    sa, sb = bm.stats(), fresh.stats()
    for key in ("documents_count", "n_terms", "postings", "tombstones", "dir_rows", "dir_tiles"):
        assert sa[key] == sb[key], (key, sa, sb)
    assert sa["postings"] == 4106 + s and sa["dir_rows"] == 1
    fresh.close()
    qt, qo = np.array(KEYS, np.uint32), np.arange(4, dtype=np.uint32)  # one query per list
    exp = oracle_expected(merged, N0 + NEW, qt, qo, 20)
    assert all(e[0].size > 0 for e in exp)
    assert bm25_mismatches(bm.search_batch(qt, qo, 20), exp, f"s={s}") == 0
    bm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("s", S)
def test_sparse_merge(s, layout):
    import cosdata_amd as ca
    n = N0 + NEW
    csr0 = ca.sparse_build_csr(BITS, UPPER, *sparse_rows(s, 0, N0))
    csr = ca.sparse_build_csr(BITS, UPPER, *sparse_rows(s, 0, n))
    ix = create(layout, BITS, csr0, N0)
    assert ix.insert(*sparse_rows(s, N0, n)) == N0
    dl = ix.download()
    assert np.array_equal(dl[0], csr[0]) and np.array_equal(dl[1], csr[1]) and np.array_equal(dl[2], csr[2])
    fresh = create(layout, BITS, csr, n)
    sa, sb = ix.stats(), fresh.stats()
    for key in ("n_vectors", "n_dims", "postings", "dir_rows", "dir_tiles", "packed", "have_raw", "raw_pairs"):
        assert sa[key] == sb[key], (key, sa, sb)
    assert sa["postings"] == 4106 + s and sa["dir_rows"] == 1 and sa["packed"] == layout
    fresh.close()
    qs = [(np.array([k], np.uint32), np.array([1.5], np.float32)) for k in KEYS]  # one query per list
    exp = sparse_expected(csr, n, BITS, 0.0, qs, 20, 0, None)
    assert all(len(e[0]) > 0 for e in exp)
    assert sparse_mismatches(ix.search_batch(*flat(qs), 20, 0.0, 0), exp, f"s={s} layout={layout}") == 0
    ix.close()
