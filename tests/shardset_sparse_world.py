"""The learned-sparse collection of the shard-set tests (test_shardset_sparse_model.py, test_gpu_shardset_sparse.py,
test_gpu_shardset_mixed.py): the corpus and queries of tests/test_sparse.py cut into id-range shards, the whole collection's expected
answers from the oracle, a numpy model of the exact scheme (per-shard candidate records + fold) and a CPU restatement
of the scheme that is NOT exact (per-shard rerank + merge) — asserted to differ from the expected answer before anything runs on the
device, so that the tests cannot pass on a scheme that is wrong.

Importable without a GPU.  The corpus gives tied groups at the cut that hold ids of two shards as it stands (assert_preconditions
counts them), so no row had to be copied between shards."""
import functools

import numpy as np

from oracle import oracle as O
from tests.test_sparse import _corpus, _queries

N, VOCAB, NQ, UPPER = 6000, 300, 40, 3.0
BOUNDS3 = [0, 1000, 4200, 6000]
BOUNDS8 = [750 * s for s in range(9)]
CONFIGS = [(6, 0.0), (4, 0.5), (8, 0.3)]            # (quantization_bits, early_terminate_threshold)


def quantize(vals, upper, bits):
    """InvertedIndexNode::quantize over an array: (((value / upper) * max).clamp(0, max) as u8).min(max), f32 arithmetic"""
    mx = np.float32((1 << bits) - 1)
    with np.errstate(invalid="ignore"):
        x = np.asarray(vals, np.float32) / np.float32(upper) * mx
    x = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), mx))
    return x.astype(np.uint8).astype(np.uint32)


def build_csr(row_off, raw_dims, raw_vals, bits, upper):
    """cos_sparse_build_csr in numpy: (dims, key_offsets [T][2^bits + 1], vec_ids), the ids of a (dimension, key) list in id order"""
    Q = 1 << bits
    n = row_off.size - 1
    vec = np.repeat(np.arange(n, dtype=np.uint32), np.diff(row_off).astype(np.int64))
    dims, t = np.unique(raw_dims, return_inverse=True)
    slot = t.astype(np.int64) * Q + quantize(raw_vals, upper, bits)
    order = np.argsort(slot, kind="stable")           # stable: id order inside a list
    counts = np.bincount(slot, minlength=dims.size * Q).reshape(dims.size, Q)
    ko = np.zeros((dims.size, Q + 1), np.uint64)
    ko[:, 1:] = np.cumsum(counts, axis=1)
    ko += np.concatenate([[0], np.cumsum(counts.sum(axis=1))[:-1]]).astype(np.uint64)[:, None]
    return dims.astype(np.uint32), ko.ravel(), vec[order]


def simkey(x):
    """device simkey(): the u32 whose unsigned order is f32 total_cmp"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b >> 31, b ^ 0xFFFFFFFF, b ^ 0x80000000).astype(np.uint64)


class Shard:
    def __init__(self, world, lo, hi, bits):
        self.lo, self.hi, self.n = lo, hi, hi - lo
        a, b = int(world.row_off[lo]), int(world.row_off[hi])
        self.row_off = (world.row_off[lo:hi + 1] - world.row_off[lo]).astype(np.uint64)
        self.raw_dims, self.raw_vals = world.raw_dims[a:b], world.raw_vals[a:b]
        self.dims, self.key_off, self.vec_ids = build_csr(self.row_off, self.raw_dims, self.raw_vals, bits, UPPER)


class World:
    """one quantization of the corpus: the whole collection's CSR and the shards of both layouts under local ids"""

    def __init__(self, bits, raw=None, queries=None):
        """raw = (row_off, raw_dims, raw_vals): another collection than the corpus (after updates, or built for one edge case)"""
        self.bits = bits
        if raw is None:
            _, self.dims, self.key_off, self.vec_ids, self.row_off, self.raw_dims, self.raw_vals = _corpus(n=N, vocab=VOCAB, bits=bits, upper=UPPER, seed=7)
            d, ko, vi = build_csr(self.row_off, self.raw_dims, self.raw_vals, bits, UPPER)   # the numpy builder against test_sparse's own
            assert np.array_equal(d, self.dims) and np.array_equal(ko, self.key_off) and np.array_equal(vi, self.vec_ids)
        else:
            self.row_off, self.raw_dims, self.raw_vals = (np.asarray(raw[0], np.uint64), np.asarray(raw[1], np.uint32), np.asarray(raw[2], np.float32))
            self.dims, self.key_off, self.vec_ids = build_csr(self.row_off, self.raw_dims, self.raw_vals, bits, UPPER)
        self.n = self.row_off.size - 1
        self.queries = _queries(NQ, VOCAB, seed=3) if queries is None else queries
        self._shards = {}

    def rows_csr(self, ids):
        """(row_offsets, raw_dims, raw_vals) of the vectors `ids`, in that order"""
        parts = [(int(self.row_off[i]), int(self.row_off[i + 1])) for i in np.asarray(ids).tolist()]
        off = np.cumsum([0] + [b - a for a, b in parts]).astype(np.uint64)
        return off, np.concatenate([self.raw_dims[a:b] for a, b in parts]), np.concatenate([self.raw_vals[a:b] for a, b in parts])

    def shards(self, bounds):
        key = tuple(bounds)
        if key not in self._shards:
            self._shards[key] = [Shard(self, lo, hi, self.bits) for lo, hi in zip(bounds[:-1], bounds[1:])]
        return self._shards[key]

    def query_csr(self, queries=None):
        qs = self.queries if queries is None else queries
        qo = np.cumsum([0] + [len(d) for d, _ in qs]).astype(np.uint32)
        qd = np.concatenate([np.asarray(d, np.uint32) for d, _ in qs]) if qo[-1] else np.zeros(0, np.uint32)
        qv = np.concatenate([np.asarray(x, np.float32) for _, x in qs]) if qo[-1] else np.zeros(0, np.float32)
        return qd, qv, qo

    # ---- the whole collection: what every scheme is held to ----
    def touched(self, thr, q):
        """every touched vector, (ids, similarities) by similarity descending, larger id first"""
        return O.sparse_search(self.dims, self.key_off, self.vec_ids, self.n, self.bits, UPPER, thr, q[0], q[1])

    def expected(self, thr, q, top_k, factor):
        C = top_k * max(factor, 1)
        ids, sims = O.sparse_search(self.dims, self.key_off, self.vec_ids, self.n, self.bits, UPPER, thr, q[0], q[1], k_with_reranking=C)
        if not factor:
            return ids[:top_k].astype(np.uint32), sims[:top_k].astype(np.float32)
        return O.sparse_rerank(self.row_off, self.raw_dims, self.raw_vals, ids, q[0], q[1], top_k=top_k)

    # ---- per shard ----
    def shard_candidates(self, sh, thr, q, C, rerank):
        """the shard's record of one query: (quantized keys u64 under global ids, raw score keys u32 or None), best C"""
        ids, sims = O.sparse_search(sh.dims, sh.key_off, sh.vec_ids, sh.n, self.bits, UPPER, thr, q[0], q[1], k_with_reranking=C)
        keys = (sims.astype(np.uint64) + 1) << np.uint64(32) | (ids.astype(np.uint64) + np.uint64(sh.lo))
        if not rerank:
            return keys, None
        rid, rsc = O.sparse_rerank(sh.row_off, sh.raw_dims, sh.raw_vals, ids, q[0], q[1], top_k=0)
        score = dict(zip(rid.tolist(), simkey(rsc).tolist()))
        return keys, np.array([score[i] for i in ids.tolist()], np.uint64)

    def model(self, bounds, thr, q, top_k, factor):
        """record + fold: the S x C gathered keys cut to the best C by the quantized key, those sorted by the raw key, cut to top_k"""
        C = top_k * max(factor, 1)
        recs = [self.shard_candidates(sh, thr, q, C, factor != 0) for sh in self.shards(bounds)]
        keys = np.concatenate([k for k, _ in recs])
        order = np.argsort(keys)[::-1][:C]
        if not factor:
            best = keys[order][:top_k]
            return (best & np.uint64(0xFFFFFFFF)).astype(np.uint32), ((best >> np.uint64(32)) - np.uint64(1)).astype(np.float32)
        raw = np.concatenate([r for _, r in recs])[order] << np.uint64(32) | (keys[order] & np.uint64(0xFFFFFFFF))
        raw = np.sort(raw)[::-1][:top_k]
        hi = (raw >> np.uint64(32)).astype(np.uint32)
        bits = np.where(hi & np.uint32(0x80000000), hi ^ np.uint32(0x80000000), ~hi)
        return (raw & np.uint64(0xFFFFFFFF)).astype(np.uint32), bits.astype(np.uint32).view(np.float32)

    def wrong_scheme(self, bounds, thr, q, top_k, factor):
        """NOT exact: every shard searches and reranks its own candidates, the lists are merged (score descending, larger id first)"""
        C = top_k * max(factor, 1)
        out = []
        for sh in self.shards(bounds):
            ids, sims = O.sparse_search(sh.dims, sh.key_off, sh.vec_ids, sh.n, self.bits, UPPER, thr, q[0], q[1], k_with_reranking=C)
            if factor:
                ids, sc = O.sparse_rerank(sh.row_off, sh.raw_dims, sh.raw_vals, ids, q[0], q[1], top_k=top_k)
            else:
                ids, sc = ids[:top_k], sims[:top_k].astype(np.float32)
            out.append(simkey(sc) << np.uint64(32) | (ids.astype(np.uint64) + np.uint64(sh.lo)))
        keys = np.sort(np.concatenate(out))[::-1][:top_k]
        hi = (keys >> np.uint64(32)).astype(np.uint32)
        bits = np.where(hi & np.uint32(0x80000000), hi ^ np.uint32(0x80000000), ~hi)
        return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), bits.astype(np.uint32).view(np.float32)

    def differing(self, scheme, bounds, thr, top_k, factor):
        """queries on which `scheme` differs from the whole collection's answer in ids or score bits"""
        n = 0
        for q in self.queries:
            ei, es = self.expected(thr, q, top_k, factor)
            gi, gs = scheme(bounds, thr, q, top_k, factor)
            n += not (np.array_equal(ei, gi) and np.array_equal(np.asarray(es, np.float32).view(np.uint32), np.asarray(gs, np.float32).view(np.uint32)))
        return n


@functools.lru_cache(maxsize=None)
def world(bits):
    return World(bits)


def cut_statistics(w, bounds, thr, C):
    """(queries whose cut at C falls inside a group of equal similarities, ... whose tied group holds ids of two shards,
    queries with fewer than C candidates in the whole collection)"""
    tied = two = short = 0
    edges = np.asarray(bounds[1:-1])
    for q in w.queries:
        ids, sims = w.touched(thr, q)
        if ids.size < C:
            short += 1
        if ids.size > C and sims[C - 1] == sims[C]:
            tied += 1
            group = ids[sims == sims[C - 1]]
            two += np.unique(np.searchsorted(edges, group, side="right")).size >= 2
    return tied, two, short


def assert_preconditions():
    """the GPU tests call this first: the wrong scheme is visibly wrong on this corpus, and the two-key order at the cut is exercised"""
    w = world(6)
    wrong = w.differing(w.wrong_scheme, BOUNDS3, 0.0, 10, 5)
    assert wrong >= 20, wrong                              # 24 measured
    tied, two, _ = cut_statistics(w, BOUNDS3, 0.0, 50)
    assert tied >= 15, tied                                # 19 measured
    assert two >= 1, two


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


# ---- device-side helpers (they import cosdata_amd when called, so this module stays importable without a GPU) --------------------------
def sparse_shards(w, bounds, keep_raw=True, layout=None):
    """fresh cos_sparse handles, shard s = the vectors [bounds[s], bounds[s + 1]) under local ids"""
    import cosdata_amd as ca
    from cosdata_amd import _lib
    out = []
    for sh in w.shards(bounds):
        if layout is None:
            out.append(ca.InvertedIndex.from_vectors(w.bits, UPPER, sh.row_off, sh.raw_dims, sh.raw_vals, keep_raw=keep_raw))
        else:
            with _lib.tuning(sparse_layout=layout):
                out.append(ca.InvertedIndex.from_vectors(w.bits, UPPER, sh.row_off, sh.raw_dims, sh.raw_vals, keep_raw=keep_raw))
            assert out[-1].packed == bool(layout)
    return out


def whole_handle(w):
    import cosdata_amd as ca
    return ca.InvertedIndex.from_vectors(w.bits, UPPER, w.row_off, w.raw_dims, w.raw_vals, keep_raw=True)
