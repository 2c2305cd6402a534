"""Host-side mirror of the reference's operators around the dense walk:

    distance_batch      DistanceMetric::calculate            src/models/types.rs:469
    BM25Index           TFIDFIndex / search_bm25             src/indexes/tf_idf/mod.rs:243, src/models/sparse_ann_query.rs:149
    rrf_fuse_batch      RRF fusion of hybrid_search          src/api/vectordb/search/repo.rs:311-340
    hybrid_search_mixed batch_hybrid_search, one arm per query   src/api/vectordb/search/repo.rs:343-555

All numeric work runs in libcosdata_hip.so (gfx950 kernels); no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .index import DistanceMetric, StorageType, _c, _p


def distance_batch(metric: DistanceMetric, storage_type: StorageType, dim: int, x_codes, x_mags, y_codes, y_mags, pair_x, pair_y):
    """out[p] = metric(x[pair_x[p]], y[pair_y[p]]) on stored vectors in the reference Storage layout.
    Returns (values f32[n_pairs], status i32[n_pairs]); status 2 = CalculationError (zero norm), 1 = StorageMismatch."""
    xc, yc = _c(x_codes, np.uint8), _c(y_codes, np.uint8)
    xm, ym = _c(x_mags, np.float32), _c(y_mags, np.float32)
    px, py = _c(pair_x, np.uint32), _c(pair_y, np.uint32)
    out = np.zeros(px.size, np.float32)
    status = np.zeros(px.size, np.int32)
    check(_lib.lib().cos_distance_batch(int(metric), int(storage_type.kind), storage_type.resolution, dim, _p(xc), _p(xm), xc.shape[0],
                                        _p(yc), _p(ym), yc.shape[0], _p(px), _p(py), px.size, _p(out), _p(status)))
    return out, status


class BM25Index:
    """Device-resident CSR postings of a TFIDFIndexRoot: term hashes ascending, offsets[T+1], (doc id, stored tf)."""

    def __init__(self, term_hashes, offsets, doc_ids, tfs, documents_count: int, device: int = 0):
        th, off = _c(term_hashes, np.uint32), _c(offsets, np.uint64)
        di, tf = _c(doc_ids, np.uint32), _c(tfs, np.float32)
        self._h = C.c_void_p()
        check(_lib.lib().cos_bm25_create(device, _p(th), _p(off), th.size, _p(di), _p(tf), documents_count, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().cos_bm25_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_batch(self, q_terms, q_offsets, top_k: int):
        """search_bm25 for B queries given as pre-hashed terms (CSR). -> ids [B][k], scores [B][k], counts [B]."""
        qt, qo = _c(q_terms, np.uint32), _c(q_offsets, np.uint32)
        B = qo.size - 1
        ids = np.full((B, top_k), 0xFFFFFFFF, np.uint32)
        sc = np.zeros((B, top_k), np.float32)
        cnt = np.zeros(B, np.uint32)
        check(_lib.lib().cos_bm25_search_batch(self._h, _p(qt), _p(qo), B, top_k, _p(ids), _p(sc), _p(cnt)))
        return ids, sc, cnt


def _bm25_search_batch_device(self, q_terms, q_offsets, top_k: int, out_ids_ptr: int, out_scores_ptr: int, out_counts_ptr: int, stream: int = 0):
    """same scoring, results left in device memory ([B][k] ids, [B][k] scores, [B] counts); enqueued on `stream`"""
    qt, qo = _c(q_terms, np.uint32), _c(q_offsets, np.uint32)
    check(_lib.lib().cos_bm25_search_batch_device(self._h, _p(qt), _p(qo), qo.size - 1, top_k, C.c_void_p(out_ids_ptr), C.c_void_p(out_scores_ptr),
                                                  C.c_void_p(out_counts_ptr), C.c_void_p(stream)))


BM25Index.search_batch_device = _bm25_search_batch_device


def _bm25_insert(self, doc_ids, doc_offsets, term_hashes, tfs):
    """TFIDFIndex::insert for m documents (cos_bm25_insert): document-major (doc_ids[m] strictly ascending and above every id the
    index has held, doc_offsets[m+1] into term_hashes / tfs); the resident postings are merged on the device"""
    di, do = _c(doc_ids, np.uint32), _c(doc_offsets, np.uint64)
    th, tf = _c(term_hashes, np.uint32), _c(tfs, np.float32)
    if do.size != di.size + 1 or th.size != tf.size or (do.size and int(do[-1]) != th.size):
        raise ValueError("doc_offsets must have len(doc_ids) + 1 entries and end at len(term_hashes) == len(tfs)")
    check(_lib.lib().cos_bm25_insert(self._h, _p(di), _p(do), di.size, _p(th), _p(tf)))
    return self


def _bm25_delete(self, doc_ids, doc_offsets, term_hashes):
    """TFIDFIndex::mark_embedding_as_deleted for m documents (cos_bm25_delete): tombstones in place, documents_count -= m"""
    di, do, th = _c(doc_ids, np.uint32), _c(doc_offsets, np.uint64), _c(term_hashes, np.uint32)
    if do.size != di.size + 1 or (do.size and int(do[-1]) != th.size):
        raise ValueError("doc_offsets must have len(doc_ids) + 1 entries and end at len(term_hashes)")
    check(_lib.lib().cos_bm25_delete(self._h, _p(di), _p(do), di.size, _p(th)))
    return self


def _bm25_stats(self) -> dict:
    """cos_bm25_stats as a dict: documents_count, n_terms, largest_doc_id, dir_rows, dir_tiles, postings, tombstones, device_bytes"""
    st = _lib.CosBM25Stats()
    st.struct_size = C.sizeof(_lib.CosBM25Stats)
    check(_lib.lib().cos_bm25_stats(self._h, C.byref(st)))
    return {name: int(getattr(st, name)) for name, _ in st._fields_ if name not in ("struct_size", "reserved")}


def _bm25_download(self):
    """cos_bm25_download -> (term_hashes, offsets, doc_ids, tfs, tombstones): the CSR cos_bm25_create takes + one flag per posting"""
    L = _lib.lib()
    nt, nnz = C.c_uint32(0), C.c_uint64(0)
    check(L.cos_bm25_download(self._h, C.byref(nt), C.byref(nnz), None, None, None, None, None))
    th, off = np.zeros(nt.value, np.uint32), np.zeros(nt.value + 1, np.uint64)
    n = int(nnz.value)
    di, tf, tomb = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint8)
    check(L.cos_bm25_download(self._h, C.byref(nt), C.byref(nnz), _p(th), _p(off), _p(di), _p(tf), _p(tomb)))
    return th, off, di[:n], tf[:n], tomb[:n].astype(bool)


BM25Index.insert = _bm25_insert
BM25Index.delete = _bm25_delete
BM25Index.stats = _bm25_stats
BM25Index.download = _bm25_download


def rrf_fuse_batch(dense_ids, dense_counts, sparse_ids, sparse_counts, fusion_constant_k: float, top_k: int):
    d, s = _c(dense_ids, np.uint32), _c(sparse_ids, np.uint32)
    dc, sc_ = _c(dense_counts, np.uint32), _c(sparse_counts, np.uint32)
    B = d.shape[0]
    ids = np.full((B, top_k), 0xFFFFFFFF, np.uint32)
    sc = np.zeros((B, top_k), np.float32)
    cnt = np.zeros(B, np.uint32)
    check(_lib.lib().cos_rrf_fuse_batch(_p(d), _p(dc), d.shape[1], _p(s), _p(sc_), s.shape[1], B, fusion_constant_k, top_k,
                                        _p(ids), _p(sc), _p(cnt)))
    return ids, sc, cnt


def hybrid_search_batch(index, bm25: "BM25Index", queries, q_terms, q_offsets, top_k: int, fusion_constant_k: float = 60.0):
    """repo::hybrid_search for B queries in one call: dense (top_k*3) + BM25 (top_k*3) concurrently on the device, RRF there"""
    q = index._queries(queries)
    qt, qo = _c(q_terms, np.uint32), _c(q_offsets, np.uint32)
    B = q.shape[0]
    ids = np.full((B, top_k), 0xFFFFFFFF, np.uint32)
    sc = np.zeros((B, top_k), np.float32)
    cnt = np.zeros(B, np.uint32)
    check(_lib.lib().cos_hybrid_search_batch(index._h, bm25._h, _p(q), _p(qt), _p(qo), B, top_k, fusion_constant_k, _p(ids), _p(sc), _p(cnt)))
    return ids, sc, cnt


ARM_DENSE_SPARSE, ARM_DENSE_BM25, ARM_SPARSE_BM25 = 0, 1, 2   # COS_HYBRID_*


class HybridContext:
    """What one mixed hybrid call keeps between calls (cos_hybrid): three streams, events, pinned staging, device buffers of the
    three list sets.  One call at a time per context; threads that search concurrently hold one each."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(_lib.lib().cos_hybrid_create(device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().cos_hybrid_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hybrid_search_mixed(ctx: "HybridContext", index, sparse, bm25, arms, dense_queries, sparse_queries, bm25_queries, top_k: int,
                        fusion_constant_k: float = 60.0, early_terminate_threshold: float = 0.0, reranking_factor: int = 0):
    """repo::batch_hybrid_search in one call (cos_hybrid_search_mixed): arms[B] names every query's arm (ARM_DENSE_SPARSE,
    ARM_DENSE_BM25, ARM_SPARSE_BM25); dense_queries [n_dense][dim], sparse_queries = (q_dims, q_vals, q_offsets) and
    bm25_queries = (q_terms, q_offsets) hold the queries of the arms that have such a half, in query order.  A half without queries
    takes None for its queries and may take None for its index.  Every half searches top_k * 3 on its own stream, RRF fuses each
    query's two lists on the device.  -> ids [B][k], scores [B][k], counts [B]; entries past counts[q] keep 0xFFFFFFFF / 0."""
    dense = (lambda x: index._queries(x)) if index is not None else (lambda x: _c(np.atleast_2d(x), np.float32))
    rq, keep, B, ids, sc, cnt = mixed_request(arms, dense, dense_queries, sparse_queries, bm25_queries, top_k, fusion_constant_k,
                                              early_terminate_threshold, reranking_factor)
    check(_lib.lib().cos_hybrid_search_mixed(ctx._h, index._h if index is not None else None, sparse._h if sparse is not None else None,
                                             bm25._h if bm25 is not None else None, C.byref(rq), _p(ids), _p(sc), _p(cnt)))
    del keep
    return ids, sc, cnt[:B]


def mixed_request(arms, dense, dense_queries, sparse_queries, bm25_queries, top_k: int, fusion_constant_k: float,
                  early_terminate_threshold: float, reranking_factor: int):
    """the cos_hybrid_request of a mixed hybrid batch and its output arrays (hybrid_search_mixed, ShardSet.hybrid_search_mixed):
    `dense` shapes the dense queries.  -> (request, arrays it points into, B, ids, scores, counts)"""
    a = _c(arms, np.uint8).ravel()
    B = a.size
    rq = _lib.CosHybridRequest()
    rq.struct_size = C.sizeof(_lib.CosHybridRequest)
    rq.B = B
    keep = [a]
    rq.arm = a.ctypes.data
    known = B == 0 or int(a.max()) <= ARM_SPARSE_BM25   # (an arm the library does not know is the library's to refuse)

    def ptr(x, dt):
        x = _c(x, dt)
        keep.append(x)
        return x.ctypes.data

    if dense_queries is not None:
        q = dense(dense_queries)
        n_dense = int(np.count_nonzero(a != ARM_SPARSE_BM25))
        if known and q.shape[0] != n_dense:
            raise ValueError(f"arms name {n_dense} queries with a dense half, dense_queries holds {q.shape[0]}")
        rq.dense_queries = ptr(q, np.float32)
    if sparse_queries is not None:
        qd, qv, qo = sparse_queries
        rq.sparse_dims, rq.sparse_vals, rq.sparse_offsets = ptr(qd, np.uint32), ptr(qv, np.float32), ptr(qo, np.uint32)
        n_sparse = int(np.count_nonzero(a != ARM_DENSE_BM25))
        if known and (keep[-1].size != n_sparse + 1 or keep[-3].size != keep[-2].size or keep[-3].size < int(keep[-1].max(initial=0))):
            raise ValueError(f"arms name {n_sparse} queries with a sparse half: q_offsets must hold {n_sparse + 1} entries inside q_dims / q_vals")
    if bm25_queries is not None:
        qt, qo = bm25_queries
        rq.bm25_terms, rq.bm25_offsets = ptr(qt, np.uint32), ptr(qo, np.uint32)
        n_bm25 = int(np.count_nonzero(a != ARM_DENSE_SPARSE))
        if known and (keep[-1].size != n_bm25 + 1 or keep[-2].size < int(keep[-1].max(initial=0))):
            raise ValueError(f"arms name {n_bm25} queries with a BM25 half: q_offsets must hold {n_bm25 + 1} entries inside q_terms")
    rq.sparse_early_terminate_threshold = early_terminate_threshold
    rq.sparse_reranking_factor = reranking_factor
    rq.top_k = top_k
    rq.fusion_constant_k = fusion_constant_k
    ids = np.full((B, max(top_k, 1)), 0xFFFFFFFF, np.uint32)
    sc = np.zeros((B, max(top_k, 1)), np.float32)
    cnt = np.zeros(max(B, 1), np.uint32)
    return rq, keep, B, ids, sc, cnt


class InvertedIndex:
    """Device-resident learned-sparse inverted index (src/indexes/inverted/mod.rs, src/models/inverted_index.rs) as CSR:
    dims ascending, key_offsets [T][2^bits + 1], vec_ids; optional raw sparse vectors (CSR) for the raw-value rerank."""

    def __init__(self, quantization_bits: int, values_upper_bound: float, dims, key_offsets, vec_ids, n_vectors: int,
                 raw_row_offsets=None, raw_dims=None, raw_vals=None, device: int = 0):
        d, ko, vi = _c(dims, np.uint32), _c(key_offsets, np.uint64), _c(vec_ids, np.uint32)
        raw = None
        if raw_row_offsets is not None:
            raw = (_c(raw_row_offsets, np.uint64), _c(raw_dims, np.uint32), _c(raw_vals, np.float32))
        self._h = C.c_void_p()
        self._bits = int(quantization_bits)
        check(_lib.lib().cos_sparse_create(device, quantization_bits, values_upper_bound, _p(d), d.size, _p(ko), _p(vi), n_vectors,
                                           _p(raw[0]) if raw else None, _p(raw[1]) if raw else None, _p(raw[2]) if raw else None,
                                           C.byref(self._h)))

    @classmethod
    def from_vectors(cls, quantization_bits: int, values_upper_bound: float, row_offsets, raw_dims, raw_vals, keep_raw: bool = True,
                     device: int = 0):
        """InvertedIndex::insert for ids 0 .. n-1 (cos_sparse_create_from_vectors): the CSR is built by the library on the host"""
        ro, rd, rv = _c(row_offsets, np.uint64), _c(raw_dims, np.uint32), _c(raw_vals, np.float32)
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self._bits = int(quantization_bits)
        check(_lib.lib().cos_sparse_create_from_vectors(device, quantization_bits, values_upper_bound, ro.size - 1, _p(ro), _p(rd), _p(rv),
                                                        1 if keep_raw else 0, C.byref(self._h)))
        return self

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().cos_sparse_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_batch(self, q_dims, q_vals, q_offsets, top_k: int, early_terminate_threshold: float = 0.0, reranking_factor: int = 0):
        """InvertedIndex::search_internal for B queries (CSR pairs): ids [B][k], scores [B][k], counts [B]"""
        qd, qv, qo = _c(q_dims, np.uint32), _c(q_vals, np.float32), _c(q_offsets, np.uint32)
        B = qo.size - 1
        ids = np.full((B, top_k), 0xFFFFFFFF, np.uint32)
        scores = np.zeros((B, top_k), np.float32)
        counts = np.zeros(B, np.uint32)
        check(_lib.lib().cos_sparse_search_batch(self._h, _p(qd), _p(qv), _p(qo), B, top_k, early_terminate_threshold, reranking_factor,
                                                 _p(ids), _p(scores), _p(counts)))
        return ids, scores, counts


def _sparse_search_batch_device(self, q_dims, q_vals, q_offsets, top_k: int, out_ids_ptr: int, out_scores_ptr: int, out_counts_ptr: int,
                                early_terminate_threshold: float = 0.0, reranking_factor: int = 0, stream: int = 0):
    """same search, results left in device memory ([B][k] ids, [B][k] scores, [B] counts); enqueued on `stream`, not synchronised"""
    qd, qv, qo = _c(q_dims, np.uint32), _c(q_vals, np.float32), _c(q_offsets, np.uint32)
    check(_lib.lib().cos_sparse_search_batch_device(self._h, _p(qd), _p(qv), _p(qo), qo.size - 1, top_k, early_terminate_threshold, reranking_factor,
                                                    C.c_void_p(out_ids_ptr), C.c_void_p(out_scores_ptr), C.c_void_p(out_counts_ptr), C.c_void_p(stream)))


InvertedIndex.search_batch_device = _sparse_search_batch_device


def _sparse_last_stats(self):
    """kernel time + visited postings of the most recent search_batch / search_batch_device on this handle"""
    st = _lib.CosSparseStats()
    check(_lib.lib().cos_sparse_last_stats(self._h, C.byref(st)))
    return st


InvertedIndex.last_stats = _sparse_last_stats


def _sparse_packed(self) -> bool:
    """True when the handle keeps one packed u32 per posting (cos_sparse_layout): the default since round 5 wherever vector ids fit 24 bits"""
    v = C.c_uint32(0)
    check(_lib.lib().cos_sparse_layout(self._h, C.byref(v)))
    return bool(v.value)


InvertedIndex.packed = property(_sparse_packed)


def _sparse_set_max_candidates(self, n: int):
    """cos_sparse_set_max_candidates: the widest top_k * max(reranking_factor, 1) a search_batch on this handle may keep, 1..1024
    (rounded up to 64, 128, 256, 512 or 1024; 64 unless set).  Narrower calls run what they ran before."""
    if not 0 <= int(n) <= 0xFFFFFFFF:
        raise ValueError("max_candidates must fit an unsigned 32-bit integer")
    check(_lib.lib().cos_sparse_set_max_candidates(self._h, int(n)))
    return self


def _sparse_max_candidates(self) -> int:
    """the rounded setting of set_max_candidates (cos_sparse_max_candidates)"""
    v = C.c_uint32(0)
    check(_lib.lib().cos_sparse_max_candidates(self._h, C.byref(v)))
    return int(v.value)


InvertedIndex.set_max_candidates = _sparse_set_max_candidates
InvertedIndex.max_candidates = property(_sparse_max_candidates)


def _sparse_insert(self, row_offsets, raw_dims, raw_vals) -> int:
    """InvertedIndex::insert for m more vectors (cos_sparse_insert): they take the ids [n, n + m); pairs of vector i are
    raw_dims / raw_vals [row_offsets[i], row_offsets[i+1]).  The resident postings are merged on the device.  -> the first new id"""
    ro, rd, rv = _c(row_offsets, np.uint64), _c(raw_dims, np.uint32), _c(raw_vals, np.float32)
    if ro.size < 1 or rd.size != rv.size or int(ro[-1]) != rd.size:
        raise ValueError("row_offsets must have m + 1 entries and end at len(raw_dims) == len(raw_vals)")
    first = C.c_uint32(0)
    check(_lib.lib().cos_sparse_insert(self._h, ro.size - 1, _p(ro), _p(rd), _p(rv), C.byref(first)))
    return int(first.value)


def _sparse_delete(self, ids, row_offsets, raw_dims, raw_vals) -> int:
    """InvertedIndex::mark_embedding_as_deleted for m vectors given with the pairs of their raw embeddings (cos_sparse_delete): the
    first posting of the id in the list of (dimension, quantize(value)) goes.  -> postings actually removed"""
    vi, ro, rd, rv = _c(ids, np.uint32), _c(row_offsets, np.uint64), _c(raw_dims, np.uint32), _c(raw_vals, np.float32)
    if ro.size != vi.size + 1 or rd.size != rv.size or int(ro[-1]) != rd.size:
        raise ValueError("row_offsets must have len(ids) + 1 entries and end at len(raw_dims) == len(raw_vals)")
    removed = C.c_uint64(0)
    check(_lib.lib().cos_sparse_delete(self._h, _p(vi), _p(ro), vi.size, _p(rd), _p(rv), C.byref(removed)))
    return int(removed.value)


def _sparse_stats(self) -> dict:
    """cos_sparse_stats as a dict: n_vectors, n_dims, dir_rows, dir_tiles, packed, have_raw, postings, removed, raw_pairs, device_bytes"""
    st = _lib.CosSparseIndexStats()
    st.struct_size = C.sizeof(_lib.CosSparseIndexStats)
    check(_lib.lib().cos_sparse_stats(self._h, C.byref(st)))
    return {name: int(getattr(st, name)) for name, _ in st._fields_ if name not in ("struct_size", "reserved")}


def _sparse_download(self):
    """cos_sparse_download -> (dims, key_offsets, vec_ids): the CSR cos_sparse_create takes, ids ascending inside a (dimension, key) list"""
    L = _lib.lib()
    nt, nnz = C.c_uint32(0), C.c_uint64(0)
    check(L.cos_sparse_download(self._h, C.byref(nt), C.byref(nnz), None, None, None))
    T, n = int(nt.value), int(nnz.value)
    w = (1 << self._bits) + 1
    dims, ko, vi = np.zeros(max(T, 1), np.uint32), np.zeros(max(T, 1) * w, np.uint64), np.zeros(max(n, 1), np.uint32)
    check(L.cos_sparse_download(self._h, C.byref(nt), C.byref(nnz), _p(dims), _p(ko), _p(vi)))
    return dims[:T], ko[:T * w], vi[:n]


InvertedIndex.insert = _sparse_insert
InvertedIndex.delete = _sparse_delete
InvertedIndex.stats = _sparse_stats
InvertedIndex.download = _sparse_download


def sparse_build_csr(quantization_bits: int, values_upper_bound: float, row_offsets, raw_dims, raw_vals):
    """cos_sparse_build_csr (host code, no device): raw sparse vectors in id order -> (dims, key_offsets, vec_ids)"""
    ro, rd, rv = _c(row_offsets, np.uint64), _c(raw_dims, np.uint32), _c(raw_vals, np.float32)
    n, nd = ro.size - 1, C.c_uint32(0)
    L = _lib.lib()
    check(L.cos_sparse_build_csr(quantization_bits, values_upper_bound, n, _p(ro), _p(rd), _p(rv), None, None, None, C.byref(nd)))
    dims = np.zeros(max(nd.value, 1), np.uint32)
    ko = np.zeros(max(nd.value, 1) * ((1 << quantization_bits) + 1), np.uint64)
    ids = np.zeros(max(int(ro[-1]), 1), np.uint32)
    check(L.cos_sparse_build_csr(quantization_bits, values_upper_bound, n, _p(ro), _p(rd), _p(rv), _p(dims), _p(ko), _p(ids), C.byref(nd)))
    return dims[:nd.value], ko[:nd.value * ((1 << quantization_bits) + 1)], ids[:int(ro[-1])]


STEM_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.POINTER(C.c_char), C.c_size_t, C.POINTER(C.c_char), C.c_size_t)


def stem_english(word: str) -> str:
    """the library's English Snowball stemmer (cos_stem_english) on one lowercased token"""
    raw = word.encode("utf-8")
    out = C.create_string_buffer(len(raw) + 8)
    n = _lib.lib().cos_stem_english(None, raw, len(raw), out, len(raw) + 8)
    return out.raw[:n].decode("utf-8")


def process_text(text: str, max_token_len: int = 40, average_document_length: float = 1.0, k1: float = 1.5, b: float = 0.75, stemmer="english"):
    """TFIDFIndex's process_text: text -> (term hashes ascending u32[], stored BM25 term frequencies f32[]).
    `stemmer`: "english" (default) = the library's English Snowball stemmer, like the reference's `Stemmer::create()`; None =
    hash the lowercased token unstemmed; or a callable str -> str (e.g. a shim over the host's own stemmer)."""
    raw = text.encode("utf-8")
    cap = max(16, len(raw) // 2 + 4)
    hashes = np.zeros(cap, np.uint32)
    tfs = np.zeros(cap, np.float32)
    n = C.c_uint32()
    cb = None
    if stemmer == "english":
        cb = C.cast(_lib.lib().cos_stem_english, C.c_void_p)
    elif stemmer is not None:
        def _shim(_ctx, tok, tok_len, out, out_cap):
            res = stemmer(C.string_at(tok, tok_len).decode("utf-8")).encode("utf-8")[:out_cap]
            C.memmove(out, res, len(res))
            return len(res)
        cb = STEM_FN(_shim)
    check(_lib.lib().cos_text_process(raw, len(raw), max_token_len, average_document_length, k1, b, C.cast(cb, C.c_void_p) if cb is not None else None, None,
                                      _p(hashes), _p(tfs), cap, C.byref(n)))
    return hashes[:n.value].copy(), tfs[:n.value].copy()


def count_tokens(text: str, max_token_len: int = 40) -> int:
    raw = text.encode("utf-8")
    return int(_lib.lib().cos_text_count_tokens(raw, len(raw), max_token_len))
