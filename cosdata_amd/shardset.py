"""Host-side mirror of the shard-set entry points of include/cosdata_hip.h.

ShardSet          every shard in this process (the reference's single-process host): batch_search() fans a query batch out to
                  the S resident shards and returns the merged global top-k — walk + rerank per shard, ONE all-gather of the
                  packed records (RCCL), merge kernel; everything below the call is C++/HIP.  search_filtered(), flat_search() and
                  bruteforce_topk() do the same with the index's other search operators (masks over the collection's GLOBAL rows).
ProcessShardSet   one process per GPU (bench.py under torchrun): the process owns one shard; exchange_device() is the
                  per-launch all-gather + merge on the caller's stream.  torch.distributed is used ONLY to hand rank 0's
                  ncclUniqueId to the other ranks.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import CosdataError, check

UNIQUE_ID_BYTES = 128


class ShardSet:
    def __init__(self, shards: Sequence["HNSWIndex"]):  # noqa: F821
        self.shards = list(shards)
        arr = (C.c_void_p * len(self.shards))(*[s._h for s in self.shards])
        self._h = C.c_void_p()
        check(_lib.lib().cos_shardset_create(arr, len(self.shards), 0, len(self.shards), None, C.byref(self._h)))
        self.dim = self.shards[0].dim
        self.bm25_shards = []                           # the attached BM25 handles (attach_bm25), kept alive while attached
        self.sparse_shards = []                         # ... and the learned-sparse ones (attach_sparse)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().cos_shardset_destroy(self._h)
            self._h = C.c_void_p()
        self.bm25_shards = []
        self.sparse_shards = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch_search(self, queries, top_k: int):
        """[B][dim] raw f32 -> merged (global ids [B][k], exact cosine scores [B][k], counts [B])"""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise CosdataError(_lib.ERR_INVALID, f"queries must be [B][{self.dim}] f32, got shape {tuple(q.shape)}")
        B = q.shape[0]
        ids = np.full((B, top_k), 0xFFFFFFFF, np.uint32)
        scores = np.zeros((B, top_k), np.float32)
        counts = np.zeros(B, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_search_batch(self._h, p(q), B, top_k, p(ids), p(scores), p(counts)))
        return ids, scores, counts

    # ---- the other search operators of an index, on every shard behind one call ----------------------------------------------
    def _outputs(self, queries, top_k: int):
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise CosdataError(_lib.ERR_INVALID, f"queries must be [B][{self.dim}] f32, got shape {tuple(q.shape)}")
        B = q.shape[0]
        return q, B, np.full((B, top_k), 0xFFFFFFFF, np.uint32), np.zeros((B, top_k), np.float32), np.zeros(B, np.uint32)

    def row_bounds(self):
        """[S + 1] global row numbers: shard s holds the rows [bounds[s], bounds[s + 1]) of the collection, in shard order"""
        return np.concatenate([[0], np.cumsum([s.n for s in self.shards])]).astype(np.int64)

    def _shard_masks(self, masks, query_mask, skip_deleted: bool, B: int):
        """masks over GLOBAL rows (bool [N] or [G][N], or uint32 [G][ceil(N / 32)] packed) -> (cos_scan_mask*[S] or None, keep-alive)"""
        from .index import pack_row_masks
        from .sharding import slice_row_masks
        if masks is None and query_mask is None and not skip_deleted:
            return None, ()
        bounds = self.row_bounds()
        N, S = int(bounds[-1]), len(self.shards)
        per_shard, qm = [None] * S, None
        if masks is not None:
            m = np.asarray(masks)
            if m.dtype == np.uint32:
                bits = np.ascontiguousarray(np.atleast_2d(m))
                if bits.ndim != 2 or bits.shape[1] != (N + 31) // 32:
                    raise CosdataError(_lib.ERR_INVALID, f"packed masks must be uint32 [G][{(N + 31) // 32}], got shape {tuple(bits.shape)}")
            else:
                m = np.atleast_2d(m.astype(bool))
                if m.ndim != 2 or m.shape[1] != N:
                    raise CosdataError(_lib.ERR_INVALID, f"masks must be bool [{N}] or [G][{N}] over the collection's rows, got shape {tuple(np.shape(masks))}")
                bits = pack_row_masks(m)
            per_shard = slice_row_masks(bits, bounds)
        if query_mask is not None:
            qm = np.ascontiguousarray(np.atleast_1d(query_mask), dtype=np.uint32)
            if qm.shape != (B,):
                raise CosdataError(_lib.ERR_INVALID, f"query_mask must hold {B} mask indices, got shape {tuple(qm.shape)}")
        structs = [_lib.CosScanMask(C.sizeof(_lib.CosScanMask), _lib.SCAN_SKIP_DELETED if skip_deleted else 0,
                                    b.shape[0] if b is not None else 0, b.ctypes.data if b is not None else None,
                                    qm.ctypes.data if qm is not None else None) for b in per_shard]
        arr = (C.POINTER(_lib.CosScanMask) * S)(*[C.pointer(s) for s in structs])
        return arr, (structs, per_shard, qm)

    def search_filtered(self, queries, filter_offsets, filter_dims, top_k: int):
        """HNSWIndex.search_filtered on every shard (each a metadata collection, id_base = first embedding x max_replicas), merged:
        (global replica ids [B][k], exact cosine scores, counts)"""
        q, B, ids, scores, counts = self._outputs(queries, top_k)
        off = np.ascontiguousarray(filter_offsets, dtype=np.uint32)
        fd = np.ascontiguousarray(np.atleast_2d(filter_dims), dtype=np.int8)
        mdim = self.shards[0].mdim
        if off.shape != (B + 1,) or fd.ndim != 2 or fd.shape[1] != mdim or off[-1] != fd.shape[0]:
            raise CosdataError(_lib.ERR_INVALID, f"filters must be [F][{mdim}] i8 with {B + 1} offsets ending at F")
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_search_filtered_batch(self._h, p(q), B, p(off), p(fd), top_k, p(ids), p(scores), p(counts)))
        return ids, scores, counts

    def flat_search(self, queries, top_k: int, masks=None, query_mask=None, skip_deleted: bool = False):
        """HNSWIndex.flat_search / flat_search_masked on every shard, merged.  `masks` are over the GLOBAL rows of the collection (row r of
        shard s is global row row_bounds()[s] + r) and are cut at the shard boundaries here; skip_deleted reads every shard's own deleted
        set.  The 5 * top_k cut of the rerank is applied per shard."""
        q, B, ids, scores, counts = self._outputs(queries, top_k)
        sm, keep = self._shard_masks(masks, query_mask, skip_deleted, B)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_flat_search_batch(self._h, p(q), B, top_k, sm, p(ids), p(scores), p(counts)))
        del keep
        return ids, scores, counts

    def bruteforce_topk(self, queries, k: int, masks=None, query_mask=None, skip_deleted: bool = False):
        """HNSWIndex.bruteforce_topk / bruteforce_topk_masked on every shard, merged: the exact global top-k of the collection (ids and
        score bits of one index holding every row).  k in [1, min(512, rows of the smallest shard)]; masks as in flat_search."""
        q, B, ids, scores, counts = self._outputs(queries, k)
        sm, keep = self._shard_masks(masks, query_mask, skip_deleted, B)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_bruteforce_topk(self._h, p(q), B, k, sm, p(ids), p(scores), p(counts)))
        del keep
        return ids, scores, counts

    # ---- the text half of the collection: BM25 and dense + BM25 hybrid search ---------------------------------------------------
    def attach_bm25(self, indexes, doc_bases=None):
        """indexes[s] (BM25Index) holds the documents of shard s under LOCAL ids; a document's global id is doc_bases[s] + local id
        (None: the dense shards' id_base).  The handles stay the caller's — inserts and deletes go to the owning shard's handle with
        local ids — and must outlive the attachment; attaching again replaces them, attach_bm25(None) detaches."""
        if indexes is None:
            check(_lib.lib().cos_shardset_attach_bm25(self._h, None, 0, None))
            self.bm25_shards = []
            return self
        indexes = list(indexes)
        arr = (C.c_void_p * max(len(indexes), 1))(*[b._h for b in indexes])
        bases = None if doc_bases is None else np.ascontiguousarray(doc_bases, dtype=np.uint32)
        if bases is not None and bases.shape != (len(indexes),):
            raise CosdataError(_lib.ERR_INVALID, f"doc_bases must hold {len(indexes)} bases, got shape {tuple(bases.shape)}")
        check(_lib.lib().cos_shardset_attach_bm25(self._h, arr, len(indexes), None if bases is None else bases.ctypes.data_as(C.c_void_p)))
        self.bm25_shards = indexes                      # (kept alive while attached)
        return self

    @staticmethod
    def _terms(q_terms, q_offsets):
        qt = np.ascontiguousarray(q_terms, dtype=np.uint32).ravel()
        qo = np.ascontiguousarray(q_offsets, dtype=np.uint32).ravel()
        if qo.size < 1 or int(qo[-1]) != qt.size:
            raise CosdataError(_lib.ERR_INVALID, "q_offsets must have B + 1 entries and end at len(q_terms)")
        if qt.size == 0:
            qt = np.zeros(1, np.uint32)                 # (a non-null pointer for a batch of empty queries)
        return qt, qo

    def bm25_search(self, q_terms, q_offsets, top_k: int):
        """BM25Index.search_batch over the attached shards: global ids [B][k], score bits and counts [B] of ONE index holding the whole
        collection's postings (the idf is the collection's, the 512 buckets are folded over the shards)"""
        qt, qo = self._terms(q_terms, q_offsets)
        B = qo.size - 1
        ids = np.full((B, top_k), 0xFFFFFFFF, np.uint32)
        scores = np.zeros((B, top_k), np.float32)
        counts = np.zeros(B, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_bm25_search_batch(self._h, p(qt), p(qo), B, top_k, p(ids), p(scores), p(counts)))
        return ids, scores, counts

    def hybrid_search(self, queries, q_terms, q_offsets, top_k: int, fusion_constant_k: float = 60.0):
        """hybrid_search_batch on the set: batch_search and bm25_search for 3 * top_k each, fused by RRF on shard 0's device"""
        q, B, ids, scores, counts = self._outputs(queries, top_k)
        qt, qo = self._terms(q_terms, q_offsets)
        if qo.size != B + 1:
            raise CosdataError(_lib.ERR_INVALID, f"{B} dense queries but {qo.size - 1} term lists")
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_hybrid_search_batch(self._h, p(q), p(qt), p(qo), B, top_k, fusion_constant_k, p(ids), p(scores), p(counts)))
        return ids, scores, counts

    # ---- the learned-sparse half of the collection, and the mixed hybrid call ---------------------------------------------------
    def attach_sparse(self, indexes, vec_bases=None):
        """indexes[s] (InvertedIndex) holds the vectors of shard s under LOCAL ids; a vector's global id is vec_bases[s] + local id
        (None: the dense shards' id_base).  Every handle has the same quantization_bits and values_upper_bound.  The handles stay the
        caller's — inserts and deletes go to the owning shard's handle with local ids — and must outlive the attachment; attaching again
        replaces them, attach_sparse(None) detaches."""
        if indexes is None:
            check(_lib.lib().cos_shardset_attach_sparse(self._h, None, 0, None))
            self.sparse_shards = []
            return self
        indexes = list(indexes)
        arr = (C.c_void_p * max(len(indexes), 1))(*[b._h for b in indexes])
        bases = None if vec_bases is None else np.ascontiguousarray(vec_bases, dtype=np.uint32)
        if bases is not None and bases.shape != (len(indexes),):
            raise CosdataError(_lib.ERR_INVALID, f"vec_bases must hold {len(indexes)} bases, got shape {tuple(bases.shape)}")
        check(_lib.lib().cos_shardset_attach_sparse(self._h, arr, len(indexes), None if bases is None else bases.ctypes.data_as(C.c_void_p)))
        self.sparse_shards = indexes                    # (kept alive while attached)
        return self

    def sparse_search(self, q_dims, q_vals, q_offsets, top_k: int, early_terminate_threshold: float = 0.0, reranking_factor: int = 0):
        """InvertedIndex.search_batch over the attached shards: global ids [B][k], score bits and counts [B] of ONE index holding the
        whole collection (every shard's best top_k * max(reranking_factor, 1) candidates are cut to the collection's, and only those are
        re-ranked by raw value); entries past counts[q] keep 0xFFFFFFFF / 0"""
        qd = np.ascontiguousarray(q_dims, dtype=np.uint32).ravel()
        qv = np.ascontiguousarray(q_vals, dtype=np.float32).ravel()
        qo = np.ascontiguousarray(q_offsets, dtype=np.uint32).ravel()
        if qo.size < 1 or qd.size != qv.size or int(qo.max(initial=0)) > qd.size:
            raise CosdataError(_lib.ERR_INVALID, "q_offsets must have B + 1 entries inside q_dims / q_vals")
        if qd.size == 0:
            qd, qv = np.zeros(1, np.uint32), np.zeros(1, np.float32)   # (non-null pointers for a batch of empty queries)
        B = qo.size - 1
        ids = np.full((B, max(top_k, 1)), 0xFFFFFFFF, np.uint32)
        scores = np.zeros((B, max(top_k, 1)), np.float32)
        counts = np.zeros(max(B, 1), np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_sparse_search_batch(self._h, p(qd), p(qv), p(qo), B, top_k, early_terminate_threshold, reranking_factor,
                                                          p(ids), p(scores), p(counts)))
        return ids, scores, counts[:B]

    def hybrid_search_mixed(self, arms, dense_queries, sparse_queries, bm25_queries, top_k: int, fusion_constant_k: float = 60.0,
                            early_terminate_threshold: float = 0.0, reranking_factor: int = 0):
        """hybrid.hybrid_search_mixed on the set (cos_shardset_hybrid_search_mixed): the same arguments without the context and the three
        indexes — the dense shards, attach_sparse and attach_bm25 stand for them; a half without queries needs nothing attached"""
        from .hybrid import mixed_request
        dense = lambda x: np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32)
        rq, keep, B, ids, scores, counts = mixed_request(arms, dense, dense_queries, sparse_queries, bm25_queries, top_k, fusion_constant_k,
                                                         early_terminate_threshold, reranking_factor)
        if rq.dense_queries and keep[1].shape[1] != self.dim:
            raise CosdataError(_lib.ERR_INVALID, f"dense queries must be [n][{self.dim}] f32, got shape {tuple(keep[1].shape)}")
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().cos_shardset_hybrid_search_mixed(self._h, C.byref(rq), p(ids), p(scores), p(counts)))
        del keep
        return ids, scores, counts[:B]


class ProcessShardSet:
    """One local shard of a world-size shard set.  Construction is COLLECTIVE: every rank must call it, and every rank gets the
    same outcome — either all ranks hold a working communicator, or all of them raise (so a caller can fall back together
    instead of leaving some ranks blocked in a collective the others never enter)."""

    def __init__(self, index, rank: int, world: int, local_rank: int, dist=None):
        import torch
        self._h = C.c_void_p()
        if world <= 1:
            arr = (C.c_void_p * 1)(index._h)
            check(_lib.lib().cos_shardset_create(arr, 1, 0, 1, None, C.byref(self._h)))
            return
        dev = f"cuda:{local_rank}"
        # 1. rank 0 obtains the ncclUniqueId; [ok flag | 128 id bytes] goes to everybody
        msg = np.zeros(1 + UNIQUE_ID_BYTES, np.uint8)
        err0 = ""
        if rank == 0:
            rc = _lib.lib().cos_shardset_unique_id(msg[1:].ctypes.data_as(C.c_void_p))
            msg[0] = 1 if rc == _lib.OK else 0
            if rc != _lib.OK:
                err0 = _lib.lib().cos_last_error_string().decode("utf-8", "replace")
        t = torch.from_numpy(msg).to(dev)
        dist.broadcast(t, 0)
        msg = t.cpu().numpy()
        if msg[0] != 1:
            raise CosdataError(_lib.ERR_HIP, "rank 0 could not create an ncclUniqueId" + (": " + err0 if err0 else ""))
        # 2. every rank joins the communicator; the outcome is agreed with a MIN all-reduce
        self._uid = np.ascontiguousarray(msg[1:])
        arr = (C.c_void_p * 1)(index._h)
        rc = _lib.lib().cos_shardset_create(arr, 1, rank, world, self._uid.ctypes.data_as(C.c_void_p), C.byref(self._h))
        err = _lib.lib().cos_last_error_string().decode("utf-8", "replace") if rc != _lib.OK else ""
        ok = torch.tensor([1 if rc == _lib.OK else 0], device=dev, dtype=torch.int32)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) != 1:
            self.close()
            raise CosdataError(rc if rc != _lib.OK else _lib.ERR_HIP, "shard set creation failed on " + ("this rank: " + err if err else "another rank"))

    def exchange_device(self, packed_ptr: int, B: int, k: int, gathered_ptr: int, out_ids_ptr: int, out_scores_ptr: int, out_counts_ptr: int,
                        stream: int = 0):
        check(_lib.lib().cos_shardset_exchange_device(self._h, C.c_void_p(packed_ptr), B, k, C.c_void_p(gathered_ptr), C.c_void_p(out_ids_ptr),
                                                      C.c_void_p(out_scores_ptr), C.c_void_p(out_counts_ptr), C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().cos_shardset_destroy(self._h)
            self._h = C.c_void_p()
