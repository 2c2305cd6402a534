// hybrid_plan.h — the host-only part of cos_hybrid_search_mixed (kernels_hybrid.hip): the split of a request's arm[] into the three
// sub-batches with every query's position in the two it belongs to, and the limit checks that refuse a request before anything is
// enqueued.  Plain C++17, no HIP header and no handle, so that a stand-alone program can check it (tests/cxx/hybrid_plan_check.cpp).
//   batch_hybrid_search's query_mapping     api/vectordb/search/repo.rs:366-419
//   first / second list of an arm           api/vectordb/search/repo.rs:485-522 (the first list's scores are inserted, the second's added)
#pragma once
#include <cstdint>

namespace hybrid_plan {

// cos_status values of include/cosdata_hip.h, restated so that the header stands alone (kernels_hybrid.hip asserts that they agree)
constexpr int32_t OK = 0, INVALID = 3, UNIMPLEMENTED = 4, NOT_READY = 6;

constexpr uint32_t DENSE_SPARSE = 0, DENSE_BM25 = 1, SPARSE_BM25 = 2; // COS_HYBRID_*
// every half is asked for 3 * top_k: BM25 keeps 512 buckets per query and the RRF kernels hold two lists of at most 1024 ids together
constexpr uint32_t LIST_FACTOR = 3, MAX_LIST = 512, MAX_TOP_K = MAX_LIST / LIST_FACTOR; // 170

constexpr bool arm_has_dense(uint32_t arm) { return arm == DENSE_SPARSE || arm == DENSE_BM25; }
constexpr bool arm_has_sparse(uint32_t arm) { return arm == DENSE_SPARSE || arm == SPARSE_BM25; }
constexpr bool arm_has_bm25(uint32_t arm) { return arm == DENSE_BM25 || arm == SPARSE_BM25; }

// one query of the request: its arm and the row of its FIRST and SECOND list inside the sub-batches of the two halves the arm names:
// (dense, sparse), (dense, BM25), (sparse, BM25).  Three words per query, read as such by rrf_mixed_kernel.
struct Slot {
    uint32_t arm, pos_first, pos_second;
};
struct Split {
    uint32_t n_dense = 0, n_sparse = 0, n_bm25 = 0;
};

// the reference's running counts: a query takes the next free row of each sub-batch it joins, in request order.
// INVALID for an arm value above 2 (*bad_query names it); slots may be written up to there.
inline int32_t split(const uint8_t *arm, uint32_t B, Slot *slots, Split &out, uint32_t *bad_query) {
    out = Split{};
    for (uint32_t q = 0; q < B; q++) {
        const uint32_t a = arm[q];
        if (a > SPARSE_BM25) {
            if (bad_query) *bad_query = q;
            return INVALID;
        }
        Slot s{a, 0, 0};
        if (a == DENSE_SPARSE) { s.pos_first = out.n_dense++; s.pos_second = out.n_sparse++; }
        else if (a == DENSE_BM25) { s.pos_first = out.n_dense++; s.pos_second = out.n_bm25++; }
        else { s.pos_first = out.n_sparse++; s.pos_second = out.n_bm25++; }
        slots[q] = s;
    }
    return OK;
}

// CSR offsets [n + 1] never decrease
inline bool offsets_ascend(const uint32_t *off, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// the request's own numbers: INVALID for a struct that ends before the last field the library reads, an empty batch or top_k == 0;
// UNIMPLEMENTED for 3 * top_k > 512
inline int32_t check_request(uint32_t struct_size, uint32_t needed_struct_size, uint32_t B, uint32_t top_k) {
    if (struct_size < needed_struct_size || B == 0 || top_k == 0) return INVALID;
    if (top_k > MAX_TOP_K) return UNIMPLEMENTED;
    return OK;
}

// a half whose sub-batch is empty needs no handle
inline int32_t check_handles(const Split &sp, bool have_dense, bool have_sparse, bool have_bm25) {
    if ((sp.n_dense && !have_dense) || (sp.n_sparse && !have_sparse) || (sp.n_bm25 && !have_bm25)) return INVALID;
    return OK;
}

// what the learned-sparse handle admits (read under its lock)
struct SparseLimits {
    uint32_t max_candidates; // cos_sparse_set_max_candidates, rounded
    bool have_raw;           // raw vectors resident: the raw-value rerank is possible
    uint32_t batch_bound;    // the sparse search refuses batches of this many queries or more
};
// the sparse half is a search for 3 * top_k with the request's reranking factor, in the order the sparse search itself checks:
// batch size (INVALID), a rerank without raw vectors (NOT_READY), 3 * top_k * max(reranking_factor, 1) above the handle's setting
// (UNIMPLEMENTED).  No sparse query, no check: a DENSE_BM25 batch asks nothing of the sparse handle.
inline int32_t check_sparse(uint32_t n_sparse, uint32_t top_k, uint32_t reranking_factor, const SparseLimits &lim) {
    if (n_sparse == 0) return OK;
    if (n_sparse >= lim.batch_bound) return INVALID;
    if (reranking_factor != 0 && !lim.have_raw) return NOT_READY;
    const uint64_t width = (uint64_t)LIST_FACTOR * top_k * (reranking_factor ? reranking_factor : 1u);
    if (width > lim.max_candidates) return UNIMPLEMENTED;
    return OK;
}

// keys per lane of the fusion kernels: one wave sorts both lists of a query, 2 * 3 * top_k ids at most (0 = above what they hold)
inline uint32_t rrf_keys_per_lane(uint32_t ids) {
    for (uint32_t r = 1; r <= 16; r *= 2)
        if (ids <= 64 * r) return r;
    return 0;
}

} // namespace hybrid_plan
