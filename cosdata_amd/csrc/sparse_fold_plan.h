// sparse_fold_plan.h — the host-only part of the learned-sparse search on a shard set (kernels_sparse.hip: the record finish kernels and
// sparse_fold_rerank_kernel<N>; shardset.hip: cos_shardset_sparse_search_batch): the layout of a shard's candidate record, which fold
// kernel takes the S gathered records of a query, and the refusal above what it holds.  Plain C++17, no HIP header and no handle, so that
// a stand-alone program can check it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sparse_fold_plan {

// cos_status values of include/cosdata_hip.h, restated so that the header stands alone (kernels_sparse.hip asserts that they agree)
constexpr int32_t OK = 0, INVALID = 3, UNIMPLEMENTED = 4;

constexpr uint32_t MIN_STRIDE = 64;      // the narrow scan keeps 64 candidates per query
constexpr uint32_t MAX_CANDIDATES = 1024; // the widest C = top_k * max(reranking_factor, 1) a handle admits (cos_sparse_set_max_candidates)
constexpr uint32_t MIN_KEYS = 256;       // the narrowest fold: one key per thread
constexpr uint32_t MAX_KEYS = 8192;      // sparse_fold_rerank_kernel<N>: N keys of 8 bytes in LDS, the ceiling of merge_lists_lds_kernel<N>
constexpr uint32_t THREADS = 256;        // one workgroup of this many threads per query

// key slots per query in a record: the pool width 64 * R of the scan that produced it, R = 1, 2, 4, 8, 16
inline uint32_t record_stride(uint64_t C) {
    uint32_t w = MIN_STRIDE;
    while (w < C && w < MAX_CANDIDATES) w *= 2;
    return w;
}

// One shard's record for a batch of B queries, in 32-bit words (what one all-gather or one copy moves):
//   [ keys   u64 [B][stride] : pack_key(similarity + 1, id_base + local id), descending, 0 behind the query's count
//   | counts u32 [B] (+ one word of padding when B is odd: S records side by side keep their keys 8-byte aligned)
//   | raw    u32 [B][stride] : simkey(raw-value dot product) of the candidate in the same slot — only when the call reranks ]
struct Layout {
    uint32_t stride;
    size_t counts, raw, words; // word offsets of the two later parts, and the record's size
};
inline Layout layout(uint32_t B, uint64_t C, bool rerank) {
    Layout l{};
    l.stride = record_stride(C);
    l.counts = (size_t)2 * B * l.stride;
    l.raw = l.counts + (((size_t)B + 1) & ~(size_t)1);
    l.words = l.raw + (rerank ? (size_t)B * l.stride : 0);
    return l;
}

struct Plan {
    uint32_t N;     // keys in LDS; 0 when refused
    int32_t status; // OK, or what the entry point returns
    uint64_t keys;  // S * record stride
    uint32_t lds_bytes() const { return N * 8u; }
};
// S shards, C candidates per query
inline Plan plan(uint32_t S, uint64_t C) {
    if (S == 0 || C == 0) return {0u, INVALID, 0ull};
    if (C > MAX_CANDIDATES) return {0u, UNIMPLEMENTED, (uint64_t)S * MAX_CANDIDATES};
    const uint64_t keys = (uint64_t)S * record_stride(C);
    if (keys > MAX_KEYS) return {0u, UNIMPLEMENTED, keys};
    uint32_t N = MIN_KEYS;
    while (N < keys) N *= 2;
    return {N, OK, keys};
}

} // namespace sparse_fold_plan
