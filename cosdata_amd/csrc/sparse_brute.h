// sparse_brute.h — what kernels_sparse.hip (the learned-sparse handle) and kernels_sparse_brute.hip (the exact scan of its raw rows)
// share: the raw-value score rule, stated once, and the scan's host interface.
#pragma once
#include "dev_mem.h"
#include "device_common.h"
#include "engine_internal.h"

namespace cosdev {

// finalize_sparse_ann_results' score of vector v (indexes/inverted/mod.rs:333-381): dp over the QUERY pairs in the order given, one f32
// multiply then one f32 add per dimension the row holds (row dimensions ascend: binary search).  The slow path of
// cos_sparse_bruteforce_topk calls this and its fast path reproduces its bits.  It restates raw_rerank_key (kernels_sparse.hip), which
// keeps its own text: routed through this function sparse_finish_kernel compiled to a different instruction stream (a branch laid out
// the other way round), and that unit's device code is held byte-identical.  tests/test_gpu_sparse_brute.py holds the two to the same bits.
__device__ __forceinline__ float sparse_raw_dot(const u64 *row_off, const u32 *raw_dims, const float *raw_vals, u32 v,
                                                const u32 *__restrict__ q_dims, const float *__restrict__ q_vals, const u32 *__restrict__ q_off, u32 q) {
    const u64 b = row_off[v], e = row_off[v + 1];
    float dp = 0.0f;
    for (u32 i = q_off[q]; i < q_off[q + 1]; i++) {
        const u32 d = q_dims[i];
        u64 lo = b, hi = e;
        while (lo < hi) { const u64 mid = lo + (hi - lo) / 2; if (raw_dims[mid] < d) lo = mid + 1; else hi = mid; }
        if (lo < e && raw_dims[lo] == d) dp = __fadd_rn(dp, __fmul_rn(raw_vals[lo], q_vals[i]));
    }
    return dp;
}

constexpr u32 SPARSE_BRUTE_MAX_K = 1024; // the widest pool of topk_select.h the sparse kernels instantiate: 64 * 16

// the raw CSR of a handle as the scan reads it (device pointers; the caller holds the handle's lock)
struct SparseBruteIndex {
    const u64 *row_off;    // [n + 1], non-decreasing, row_off[n] == nnz (cos_sparse_create checks, cos_sparse_insert keeps it)
    const u32 *raw_dims;   // [nnz]
    const float *raw_vals; // [nnz]
    const u32 *dead;       // [(n + 31) / 32] bit v % 32 of word v / 32: vector v was given to cos_sparse_delete
    u32 n;
    u64 nnz;
    bool rows_ascend;      // the dimensions of every row strictly ascend: the fast path's order argument holds
};

// grow-only workspace and the figures of the last call; owned by the handle
struct SparseBruteWs {
    DevBuf w_in, w_part, w_oi, w_os, w_oc;
    PinArr<unsigned char> h_in;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    u32 queries = 0, slow_queries = 0, blocks = 0, pool = 0;
    float kernel_ms = 0.0f;
    u64 raw_bytes = 0;
    ~SparseBruteWs() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// The exact top k of every query over the live rows that share a dimension with it; host arrays in and out, default stream, returns
// with the results copied back.  k > SPARSE_BRUTE_MAX_K is COS_ERR_UNIMPLEMENTED.
int32_t sparse_brute_topk(SparseBruteWs &ws, const SparseBruteIndex &ix, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 k,
                          uint32_t *out_ids, float *out_scores, uint32_t *out_counts);

} // namespace cosdev
