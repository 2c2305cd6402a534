// exact_rerank.h — the rule every dense answer ends with (replace_with_exact_distances / finalize_ann_results,
// vector_store.rs:404-445), written once (device only, apart from the LDS size both sides of a launch need):
//   a few candidates are re-scored on the raw f32 rows, cs = dot_f32(q, x) / (|q| * |x|), sorted by f32::total_cmp descending with
//   the larger id first on ties, and the best top_k are the answer.
// Bit parity with the reference rests on four details:
//   * the dot's eight chains and their pairwise tree (dot_product_f32_simd, x86_64.rs:418-444): f32_pair_dot / f32_oct_dot of
//     dot_engines.h, the same bits from two or eight lanes per row;
//   * |q| * |x| is a product of its own, never fused into the division;
//   * 0/0 is x86's NEGATIVE NaN, which total_cmp ranks last (x86_div);
//   * the order is that of the u64 key (simkey(cs) << 32 | id), the conventions of topk_select.h.
// The kernel calls the dot itself, as one line at the call site, and hands the result to exact_key: wrapped in a second inlined
// layer the row loads are scheduled differently (flat_rescore has a register budget, tests/test_flat_wide_registers.py).
// Used by kernels_finalize.hip (every rerank loop; write_topk in finalize_fast_kernel), kernels_flat.hip (flat_rescore,
// flat_rerank_top5k; score_key in the scans) and kernels_flat_wide.hip (flat_rerank_w).
// Checked on the device against a host model of the rule by tests/cxx/exact_rerank_check.hip.
#pragma once
#include "dot_engines.h"
#include "topk_select.h"

namespace cosdev {

// LDS of a staged f32 query: dim floats, padded to 16 bytes (what follows it stays 16-byte aligned)
__host__ __device__ constexpr size_t staged_query_bytes(u32 dim) { return ((size_t)dim * 4 + 15) & ~(size_t)15; }

// the key of a score: total_cmp descending, the larger id first on ties
__device__ __forceinline__ u64 score_key(float score, u32 id) { return pack_key(simkey(score), id); }

// The key of candidate `id` from its dot: cs = dp / (mag_query * mag_raw), vector_store.rs:425-427.  No zero check there: a zero raw
// vector or a zero query divides 0 by 0, x86's negative NaN, and ranks last.  The empty key when the lane has no candidate.
__device__ __forceinline__ u64 exact_key(float dp, float mq, float xmag, u32 id, bool valid) {
    const float cs = x86_div(dp, __fmul_rn(mq, xmag));
    return valid ? score_key(cs, id) : 0ull;
}

// A pass of 32 candidates, one lane pair each: candidate base + j, computed by lanes 2j and 2j + 1, lands in lane base + j
// (base = 0 or 32; the other lanes keep their res)
__device__ __forceinline__ void pair_keys_to_lanes(u64 key, u32 base, int lane, u64 &res) {
    const int from = (2 * (lane - (int)base)) & 63;
    const u32 klo = (u32)__shfl((int)(u32)key, from, 64), khi = (u32)__shfl((int)(u32)(key >> 32), from, 64);
    if ((u32)lane >= base && (u32)lane < base + 32) res = ((u64)khi << 32) | klo;
}

// The first nout keys of a sorted blocked array (e = lane * R + r) as query q's results: id + id_base, the score's bits back.
// FILL (the brute-force contract, nout = k): an empty key is written as 0xFFFFFFFF / 0.0f.
template <int R, bool FILL>
__device__ __forceinline__ void write_topk(const u64 (&res)[R], u32 nout, u32 k, u32 q, u32 id_base, u32 *out_ids, float *out_scores, int lane) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const u32 e = (u32)lane * R + r;
        if (e < nout) {
            const bool ok = !FILL || res[r] != 0ull;
            out_ids[(u64)q * k + e] = ok ? (u32)res[r] + id_base : 0xFFFFFFFFu;
            out_scores[(u64)q * k + e] = ok ? simkey_inv((u32)(res[r] >> 32)) : 0.0f;
        }
    }
}

} // namespace cosdev
