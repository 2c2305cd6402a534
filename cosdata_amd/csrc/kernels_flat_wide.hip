// kernels_flat_wide.hip — what stands behind the exhaustive scans' MFMA kernels when a query keeps more than 64 survivors
// (cos_flat_search_batch with top_k > 12, cos_bruteforce_topk with k > 32): pools of P = 64 * R keys, R = 2, 4, 8, 16.  The scan
// kernels (kernels_flat.hip, kernels_scan.hip) do not know the width: they read a threshold per query and append to app[B][cap].
//   flat_select_segments_w<R>  one wave per (query, segment of the score chunk) -> the segment's sorted top P
//   flat_select_merge_w<R>     one wave per query merges the S sorted partial lists into the query's pool
//   flat_select_append_w<R>    one wave per query folds the fused scan's append buffer into the pool
//   flat_rerank_w<R, BRUTE>    one workgroup (4 waves) per query: exact re-score of the survivors, sort, top k
// A pool lives sorted in registers, R keys per lane, and in memory as pool[q][e] (the conventions of topk_select.h).  Keys enter it
// BATCH-WISE through fold_stream<R> of that header (sort a batch of up to P keys, one bitonic merge with the pool): the seed chunk and
// an append fold pass thousands of keys per query, and a single insert into a 64 * R register pool costs ~6 R instructions
// (DESIGN.md §4.9).  This file holds the kernels and their launchers only.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "exact_rerank.h"
#include "flat_scan.h"

using namespace cosdev;

namespace {

// MASKED (flat_select_segments_w_masked): a row outside the query's mask gives the empty key (flat_scan.h ScanMask)
template <int R, bool MASKED>
__device__ __forceinline__ void select_segments_w_body(const float *__restrict__ scores, u64 s_stride, u32 B, u32 n0, u32 n_chunk, u32 seg_len,
                                                       u64 *__restrict__ part /*[B][S][64 R]*/, const ScanMask &m, u64 *batch /* LDS [64 R] */) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x, seg = blockIdx.y, S = gridDim.y;
    if (q >= B) return;
    u64 pool[R];
#pragma unroll
    for (int r = 0; r < R; r++) pool[r] = 0ull;
    u64 thr = 0ull;
    const float *sr = scores + (u64)q * s_stride;
    const u32 c0 = seg * seg_len, c1 = (c0 + seg_len < n_chunk) ? c0 + seg_len : n_chunk;
    const u32 count = c1 > c0 ? c1 - c0 : 0u;
    fold_stream<R>(pool, thr, batch, count, [&](u32 i) { return scan_live<MASKED>(m, q, n0 + c0 + i) ? score_key(sr[c0 + i], n0 + c0 + i) : 0ull; }, lane);
    u64 *dst = part + ((u64)q * S + seg) * (WAVE * R) + (u32)lane * R;
#pragma unroll
    for (int r = 0; r < R; r++) dst[r] = pool[r];
}
template <int R>
__global__ __launch_bounds__(64) void flat_select_segments_w(const float *__restrict__ scores, u64 s_stride, u32 B, u32 n0, u32 n_chunk, u32 seg_len,
                                                             u64 *__restrict__ part /*[B][S][64 R]*/) {
    __shared__ u64 batch[WAVE * R];
    select_segments_w_body<R, false>(scores, s_stride, B, n0, n_chunk, seg_len, part, ScanMask{nullptr, nullptr, 0u}, batch);
}
template <int R>
__global__ __launch_bounds__(64) void flat_select_segments_w_masked(const float *__restrict__ scores, u64 s_stride, u32 B, u32 n0, u32 n_chunk, u32 seg_len,
                                                                    u64 *__restrict__ part /*[B][S][64 R]*/, const ScanMask m) {
    __shared__ u64 batch[WAVE * R];
    select_segments_w_body<R, true>(scores, s_stride, B, n0, n_chunk, seg_len, part, m, batch);
}

template <int R>
__global__ __launch_bounds__(64) void flat_select_merge_w(const u64 *__restrict__ part, u32 B, u32 S, u64 *__restrict__ pool_mem /*[B][64 R]*/,
                                                          u64 *__restrict__ thr_out /*optional [B]*/) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    u64 pool[R], b[R];
    u64 *pm = pool_mem + (u64)q * (WAVE * R) + (u32)lane * R;
#pragma unroll
    for (int r = 0; r < R; r++) pool[r] = pm[r];
    for (u32 sgm = 0; sgm < S; sgm++) {
        const u64 *src = part + ((u64)q * S + sgm) * (WAVE * R) + (u32)lane * R;
#pragma unroll
        for (int r = 0; r < R; r++) b[r] = src[r];
        merge_sorted_desc<R>(pool, b, lane);
    }
#pragma unroll
    for (int r = 0; r < R; r++) pm[r] = pool[r];
    const u64 thr = readlane_u64(pool[R - 1], WAVE - 1);
    if (thr_out && lane == 0) thr_out[q] = thr;
}

// a counter above `cap` means the scan dropped entries: the flag makes the host repeat the search on the unfused path
template <int R>
__global__ __launch_bounds__(64) void flat_select_append_w(const u64 *__restrict__ app, u32 *__restrict__ app_cnt, u32 cap, u32 B, u64 *__restrict__ pool_mem,
                                                           u64 *__restrict__ thr_out, u32 *__restrict__ overflow) {
    __shared__ u64 batch[WAVE * R];
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    u64 pool[R];
    u64 *pm = pool_mem + (u64)q * (WAVE * R) + (u32)lane * R;
#pragma unroll
    for (int r = 0; r < R; r++) pool[r] = pm[r];
    u64 thr = readlane_u64(pool[R - 1], WAVE - 1);
    u32 cnt = uniform_u32(app_cnt[q]);
    if (cnt > cap) { if (lane == 0) atomicOr(overflow, 1u); cnt = cap; }
    const u64 *src = app + (u64)q * cap;
    fold_stream<R>(pool, thr, batch, cnt, [&](u32 i) { return src[i]; }, lane);
#pragma unroll
    for (int r = 0; r < R; r++) pm[r] = pool[r];
    if (lane == 0) { thr_out[q] = thr; app_cnt[q] = 0; }
}

// Exact re-score of a query's survivors against the raw f32 rows, sort, top k (the rule of exact_rerank.h), one lane pair per
// survivor, 128 survivors per pass of the 4 waves.
//   BRUTE = false (code scan): the best min(have, ncand_max) entries of the pool (sorted by quantized score) are re-scored;
//                              min(that, k) results and out_counts
//   BRUTE = true  (brute force): every survivor with a non-zero score key; k results, ~0 / 0.0 where there is none
template <int R, bool BRUTE>
__global__ __launch_bounds__(256) void flat_rerank_w(const float *__restrict__ Q, u64 q_stride, const float *__restrict__ qmags, u32 B,
                                                     const float *__restrict__ X, u64 x_stride, const float *__restrict__ xmags, u32 dim,
                                                     const u64 *__restrict__ pool_mem, u32 ncand_max, u32 k, u32 id_base, u32 *__restrict__ out_ids,
                                                     float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    constexpr u32 P = WAVE * R;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;                                            // [dim], padded to 16 B
    u64 *keys = (u64 *)(smem_raw + staged_query_bytes(dim));   // [P]
    const int tid = threadIdx.x, lane = tid & 63;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    for (u32 i = tid; i < dim; i += 256) qf[i] = Q[(u64)q * q_stride + i];
    __syncthreads();
    const u64 *pm = pool_mem + (u64)q * P;
    const float mq = qmags[q];
    const u32 lim = BRUTE ? P : (ncand_max < P ? ncand_max : P);
    for (u32 c0 = 0; c0 < P; c0 += 128) { // (P is a multiple of 128: every lane of a wave runs every pass)
        const u32 c = c0 + ((u32)tid >> 1);
        u64 key = 0ull;
        if (c0 < lim) { // workgroup-uniform
            const u64 pk = pm[c];
            const bool valid = BRUTE ? (u32)(pk >> 32) != 0u : (pk != 0ull && c < lim);
            const u32 sid = (u32)pk, row = valid ? sid : 0u;
            const float dp = f32_pair_dot(X + (u64)row * x_stride, qf, dim, tid & 1);
            key = exact_key(dp, mq, xmags[row], sid, valid);
        }
        if ((tid & 1) == 0) keys[c] = key;
    }
    __syncthreads();
    if (tid >= 64) return;
    u64 res[R];
    u32 have = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        res[r] = keys[(u32)lane * R + r];
        if constexpr (!BRUTE) have += (u32)__popcll(ballot64(pm[(u32)lane * R + r] != 0ull));
    }
    bitonic_sort_desc<R>(res, lane);
    if constexpr (BRUTE) {
        write_topk<R, true>(res, k, k, q, id_base, out_ids, out_scores, lane);
    } else {
        const u32 ncand = have < lim ? have : lim;
        const u32 nout = ncand < k ? ncand : k;
        write_topk<R, false>(res, nout, k, q, id_base, out_ids, out_scores, lane);
        if (lane == 0) out_counts[q] = nout;
    }
}

} // namespace

namespace cosdev {

#define WIDE_DISPATCH(R, CALL)                       \
    switch (R) {                                     \
    case 2: { constexpr int RR = 2; CALL; } break;   \
    case 4: { constexpr int RR = 4; CALL; } break;   \
    case 8: { constexpr int RR = 8; CALL; } break;   \
    case 16: { constexpr int RR = 16; CALL; } break; \
    default: return hipErrorInvalidValue;            \
    }

hipError_t launch_flat_select_wide(u32 R, const float *d_scores, u64 s_stride, u32 B, u32 n0, u32 nc, u64 *d_part, u32 S, u64 *d_pool, u64 *d_thr,
                                   hipStream_t st, const ScanMask &m) {
    const u32 seg_len = ((nc + S - 1) / S + 63) / 64 * 64;
    if (m.bits) {
        WIDE_DISPATCH(R, hipLaunchKernelGGL(flat_select_segments_w_masked<RR>, dim3(B, S), dim3(64), 0, st, d_scores, s_stride, B, n0, nc, seg_len, d_part, m))
    } else {
        WIDE_DISPATCH(R, hipLaunchKernelGGL(flat_select_segments_w<RR>, dim3(B, S), dim3(64), 0, st, d_scores, s_stride, B, n0, nc, seg_len, d_part))
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    WIDE_DISPATCH(R, hipLaunchKernelGGL(flat_select_merge_w<RR>, dim3(B), dim3(64), 0, st, (const u64 *)d_part, B, S, d_pool, d_thr))
    return hipGetLastError();
}

hipError_t launch_flat_append_wide(u32 R, const u64 *d_app, u32 *d_appcnt, u32 cap, u32 B, u64 *d_pool, u64 *d_thr, u32 *d_overflow, hipStream_t st) {
    WIDE_DISPATCH(R, hipLaunchKernelGGL(flat_select_append_w<RR>, dim3(B), dim3(64), 0, st, d_app, d_appcnt, cap, B, d_pool, d_thr, d_overflow))
    return hipGetLastError();
}

hipError_t launch_flat_rerank_wide(u32 R, bool brute, const float *Q, u64 q_stride, const float *qmags, u32 B, const float *X, u64 x_stride,
                                   const float *xmags, u32 dim, const u64 *d_pool, u32 ncand_max, u32 k, u32 id_base, u32 *out_ids, float *out_scores,
                                   u32 *out_counts, hipStream_t st) {
    const size_t smem = staged_query_bytes(dim) + (size_t)R * 64 * 8;
#define RERANK_ARGS Q, q_stride, qmags, B, X, x_stride, xmags, dim, d_pool, ncand_max, k, id_base, out_ids, out_scores, out_counts
    if (brute) {
        WIDE_DISPATCH(R, hipLaunchKernelGGL((flat_rerank_w<RR, true>), dim3(B), dim3(256), smem, st, RERANK_ARGS))
    } else {
        WIDE_DISPATCH(R, hipLaunchKernelGGL((flat_rerank_w<RR, false>), dim3(B), dim3(256), smem, st, RERANK_ARGS))
    }
#undef RERANK_ARGS
    return hipGetLastError();
}

#undef WIDE_DISPATCH

} // namespace cosdev
