// kernels_brute_dot.hip — cos_bruteforce_topk_dot: the exact top k by INNER PRODUCT over the resident raw f32 rows, masked or not.
// The flow is cos_bruteforce_topk's (kernels_flat.hip bruteforce_run): the chunk schedule of flat_plan.h, the survivor pools and
// their folds (fold_chunk: kernels_flat.hip, kernels_flat_wide.hip), the row masks (flat_scan.h), a margin rule with an exact second
// pass.  What is its own is the scoring — no norm enters a score — and the rule that says when a pool can be trusted when scores are
// not bounded by 1 (flat_plan.h brute_dot_margin_safe).  Per chunk:
//   brute_dot_gemm          S = Q . X^T on v_mfma_f32_32x32x2_f32, 128 x 128 tiles; unfused (score matrix out), fused (thresholds in raw
//                           dot units held in LDS, survivors appended) and fused + masked
//   brute_dot_exact_scores  the exact pass: every row's dot in the reference's order (dot_engines.h f32_pair_dot), no division
// and per call:
//   brute_dot_xmax_kernel   the largest stored row norm, once per upload (cached on the handle, dropped by cos_flat_ws_release)
//   brute_dot_margin_kernel flags the queries whose pool the MFMA's ranking may have cut wrongly
//   brute_dot_rerank<P>     the pool's rows scored in the reference's order, sorted in LDS, k kept: one wave per query at P = 64, four
//                           waves at P = 128 .. 1024
// The MFMA's k-ordered chain and the reference's eight chains differ in the last bits, so the GEMM only GENERATES candidates: ids and
// scores come from brute_dot_rerank and are the reference-order dot bit for bit.
// Keys: (simkey(dot) << 32 | row), descending, the larger id first on ties — topk_select.h.  simkey of every finite score, negative
// ones included, is at least 0x00800000 (device_common.h: a negative float's bits are inverted, and -FLT_MAX inverts to 0x00800000), so
// the all-zero key of an empty pool slot and the zero threshold of a pool that is not full order below every finite score: pools whose
// every score is negative start from the same zero fill as cosine's.
// Out of scope: the shard set, k above 512, masks that are already on the device, and the f16 and code scans (they keep refusing the
// dot-product metric).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"
#include "exact_rerank.h"
#include "flat_scan.h"

using namespace cosdev;
namespace fp = flat_plan;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- the candidate GEMM -------------------------------------------------------------------------------------------------------------
// Tile 128 queries x 128 rows per four-wave workgroup, each wave 64 x 64 as 2 x 2 MFMA blocks; K panels of 32 floats in LDS rows of 36
// floats (16-byte aligned, conflict-free ds_read_b128 / ds_write_b128), two LDS buffers.  Without the norms and the quotient the
// kernel has registers to spare at two workgroups per CU, and it spends them on the pipeline: a RING OF TWO register stages, so three
// panels are under way at once — panel p is multiplied from LDS, panel p + 1 waits in registers for the other LDS buffer, panel p + 2
// travels HBM -> registers.  A panel is 64 MFMAs of 64 cycles per wave, ~1.7 us: with one register stage a load has to land within one
// panel, which a loaded HBM does not always do; with two it has ~3.4 us.  One barrier per panel, as before.
// A lane's MFMA operand for k-step s of an 8-wide k block is element s of ONE ds_read_b128 (k = 4 * (lane >> 5) + s): the same k
// permutation for both operands, so the sum is over the same products.
constexpr int TM = 128, TN = 128, PK = 32, LDR = PK + 4;
constexpr size_t DOT_GEMM_LDS = 2ull * (TM + TN) * LDR * sizeof(float); // 73 728 B: two workgroups per CU

template <bool VEC /* dim % 4 == 0 and 16-byte aligned rows */, bool FUSED, bool MASKED /* FUSED: a survivor also passes its query's row mask */>
__global__ __launch_bounds__(256) void brute_dot_gemm(const float *__restrict__ Q, u32 B, const float *__restrict__ X, u32 n0, u32 n_chunk, u32 dim,
                                                      float *__restrict__ scores /*[B][s_stride], unfused*/, u64 s_stride, const FusedOut fo) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // Tile order: workgroup ids go round the 8 XCDs (id % 8).  Each XCD is given one contiguous strip of the tile sequence, and the
    // sequence runs query-tile-fastest, so the workgroups that share a 128-row X tile run back to back on one XCD: X streams from HBM
    // once and is shared through that XCD's L2.
    const u32 tiles_m = gridDim.y, total = gridDim.x * tiles_m;
    u32 t = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const u32 per = total / 8, extra = total % 8, xcd = t % 8;
        t = xcd * per + (xcd < extra ? xcd : extra) + t / 8; // strips of per + 1 tiles for the first `extra` XCDs: a bijection for any total
    }
    const u32 row0 = (t % tiles_m) * TM, col0 = (t / tiles_m) * TN;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    // staging: 8 consecutive lanes fetch the 128 B that one row contributes to a panel, 32 rows per pass, 4 passes per operand.  The
    // rows a thread stages do not change from panel to panel: their addresses and their validity are formed once.
    const int sr = tid >> 3, sc = (tid & 7) * 4;
    const float *qrow[4], *xrow[4];
    bool qin[4], xin[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u32 qr = row0 + i * 32 + sr, xr = col0 + i * 32 + sr;
        qin[i] = qr < B;
        xin[i] = xr < n_chunk;
        qrow[i] = Q + (u64)(qin[i] ? qr : 0u) * dim + sc;
        xrow[i] = X + (u64)(n0 + (xin[i] ? xr : 0u)) * dim + sc;
    }
    float4 stage_q[2][4], stage_x[2][4]; // the register ring
    auto load4 = [&](const float *p, bool in, u32 k) {
        if constexpr (VEC) {
            return in && k < dim ? *(const float4 *)(p + (k - sc)) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else { // any dim, rows that are only 4-byte aligned
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = in && k + e < dim ? p[k - sc + e] : 0.f;
            return make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    auto fetch = [&](auto slot, u32 k0) { // panel at k0: HBM -> ring stage `slot`
        constexpr int S = decltype(slot)::value;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            stage_q[S][i] = load4(qrow[i], qin[i], k0 + sc);
            stage_x[S][i] = load4(xrow[i], xin[i], k0 + sc);
        }
    };
    auto stash = [&](auto slot) { // ring stage `slot` -> LDS buffer `slot`
        constexpr int S = decltype(slot)::value;
        float *qs = lds + (size_t)S * (TM + TN) * LDR, *xs = qs + TM * LDR;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *(float4 *)(qs + (i * 32 + sr) * LDR + sc) = stage_q[S][i];
            *(float4 *)(xs + (i * 32 + sr) * LDR + sc) = stage_x[S][i];
        }
    };
    const u32 npanels = (dim + PK - 1) / PK;
    const int orow = lane & 31, okq = (lane >> 5) * 4;
    // panel p (in LDS buffer S = p % 2, ring stage S free again): start panel p + 2 into stage S, multiply panel p, move panel p + 1
    // from stage 1 - S into buffer 1 - S (last read before the previous barrier)
    auto panel = [&](auto slot, u32 p) {
        constexpr int S = decltype(slot)::value;
        if (p + 2 < npanels) fetch(slot, (p + 2) * PK);
        const float *qs = lds + (size_t)S * (TM + TN) * LDR, *xs = qs + TM * LDR;
#pragma unroll
        for (int kb = 0; kb < PK; kb += 8) {
            const float4 a0 = *(const float4 *)(qs + (wr * 64 + orow) * LDR + kb + okq);
            const float4 a1 = *(const float4 *)(qs + (wr * 64 + 32 + orow) * LDR + kb + okq);
            const float4 b0 = *(const float4 *)(xs + (wc * 64 + orow) * LDR + kb + okq);
            const float4 b1 = *(const float4 *)(xs + (wc * 64 + 32 + orow) * LDR + kb + okq);
            const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
            const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int s = 0; s < 4; s++) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], bv0[s], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], bv1[s], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], bv0[s], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], bv1[s], acc[1][1], 0, 0, 0);
            }
        }
        if (p + 1 < npanels) stash(std::integral_constant<int, 1 - S>{});
        __syncthreads();
    };
    const std::integral_constant<int, 0> s0;
    const std::integral_constant<int, 1> s1;
    fetch(s0, 0);
    stash(s0);
    if (npanels > 1) fetch(s1, PK);
    __syncthreads();
    for (u32 p = 0; p < npanels; p += 2) {
        panel(s0, p);
        if (p + 1 < npanels) panel(s1, p + 1);
    }
    // epilogue.  C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if constexpr (FUSED) {
        // Only what beats its query's P-th best so far is kept.  The tile's 128 thresholds are read once into LDS (the panels are dead:
        // the k loop ended with a barrier) as the key and as the score it encodes; an element is screened with one float compare in raw
        // dot units, and the key — which also settles ties by id — is formed only for what passes.  NaN-safe: a score that is not
        // provably below the bar goes on to the key compare.
        u64 *thr_key = (u64 *)lds;                 // [TM]
        float *thr_dot = (float *)(thr_key + TM);  // [TM]
        for (int idx = tid; idx < TM; idx += 256) {
            const u32 row = row0 + idx;
            const u64 key = row < B ? fo.thr[row] : ~0ull; // a row past the batch keeps nothing
            thr_key[idx] = key;
            thr_dot[idx] = row >= B ? __builtin_inff() : key == 0ull ? -__builtin_inff() : simkey_inv((u32)(key >> 32)); // 0 = pool not full
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const u32 col = col0 + wc * 64 + j * 32 + (lane & 31);
                if (col >= n_chunk) continue;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int rl = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const float v = acc[i][j][r];
                    if (!(v < thr_dot[rl])) {
                        const u64 key = score_key(v, n0 + col);
                        if (key > thr_key[rl] && scan_live<MASKED>(fo.m, row0 + (u32)rl, n0 + col)) {
                            const u32 row = row0 + (u32)rl;
                            const u32 pos = atomicAdd(&fo.app_cnt[row], 1u);
                            if (pos < fo.cap) fo.app[(u64)row * fo.cap + pos] = key;
                        }
                    }
                }
            }
    } else {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const u32 col = col0 + wc * 64 + j * 32 + (lane & 31);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const u32 row = row0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (row < B && col < n_chunk) scores[(u64)row * s_stride + col] = acc[i][j][r];
                }
            }
    }
}

// an unfused chunk has no masked form: its selection applies the mask
using DotGemmKernel = decltype(&brute_dot_gemm<true, false, false>);
DotGemmKernel dot_gemm_kernel(bool vec, bool fused, bool masked) {
    if (!fused) return vec ? brute_dot_gemm<true, false, false> : brute_dot_gemm<false, false, false>;
    if (!masked) return vec ? brute_dot_gemm<true, true, false> : brute_dot_gemm<false, true, false>;
    return vec ? brute_dot_gemm<true, true, true> : brute_dot_gemm<false, true, true>;
}
hipError_t dot_gemm_allow_lds() {
    hipError_t e = hipSuccess;
    for (int vec = 0; vec < 2; vec++)
        for (int fused = 0; fused < 2; fused++)
            for (int masked = 0; masked <= fused && e == hipSuccess; masked++)
                e = hipFuncSetAttribute((const void *)dot_gemm_kernel(vec, fused, masked), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DOT_GEMM_LDS);
    return e;
}
// dots of rows [n0, n0 + nc) of X with the B queries
hipError_t launch_dot_gemm(bool vec, bool fused, bool masked, const float *Q, u32 B, const float *X, u32 n0, u32 nc, u32 dim, float *scores, u64 s_stride,
                           const FusedOut &fo, hipStream_t st) {
    const dim3 grid((nc + TN - 1) / TN, (B + TM - 1) / TM);
    hipLaunchKernelGGL(dot_gemm_kernel(vec, fused, masked), grid, dim3(256), DOT_GEMM_LDS, st, Q, B, X, n0, nc, dim, scores, s_stride, fo);
    return hipGetLastError();
}

// ---- the exact pass's scores ----------------------------------------------------------------------------------------------------------
// scores[q][c] = the dot of row n0 + c in the REFERENCE's order (f32_pair_dot: eight chains, a pairwise tree, a scalar tail) — the value
// brute_dot_rerank ranks and returns, so the selection over this matrix keeps the exact top P.  A lane pair per row, 128 rows per pass
// of the four waves, DOT_EXACT_ROWS rows per workgroup so that the query is staged once per 8 passes.  Grid (B, ceil(n_chunk / DOT_EXACT_ROWS)).
constexpr u32 DOT_EXACT_ROWS = 1024;
__global__ __launch_bounds__(256) void brute_dot_exact_scores(const float *__restrict__ Q, const float *__restrict__ X, u32 n0, u32 n_chunk, u32 dim,
                                                              float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const u32 tid = threadIdx.x, q = blockIdx.x;
    for (u32 i = tid; i < dim; i += 256) qf[i] = Q[(u64)q * dim + i];
    __syncthreads();
    const u32 c_begin = blockIdx.y * DOT_EXACT_ROWS, c_end = c_begin + DOT_EXACT_ROWS < n_chunk ? c_begin + DOT_EXACT_ROWS : n_chunk;
    for (u32 c0 = c_begin; c0 < c_end; c0 += 128) { // (workgroup-uniform: both lanes of a pair run every pass)
        const u32 col = c0 + (tid >> 1);
        const bool valid = col < n_chunk;
        const float dp = f32_pair_dot(X + (u64)(n0 + (valid ? col : 0u)) * dim, qf, dim, (int)(tid & 1));
        if (valid && (tid & 1) == 0) scores[(u64)q * s_stride + col] = dp;
    }
}
hipError_t launch_dot_exact_scores(const float *Q, u32 B, const float *X, u32 n0, u32 nc, u32 dim, float *scores, u64 s_stride, hipStream_t st) {
    hipLaunchKernelGGL(brute_dot_exact_scores, dim3(B, (nc + DOT_EXACT_ROWS - 1) / DOT_EXACT_ROWS), dim3(256), staged_query_bytes(dim), st, Q, X, n0, nc, dim, scores,
                       s_stride);
    return hipGetLastError();
}

// ---- the margin rule --------------------------------------------------------------------------------------------------------------------
// *out = the bits of the largest |x| among n norms (norms are >= 0, where the order of the bits is the order of the values; a NaN norm
// ends above every number and makes every product NaN: no pool is trusted).  *out is zeroed before the launch.
__global__ void brute_dot_xmax_kernel(const float *__restrict__ mags, u32 n, u32 *__restrict__ out) {
    u32 m = 0u;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 b = __float_as_uint(mags[i]) & 0x7FFFFFFFu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const u32 o = (u32)__shfl_xor((int)m, s, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// flags[q] = 1 and *n_flagged += 1 where flat_plan.h brute_dot_margin_safe says no.  The pool is sorted descending, P keys, at every
// width pool[q][e].  One thread per query.
__global__ void brute_dot_margin_kernel(const u64 *__restrict__ pool_mem, u32 P, u32 B, u32 k, u32 dim, const float *__restrict__ qmags,
                                        const u32 *__restrict__ xmax_bits, u32 *__restrict__ flags, u32 *__restrict__ n_flagged) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    const u64 kth = pool_mem[(u64)q * P + k - 1], pth = pool_mem[(u64)q * P + P - 1];
    const bool safe = fp::brute_dot_margin_safe(simkey_inv((u32)(kth >> 32)), simkey_inv((u32)(pth >> 32)), dim, qmags[q], __uint_as_float(*xmax_bits),
                                                (u32)(pth >> 32) != 0u);
    flags[q] = safe ? 0u : 1u;
    if (!safe) atomicAdd(n_flagged, 1u);
}

// ---- re-score of the pool, sort, top k --------------------------------------------------------------------------------------------------
// One workgroup per query: one wave at P = 64, four waves at P = 128 .. 1024.  A lane pair scores one survivor in the reference's order
// (no norm, no quotient: the dot is the score), the P keys are sorted in LDS by the whole workgroup (topk_select.h
// lds_bitonic_sort_desc: log^2(P) rounds of one compare-exchange per thread and pair, no key held in registers), the first k go out;
// ~0 / 0.0 where the pool has fewer than k survivors (a masked query with fewer live rows).
template <u32 P>
__global__ __launch_bounds__(P == 64 ? 64 : 256) void brute_dot_rerank(const float *__restrict__ Q, u32 B, const float *__restrict__ X, u32 dim,
                                                                        const u64 *__restrict__ pool_mem, u32 k, u32 id_base, u32 *__restrict__ out_ids,
                                                                        float *__restrict__ out_scores) {
    constexpr u32 NT = P == 64 ? 64 : 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;                           // [dim], padded to 16 B
    u64 *keys = (u64 *)(smem_raw + staged_query_bytes(dim)); // [P]
    const u32 tid = threadIdx.x, q = blockIdx.x;
    for (u32 i = tid; i < dim; i += NT) qf[i] = Q[(u64)q * dim + i];
    __syncthreads();
    const u64 *pm = pool_mem + (u64)q * P;
    for (u32 c0 = 0; c0 < P; c0 += NT / 2) { // (P is a multiple of NT / 2: every lane runs every pass)
        const u32 c = c0 + (tid >> 1);
        const u64 pk = pm[c];
        const bool valid = (u32)(pk >> 32) != 0u;
        const u32 sid = (u32)pk;
        const float dp = f32_pair_dot(X + (u64)(valid ? sid : 0u) * dim, qf, dim, (int)(tid & 1));
        if ((tid & 1) == 0) keys[c] = valid ? score_key(dp, sid) : 0ull;
    }
    lds_bitonic_sort_desc<P>(keys);
    for (u32 e = tid; e < k; e += NT) {
        const u64 key = keys[e];
        out_ids[(u64)q * k + e] = key != 0ull ? (u32)key + id_base : 0xFFFFFFFFu;
        out_scores[(u64)q * k + e] = key != 0ull ? simkey_inv((u32)(key >> 32)) : 0.0f;
    }
}
hipError_t launch_dot_rerank(u32 P, const float *Q, u32 B, const float *X, u32 dim, const u64 *pool, u32 k, u32 id_base, u32 *out_ids, float *out_scores,
                             hipStream_t st) {
    const size_t smem = staged_query_bytes(dim) + (size_t)P * 8;
#define DOT_RERANK(PP) hipLaunchKernelGGL(brute_dot_rerank<PP>, dim3(B), dim3(PP == 64 ? 64 : 256), smem, st, Q, B, X, dim, pool, k, id_base, out_ids, out_scores)
    switch (P) {
    case 64: DOT_RERANK(64); break;
    case 128: DOT_RERANK(128); break;
    case 256: DOT_RERANK(256); break;
    case 512: DOT_RERANK(512); break;
    case 1024: DOT_RERANK(1024); break;
    default: return hipErrorInvalidValue;
    }
#undef DOT_RERANK
    return hipGetLastError();
}

// the largest stored row norm on the device, computed once per upload: cos_flat_ws_release (every upload, cos_index_append, destroy)
// drops it with the code scan's cached flags
hipError_t dot_xmax_ensure(cos_index *ix, hipStream_t st) {
    if (ix->brute_xmax_valid && ix->brute_xmax_n == ix->n) return hipSuccess;
    hipError_t e = ix->brute_xmax.grow(1);
    if (e == hipSuccess) e = hipMemsetAsync(ix->brute_xmax.p, 0, 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(brute_dot_xmax_kernel, dim3(ix->n > 65536u ? 256u : 16u), dim3(256), 0, st, (const float *)ix->d_raw_mags.p, ix->n, ix->brute_xmax.p);
    e = hipGetLastError();
    if (e == hipSuccess) { ix->brute_xmax_valid = true; ix->brute_xmax_n = ix->n; }
    return e;
}

// cos_bruteforce_topk_dot, masked or not.  The steps of bruteforce_run (kernels_flat.hip) with this file's kernels: the plan
// (fp::brute_scan), the chunks (run_chunks: a fused attempt, repeated unfused when an append buffer overflowed), the margin flags, the
// re-score, the counts; the flagged queries are answered again by this function on their sub-batch with exact_pass set — every chunk
// unfused, its score matrix written by brute_dot_exact_scores — and those rows replace the first answer's.
int32_t brute_dot_run(cos_index *ix, const float *queries, uint32_t B, uint32_t k, const cos_scan_mask *mask, uint32_t *out_ids, float *out_scores,
                      uint32_t *out_counts, bool exact_pass = false) {
    if (!ix || !queries || !out_ids || !out_scores || B == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (mask && !out_counts) return cos_fail(COS_ERR_INVALID, "out_counts is NULL with a mask");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    if (int32_t krc = fp::check_brute_k(k, ix->n)) return cos_fail(krc, "k must be in [1, min(512, n)]");
    MaskPlan mp;
    if (int32_t mrc = scan_mask_plan(mask, B, mp)) return mrc;
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 dim = ix->p.dim, n = ix->n;
    const int exact_mode = exact_pass ? (int)fp::BRUTE_EXACT_ALWAYS : (int)tune_or(TUNE_FLAT_BRUTE_EXACT, fp::BRUTE_EXACT_BY_RULE);
    const bool exact = exact_mode >= fp::BRUTE_EXACT_ALWAYS, by_rule = exact_mode == fp::BRUTE_EXACT_BY_RULE;
    const fp::Scan plan = fp::brute_scan(n, B, k, exact || tune_or(TUNE_FLAT_UNFUSED, 0) != 0);
    const u32 P = plan.P;
    const u64 s_stride = fp::score_stride(plan.unfused);
    DevArr<float> d_q, d_qm, d_scores, d_os, d_dummy;
    DevArr<u64> d_pool, d_part, d_thr, d_app;
    DevArr<u32> d_oi, d_appcnt, d_over, d_oc, d_flag;
    DevArr<uint8_t> d_codes;
    MaskBufs mb;
    hipStream_t st = ix->own_stream;
    HIP_TRY(d_q.alloc((size_t)B * dim));
    HIP_TRY(d_part.alloc((size_t)B * fp::select_segments(B, plan.unfused) * P));
    HIP_TRY(d_scores.alloc((size_t)B * s_stride));
    HIP_TRY(d_pool.alloc((size_t)B * P));
    HIP_TRY(d_thr.alloc(B));
    if (plan.allow_fused) HIP_TRY(d_app.alloc((size_t)B * plan.app_cap()));
    HIP_TRY(d_appcnt.alloc(B));
    HIP_TRY(d_over.alloc(2)); // [the fused path's overflow flag, queries the margin rule flagged]
    HIP_TRY(d_oi.alloc((size_t)B * k));
    HIP_TRY(d_os.alloc((size_t)B * k));
    if (mp.masked) HIP_TRY(d_oc.alloc(B));
    if (by_rule) { // the rule's |q|
        HIP_TRY(d_flag.alloc(B));
        HIP_TRY(d_qm.alloc(B));
        HIP_TRY(d_dummy.alloc(B));
        HIP_TRY(d_codes.alloc((size_t)B * staged_query_bytes(dim)));
    }
    // (from here on a ladder: the stream is drained below on every path before the buffers and `hover` go out of scope)
    hipError_t e = hipMemcpyAsync(d_q, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, st);
    // |q| as the handle keeps |x|: the F32 quantize kernel's sequential raw norm
    if (e == hipSuccess && by_rule) e = launch_quantize_rows(ENG_F32, d_q, dim, B, dim, 0.f, 0.f, d_codes, staged_query_bytes(dim), d_dummy, d_qm, st);
    if (e == hipSuccess && by_rule) e = dot_xmax_ensure(ix, st); // the largest norm of ALL rows: a valid, looser bound for a masked call
    if (e == hipSuccess) e = dot_gemm_allow_lds();
    ScanMask sm{nullptr, nullptr, 0u};
    const u32 *d_uni = nullptr;
    if (e == hipSuccess && mp.masked) e = scan_mask_upload(ix, mask, mp, B, mb, st, sm, &d_uni);
    // float4 staging needs 16-byte aligned rows: dim % 4 == 0 and an aligned base (a borrowed table need not be)
    const bool vec = dim % 4 == 0 && ((uintptr_t)ix->d_raw & 15) == 0;
    u32 n_flagged = 0;
    for (int attempt = 0; attempt < 2 && e == hipSuccess; attempt++) {
        // empty pools, thresholds "not full", counters and both flags zero: the zero key orders below every finite score (header comment)
        e = launch_flat_reset(d_pool, (u64)B * P, d_thr, d_appcnt, B, d_over, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_over.p + 1, 0, 4, st);
        const ScanBufs bufs{d_scores, s_stride, d_part, d_pool, d_thr, d_app, d_appcnt, d_over, sm};
        const FusedOut fo = bufs.fused_out(plan, nullptr);
        if (e == hipSuccess)
            e = run_chunks(plan, attempt, bufs, st, [&](const fp::Chunk &c) {
                if (exact) return launch_dot_exact_scores(d_q, B, ix->d_raw, c.n0, c.nc, dim, d_scores, s_stride, st);
                return launch_dot_gemm(vec, c.fused, mp.masked, d_q, B, ix->d_raw, c.n0, c.nc, dim, d_scores, s_stride, fo, st);
            });
        if (e == hipSuccess && by_rule) { // the pools are final (or about to be repeated): ranks k and P of each
            hipLaunchKernelGGL(brute_dot_margin_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const u64 *)d_pool, P, B, k, dim, (const float *)d_qm.p,
                               (const u32 *)ix->brute_xmax.p, d_flag.p, d_over.p + 1);
            e = hipGetLastError();
        }
        u32 hover[2] = {0u, 0u};
        if (e == hipSuccess) e = hipMemcpyAsync(hover, d_over, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        n_flagged = hover[1];
        if (e != hipSuccess || !plan.fused(attempt) || hover[0] == 0) break; // done; otherwise the append buffer overflowed: repeat unfused
    }
    if (e == hipSuccess) e = launch_dot_rerank(P, d_q, B, ix->d_raw, dim, d_pool, k, ix->p.id_base, d_oi, d_os, st);
    if (e == hipSuccess) e = hipMemcpyAsync(out_ids, d_oi, (size_t)B * k * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(out_scores, d_os, (size_t)B * k * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && mp.masked) { // a query may have fewer live rows than k
        e = launch_pool_count(d_pool, P, B, k, d_oc, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_counts, d_oc, (size_t)B * 4, hipMemcpyDeviceToHost, st);
    }
    std::vector<u32> h_flag;
    if (e == hipSuccess && n_flagged) {
        h_flag.resize(B);
        e = hipMemcpyAsync(h_flag.data(), d_flag.p, (size_t)B * 4, hipMemcpyDeviceToHost, st);
    }
    { // drained on every path: the buffers above and the caller's arrays are free again
        const hipError_t se = hipStreamSynchronize(st);
        if (e == hipSuccess) e = se;
    }
    HIP_TRY(e);
    if (!mp.masked && out_counts) std::fill(out_counts, out_counts + B, k); // k <= n: every list is full
    if (!exact_pass) ix->brute_last = cos_brute_stats{(u32)sizeof(cos_brute_stats), B, exact ? B : n_flagged, P};
    if (n_flagged == 0) return COS_OK;
    // the flagged queries again, exactly: the big buffers of this pass go first, the sub-batch's answer replaces theirs
    d_scores.reset(); d_part.reset(); d_app.reset(); d_pool.reset();
    std::vector<u32> sel;
    for (u32 b = 0; b < B; b++)
        if (h_flag[b]) sel.push_back(b);
    const u32 Bx = (u32)sel.size();
    std::vector<float> xq((size_t)Bx * dim), xs((size_t)Bx * k);
    std::vector<u32> xi((size_t)Bx * k), xc(Bx), xqm;
    for (u32 i = 0; i < Bx; i++) memcpy(xq.data() + (size_t)i * dim, queries + (size_t)sel[i] * dim, (size_t)dim * 4);
    cos_scan_mask xmask;
    if (mask) {
        xmask = *mask;
        if (mask->query_mask) {
            for (u32 i = 0; i < Bx; i++) xqm.push_back(mask->query_mask[sel[i]]);
            xmask.query_mask = xqm.data();
        }
    }
    if (int32_t xrc = brute_dot_run(ix, xq.data(), Bx, k, mask ? &xmask : nullptr, xi.data(), xs.data(), xc.data(), true)) return xrc;
    for (u32 i = 0; i < Bx; i++) {
        memcpy(out_ids + (size_t)sel[i] * k, xi.data() + (size_t)i * k, (size_t)k * 4);
        memcpy(out_scores + (size_t)sel[i] * k, xs.data() + (size_t)i * k, (size_t)k * 4);
        if (out_counts) out_counts[sel[i]] = xc[i]; // (an unmasked call's counts are k in both passes)
    }
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_bruteforce_topk_dot(cos_index *ix, const float *queries, uint32_t B, uint32_t k, const cos_scan_mask *mask, uint32_t *out_ids,
                                           float *out_scores, uint32_t *out_counts) {
    return brute_dot_run(ix, queries, B, k, mask, out_ids, out_scores, out_counts);
}
