// kernels_flat.hip — exhaustive (flat) cosine scan of the resident raw vectors: the one genuine dense
// contraction of the path, S = Q[B x d] . X^T[d x N], on the f32 MFMA
// (v_mfma_f32_32x32x2_f32: exact f32 products, k-ordered fmaf chain, 157 TF peak on gfx950).
// Used for recall ground truth and as the exhaustive per-shard mode.  Pipeline per N-chunk:
//   flat_gemm_f32      128x128 tile per workgroup (4 waves, 2x2 MFMA tiles of 32x32 per wave), LDS-staged K panels,
//                      epilogue divides by |q|*|x| and writes cosine scores [B][chunk]
//   flat_select_*      waves per (query, segment) keep a top-64 (sorted register pool, threshold filter); merged per query
//   flat_rescore       exact reference-order re-score (dot_product_f32_simd order) of the 64 survivors -> top-k
// MFMA accumulation order differs from the reference's 8-lane tree in the last ulp, so the GEMM only
// GENERATES candidates (a pool of P >= 2k); the returned ids/scores come from the reference-order kernel
// and are bit-identical to the oracle's brute force.  The pool is trusted only while its P-th GEMM score lies more
// than twice a derived error bound under its k-th (flat_plan.h brute_margin_safe; brute_margin_kernel flags the rest):
// a query with more than P - k rows that close to the k-th score (copies, scaled copies of one vector) is answered by the
// exact path — flat_exact_scores writes the reference-order score of EVERY row where the GEMM wrote its own, the same
// selection and re-score follow (bruteforce_run, exact_pass).
// Calls that need more than 64 survivors (k > 32 here, top_k > 12 in the code scan) keep pools of 128 .. 1024 keys: the kernels
// behind the GEMMs are then those of kernels_flat_wide.hip, the GEMMs and the flow below are the same.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "engine_internal.h"
#include "exact_rerank.h"
#include "flat_scan.h"

using namespace cosdev;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 32, LDT = BK + 4; // 36-float rows: 16 B aligned, conflict-free ds_read/ds_write_b128
constexpr int SEL = 64;                                  // survivors per query
constexpr size_t GEMM_SMEM = 2ull * (BM + BN) * LDT * sizeof(float); // double-buffered Q and X panels: 73 728 B -> 2 workgroups per CU

// S = Q . X^T on v_mfma_f32_32x32x2_f32.  128x128 tile per 4-wave workgroup (each wave 64x64 = 2x2 MFMA blocks), K panels
// of 32 double-buffered in LDS: panel p+1 travels HBM -> registers while panel p is multiplied, then registers -> LDS, one
// barrier per panel.  A lane's MFMA operand for k-step s of an 8-wide k block is element s of ONE ds_read_b128
// (k = 4*(lane>>5) + s): the k permutation is the same for both operands, so the sum is unchanged.
template <bool VEC, bool FUSED, bool MASKED = false /* FUSED: a survivor also passes its query's row mask (flat_scan.h ScanMask) */>
__global__ __launch_bounds__(256) void flat_gemm_f32(const float *__restrict__ Q, u64 q_stride, const float *__restrict__ qmags, u32 B,
                                                     const float *__restrict__ X, u64 x_stride, const float *__restrict__ xmags, u32 n0,
                                                     u32 n_chunk, u32 dim, float *__restrict__ scores /*[B][n_chunk_padded]*/, u64 s_stride,
                                                     const FusedOut fo /*FUSED: thresholds in, survivors out (see flat_codes_gemm_i8)*/) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // XCD-aware tile order: consecutive workgroup ids land on different XCDs (id % 8); remap so that each XCD walks a
    // contiguous strip of the tile sequence, and order the sequence query-tile-fastest: the tiles_m workgroups that share
    // one 128-row X tile run back to back on one XCD, so X streams from HBM once and is re-used from that XCD's L2
    // (the query panel, a few MB, stays in L2 / Infinity Cache).
    const u32 tiles_n = gridDim.x, tiles_m = gridDim.y;
    u32 wg = blockIdx.y * tiles_n + blockIdx.x;
    const u32 total = tiles_n * tiles_m;
    {
        const u32 q = total / 8, r = total % 8, xcd = wg % 8, idx = wg / 8;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx; // bijective for any total
    }
    const u32 tm = wg % tiles_m, tn = wg / tiles_m;
    const u32 row0 = tm * BM, col0 = tn * BN;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    // staging: 8 consecutive lanes fetch one row's 128 B of the panel (float4 each), 32 rows per pass, 4 passes per operand
    const int sr = tid >> 3, sc = (tid & 7) * 4;
    float4 ra[4], rb[4];
    auto fetch = [&](u32 k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const u32 qr = row0 + i * 32 + sr, xr = col0 + i * 32 + sr, k = k0 + sc;
            const float *pa = Q + (u64)qr * q_stride + k;
            const float *pb = X + (u64)(n0 + xr) * x_stride + k;
            if constexpr (VEC) { // dim % 4 == 0 and 16 B aligned rows
                ra[i] = (qr < B && k < dim) ? *(const float4 *)pa : make_float4(0.f, 0.f, 0.f, 0.f);
                rb[i] = (xr < n_chunk && k < dim) ? *(const float4 *)pb : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                float a[4], b[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    a[e] = (qr < B && k + e < dim) ? pa[e] : 0.f;
                    b[e] = (xr < n_chunk && k + e < dim) ? pb[e] : 0.f;
                }
                ra[i] = make_float4(a[0], a[1], a[2], a[3]);
                rb[i] = make_float4(b[0], b[1], b[2], b[3]);
            }
        }
    };
    auto stash = [&](int buf) {
        float *As = gsm + (size_t)buf * (BM + BN) * LDT, *Bs = As + BM * LDT;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *(float4 *)(As + (i * 32 + sr) * LDT + sc) = ra[i];
            *(float4 *)(Bs + (i * 32 + sr) * LDT + sc) = rb[i];
        }
    };

    const u32 npanels = (dim + BK - 1) / BK;
    fetch(0);
    stash(0);
    __syncthreads();
    const int orow = lane & 31, okq = (lane >> 5) * 4;
    for (u32 p = 0; p < npanels; p++) {
        if (p + 1 < npanels) fetch((p + 1) * BK);
        const float *As = gsm + (size_t)(p & 1) * (BM + BN) * LDT, *Bs = As + BM * LDT;
#pragma unroll
        for (int kb = 0; kb < BK; kb += 8) {
            const float4 a0 = *(const float4 *)(As + (wr * 64 + orow) * LDT + kb + okq);
            const float4 a1 = *(const float4 *)(As + (wr * 64 + 32 + orow) * LDT + kb + okq);
            const float4 b0 = *(const float4 *)(Bs + (wc * 64 + orow) * LDT + kb + okq);
            const float4 b1 = *(const float4 *)(Bs + (wc * 64 + 32 + orow) * LDT + kb + okq);
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
        if (p + 1 < npanels) stash((p + 1) & 1); // the other buffer: last read before the previous barrier
        __syncthreads();
    }
    // epilogue: C/D layout of 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if constexpr (FUSED) {
        // The score matrix never reaches HBM: only what beats the query's 64th best so far is kept.  Per-row filter state lives in LDS
        // (the operand panels are dead: the k loop ended with a barrier) and a reciprocal-based estimate screens the 64 elements a
        // lane holds — the exact quotient, the key and the compare are formed only for estimates within 4e-6 (relative) of the
        // row's threshold or above.  The first version of this epilogue loaded |q| and the threshold from global memory per
        // ELEMENT and waited for each pair: 64 dependent L2 round trips per lane per tile, as long as the tile's MFMAs.
        u64 *thr_key = (u64 *)gsm;                 // [BM]
        float *thr_lo = (float *)(thr_key + BM);   // [BM] estimate a candidate must reach to be worth the exact quotient
        float *rq = thr_lo + BM;                   // [BM] ~1 / |q|
        float *qm = rq + BM;                       // [BM] |q|
        for (int idx = tid; idx < BM; idx += 256) {
            const u32 row = row0 + idx;
            const u64 k = row < B ? fo.thr[row] : ~0ull;
            const float tsc = simkey_inv((u32)(k >> 32));
            const float qv = row < B ? qmags[row] : 1.0f;
            thr_key[idx] = k;
            thr_lo[idx] = k == 0ull ? -__builtin_inff() : tsc - 4e-6f * __builtin_fabsf(tsc); // 0 = pool not full: everything passes
            qm[idx] = qv;
            rq[idx] = __builtin_amdgcn_rcpf(qv);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const u32 col = col0 + wc * 64 + j * 32 + (lane & 31);
                const bool cv = col < n_chunk;
                const float xm = cv ? xmags[n0 + col] : 1.0f;
                const float rx = __builtin_amdgcn_rcpf(xm);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int rl = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const float est = acc[i][j][r] * rx * rq[rl];
                    // NaN-safe: an estimate that is not provably below the bar (incl. 0 * inf of a zero-norm operand) takes the exact path
                    if (row0 + (u32)rl < B && cv && !(est < thr_lo[rl])) {
                        const float sc = x86_div(acc[i][j][r], qm[rl] * xm);
                        const u64 key = score_key(sc, n0 + col);
                        if (key > thr_key[rl] && scan_live<MASKED>(fo.m, row0 + (u32)rl, n0 + col)) {
                            const u32 row = row0 + (u32)rl;
                            const u32 pos = atomicAdd(&fo.app_cnt[row], 1u);
                            if (pos < fo.cap) fo.app[(u64)row * fo.cap + pos] = key;
                        }
                    }
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32 col = col0 + wc * 64 + j * 32 + (lane & 31);
            const float xm = col < n_chunk ? xmags[n0 + col] : 1.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const u32 row = row0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < B && col < n_chunk) scores[(u64)row * s_stride + col] = x86_div(acc[i][j][r], qmags[row] * xm);
            }
        }
}

// Selection of the SEL best of a chunk in two steps so that a small query batch still fills the chip:
//   flat_select_segments  grid (B, S): one wave per (query, segment of the chunk) keeps the segment's top-SEL
//                         (sorted register pool, ballot threshold filter) -> part[B][S][SEL]
//   flat_select_merge     one wave per query folds the S sorted partial lists into the running pool[B][SEL]
// keys = (simkey(score), global id): ties go to the larger id, like everywhere else.
// MASKED (flat_select_segments_masked): a row outside the query's mask gives the empty key
template <bool MASKED>
__device__ __forceinline__ void select_segments_body(const float *__restrict__ scores, u64 s_stride, u32 B, u32 n0, u32 n_chunk, u32 seg_len,
                                                     u64 *__restrict__ part /*[B][S][64]*/, const ScanMask &m) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x, seg = blockIdx.y, S = gridDim.y;
    if (q >= B) return;
    Pool<1> pool;
    pool.clear();
    u64 thr = 0ull; // SEL-th best so far (0 while not full)
    const float *sr = scores + (u64)q * s_stride;
    const u32 c0 = seg * seg_len, c1 = (c0 + seg_len < n_chunk) ? c0 + seg_len : n_chunk;
    for (u32 c = c0; c < c1; c += 64) {
        const u32 col = c + lane;
        u64 key = 0ull;
        if (col < c1 && scan_live<MASKED>(m, q, n0 + col)) key = score_key(sr[col], n0 + col);
        pool_fold_lanes<1>(pool, thr, key, lane);
    }
    part[((u64)q * S + seg) * SEL + lane] = pool.e[0];
}
__global__ __launch_bounds__(64) void flat_select_segments(const float *__restrict__ scores, u64 s_stride, u32 B, u32 n0, u32 n_chunk, u32 seg_len,
                                                           u64 *__restrict__ part /*[B][S][64]*/) {
    select_segments_body<false>(scores, s_stride, B, n0, n_chunk, seg_len, part, ScanMask{nullptr, nullptr, 0u});
}
__global__ __launch_bounds__(64) void flat_select_segments_masked(const float *__restrict__ scores, u64 s_stride, u32 B, u32 n0, u32 n_chunk, u32 seg_len,
                                                                  u64 *__restrict__ part /*[B][S][64]*/, const ScanMask m) {
    select_segments_body<true>(scores, s_stride, B, n0, n_chunk, seg_len, part, m);
}

__global__ __launch_bounds__(64) void flat_select_merge(const u64 *__restrict__ part, u32 B, u32 S, u64 *__restrict__ pool_mem /*[B][64]*/,
                                                        u64 *__restrict__ thr_out /*optional [B]: the SEL-th best key so far (0 while the pool is not full)*/) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    Pool<1> pool;
    pool.e[0] = pool_mem[(u64)q * SEL + lane];
    u64 thr = readlane_u64(pool.e[0], SEL - 1);
    for (u32 sgm = 0; sgm < S; sgm++) {
        const u64 key = part[((u64)q * S + sgm) * SEL + lane];
        pool_fold_lanes<1>(pool, thr, key, lane);
    }
    pool_mem[(u64)q * SEL + lane] = pool.e[0];
    if (thr_out && lane == 0) thr_out[q] = thr;
}

// Fused scans (flat_codes_gemm_i8<ENG, true>): the GEMM epilogue appended only the candidates that beat the query's
// threshold to app[B][cap]; one wave per query folds them into the pool, publishes the new threshold and clears the counter.
// A counter above `cap` means entries were dropped: the flag makes the host repeat the search on the unfused path.
__global__ __launch_bounds__(64) void flat_select_append(const u64 *__restrict__ app, u32 *__restrict__ app_cnt, u32 cap, u32 B, u64 *__restrict__ pool_mem,
                                                         u64 *__restrict__ thr_out, u32 *__restrict__ overflow) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    Pool<1> pool;
    pool.e[0] = pool_mem[(u64)q * SEL + lane];
    u64 thr = readlane_u64(pool.e[0], SEL - 1);
    u32 cnt = app_cnt[q];
    if (cnt > cap) { if (lane == 0) atomicOr(overflow, 1u); cnt = cap; }
    for (u32 c = 0; c < cnt; c += 64) {
        const u64 key = c + lane < cnt ? app[(u64)q * cap + c + lane] : 0ull;
        pool_fold_lanes<1>(pool, thr, key, lane);
    }
    pool_mem[(u64)q * SEL + lane] = pool.e[0];
    if (lane == 0) { thr_out[q] = thr; app_cnt[q] = 0; }
}

// S = segments per query (flat_plan.h select_segments)
static hipError_t launch_select(const float *d_scores, u64 s_stride, u32 B, u32 n0, u32 nc, u64 *d_part, u32 S, u64 *d_pool, hipStream_t st,
                                u64 *d_thr, const ScanMask &m) {
    const u32 seg_len = ((nc + S - 1) / S + 63) / 64 * 64;
    if (m.bits) hipLaunchKernelGGL(flat_select_segments_masked, dim3(B, S), dim3(64), 0, st, d_scores, s_stride, B, n0, nc, seg_len, d_part, m);
    else hipLaunchKernelGGL(flat_select_segments, dim3(B, S), dim3(64), 0, st, d_scores, s_stride, B, n0, nc, seg_len, d_part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flat_select_merge, dim3(B), dim3(64), 0, st, (const u64 *)d_part, B, S, d_pool, d_thr);
    return hipGetLastError();
}

// any zero among n floats -> *flag = 1 (cosine zero-norm screening without copying the norms to the host)
__global__ void any_zero_kernel(const float *__restrict__ v, u32 n, u32 *__restrict__ flag) {
    bool z = false;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) z |= (v[i] == 0.0f);
    if (__any(z) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ---- row masks of the masked scans (flat_scan.h ScanMask) ----
// The call's effective masks: eff[g] = user[g] (all ones without an allow-list) AND NOT deleted (when asked), bits at and past n cleared;
// uni = the OR of them, the rows that some query of the call can be given (the masked zero-norm screen reads it).  One thread per word.
__global__ void scan_mask_build_kernel(const u32 *__restrict__ user /*[G][words] or null*/, const u32 *__restrict__ deleted /*[words] or null*/, u32 G,
                                       u32 words, u32 n, u32 *__restrict__ eff /*[G][words]*/, u32 *__restrict__ uni /*[words]*/) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    u32 keep = deleted ? ~deleted[w] : ~0u;
    if (w == words - 1 && (n & 31u)) keep &= (1u << (n & 31u)) - 1u;
    u32 u = 0;
    for (u32 g = 0; g < G; g++) {
        const u32 v = (user ? user[(u64)g * words + w] : ~0u) & keep;
        eff[(u64)g * words + w] = v;
        u |= v;
    }
    uni[w] = u;
}
// any_zero_kernel over the rows of a bitmap
__global__ void any_zero_masked_kernel(const float *__restrict__ v, u32 n, const u32 *__restrict__ rows, u32 *__restrict__ flag) {
    bool z = false;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        z |= ((rows[i >> 5] >> (i & 31u)) & 1u) != 0u && v[i] == 0.0f;
    if (__any(z) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
// masked brute force: out_counts[q] = min(k, survivors in the query's pool) — the pool (P >= 2k keys) holds every live row while there are
// fewer than P of them.  One wave per query.
__global__ __launch_bounds__(64) void pool_count_kernel(const u64 *__restrict__ pool_mem, u32 P, u32 B, u32 k, u32 *__restrict__ out_counts) {
    const u32 q = blockIdx.x;
    if (q >= B) return;
    u32 have = 0;
    for (u32 c = threadIdx.x; c < P; c += 64) have += (u32)(pool_mem[(u64)q * P + c] >> 32) != 0u ? 1u : 0u;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) have += (u32)__shfl_xor((int)have, m, 64);
    if (threadIdx.x == 0) out_counts[q] = have < k ? have : k;
}

// ---- the handle's deleted set: one bit per row (cos_index::d_deleted) ----
__global__ void deleted_mark_kernel(const u32 *__restrict__ ids, u32 m, u32 *__restrict__ bits) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) atomicOr(&bits[ids[t] >> 5], 1u << (ids[t] & 31u));
}
__global__ void popcount_kernel(const u32 *__restrict__ bits, u32 words, u32 *__restrict__ out) {
    u32 c = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) c += (u32)__popc(bits[i]);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) c += (u32)__shfl_xor((int)c, m, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// one launch instead of four memsets in front of every scan: the survivor pools, the thresholds, the append counters, the overflow flag
__global__ void flat_reset_kernel(u64 *__restrict__ pool, u64 n_pool, u64 *__restrict__ thr, u32 *__restrict__ appcnt, u32 B, u32 *__restrict__ overflow) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x, step = (u64)gridDim.x * blockDim.x;
    for (u64 i = t; i < n_pool; i += step) pool[i] = 0ull;
    for (u64 i = t; i < B; i += step) { thr[i] = 0ull; appcnt[i] = 0u; }
    if (t == 0) *overflow = 0u;
}
// the call's results and its two flags side by side, for one copy back
__global__ void flat_pack_out_kernel(const u32 *__restrict__ oi, const float *__restrict__ os, const u32 *__restrict__ oc, const u32 *__restrict__ flags,
                                     u32 B, u32 k, u32 *__restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x, nk = (u64)B * k;
    if (t < nk) { out[t] = oi[t]; out[nk + t] = __float_as_uint(os[t]); }
    if (t < B) out[2 * nk + t] = oc[t];
    if (t < 2) out[2 * nk + B + t] = flags[t];
}

// exact re-score of the survivors in the reference order, sort, top-k
__global__ __launch_bounds__(64) void flat_rescore(const float *__restrict__ Q, u64 q_stride, const float *__restrict__ qmags, u32 B,
                                                   const float *__restrict__ X, u64 x_stride, const float *__restrict__ xmags, u32 dim,
                                                   const u64 *__restrict__ pool_mem, u32 k, u32 id_base, u32 *__restrict__ out_ids,
                                                   float *__restrict__ out_scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    for (u32 i = lane; i < dim; i += 64) qf[i] = Q[(u64)q * q_stride + i];
    const u64 mine = pool_mem[(u64)q * SEL + lane];
    const float mq = qmags[q];
    u64 res[1] = {0ull};
    for (int base = 0; base < SEL; base += 32) { // 32 survivors per pass, one lane pair each
        const int src = base + (lane >> 1);
        const u32 sid = (u32)__shfl((int)(u32)mine, src, 64);
        const bool valid = __shfl((int)(u32)(mine >> 32), src, 64) != 0;
        const u32 row = valid ? sid : 0u;
        const float dp = f32_pair_dot(X + (u64)row * x_stride, qf, dim, lane & 1);
        pair_keys_to_lanes(exact_key(dp, mq, xmags[row], sid, valid), (u32)base, lane, res[0]);
    }
    bitonic_sort_desc<1>(res, lane);
    if ((u32)lane < k) { // (as write_topk<1, true>)
        const bool ok = res[0] != 0ull;
        out_ids[(u64)q * k + lane] = ok ? (u32)res[0] + id_base : 0xFFFFFFFFu;
        out_scores[(u64)q * k + lane] = ok ? simkey_inv((u32)(res[0] >> 32)) : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------
// Exhaustive scan over the QUANTIZED codes as an exact-integer i8 MFMA GEMM (config c3 / per-shard flat mode).
//   u8 codes   : a' = a - 128 (flip the top bit) makes them signed; sum(a*b) = S' + 128*sum(a) + 128*sum(b) - 16384*K
//                with S' = sum(a'*b') from v_mfma_i32_32x32x32_i8 — every term an exact integer
//   quaternary : the two bit planes are expanded to the digit (plane0 bit + 2 * plane1 bit), i.e. exactly the
//                value dot_product_quaternary multiplies (dot_product.rs:35-57), 4 digits per u32 via
//                (nibble * 0x00204081) & 0x01010101
//   binary     : the digit is the bit of the row's one plane, 128 dims per 16-byte chunk (dot_product_binary, dot_product.rs:21-33)
//   octal      : three planes of 32 dims per 16-byte chunk [plane0 | plane1 | plane2 | 0]; digit = p0 + 2 p1 + 4 p2 on the planes as
//                stored (dot_product_octal, dot_product.rs:64-90; chunk_dot<ENG_Q3> has the quirk).  Accumulators stay below 49 * dim
// A/B fragments are read K-contiguous (16 B per lane, k-block = lane >> 5) for both operands, so the result is
// the plain sum over k whatever the hardware's internal k order is; C/D layout as in flat_gemm_f32.
// Workgroup = 8 waves, tile 256 queries x 128 candidates, K step 64; rows padded to 80 B in LDS (conflict-free
// ds_read_b128).  Integer dots are converted with RNE and divided by |q|*|v| like cosine.rs:223-235.
// ------------------------------------------------------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
constexpr int CM = 256, CN = 128, CK = 64, CLD = 80;

__device__ __forceinline__ u32 spread4(u32 nib) { return (nib * 0x00204081u) & 0x01010101u; }

// 16 digits (dims k0..k0+15 of a 64-dim chunk) -> 16 i8 values, in two halves so the global load of a later k panel can be in
// flight while the current one is multiplied: load16_raw (16 B as stored) and unpack16 (what the MFMA reads from LDS)
template <int ENG>
__device__ __forceinline__ uint4 load16_raw(const uint8_t *__restrict__ row, u32 k0 /*multiple of 16*/, bool valid) {
    if (!valid) return make_uint4(0, 0, 0, 0);
    if constexpr (ENG == ENG_U8) return *(const uint4 *)(row + k0);
    else if constexpr (ENG == ENG_Q1) return *(const uint4 *)(row + (u64)(k0 >> 7) * 16); // 16 B per 128 dims: the one plane
    else if constexpr (ENG == ENG_Q3) return *(const uint4 *)(row + (u64)(k0 >> 5) * 16); // 16 B per 32 dims: [plane0 4 B | plane1 4 B | plane2 4 B | 0]
    else return *(const uint4 *)(row + (u64)(k0 >> 6) * 16); // 16 B per 64 dims: [plane0 8 B | plane1 8 B]
}
// dims that one 16-byte chunk of a code row covers
template <int ENG>
constexpr u32 chunk_dims() { return ENG == ENG_U8 ? 16u : ENG == ENG_Q1 ? 128u : ENG == ENG_Q3 ? 32u : 64u; }
template <int ENG>
__device__ __forceinline__ uint4 unpack16(uint4 raw, u32 k0, bool valid) {
    uint4 o = make_uint4(0, 0, 0, 0);
    if constexpr (ENG == ENG_U8) {
        o = raw;
        o.x ^= 0x80808080u; o.y ^= 0x80808080u; o.z ^= 0x80808080u; o.w ^= 0x80808080u; // padding (0) becomes -128 too: see epilogue
    } else if constexpr (ENG == ENG_Q1) { // binary: the digit is the bit (dot_product_binary, dot_product.rs:21-33)
        if (valid) {
            const u32 sh = k0 & 127, wd = sh >> 5;
            const u32 b0 = ((wd == 0 ? raw.x : wd == 1 ? raw.y : wd == 2 ? raw.z : raw.w) >> (sh & 31)) & 0xFFFFu;
            o.x = spread4(b0 & 15u);
            o.y = spread4((b0 >> 4) & 15u);
            o.z = spread4((b0 >> 8) & 15u);
            o.w = spread4((b0 >> 12) & 15u);
        }
    } else if constexpr (ENG == ENG_Q3) { // octal: p0 + 2 p1 + 4 p2 on the planes as stored (dot_product_octal, dot_product.rs:64-90; chunk_dot<ENG_Q3>)
        if (valid) {
            const u32 sh = k0 & 31;
            const u32 b0 = (raw.x >> sh) & 0xFFFFu, b1 = (raw.y >> sh) & 0xFFFFu, b2 = (raw.z >> sh) & 0xFFFFu;
            o.x = spread4(b0 & 15u) + 2u * spread4(b1 & 15u) + 4u * spread4(b2 & 15u);
            o.y = spread4((b0 >> 4) & 15u) + 2u * spread4((b1 >> 4) & 15u) + 4u * spread4((b2 >> 4) & 15u);
            o.z = spread4((b0 >> 8) & 15u) + 2u * spread4((b1 >> 8) & 15u) + 4u * spread4((b2 >> 8) & 15u);
            o.w = spread4((b0 >> 12) & 15u) + 2u * spread4((b1 >> 12) & 15u) + 4u * spread4((b2 >> 12) & 15u);
        }
    } else {
        if (valid) {
            const u32 sh = k0 & 63;
            const u64 p0 = (u64)raw.x | ((u64)raw.y << 32), p1 = (u64)raw.z | ((u64)raw.w << 32);
            const u32 b0 = (u32)(p0 >> sh) & 0xFFFFu, b1 = (u32)(p1 >> sh) & 0xFFFFu;
            o.x = spread4(b0 & 15u) + 2u * spread4(b1 & 15u);
            o.y = spread4((b0 >> 4) & 15u) + 2u * spread4((b1 >> 4) & 15u);
            o.z = spread4((b0 >> 8) & 15u) + 2u * spread4((b1 >> 8) & 15u);
            o.w = spread4((b0 >> 12) & 15u) + 2u * spread4((b1 >> 12) & 15u);
        }
    }
    return o;
}
template <int ENG>
__device__ __forceinline__ uint4 stage16(const uint8_t *__restrict__ row, u32 k0 /*multiple of 16*/, bool valid) {
    return unpack16<ENG>(load16_raw<ENG>(row, k0, valid), k0, valid);
}

// queries' bit planes (binary, quaternary, octal) -> the i8 digits the GEMM multiplies, once per batch ([B][kdims] bytes): the scan kernel
// then stages the query operand with plain 16 B copies instead of re-expanding it for every one of the N / 128 candidate tiles
template <int ENG>
__global__ void expand_digits_kernel(const uint8_t *__restrict__ qcodes, u64 row_stride, u32 B, u32 kdims, uint8_t *__restrict__ digits) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 pieces = kdims / 16;
    if (t >= (u64)B * pieces) return;
    const u32 q = (u32)(t / pieces), k0 = (u32)(t % pieces) * 16;
    const u32 code_k = (u32)(row_stride / 16) * chunk_dims<ENG>();
    *(uint4 *)(digits + (u64)q * kdims + k0) = stage16<ENG>(qcodes + (u64)q * row_stride, k0, k0 < code_k);
}

template <int ENG, bool FUSED, int PF, bool MASKED = false /* FUSED: as in flat_gemm_f32 */>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void flat_codes_gemm_i8(const uint8_t *__restrict__ qcodes, const float *__restrict__ qmags,
                                                          const u32 *__restrict__ qsums, u32 B, const uint8_t *__restrict__ codes,
                                                          const float *__restrict__ mags, const u32 *__restrict__ csums, u64 row_stride,
                                                          u32 n0, u32 n_chunk, u32 kdims /*padded to 64*/, u32 metric,
                                                          float *__restrict__ scores, u64 s_stride, const FusedOut fo) {
    __shared__ __attribute__((aligned(16))) unsigned char As[CM * CLD];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[CN * CLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1; // 4 x 2 waves, 64 x 64 outputs each
    const u32 row0 = blockIdx.y * CM, col0 = blockIdx.x * CN;
    i32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0;
    const u32 code_k = ENG == ENG_U8 ? (u32)row_stride : (u32)(row_stride / 16) * chunk_dims<ENG>(); // dims covered by stored bytes
    // Register ring of PF k panels: the 16 B pieces of panels k+1 .. k+PF are in flight (global -> VGPR) while panel k is
    // unpacked into LDS and multiplied.  With only 2 workgroups per CU the un-prefetched loop exposed the full HBM latency on
    // every panel (0.21 of the MFMA peak); the ring hides it behind PF panels of MFMA work per workgroup.
    // A: 256 rows x 64 B = 1024 x 16 B pieces, 2 per thread;  B: 128 rows x 64 B = 512 pieces, 1 per thread
    const int ar[2] = {(tid * 2) >> 2, (tid * 2 + 1) >> 2}, akq[2] = {((tid * 2) & 3) * 16, ((tid * 2 + 1) & 3) * 16};
    const int br = tid >> 2, bkq = (tid & 3) * 16;
    const bool b_in = col0 + br < n_chunk;
    const uint8_t *b_row = codes + (u64)(n0 + (b_in ? col0 + br : 0)) * row_stride;
    uint4 ra[PF][2], rb[PF];
    auto fetch = [&](int s, u32 k0) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const u32 qr = row0 + ar[h];
            if constexpr (FUSED && ENG != ENG_U8)
                ra[s][h] = qr < B ? *(const uint4 *)(fo.qdigits + (u64)qr * kdims + k0 + akq[h]) : make_uint4(0, 0, 0, 0);
            else
                ra[s][h] = load16_raw<ENG>(qcodes + (u64)(qr < B ? qr : 0) * row_stride, k0 + akq[h], qr < B && k0 + akq[h] < code_k);
        }
        rb[s] = load16_raw<ENG>(b_row, k0 + bkq, b_in && k0 + bkq < code_k);
    };
#pragma unroll
    for (int s = 0; s < PF; s++)
        if ((u32)s * CK < kdims) fetch(s, (u32)s * CK);
    for (u32 kb = 0; kb < kdims; kb += PF * CK) {
#pragma unroll
        for (int s = 0; s < PF; s++) {
            const u32 k0 = kb + (u32)s * CK;
            if (k0 >= kdims) break; // uniform
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if constexpr (FUSED && ENG != ENG_U8)
                    *(uint4 *)(As + ar[h] * CLD + akq[h]) = ra[s][h];
                else
                    *(uint4 *)(As + ar[h] * CLD + akq[h]) = unpack16<ENG>(ra[s][h], k0 + akq[h], row0 + ar[h] < B && k0 + akq[h] < code_k);
            }
            *(uint4 *)(Bs + br * CLD + bkq) = unpack16<ENG>(rb[s], k0 + bkq, b_in && k0 + bkq < code_k);
            if (k0 + PF * CK < kdims) fetch(s, k0 + PF * CK);
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < CK; ks += 32) {
                const int ko = ks + (lane >> 5) * 16;
                const i32x4 a0 = *(const i32x4 *)(As + (wr * 64 + (lane & 31)) * CLD + ko), a1 = *(const i32x4 *)(As + (wr * 64 + 32 + (lane & 31)) * CLD + ko);
                const i32x4 b0 = *(const i32x4 *)(Bs + (wc * 64 + (lane & 31)) * CLD + ko), b1 = *(const i32x4 *)(Bs + (wc * 64 + 32 + (lane & 31)) * CLD + ko);
                acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
            }
            __syncthreads();
        }
    }
    if constexpr (FUSED) {
        // per-row filter state in LDS (the operand panels are dead: the k loop ended with a barrier)
        u64 *thr_key = (u64 *)As;                         // [CM]
        float *thr_lo = (float *)(As + CM * 8);           // [CM] score a candidate must reach to be worth the exact quotient
        float *rq = (float *)(As + CM * 12);              // [CM] ~1/|q|
        for (int idx = tid; idx < CM; idx += 512) {
            const u32 row = row0 + idx;
            const u64 k = row < B ? fo.thr[row] : ~0ull;
            thr_key[idx] = k;
            thr_lo[idx] = k == 0ull ? -1.0f : simkey_inv((u32)(k >> 32)) * (1.0f - 4e-6f); // scores of u8 / bit-plane codes are >= 0
            rq[idx] = row < B ? __builtin_amdgcn_rcpf(qmags[row]) : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const u32 col = col0 + wc * 64 + j * 32 + (lane & 31);
                const bool cv = col < n_chunk;
                const float xm = cv ? mags[n0 + col] : 1.0f;
                const float rx = __builtin_amdgcn_rcpf(xm);
                const int cs = (ENG == ENG_U8 && cv) ? (int)csums[n0 + col] : 0;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int rl = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const u32 row = row0 + rl;
                    int dot = acc[i][j][r];
                    if constexpr (ENG == ENG_U8) dot += 128 * (int)qsums[row < B ? row : 0] + 128 * cs - 16384 * (int)kdims;
                    const float dotf = (float)(u32)dot;
                    const float est = metric == 0u ? dotf * rx * rq[rl] : dotf;
                    if (row < B && cv && est >= thr_lo[rl]) {
                        const float sc = metric == 0u ? __fdiv_rn(dotf, __fmul_rn(qmags[row], xm)) : dotf;
                        const u64 key = score_key(sc, n0 + col);
                        if (key > thr_key[rl] && scan_live<MASKED>(fo.m, row, n0 + col)) {
                            const u32 pos = atomicAdd(&fo.app_cnt[row], 1u);
                            if (pos < fo.cap) fo.app[(u64)row * fo.cap + pos] = key;
                        }
                    }
                }
            }
        return;
    }
    // Unfused epilogue (score matrix out: the unfused flat scan and the walk's level table, where it is most of the kernel — K = 768
    // is short and every output needs an exact quotient).  The per-row terms (|q| and the query's share of the u8 recentring) are
    // staged in LDS once per workgroup (the operand panels are dead: the k loop ended with a barrier) instead of two global loads per
    // output; the output pointer of a 32 x 32 block advances by a constant stride; tiles inside the matrix skip the bounds tests.
    float *rqm = (float *)As;             // [CM] |q|
    int *rqs = (int *)(As + CM * 4);      // [CM] 128 * sum(q) - 16384 * kdims (u8), 0 otherwise
    for (int idx = tid; idx < CM; idx += 512) {
        const u32 row = row0 + idx;
        rqm[idx] = row < B ? qmags[row] : 1.0f;
        rqs[idx] = (ENG == ENG_U8 && row < B) ? 128 * (int)qsums[row] - 16384 * (int)kdims : 0;
    }
    __syncthreads();
    const bool inside = row0 + CM <= B && col0 + CN <= n_chunk; // workgroup-uniform
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32 col = col0 + wc * 64 + j * 32 + (lane & 31);
            const bool cv = col < n_chunk;
            const float xm = cv ? mags[n0 + col] : 1.0f;
            const int cs = (ENG == ENG_U8 && cv) ? 128 * (int)csums[n0 + col] : 0;
            const int rl0 = wr * 64 + i * 32 + 4 * (lane >> 5);
            float *out = scores + (u64)(row0 + rl0) * s_stride + col;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int dr = (r & 3) + 8 * (r >> 2);
                const int rl = rl0 + dr;
                if (inside || (row0 + (u32)rl < B && cv)) {
                    int dot = acc[i][j][r];
                    if constexpr (ENG == ENG_U8) dot += rqs[rl] + cs;
                    const float dotf = (float)(u32)dot; // exact integer -> f32 RNE, like `as f32` on the u64 dot
                    float sc = dotf;
                    if (metric == 0u) sc = __fdiv_rn(dotf, __fmul_rn(rqm[rl], xm)); // zero norms are screened on the host side
                    out[(u64)dr * s_stride] = sc;
                }
            }
        }
}

__global__ void code_sums_kernel(const uint8_t *__restrict__ codes, u64 row_stride, u32 n, u32 *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const u32 row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    u32 s = 0;
    for (u32 i = lane * 4; i < (u32)row_stride; i += 256) {
        const u32 w = *(const u32 *)(codes + (u64)row * row_stride + i);
        s += (w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += (u32)__shfl_xor((int)s, m, 64);
    if (lane == 0) sums[row] = s;
}

// exact rerank of the best `ncand` survivors (pool is sorted desc by quantized score, larger id first) -> top k
__global__ __launch_bounds__(64) void flat_rerank_top5k(const float *__restrict__ Q, u64 q_stride, const float *__restrict__ qraw_mags, u32 B,
                                                        const float *__restrict__ X, u64 x_stride, const float *__restrict__ xmags, u32 dim,
                                                        const u64 *__restrict__ pool_mem, u32 ncand_max, u32 k, u32 id_base,
                                                        u32 *__restrict__ out_ids, float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    for (u32 i = lane; i < dim; i += 64) qf[i] = Q[(u64)q * q_stride + i];
    const u64 mine = pool_mem[(u64)q * SEL + lane];
    const u32 have = (u32)__popcll(__ballot(mine != 0ull));
    const u32 ncand = have < ncand_max ? have : ncand_max;
    const float mq = qraw_mags[q];
    u64 res[1] = {0ull};
    for (int base = 0; base < SEL; base += 32) {
        if ((u32)base >= ncand) break;
        const int src = base + (lane >> 1);
        const u32 sid = (u32)__shfl((int)(u32)mine, src, 64);
        const bool valid = (u32)src < ncand;
        const u32 row = valid ? sid : 0u;
        const float dp = f32_pair_dot(X + (u64)row * x_stride, qf, dim, lane & 1);
        pair_keys_to_lanes(exact_key(dp, mq, xmags[row], sid, valid), (u32)base, lane, res[0]);
    }
    bitonic_sort_desc<1>(res, lane);
    const u32 nout = ncand < k ? ncand : k;
    if ((u32)lane < nout) { // (as write_topk<1, false>)
        out_ids[(u64)q * k + lane] = (u32)res[0] + id_base;
        out_scores[(u64)q * k + lane] = simkey_inv((u32)(res[0] >> 32));
    }
    if (lane == 0) out_counts[q] = nout;
}

// ---- a call's cos_scan_mask: checked on the host, then one set of device buffers ----
struct MaskPlan {
    bool masked = false;        // false: the unmasked call (mask == NULL, or no allow-list and no flag)
    bool skip_deleted = false;
    std::vector<u32> used;      // the caller's masks that some query names, ascending; empty = no allow-list (one all-ones mask)
    std::vector<u32> qmask;     // [B] -> index into `used`
};
// COS_OK or the refusal.  Masks no query names are neither uploaded nor part of the zero-norm screen.
int32_t scan_mask_plan(const cos_scan_mask *mask, u32 B, MaskPlan &mp) {
    if (!mask) return COS_OK;
    if (mask->struct_size != sizeof(cos_scan_mask)) return cos_fail(COS_ERR_INVALID, "cos_scan_mask::struct_size is %u, expected %zu", mask->struct_size, sizeof(cos_scan_mask));
    if (mask->flags & ~COS_SCAN_SKIP_DELETED) return cos_fail(COS_ERR_INVALID, "unknown cos_scan_mask::flags 0x%x", mask->flags);
    const u32 G = mask->n_masks;
    if (G > 0 && !mask->bits) return cos_fail(COS_ERR_INVALID, "cos_scan_mask::bits is NULL with n_masks = %u", G);
    if (G > 1 && !mask->query_mask) return cos_fail(COS_ERR_INVALID, "cos_scan_mask::query_mask is NULL with n_masks = %u", G);
    mp.skip_deleted = (mask->flags & COS_SCAN_SKIP_DELETED) != 0;
    if (G == 0 && !mp.skip_deleted) return COS_OK;
    mp.qmask.assign(B, 0u);
    if (G > 0) {
        std::vector<u32> slot(G, 0xFFFFFFFFu);
        if (mask->query_mask) {
            for (u32 b = 0; b < B; b++) {
                if (mask->query_mask[b] >= G) return cos_fail(COS_ERR_INVALID, "query_mask[%u] = %u with n_masks = %u", b, mask->query_mask[b], G);
                slot[mask->query_mask[b]] = 0;
            }
        } else
            slot[0] = 0;
        for (u32 g = 0; g < G; g++)
            if (slot[g] == 0) { slot[g] = (u32)mp.used.size(); mp.used.push_back(g); }
        if (mask->query_mask)
            for (u32 b = 0; b < B; b++) mp.qmask[b] = slot[mask->query_mask[b]];
    }
    mp.masked = true;
    return COS_OK;
}
struct MaskBufs { // grow-only, like the other buffers of a scan
    DevArr<u32> user, eff, uni, qmask;
};
// the plan's masks on the device (stream st: the plan and the caller's arrays stay until the caller has drained it): sm for the kernels,
// *uni = the union of the live sets
hipError_t scan_mask_upload(const cos_index *ix, const cos_scan_mask *mask, const MaskPlan &mp, u32 B, MaskBufs &mb, hipStream_t st, ScanMask &sm, const u32 **uni) {
    const u32 n = ix->n, words = (n + 31) / 32, G = mp.used.empty() ? 1u : (u32)mp.used.size();
    hipError_t e = mb.eff.grow((size_t)G * words);
    if (e == hipSuccess) e = mb.uni.grow(words);
    if (e == hipSuccess) e = mb.qmask.grow(B);
    if (e == hipSuccess && !mp.used.empty()) e = mb.user.grow((size_t)G * words);
    for (u32 g = 0; g < (u32)mp.used.size() && e == hipSuccess; g++)
        e = hipMemcpyAsync(mb.user.p + (size_t)g * words, mask->bits + (size_t)mp.used[g] * words, (size_t)words * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(mb.qmask.p, mp.qmask.data(), (size_t)B * 4, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scan_mask_build_kernel, dim3((words + 255) / 256), dim3(256), 0, st, mp.used.empty() ? (const u32 *)nullptr : (const u32 *)mb.user.p,
                       mp.skip_deleted ? (const u32 *)ix->d_deleted.p : (const u32 *)nullptr, G, words, n, mb.eff.p, mb.uni.p);
    e = hipGetLastError();
    sm =ScanMask{mb.eff.p, mb.qmask.p, words};
    *uni = mb.uni.p;
    return e;
}

// ---- what the two scans share: the numbers are flat_plan.h's, the launches are here ----
namespace fp = flat_plan;
static_assert(fp::OK == COS_OK && fp::INVALID == COS_ERR_INVALID && fp::UNIMPLEMENTED == COS_ERR_UNIMPLEMENTED, "flat_plan.h restates cos_status");
static_assert(fp::U8 == ENG_U8 && fp::Q2 == ENG_Q2 && fp::Q1 == ENG_Q1 && fp::Q3 == ENG_Q3, "flat_plan.h restates the engines");
static_assert(BN == 128 && CN == 128, "flat_plan.h unfused_chunk: whole tiles of 128 candidates");
static_assert(SEL == 64, "flat_plan.h flat_pool_width: the narrowest pool");

// the device buffers that the chunks of an attempt go through, sized by the caller from its plan
struct ScanBufs {
    float *scores;    // [B][s_stride]: the score matrix of an unfused chunk
    u64 s_stride;
    u64 *part;        // [B][S][P]: its selection's partial lists
    u64 *pool, *thr;  // [B][P] survivors, [B] their P-th best
    u64 *app;         // [B][app_cap]: what a fused chunk lets through, appcnt[B] of them
    u32 *appcnt, *overflow; // *overflow |= 1 by a fold that found a counter above app_cap
    ScanMask sm;
    FusedOut fused_out(const fp::Scan &plan, const uint8_t *qdigits) const { return FusedOut{thr, app, appcnt, plan.app_cap(), qdigits, sm}; }
};

// a scored chunk into the pools: a fused chunk's append buffer, or the selection over an unfused chunk's score matrix; 64-key pools on the
// kernels above, wider ones on kernels_flat_wide.hip
hipError_t fold_chunk(const fp::Scan &plan, const fp::Chunk &c, const ScanBufs &b, hipStream_t st) {
    const u32 B = plan.B, R = plan.P / SEL;
    if (c.fused && R == 1) {
        hipLaunchKernelGGL(flat_select_append, dim3(B), dim3(64), 0, st, (const u64 *)b.app, b.appcnt, plan.app_cap(), B, b.pool, b.thr, b.overflow);
        return hipGetLastError();
    }
    if (c.fused) return launch_flat_append_wide(R, b.app, b.appcnt, plan.app_cap(), B, b.pool, b.thr, b.overflow, st);
    const u32 S = fp::select_segments(B, c.nc);
    if (R == 1) return launch_select(b.scores, b.s_stride, B, c.n0, c.nc, b.part, S, b.pool, st, b.thr, b.sm);
    return launch_flat_select_wide(R, b.scores, b.s_stride, B, c.n0, c.nc, b.part, S, b.pool, b.thr, st, b.sm);
}

// the chunks of one attempt, in order: score(chunk) enqueues the kernel that scores it, then the chunk is folded.  The first failed HIP
// call ends it: nothing further is started on the stream
template <class Score>
hipError_t run_chunks(const fp::Scan &plan, int attempt, const ScanBufs &b, hipStream_t st, Score &&score) {
    fp::Schedule sched = plan.schedule(attempt);
    fp::Chunk c;
    hipError_t e = hipSuccess;
    while (e == hipSuccess && sched.next(c)) {
        e = score(c);
        if (e == hipSuccess) e = fold_chunk(plan, c, b, st);
    }
    return e;
}

// flat_gemm_f32<VEC, FUSED, MASKED>.  An unfused chunk has no masked form: its selection applies the mask
using GemmF32Kernel = decltype(&flat_gemm_f32<true, false>);
GemmF32Kernel gemm_f32_kernel(bool vec, bool fused, bool masked) {
    if (!fused) return vec ? flat_gemm_f32<true, false> : flat_gemm_f32<false, false>;
    if (!masked) return vec ? flat_gemm_f32<true, true> : flat_gemm_f32<false, true>;
    return vec ? flat_gemm_f32<true, true, true> : flat_gemm_f32<false, true, true>;
}
// every instantiation above may use GEMM_SMEM bytes of dynamic LDS
hipError_t gemm_f32_allow_lds() {
    hipError_t e = hipSuccess;
    for (int vec = 0; vec < 2; vec++)
        for (int fused = 0; fused < 2; fused++)
            for (int masked = 0; masked <= fused && e == hipSuccess; masked++)
                e = hipFuncSetAttribute((const void *)gemm_f32_kernel(vec, fused, masked), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEMM_SMEM);
    return e;
}
// scores of rows [n0, n0 + nc) of X against the B queries
hipError_t launch_gemm_f32(bool vec, bool fused, bool masked, const float *Q, const float *qmags, u32 B, const float *X, const float *xmags, u32 n0, u32 nc,
                           u32 dim, float *scores, u64 s_stride, const FusedOut &fo, hipStream_t st) {
    const dim3 grid((nc + BN - 1) / BN, (B + BM - 1) / BM);
    hipLaunchKernelGGL(gemm_f32_kernel(vec, fused, masked), grid, dim3(256), GEMM_SMEM, st, Q, (u64)dim, qmags, B, X, (u64)dim, xmags, n0, nc, dim, scores, s_stride, fo);
    return hipGetLastError();
}

// the queries' bit planes -> the digit bytes [B][kdims] the tile kernel multiplies; eng = ENG_Q2, ENG_Q1 or ENG_Q3
hipError_t launch_expand_digits(int eng, const uint8_t *qcodes, u64 row_stride, u32 B, u32 kdims, uint8_t *digits, hipStream_t st) {
    const u64 pieces = (u64)B * (kdims / 16);
    const dim3 grid((u32)((pieces + 255) / 256));
    if (eng == ENG_Q2) hipLaunchKernelGGL(expand_digits_kernel<ENG_Q2>, grid, dim3(256), 0, st, qcodes, row_stride, B, kdims, digits);
    else if (eng == ENG_Q1) hipLaunchKernelGGL(expand_digits_kernel<ENG_Q1>, grid, dim3(256), 0, st, qcodes, row_stride, B, kdims, digits);
    else hipLaunchKernelGGL(expand_digits_kernel<ENG_Q3>, grid, dim3(256), 0, st, qcodes, row_stride, B, kdims, digits);
    return hipGetLastError();
}

// flat_codes_gemm_i8<ENG, FUSED, PF, MASKED>: pf = k panels prefetched into registers (1..3; results do not depend on it).  A fused chunk
// of a masked call keeps one panel in flight whatever pf says; an unfused chunk has no masked form
using CodesGemmKernel = decltype(&flat_codes_gemm_i8<ENG_U8, false, 1>);
template <int ENG>
CodesGemmKernel codes_gemm_kernel_of(bool fused, int pf, bool masked) {
    if (fused && masked) return flat_codes_gemm_i8<ENG, true, 1, true>;
    if (fused && pf == 2) return flat_codes_gemm_i8<ENG, true, 2>;
    if (fused && pf == 3) return flat_codes_gemm_i8<ENG, true, 3>;
    if (fused) return flat_codes_gemm_i8<ENG, true, 1>;
    if (pf == 2) return flat_codes_gemm_i8<ENG, false, 2>;
    if (pf == 3) return flat_codes_gemm_i8<ENG, false, 3>;
    return flat_codes_gemm_i8<ENG, false, 1>;
}
// the operands of the tile kernel that stay the same from chunk to chunk
struct CodesGemm {
    const uint8_t *qcodes; const float *qmags; const u32 *qsums; u32 B;             // the queries
    const uint8_t *codes; const float *mags; const u32 *csums; u64 row_stride;      // the rows
    u32 kdims, metric;
    float *scores; u64 s_stride;                                                    // unfused: [B][s_stride]
    FusedOut fo;
};
// rows [n0, n0 + nc) of the codes; eng = ENG_U8, ENG_Q2, ENG_Q1 or ENG_Q3
hipError_t launch_codes_gemm(int eng, bool fused, int pf, bool masked, const CodesGemm &g, u32 n0, u32 nc, hipStream_t st) {
    const CodesGemmKernel kernel = eng == ENG_U8   ? codes_gemm_kernel_of<ENG_U8>(fused, pf, masked)
                                   : eng == ENG_Q2 ? codes_gemm_kernel_of<ENG_Q2>(fused, pf, masked)
                                   : eng == ENG_Q1 ? codes_gemm_kernel_of<ENG_Q1>(fused, pf, masked)
                                                   : codes_gemm_kernel_of<ENG_Q3>(fused, pf, masked);
    const dim3 grid((nc + CN - 1) / CN, (g.B + CM - 1) / CM);
    hipLaunchKernelGGL(kernel, grid, dim3(512), 0, st, g.qcodes, g.qmags, g.qsums, g.B, g.codes, g.mags, g.csums, g.row_stride, n0, nc, g.kdims, g.metric, g.scores,
                       g.s_stride, g.fo);
    return hipGetLastError();
}

// ---- brute force: which pools the GEMM's ranking may have cut wrongly, and the scores of the exact path ----
// flags[q] = 1 and *n_flagged += 1 where flat_plan.h brute_margin_safe says no: the pool (sorted descending, P keys, at every width
// pool[q][e]) is full and its P-th score is not more than twice the bound under its k-th.  One thread per query.
__global__ void brute_margin_kernel(const u64 *__restrict__ pool_mem, u32 P, u32 B, u32 k, u32 dim, u32 *__restrict__ flags, u32 *__restrict__ n_flagged) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    const u64 kth = pool_mem[(u64)q * P + k - 1], pth = pool_mem[(u64)q * P + P - 1];
    const bool safe = fp::brute_margin_safe(simkey_inv((u32)(kth >> 32)), simkey_inv((u32)(pth >> 32)), dim, (u32)(pth >> 32) != 0u);
    flags[q] = safe ? 0u : 1u;
    if (!safe) atomicAdd(n_flagged, 1u);
}
// The exact path's scores: scores[q][c] = dot_f32(q, x) / (|q| * |x|) of row n0 + c in the REFERENCE's order — the value exact_key ranks
// and flat_rescore returns, so the selection over this matrix (the unfused chunk's, ties to the larger id, masks applied there) keeps
// the exact top P and the re-score that follows reproduces it.  A lane pair per row (f32_pair_dot), 128 rows per pass of the 4 waves,
// EXACT_ROWS rows per workgroup so that the query is staged once per 8 passes.  Grid (B, ceil(n_chunk / EXACT_ROWS)).
constexpr u32 EXACT_ROWS = 1024;
__global__ __launch_bounds__(256) void flat_exact_scores(const float *__restrict__ Q, u64 q_stride, const float *__restrict__ qmags,
                                                         const float *__restrict__ X, u64 x_stride, const float *__restrict__ xmags, u32 n0,
                                                         u32 n_chunk, u32 dim, float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const u32 tid = threadIdx.x, q = blockIdx.x;
    for (u32 i = tid; i < dim; i += 256) qf[i] = Q[(u64)q * q_stride + i];
    __syncthreads();
    const float mq = qmags[q];
    const u32 c_begin = blockIdx.y * EXACT_ROWS, c_end = c_begin + EXACT_ROWS < n_chunk ? c_begin + EXACT_ROWS : n_chunk;
    for (u32 c0 = c_begin; c0 < c_end; c0 += 128) { // (workgroup-uniform: both lanes of a pair run every pass)
        const u32 col = c0 + (tid >> 1);
        const bool valid = col < n_chunk;
        const u32 row = n0 + (valid ? col : 0u);
        const float dp = f32_pair_dot(X + (u64)row * x_stride, qf, dim, (int)(tid & 1));
        if (valid && (tid & 1) == 0) scores[(u64)q * s_stride + col] = x86_div(dp, __fmul_rn(mq, xmags[row]));
    }
}
hipError_t launch_exact_scores(const float *Q, const float *qmags, u32 B, const float *X, const float *xmags, u32 n0, u32 nc, u32 dim, float *scores,
                               u64 s_stride, hipStream_t st) {
    hipLaunchKernelGGL(flat_exact_scores, dim3(B, (nc + EXACT_ROWS - 1) / EXACT_ROWS), dim3(256), staged_query_bytes(dim), st, Q, (u64)dim, qmags, X, (u64)dim,
                       xmags, n0, nc, dim, scores, s_stride);
    return hipGetLastError();
}

// cos_bruteforce_topk (mask == nullptr, out_counts optional) and cos_bruteforce_topk_masked; with d_record (device memory on the index's
// device, B * (2k + 1) words) the shard set's form: the same launches, the rerank writes [ids B*k | scores B*k | counts B] there instead of
// the call's own buffers, nothing is copied out (out_* unused) and the record is complete when the call returns.
// The exact path (flat_plan.h brute_margin_safe; tuning knob flat_brute_exact): a query whose pool the GEMM's ranking may have cut
// wrongly is answered again by the same call on the sub-batch of such queries with exact_pass set — every chunk unfused, its score
// matrix written by flat_exact_scores instead of the GEMM, the same selection, masks, re-score and counts — and its rows replace the
// first answer's.  The flags' count comes back with the overflow flag: a call with nothing flagged makes no further round trip.
int32_t bruteforce_run(cos_index *ix, const float *queries, uint32_t B, uint32_t k, const cos_scan_mask *mask, uint32_t *out_ids, float *out_scores,
                       uint32_t *out_counts, u32 *d_record = nullptr, bool exact_pass = false) {
    if (!ix || !queries || ((!out_ids || !out_scores) && !d_record) || B == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    if (int32_t krc = fp::check_brute_k(k, ix->n)) return cos_fail(krc, "k must be in [1, min(512, n)]");
    MaskPlan mp;
    if (int32_t mrc = scan_mask_plan(mask, B, mp)) return mrc;
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 dim = ix->p.dim, n = ix->n;
    // Same schedule as cos_flat_search_batch (flat_plan.h): the seed chunk goes through the score matrix + segmented selection and
    // seeds every query's threshold; later chunks grow and the GEMM epilogue appends only what beats the threshold.  An
    // append-buffer overflow repeats the call on the unfused path (tuning knob flat_unfused = 1 forces it).
    // Survivors per query: the GEMM only generates candidates, so the pool holds at least 2k of them (64 for k <= 32, as ever).
    const int exact_mode = exact_pass ? (int)fp::BRUTE_EXACT_ALWAYS : (int)tune_or(TUNE_FLAT_BRUTE_EXACT, fp::BRUTE_EXACT_BY_RULE);
    const bool exact = exact_mode >= fp::BRUTE_EXACT_ALWAYS, by_rule = exact_mode == fp::BRUTE_EXACT_BY_RULE;
    const fp::Scan plan = fp::brute_scan(n, B, k, exact || tune_or(TUNE_FLAT_UNFUSED, 0) != 0);
    const u32 P = plan.P, R = P / SEL;
    // the score matrix and the selection's lists serve the unfused chunks of both attempts
    const u64 s_stride = fp::score_stride(plan.unfused);
    DevArr<float> d_q, d_qm, d_scores, d_os, d_dummy;
    DevArr<u64> d_pool, d_part, d_thr, d_app;
    DevArr<u32> d_oi, d_appcnt, d_over, d_oc, d_flag;
    DevArr<uint8_t> d_codes;
    MaskBufs mb;
    hipStream_t st = ix->own_stream;
    HIP_TRY(d_q.alloc((size_t)B * dim));
    HIP_TRY(d_part.alloc((size_t)B * fp::select_segments(B, plan.unfused) * P));
    HIP_TRY(d_qm.alloc(B));
    HIP_TRY(d_dummy.alloc(B));
    HIP_TRY(d_codes.alloc((size_t)B * (((size_t)dim * 4 + 15) & ~(size_t)15)));
    HIP_TRY(d_scores.alloc((size_t)B * s_stride));
    HIP_TRY(d_pool.alloc((size_t)B * P));
    HIP_TRY(d_thr.alloc(B));
    if (plan.allow_fused) HIP_TRY(d_app.alloc((size_t)B * plan.app_cap()));
    HIP_TRY(d_appcnt.alloc(B));
    HIP_TRY(d_over.alloc(2)); // [the fused path's overflow flag, queries the margin rule flagged]
    if (by_rule) HIP_TRY(d_flag.alloc(B));
    if (!d_record) {
        HIP_TRY(d_oi.alloc((size_t)B * k));
        HIP_TRY(d_os.alloc((size_t)B * k));
        if (mp.masked) HIP_TRY(d_oc.alloc(B));
    }
    u32 *const r_oi = d_record ? d_record : d_oi.p, *const r_oc = d_record ? d_record + 2 * (size_t)B * k : d_oc.p;
    float *const r_os = d_record ? reinterpret_cast<float *>(d_record + (size_t)B * k) : d_os.p;
    // (from here on a ladder: the stream is drained below on every path before the buffers and `hover` go out of scope)
    hipError_t e = hipMemcpyAsync(d_q, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, st);
    // |q| in the reference's sequential order (vector_store.rs:414): reuse the F32 quantize kernel's raw_mags output
    if (e == hipSuccess) e = launch_quantize_rows(ENG_F32, d_q, dim, B, dim, 0.f, 0.f, d_codes, ((u64)dim * 4 + 15) & ~15ull, d_dummy, d_qm, st);
    if (e == hipSuccess) e = gemm_f32_allow_lds();
    ScanMask sm{nullptr, nullptr, 0u};
    const u32 *d_uni = nullptr; // (the brute force has no zero-norm screen)
    if (e == hipSuccess && mp.masked) e = scan_mask_upload(ix, mask, mp, B, mb, st, sm, &d_uni);
    // float4 staging needs 16 B aligned rows: dim % 4 == 0 (hipMalloc'd bases are 256 B aligned; a borrowed raw pointer is checked)
    const bool vec = dim % 4 == 0 && ((uintptr_t)ix->d_raw & 15) == 0;
    u32 n_flagged = 0;
    for (int attempt = 0; attempt < 2 && e == hipSuccess; attempt++) {
        if (e == hipSuccess) e = hipMemsetAsync(d_pool, 0, (size_t)B * P * 8, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_thr, 0, (size_t)B * 8, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_appcnt, 0, (size_t)B * 4, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_over, 0, 8, st);
        const ScanBufs bufs{d_scores, s_stride, d_part, d_pool, d_thr, d_app, d_appcnt, d_over, sm};
        const FusedOut fo = bufs.fused_out(plan, nullptr);
        if (e == hipSuccess)
            e = run_chunks(plan, attempt, bufs, st, [&](const fp::Chunk &c) {
                if (exact) return launch_exact_scores(d_q, d_qm, B, ix->d_raw, ix->d_raw_mags, c.n0, c.nc, dim, d_scores, s_stride, st);
                return launch_gemm_f32(vec, c.fused, mp.masked, d_q, d_qm, B, ix->d_raw, ix->d_raw_mags, c.n0, c.nc, dim, d_scores, s_stride, fo, st);
            });
        if (e == hipSuccess && by_rule) { // the pools are final (or about to be repeated): ranks k and P of each
            hipLaunchKernelGGL(brute_margin_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const u64 *)d_pool, P, B, k, dim, d_flag.p, d_over.p + 1);
            e = hipGetLastError();
        }
        u32 hover[2] = {0u, 0u};
        if (e == hipSuccess) e = hipMemcpyAsync(hover, d_over, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        n_flagged = hover[1];
        if (e != hipSuccess || !plan.fused(attempt) || hover[0] == 0) break; // done; otherwise the append buffer overflowed: repeat unfused
    }
    if (e == hipSuccess && R == 1) {
        hipLaunchKernelGGL(flat_rescore, dim3(B), dim3(64), staged_query_bytes(dim), st, d_q, (u64)dim, d_qm, B, ix->d_raw, (u64)dim,
                           ix->d_raw_mags, dim, d_pool, k, ix->p.id_base, r_oi, r_os);
        e = hipGetLastError();
    } else if (e == hipSuccess)
        e = launch_flat_rerank_wide(R, true, d_q, (u64)dim, d_qm, B, ix->d_raw, (u64)dim, ix->d_raw_mags, dim, d_pool, P, k, ix->p.id_base, r_oi, r_os, nullptr, st);
    if (e == hipSuccess && !d_record) e = hipMemcpyAsync(out_ids, r_oi, (size_t)B * k * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !d_record) e = hipMemcpyAsync(out_scores, r_os, (size_t)B * k * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && mp.masked) { // a query may have fewer live rows than k
        hipLaunchKernelGGL(pool_count_kernel, dim3(B), dim3(64), 0, st, (const u64 *)d_pool, P, B, k, r_oc);
        e = hipGetLastError();
        if (e == hipSuccess && !d_record) e = hipMemcpyAsync(out_counts, r_oc, (size_t)B * 4, hipMemcpyDeviceToHost, st);
    } else if (e == hipSuccess && d_record)
        e = launch_fill_i32(reinterpret_cast<int32_t *>(r_oc), B, (int32_t)k, st); // k <= n: every list is full
    std::vector<u32> h_flag;
    if (e == hipSuccess && n_flagged) {
        h_flag.resize(B);
        e = hipMemcpyAsync(h_flag.data(), d_flag.p, (size_t)B * 4, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    HIP_TRY(e);
    if (!mp.masked && out_counts && !d_record) std::fill(out_counts, out_counts + B, k); // k <= n: every list is full
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
    if (int32_t xrc = bruteforce_run(ix, xq.data(), Bx, k, mask ? &xmask : nullptr, xi.data(), xs.data(), xc.data(), nullptr, true)) return xrc;
    const size_t nk = (size_t)B * k;
    std::vector<u32> h_rec;
    u32 *h_i = out_ids, *h_c = out_counts;
    float *h_s = out_scores;
    if (d_record) { // the shard set's form: the record comes down, takes the rows and goes back
        h_rec.resize(2 * nk + B);
        e = hipMemcpyAsync(h_rec.data(), d_record, h_rec.size() * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        HIP_TRY(e);
        h_i = h_rec.data();
        h_s = reinterpret_cast<float *>(h_rec.data() + nk);
        h_c = h_rec.data() + 2 * nk;
    }
    for (u32 i = 0; i < Bx; i++) {
        memcpy(h_i + (size_t)sel[i] * k, xi.data() + (size_t)i * k, (size_t)k * 4);
        memcpy(h_s + (size_t)sel[i] * k, xs.data() + (size_t)i * k, (size_t)k * 4);
        if (h_c) h_c[sel[i]] = xc[i]; // (an unmasked call's counts are k in both passes)
    }
    if (d_record) {
        e = hipMemcpyAsync(d_record, h_rec.data(), h_rec.size() * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        HIP_TRY(e);
    }
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_bruteforce_topk(cos_index *ix, const float *queries, uint32_t B, uint32_t k, uint32_t *out_ids, float *out_scores) {
    return bruteforce_run(ix, queries, B, k, nullptr, out_ids, out_scores, nullptr);
}
extern "C" int32_t cos_bruteforce_topk_masked(cos_index *ix, const float *queries, uint32_t B, uint32_t k, const cos_scan_mask *mask, uint32_t *out_ids,
                                              float *out_scores, uint32_t *out_counts) {
    if (!out_counts) return cos_fail(COS_ERR_INVALID, "bad argument");
    return bruteforce_run(ix, queries, B, k, mask, out_ids, out_scores, out_counts);
}
extern "C" int32_t cos_index_last_brute_stats(cos_index *ix, cos_brute_stats *out) {
    if (!ix || !out) return cos_fail(COS_ERR_INVALID, "null argument");
    if (out->struct_size != sizeof(cos_brute_stats)) return cos_fail(COS_ERR_INVALID, "cos_brute_stats::struct_size is %u, expected %zu", out->struct_size, sizeof(cos_brute_stats));
    *out = ix->brute_last;
    return COS_OK;
}

// Per-index workspace of cos_flat_search_batch: every buffer is grow-only and lives until the index is destroyed (or its
// vectors are replaced), so a scan makes no allocation and creates no event on the query path — 17 hipMalloc / hipFree pairs
// and a dozen event create / destroy calls used to cost about as much wall time as the scan kernel itself.
struct FlatWs {
    std::mutex mu; // the scan runs on the index's own stream: one call at a time
    DevArr<float> q, qm, qrm, os, scores;
    DevArr<uint8_t> qc, qd, qdp;
    DevArr<u32> zero, qs, cs, appcnt, oi, oc;
    DevArr<u64> pool, thr, app, part;
    bool cs_valid = false; // code sums of the stored vectors (u8 engine) computed for the current upload
    u32 cs_n = 0;
    bool zn_valid = false, zn_zero = false; // "a stored vector has a zero norm" for the current upload (cosine's CalculationError screen)
    u32 zn_n = 0;
    // a masked call's effective masks.  Its zero-norm answer depends on the masks and is computed per call: the cached flag above stays
    // the unmasked calls'; the code sums above do not depend on a mask and serve both
    MaskBufs mask;
    DevArr<u32> out;         // [ids B x k | scores B x k | counts B | zero-norm flag, overflow flag]: ONE copy back per call
    PinArr<u32> h_out;        // its pinned landing area
    std::vector<hipEvent_t> evs;
    hipError_t event(size_t i, hipEvent_t *out) {
        while (evs.size() <= i) {
            hipEvent_t ev = nullptr;
            hipError_t e = hipEventCreate(&ev);
            if (e != hipSuccess) return e;
            evs.push_back(ev);
        }
        *out = evs[i];
        return hipSuccess;
    }
    ~FlatWs() {
        for (hipEvent_t ev : evs) (void)hipEventDestroy(ev);
    }
};

void cos_flat_ws_release(cos_index *ix) { // cos_index_destroy, and every upload that replaces the stored vectors
    delete ix->flat_ws;
    ix->flat_ws = nullptr;
}

// ------------------------------------------------------------------------------------------------
// cos_flat_search_batch: exhaustive search over the index's quantized codes (i8 MFMA) + exact rerank of the best 5k.
// u8 and the three bit-plane storages (binary, quaternary, octal): integer dots, exact in any order.  f16 / f32 codes are refused: their
// reference dots are order-dependent f32 chains that an MFMA cannot reproduce, so the candidate set could not be exact.
// ------------------------------------------------------------------------------------------------
// cos_flat_search_batch (mask == nullptr) and cos_flat_search_masked_batch; with d_record (device memory on the index's device,
// B * (2 top_k + 1) words) the shard set's form: the same launches and read-backs, and the first 2 B top_k + B words of the packed output
// [ids | scores | counts] go to d_record by a device copy instead of to out_* (unused); the record is complete when the call returns
static int32_t flat_search_run(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, const cos_scan_mask *mask, uint32_t *out_ids,
                               float *out_scores, uint32_t *out_counts, cos_flat_stats *stats, u32 *d_record = nullptr) {
    if (!ix || !queries || ((!out_ids || !out_scores || !out_counts) && !d_record) || B == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    MaskPlan mp;
    if (int32_t mrc = scan_mask_plan(mask, B, mp)) return mrc;
    if (int32_t krc = fp::check_code_top_k(top_k)) return cos_fail(krc, "flat search keeps at most 1024 survivors (5 * top_k): top_k must be in [1, 204]");
    const bool planes = fp::bit_planes(ix->eng); // bit-plane storage: the operands are expanded to digits
    if (ix->eng != ENG_U8 && !planes)
        return cos_fail(COS_ERR_UNIMPLEMENTED, "flat search over codes implements u8, binary, quaternary and octal storage");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 dim = ix->p.dim, n = ix->n;
    const u32 kdims = fp::code_kdims(ix->eng, ix->row_stride);
    // Fused chunks run on a query-resident kernel where the storage and K have an instantiation (kernels_scan.hip: flat_scan_q2_* for
    // bit-plane codes, with e2m1 digits on the scaled MFMA by default; flat_scan_u8_areg for u8 rows of whole 64-byte chunks — 1024 dims:
    // 32 query rows per wave instead of 64), on the tile kernel otherwise, and always with tuning knob flat_tile_kernel = 1.
    const fp::ScanKernel kernel = fp::fused_kernel(ix->eng, kdims, ix->row_stride, tune_or(TUNE_FLAT_TILE_KERNEL, 0) != 0, flat_scan_supported(ix->eng, kdims),
                                                   flat_scan_supported(kdims));
    const bool use_areg = kernel == fp::ScanKernel::RESIDENT_PLANES, use_fp4 = fp::scan_fp4(kernel, ix->eng, tune_or(TUNE_FLAT_FP4, 1) != 0);
    // Scan schedule (flat_plan.h).  The first candidates go through the unfused path — score matrix + segmented selection — and seed
    // every query's threshold; from then on chunks grow and the fused kernel appends only what beats the threshold.  An adversarially
    // ordered corpus can still overflow the append buffer; that is detected on the device and the call is repeated on the unfused path,
    // so the result never depends on the shortcut.  Tuning knob flat_unfused = 1 forces that path.
    // Survivors per query: the smallest pool that holds the 5 * top_k rerank candidates (64 for top_k <= 12, as ever).  Every buffer
    // below is sized and indexed by this call's P, not by the widest call the handle has served.
    const fp::Scan plan = fp::code_scan(n, B, top_k, tune_or(TUNE_FLAT_UNFUSED, 0) != 0, kernel);
    const u32 P = plan.P, R = P / SEL;
    const int pf = (int)tune_or(TUNE_FLAT_PF, 1); // the tile kernel's k panels in flight
    int n_cus = 0;
    if (hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, ix->p.device) != hipSuccess || n_cus <= 0) n_cus = 256;
    hipStream_t st = ix->own_stream;
    {
        std::lock_guard<std::mutex> g(ix->mu);
        if (!ix->flat_ws) ix->flat_ws = new FlatWs();
    }
    FlatWs *W = ix->flat_ws;
    std::lock_guard<std::mutex> wg(W->mu);
    float *d_q = nullptr, *d_qm = nullptr, *d_qrm = nullptr, *d_scores = nullptr, *d_os = nullptr;
    uint8_t *d_qc = nullptr, *d_qd = nullptr, *d_qdp = nullptr;
    u32 *d_qs = nullptr, *d_cs = nullptr, *d_oi = nullptr, *d_oc = nullptr, *d_zero = nullptr, *d_appcnt = nullptr;
    u64 *d_pool = nullptr, *d_part = nullptr, *d_thr = nullptr, *d_app = nullptr;
    ScanMask sm{nullptr, nullptr, 0u}; // masked call: the effective masks (W->mask)
    const u32 *d_uni = nullptr;        // ... and the union of the queries' live sets
    size_t n_ev = 0; // (start, stop) events of the GEMM launches, read after the last one
    float gemm_ms = 0.f;
    u32 launches = 0;
    double streamed = 0.0;
    bool zero = false;
    hipError_t e = hipSuccess;
    auto need = [&e](auto &buf, auto *&ptr, size_t count) { // the workspace's buffer grown to `count` elements
        if (e == hipSuccess) { e = buf.grow(count); ptr = buf; }
    };
    for (int attempt = 0; attempt < 2 && e == hipSuccess; attempt++) {
        // the score matrix and the selection's lists: as wide as this attempt's first chunk, its widest unfused one
        const u64 s_stride = fp::score_stride(plan.first(attempt));
        const u32 S = fp::select_segments(B, plan.first(attempt));
        if (attempt == 0) {
            need(W->q, d_q, (size_t)B * dim);
            need(W->zero, d_zero, 2);
            if (e == hipSuccess) e = hipMemsetAsync(d_zero, 0, 8, st);
            need(W->qm, d_qm, B);
            need(W->qrm, d_qrm, B);
            need(W->qc, d_qc, (size_t)B * ix->row_stride);
            need(W->qd, d_qd, (size_t)B * kdims);
            if (use_areg) need(W->qdp, d_qdp, (size_t)B * kdims);
            need(W->qs, d_qs, B);
            need(W->cs, d_cs, (size_t)n + 1);
            need(W->pool, d_pool, (size_t)B * P);
            need(W->thr, d_thr, B);
            need(W->app, d_app, (size_t)B * plan.app_cap());
            need(W->appcnt, d_appcnt, B);
            need(W->oi, d_oi, (size_t)B * top_k);
            need(W->os, d_os, (size_t)B * top_k);
            need(W->oc, d_oc, B);
            if (e == hipSuccess && mp.masked) e = scan_mask_upload(ix, mask, mp, B, W->mask, st, sm, &d_uni);
            if (e == hipSuccess) e = hipMemcpyAsync(d_q, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = launch_quantize_rows(ix->eng, d_q, dim, B, dim, ix->p.range_lo, ix->p.range_hi, d_qc, ix->row_stride, d_qm, d_qrm, st);
            if (e == hipSuccess && ix->eng == ENG_U8) {
                hipLaunchKernelGGL(code_sums_kernel, dim3((B + 3) / 4), dim3(256), 0, st, d_qc, ix->row_stride, B, d_qs);
                if (!W->cs_valid || W->cs_n != n) { // the stored vectors' sums: once per upload
                    hipLaunchKernelGGL(code_sums_kernel, dim3((n + 3) / 4), dim3(256), 0, st, ix->d_codes, ix->row_stride, n, d_cs);
                    W->cs_valid = true;
                    W->cs_n = n;
                }
                e = hipGetLastError();
            }
            if (e == hipSuccess && planes) {
                e = launch_expand_digits(ix->eng, d_qc, ix->row_stride, B, kdims, d_qd, st);
                if (e == hipSuccess && use_areg) e = launch_flat_scan_expand_queries(ix->eng, d_qc, ix->row_stride, B, kdims, d_qdp, st, use_fp4);
            }
            // zero-norm screening (cosine): the reference aborts a search on the first zero denominator it meets; an
            // exhaustive scan meets every vector, so any zero |q| or zero |v| is a CalculationError for the call.
            // The stored vectors' answer is computed once per upload (and read back then); the queries' flag stays on the device and comes
            // back with the results: a call with a zero-norm query runs its scan for nothing and then reports the error — until round 6
            // every call stopped here for a device round trip (~50 us of a 1.9 ms call) before its first GEMM.
            // A masked call screens the rows that are live for at least one of its queries, every time (the answer is the masks'); its flag
            // travels back with the queries' flag.
            if (e == hipSuccess && ix->p.metric == COS_METRIC_COSINE && mp.masked) {
                hipLaunchKernelGGL(any_zero_masked_kernel, dim3(1024), dim3(256), 0, st, (const float *)ix->d_mags, n, d_uni, d_zero);
                hipLaunchKernelGGL(any_zero_kernel, dim3(64), dim3(256), 0, st, (const float *)d_qm, B, d_zero);
                e = hipGetLastError();
            } else if (e == hipSuccess && ix->p.metric == COS_METRIC_COSINE) {
                if (!W->zn_valid || W->zn_n != n) {
                    u32 hz = 0;
                    hipLaunchKernelGGL(any_zero_kernel, dim3(1024), dim3(256), 0, st, (const float *)ix->d_mags, n, d_zero);
                    e = hipGetLastError();
                    if (e == hipSuccess) e = hipMemcpyAsync(&hz, d_zero, 4, hipMemcpyDeviceToHost, st);
                    if (e == hipSuccess) e = hipStreamSynchronize(st);
                    if (e == hipSuccess) { W->zn_valid = true; W->zn_n = n; W->zn_zero = hz != 0; }
                    if (e == hipSuccess) e = hipMemsetAsync(d_zero, 0, 4, st);
                }
                if (e == hipSuccess && W->zn_zero) { zero = true; break; }
                if (e == hipSuccess) {
                    hipLaunchKernelGGL(any_zero_kernel, dim3(64), dim3(256), 0, st, (const float *)d_qm, B, d_zero);
                    e = hipGetLastError();
                }
            }
        }
        need(W->scores, d_scores, (size_t)B * s_stride);
        need(W->part, d_part, (size_t)B * S * P);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(flat_reset_kernel, dim3(64), dim3(256), 0, st, d_pool, (u64)B * P, d_thr, d_appcnt, B, d_zero + 1); // (d_zero + 1: overflow flag of the fused path)
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            const ScanBufs bufs{d_scores, s_stride, d_part, d_pool, d_thr, d_app, d_appcnt, d_zero + 1, sm};
            const FusedOut fo = bufs.fused_out(plan, d_qd);
            const CodesGemm tile{d_qc, d_qm, d_qs, B, ix->d_codes, ix->d_mags, d_cs, ix->row_stride, kdims, ix->p.metric, d_scores, s_stride, fo};
            // a chunk's scoring kernel stands between a (start, stop) pair of events, read after the last chunk
            e = run_chunks(plan, attempt, bufs, st, [&](const fp::Chunk &c) {
                hipEvent_t ev0 = nullptr, ev1 = nullptr;
                hipError_t ce = W->event(n_ev, &ev0);
                if (ce == hipSuccess) ce = W->event(n_ev + 1, &ev1);
                if (ce == hipSuccess) { n_ev += 2; ce = hipEventRecord(ev0, st); }
                if (ce != hipSuccess) return ce;
                if (c.fused && kernel == fp::ScanKernel::RESIDENT_PLANES)
                    ce = launch_flat_scan(ix->eng, kdims, (u32)n_cus, st, d_qdp, d_qm, B, ix->d_codes, ix->d_mags, ix->row_stride, c.n0, c.nc, ix->p.metric, fo, use_fp4);
                else if (c.fused && kernel == fp::ScanKernel::RESIDENT_U8)
                    ce = launch_flat_scan_u8(kdims, (u32)n_cus, st, d_qc, d_qs, d_qm, B, ix->d_codes, d_cs, ix->d_mags, ix->row_stride, c.n0, c.nc, ix->p.metric, fo);
                else
                    ce = launch_codes_gemm(ix->eng, c.fused, pf, mp.masked, tile, c.n0, c.nc, st);
                if (ce != hipSuccess) return ce;
                launches++;
                streamed += (double)c.nc * (double)ix->row_stride * (double)((B + CM - 1) / CM);
                return hipEventRecord(ev1, st);
            });
        }
        // rerank, then ONE copy back: results, the zero-norm flag of the queries and the overflow flag of the fused path.  (Until round 6: a
        // device round trip for the overflow flag, then the rerank, then three pageable copies.)  An overflow repeats the scan unfused.
        const size_t nk = (size_t)B * top_k, out_words = 2 * nk + B + 2;
        if (e == hipSuccess) e = W->out.grow(out_words);
        if (e == hipSuccess) e = W->h_out.grow(out_words);
        if (e != hipSuccess) break;
        if (R == 1) {
            hipLaunchKernelGGL(flat_rerank_top5k, dim3(B), dim3(64), staged_query_bytes(dim), st, d_q, (u64)dim, d_qrm, B, ix->d_raw, (u64)dim,
                               ix->d_raw_mags, dim, d_pool, 5 * top_k, top_k, ix->p.id_base, d_oi, d_os, d_oc);
        } else {
            e = launch_flat_rerank_wide(R, false, d_q, (u64)dim, d_qrm, B, ix->d_raw, (u64)dim, ix->d_raw_mags, dim, d_pool, 5 * top_k, top_k, ix->p.id_base,
                                        d_oi, d_os, d_oc, st);
            if (e != hipSuccess) break;
        }
        hipLaunchKernelGGL(flat_pack_out_kernel, dim3((u32)((std::max<size_t>(nk, B) + 255) / 256)), dim3(256), 0, st, d_oi, d_os, d_oc, d_zero, B, top_k, W->out.p);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(W->h_out, W->out.p, out_words * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        const u32 *ho = W->h_out;
        zero = ho[2 * nk + B] != 0;
        const u32 hover = ho[2 * nk + B + 1];
        if (zero) break;
        if (plan.fused(attempt) && hover != 0) continue; // the append buffer overflowed: repeat unfused
        if (d_record) {
            e = hipMemcpyAsync(d_record, W->out.p, (2 * nk + B) * 4, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            break;
        }
        memcpy(out_ids, ho, nk * 4);
        memcpy(out_scores, ho + nk, nk * 4);
        memcpy(out_counts, ho + 2 * nk, (size_t)B * 4);
        break;
    }
    if (e == hipSuccess && !zero) {
        for (size_t i = 0; i + 1 < n_ev && e == hipSuccess; i += 2) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, W->evs[i], W->evs[i + 1]);
            gemm_ms += ms;
        }
    }
    if (stats) {
        stats->gemm_ms = gemm_ms;
        stats->gemm_launches = launches;
        stats->int8_ops = 2.0 * (double)B * (double)n * (double)kdims;
        stats->code_bytes = streamed;
    }
    HIP_TRY(e);
    if (zero) return cos_fail(COS_ERR_CALCULATION, "zero-norm query or stored vector: DistanceError::CalculationError (cosine.rs:228-232)");
    return COS_OK;
}

extern "C" int32_t cos_flat_search_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, uint32_t *out_ids, float *out_scores,
                                         uint32_t *out_counts, cos_flat_stats *stats) {
    return flat_search_run(ix, queries, B, top_k, nullptr, out_ids, out_scores, out_counts, stats);
}
extern "C" int32_t cos_flat_search_masked_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, const cos_scan_mask *mask, uint32_t *out_ids,
                                                float *out_scores, uint32_t *out_counts, cos_flat_stats *stats) {
    return flat_search_run(ix, queries, B, top_k, mask, out_ids, out_scores, out_counts, stats);
}

namespace cosdev {
// The per-shard forms of a shard set (shardset.hip): the single-index operator with its refusals and its zero-norm rule, the packed record
// [ids B*k | scores B*k | counts B] left in d_record on the index's device.
int32_t flat_search_record(cos_index *ix, const float *queries, u32 B, u32 top_k, const cos_scan_mask *mask, u32 *d_record) {
    if (!d_record) return cos_fail(COS_ERR_INVALID, "bad argument");
    return flat_search_run(ix, queries, B, top_k, mask, nullptr, nullptr, nullptr, nullptr, d_record);
}
int32_t bruteforce_record(cos_index *ix, const float *queries, u32 B, u32 k, const cos_scan_mask *mask, u32 *d_record) {
    if (!d_record) return cos_fail(COS_ERR_INVALID, "bad argument");
    return bruteforce_run(ix, queries, B, k, mask, nullptr, nullptr, nullptr, d_record);
}
} // namespace cosdev

// ---- the deleted set ----
hipError_t cos_deleted_reset(cos_index *ix, u32 n, hipStream_t st) {
    const size_t words = ((size_t)n + 31) / 32;
    hipError_t e = ix->d_deleted.alloc(words);
    if (e == hipSuccess) e = hipMemsetAsync(ix->d_deleted.p, 0, words * 4, st);
    return e;
}
hipError_t cos_deleted_grow(cos_index *ix, u32 n0, u32 n1, hipStream_t st) {
    const size_t w0 = ((size_t)n0 + 31) / 32, w1 = ((size_t)n1 + 31) / 32;
    DevArr<u32> grown;
    hipError_t e = grown.alloc(w1);
    if (e == hipSuccess) e = hipMemsetAsync(grown.p, 0, w1 * 4, st);
    // (bits at and past n0 of the old last word are clear: cos_index_delete refuses ids >= n)
    if (e == hipSuccess && ix->d_deleted.p) e = hipMemcpyAsync(grown.p, ix->d_deleted.p, w0 * 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st); // before the old bitmap is freed
    if (e == hipSuccess) grown.swap(ix->d_deleted);
    return e;
}
hipError_t cos_deleted_mark(cos_index *ix, const u32 *ids, u32 m, hipStream_t st) {
    if (m == 0) return hipSuccess;
    DevArr<u32> d_ids;
    hipError_t e = d_ids.alloc(m);
    if (e == hipSuccess && !ix->d_deleted.p) e = cos_deleted_reset(ix, ix->n, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ids.p, ids, (size_t)m * 4, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(deleted_mark_kernel, dim3((m + 255) / 256), dim3(256), 0, st, (const u32 *)d_ids.p, m, ix->d_deleted.p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st); // d_ids goes out of scope
    return e;
}
extern "C" int32_t cos_index_deleted_count(cos_index *ix, uint32_t *out) {
    if (!ix || !out) return cos_fail(COS_ERR_INVALID, "null argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 words = (ix->n + 31) / 32;
    hipStream_t st = ix->own_stream;
    DevArr<u32> d_cnt;
    HIP_TRY(d_cnt.alloc(1));
    hipError_t e = hipMemsetAsync(d_cnt.p, 0, 4, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(popcount_kernel, dim3(std::min<u32>((words + 255) / 256, 1024u)), dim3(256), 0, st, (const u32 *)ix->d_deleted.p, words, d_cnt.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_cnt.p, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    HIP_TRY(e);
    return COS_OK;
}
extern "C" int32_t cos_index_download_deleted(cos_index *ix, uint32_t *bits) {
    if (!ix || !bits) return cos_fail(COS_ERR_INVALID, "null argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(bits, ix->d_deleted.p, (size_t)((ix->n + 31) / 32) * 4, hipMemcpyDeviceToHost, ix->own_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->own_stream);
    HIP_TRY(e);
    return COS_OK;
}

// ------------------------------------------------------------------------------------------------
// Level table of the walk (WalkArgs::tab, walk_operands.hip cos_ensure_level_table / engine.hip run_search): similarity of every query of a big launch to
// every node of the graph's small upper levels, as ONE pass of the exact-integer i8 GEMM above with its unfused epilogue —
// `(u32 dot) as f32` and the IEEE quotient by |q| * |v|, the very operations the walk applies to a row it dots itself
// (cosine.rs:223-235), so the table holds the bits the walk would have computed.  The walk then reads 4 bytes per evaluation on
// those levels.  The nodes' code rows are gathered once per graph into a compact operand (level_table_gather).
// ------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void level_table_gather_kernel(const uint8_t *__restrict__ codes, const float *__restrict__ mags, u64 row_stride,
                                                                 const u32 *__restrict__ node_vec, u32 n, u32 col0, uint8_t *__restrict__ tcodes,
                                                                 float *__restrict__ tmags) {
    const int lane = threadIdx.x & 63;
    const u32 node = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (node >= n) return;
    const u32 row = node_vec[node];
    const uint4 *src = (const uint4 *)(codes + (u64)row * row_stride);
    uint4 *dst = (uint4 *)(tcodes + (u64)(col0 + node) * row_stride);
    for (u32 c = lane; c < (u32)(row_stride / 16); c += 64) dst[c] = src[c];
    if (lane == 0) tmags[col0 + node] = mags[row];
}
} // namespace

namespace cosdev {

hipError_t launch_level_table_gather(const uint8_t *codes, const float *mags, u64 row_stride, const u32 *node_vec, u32 n, u32 col0,
                                     uint8_t *tcodes, float *tmags, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(level_table_gather_kernel, dim3((n + 3) / 4), dim3(256), 0, st, codes, mags, row_stride, node_vec, n, col0, tcodes, tmags);
    return hipGetLastError();
}

hipError_t launch_code_sums(const uint8_t *codes, u64 row_stride, u32 n, u32 *sums, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(code_sums_kernel, dim3((n + 3) / 4), dim3(256), 0, st, codes, row_stride, n, sums);
    return hipGetLastError();
}

// storages with a level table: u8 codes (any row length: the tile kernel covers what the query-resident one does not) and quaternary
// codes whose dims the query-resident kernel is instantiated for (the tile kernel's quaternary path assumes whole 64-dim chunks too)
bool level_table_eng_supported(int eng, u64 row_stride) {
    return eng == ENG_U8 || (eng == ENG_Q2 && level_table_areg_supported(ENG_Q2, row_stride));
}

// tab[q][c] = the integer dot of query q with table column c (dot_product_u8 / dot_product_quaternary) `as f32` for q < B, c < ncols;
// u8 and quaternary codes.  The walk divides by |q| * |v|
// for the entries it reads (walk_kernel.inc, table levels): the GEMM's epilogue is an add, a convert and a store.  The
// query-resident kernel (kernels_scan.hip level_table_areg) wherever the code rows are whole 64-byte chunks with an
// instantiation (768, 1024, ...), the 256 x 128 tile kernel otherwise (and with tuning knob walk_table_gemm = 0); same table.
// qsums: the queries' code sums (u8; quantize_rows_kernel leaves them beside the codes).  The query-resident kernel's workgroups claim
// their work from *queue, which the caller zeroes before the FIRST launch over a table; a table may be computed by several launches of
// `wgs` workgroups each (0 = the full width), one after the other on `st`; `first` = this is the first of them (it prepares the
// quaternary query operand).  shared: the size of the work items (walk_plan.h table_gemm_stripe_tiles).
bool level_table_gemm_queue(int eng, u64 row_stride) { return level_table_areg_supported(eng, row_stride) && tune_or(TUNE_WALK_TABLE_GEMM, 1) != 0; }
hipError_t launch_level_table(int eng, const uint8_t *qcodes, const float *qmags, const u32 *qsums /*[B] (u8)*/, uint8_t *qdig /*[B][dims] scratch (quaternary)*/,
                              u32 B, const uint8_t *tcodes, const float *tmags, const u32 *tcsums, u64 row_stride, u32 ncols, float *tab, u64 tab_stride,
                              u32 n_cus, hipStream_t st, u32 *queue, u32 wgs, bool first, bool shared) {
    if (B == 0 || ncols == 0) return hipSuccess;
    const bool q2 = eng == ENG_Q2;
    const u32 kdims = q2 ? (u32)(row_stride / 16) * 64 : (u32)((row_stride + 63) / 64 * 64);
    hipError_t e = hipSuccess;
    if (level_table_gemm_queue(eng, row_stride)) {
        if (q2 && first) { // the queries' planes -> the permuted i8 digit rows the kernel keeps resident
            e = launch_flat_scan_expand_queries(ENG_Q2, qcodes, row_stride, B, kdims, qdig, st, false);
            if (e != hipSuccess) return e;
        }
        // (one workgroup per CU; on half the CUs — so that the previous launch's walk keeps the other half — the GEMM takes 1.31 instead
        // of 0.85 ms and the step 6.57 instead of 6.49: profiles/r05_table_gemm_half_the_cus_probe_not_kept.jsonl)
        return launch_level_table_areg(eng, n_cus ? n_cus : 256u, st, q2 ? qdig : qcodes, qsums, B, tcodes, tcsums, row_stride, ncols, tab, tab_stride, queue, wgs, shared);
    }
    if (!first) return hipSuccess; // (the tile kernel has no queue: one launch computes the table)
    const u32 metric = 1u; // the tile kernel's unfused epilogue with the dot-product metric: the converted integer dot, no quotient
    const CodesGemm g{qcodes, qmags, qsums, B, tcodes, tmags, tcsums, row_stride, kdims, metric, tab, tab_stride, FusedOut{nullptr, nullptr, nullptr, 0u, nullptr}};
    // unfused, two k panels in flight (one and three were measured slower in round 4)
    return launch_codes_gemm(q2 ? ENG_Q2 : ENG_U8, false, 2, false, g, 0u, ncols, st);
}

} // namespace cosdev
