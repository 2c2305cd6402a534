// kernels_flat_f16.hip — cos_flat_search_f16_batch: the exhaustive scan of kernels_flat.hip over HalfPrecisionFP rows.  The answer is
// the reference's finalisation over every row — sort by the f16 score, keep N = 5 * top_k, exact f32 rerank, top_k — but the f16 score
// is dot_product_f16 (dot_product.rs:13-19), ONE sequential f32 chain per row, which no MFMA reproduces.  So, as in the brute force:
//   flat_scan_f16     query-resident f16 MFMA GEMM (v_mfma_f32_32x32x16_f16, f32 accumulation): only GENERATES candidates, a pool of
//                     P >= 2 N per query, through the shared schedule (seed chunk unfused -> thresholds -> fused appends)
//   f16_margin_kernel flags the queries whose pool the MFMA's ranking may have cut wrongly (flat_plan.h f16_margin_safe)
//   f16_rescore       the P pool rows again in the reference's order, sorted: the first N are the reference's candidates
//   f16_exact_scores  flagged queries (exact_mode 1) or all (2): EVERY row in the reference's order where the MFMA wrote its score;
//                     the same selection and re-score follow
//   launch_flat_rerank  the code scan's exact f32 rerank of the N candidates, cut to top_k
// The scan kernel.  A workgroup is 4 waves; wave w keeps the A fragments of 32 query rows for the WHOLE k range in AccVGPRs (dim <=
// 1024: 4 dwords per 16 dims, 256 registers at 1024) — a wider row re-reads them from L2 step by step (NPAN = 0).  Row tiles of 64
// stored rows stream from HBM in 16-byte loads through double-buffered LDS, a k panel of 256 dims at a time (64 x 528 B; the panel
// after the one being multiplied is in flight in registers), every wave reads its B fragments from there: 32 MFMAs per panel between
// two barriers.  Both operands are read k-contiguous (8 f16 per lane, k block = lane >> 5), so the sum is the plain sum over k
// whatever the instruction's internal order.  Rows are padded to 16 bytes (row_stride = (2 dim + 15) & ~15): a piece past dim is never
// loaded, the piece that holds dim is masked, so the k tail is zero in LDS and in the fragments; a tail of at most 8 dims runs on
// v_mfma_f32_32x32x8_f16 instead of a half-empty x16 step.
// Masks and the deleted set: kernels_flat_f16_masked.hip (cos_flat_search_f16_masked_batch), a scan kernel of its own over the live
// tiles; the dot-product metric: kernels_flat_f16_dot.hip (cos_flat_search_f16_dot_batch); flat_f16.h holds what the three share.
// The shard set, f32 storage and top_k > 102 are not served (include/cosdata_hip.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "engine_internal.h"
#include "exact_rerank.h"
#include "flat_f16.h"
#include "flat_scan.h"

using namespace cosdev;
namespace fp = flat_plan;

namespace {

// scores of rows [n0, n0 + n_chunk) against the B queries.  Grid (workgroups that stride over the row tiles, ceil(B / 128)).
//   FUSED   the epilogue screens acc / |x| against the query's threshold * |q| and appends the survivors' keys (flat_gemm_f32's rule:
//           the exact quotient, the value that is ranked, is formed for estimates within 4e-6 of the threshold or above it)
//   !FUSED  scores[q][col] = acc / (|q| * |x|)
template <int NPAN /* k panels of resident fragments, dim <= 256 NPAN; 0 = any dim, fragments re-read per step */, bool FUSED>
__global__ __launch_bounds__(256) void flat_scan_f16(const uint8_t *__restrict__ qh /*[B][row_stride] f16 rows*/, const float *__restrict__ qmags, u32 B,
                                                     const uint8_t *__restrict__ codes, const float *__restrict__ mags, u64 row_stride, u32 n0, u32 n_chunk,
                                                     u32 dim, float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride, const FusedOut fo) {
    constexpr bool RES = NPAN > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char f16_lds[]; // [2][F_ROWS][F_LDP]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const u32 row0 = blockIdx.y * 128 + (u32)w * 32;
    const u32 n_tiles = (n_chunk + F_ROWS - 1) / F_ROWS, G = gridDim.x;
    u32 t = blockIdx.x;
    if (t >= n_tiles) return; // uniform
    const bool tail8 = (dim & 15u) != 0u && (dim & 15u) <= 8u; // the last dims run on the x8 form
    const u32 steps16 = tail8 ? dim / 16 : (dim + 15) / 16, kt = dim / 16 * 16;
    const u32 npan = RES ? (u32)NPAN : (dim + F_PAN - 1) / F_PAN;
    // this lane's query row: the A fragment of step s is its 8 halves at k = 16 s + 8 half (x8 tail: 4 halves at kt + 4 half)
    const u32 qrow = row0 + (u32)l31;
    const bool qv = qrow < B;
    const uint8_t *qp = qh + (u64)(qv ? qrow : 0u) * row_stride;
    auto qfrag = [&](u32 s) __attribute__((always_inline)) {
        const u32 k0 = 16 * s + 8 * (u32)half;
        i32x4 v = {0, 0, 0, 0};
        if (qv && k0 < dim) v = keep_halves(*(const i32x4 *)(qp + 2 * (u64)k0), (int)(dim - k0)); // 2 k0 + 16 <= row_stride
        return v;
    };
    i32x4 a[RES ? NPAN * 16 : 1];
    if constexpr (RES) {
        static_for<0, NPAN * 16>([&](auto Sc) __attribute__((always_inline)) {
            constexpr int s = decltype(Sc)::value;
            a[s] = qfrag((u32)s);
            asm volatile("" : "+a"(a[s]));
        });
    }
    i32x2 a8 = {0, 0};
    if (tail8) {
        const u32 k0 = kt + 4 * (u32)half;
        if (qv && k0 < dim) { // 2 k0 + 8 <= 2 kt + 16 <= row_stride
            const i32x2 v = *(const i32x2 *)(qp + 2 * (u64)k0);
            a8[0] = (int)keep_word((u32)v[0], (int)(dim - k0));
            a8[1] = (int)keep_word((u32)v[1], (int)(dim - k0) - 2);
        }
    }
    // per accumulator row: FUSED the bar an estimate acc / |x| must reach, threshold * |q| (+inf past B: nothing passes); else |q|
    float T[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const u32 row = row0 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half), rc = row < B ? row : B - 1;
        const float qm = qmags[rc];
        if constexpr (FUSED) {
            const u64 k = fo.thr[rc];
            const float tsc = simkey_inv((u32)(k >> 32));
            const float lo = k == 0ull ? -__builtin_inff() : tsc - 4e-6f * __builtin_fabsf(tsc); // 0 = pool not full: everything passes
            T[r] = row < B ? lo * qm : __builtin_inff();
        } else
            T[r] = qm;
    }
    // a panel of a tile: 64 rows x 32 pieces of 16 bytes, 32 consecutive threads per row; rows past the chunk re-read its last row
    i32x4 raw[F_NP];
    auto load_panel = [&](u32 tile, u32 pan) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < F_NP; p++) {
            const u32 g = (u32)p * 256u + (u32)tid, c = g >> 5, pc = g & 31u;
            const u32 col = tile * F_ROWS + c, cc = col < n_chunk ? col : n_chunk - 1;
            const u32 k0 = pan * F_PAN + pc * 8;
            i32x4 v = {0, 0, 0, 0};
            if (k0 < dim) { // 2 k0 + 16 <= row_stride
                v = *(const i32x4 *)(codes + (u64)(n0 + cc) * row_stride + 2 * (u64)k0);
                if (dim - k0 < 8u) v = keep_halves(v, (int)(dim - k0));
            }
            raw[p] = v;
        }
    };
    auto store_panel = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < F_NP; p++) {
            const u32 g = (u32)p * 256u + (u32)tid, c = g >> 5, pc = g & 31u;
            *(i32x4 *)(f16_lds + (size_t)buf * F_ROWS * F_LDP + (size_t)c * F_LDP + (size_t)pc * 16) = raw[p];
        }
    };
    load_panel(t, 0);
    store_panel(0);
    __syncthreads();
    int buf = 0;
    for (;; t += G) {
        const bool more_tiles = t + G < n_tiles; // uniform
        // the two column blocks' norms: requested in front of the k loop, used after it
        float xmj[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32 col = t * F_ROWS + 32 * (u32)j + (u32)l31;
            xmj[j] = mags[n0 + (col < n_chunk ? col : n_chunk - 1)];
        }
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[j][r] = 0.0f;
        auto panel = [&](auto Pc, u32 p) __attribute__((always_inline)) {
            constexpr int PI = decltype(Pc)::value;
            const bool last_p = p + 1 == npan, more = !last_p || more_tiles; // uniform
            if (more) load_panel(last_p ? t + G : t, last_p ? 0u : p + 1); // in flight while this panel is multiplied
            const unsigned char *brow = f16_lds + (size_t)buf * F_ROWS * F_LDP + (size_t)l31 * F_LDP;
            const u32 ns = steps16 > 16 * p ? steps16 - 16 * p : 0u; // x16 steps of this panel (16 unless it is the last)
            static_for<0, 16>([&](auto Sc) __attribute__((always_inline)) {
                constexpr int s = decltype(Sc)::value;
                if ((u32)s < ns) { // uniform
                    const i32x4 b0 = *(const i32x4 *)(brow + 32 * s + 16 * half), b1 = *(const i32x4 *)(brow + 32 * F_LDP + 32 * s + 16 * half);
                    i32x4 af;
                    if constexpr (RES) af = a[PI * 16 + s];
                    else af = qfrag(16 * p + (u32)s);
                    mfma16(acc[0], af, b0);
                    mfma16(acc[1], af, b1);
                }
            });
            if (tail8 && last_p) { // kt lies in the last panel
                const u32 off = 2 * (kt - p * F_PAN) + 8 * (u32)half;
                const i32x2 b0 = *(const i32x2 *)(brow + off), b1 = *(const i32x2 *)(brow + 32 * F_LDP + off);
                mfma8(acc[0], a8, b0);
                mfma8(acc[1], a8, b1);
            }
            if (more) store_panel(buf ^ 1); // the other buffer: every wave finished reading it before the last barrier
            __syncthreads();
            buf ^= 1;
        };
        if constexpr (RES) {
            static_for<0, NPAN>([&](auto Pc) __attribute__((always_inline)) { panel(Pc, (u32) decltype(Pc)::value); });
        } else {
            for (u32 p = 0; p < npan; p++) panel(std::integral_constant<int, 0>{}, p);
        }
        // epilogue: C/D layout of a 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32 col = t * F_ROWS + 32 * (u32)j + (u32)l31;
            const bool cv = col < n_chunk;
            const float xm = xmj[j];
            if constexpr (FUSED) {
                const float rx = __builtin_amdgcn_rcpf(xm);
                bool any = false;
                // NaN-safe: an estimate that is not provably below the bar takes the exact path
#pragma unroll
                for (int r = 0; r < 16; r++) any |= !(acc[j][r] * rx < T[r]);
                if (any && cv) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const u32 row = row0 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half);
                        if (row < B && !(acc[j][r] * rx < T[r])) {
                            const float sc = x86_div(acc[j][r], qmags[row] * xm);
                            const u64 key = score_key(sc, n0 + col);
                            if (key > fo.thr[row]) {
                                const u32 pos = atomicAdd(&fo.app_cnt[row], 1u);
                                if (pos < fo.cap) fo.app[(u64)row * fo.cap + pos] = key;
                            }
                        }
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const u32 row = row0 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half);
                    if (row < B && cv) scores[(u64)row * s_stride + col] = x86_div(acc[j][r], T[r] * xm);
                }
            }
        }
        if (!more_tiles) break;
    }
}

template <int NPAN>
hipError_t launch_scan_npan(bool fused, dim3 grid, hipStream_t st, const uint8_t *qh, const float *qmags, u32 B, const uint8_t *codes, const float *mags,
                            u64 row_stride, u32 n0, u32 nc, u32 dim, float *scores, u64 s_stride, const FusedOut &fo) {
    const auto kernel = fused ? flat_scan_f16<NPAN, true> : flat_scan_f16<NPAN, false>;
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)F16_SCAN_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), F16_SCAN_LDS, st, qh, qmags, B, codes, mags, row_stride, n0, nc, dim, scores, s_stride, fo);
    return hipGetLastError();
}
// rows [n0, n0 + nc) of the f16 codes against the B quantized queries: one workgroup per CU strides over the row tiles
hipError_t launch_f16_scan(bool fused, u32 n_cus, hipStream_t st, const uint8_t *qh, const float *qmags, u32 B, const uint8_t *codes, const float *mags,
                           u64 row_stride, u32 n0, u32 nc, u32 dim, float *scores, u64 s_stride, const FusedOut &fo) {
    const dim3 grid(std::min((nc + F_ROWS - 1) / F_ROWS, n_cus), (B + 127) / 128);
    const u32 npan = (dim + F_PAN - 1) / F_PAN;
#define F16_SCAN_ARGS fused, grid, st, qh, qmags, B, codes, mags, row_stride, n0, nc, dim, scores, s_stride, fo
    switch (npan <= (u32)F_MAX_NPAN ? npan : 0u) {
    case 1: return launch_scan_npan<1>(F16_SCAN_ARGS);
    case 2: return launch_scan_npan<2>(F16_SCAN_ARGS);
    case 3: return launch_scan_npan<3>(F16_SCAN_ARGS);
    case 4: return launch_scan_npan<4>(F16_SCAN_ARGS);
    default: return launch_scan_npan<0>(F16_SCAN_ARGS);
    }
#undef F16_SCAN_ARGS
}

// flags[q] = 1 and *n_flagged += 1 where flat_plan.h f16_margin_safe says no: the pool (sorted descending, P keys) is full and its P-th
// score is not more than twice the bound under its N-th.  One thread per query.
__global__ void f16_margin_kernel(const u64 *__restrict__ pool_mem, u32 P, u32 B, u32 N, u32 dim, u32 *__restrict__ flags, u32 *__restrict__ n_flagged) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    const u64 nth = pool_mem[(u64)q * P + N - 1], pth = pool_mem[(u64)q * P + P - 1];
    const bool safe = fp::f16_margin_safe(simkey_inv((u32)(nth >> 32)), simkey_inv((u32)(pth >> 32)), dim, (u32)(pth >> 32) != 0u);
    flags[q] = safe ? 0u : 1u;
    if (!safe) atomicAdd(n_flagged, 1u);
}

// The pool's rows again in the REFERENCE's order — dot_product_f16's sequential chain, one lane per row (f16_lane_dot), the quotient by
// |q| * |x| of cosine.rs:223-235 — and sorted by the key of that score (total_cmp descending, larger id first): sorted[q][0 .. N) are
// the reference's N candidates when the pool holds them (the margin rule, or an exact pass whose pool was selected by these very
// scores).  One workgroup per query; the sort is the shared LDS network.
template <u32 P>
__global__ __launch_bounds__(256) void f16_rescore(const uint8_t *__restrict__ qh, u64 row_stride, const float *__restrict__ qmags, const uint8_t *__restrict__ codes,
                                                   const float *__restrict__ mags, u32 dim, const u64 *__restrict__ pool_mem, u64 *__restrict__ sorted /*[B][P]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;                           // [dim], padded to 16 B
    u64 *keys = (u64 *)(smem_raw + staged_query_bytes(dim)); // [P]
    const u32 q = blockIdx.x;
    stage_f16_query(qf, qh + (u64)q * row_stride, dim);
    const float mq = qmags[q];
    for (u32 c = threadIdx.x; c < P; c += 256) {
        const u64 pk = pool_mem[(u64)q * P + c];
        const bool valid = pk != 0ull;
        const u32 sid = (u32)pk, row = valid ? sid : 0u;
        const float dp = f16_lane_dot(codes + (u64)row * row_stride, qf, dim);
        keys[c] = valid ? score_key(x86_div(dp, __fmul_rn(mq, mags[row])), sid) : 0ull;
    }
    lds_bitonic_sort_desc<P>(keys);
    for (u32 c = threadIdx.x; c < P; c += 256) sorted[(u64)q * P + c] = keys[c];
}
} // namespace
hipError_t cosdev::launch_f16_rescore(u32 P, const uint8_t *qh, u64 row_stride, const float *qmags, u32 B, const uint8_t *codes, const float *mags, u32 dim,
                              const u64 *pool, u64 *sorted, hipStream_t st) {
    const size_t smem = staged_query_bytes(dim) + (size_t)P * 8;
#define F16_RESCORE(PP) case PP: hipLaunchKernelGGL(f16_rescore<PP>, dim3(B), dim3(256), smem, st, qh, row_stride, qmags, codes, mags, dim, pool, sorted); break
    switch (P) {
        F16_RESCORE(64); F16_RESCORE(128); F16_RESCORE(256); F16_RESCORE(512); F16_RESCORE(1024);
        default: return hipErrorInvalidValue;
    }
#undef F16_RESCORE
    return hipGetLastError();
}
namespace {

// The exact path's scores: scores[q][c] = the reference-order score of row n0 + c, the value f16_rescore ranks, so the selection over
// this matrix keeps the exact top P.  One workgroup per (query, range of F16_EXACT_ROWS rows), one lane per row.
constexpr u32 F16_EXACT_ROWS = 1024;
__global__ __launch_bounds__(256) void f16_exact_scores(const uint8_t *__restrict__ qh, u64 row_stride, const float *__restrict__ qmags,
                                                        const uint8_t *__restrict__ codes, const float *__restrict__ mags, u32 n0, u32 n_chunk, u32 dim,
                                                        float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const u32 q = blockIdx.x;
    stage_f16_query(qf, qh + (u64)q * row_stride, dim);
    const float mq = qmags[q];
    const u32 c_begin = blockIdx.y * F16_EXACT_ROWS, c_end = c_begin + F16_EXACT_ROWS < n_chunk ? c_begin + F16_EXACT_ROWS : n_chunk;
    for (u32 c = c_begin + threadIdx.x; c < c_end; c += 256) {
        const u32 row = n0 + c;
        const float dp = f16_lane_dot(codes + (u64)row * row_stride, qf, dim);
        scores[(u64)q * s_stride + c] = x86_div(dp, __fmul_rn(mq, mags[row]));
    }
}

} // namespace

FlatF16Ws *cos_flat_f16_ws(cos_index *ix) {
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->flat_f16_ws) ix->flat_f16_ws = new FlatF16Ws();
    return ix->flat_f16_ws;
}
void cos_flat_f16_ws_release(cos_index *ix) {
    delete ix->flat_f16_ws;
    ix->flat_f16_ws = nullptr;
}

namespace {

// One pass over B queries under W->mu.  exact_pass: the flagged queries of an exact_mode 1 call again, every chunk unfused with its score
// matrix from f16_exact_scores; its rows replace the first answer's.
int32_t f16_run(cos_index *ix, FlatF16Ws *W, const float *queries, u32 B, u32 top_k, u32 mode, bool exact_pass, u32 *out_ids, float *out_scores,
                u32 *out_counts, cos_flat_f16_stats *stats) {
    const u32 dim = ix->p.dim, n = ix->n, N = fp::CODE_POOL_FACTOR * top_k;
    const bool exact = exact_pass || mode == fp::F16_EXACT_ALWAYS, by_rule = !exact && mode == fp::F16_EXACT_BY_RULE;
    const fp::Scan plan = fp::f16_scan(n, B, top_k, exact);
    const u32 P = plan.P, R = P / 64;
    const u64 row_stride = ix->row_stride;
    hipStream_t st = ix->own_stream;
    float *d_q = nullptr, *d_qm = nullptr, *d_qrm = nullptr, *d_scores = nullptr, *d_os = nullptr;
    uint8_t *d_qc = nullptr;
    u32 *d_flags = nullptr, *d_appcnt = nullptr, *d_oi = nullptr, *d_oc = nullptr, *d_qflag = nullptr;
    u64 *d_pool = nullptr, *d_sorted = nullptr, *d_thr = nullptr, *d_app = nullptr, *d_part = nullptr;
    hipError_t e = hipSuccess;
    auto need = [&e](auto &buf, auto *&ptr, size_t count) { // the workspace's buffer grown to `count` elements
        if (e == hipSuccess) { e = buf.grow(count); ptr = buf; }
    };
    need(W->q, d_q, (size_t)B * dim);
    need(W->qm, d_qm, B);
    need(W->qrm, d_qrm, B);
    need(W->qc, d_qc, (size_t)B * row_stride);
    need(W->flags, d_flags, 3);
    need(W->appcnt, d_appcnt, B);
    need(W->qflag, d_qflag, B);
    need(W->pool, d_pool, (size_t)B * P);
    need(W->sorted, d_sorted, (size_t)B * P);
    need(W->thr, d_thr, B);
    if (plan.allow_fused) need(W->app, d_app, (size_t)B * plan.app_cap());
    need(W->oi, d_oi, (size_t)B * top_k);
    need(W->os, d_os, (size_t)B * top_k);
    need(W->oc, d_oc, B);
    if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, 12, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_q, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, st);
    // the queries as f16 rows (f16::from_f32, padded with zeros) with the norm of the original vector (scalar.rs:41) and |q| of the rerank
    if (e == hipSuccess) e = launch_quantize_rows(ENG_F16, d_q, dim, B, dim, ix->p.range_lo, ix->p.range_hi, d_qc, row_stride, d_qm, d_qrm, st);
    // zero norms, as in the code scan: the stored rows' answer once per upload, the queries' flag comes back with the results
    bool zero = false;
    if (e == hipSuccess && !exact_pass) {
        if (!W->zn_valid || W->zn_n != n) {
            u32 hz = 0;
            e = launch_any_zero(ix->d_mags, n, d_flags, st);
            if (e == hipSuccess) e = hipMemcpyAsync(&hz, d_flags, 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e == hipSuccess) { W->zn_valid = true; W->zn_n = n; W->zn_zero = hz != 0; }
            if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, 4, st);
        }
        zero = e == hipSuccess && W->zn_zero;
        if (e == hipSuccess && !zero) e = launch_any_zero(d_qm, B, d_flags, st);
    }
    u32 hflags[3] = {0u, 0u, 0u};
    size_t n_ev = 0;
    u32 launches = 0;
    for (int attempt = 0; attempt < 2 && e == hipSuccess && !zero; attempt++) {
        // the score matrix and the selection's lists: as wide as this attempt's first chunk, its widest unfused one
        const u64 s_stride = fp::score_stride(plan.first(attempt));
        need(W->scores, d_scores, (size_t)B * s_stride);
        need(W->part, d_part, (size_t)B * fp::select_segments(B, plan.first(attempt)) * P);
        if (e == hipSuccess) e = launch_flat_reset(d_pool, (u64)B * P, d_thr, d_appcnt, B, d_flags + 1, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_flags + 2, 0, 4, st);
        if (e != hipSuccess) break;
        const ScanBufs bufs{d_scores, s_stride, d_part, d_pool, d_thr, d_app, d_appcnt, d_flags + 1, ScanMask{nullptr, nullptr, 0u}};
        const FusedOut fo = bufs.fused_out(plan, nullptr);
        // a chunk's scoring kernel stands between a (start, stop) pair of events, read after the last chunk
        e = run_chunks(plan, attempt, bufs, st, [&](const fp::Chunk &c) {
            hipEvent_t ev0 = nullptr, ev1 = nullptr;
            hipError_t ce = W->event(n_ev, &ev0);
            if (ce == hipSuccess) ce = W->event(n_ev + 1, &ev1);
            if (ce == hipSuccess) { n_ev += 2; ce = hipEventRecord(ev0, st); }
            if (ce != hipSuccess) return ce;
            if (exact) {
                hipLaunchKernelGGL(f16_exact_scores, dim3(B, (c.nc + F16_EXACT_ROWS - 1) / F16_EXACT_ROWS), dim3(256), staged_query_bytes(dim), st, (const uint8_t *)d_qc,
                                   row_stride, (const float *)d_qm, (const uint8_t *)ix->d_codes.p, (const float *)ix->d_mags.p, c.n0, c.nc, dim, d_scores, s_stride);
                ce = hipGetLastError();
            } else
                ce = launch_f16_scan(c.fused, ix->n_cus, st, d_qc, d_qm, B, ix->d_codes, ix->d_mags, row_stride, c.n0, c.nc, dim, d_scores, s_stride, fo);
            if (ce != hipSuccess) return ce;
            launches++;
            return hipEventRecord(ev1, st);
        });
        if (e == hipSuccess && by_rule) { // the pools are final (or about to be repeated): ranks N and P of each
            hipLaunchKernelGGL(f16_margin_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const u64 *)d_pool, P, B, N, dim, d_qflag, d_flags + 2);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = launch_f16_rescore(P, d_qc, row_stride, d_qm, B, ix->d_codes, ix->d_mags, dim, d_pool, d_sorted, st);
        if (e == hipSuccess) e = launch_flat_rerank(R, d_q, d_qrm, B, ix->d_raw, ix->d_raw_mags, dim, d_sorted, N, top_k, ix->p.id_base, d_oi, d_os, d_oc, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_ids, d_oi, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_scores, d_os, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_counts, d_oc, (size_t)B * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hflags, d_flags, 12, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        zero = hflags[0] != 0;
        if (!(plan.fused(attempt) && hflags[1] != 0)) break; // done; otherwise the append buffer overflowed: repeat unfused
    }
    std::vector<u32> h_flag;
    const u32 n_flagged = by_rule && !zero ? hflags[2] : 0u;
    if (e == hipSuccess && n_flagged) {
        h_flag.resize(B);
        e = hipMemcpyAsync(h_flag.data(), d_qflag, (size_t)B * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    float gemm_ms = 0.f;
    for (size_t i = 0; i + 1 < n_ev && e == hipSuccess && !zero; i += 2) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, W->evs[i], W->evs[i + 1]);
        gemm_ms += ms;
    }
    HIP_TRY(e);
    if (zero) return cos_fail(COS_ERR_CALCULATION, "zero-norm query or stored vector: DistanceError::CalculationError (cosine.rs:228-232)");
    if (stats && !exact_pass) {
        stats->queries = B;
        stats->exact_queries = exact ? B : n_flagged;
        stats->pool = P;
        stats->gemm_ms = gemm_ms;
        stats->gemm_launches = launches;
    }
    if (n_flagged == 0) return COS_OK;
    // the flagged queries again, exactly: the sub-batch's answer replaces theirs
    std::vector<u32> sel;
    for (u32 b = 0; b < B; b++)
        if (h_flag[b]) sel.push_back(b);
    const u32 Bx = (u32)sel.size();
    std::vector<float> xq((size_t)Bx * dim), xs((size_t)Bx * top_k);
    std::vector<u32> xi((size_t)Bx * top_k), xc(Bx);
    for (u32 i = 0; i < Bx; i++) memcpy(xq.data() + (size_t)i * dim, queries + (size_t)sel[i] * dim, (size_t)dim * 4);
    if (int32_t xrc = f16_run(ix, W, xq.data(), Bx, top_k, mode, true, xi.data(), xs.data(), xc.data(), nullptr)) return xrc;
    for (u32 i = 0; i < Bx; i++) {
        memcpy(out_ids + (size_t)sel[i] * top_k, xi.data() + (size_t)i * top_k, (size_t)top_k * 4);
        memcpy(out_scores + (size_t)sel[i] * top_k, xs.data() + (size_t)i * top_k, (size_t)top_k * 4);
        out_counts[sel[i]] = xc[i];
    }
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_flat_search_f16_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, const cos_flat_f16_opts *opts, uint32_t *out_ids,
                                             float *out_scores, uint32_t *out_counts, cos_flat_f16_stats *stats) {
    if (!ix || !queries || !out_ids || !out_scores || !out_counts || B == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    if (opts && opts->struct_size != sizeof(cos_flat_f16_opts)) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::struct_size is %u, expected %zu", opts->struct_size, sizeof(cos_flat_f16_opts));
    if (stats && stats->struct_size != sizeof(cos_flat_f16_stats) && stats->struct_size != COS_FLAT_F16_STATS_SIZE_V1)
        return cos_fail(COS_ERR_INVALID, "cos_flat_f16_stats::struct_size is %u, expected %zu (or %u)", stats->struct_size, sizeof(cos_flat_f16_stats), COS_FLAT_F16_STATS_SIZE_V1);
    const u32 mode = opts ? opts->exact_mode : (u32)fp::F16_EXACT_BY_RULE;
    if (mode > fp::F16_EXACT_ALWAYS) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::exact_mode is %u: 0, 1 or 2", mode);
    if (ix->eng != ENG_F16) return cos_fail(COS_ERR_STORAGE_MISMATCH, "cos_flat_search_f16_batch scans HalfPrecisionFP rows (cos_flat_search_batch: u8 and bit-plane codes)");
    if (ix->p.metric != COS_METRIC_COSINE) return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_flat_search_f16_batch implements the cosine metric (dot product: cos_flat_search_f16_dot_batch)");
    if (int32_t krc = fp::check_f16_top_k(top_k)) return cos_fail(krc, "the f16 scan keeps at most 1024 survivors (2 * 5 * top_k): top_k must be in [1, 102]");
    if (int32_t rc = cos_set_device(ix)) return rc;
    FlatF16Ws *W = cos_flat_f16_ws(ix);
    std::lock_guard<std::mutex> wg(W->mu);
    const int32_t rc = f16_run(ix, W, queries, B, top_k, mode, false, out_ids, out_scores, out_counts, stats);
    if (rc == COS_OK && stats && stats->struct_size == sizeof(cos_flat_f16_stats)) // every tile, for every block of queries
        stats->tiles_scanned = stats->tiles_total = fp::f16_tiles(ix->n) * fp::f16_query_blocks(B);
    return rc;
}
