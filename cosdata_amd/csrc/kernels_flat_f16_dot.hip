// kernels_flat_f16_dot.hip — cos_flat_search_f16_dot_batch: the exhaustive scan of a HalfPrecisionFP collection with the DOT-PRODUCT
// metric, masked or not.  The answer is cos_flat_search_f16_batch's with the dot metric's first-pass score: every live row scored by
// dot_product_f16 (ONE sequential f32 chain from -0.0, no quotient), sorted (desc, larger id first), the best N = 5 * top_k reranked
// exactly in f32 (cosine whatever the metric, as in the reference), top_k.  The stages are the cosine call's and so are the plan, the
// chunk driver, the pools and their folds, the selection, the workspace and the rerank (flat_plan.h, flat_scan.h, flat_f16.h); what is
// this file's own is everything that scores:
//   flat_scan_f16_dot     the candidate GEMM in raw dot units.  flat_scan_f16's data movement (four waves, each with the A fragments of
//                         32 queries resident in AccVGPRs up to 1024 dims, 64-row tiles through double-buffered 64 x 528 B LDS panels,
//                         v_mfma_f32_32x32x16_f16 and the x8 form for a k tail of at most 8) — but no norm is loaded anywhere, and the
//                         ranked value IS the accumulator: the fused epilogue compares score_key(acc, id) with the query's threshold
//                         key exactly, after one float compare in dot units.  No reciprocal estimate, no slack, no second quotient.
//                         The 128 thresholds of the query block sit in LDS (the float and the key), read per tile by the epilogue, so
//                         no register holds one across the k loop.  ONE kernel serves both calls: MASKED walks the query block's list
//                         of live tiles and tests the row's bit from LDS where a key is about to be appended, !MASKED strides over
//                         every tile.
//   f16d_exact_scores     the exact path: every (live) row by the sequential chain, written where the MFMA would write
//   f16d_rescore          the P pool rows again in the reference's order, sorted: the first N are the rerank's candidates
//   f16d_code_norms       f32 norms of f16 VALUES, rounded up: |q^| per query, and the largest stored row's, X^max, once per upload
//   f16d_margin_kernel    flat_plan.h f16_dot_margin_safe: g_N - g_P > 2 * 4 dim u |q^| X^max, or the query takes the exact path
// Thresholds and keys are in raw dot units throughout.  simkey is monotone over every finite f32 (device_common.h: total_cmp as an
// unsigned key) and at least 0x00800000 there, so the zero key of an empty slot and the zero threshold of a pool that is not full order
// below every finite score, negative ones included — the property kernels_brute_dot.hip relies on.
// There is no zero-norm error: the dot metric has none (the rerank's handling of such rows is launch_flat_rerank's, unchanged).
// Out of scope: the shard set, FullPrecisionFP storage, top_k > 102 and masks that are already on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"
#include "exact_rerank.h"
#include "flat_f16.h"
#include "flat_scan.h"

using namespace cosdev;
namespace fp = flat_plan;

namespace {

constexpr u32 QB = fp::F16_QUERY_BLOCK;
static_assert(QB == 128 && QB * 2 == 256, "four waves of 32 queries; one mask word per thread and tile");
// LDS: [2][F_ROWS][F_LDP] panels | FUSED: [128] threshold scores, [128] threshold keys | FUSED && MASKED: [3][128][2] mask words
constexpr size_t F16D_THR_OFF = F16_SCAN_LDS, F16D_KEY_OFF = F16D_THR_OFF + QB * 4, F16D_MASK_OFF = F16D_KEY_OFF + QB * 8;
constexpr size_t f16d_scan_lds(bool fused, bool masked) { return !fused ? F16_SCAN_LDS : !masked ? F16D_MASK_OFF : F16D_MASK_OFF + (size_t)3 * QB * 2 * 4; }
static_assert(2 * f16d_scan_lds(true, true) <= 160 * 1024, "two workgroups per CU");

// the live tiles of a query block: lists[block][0 .. list_len[block]) ascending tile numbers (row / 64)
struct DotTiles {
    const u32 *lists, *list_len;
    u32 stride; // tiles of the corpus
};
// first position of list[0 .. len) that holds a tile >= t
__device__ __forceinline__ u32 first_tile_at(const u32 *__restrict__ list, u32 len, u32 t) {
    u32 lo = 0, hi = len;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (list[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// dots of rows [n0, n0 + n_chunk) with the B queries' f16 codes.  Grid (workgroups that stride over the tiles, ceil(B / 128)).
//   MASKED  the tiles are those of the block's list inside the chunk (n0 a multiple of 64); a workgroup past the list's end leaves
//   FUSED   a score not below its query's threshold becomes a key; the key is appended where it beats the threshold key and (MASKED)
//           bit `row` of the query's effective mask is set
//   !FUSED  scores[q][col] = acc for the columns of the tiles visited (a masked selection reads live columns only)
template <int NPAN /* k panels of resident fragments, dim <= 256 NPAN; 0 = any dim, fragments re-read per step */, bool FUSED, bool MASKED>
__global__ __launch_bounds__(256) void flat_scan_f16_dot(const uint8_t *__restrict__ qh /*[B][row_stride] f16 rows*/, u32 B, const uint8_t *__restrict__ codes,
                                                         u64 row_stride, u32 n0, u32 n_chunk, u32 dim, float *__restrict__ scores /*[B][s_stride]*/,
                                                         u64 s_stride, const FusedOut fo, const DotTiles tl) {
    constexpr bool RES = NPAN > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char f16_lds[];
    float *thr_dot = (float *)(f16_lds + F16D_THR_OFF);
    u64 *thr_key = (u64 *)(f16_lds + F16D_KEY_OFF);
    u32 *mask_lds = (u32 *)(f16_lds + F16D_MASK_OFF);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const u32 row0 = blockIdx.y * QB + (u32)w * 32, G = gridDim.x;
    // the tiles of this workgroup: positions pos, pos + G, ... below pos_end — of the block's list (MASKED) or of the chunk
    const u32 t_base = n0 / F_ROWS;
    const u32 *__restrict__ list = nullptr;
    u32 pos = blockIdx.x, pos_end = (n_chunk + F_ROWS - 1) / F_ROWS;
    if constexpr (MASKED) {
        list = tl.lists + (u64)blockIdx.y * tl.stride;
        const u32 len = tl.list_len[blockIdx.y];
        pos_end = first_tile_at(list, len, (n0 + n_chunk + F_ROWS - 1) / F_ROWS);
        pos += first_tile_at(list, len, t_base);
    }
    if (pos >= pos_end) return; // uniform
    auto tile_at = [&](u32 p) __attribute__((always_inline)) { // the chunk's tile at a position
        if constexpr (MASKED) return list[p] - t_base;
        else return p;
    };
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
    // the block's thresholds, once per launch (a fold between two launches moves them): the key, and the score it encodes for the
    // screen.  A key of 0 = no threshold yet: every (live) row passes.  A row past the batch keeps nothing.
    if constexpr (FUSED) {
        if (tid < (int)QB) {
            const u32 row = blockIdx.y * QB + (u32)tid;
            const u64 key = row < B ? fo.thr[row] : ~0ull;
            thr_key[tid] = key;
            thr_dot[tid] = row >= B ? __builtin_inff() : key == 0ull ? -__builtin_inff() : simkey_inv((u32)(key >> 32));
        }
    }
    // this thread's share of a tile's mask words: word (tid & 1) of the tile for query (tid >> 1) of the block; 0 past B and past the mask
    const u32 *mrow = nullptr;
    if constexpr (FUSED && MASKED) {
        const u32 mq = blockIdx.y * QB + ((u32)tid >> 1);
        if (mq < B) mrow = fo.m.bits + (u64)fo.m.qmask[mq] * fo.m.words;
    }
    auto load_mask = [&](u32 tile) __attribute__((always_inline)) {
        const u32 wi = 2 * (tile + t_base) + ((u32)tid & 1u);
        return mrow && wi < fo.m.words ? mrow[wi] : 0u;
    };
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
    u32 t = tile_at(pos);
    load_panel(t, 0);
    store_panel(0);
    if constexpr (FUSED && MASKED) mask_lds[tid] = load_mask(t);
    __syncthreads(); // the first panel, the thresholds, the first tile's mask words
    int buf = 0;
    u32 mbuf = 0, mw_next = 0;
    for (;; pos += G) {
        const bool more_tiles = pos + G < pos_end; // uniform
        const u32 t_next = more_tiles ? tile_at(pos + G) : t;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[j][r] = 0.0f;
        auto panel = [&](auto Pc, u32 p) __attribute__((always_inline)) {
            constexpr int PI = decltype(Pc)::value;
            const bool last_p = p + 1 == npan, more = !last_p || more_tiles; // uniform
            if (more) {
                load_panel(last_p ? t_next : t, last_p ? 0u : p + 1); // in flight while this panel is multiplied
                if constexpr (FUSED && MASKED)
                    if (last_p) mw_next = load_mask(t_next);
            }
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
            if (more) {
                store_panel(buf ^ 1); // the other buffer: every wave finished reading it before the last barrier
                // the next tile's words go two buffers ahead of the one a slower wave's epilogue may still be reading
                if constexpr (FUSED && MASKED)
                    if (last_p) mask_lds[(mbuf + 1) % 3 * 256 + (u32)tid] = mw_next;
            }
            __syncthreads();
            buf ^= 1;
        };
        if constexpr (RES) {
            static_for<0, NPAN>([&](auto Pc) __attribute__((always_inline)) { panel(Pc, (u32) decltype(Pc)::value); });
        } else {
            for (u32 p = 0; p < npan; p++) panel(std::integral_constant<int, 0>{}, p);
        }
        // epilogue: C/D layout of a 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  Registers 4 g .. 4 g + 3
        // are four consecutive queries of the block: their thresholds are one 16-byte LDS read, the same address for a half-wave
        if constexpr (FUSED) {
            float td[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float4 v = *(const float4 *)(thr_dot + w * 32 + 8 * g + 4 * half);
                td[4 * g] = v.x, td[4 * g + 1] = v.y, td[4 * g + 2] = v.z, td[4 * g + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const u32 col = t * F_ROWS + 32 * (u32)j + (u32)l31; // row n0 + col of the corpus: bit l31 of the tile's word j
                bool any = false;
                // NaN-safe: a score that is not provably below the bar goes on to the key compare
#pragma unroll
                for (int r = 0; r < 16; r++) any |= !(acc[j][r] < td[r]);
                if (any && col < n_chunk) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const u32 rl = (u32)w * 32 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half);
                        if (!(acc[j][r] < td[r])) {
                            const u64 key = score_key(acc[j][r], n0 + col);
                            bool keep = key > thr_key[rl]; // ~0 past the batch: nothing is kept
                            if constexpr (MASKED) keep = keep && ((mask_lds[mbuf * 256 + rl * 2 + (u32)j] >> l31) & 1u) != 0u;
                            if (keep) {
                                const u32 row = blockIdx.y * QB + rl;
                                const u32 at = atomicAdd(&fo.app_cnt[row], 1u);
                                if (at < fo.cap) fo.app[(u64)row * fo.cap + at] = key;
                            }
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const u32 col = t * F_ROWS + 32 * (u32)j + (u32)l31;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const u32 row = row0 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half);
                    if (row < B && col < n_chunk) scores[(u64)row * s_stride + col] = acc[j][r];
                }
            }
        }
        if (!more_tiles) break;
        t = t_next;
        mbuf = (mbuf + 1) % 3;
    }
}

struct DotScanArgs { // what every chunk's launch repeats
    const uint8_t *qh;
    u32 B;
    const uint8_t *codes;
    u64 row_stride;
    u32 dim;
    float *scores;
    u64 s_stride;
    FusedOut fo;
    DotTiles tl;
};
template <int NPAN, bool FUSED, bool MASKED>
hipError_t launch_scan_inst(dim3 grid, hipStream_t st, const DotScanArgs &a, u32 n0, u32 nc) {
    constexpr size_t lds = f16d_scan_lds(FUSED, MASKED);
    const auto kernel = flat_scan_f16_dot<NPAN, FUSED, MASKED>;
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a.qh, a.B, a.codes, a.row_stride, n0, nc, a.dim, a.scores, a.s_stride, a.fo, a.tl);
    return hipGetLastError();
}
template <int NPAN>
hipError_t launch_scan_npan(bool fused, bool masked, dim3 grid, hipStream_t st, const DotScanArgs &a, u32 n0, u32 nc) {
    if (masked) return fused ? launch_scan_inst<NPAN, true, true>(grid, st, a, n0, nc) : launch_scan_inst<NPAN, false, true>(grid, st, a, n0, nc);
    return fused ? launch_scan_inst<NPAN, true, false>(grid, st, a, n0, nc) : launch_scan_inst<NPAN, false, false>(grid, st, a, n0, nc);
}
// rows [n0, n0 + nc): as many workgroups as the chunk has tiles, at most one per CU and query block — a masked block's list says how
// many of them find work
hipError_t launch_f16_dot_scan(bool fused, bool masked, u32 n_cus, hipStream_t st, const DotScanArgs &a, u32 n0, u32 nc) {
    if (masked && n0 % F_ROWS) return hipErrorInvalidValue; // a tile of the lists is a tile of the chunk
    const dim3 grid(std::min((nc + F_ROWS - 1) / F_ROWS, n_cus), (a.B + QB - 1) / QB);
    const u32 npan = (a.dim + F_PAN - 1) / F_PAN;
    switch (npan <= (u32)F_MAX_NPAN ? npan : 0u) {
    case 1: return launch_scan_npan<1>(fused, masked, grid, st, a, n0, nc);
    case 2: return launch_scan_npan<2>(fused, masked, grid, st, a, n0, nc);
    case 3: return launch_scan_npan<3>(fused, masked, grid, st, a, n0, nc);
    case 4: return launch_scan_npan<4>(fused, masked, grid, st, a, n0, nc);
    default: return launch_scan_npan<0>(fused, masked, grid, st, a, n0, nc);
    }
}

// ---- the exact-order kernels: dot_product_f16's chain, no quotient ----
// scores[q][c] = the reference-order dot of row n0 + c, the value f16d_rescore ranks, so the selection over this matrix keeps the exact
// top P.  One workgroup per (query, range of F16D_EXACT_ROWS rows), one lane per row.  MASKED (n0 a multiple of 64): only the query's
// live rows are scored and written; a range without a live tile ends at once, a wave skips a dead tile through the per-mask tile bits.
constexpr u32 F16D_EXACT_ROWS = 1024;
template <bool MASKED>
__global__ __launch_bounds__(256) void f16d_exact_scores(const uint8_t *__restrict__ qh, u64 row_stride, const uint8_t *__restrict__ codes, u32 n0, u32 n_chunk,
                                                         u32 dim, float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride, const ScanMask m,
                                                         const u64 *__restrict__ tile_bits, u32 tb_stride, u32 tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const u32 q = blockIdx.x;
    const u32 c_begin = blockIdx.y * F16D_EXACT_ROWS, c_end = c_begin + F16D_EXACT_ROWS < n_chunk ? c_begin + F16D_EXACT_ROWS : n_chunk;
    const u64 *tb = MASKED ? tile_bits + (u64)m.qmask[q] * tb_stride : nullptr;
    auto tile_live = [&](u32 t) { return !MASKED || (t < tiles && ((tb[t >> 6] >> (t & 63u)) & 1ull) != 0ull); };
    if constexpr (MASKED) {
        bool any = false;
        for (u32 i = 0; i < F16D_EXACT_ROWS / F_ROWS; i++) any |= tile_live((n0 + c_begin) / F_ROWS + i);
        if (!any) return; // uniform: nothing of this query lives in the range
    }
    stage_f16_query(qf, qh + (u64)q * row_stride, dim);
    for (u32 c0 = c_begin; c0 < c_end; c0 += 256) {
        const u32 c = c0 + threadIdx.x, row = n0 + c;
        if (!tile_live((n0 + c0) / F_ROWS + (threadIdx.x >> 6))) continue; // the wave's tile
        if (c < c_end && scan_live<MASKED>(m, q, row)) scores[(u64)q * s_stride + c] = f16_lane_dot(codes + (u64)row * row_stride, qf, dim);
    }
}

// The pool's rows again in the reference's order and sorted by the key of that dot (total_cmp descending, larger id first):
// sorted[q][0 .. N) are the reference's N candidates when the pool holds them.  Empty keys stay empty and sort last.  One workgroup
// per query; the sort is the shared LDS network.
template <u32 P>
__global__ __launch_bounds__(256) void f16d_rescore(const uint8_t *__restrict__ qh, u64 row_stride, const uint8_t *__restrict__ codes, u32 dim,
                                                    const u64 *__restrict__ pool_mem, u64 *__restrict__ sorted /*[B][P]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;                           // [dim], padded to 16 B
    u64 *keys = (u64 *)(smem_raw + staged_query_bytes(dim)); // [P]
    const u32 q = blockIdx.x;
    stage_f16_query(qf, qh + (u64)q * row_stride, dim);
    for (u32 c = threadIdx.x; c < P; c += 256) {
        const u64 pk = pool_mem[(u64)q * P + c];
        const bool valid = pk != 0ull;
        const u32 sid = (u32)pk;
        const float dp = f16_lane_dot(codes + (u64)(valid ? sid : 0u) * row_stride, qf, dim);
        keys[c] = valid ? score_key(dp, sid) : 0ull;
    }
    lds_bitonic_sort_desc<P>(keys);
    for (u32 c = threadIdx.x; c < P; c += 256) sorted[(u64)q * P + c] = keys[c];
}
hipError_t launch_f16d_rescore(u32 P, const uint8_t *qh, u64 row_stride, u32 B, const uint8_t *codes, u32 dim, const u64 *pool, u64 *sorted, hipStream_t st) {
    const size_t smem = staged_query_bytes(dim) + (size_t)P * 8;
#define F16D_RESCORE(PP) case PP: hipLaunchKernelGGL(f16d_rescore<PP>, dim3(B), dim3(256), smem, st, qh, row_stride, codes, dim, pool, sorted); break
    switch (P) {
        F16D_RESCORE(64); F16D_RESCORE(128); F16D_RESCORE(256); F16D_RESCORE(512); F16D_RESCORE(1024);
        default: return hipErrorInvalidValue;
    }
#undef F16D_RESCORE
    return hipGetLastError();
}

// ---- the margin rule ----
// The f32 norm of each of n f16 rows, from the f16 VALUES, rounded UP: squares of f16 values are exact in f32, their f32 sum (any
// order) is within dim u of the true sum, the root within dim u / 2 + u, and the factor (1 + dim u) covers both; the three roundings
// of forming and applying it (at most u each) are paid back by three ulps (at least u each) added to the result's bits.  One wave per
// row, a lane per pair of halves.  EACH: out[row] = the norm; else *out = max of the norms' bits (norms are >= 0, where the order of
// the bits is the order of the values; an infinity or a NaN ends above every number and no pool is trusted), *out zeroed before the
// launch.
template <bool EACH>
__global__ __launch_bounds__(256) void f16d_code_norms(const uint8_t *__restrict__ codes, u64 row_stride, u32 n, u32 dim, float *__restrict__ out) {
    const u32 lane = threadIdx.x & 63u, waves = gridDim.x * 4u;
    const float up = __fadd_rn(1.0f, (float)dim * (1.0f / 16777216.0f));
    u32 best = 0u;
    for (u32 row = blockIdx.x * 4u + (threadIdx.x >> 6); row < n; row += waves) { // wave-uniform
        const uint8_t *rp = codes + (u64)row * row_stride;
        float s = 0.0f;
        for (u32 i = 2 * lane; i < dim; i += 128) { // 2 i + 4 <= row_stride: rows are padded to 16 bytes
            const u32 wv = *(const u32 *)(rp + 2 * (u64)i);
            const float lo = __half2float(__ushort_as_half((unsigned short)(wv & 0xFFFFu)));
            const float hi = i + 1 < dim ? __half2float(__ushort_as_half((unsigned short)(wv >> 16))) : 0.0f;
            s = __fadd_rn(s, __fadd_rn(__fmul_rn(lo, lo), __fmul_rn(hi, hi)));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
        const float nrm = __uint_as_float(__float_as_uint(__fmul_rn(__fsqrt_rn(s), up)) + 3u); // s >= 0: the bits count upwards
        if constexpr (EACH) {
            if (lane == 0) out[row] = nrm;
        } else {
            const u32 b = __float_as_uint(nrm) & 0x7FFFFFFFu;
            best = b > best ? b : best;
        }
    }
    if constexpr (!EACH)
        if (lane == 0 && best) atomicMax((u32 *)out, best);
}
// X^max of the stored rows on the device, once per upload: the workspace — and the cached value with it — is dropped by every upload and
// append (cos_flat_ws_release)
hipError_t f16d_xmax_ensure(cos_index *ix, FlatF16Ws *W, hipStream_t st) {
    if (W->xmax_valid && W->xmax_n == ix->n) return hipSuccess;
    hipError_t e = W->xmax.grow(1);
    if (e == hipSuccess) e = hipMemsetAsync(W->xmax.p, 0, 4, st);
    if (e != hipSuccess) return e;
    const u32 wgs = std::min((ix->n + 3) / 4, 4096u);
    hipLaunchKernelGGL(f16d_code_norms<false>, dim3(wgs), dim3(256), 0, st, (const uint8_t *)ix->d_codes.p, ix->row_stride, ix->n, ix->p.dim, (float *)W->xmax.p);
    e = hipGetLastError();
    if (e == hipSuccess) { W->xmax_valid = true; W->xmax_n = ix->n; }
    return e;
}

// flags[q] = 1 and *n_flagged += 1 where flat_plan.h f16_dot_margin_safe says no.  The pool is sorted descending, P keys.  qmask /
// live set: a masked call, where a query with at most P live rows is not tested.  One thread per query.
__global__ void f16d_margin_kernel(const u64 *__restrict__ pool_mem, u32 P, u32 B, u32 N, u32 dim, const float *__restrict__ qnorm,
                                   const u32 *__restrict__ xmax_bits, const u32 *__restrict__ qmask, const u32 *__restrict__ live, u32 *__restrict__ flags,
                                   u32 *__restrict__ n_flagged) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    const u64 nth = pool_mem[(u64)q * P + N - 1], pth = pool_mem[(u64)q * P + P - 1];
    const float gn = simkey_inv((u32)(nth >> 32)), gp = simkey_inv((u32)(pth >> 32)), xmax = __uint_as_float(*xmax_bits);
    const bool safe = live ? fp::f16_dot_masked_margin_safe(gn, gp, dim, qnorm[q], xmax, live[qmask[q]], P)
                           : fp::f16_dot_margin_safe(gn, gp, dim, qnorm[q], xmax, (u32)(pth >> 32) != 0u);
    flags[q] = safe ? 0u : 1u;
    if (!safe) atomicAdd(n_flagged, 1u);
}

// One pass over B queries under W->mu: f16_run / f16m_run (kernels_flat_f16.hip, kernels_flat_f16_masked.hip) with this file's
// kernels.  mp.masked: `mask` with the plan's `used` masks and qmask[B]; else every row.  exact_pass: the flagged queries of an
// exact_mode 1 call again, every chunk unfused with its score matrix from f16d_exact_scores; its rows replace the first answer's.
int32_t f16d_run(cos_index *ix, FlatF16Ws *W, const float *queries, u32 B, u32 top_k, u32 mode, bool exact_pass, const cos_scan_mask *mask, const MaskPlan &mp,
                 u32 *out_ids, float *out_scores, u32 *out_counts, cos_flat_f16_stats *stats) {
    const u32 dim = ix->p.dim, n = ix->n, N = fp::CODE_POOL_FACTOR * top_k;
    const bool exact = exact_pass || mode == fp::F16_EXACT_ALWAYS, by_rule = !exact && mode == fp::F16_EXACT_BY_RULE, masked = mp.masked;
    const fp::Scan plan = fp::f16_scan(n, B, top_k, exact);
    const u32 P = plan.P, R = P / 64, tiles = fp::f16_tiles(n), blocks = fp::f16_query_blocks(B);
    const u64 row_stride = ix->row_stride;
    hipStream_t st = ix->own_stream;
    float *d_q = nullptr, *d_qn = nullptr, *d_qrm = nullptr, *d_scores = nullptr, *d_os = nullptr;
    uint8_t *d_qc = nullptr;
    u32 *d_flags = nullptr, *d_appcnt = nullptr, *d_oi = nullptr, *d_oc = nullptr, *d_qflag = nullptr;
    u64 *d_pool = nullptr, *d_sorted = nullptr, *d_thr = nullptr, *d_app = nullptr, *d_part = nullptr;
    hipError_t e = hipSuccess;
    auto need = [&e](auto &buf, auto *&ptr, size_t count) { // the workspace's buffer grown to `count` elements
        if (e == hipSuccess) { e = buf.grow(count); ptr = buf; }
    };
    need(W->q, d_q, (size_t)B * dim);
    need(W->qm, d_qn, B);
    need(W->qrm, d_qrm, B);
    need(W->qc, d_qc, (size_t)B * row_stride);
    need(W->flags, d_flags, 3); // [unused: no zero-norm error, overflow, queries flagged]
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
    F16MaskDev md{};
    if (e == hipSuccess && masked) e = f16_mask_prepare(ix, W, mask, mp.used, mp.skip_deleted, mp.qmask, B, st, md);
    if (e == hipSuccess) e = hipMemcpyAsync(d_q, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, st);
    // the queries as f16 rows (f16::from_f32, padded with zeros) and |q| of the rerank; then |q^| of the f16 codes over the first norm
    if (e == hipSuccess) e = launch_quantize_rows(ENG_F16, d_q, dim, B, dim, ix->p.range_lo, ix->p.range_hi, d_qc, row_stride, d_qn, d_qrm, st);
    if (e == hipSuccess && by_rule) {
        hipLaunchKernelGGL(f16d_code_norms<true>, dim3((B + 3) / 4), dim3(256), 0, st, (const uint8_t *)d_qc, row_stride, B, dim, d_qn);
        e = hipGetLastError();
        if (e == hipSuccess) e = f16d_xmax_ensure(ix, W, st); // of ALL rows: a valid, looser bound for a masked call
    }
    const ScanMask sm = masked ? md.sm : ScanMask{nullptr, nullptr, 0u};
    u32 hflags[3] = {0u, 0u, 0u};
    std::vector<u32> h_len(masked ? blocks : 0u, 0u);
    size_t n_ev = 0;
    u32 launches = 0;
    for (int attempt = 0; attempt < 2 && e == hipSuccess; attempt++) {
        // the score matrix and the selection's lists: as wide as this attempt's first chunk, its widest unfused one
        const u64 s_stride = fp::score_stride(plan.first(attempt));
        need(W->scores, d_scores, (size_t)B * s_stride);
        need(W->part, d_part, (size_t)B * fp::select_segments(B, plan.first(attempt)) * P);
        if (e == hipSuccess) e = launch_flat_reset(d_pool, (u64)B * P, d_thr, d_appcnt, B, d_flags + 1, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_flags + 2, 0, 4, st);
        if (e != hipSuccess) break;
        const ScanBufs bufs{d_scores, s_stride, d_part, d_pool, d_thr, d_app, d_appcnt, d_flags + 1, sm};
        const DotScanArgs args{d_qc, B, ix->d_codes, row_stride, dim, d_scores, s_stride, bufs.fused_out(plan, nullptr), DotTiles{md.lists, md.list_len, tiles}};
        // a chunk's scoring kernel stands between a (start, stop) pair of events, read after the last chunk
        e = run_chunks(plan, attempt, bufs, st, [&](const fp::Chunk &c) {
            hipEvent_t ev0 = nullptr, ev1 = nullptr;
            hipError_t ce = W->event(n_ev, &ev0);
            if (ce == hipSuccess) ce = W->event(n_ev + 1, &ev1);
            if (ce == hipSuccess) { n_ev += 2; ce = hipEventRecord(ev0, st); }
            if (ce != hipSuccess) return ce;
            if (exact) {
                if (masked && c.n0 % F_ROWS) return hipErrorInvalidValue;
                const dim3 grid(B, (c.nc + F16D_EXACT_ROWS - 1) / F16D_EXACT_ROWS);
                const auto kernel = masked ? f16d_exact_scores<true> : f16d_exact_scores<false>;
                hipLaunchKernelGGL(kernel, grid, dim3(256), staged_query_bytes(dim), st, (const uint8_t *)d_qc,
                                   row_stride, (const uint8_t *)ix->d_codes.p, c.n0, c.nc, dim, d_scores, s_stride, sm, md.tile_bits, md.tb_stride, tiles);
                ce = hipGetLastError();
            } else
                ce = launch_f16_dot_scan(c.fused, masked, ix->n_cus, st, args, c.n0, c.nc);
            if (ce != hipSuccess) return ce;
            launches++;
            return hipEventRecord(ev1, st);
        });
        if (e == hipSuccess && by_rule) { // the pools are final (or about to be repeated): ranks N and P of each
            hipLaunchKernelGGL(f16d_margin_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const u64 *)d_pool, P, B, N, dim, (const float *)d_qn,
                               (const u32 *)W->xmax.p, masked ? md.sm.qmask : (const u32 *)nullptr, masked ? md.live : (const u32 *)nullptr, d_qflag, d_flags + 2);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = launch_f16d_rescore(P, d_qc, row_stride, B, ix->d_codes, dim, d_pool, d_sorted, st);
        if (e == hipSuccess) e = launch_flat_rerank(R, d_q, d_qrm, B, ix->d_raw, ix->d_raw_mags, dim, d_sorted, N, top_k, ix->p.id_base, d_oi, d_os, d_oc, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_ids, d_oi, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_scores, d_os, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_counts, d_oc, (size_t)B * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hflags, d_flags, 12, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && masked) e = hipMemcpyAsync(h_len.data(), md.list_len, (size_t)blocks * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        if (!(plan.fused(attempt) && hflags[1] != 0)) break; // done; otherwise the append buffer overflowed: repeat unfused
    }
    std::vector<u32> h_flag;
    const u32 n_flagged = by_rule ? hflags[2] : 0u;
    if (e == hipSuccess && n_flagged) {
        h_flag.resize(B);
        e = hipMemcpyAsync(h_flag.data(), d_qflag, (size_t)B * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    float gemm_ms = 0.f;
    for (size_t i = 0; i + 1 < n_ev && e == hipSuccess; i += 2) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, W->evs[i], W->evs[i + 1]);
        gemm_ms += ms;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st); // the caller's arrays and the workspace's host arrays are free again
    HIP_TRY(e);
    if (stats && !exact_pass) {
        stats->queries = B;
        stats->exact_queries = exact ? B : n_flagged;
        stats->pool = P;
        stats->gemm_ms = gemm_ms;
        stats->gemm_launches = launches;
        if (stats->struct_size == sizeof(cos_flat_f16_stats)) { // a masked call: its blocks' live tiles; else every tile for every block
            stats->tiles_total = stats->tiles_scanned = blocks * tiles;
            if (masked) {
                stats->tiles_scanned = 0;
                for (u32 len : h_len) stats->tiles_scanned += len;
            }
        }
    }
    if (n_flagged == 0) return COS_OK;
    // the flagged queries again, exactly, each with its mask: the sub-batch's answer replaces theirs
    std::vector<u32> sel;
    MaskPlan xmp = mp;
    xmp.qmask.clear();
    for (u32 b = 0; b < B; b++)
        if (h_flag[b]) {
            sel.push_back(b);
            if (masked) xmp.qmask.push_back(mp.qmask[b]);
        }
    const u32 Bx = (u32)sel.size();
    std::vector<float> xq((size_t)Bx * dim), xs((size_t)Bx * top_k);
    std::vector<u32> xi((size_t)Bx * top_k), xc(Bx);
    for (u32 i = 0; i < Bx; i++) memcpy(xq.data() + (size_t)i * dim, queries + (size_t)sel[i] * dim, (size_t)dim * 4);
    if (int32_t xrc = f16d_run(ix, W, xq.data(), Bx, top_k, mode, true, mask, xmp, xi.data(), xs.data(), xc.data(), nullptr)) return xrc;
    for (u32 i = 0; i < Bx; i++) {
        memcpy(out_ids + (size_t)sel[i] * top_k, xi.data() + (size_t)i * top_k, (size_t)top_k * 4);
        memcpy(out_scores + (size_t)sel[i] * top_k, xs.data() + (size_t)i * top_k, (size_t)top_k * 4);
        out_counts[sel[i]] = xc[i];
    }
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_flat_search_f16_dot_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, const cos_scan_mask *mask,
                                                 const cos_flat_f16_opts *opts, uint32_t *out_ids, float *out_scores, uint32_t *out_counts,
                                                 cos_flat_f16_stats *stats) {
    if (!ix || !queries || !out_ids || !out_scores || !out_counts || B == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    if (opts && opts->struct_size != sizeof(cos_flat_f16_opts)) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::struct_size is %u, expected %zu", opts->struct_size, sizeof(cos_flat_f16_opts));
    if (stats && stats->struct_size != sizeof(cos_flat_f16_stats) && stats->struct_size != COS_FLAT_F16_STATS_SIZE_V1)
        return cos_fail(COS_ERR_INVALID, "cos_flat_f16_stats::struct_size is %u, expected %zu (or %u)", stats->struct_size, sizeof(cos_flat_f16_stats), COS_FLAT_F16_STATS_SIZE_V1);
    const u32 mode = opts ? opts->exact_mode : (u32)fp::F16_EXACT_BY_RULE;
    if (mode > fp::F16_EXACT_ALWAYS) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::exact_mode is %u: 0, 1 or 2", mode);
    if (ix->eng != ENG_F16) return cos_fail(COS_ERR_STORAGE_MISMATCH, "cos_flat_search_f16_dot_batch scans HalfPrecisionFP rows (cos_bruteforce_topk_dot: the raw f32 rows of any index)");
    if (ix->p.metric != COS_METRIC_DOT)
        return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_flat_search_f16_dot_batch implements the dot-product metric (cosine: cos_flat_search_f16_batch, cos_flat_search_f16_masked_batch)");
    if (int32_t krc = fp::check_f16_top_k(top_k)) return cos_fail(krc, "the f16 scan keeps at most 1024 survivors (2 * 5 * top_k): top_k must be in [1, 102]");
    MaskPlan mp;
    if (int32_t mrc = scan_mask_plan(mask, B, mp)) return mrc;
    if (int32_t rc = cos_set_device(ix)) return rc;
    FlatF16Ws *W = cos_flat_f16_ws(ix);
    std::lock_guard<std::mutex> wg(W->mu);
    return f16d_run(ix, W, queries, B, top_k, mode, false, mask, mp, out_ids, out_scores, out_counts, stats);
}
