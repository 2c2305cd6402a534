// kernels_flat_f16_masked.hip — cos_flat_search_f16_masked_batch: cos_flat_search_f16_batch's answer over each query's LIVE rows (its
// allow-list AND NOT the handle's deleted set), with the original ids.  The stages are kernels_flat_f16.hip's — MFMA scan -> margin
// rule -> reference-order re-score -> exact rerank, the exact path for flagged queries — but the scan does not visit what is dead:
//   f16m_prepare           once per call, from the uploaded mask words and the deleted bitmap: the effective words eff[g][w], their OR
//                          (the zero-norm screen's rows), live rows and one bit per 64-row tile for every mask, and for every block of
//                          128 queries the ascending list of the tiles that hold a row live for one of its queries (ballot + wave
//                          prefix sum; nothing goes through the host)
//   flat_scan_f16_masked   flat_scan_f16's data movement — double-buffered LDS panels, AccVGPR-resident query fragments, the x8 tail —
//                          over the block's tile LIST: a dead tile costs no load, no panel and no MFMA.  The two mask words of the
//                          tile's 64 rows are staged per query of the block in LDS (one load per thread, issued with the tile's first
//                          panel; three buffers, because the epilogue reads them after the barrier that frees the panel), and the
//                          fused epilogue tests the row's bit there before it forms the exact quotient and appends
//   the unfused chunks     (the seed, or every chunk after an append overflow) write the live tiles' scores only; the selection
//                          (flat_scan.h ScanMask) reads a score only where the query's bit is set, so a threshold is one of live rows
//                          and a query with fewer than P of them keeps "no threshold yet"
//   f16m_exact_scores      the exact path, live rows only: a range without a live tile ends at once, a wave skips a dead tile through
//                          the per-mask tile bits, a lane a dead row through its bit
//   f16m_margin_kernel     flat_plan.h f16_masked_margin_safe: no test for a query with at most P live rows
// Pools hold live rows only, so f16_rescore and the rerank run unchanged and the counts are min(top_k, live rows).
// An append overflow repeats the call unfused, as there; a mask whose live rows all lie behind the seed chunk (no threshold when the
// first fused chunk meets them) takes that road when a query has more live rows in one chunk than the append buffer holds.
// Out of scope: the shard set, FullPrecisionFP storage, top_k > 102 and masks that are already on the device.  The dot-product metric
// is kernels_flat_f16_dot.hip's, which shares this file's prepare step (f16_mask_prepare).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
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
constexpr size_t F16M_MASK_LDS = (size_t)3 * QB * 2 * 4;     // [3][128 queries][2 words]
constexpr size_t F16M_SCAN_LDS = F16_SCAN_LDS + F16M_MASK_LDS; // 70 656 B: two workgroups per CU, as unmasked
static_assert(QB * 2 == 256, "one mask word per thread and tile");

// ---- prepare: effective words, tile bits, tile lists ----
// word w of the rows that may be returned at all: not deleted, inside n
__device__ __forceinline__ u32 keep_rows(const u32 *__restrict__ deleted, u32 w, u32 words, u32 n) {
    if (w >= words) return 0u;
    u32 keep = deleted ? ~deleted[w] : ~0u;
    if (w == words - 1 && (n & 31u)) keep &= (1u << (n & 31u)) - 1u;
    return keep;
}
// Grid: `blocks` list builders, then ceil(tiles / 256) word workgroups; 256 threads, thread = tile.  Both read the uploaded words, so
// neither waits for the other.  live[] is zero on entry.
__global__ __launch_bounds__(256) void f16m_prepare(const u32 *__restrict__ user /*[G][words] or null: all ones*/, const u32 *__restrict__ deleted /*or null*/,
                                                    u32 G, u32 words, u32 n, u32 tiles, u32 blocks, const u32 *__restrict__ blk_off,
                                                    const u32 *__restrict__ blk_masks, u32 *__restrict__ eff, u32 *__restrict__ uni,
                                                    u32 *__restrict__ live, u64 *__restrict__ tile_bits, u32 tb_stride, u32 *__restrict__ lists,
                                                    u32 *__restrict__ list_len) {
    __shared__ u32 wave_cnt[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (blockIdx.x < blocks) { // the live tiles of query block b, compacted in order
        const u32 b = blockIdx.x, m0 = blk_off[b], m1 = blk_off[b + 1];
        u32 base = 0;
        for (u32 t0 = 0; t0 < tiles; t0 += 256) {
            const u32 t = t0 + tid;
            const u32 k0 = keep_rows(deleted, 2 * t, words, n), k1 = keep_rows(deleted, 2 * t + 1, words, n);
            u32 any = 0;
            if (k0 | k1)
                for (u32 i = m0; i < m1; i++) {
                    const u32 *ug = user ? user + (u64)blk_masks[i] * words : nullptr;
                    any |= (k0 ? (ug ? ug[2 * t] : ~0u) & k0 : 0u) | (k1 ? (ug ? ug[2 * t + 1] : ~0u) & k1 : 0u);
                }
            const u64 bal = __ballot(any != 0u);
            if (lane == 0) wave_cnt[w] = (u32)__popcll(bal);
            __syncthreads();
            u32 before = 0, total = 0;
#pragma unroll
            for (u32 i = 0; i < 4; i++) {
                before += i < w ? wave_cnt[i] : 0u;
                total += wave_cnt[i];
            }
            if (any) lists[(u64)b * tiles + base + before + (u32)__popcll(bal & ((1ull << lane) - 1ull))] = t;
            base += total;
            __syncthreads();
        }
        if (tid == 0) list_len[b] = base;
        return;
    }
    const u32 t = (blockIdx.x - blocks) * 256 + tid; // a wave's 64 tiles are one word of tile bits
    const u32 k0 = keep_rows(deleted, 2 * t, words, n), k1 = keep_rows(deleted, 2 * t + 1, words, n);
    u32 u0 = 0, u1 = 0;
    for (u32 g = 0; g < G; g++) {
        const u32 *ug = user ? user + (u64)g * words : nullptr;
        const u32 e0 = k0 ? (ug ? ug[2 * t] : ~0u) & k0 : 0u, e1 = k1 ? (ug ? ug[2 * t + 1] : ~0u) & k1 : 0u;
        if (2 * t < words) eff[(u64)g * words + 2 * t] = e0;
        if (2 * t + 1 < words) eff[(u64)g * words + 2 * t + 1] = e1;
        u0 |= e0;
        u1 |= e1;
        const u64 bal = __ballot((e0 | e1) != 0u);
        u32 c = (u32)__popc(e0) + (u32)__popc(e1);
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) c += (u32)__shfl_xor((int)c, m, 64);
        if (lane == 0 && t < tiles) {
            tile_bits[(u64)g * tb_stride + (t >> 6)] = bal;
            if (c) atomicAdd(&live[g], c);
        }
    }
    if (2 * t < words) uni[2 * t] = u0;
    if (2 * t + 1 < words) uni[2 * t + 1] = u1;
}

// *flag |= 1 when a row of the bitmap has a zero norm: the rows that are live for at least one query of the call
__global__ void f16m_zero_rows(const float *__restrict__ v, u32 n, const u32 *__restrict__ rows, u32 *__restrict__ flag) {
    bool z = false;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        z |= ((rows[i >> 5] >> (i & 31u)) & 1u) != 0u && v[i] == 0.0f;
    if (__any(z) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// the live tiles of one query block: list[0 .. len) ascending tile numbers (row / 64)
struct TileLists {
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

// flat_scan_f16 (kernels_flat_f16.hip) over the live tiles of rows [n0, n0 + n_chunk), n0 a multiple of 64 (every chunk start of
// flat_plan.h is).  Grid (workgroups that stride over the block's list, ceil(B / 128)); a workgroup past the list's end leaves.
//   FUSED   the epilogue keeps a survivor only where bit `row` of its query's effective mask is set (fo.m), read from LDS
//   !FUSED  scores[q][col] = acc / (|q| * |x|) for the columns of live tiles; the rest of the matrix is not written and not read
template <int NPAN /* as flat_scan_f16 */, bool FUSED>
__global__ __launch_bounds__(256) void flat_scan_f16_masked(const uint8_t *__restrict__ qh, const float *__restrict__ qmags, u32 B, const uint8_t *__restrict__ codes,
                                                            const float *__restrict__ mags, u64 row_stride, u32 n0, u32 n_chunk, u32 dim,
                                                            float *__restrict__ scores, u64 s_stride, const FusedOut fo, const TileLists tl) {
    constexpr bool RES = NPAN > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char f16_lds[]; // [2][F_ROWS][F_LDP] panels, [3][128][2] mask words
    u32 *mask_lds = (u32 *)(f16_lds + F16_SCAN_LDS);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const u32 row0 = blockIdx.y * QB + (u32)w * 32;
    const u32 *__restrict__ list = tl.lists + (u64)blockIdx.y * tl.stride;
    const u32 len = tl.list_len[blockIdx.y], t_base = n0 / F_ROWS, G = gridDim.x;
    const u32 li_end = first_tile_at(list, len, (n0 + n_chunk + F_ROWS - 1) / F_ROWS);
    u32 li = first_tile_at(list, len, t_base) + blockIdx.x;
    if (li >= li_end) return; // uniform
    const bool tail8 = (dim & 15u) != 0u && (dim & 15u) <= 8u;
    const u32 steps16 = tail8 ? dim / 16 : (dim + 15) / 16, kt = dim / 16 * 16;
    const u32 npan = RES ? (u32)NPAN : (dim + F_PAN - 1) / F_PAN;
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
    float T[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const u32 row = row0 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half), rc = row < B ? row : B - 1;
        const float qm = qmags[rc];
        if constexpr (FUSED) {
            const u64 k = fo.thr[rc];
            const float tsc = simkey_inv((u32)(k >> 32));
            const float lo = k == 0ull ? -__builtin_inff() : tsc - 4e-6f * __builtin_fabsf(tsc); // 0 = no threshold yet: every live row passes
            T[r] = row < B ? lo * qm : __builtin_inff();
        } else
            T[r] = qm;
    }
    // this thread's share of a tile's mask words: word (tid & 1) of the tile for query (tid >> 1) of the block; 0 past B and past the mask
    const u32 mq = blockIdx.y * QB + ((u32)tid >> 1);
    const u32 *mrow = FUSED && mq < B ? fo.m.bits + (u64)fo.m.qmask[mq] * fo.m.words : nullptr;
    auto load_mask = [&](u32 gtile) __attribute__((always_inline)) {
        const u32 wi = 2 * gtile + ((u32)tid & 1u);
        return mrow && wi < fo.m.words ? mrow[wi] : 0u;
    };
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
    u32 gt = list[li]; // the tile of the corpus; the chunk's tile is gt - t_base
    load_panel(gt - t_base, 0);
    store_panel(0);
    if constexpr (FUSED) mask_lds[tid] = load_mask(gt);
    __syncthreads();
    int buf = 0;
    u32 mbuf = 0, mw_next = 0;
    for (;; li += G) {
        const bool more_tiles = li + G < li_end; // uniform
        const u32 gt_next = more_tiles ? list[li + G] : gt;
        const u32 t = gt - t_base;
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
            if (more) {
                load_panel(last_p ? gt_next - t_base : t, last_p ? 0u : p + 1); // in flight while this panel is multiplied
                if constexpr (FUSED)
                    if (last_p) mw_next = load_mask(gt_next);
            }
            const unsigned char *brow = f16_lds + (size_t)buf * F_ROWS * F_LDP + (size_t)l31 * F_LDP;
            const u32 ns = steps16 > 16 * p ? steps16 - 16 * p : 0u;
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
                if constexpr (FUSED)
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
        // epilogue: C/D layout of a 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32 col = t * F_ROWS + 32 * (u32)j + (u32)l31; // row n0 + col of the corpus: bit l31 of the tile's word j
            const bool cv = col < n_chunk;
            const float xm = xmj[j];
            if constexpr (FUSED) {
                const float rx = __builtin_amdgcn_rcpf(xm);
                bool any = false;
#pragma unroll
                for (int r = 0; r < 16; r++) any |= !(acc[j][r] * rx < T[r]);
                if (any && cv) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const u32 rl = (u32)w * 32 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half), row = blockIdx.y * QB + rl;
                        if (row < B && !(acc[j][r] * rx < T[r]) && ((mask_lds[mbuf * 256 + rl * 2 + (u32)j] >> l31) & 1u) != 0u) {
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
        gt = gt_next;
        mbuf = (mbuf + 1) % 3;
    }
}

struct ScanArgs { // what every chunk's launch repeats
    const uint8_t *qh;
    const float *qmags;
    u32 B;
    const uint8_t *codes;
    const float *mags;
    u64 row_stride;
    u32 dim;
    float *scores;
    u64 s_stride;
    FusedOut fo;
    TileLists tl;
};
template <int NPAN>
hipError_t launch_scan_npan(bool fused, dim3 grid, hipStream_t st, const ScanArgs &a, u32 n0, u32 nc) {
    const auto kernel = fused ? flat_scan_f16_masked<NPAN, true> : flat_scan_f16_masked<NPAN, false>;
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)F16M_SCAN_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), F16M_SCAN_LDS, st, a.qh, a.qmags, a.B, a.codes, a.mags, a.row_stride, n0, nc, a.dim, a.scores, a.s_stride, a.fo, a.tl);
    return hipGetLastError();
}
// rows [n0, n0 + nc): as many workgroups as the chunk has tiles, at most one per CU — how many of them find work is the list's business
hipError_t launch_f16_scan_masked(bool fused, u32 n_cus, hipStream_t st, const ScanArgs &a, u32 n0, u32 nc) {
    if (n0 % F_ROWS) return hipErrorInvalidValue; // a tile of the lists is a tile of the chunk
    const dim3 grid(std::min((nc + F_ROWS - 1) / F_ROWS, n_cus), (a.B + QB - 1) / QB);
    const u32 npan = (a.dim + F_PAN - 1) / F_PAN;
    switch (npan <= (u32)F_MAX_NPAN ? npan : 0u) {
    case 1: return launch_scan_npan<1>(fused, grid, st, a, n0, nc);
    case 2: return launch_scan_npan<2>(fused, grid, st, a, n0, nc);
    case 3: return launch_scan_npan<3>(fused, grid, st, a, n0, nc);
    case 4: return launch_scan_npan<4>(fused, grid, st, a, n0, nc);
    default: return launch_scan_npan<0>(fused, grid, st, a, n0, nc);
    }
}

// f16_margin_kernel over pools of live rows: a query with at most P of them is not tested (its count decides, flat_plan.h)
__global__ void f16m_margin_kernel(const u64 *__restrict__ pool_mem, u32 P, u32 B, u32 N, u32 dim, const u32 *__restrict__ qmask, const u32 *__restrict__ live,
                                   u32 *__restrict__ flags, u32 *__restrict__ n_flagged) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    const u64 nth = pool_mem[(u64)q * P + N - 1], pth = pool_mem[(u64)q * P + P - 1];
    const bool safe = fp::f16_masked_margin_safe(simkey_inv((u32)(nth >> 32)), simkey_inv((u32)(pth >> 32)), dim, live[qmask[q]], P);
    flags[q] = safe ? 0u : 1u;
    if (!safe) atomicAdd(n_flagged, 1u);
}

// f16_exact_scores over the query's live rows: scores[q][c] is written where row n0 + c is live, n0 a multiple of 64.  One workgroup per
// (query, range of F16M_EXACT_ROWS rows), one wave per tile, one lane per row.
constexpr u32 F16M_EXACT_ROWS = 1024;
__global__ __launch_bounds__(256) void f16m_exact_scores(const uint8_t *__restrict__ qh, u64 row_stride, const float *__restrict__ qmags,
                                                         const uint8_t *__restrict__ codes, const float *__restrict__ mags, u32 n0, u32 n_chunk, u32 dim,
                                                         float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride, const ScanMask m,
                                                         const u64 *__restrict__ tile_bits, u32 tb_stride, u32 tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const u32 q = blockIdx.x, g = m.qmask[q];
    const u64 *tb = tile_bits + (u64)g * tb_stride;
    const u32 c_begin = blockIdx.y * F16M_EXACT_ROWS, c_end = c_begin + F16M_EXACT_ROWS < n_chunk ? c_begin + F16M_EXACT_ROWS : n_chunk;
    const u32 t_first = (n0 + c_begin) / F_ROWS;
    auto tile_live = [&](u32 t) { return t < tiles && ((tb[t >> 6] >> (t & 63u)) & 1ull) != 0ull; };
    bool any = false;
    for (u32 i = 0; i < F16M_EXACT_ROWS / F_ROWS; i++) any |= tile_live(t_first + i);
    if (!any) return; // uniform: nothing of this query lives in the range
    stage_f16_query(qf, qh + (u64)q * row_stride, dim);
    const float mq = qmags[q];
    for (u32 c0 = c_begin; c0 < c_end; c0 += 256) {
        const u32 c = c0 + threadIdx.x, row = n0 + c;
        if (!tile_live((n0 + c0) / F_ROWS + (threadIdx.x >> 6))) continue; // the wave's tile
        if (c < c_end && scan_live<true>(m, q, row)) {
            const float dp = f16_lane_dot(codes + (u64)row * row_stride, qf, dim);
            scores[(u64)q * s_stride + c] = x86_div(dp, __fmul_rn(mq, mags[row]));
        }
    }
}

} // namespace

// The masks of a call on the device, for both masked f16 scans (this file's, kernels_flat_f16_dot.hip's): the masks of each query block
// (host), the uploads and f16m_prepare, enqueued on st.  The host arrays that the uploads read live in the workspace until the next call.
hipError_t f16_mask_prepare(cos_index *ix, FlatF16Ws *W, const cos_scan_mask *mask, const std::vector<u32> &used, bool skip_deleted,
                            const std::vector<u32> &qmask, u32 B, hipStream_t st, cosdev::F16MaskDev &out) {
    const u32 n = ix->n, words = (n + 31) / 32, G = used.empty() ? 1u : (u32)used.size(), tiles = fp::f16_tiles(n), blocks = fp::f16_query_blocks(B);
    const u32 tb_stride = (tiles + 63) / 64;
    FlatF16MaskBufs &M = W->mask;
    std::vector<u32> &blk_off = M.h_blk_off, &blk_masks = M.h_blk_masks;
    blk_off.assign(blocks + 1, 0u);
    blk_masks.clear();
    for (u32 b = 0; b < blocks; b++) {
        std::vector<u32> ms(qmask.begin() + (size_t)b * QB, qmask.begin() + std::min<size_t>((size_t)(b + 1) * QB, B));
        std::sort(ms.begin(), ms.end());
        ms.erase(std::unique(ms.begin(), ms.end()), ms.end());
        blk_masks.insert(blk_masks.end(), ms.begin(), ms.end());
        blk_off[b + 1] = (u32)blk_masks.size();
    }
    u32 *d_user = nullptr, *d_qmask = nullptr, *d_blk_off = nullptr, *d_blk_masks = nullptr, *d_eff = nullptr, *d_uni = nullptr, *d_live = nullptr,
        *d_lists = nullptr, *d_list_len = nullptr;
    u64 *d_tile_bits = nullptr;
    hipError_t e = hipSuccess;
    auto need = [&e](auto &buf, auto *&ptr, size_t count) {
        if (e == hipSuccess) { e = buf.grow(count); ptr = buf; }
    };
    if (!used.empty()) need(M.user, d_user, (size_t)G * words);
    need(M.qmask, d_qmask, B);
    need(M.blk_off, d_blk_off, blocks + 1);
    need(M.blk_masks, d_blk_masks, blk_masks.size());
    need(M.eff, d_eff, (size_t)G * words);
    need(M.uni, d_uni, words);
    need(M.live, d_live, G);
    need(M.tile_bits, d_tile_bits, (size_t)G * tb_stride);
    need(M.lists, d_lists, (size_t)(fp::f16_tile_list_bytes(n, B) / 4) - blocks);
    need(M.list_len, d_list_len, blocks);
    if (e == hipSuccess) e = hipMemsetAsync(d_live, 0, (size_t)G * 4, st);
    for (u32 g = 0; g < (u32)used.size() && e == hipSuccess; g++)
        e = hipMemcpyAsync(d_user + (size_t)g * words, mask->bits + (size_t)used[g] * words, (size_t)words * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_qmask, qmask.data(), (size_t)B * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk_off, blk_off.data(), (size_t)(blocks + 1) * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk_masks, blk_masks.data(), blk_masks.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(f16m_prepare, dim3(blocks + (tiles + 255) / 256), dim3(256), 0, st, (const u32 *)d_user,
                           skip_deleted ? (const u32 *)ix->d_deleted.p : (const u32 *)nullptr, G, words, n, tiles, blocks, (const u32 *)d_blk_off,
                           (const u32 *)d_blk_masks, d_eff, d_uni, d_live, d_tile_bits, tb_stride, d_lists, d_list_len);
        e = hipGetLastError();
    }
    out = cosdev::F16MaskDev{ScanMask{d_eff, d_qmask, words}, d_uni, d_live, d_tile_bits, tb_stride, d_lists, d_list_len, tiles, blocks};
    return e;
}

namespace {

// One pass over B queries under W->mu, f16_run's (kernels_flat_f16.hip) with the masks: `used` = the caller's masks in use (empty: one
// all-ones mask), qmask[B] -> index into them.  exact_pass: the flagged queries of an exact_mode 1 call again.
int32_t f16m_run(cos_index *ix, FlatF16Ws *W, const float *queries, u32 B, u32 top_k, u32 mode, bool exact_pass, const cos_scan_mask *mask,
                 const std::vector<u32> &used, bool skip_deleted, const std::vector<u32> &qmask, u32 *out_ids, float *out_scores, u32 *out_counts,
                 cos_flat_f16_stats *stats) {
    const u32 dim = ix->p.dim, n = ix->n, N = fp::CODE_POOL_FACTOR * top_k;
    const bool exact = exact_pass || mode == fp::F16_EXACT_ALWAYS, by_rule = !exact && mode == fp::F16_EXACT_BY_RULE;
    const fp::Scan plan = fp::f16_scan(n, B, top_k, exact);
    const u32 P = plan.P, R = P / 64;
    const u32 tiles = fp::f16_tiles(n), blocks = fp::f16_query_blocks(B), tb_stride = (tiles + 63) / 64;
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
    F16MaskDev md{};
    if (e == hipSuccess) e = f16_mask_prepare(ix, W, mask, used, skip_deleted, qmask, B, st, md);
    const u32 *d_uni = md.uni, *d_live = md.live, *d_lists = md.lists, *d_list_len = md.list_len, *d_qmask = md.sm.qmask;
    const u64 *d_tile_bits = md.tile_bits;
    if (e == hipSuccess) e = hipMemcpyAsync(d_q, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_quantize_rows(ENG_F16, d_q, dim, B, dim, ix->p.range_lo, ix->p.range_hi, d_qc, row_stride, d_qm, d_qrm, st);
    // zero norms, the masked code scan's rule: the rows that are live for at least one query of the call, and the queries; every call
    if (e == hipSuccess && !exact_pass) {
        hipLaunchKernelGGL(f16m_zero_rows, dim3(1024), dim3(256), 0, st, (const float *)ix->d_mags.p, n, (const u32 *)d_uni, d_flags);
        e = hipGetLastError();
        if (e == hipSuccess) e = launch_any_zero(d_qm, B, d_flags, st);
    }
    const ScanMask sm = md.sm;
    u32 hflags[3] = {0u, 0u, 0u};
    std::vector<u32> h_len(blocks, 0u);
    bool zero = false;
    size_t n_ev = 0;
    u32 launches = 0;
    for (int attempt = 0; attempt < 2 && e == hipSuccess; attempt++) {
        const u64 s_stride = fp::score_stride(plan.first(attempt));
        need(W->scores, d_scores, (size_t)B * s_stride);
        need(W->part, d_part, (size_t)B * fp::select_segments(B, plan.first(attempt)) * P);
        if (e == hipSuccess) e = launch_flat_reset(d_pool, (u64)B * P, d_thr, d_appcnt, B, d_flags + 1, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_flags + 2, 0, 4, st);
        if (e != hipSuccess) break;
        const ScanBufs bufs{d_scores, s_stride, d_part, d_pool, d_thr, d_app, d_appcnt, d_flags + 1, sm};
        const ScanArgs args{d_qc, d_qm, B, ix->d_codes, ix->d_mags, row_stride, dim, d_scores, s_stride, bufs.fused_out(plan, nullptr),
                            TileLists{d_lists, d_list_len, tiles}};
        e = run_chunks(plan, attempt, bufs, st, [&](const fp::Chunk &c) {
            hipEvent_t ev0 = nullptr, ev1 = nullptr;
            hipError_t ce = W->event(n_ev, &ev0);
            if (ce == hipSuccess) ce = W->event(n_ev + 1, &ev1);
            if (ce == hipSuccess) { n_ev += 2; ce = hipEventRecord(ev0, st); }
            if (ce != hipSuccess) return ce;
            if (exact) {
                if (c.n0 % F_ROWS) return hipErrorInvalidValue;
                hipLaunchKernelGGL(f16m_exact_scores, dim3(B, (c.nc + F16M_EXACT_ROWS - 1) / F16M_EXACT_ROWS), dim3(256), staged_query_bytes(dim), st,
                                   (const uint8_t *)d_qc, row_stride, (const float *)d_qm, (const uint8_t *)ix->d_codes.p, (const float *)ix->d_mags.p, c.n0, c.nc,
                                   dim, d_scores, s_stride, sm, (const u64 *)d_tile_bits, tb_stride, tiles);
                ce = hipGetLastError();
            } else
                ce = launch_f16_scan_masked(c.fused, ix->n_cus, st, args, c.n0, c.nc);
            if (ce != hipSuccess) return ce;
            launches++;
            return hipEventRecord(ev1, st);
        });
        if (e == hipSuccess && by_rule) {
            hipLaunchKernelGGL(f16m_margin_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const u64 *)d_pool, P, B, N, dim, (const u32 *)d_qmask,
                               (const u32 *)d_live, d_qflag, d_flags + 2);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = launch_f16_rescore(P, d_qc, row_stride, d_qm, B, ix->d_codes, ix->d_mags, dim, d_pool, d_sorted, st);
        if (e == hipSuccess) e = launch_flat_rerank(R, d_q, d_qrm, B, ix->d_raw, ix->d_raw_mags, dim, d_sorted, N, top_k, ix->p.id_base, d_oi, d_os, d_oc, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_ids, d_oi, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_scores, d_os, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_counts, d_oc, (size_t)B * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hflags, d_flags, 12, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_len.data(), d_list_len, (size_t)blocks * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        zero = hflags[0] != 0;
        if (zero || !(plan.fused(attempt) && hflags[1] != 0)) break; // done; otherwise the append buffer overflowed: repeat unfused
    }
    std::vector<u32> h_flag;
    const u32 n_flagged = by_rule && !zero ? hflags[2] : 0u;
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
    HIP_TRY(e);
    if (zero) return cos_fail(COS_ERR_CALCULATION, "zero-norm query or live stored vector: DistanceError::CalculationError (cosine.rs:228-232)");
    if (stats && !exact_pass) {
        stats->queries = B;
        stats->exact_queries = exact ? B : n_flagged;
        stats->pool = P;
        stats->gemm_ms = gemm_ms;
        stats->gemm_launches = launches;
        if (stats->struct_size == sizeof(cos_flat_f16_stats)) {
            stats->tiles_total = blocks * tiles;
            stats->tiles_scanned = 0;
            for (u32 len : h_len) stats->tiles_scanned += len;
        }
    }
    if (n_flagged == 0) return COS_OK;
    // the flagged queries again, exactly, each with its mask: the sub-batch's answer replaces theirs
    std::vector<u32> sel, xqm;
    for (u32 b = 0; b < B; b++)
        if (h_flag[b]) { sel.push_back(b); xqm.push_back(qmask[b]); }
    const u32 Bx = (u32)sel.size();
    std::vector<float> xq((size_t)Bx * dim), xs((size_t)Bx * top_k);
    std::vector<u32> xi((size_t)Bx * top_k), xc(Bx);
    for (u32 i = 0; i < Bx; i++) memcpy(xq.data() + (size_t)i * dim, queries + (size_t)sel[i] * dim, (size_t)dim * 4);
    if (int32_t xrc = f16m_run(ix, W, xq.data(), Bx, top_k, mode, true, mask, used, skip_deleted, xqm, xi.data(), xs.data(), xc.data(), nullptr)) return xrc;
    for (u32 i = 0; i < Bx; i++) {
        memcpy(out_ids + (size_t)sel[i] * top_k, xi.data() + (size_t)i * top_k, (size_t)top_k * 4);
        memcpy(out_scores + (size_t)sel[i] * top_k, xs.data() + (size_t)i * top_k, (size_t)top_k * 4);
        out_counts[sel[i]] = xc[i];
    }
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_flat_search_f16_masked_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, const cos_scan_mask *mask,
                                                    const cos_flat_f16_opts *opts, uint32_t *out_ids, float *out_scores, uint32_t *out_counts,
                                                    cos_flat_f16_stats *stats) {
    // no mask: the unmasked call, its kernels and its bits
    if (!mask || (mask->struct_size == sizeof(cos_scan_mask) && mask->n_masks == 0 && mask->flags == 0))
        return cos_flat_search_f16_batch(ix, queries, B, top_k, opts, out_ids, out_scores, out_counts, stats);
    if (!ix || !queries || !out_ids || !out_scores || !out_counts || B == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    if (opts && opts->struct_size != sizeof(cos_flat_f16_opts)) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::struct_size is %u, expected %zu", opts->struct_size, sizeof(cos_flat_f16_opts));
    if (stats && stats->struct_size != sizeof(cos_flat_f16_stats) && stats->struct_size != COS_FLAT_F16_STATS_SIZE_V1)
        return cos_fail(COS_ERR_INVALID, "cos_flat_f16_stats::struct_size is %u, expected %zu (or %u)", stats->struct_size, sizeof(cos_flat_f16_stats), COS_FLAT_F16_STATS_SIZE_V1);
    const u32 mode = opts ? opts->exact_mode : (u32)fp::F16_EXACT_BY_RULE;
    if (mode > fp::F16_EXACT_ALWAYS) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::exact_mode is %u: 0, 1 or 2", mode);
    if (ix->eng != ENG_F16) return cos_fail(COS_ERR_STORAGE_MISMATCH, "cos_flat_search_f16_masked_batch scans HalfPrecisionFP rows (cos_flat_search_masked_batch: u8 and bit-plane codes)");
    if (ix->p.metric != COS_METRIC_COSINE) return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_flat_search_f16_masked_batch implements the cosine metric (dot product: cos_flat_search_f16_dot_batch)");
    if (int32_t krc = fp::check_f16_top_k(top_k)) return cos_fail(krc, "the f16 scan keeps at most 1024 survivors (2 * 5 * top_k): top_k must be in [1, 102]");
    MaskPlan mp;
    if (int32_t mrc = scan_mask_plan(mask, B, mp)) return mrc;
    if (int32_t rc = cos_set_device(ix)) return rc;
    FlatF16Ws *W = cos_flat_f16_ws(ix);
    std::lock_guard<std::mutex> wg(W->mu);
    return f16m_run(ix, W, queries, B, top_k, mode, false, mask, mp.used, mp.skip_deleted, mp.qmask, out_ids, out_scores, out_counts, stats);
}
