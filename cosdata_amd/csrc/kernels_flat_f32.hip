// kernels_flat_f32.hip — cos_flat_search_f32_batch: the exhaustive scan of a FullPrecisionFP collection (cosine), masked or not.  The
// answer is cos_flat_search_f16_batch's with the f32 arm of the first-pass score: every live row scored by the reference-order f32 dot
// of the stored f32 codes (dot_product_f32_simd: eight chains, a pairwise tree, an unfused tail — dot_engines.h f32_oct_dot) over
// |q| * |x| of the quantizer's norms, sorted (desc, larger id first), the best N = 5 * top_k reranked exactly, top_k.  The stages are
// the f16 calls' and so are the plan, the chunk driver, the pools and their folds, the selection, the masks' prepare step, the
// workspace and the rerank (flat_plan.h, flat_scan.h, flat_f16.h); what is this file's own is everything that scores:
//   flat_scan_f32      the candidate GEMM on v_mfma_f32_32x32x2_f32.  Four waves, each with 32 queries; a lane's A fragment of a k step
//                      is 16 bytes: the four floats at k = 8 s + 4 (lane >> 5) .. + 3, one per MFMA of the step, and the B fragment is
//                      the same four floats of a stored row — both operands k-contiguous, so the sum is the plain sum over k whatever
//                      the pairing inside an instruction.  The fragments of up to 512 dims stay in AccVGPRs (NPAN panels of 128 dims,
//                      64 registers each: 256 at 512 dims — half the f16 scans' reach, the fragments being twice the bytes); a wider
//                      row re-reads them from L2 step by step (NPAN = 0).  Stored rows stream through the f16 scans' LDS panels —
//                      64 rows x 528 B, double-buffered, the next panel in flight in registers — which hold 128 f32 dims where they
//                      held 256 halves: 64 MFMAs per wave and panel between two barriers.  Rows are padded to 16 bytes; a piece past
//                      dim is never loaded and the piece that holds dim is masked, so the k tail is zero on both sides.  The query
//                      block's norms, thresholds (the bar an estimate must reach, and the key) sit in LDS.  ONE kernel serves both
//                      forms: MASKED walks the block's list of live tiles and tests the row's bit from LDS before a quotient is
//                      formed, !MASKED strides over every tile.
//   f32x_exact_scores  the exact path: every (live) row by f32_oct_dot, eight lanes per row, written where the MFMA would write
//   f32x_rescore       the P pool rows again in the reference's order, sorted: the first N are the rerank's candidates
//   f32x_margin_kernel flat_plan.h f32_margin_safe, or the query takes the exact path
// Out of scope: the shard set, top_k > 102 and masks that are already on the device.
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
constexpr int F32_PAN = F_PAN / 2;   // dims per k panel: the f16 panel's bytes
constexpr int F32_MAX_NPAN = 4;      // resident fragments: up to 512 dims, 256 AccVGPRs
// LDS: [2][F_ROWS][F_LDP] panels | [128] |q| | FUSED: [128] bars, [128] threshold keys | FUSED && MASKED: [3][128][2] mask words
constexpr size_t F32_QM_OFF = F16_SCAN_LDS, F32_BAR_OFF = F32_QM_OFF + QB * 4, F32_KEY_OFF = F32_BAR_OFF + QB * 4, F32_MASK_OFF = F32_KEY_OFF + QB * 8;
constexpr size_t f32_scan_lds(bool fused, bool masked) { return !fused ? F32_BAR_OFF : !masked ? F32_MASK_OFF : F32_MASK_OFF + (size_t)3 * QB * 2 * 4; }
static_assert(2 * f32_scan_lds(true, true) <= 160 * 1024, "two workgroups per CU where the registers allow it");

// the live tiles of a query block: lists[block][0 .. list_len[block]) ascending tile numbers (row / 64)
struct F32Tiles {
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
// the first `keep` floats of a piece survive, the rest become +0.0
__device__ __forceinline__ i32x4 keep_floats(i32x4 v, int keep) {
    v[1] = keep > 1 ? v[1] : 0;
    v[2] = keep > 2 ? v[2] : 0;
    v[3] = keep > 3 ? v[3] : 0;
    return v;
}
// one k step of 8 dims: four MFMAs, float i of both fragments in the i-th
__device__ __forceinline__ void mfma_step(f32x16 &acc, const i32x4 &a, const i32x4 &b) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int ai = a[i], bi = b[i]; // by value: a bit cast of a vector's element reads the vector's first bytes
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__int_as_float(ai), __int_as_float(bi), acc, 0, 0, 0);
    }
}

// scores of rows [n0, n0 + n_chunk) against the B queries' f32 rows.  Grid (workgroups that stride over the tiles, ceil(B / 128)).
//   MASKED  the tiles are those of the block's list inside the chunk (n0 a multiple of 64); a workgroup past the list's end leaves
//   FUSED   the estimate acc / |x| is screened against the query's bar, threshold * |q| (flat_gemm_f32's rule: the exact quotient, the
//           value that is ranked, is formed for estimates within 4e-6 of the threshold or above it), after (MASKED) the row's bit
//   !FUSED  scores[q][col] = acc / (|q| * |x|) for the columns of the tiles visited (a masked selection reads live columns only)
template <int NPAN /* k panels of resident fragments, dim <= 128 NPAN; 0 = any dim, fragments re-read per step */, bool FUSED, bool MASKED>
__global__ __launch_bounds__(256) void flat_scan_f32(const uint8_t *__restrict__ qf /*[B][row_stride] f32 rows*/, const float *__restrict__ qmags, u32 B,
                                                     const uint8_t *__restrict__ codes, const float *__restrict__ mags, u64 row_stride, u32 n0, u32 n_chunk,
                                                     u32 dim, float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride, const FusedOut fo, const F32Tiles tl) {
    constexpr bool RES = NPAN > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char f32_lds[];
    float *qm_lds = (float *)(f32_lds + F32_QM_OFF), *bar_lds = (float *)(f32_lds + F32_BAR_OFF);
    u64 *thr_key = (u64 *)(f32_lds + F32_KEY_OFF);
    u32 *mask_lds = (u32 *)(f32_lds + F32_MASK_OFF);
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
    const u32 steps = (dim + 7) / 8, npan = RES ? (u32)NPAN : (dim + F32_PAN - 1) / F32_PAN;
    // this lane's query row: the A fragment of step s is its 4 floats at k = 8 s + 4 half
    const u32 qrow = row0 + (u32)l31;
    const bool qv = qrow < B;
    const uint8_t *qp = qf + (u64)(qv ? qrow : 0u) * row_stride;
    auto qfrag = [&](u32 s) __attribute__((always_inline)) {
        const u32 k0 = 8 * s + 4 * (u32)half;
        i32x4 v = {0, 0, 0, 0};
        if (qv && k0 < dim) v = keep_floats(*(const i32x4 *)(qp + 4 * (u64)k0), (int)(dim - k0)); // 4 k0 + 16 <= row_stride
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
    // the block's norms and thresholds, once per launch (a fold between two launches moves them).  A key of 0 = no threshold yet: every
    // (live) row passes.  A row past the batch keeps nothing: its key is all ones.
    if (tid < (int)QB) {
        const u32 row = blockIdx.y * QB + (u32)tid, rc = row < B ? row : B - 1;
        const float qm = qmags[rc];
        qm_lds[tid] = qm;
        if constexpr (FUSED) {
            const u64 key = row < B ? fo.thr[row] : ~0ull;
            const float tsc = simkey_inv((u32)(key >> 32));
            const float lo = key == 0ull ? -__builtin_inff() : tsc - 4e-6f * __builtin_fabsf(tsc);
            thr_key[tid] = key;
            bar_lds[tid] = row < B ? lo * qm : __builtin_inff();
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
            const u32 k0 = pan * F32_PAN + pc * 4;
            i32x4 v = {0, 0, 0, 0};
            if (k0 < dim) { // 4 k0 + 16 <= row_stride
                v = *(const i32x4 *)(codes + (u64)(n0 + cc) * row_stride + 4 * (u64)k0);
                if (dim - k0 < 4u) v = keep_floats(v, (int)(dim - k0));
            }
            raw[p] = v;
        }
    };
    auto store_panel = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < F_NP; p++) {
            const u32 g = (u32)p * 256u + (u32)tid, c = g >> 5, pc = g & 31u;
            *(i32x4 *)(f32_lds + (size_t)buf * F_ROWS * F_LDP + (size_t)c * F_LDP + (size_t)pc * 16) = raw[p];
        }
    };
    u32 t = tile_at(pos);
    load_panel(t, 0);
    store_panel(0);
    if constexpr (FUSED && MASKED) mask_lds[tid] = load_mask(t);
    __syncthreads(); // the first panel, the norms and thresholds, the first tile's mask words
    int buf = 0;
    u32 mbuf = 0, mw_next = 0;
    for (;; pos += G) {
        const bool more_tiles = pos + G < pos_end; // uniform
        const u32 t_next = more_tiles ? tile_at(pos + G) : t;
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
            if (more) {
                load_panel(last_p ? t_next : t, last_p ? 0u : p + 1); // in flight while this panel is multiplied
                if constexpr (FUSED && MASKED)
                    if (last_p) mw_next = load_mask(t_next);
            }
            const unsigned char *brow = f32_lds + (size_t)buf * F_ROWS * F_LDP + (size_t)l31 * F_LDP;
            const u32 ns = steps > 16 * p ? steps - 16 * p : 0u; // steps of this panel (16 unless it is the last)
            static_for<0, 16>([&](auto Sc) __attribute__((always_inline)) {
                constexpr int s = decltype(Sc)::value;
                if ((u32)s < ns) { // uniform
                    const i32x4 b0 = *(const i32x4 *)(brow + 32 * s + 16 * half), b1 = *(const i32x4 *)(brow + 32 * F_LDP + 32 * s + 16 * half);
                    i32x4 af;
                    if constexpr (RES) af = a[PI * 16 + s];
                    else af = qfrag(16 * p + (u32)s);
                    mfma_step(acc[0], af, b0);
                    mfma_step(acc[1], af, b1);
                }
            });
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
        // are four consecutive queries of the block: their bars (FUSED) or norms are one 16-byte LDS read, the same address for a half-wave
        float T[16];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 v = *(const float4 *)((FUSED ? bar_lds : qm_lds) + w * 32 + 8 * g + 4 * half);
            T[4 * g] = v.x, T[4 * g + 1] = v.y, T[4 * g + 2] = v.z, T[4 * g + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32 col = t * F_ROWS + 32 * (u32)j + (u32)l31; // row n0 + col of the corpus: bit l31 of the tile's word j
            const bool cv = col < n_chunk;
            const float xm = xmj[j];
            if constexpr (FUSED) {
                const float rx = __builtin_amdgcn_rcpf(xm);
                bool any = false;
                // NaN-safe: an estimate that is not provably below the bar goes on to the exact quotient
#pragma unroll
                for (int r = 0; r < 16; r++) any |= !(acc[j][r] * rx < T[r]);
                if (any && cv) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const u32 rl = (u32)w * 32 + (u32)((r & 3) + 8 * (r >> 2) + 4 * half);
                        bool keep = !(acc[j][r] * rx < T[r]);
                        if constexpr (MASKED) keep = keep && ((mask_lds[mbuf * 256 + rl * 2 + (u32)j] >> l31) & 1u) != 0u;
                        if (keep) {
                            const float sc = x86_div(acc[j][r], qm_lds[rl] * xm);
                            const u64 key = score_key(sc, n0 + col);
                            if (key > thr_key[rl]) { // ~0 past the batch: nothing is kept
                                const u32 row = blockIdx.y * QB + rl;
                                const u32 at = atomicAdd(&fo.app_cnt[row], 1u);
                                if (at < fo.cap) fo.app[(u64)row * fo.cap + at] = key;
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
        t = t_next;
        mbuf = (mbuf + 1) % 3;
    }
}

struct F32ScanArgs { // what every chunk's launch repeats
    const uint8_t *qf;
    const float *qmags;
    u32 B;
    const uint8_t *codes;
    const float *mags;
    u64 row_stride;
    u32 dim;
    float *scores;
    u64 s_stride;
    FusedOut fo;
    F32Tiles tl;
};
template <int NPAN, bool FUSED, bool MASKED>
hipError_t launch_scan_inst(dim3 grid, hipStream_t st, const F32ScanArgs &a, u32 n0, u32 nc) {
    constexpr size_t lds = f32_scan_lds(FUSED, MASKED);
    const auto kernel = flat_scan_f32<NPAN, FUSED, MASKED>;
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a.qf, a.qmags, a.B, a.codes, a.mags, a.row_stride, n0, nc, a.dim, a.scores, a.s_stride, a.fo, a.tl);
    return hipGetLastError();
}
template <int NPAN>
hipError_t launch_scan_npan(bool fused, bool masked, dim3 grid, hipStream_t st, const F32ScanArgs &a, u32 n0, u32 nc) {
    if (masked) return fused ? launch_scan_inst<NPAN, true, true>(grid, st, a, n0, nc) : launch_scan_inst<NPAN, false, true>(grid, st, a, n0, nc);
    return fused ? launch_scan_inst<NPAN, true, false>(grid, st, a, n0, nc) : launch_scan_inst<NPAN, false, false>(grid, st, a, n0, nc);
}
// rows [n0, n0 + nc): as many workgroups as the chunk has tiles, at most one per CU and query block — a masked block's list says how
// many of them find work
hipError_t launch_f32_scan(bool fused, bool masked, u32 n_cus, hipStream_t st, const F32ScanArgs &a, u32 n0, u32 nc) {
    if (masked && n0 % F_ROWS) return hipErrorInvalidValue; // a tile of the lists is a tile of the chunk
    const dim3 grid(std::min((nc + F_ROWS - 1) / F_ROWS, n_cus), (a.B + QB - 1) / QB);
    const u32 npan = (a.dim + F32_PAN - 1) / F32_PAN;
    switch (npan <= (u32)F32_MAX_NPAN ? npan : 0u) {
    case 1: return launch_scan_npan<1>(fused, masked, grid, st, a, n0, nc);
    case 2: return launch_scan_npan<2>(fused, masked, grid, st, a, n0, nc);
    case 3: return launch_scan_npan<3>(fused, masked, grid, st, a, n0, nc);
    case 4: return launch_scan_npan<4>(fused, masked, grid, st, a, n0, nc);
    default: return launch_scan_npan<0>(fused, masked, grid, st, a, n0, nc);
    }
}

// ---- the exact-order kernels: f32_oct_dot, eight lanes per row, then cosine.rs's quotient ----
// the query's f32 row into LDS: what f32_oct_dot multiplies the stored floats with
__device__ __forceinline__ void stage_f32_query(float *q_lds, const uint8_t *__restrict__ qrow, u32 dim) {
    for (u32 i = threadIdx.x; i < dim; i += blockDim.x) q_lds[i] = ((const float *)qrow)[i];
    __syncthreads();
}
// scores[q][c] = the reference-order score of row n0 + c, the value f32x_rescore ranks, so the selection over this matrix keeps the exact
// top P.  One workgroup per (query, range of F32X_EXACT_ROWS rows), 32 rows per pass.  MASKED (n0 a multiple of 64): only the query's
// live rows are written; a range without a live tile ends at once, a wave skips its eight rows where none of them is live.
constexpr u32 F32X_EXACT_ROWS = 1024;
template <bool MASKED>
__global__ __launch_bounds__(256) void f32x_exact_scores(const uint8_t *__restrict__ qf, u64 row_stride, const float *__restrict__ qmags,
                                                         const uint8_t *__restrict__ codes, const float *__restrict__ mags, u32 n0, u32 n_chunk, u32 dim,
                                                         float *__restrict__ scores /*[B][s_stride]*/, u64 s_stride, const ScanMask m,
                                                         const u64 *__restrict__ tile_bits, u32 tb_stride, u32 tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *q_lds = (float *)smem_raw;
    const u32 q = blockIdx.x;
    const u32 c_begin = blockIdx.y * F32X_EXACT_ROWS, c_end = c_begin + F32X_EXACT_ROWS < n_chunk ? c_begin + F32X_EXACT_ROWS : n_chunk;
    if constexpr (MASKED) {
        const u64 *tb = tile_bits + (u64)m.qmask[q] * tb_stride;
        bool any = false;
        for (u32 i = 0; i < F32X_EXACT_ROWS / F_ROWS; i++) {
            const u32 t = (n0 + c_begin) / F_ROWS + i;
            any |= t < tiles && ((tb[t >> 6] >> (t & 63u)) & 1ull) != 0ull;
        }
        if (!any) return; // uniform: nothing of this query lives in the range
    }
    stage_f32_query(q_lds, qf + (u64)q * row_stride, dim);
    const float mq = qmags[q];
    for (u32 c0 = c_begin; c0 < c_end; c0 += 32) { // workgroup-uniform; the eight lanes of a row stay together
        const u32 c = c0 + (threadIdx.x >> 3);
        const bool live = c < c_end && scan_live<MASKED>(m, q, n0 + (c < c_end ? c : c_begin));
        if (!__any(live)) continue; // wave-uniform
        const u32 row = n0 + (live ? c : c_begin);
        const float dp = f32_oct_dot((const float *)(codes + (u64)row * row_stride), q_lds, dim, (int)(threadIdx.x & 7u));
        if (live && (threadIdx.x & 7u) == 0u) scores[(u64)q * s_stride + c] = x86_div(dp, __fmul_rn(mq, mags[row]));
    }
}

// The pool's rows again in the reference's order and sorted by the key of that score (total_cmp descending, larger id first):
// sorted[q][0 .. N) are the reference's N candidates when the pool holds them.  Empty keys stay empty and sort last.  One workgroup
// per query, 32 rows per pass; the sort is the shared LDS network.
template <u32 P>
__global__ __launch_bounds__(256) void f32x_rescore(const uint8_t *__restrict__ qf, u64 row_stride, const float *__restrict__ qmags, const uint8_t *__restrict__ codes,
                                                    const float *__restrict__ mags, u32 dim, const u64 *__restrict__ pool_mem, u64 *__restrict__ sorted /*[B][P]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *q_lds = (float *)smem_raw;                        // [dim], padded to 16 B
    u64 *keys = (u64 *)(smem_raw + staged_query_bytes(dim)); // [P]
    const u32 q = blockIdx.x;
    stage_f32_query(q_lds, qf + (u64)q * row_stride, dim);
    const float mq = qmags[q];
    for (u32 c = threadIdx.x >> 3; c < P; c += 32) { // P is a multiple of 32: workgroup-uniform
        const u64 pk = pool_mem[(u64)q * P + c];
        const bool valid = pk != 0ull;
        const u32 sid = (u32)pk, row = valid ? sid : 0u;
        const float dp = f32_oct_dot((const float *)(codes + (u64)row * row_stride), q_lds, dim, (int)(threadIdx.x & 7u));
        if ((threadIdx.x & 7u) == 0u) keys[c] = valid ? score_key(x86_div(dp, __fmul_rn(mq, mags[row])), sid) : 0ull;
    }
    lds_bitonic_sort_desc<P>(keys);
    for (u32 c = threadIdx.x; c < P; c += 256) sorted[(u64)q * P + c] = keys[c];
}
hipError_t launch_f32x_rescore(u32 P, const uint8_t *qf, u64 row_stride, const float *qmags, u32 B, const uint8_t *codes, const float *mags, u32 dim,
                               const u64 *pool, u64 *sorted, hipStream_t st) {
    const size_t smem = staged_query_bytes(dim) + (size_t)P * 8;
#define F32X_RESCORE(PP) case PP: hipLaunchKernelGGL(f32x_rescore<PP>, dim3(B), dim3(256), smem, st, qf, row_stride, qmags, codes, mags, dim, pool, sorted); break
    switch (P) {
        F32X_RESCORE(64); F32X_RESCORE(128); F32X_RESCORE(256); F32X_RESCORE(512); F32X_RESCORE(1024);
        default: return hipErrorInvalidValue;
    }
#undef F32X_RESCORE
    return hipGetLastError();
}

// flags[q] = 1 and *n_flagged += 1 where flat_plan.h f32_margin_safe says no.  The pool is sorted descending, P keys.  qmask / live
// set: a masked call, where a query with at most P live rows is not tested.  One thread per query.
__global__ void f32x_margin_kernel(const u64 *__restrict__ pool_mem, u32 P, u32 B, u32 N, u32 dim, const u32 *__restrict__ qmask, const u32 *__restrict__ live,
                                   u32 *__restrict__ flags, u32 *__restrict__ n_flagged) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    const u64 nth = pool_mem[(u64)q * P + N - 1], pth = pool_mem[(u64)q * P + P - 1];
    const float gn = simkey_inv((u32)(nth >> 32)), gp = simkey_inv((u32)(pth >> 32));
    const bool safe = live ? fp::f32_masked_margin_safe(gn, gp, dim, live[qmask[q]], P) : fp::f32_margin_safe(gn, gp, dim, (u32)(pth >> 32) != 0u);
    flags[q] = safe ? 0u : 1u;
    if (!safe) atomicAdd(n_flagged, 1u);
}
// *flag |= 1 when a row of the bitmap has a zero norm: the rows that are live for at least one query of a masked call
__global__ void f32x_zero_rows(const float *__restrict__ v, u32 n, const u32 *__restrict__ rows, u32 *__restrict__ flag) {
    bool z = false;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        z |= ((rows[i >> 5] >> (i & 31u)) & 1u) != 0u && v[i] == 0.0f;
    if (__any(z) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// One pass over B queries under W->mu: f16_run / f16m_run (kernels_flat_f16.hip, kernels_flat_f16_masked.hip) with this file's
// kernels.  mp.masked: `mask` with the plan's `used` masks and qmask[B]; else every row.  exact_pass: the flagged queries of an
// exact_mode 1 call again, every chunk unfused with its score matrix from f32x_exact_scores; its rows replace the first answer's.
int32_t f32x_run(cos_index *ix, FlatF16Ws *W, const float *queries, u32 B, u32 top_k, u32 mode, bool exact_pass, const cos_scan_mask *mask, const MaskPlan &mp,
                 u32 *out_ids, float *out_scores, u32 *out_counts, cos_flat_f16_stats *stats) {
    const u32 dim = ix->p.dim, n = ix->n, N = fp::CODE_POOL_FACTOR * top_k;
    const bool exact = exact_pass || mode == fp::F16_EXACT_ALWAYS, by_rule = !exact && mode == fp::F16_EXACT_BY_RULE, masked = mp.masked;
    const fp::Scan plan = fp::f16_scan(n, B, top_k, exact);
    const u32 P = plan.P, R = P / 64, tiles = fp::f16_tiles(n), blocks = fp::f16_query_blocks(B);
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
    need(W->flags, d_flags, 3); // [zero norm, overflow, queries flagged]
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
    // the queries as padded f32 rows with the quantizer's norm (scalar.rs:45) and |q| of the rerank
    if (e == hipSuccess) e = launch_quantize_rows(ENG_F32, d_q, dim, B, dim, ix->p.range_lo, ix->p.range_hi, d_qc, row_stride, d_qm, d_qrm, st);
    // zero norms, the f16 calls' rules: unmasked, the stored rows' answer once per upload; masked, the rows live for at least one query,
    // every call; the queries' flag comes back with the results
    bool zero = false;
    if (e == hipSuccess && !exact_pass && masked) {
        hipLaunchKernelGGL(f32x_zero_rows, dim3(1024), dim3(256), 0, st, (const float *)ix->d_mags.p, n, md.uni, d_flags);
        e = hipGetLastError();
    } else if (e == hipSuccess && !exact_pass) {
        if (!W->zn_valid || W->zn_n != n) {
            u32 hz = 0;
            e = launch_any_zero(ix->d_mags, n, d_flags, st);
            if (e == hipSuccess) e = hipMemcpyAsync(&hz, d_flags, 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e == hipSuccess) { W->zn_valid = true; W->zn_n = n; W->zn_zero = hz != 0; }
            if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, 4, st);
        }
        zero = e == hipSuccess && W->zn_zero;
    }
    if (e == hipSuccess && !exact_pass && !zero) e = launch_any_zero(d_qm, B, d_flags, st);
    const ScanMask sm = masked ? md.sm : ScanMask{nullptr, nullptr, 0u};
    u32 hflags[3] = {0u, 0u, 0u};
    std::vector<u32> h_len(masked ? blocks : 0u, 0u);
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
        const ScanBufs bufs{d_scores, s_stride, d_part, d_pool, d_thr, d_app, d_appcnt, d_flags + 1, sm};
        const F32ScanArgs args{d_qc, d_qm, B, ix->d_codes, ix->d_mags, row_stride, dim, d_scores, s_stride, bufs.fused_out(plan, nullptr),
                               F32Tiles{md.lists, md.list_len, tiles}};
        // a chunk's scoring kernel stands between a (start, stop) pair of events, read after the last chunk
        e = run_chunks(plan, attempt, bufs, st, [&](const fp::Chunk &c) {
            hipEvent_t ev0 = nullptr, ev1 = nullptr;
            hipError_t ce = W->event(n_ev, &ev0);
            if (ce == hipSuccess) ce = W->event(n_ev + 1, &ev1);
            if (ce == hipSuccess) { n_ev += 2; ce = hipEventRecord(ev0, st); }
            if (ce != hipSuccess) return ce;
            if (exact) {
                if (masked && c.n0 % F_ROWS) return hipErrorInvalidValue;
                const dim3 grid(B, (c.nc + F32X_EXACT_ROWS - 1) / F32X_EXACT_ROWS);
                const auto kernel = masked ? f32x_exact_scores<true> : f32x_exact_scores<false>;
                hipLaunchKernelGGL(kernel, grid, dim3(256), staged_query_bytes(dim), st, (const uint8_t *)d_qc, row_stride, (const float *)d_qm,
                                   (const uint8_t *)ix->d_codes.p, (const float *)ix->d_mags.p, c.n0, c.nc, dim, d_scores, s_stride, sm, md.tile_bits,
                                   md.tb_stride, tiles);
                ce = hipGetLastError();
            } else
                ce = launch_f32_scan(c.fused, masked, ix->n_cus, st, args, c.n0, c.nc);
            if (ce != hipSuccess) return ce;
            launches++;
            return hipEventRecord(ev1, st);
        });
        if (e == hipSuccess && by_rule) { // the pools are final (or about to be repeated): ranks N and P of each
            hipLaunchKernelGGL(f32x_margin_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const u64 *)d_pool, P, B, N, dim,
                               masked ? md.sm.qmask : (const u32 *)nullptr, masked ? md.live : (const u32 *)nullptr, d_qflag, d_flags + 2);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = launch_f32x_rescore(P, d_qc, row_stride, d_qm, B, ix->d_codes, ix->d_mags, dim, d_pool, d_sorted, st);
        if (e == hipSuccess) e = launch_flat_rerank(R, d_q, d_qrm, B, ix->d_raw, ix->d_raw_mags, dim, d_sorted, N, top_k, ix->p.id_base, d_oi, d_os, d_oc, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_ids, d_oi, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_scores, d_os, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_counts, d_oc, (size_t)B * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hflags, d_flags, 12, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && masked) e = hipMemcpyAsync(h_len.data(), md.list_len, (size_t)blocks * 4, hipMemcpyDeviceToHost, st);
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
    for (size_t i = 0; i + 1 < n_ev && e == hipSuccess && !zero; i += 2) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, W->evs[i], W->evs[i + 1]);
        gemm_ms += ms;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st); // the caller's arrays and the workspace's host arrays are free again
    HIP_TRY(e);
    if (zero) return cos_fail(COS_ERR_CALCULATION, "zero-norm query or live stored vector: DistanceError::CalculationError (cosine.rs:228-232)");
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
    if (int32_t xrc = f32x_run(ix, W, xq.data(), Bx, top_k, mode, true, mask, xmp, xi.data(), xs.data(), xc.data(), nullptr)) return xrc;
    for (u32 i = 0; i < Bx; i++) {
        memcpy(out_ids + (size_t)sel[i] * top_k, xi.data() + (size_t)i * top_k, (size_t)top_k * 4);
        memcpy(out_scores + (size_t)sel[i] * top_k, xs.data() + (size_t)i * top_k, (size_t)top_k * 4);
        out_counts[sel[i]] = xc[i];
    }
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_flat_search_f32_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, const cos_scan_mask *mask,
                                             const cos_flat_f16_opts *opts, uint32_t *out_ids, float *out_scores, uint32_t *out_counts,
                                             cos_flat_f16_stats *stats) {
    if (!ix || !queries || !out_ids || !out_scores || !out_counts || B == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors first");
    if (opts && opts->struct_size != sizeof(cos_flat_f16_opts)) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::struct_size is %u, expected %zu", opts->struct_size, sizeof(cos_flat_f16_opts));
    if (stats && stats->struct_size != sizeof(cos_flat_f16_stats) && stats->struct_size != COS_FLAT_F16_STATS_SIZE_V1)
        return cos_fail(COS_ERR_INVALID, "cos_flat_f16_stats::struct_size is %u, expected %zu (or %u)", stats->struct_size, sizeof(cos_flat_f16_stats), COS_FLAT_F16_STATS_SIZE_V1);
    const u32 mode = opts ? opts->exact_mode : (u32)fp::F16_EXACT_BY_RULE;
    if (mode > fp::F16_EXACT_ALWAYS) return cos_fail(COS_ERR_INVALID, "cos_flat_f16_opts::exact_mode is %u: 0, 1 or 2", mode);
    if (ix->eng != ENG_F32) return cos_fail(COS_ERR_STORAGE_MISMATCH, "cos_flat_search_f32_batch scans FullPrecisionFP rows (HalfPrecisionFP: cos_flat_search_f16_batch; codes: cos_flat_search_batch)");
    if (ix->p.metric != COS_METRIC_COSINE) return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_flat_search_f32_batch implements the cosine metric");
    if (int32_t krc = fp::check_f16_top_k(top_k)) return cos_fail(krc, "the f32 scan keeps at most 1024 survivors (2 * 5 * top_k): top_k must be in [1, 102]");
    MaskPlan mp;
    if (int32_t mrc = scan_mask_plan(mask, B, mp)) return mrc;
    if (int32_t rc = cos_set_device(ix)) return rc;
    FlatF16Ws *W = cos_flat_f16_ws(ix);
    std::lock_guard<std::mutex> wg(W->mu);
    return f32x_run(ix, W, queries, B, top_k, mode, false, mask, mp, out_ids, out_scores, out_counts, stats);
}
