// walk_common.h — the reference rules every HNSW walk kernel restates (ann_search / traverse_find_nearest, vector_store.rs:256-402,
// 1112-1204), written once: walk_kernel (walk_kernel.inc), walk_lat_kernel, walk_lat4_kernel, walk_general_kernel, walk_meta_kernel.
// Every piece is inlined into its caller; what decides unrolling or register residency (engine, chunk passes, lanes per row, rows
// in flight, pool width) is a template parameter or a value that is a constant at the call site.  The round structure of a kernel
// (windows, commit rules, pools) is its own and is not here.
#pragma once
#include "engine_types.h"
#include "dot_engines.h"
#include "topk_select.h"

namespace cosdev {

// status codes of include/cosdata_hip.h (the kernels do not see the C header) and the two ids that are not vector rows
constexpr int32_t COS_OK = 0, COS_ERR_CALCULATION = 2, COS_ERR_UNIMPLEMENTED = 4;
constexpr u32 COS_QUERY_ID = 0xFFFFFFFEu; // what a search pre-inserts in the visited filter in place of a node's own id
constexpr u32 COS_ROOT_ID = 0xFFFFFFFFu;  // internal id of the root (vector row N)
constexpr int LAT_ROW_LANES = 16;         // lanes per code row in both latency kernels: their rows hold <= 4 passes of 16 chunks

// the widest neighbour row of the graph (level 0 against the levels above it): sizes the visited filter, in the kernels and in
// their *_smem_bytes functions alike
__host__ __device__ __forceinline__ u32 walk_mmax(const IndexDev &ix) {
    return ix.lv[0].M > ix.lv[ix.num_layers].M ? ix.lv[0].M : ix.lv[ix.num_layers].M;
}

// ---- visited filter: PerformantFixedSet, 2 * M words of LDS per level ---------------------------------------------------------
// bucket = (id >> 6) & (M - 1), bit = id & 63  <=>  linear bit id & (64 * M - 1) (bitmask); the id of vector row `row`
__device__ __forceinline__ u32 vis_bit_of(u32 row, u32 N, u32 id_stride, u32 bitmask) {
    const u32 id = row == N ? COS_ROOT_ID : row * id_stride;
    return id & bitmask;
}
// a fresh filter for a level (vector_store.rs:266-271), by the NT threads that share it
template <int NT>
__device__ __forceinline__ void vis_clear(u32 *vis, u32 M, int tid) {
    for (u32 w = tid; w < 2 * M; w += NT) vis[w] = 0;
}
// the seeds of a level — the query's / new node's own id (vector_store.rs:266-271, :807) and the start node — set by ONE lane
__device__ __forceinline__ void vis_set_bit(u32 *vis, u32 bit) { vis[bit >> 5] |= 1u << (bit & 31); }
// Two slots of one expansion alias the same residue: the LOWER slot wins (sequential scan order).  cmask: the lanes that claimed
// their bit with an atomic OR, lostmask: those that found it set by then (by another lane of this expansion: it was clear when the
// expansion began).  Returns the expansion's winners.  Checked by tests/cxx/wave_prims_check.hip.
__device__ __forceinline__ u64 vis_alias_winners(u64 cmask, u32 bit, u64 lostmask) {
    u64 wmask = cmask & ~lostmask;
    while (lostmask) {
        const int l = __ffsll((long long)lostmask) - 1;
        const u64 g = cmask & ballot64(bit == readlane_u32(bit, l));
        wmask = (wmask & ~g) | (g & (0ull - g)); // of the slots that share the residue only the lowest stays
        lostmask &= ~g;
    }
    return wmask;
}

// ---- similarity from a dot product ---------------------------------------------------------------------------------------------
// metric 0: cosine_similarity_from_dot_product (cosine.rs:223-235), dot / (|q| * |v|); a zero denominator is a CalculationError,
// reported in `bad` (the quotient is then never used).  Any other metric: DotProductDistance (dotproduct.rs:14-64), the dot itself.
// UNSCALED is the one variant, and it differs in the division only: walk_kernel's evaluation blocks over u8 codes take
// div_rn_unscaled (device_common.h: same bits for their operand ranges, four instructions less).
template <bool UNSCALED = false>
__device__ __forceinline__ float cosine_or_dot(u32 metric, float dotf, float qmag, float mag, bool &bad) {
    bad = false;
    if (metric != 0u) return dotf;
    const float den = __fmul_rn(qmag, mag);
    bad = den == 0.0f;
    return UNSCALED ? div_rn_unscaled(dotf, den) : __fdiv_rn(dotf, den);
}

// ---- integer dots ----------------------------------------------------------------------------------------------------------------
// ONE row (a level's start node) by lane group 0: G lanes, CH chunk passes; the dot in every lane of the wave
template <int ENG, int CH>
__device__ __forceinline__ u32 int_row_dot_group0(const uint4 (&qreg)[CH], const uint8_t *row_ptr, u32 nchunks, int lig, int grp, int G) {
    u32 acc = 0;
    if (grp == 0) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const u32 chunk = (u32)lig + (u32)c * (u32)G;
            if (chunk < nchunks) acc = chunk_dot<ENG>(qreg[c], *(const uint4 *)(row_ptr + (u64)chunk * 16), acc);
        }
    }
    acc = group_reduce_add_u32(acc, G);
    return readlane_u32(acc, 0);
}

// The speculative evaluation block of the latency kernels: the similarities of the T compacted candidates cl[] (vector row |
// position << 32), 64 / GL rows per wave pass and PB passes in flight, parked at spec[position] as key | zero-denominator << 32.
// No lane is ever masked off: a lane group without a candidate re-reads the block's first row and a lane past the row's last
// chunk re-reads that chunk against a zero query chunk (both dropped / worth 0) — every predicated load was three scalar
// instructions of exec bookkeeping, 40 % of the one-wave kernel's instructions were scalar
// (profiles/archive/r02_single_batch_latency_walk_sq_counters.txt).
template <int ENG, int CH, int GL, int PB>
__device__ __forceinline__ void spec_row_dots(const u64 *cl, u64 *spec, u32 T, const uint4 (&qreg)[CH], const IndexDev &ix, float qmag, int lig, int grp) {
    constexpr int RP = 64 / GL; // rows per wave pass
    for (u32 b0 = 0; b0 < T; b0 += RP * PB) {
        uint4 buf[PB][CH];
        float pmag[PB];
        u32 ppos[PB], prow[PB];
#pragma unroll
        for (int p = 0; p < PB; p++) { // the candidates' rows first: one LDS round trip for the whole block
            if (b0 + (u32)(p * RP) >= T) break; // wave-uniform
            const u32 my = b0 + (u32)(p * RP + grp);
            const bool v = my < T;
            const u64 e = cl[v ? my : b0];
            prow[p] = (u32)e;
            ppos[p] = v ? (u32)(e >> 32) : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int p = 0; p < PB; p++) {
            if (b0 + (u32)(p * RP) >= T) break; // wave-uniform
            pmag[p] = ix.mags[prow[p]];
            const uint8_t *rp = ix.codes + (u64)prow[p] * ix.row_stride;
#pragma unroll
            for (int c = 0; c < CH; c++) {
                u32 chunk = (u32)lig + (u32)c * (u32)GL;
                if (c == CH - 1) chunk = chunk < ix.nchunks ? chunk : ix.nchunks - 1u; // only the last round of chunks can overshoot
                buf[p][c] = *(const uint4 *)(rp + (u64)chunk * 16);
            }
        }
#pragma unroll
        for (int p = 0; p < PB; p++) {
            if (b0 + (u32)(p * RP) >= T) break; // wave-uniform
            u32 part[CH]; // one chain per chunk: independent dot4 chains interleave instead of waiting on each other
#pragma unroll
            for (int c = 0; c < CH; c++) part[c] = chunk_dot<ENG>(qreg[c], buf[p][c], 0u);
            u32 acc = part[0];
#pragma unroll
            for (int c = 1; c < CH; c++) acc += part[c];
            acc = group_reduce_add_u32(acc, GL);
            bool bad;
            const float sim = cosine_or_dot(ix.metric, (float)acc, qmag, pmag[p], bad); // integer dot `as f32` (RNE)
            if (lig == 0 && ppos[p] != 0xFFFFFFFFu) spec[ppos[p]] = (u64)metric_key(ix.metric, sim) | (bad ? (1ull << 32) : 0ull);
        }
    }
}

// ---- level epilogue --------------------------------------------------------------------------------------------------------------
// the popped (key, node) list, R entries per lane, sorted descending (vector_store.rs:1194-1201)
template <int R>
__device__ __forceinline__ void sort_popped_list(u64 (&rk)[R], const u64 *res, u32 npop, int lane) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const u32 e = (u32)lane * R + r;
        rk[r] = e < npop ? res[e] : 0ull;
    }
    bitonic_sort_desc<R>(rk, lane);
}
// entry `pos` of a level's result list (obase: the list's first entry): internal id, similarity, node index
__device__ __forceinline__ void write_level_entry(u64 key, u64 pos, const IndexDev &ix, const LevelDev &lv, const WalkArgs &wa) {
    const u32 nd = (u32)key;
    const u32 vrow = lv.node_vec ? lv.node_vec[nd] : nd;
    wa.out_ids[pos] = vrow == ix.n ? COS_ROOT_ID : vrow * ix.id_stride;
    wa.out_sims[pos] = metric_key_inv(ix.metric, (u32)(key >> 32));
    if (wa.out_nodes) wa.out_nodes[pos] = nd;
}
__device__ __forceinline__ u64 level_list_base(const IndexDev &ix, const WalkArgs &wa, u32 qi, u32 out_slot) {
    return ((u64)qi * (ix.num_layers + 1) + out_slot) * wa.keep;
}
// the first cnt entries of the sorted list rk and the level's count, by one wave
template <int R>
__device__ __forceinline__ void write_level_list(const u64 (&rk)[R], u32 cnt, const IndexDev &ix, const LevelDev &lv, const WalkArgs &wa, u32 qi, u32 out_slot, int lane) {
    const u64 obase = level_list_base(ix, wa, qi, out_slot);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const u32 e = (u32)lane * R + r;
        if (e < cnt) write_level_entry(rk[r], obase + e, ix, lv, wa);
    }
    if (lane == 0) wa.out_counts[(u64)qi * (ix.num_layers + 1) + out_slot] = cnt;
}
// a query's counters (WalkArgs::out_stats), by one lane
__device__ __forceinline__ void write_walk_stats(u64 *out_stats, u32 qi, u64 n_evals, u64 n_exp, u64 adj_bytes, u64 n_rounds) {
    if (!out_stats) return;
    out_stats[(u64)qi * 4 + 0] = n_evals;
    out_stats[(u64)qi * 4 + 1] = n_exp;
    out_stats[(u64)qi * 4 + 2] = adj_bytes;
    out_stats[(u64)qi * 4 + 3] = n_rounds;
}

} // namespace cosdev
