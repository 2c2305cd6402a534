// kernels_meta_general.hip — the metadata walk OUTSIDE walk_meta_kernel's parameter domain (kernels_meta.hip): the same ann_search with
// query_filter_dims (vector_store.rs:256-402), the same per-level lists bit for bit, for
//   * code rows of any number of 16-byte chunks (walk_meta_kernel: the query row in <= 2 registers per lane — u8 up to 2048
//     dimensions, SubByte up to 64 chunks), and
//   * up to 256 scanned neighbour slots per node (walk_meta_kernel: one lane per slot, 64) — what the link kernels hold.
// One wave per query.  What differs from walk_meta_kernel is where things live and how an expansion is scheduled:
//   * the query row lies in LDS: the code row (integer engines) or its f32 values (f16 / f32), as in walk_general_kernel;
//   * the candidates stay in the register Pool<R> (ef <= 1024): a sorted set truncated at ef - popped does not depend on the order of
//     its inserts, so the pool, the popped list and the end-of-walk sort + merge (meta_walk.h) are walk_meta_kernel's;
//   * an expansion pops ONE entry and scans its slots in passes of 64, in slot order.  For all passes of the expansion together the
//     wave fetches the adjacency entries, then — together again — node_id / node_meta / node_vec of what they name, then mmags: three
//     trips to memory per expansion, parked in an LDS window of one row per pass (walk_meta_kernel's lookahead window, with the
//     passes of one expansion in the place of its window entries: nothing speculative, no commit rule);
//   * every pass tests and sets the level's shared visited filter with vis_alias_winners: the lower slot wins an alias, and passes in
//     ascending slot order keep that rule across passes;
//   * winners whose similarity the node-kind dispatch knows are inserted first; those that need the vector cosine are compacted in
//     slot order and evaluated one row at a time by the WHOLE wave — lane l takes chunks l, l + 64, ... against the query row in LDS.
//     The first MG_CB chunk passes of the NEXT winner's row are loaded before the current row is reduced and inserted, so two rows
//     are in flight and a row's latency hides under its predecessor (integer engines; f16 / f32 rows are reference-order chains —
//     one lane / eight lanes per row, f16_lane_dot / f32_oct_dot as in walk_meta_kernel).
// ef bound, keep, the dropped -1.0 entries, the empty-level fallback, INDEXING (self_ids, pre-inserted id, out_nodes, nothing
// dropped) and the status are walk_meta_kernel's.  launch_walk_meta[_index] send a launch here exactly when walk_meta_kernel cannot
// hold it (walk_meta_general_needed) or the knob meta_walk_general asks for it.  A domain, not a fast path: DESIGN.md §9.1.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "meta_walk.h"

using namespace cosdev;

namespace {

constexpr int MG_PASSES = 4; // passes of 64 slots per expansion: 256 slots, the widest neighbour row there is
constexpr int MG_CB = 4;     // chunk passes of the next row held in registers while the current one reduces (4 x 64 x 16 B = 4 KB of row)
constexpr int MG_FPB = 2;    // float engines: wave passes of rows in flight

// the kernel's LDS, in bytes from its base: ONE statement for the kernel, the launcher and cos_index_enable_metadata's check
struct MetaGenLayout {
    u32 vis, res, acc, wl_vec, wl_node, fq, fqi, win, qrow, total;
};
__host__ __device__ inline MetaGenLayout meta_general_layout(u32 mmax, u32 ef, u32 qbytes) {
    MetaGenLayout l;
    u32 p = 0;
    l.vis = p;     p += mmax * 8u;                         // PerformantFixedSet replica of the widest level: 2 x M words
    l.res = p;     p += (ef < 128u ? 128u : ef) * 8u;      // popped list of the current walk; doubles as the merge's 128-entry staging list
    l.acc = p;     p += 128u * 8u;                         // the level's list so far (<= 100)
    l.wl_vec = p;  p += 64u * 4u;                          // winners that need the vector cosine: rows | nodes
    l.wl_node = p; p += 64u * 4u;
    l.fq = p;      p += 64u * 4u;                          // the current filter's dimensions as f32 | i32
    l.fqi = p;     p += 64u * 4u;
    l.win = p;     p += 5u * MG_PASSES * 64u * 4u;         // pass window: [node | id | metadata row | vector row | metadata norm][pass][slot]
    p = (p + 15u) & ~15u;
    l.qrow = p;    p += (qbytes + 15u) & ~15u;             // the query row
    l.total = p + 16u;
    return l;
}
// bytes of the query row in LDS: the code row, the padded f32 row, or the f16 code widened to f32
__host__ __device__ inline u32 meta_general_query_bytes(int eng, const IndexDev &ix) {
    return eng == ENG_F16 ? ix.dim * 4u : (u32)ix.row_stride;
}

__device__ __forceinline__ void wave_lds_sync() { // one wave's LDS writes before its (other lanes') LDS reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int ENG, int R, bool INDEXING>
__global__ __launch_bounds__(64) void walk_meta_general_kernel(const IndexDev ix, const WalkArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const u32 qi = blockIdx.x;
    if (qi >= wa.B) return;
    constexpr bool FLOAT_ENG = ENG == ENG_F32 || ENG == ENG_F16;
    const u32 L = ix.num_layers, metric = ix.metric, md = ix.mdim, nchunks = ix.nchunks;
    const MetaGenLayout lay = meta_general_layout(walk_mmax(ix), wa.ef, meta_general_query_bytes(ENG, ix));
    u32 *vis = (u32 *)(smem_raw + lay.vis);
    u64 *res = (u64 *)(smem_raw + lay.res);
    u64 *acc = (u64 *)(smem_raw + lay.acc);
    u32 *wl_vec = (u32 *)(smem_raw + lay.wl_vec), *wl_node = (u32 *)(smem_raw + lay.wl_node);
    float *fq = (float *)(smem_raw + lay.fq);
    int32_t *fqi = (int32_t *)(smem_raw + lay.fqi);
    u32 *win = (u32 *)(smem_raw + lay.win);
    const uint4 *qrow4 = (const uint4 *)(smem_raw + lay.qrow); // integer engines: chunk c of the query's code row
    float *qf = (float *)(smem_raw + lay.qrow);                // float engines: the query's values

    const u32 qrow = (INDEXING && wa.q_rows) ? wa.q_rows[qi] : qi;
    const u32 self_id = INDEXING ? wa.self_ids[qi] : COS_QUERY_ID;
    const bool self_pseudo = INDEXING && self_id >= PSEUDO_LO && self_id <= PSEUDO_HI;
    const u32 keep_n = INDEXING ? wa.keep : (u32)KEEP_SEARCH;
    const uint8_t *qcode = wa.qcodes + (u64)qrow * ix.row_stride;
    const float qmag = wa.qmags[qrow];
    const u32 f0 = wa.f_off[qi], f1 = wa.f_off[qi + 1];

    if constexpr (FLOAT_ENG) stage_float_query<ENG, 64>(qf, qcode, ix, lane);
    else
        for (u32 c = lane; c < nchunks; c += 64) *(uint4 *)(smem_raw + lay.qrow + (size_t)c * 16) = *(const uint4 *)(qcode + (u64)c * 16);
    wave_lds_sync();

    // ---- one code row by the whole wave (integer engines) ------------------------------------------------------------------------
    // row_issue: the loads of the row's first MG_CB chunk passes (lane l: chunks l, l + 64, ...) and of its norm — nothing waits;
    // row_dot: those chunks against the query row, then whatever the row has beyond them, reduced over the wave (every lane)
    auto row_issue = [&](u32 row, uint4 (&b)[MG_CB], float &mag) {
        const uint8_t *rp = ix.codes + (u64)row * ix.row_stride;
#pragma unroll
        for (int c = 0; c < MG_CB; c++) {
            const u32 chunk = (u32)lane + (u32)c * 64u;
            b[c] = make_uint4(0, 0, 0, 0);
            if (chunk < nchunks) b[c] = *(const uint4 *)(rp + (u64)chunk * 16);
        }
        mag = ix.mags[row];
    };
    auto row_dot = [&](u32 row, const uint4 (&b)[MG_CB]) -> u32 {
        u32 a = 0u;
        if constexpr (!FLOAT_ENG) {
            u32 part[MG_CB]; // one chain per chunk pass: independent chains interleave
#pragma unroll
            for (int c = 0; c < MG_CB; c++) {
                const u32 chunk = (u32)lane + (u32)c * 64u;
                part[c] = 0u;
                if (chunk < nchunks) part[c] = chunk_dot<ENG>(qrow4[chunk], b[c], 0u);
            }
            a = (part[0] + part[1]) + (part[2] + part[3]);
            const uint8_t *rp = ix.codes + (u64)row * ix.row_stride;
            for (u32 chunk = (u32)lane + (u32)MG_CB * 64u; chunk < nchunks; chunk += 64u) a = chunk_dot<ENG>(qrow4[chunk], *(const uint4 *)(rp + (u64)chunk * 16), a);
            a = group_reduce_add_u32(a, 64);
        }
        return readlane_u32(a, 0);
    };
    static_assert(MG_CB == 4, "row_dot sums four partial chains");

    // vector cosine / dot of ONE row (a level's start node); valid in every lane
    auto vec_distance_single = [&](u32 row, float &sim_out) -> bool {
        float dotf, mag;
        if constexpr (!FLOAT_ENG) {
            uint4 b[MG_CB];
            row_issue(row, b, mag);
            dotf = (float)row_dot(row, b); // integer dot `as f32` (RNE)
        } else {
            dotf = float_row_dot_wave<ENG>(ix.codes + (u64)row * ix.row_stride, qf, ix.dim, lane);
            mag = ix.mags[row];
        }
        bool bad;
        sim_out = cosine_or_dot(metric, dotf, qmag, mag, bad);
        return !bad;
    };

    int32_t status = COS_OK;
    u32 entry = ix.lv[L].root_idx;

    for (int level = (int)L; level >= 0 && status == COS_OK; level--) {
        const LevelDev lv = ix.lv[level];
        const u32 M = lv.M;
        const u32 slots = M < ix.shortlist ? M : ix.shortlist; // <= 256 = MG_PASSES x 64 (cos_index_create)
        const u32 bitmask = 64u * M - 1u;
        const u32 out_slot = L - (u32)level;
        vis_clear<64>(vis, M, lane);
        wave_lds_sync();
        if (lane == 0) vis_set_bit(vis, self_id & bitmask);
        u32 nacc = 0; // merged candidates so far (acc)

        for (u32 f = f0; f < f1 && status == COS_OK; f++) {
            meta_stage_filter(wa, f, md, fqi, fq, lane); // this filter's dimensions -> LDS
            const float fmag = wa.f_mags[f];
            const int xkind = meta_query_kind(fmag, self_pseudo);

            Pool<R> pool;
            pool.clear();
            u32 npool = 0, npop = 0;
            { // start node: evaluated and pushed whatever the visited filter says (vector_store.rs:1144-1148)
                const u32 eid = lv.node_id[entry], ek = lv.node_meta[entry];
                const float eymag = ix.mmags[ek];
                float s0 = 0.0f;
                int dec = 0;
                if (lane == 0) dec = meta_decide(ix, fq, fqi, ek, eymag, eid, fmag, xkind, s0);
                dec = (int)readlane_u32((u32)dec, 0);
                s0 = __uint_as_float(readlane_u32(__float_as_uint(s0), 0));
                if (dec < 0) { status = -dec; break; }
                if (dec == 1 && !vec_distance_single(lv.node_vec[entry], s0)) { status = COS_ERR_CALCULATION; break; }
                if (lane == 0) vis_set_bit(vis, eid & bitmask);
                pool.insert_at(pack_key(metric_key(metric, s0), entry), 0, lane);
                npool = 1;
                wave_lds_sync();
            }
            bool failed = false;
            while (npool > 0 && npop < wa.ef && !failed) {
                const u64 cur = pool.head();
                pool.pop_head(lane);
                npool--;
                if (lane == 0) res[npop] = cur;
                npop++;
                const int limit = (int)wa.ef - (int)npop; // future pops still allowed = the candidates worth keeping
                const u32 node = (u32)cur;
                { // the expansion's window: three trips to memory for ALL its passes.  No lane is masked off: a lane past the last
                  // slot re-reads slot slots - 1 and drops it, an empty slot reads node 0 and never looks at it.
                    u32 wnb[MG_PASSES], wid[MG_PASSES], wk[MG_PASSES], wvr[MG_PASSES];
                    float wym[MG_PASSES];
                    static_for<0, MG_PASSES>([&](auto pc) {
                        constexpr int p = decltype(pc)::value;
                        if ((u32)p * 64u < slots) { // wave-uniform
                            const u32 slot = (u32)p * 64u + (u32)lane;
                            wnb[p] = lv.adj_node[(u64)node * M + (slot < slots ? slot : slots - 1u)];
                        }
                    });
                    static_for<0, MG_PASSES>([&](auto pc) {
                        constexpr int p = decltype(pc)::value;
                        if ((u32)p * 64u < slots) {
                            if ((u32)p * 64u + (u32)lane >= slots) wnb[p] = ROW_EMPTY;
                            const u32 nbs = wnb[p] != ROW_EMPTY ? wnb[p] : 0u;
                            wid[p] = lv.node_id[nbs];
                            wk[p] = lv.node_meta[nbs];
                            wvr[p] = lv.node_vec[nbs];
                        }
                    });
                    static_for<0, MG_PASSES>([&](auto pc) {
                        constexpr int p = decltype(pc)::value;
                        if ((u32)p * 64u < slots) wym[p] = ix.mmags[wk[p]];
                    });
                    static_for<0, MG_PASSES>([&](auto pc) {
                        constexpr int p = decltype(pc)::value;
                        if ((u32)p * 64u < slots) {
                            win[(0 * MG_PASSES + p) * 64 + lane] = wnb[p];
                            win[(1 * MG_PASSES + p) * 64 + lane] = wid[p];
                            win[(2 * MG_PASSES + p) * 64 + lane] = wk[p];
                            win[(3 * MG_PASSES + p) * 64 + lane] = wvr[p];
                            win[(4 * MG_PASSES + p) * 64 + lane] = __float_as_uint(wym[p]);
                        }
                    });
                }
                // inserts one evaluated winner (wave-uniform key) into the truncated pool
                auto pool_insert = [&](u64 kk) {
                    const int pos = pool.rank_of(kk);
                    if (pos < limit) { pool.insert_at(kk, pos, lane); if (npool < (u32)(64 * R)) npool++; }
                };
                for (u32 p = 0; p * 64u < slots && !failed; p++) { // passes in ascending slot order (vector_store.rs:1161-1171)
                    const u32 nb_node = win[(0 * MG_PASSES + p) * 64 + lane];
                    const bool valid = nb_node != ROW_EMPTY;
                    const u32 nid_l = win[(1 * MG_PASSES + p) * 64 + lane], nk = win[(2 * MG_PASSES + p) * 64 + lane], nvrow = win[(3 * MG_PASSES + p) * 64 + lane];
                    const float nymag = __uint_as_float(win[(4 * MG_PASSES + p) * 64 + lane]);
                    const u32 nid = valid ? nid_l : 0u;
                    const u32 bit = nid & bitmask, word = bit >> 5, msk = 1u << (bit & 31);
                    const bool pre = valid && (vis[word] & msk);
                    const bool cand = valid && !pre;
                    if (!__any(cand)) continue;
                    u32 old = 0;
                    if (cand) old = atomicOr(&vis[word], msk);
                    const bool winr = __builtin_amdgcn_inverse_ballot_w64(vis_alias_winners(__ballot(cand), bit, __ballot(cand && (old & msk))));
                    wave_lds_sync(); // the next pass reads the filter this one set
                    // node-kind dispatch per winner
                    float csim = 0.0f;
                    int dec = 0;
                    if (winr) dec = meta_decide(ix, fq, fqi, nk, nymag, nid, fmag, xkind, csim);
                    const u64 errm = __ballot(winr && dec < 0);
                    if (errm) { status = -(int)readlane_u32((u32)dec, __ffsll((long long)errm) - 1); failed = true; break; }
                    // winners whose similarity is already known, in slot order
                    u64 cm = __ballot(winr && dec == 0);
                    const u32 ckey = metric_key(metric, csim);
                    while (cm) {
                        const int l = __ffsll((long long)cm) - 1;
                        cm &= cm - 1;
                        pool_insert(pack_key(readlane_u32(ckey, l), readlane_u32(nb_node, l)));
                    }
                    // winners that need the vector cosine: compacted in slot order
                    const bool vwin = winr && dec == 1;
                    const u64 vmask = __ballot(vwin);
                    const int W = __popcll(vmask);
                    if (W == 0) continue;
                    if (vwin) {
                        const int rank = __popcll(vmask & ((1ull << lane) - 1ull));
                        wl_vec[rank] = nvrow;
                        wl_node[rank] = nb_node;
                    }
                    wave_lds_sync();
                    if constexpr (!FLOAT_ENG) {
                        // one row at a time by the whole wave, two rows in flight: row w + 1's loads are issued before row w is
                        // reduced and inserted (two register buffers, taken in turn)
                        uint4 bufa[MG_CB], bufb[MG_CB];
                        float maga, magb = 1.0f;
                        auto finish = [&](int w, const uint4 (&b)[MG_CB], float mag) {
                            const u32 dot = row_dot(wl_vec[w], b);
                            bool bad;
                            const float sim = cosine_or_dot(metric, (float)dot, qmag, mag, bad); // integer dot `as f32` (RNE)
                            if (bad) { status = COS_ERR_CALCULATION; failed = true; return; }
                            pool_insert(pack_key(metric_key(metric, sim), wl_node[w]));
                        };
                        row_issue(wl_vec[0], bufa, maga);
                        for (int w = 0; w < W && !failed; w += 2) {
                            if (w + 1 < W) row_issue(wl_vec[w + 1], bufb, magb);
                            finish(w, bufa, maga);
                            if (failed || w + 1 >= W) break;
                            if (w + 2 < W) row_issue(wl_vec[w + 2], bufa, maga);
                            finish(w + 1, bufb, magb);
                        }
                    } else {
                        // reference-order chains: f32 eight lanes per row, f16 one lane per row; RP rows per wave pass
                        constexpr int G = ENG == ENG_F32 ? 8 : 1, RP = 64 / G;
                        const int grp = lane / G;
                        for (int base = 0; base < W && !failed; base += RP * MG_FPB) {
                            float pmag[MG_FPB], fdot[MG_FPB];
#pragma unroll
                            for (int q = 0; q < MG_FPB; q++) {
                                if (base + q * RP >= W) break;
                                const int my = base + q * RP + grp;
                                const u32 prow = my < W ? wl_vec[my] : 0u; // a lane group without a winner chains row 0 (dropped)
                                pmag[q] = my < W ? ix.mags[prow] : 1.0f;
                                if constexpr (ENG == ENG_F32) fdot[q] = f32_oct_dot((const float *)(ix.codes + (u64)prow * ix.row_stride), qf, ix.dim, lane & 7);
                                else fdot[q] = f16_lane_dot(ix.codes + (u64)prow * ix.row_stride, qf, ix.dim);
                            }
#pragma unroll
                            for (int q = 0; q < MG_FPB; q++) {
                                if (base + q * RP >= W) break;
                                bool bad;
                                const float sim = cosine_or_dot(metric, fdot[q], qmag, pmag[q], bad);
                                if (__any(bad && base + q * RP + grp < W)) { status = COS_ERR_CALCULATION; failed = true; break; }
                                const u32 key = metric_key(metric, sim);
                                for (int g = 0; g < RP; g++) {
                                    const int my = base + q * RP + g;
                                    if (my >= W) break;
                                    pool_insert(pack_key(readlane_u32(key, g * G), wl_node[my]));
                                }
                            }
                        }
                    }
                    wave_lds_sync(); // the next pass rewrites the winner lists
                }
            }
            if (failed || status != COS_OK) break;
            // this walk's result: popped list sorted descending, first 100; entries with cosine exactly -1.0 are dropped;
            // merged into the level's candidate list (sorted descending, first 100 kept)
            wave_lds_sync();
            nacc = meta_merge_walk<R, INDEXING>(res, acc, npop, nacc, keep_n, metric, lane);
        }
        if (status != COS_OK) break;

        if (nacc == 0) { // no candidate survived: the entry node with its strongest match over the filters
            u64 best = 0ull;
            for (u32 f = f0; f < f1 && status == COS_OK; f++) {
                meta_stage_filter(wa, f, md, fqi, fq, lane);
                const float fmag = wa.f_mags[f];
                const int xkind = fmag == 0.0f ? KIND_BASE : KIND_METADATA; // (vector_store.rs:329-367: the fallback builds the query without an id)
                const u32 eid = lv.node_id[entry], ek = lv.node_meta[entry];
                const float eymag = ix.mmags[ek];
                float s0 = 0.0f;
                int dec = 0;
                if (lane == 0) dec = meta_decide(ix, fq, fqi, ek, eymag, eid, fmag, xkind, s0);
                dec = (int)readlane_u32((u32)dec, 0);
                s0 = __uint_as_float(readlane_u32(__float_as_uint(s0), 0));
                if (dec < 0) { status = -dec; break; }
                if (dec == 1 && !vec_distance_single(lv.node_vec[entry], s0)) { status = COS_ERR_CALCULATION; break; }
                const u64 kk = pack_key(metric_key(metric, s0), entry);
                if (best == 0ull || (u32)(kk >> 32) > (u32)(best >> 32)) best = kk;
                __builtin_amdgcn_wave_barrier();
            }
            if (status != COS_OK) break;
            if (best == 0ull) { status = COS_ERR_UNIMPLEMENTED; break; } // a query without any filter does not come here
            if (lane == 0) acc[0] = best;
            nacc = 1;
            wave_lds_sync();
        }
        meta_write_level<INDEXING>(acc, nacc, ix, lv, wa, qi, out_slot, lane);
        if (level > 0) entry = lv.child[(u32)acc[0]];
        wave_lds_sync();
    }
    if (lane == 0) wa.out_status[qi] = status;
}

template <int ENG, int R, bool INDEXING>
hipError_t launch_inst(const IndexDev &ix, const WalkArgs &wa, size_t smem, hipStream_t st) {
    const hipError_t e = hipFuncSetAttribute((const void *)walk_meta_general_kernel<ENG, R, INDEXING>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((walk_meta_general_kernel<ENG, R, INDEXING>), dim3(wa.B), dim3(64), smem, st, ix, wa);
    return hipGetLastError();
}

template <int ENG, bool INDEXING>
hipError_t launch_r(const IndexDev &ix, const WalkArgs &wa, hipStream_t st) {
    const size_t smem = walk_meta_general_smem_bytes(ix, wa.ef, ENG);
    if (wa.ef <= 64) return launch_inst<ENG, 1, INDEXING>(ix, wa, smem, st);
    if (wa.ef <= 256) return launch_inst<ENG, 4, INDEXING>(ix, wa, smem, st);
    if (wa.ef <= 512) return launch_inst<ENG, 8, INDEXING>(ix, wa, smem, st);
    if (wa.ef <= WALK_FAST_MAX_EF) return launch_inst<ENG, 16, INDEXING>(ix, wa, smem, st);
    return hipErrorInvalidValue;
}

template <bool INDEXING>
hipError_t launch_eng(int eng, const IndexDev &ix, const WalkArgs &wa, hipStream_t st) {
    switch (eng) {
    case ENG_U8: return launch_r<ENG_U8, INDEXING>(ix, wa, st);
    case ENG_Q2: return launch_r<ENG_Q2, INDEXING>(ix, wa, st);
    case ENG_Q1: return launch_r<ENG_Q1, INDEXING>(ix, wa, st);
    case ENG_Q3: return launch_r<ENG_Q3, INDEXING>(ix, wa, st);
    case ENG_F32: return launch_r<ENG_F32, INDEXING>(ix, wa, st);
    case ENG_F16: return launch_r<ENG_F16, INDEXING>(ix, wa, st);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

namespace cosdev {

// filter words of the widest level, popped list, level list, winner lists, filter, pass window, query row (meta_general_layout)
size_t walk_meta_general_smem_bytes(const IndexDev &ix, u32 ef, int eng) {
    return meta_general_layout(walk_mmax(ix), ef, meta_general_query_bytes(eng, ix)).total;
}

// a chunk-pass count above walk_meta_kernel's (u8: 2 passes of G lanes, SubByte: 1), or more than 64 scanned slots on any level
bool walk_meta_general_needed(int eng, const IndexDev &ix) {
    if (eng != ENG_F32 && eng != ENG_F16 && ix.nchunks != 0u && (ix.nchunks + ix.G - 1u) / ix.G > (eng == ENG_U8 ? 2u : 1u)) return true;
    for (u32 l = 0; l <= ix.num_layers; l++)
        if (std::min(ix.lv[l].M, ix.shortlist) > 64u) return true;
    return false;
}

hipError_t launch_walk_meta_general(int eng, bool indexing, const IndexDev &ix, const WalkArgs &wa, hipStream_t st) {
    if (wa.B == 0) return hipSuccess;
    for (u32 l = 0; l <= ix.num_layers; l++)
        if (std::min(ix.lv[l].M, ix.shortlist) > 64u * MG_PASSES) return hipErrorInvalidValue; // the pass window holds 256 slots
    return indexing ? launch_eng<true>(eng, ix, wa, st) : launch_eng<false>(eng, ix, wa, st);
}

} // namespace cosdev
