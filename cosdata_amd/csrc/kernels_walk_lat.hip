// kernels_walk_lat.hip — the LATENCY variant of walk_kernel (kernels_walk.hip) for small launches: same walk
// (ann_search / traverse_find_nearest, vector_store.rs:256-402, 1112-1204), same per-level lists bit for bit.
//
// A lone 256-query batch (the reference's `query-batch = 256`) gives the throughput kernel one wave per CU: that wave spends
// 42 % of its cycles issuing (77 instructions per distance evaluation with one code row per wave pass) and 58 % parked on a
// chain of dependent HBM round trips — adjacency row, then the code rows of every window entry one entry after the other.
// Here, still one wave per query:
//   * SPECULATION across the lookahead window.  The adjacency rows of the next `la` (<= 4) pool entries arrive together; every
//     neighbour that is unvisited *under the filter as it stands at the start of the round* is a candidate, the code rows of ALL
//     candidates of ALL window entries are fetched together (up to 32 rows in flight) and their similarities parked in LDS.  The
//     entries are then COMMITTED in pop order exactly like the throughput kernel: visited claims, inserts, the "still provably
//     the next pop" rule.  The filter only gains bits during a round, so a slot that wins at commit time was a candidate at
//     the start of the round: its similarity is there.  A similarity is a pure function of (query, row), so using the parked
//     value changes nothing; candidates that lose (claimed by an earlier entry of the round, or the window went stale) are
//     wasted bandwidth — on a chip that a small launch leaves idle.  A round is two dependent HBM round trips whatever the
//     window holds.
//   * 16 lanes per code row (4 rows per wave pass, 48-64 B per lane at 768-1024 u8 dims), no predicated load, one v_dot4 chain per
//     chunk; the commit is unrolled over the window (rows and keys stay in registers) and screens an expansion's winners with one
//     vector compare before the insertion loop.  A lone wave pays ~4 clocks for EVERY instruction, scalar ones included, so the
//     kernel is written for instruction count (DESIGN.md 4.1 has the step-by-step measurements).
// Integer engines ENG_U8 / ENG_Q2 with <= 64 chunks per row, ef <= 256, reference visited filter; everything else stays on
// walk_kernel (launch_walk decides; cos_index_set_latency_mode).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "engine_types.h"
#include "tuning.h"
#include "walk_common.h"

using namespace cosdev;

namespace {

constexpr int LAL = 4;  // window capacity (adjacency rows prefetched per round); the launch picks la <= LAL.  8 measured slower (see launch_walk_lat)
constexpr int GL = LAT_ROW_LANES; // lanes per code row (4 rows per wave pass)
constexpr int PBL = 8;  // passes in flight before the dots are consumed (32 rows)

template <int ENG, int CH, int R, bool PREFETCH_ADJ>
__global__ __launch_bounds__(64) void walk_lat_kernel(const IndexDev ix, const WalkArgs wa, const u32 la) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const u32 qi = blockIdx.x;
    if (qi >= wa.B) return;

    u64 *s_spec, *s_cl, *s_res;
    u32 *s_vis;
    {
        unsigned char *p = smem_raw;
        s_spec = (u64 *)p;     p += (size_t)LAL * 64 * 8; // per (window entry, slot): similarity key | zero-denominator flag << 32
        s_cl = (u64 *)p;       p += (size_t)LAL * 64 * 8; // compacted candidates: vector row | (entry * 64 + slot) << 32
        s_res = (u64 *)p;      p += (size_t)wa.ef * 8;    // popped (key, node) list
        s_vis = (u32 *)p;      // visited filter words, Mmax * 2
    }

    const u32 qrow = wa.q_rows ? wa.q_rows[qi] : qi;
    const u32 self_id = wa.self_ids ? wa.self_ids[qi] * ix.id_stride : COS_QUERY_ID;
    const uint8_t *qcode = wa.qcodes + (u64)qrow * ix.row_stride;
    const float qmag = wa.qmags[qrow];
    const u32 N = ix.n;
    const u32 L = ix.num_layers;
    const u32 metric = ix.metric;

    const int lig = lane & (GL - 1);
    const int grp = lane / GL;
    const u64 lt_mask = (1ull << lane) - 1ull;
    uint4 qreg[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const u32 chunk = (u32)lig + (u32)c * (u32)GL;
        qreg[c] = chunk < ix.nchunks ? *(const uint4 *)(qcode + (u64)chunk * 16) : make_uint4(0, 0, 0, 0);
    }

    u64 n_evals = 0, n_exp = 0, adj_bytes = 0, n_rounds = 0;
    int32_t status = COS_OK;
    u32 entry = ix.lv[L].root_idx;
    u32 warm = 0; // see the L2 warm-up in step 2

    // similarity of ONE row, computed by lane group 0; result in every lane
    auto single_distance = [&](u32 row, float &sim_out) -> bool {
        const u32 acc = int_row_dot_group0<ENG, CH>(qreg, ix.codes + (u64)row * ix.row_stride, ix.nchunks, lig, grp, GL);
        bool bad;
        sim_out = cosine_or_dot(metric, (float)acc, qmag, ix.mags[row], bad); // integer dot `as f32` (RNE)
        return !bad;
    };

    for (int level = (int)L; level >= 0; level--) {
        const LevelDev lv = ix.lv[level];
        const u32 M = lv.M;
        const u32 slots = M < ix.shortlist ? M : ix.shortlist;
        const u32 bitmask = 64u * M - 1u;
        const u32 out_slot = L - (u32)level;

        // fresh visited filter, pre-seeded with the query / new-node id (vector_store.rs:266-271, :807)
        vis_clear<64>(s_vis, M, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) vis_set_bit(s_vis, self_id & bitmask);

        Pool<R> pool;
        pool.clear();
        u32 npool = 0, npop = 0;

        { // start node (vector_store.rs:1144-1148)
            const u32 erow = lv.node_vec ? lv.node_vec[entry] : entry;
            float s0;
            n_evals++;
            if (!single_distance(erow, s0)) { status = COS_ERR_CALCULATION; break; }
            if (lane == 0) vis_set_bit(s_vis, vis_bit_of(erow, N, ix.id_stride, bitmask));
            pool.insert_at(pack_key(metric_key(metric, s0), entry), 0, lane);
            npool = 1;
        }
        __builtin_amdgcn_wave_barrier();

        bool failed = false;
        while (npool > 0 && npop < wa.ef) {
            n_rounds++;
            u32 kwin = npool < la ? npool : la;
            if (kwin > wa.ef - npop) kwin = wa.ef - npop;

            // ---- 1. adjacency rows of the window entries: independent loads, one latency -----------------------------------
            u32 av[LAL], an[LAL];
            u64 wkey[LAL]; // wave-uniform: the window entries' (key, node); entries past kwin are never looked at
            // Every load is issued before the first value is looked at, and none is predicated: entries past kwin re-read node 0's
            // row, lanes past `slots` re-read the last slot (both replaced by ROW_EMPTY afterwards).  The first version wrote
            // `an[i] = level == 0 ? av[i] : ...` inside the per-entry `if`: the copy made the compiler wait for av[i] (s_waitcnt
            // vmcnt(0)) before it issued entry i+1's load — four DEPENDENT round trips per round instead of one.
            const u32 slot_l = (u32)lane < slots ? (u32)lane : slots - 1u;
            static_for<0, LAL>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                wkey[i] = pool.template peek<i>();
                const u32 nd = (u32)i < kwin ? (u32)wkey[i] : 0u;
                av[i] = lv.adj_vec[(u64)nd * M + slot_l];
            });
            if (level != 0) {
                static_for<0, LAL>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    const u32 nd = (u32)i < kwin ? (u32)wkey[i] : 0u;
                    an[i] = lv.adj_node[(u64)nd * M + slot_l];
                });
            }
            static_for<0, LAL>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const bool live = (u32)i < kwin && (u32)lane < slots;
                av[i] = live ? av[i] : ROW_EMPTY;
                an[i] = live ? (level == 0 ? av[i] : an[i]) : ROW_EMPTY;
            });

            // ---- 2. candidates: unvisited under the filter as it stands now (read only), compacted entry by entry ----------
            u32 T = 0;
            u32 wv[2 * LAL]; // L2 warm-up loads (below)
            u32 vword[LAL]; // the filter words first (one LDS round trip for the window), then the ballots
            static_for<0, LAL>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                vword[i] = s_vis[vis_bit_of(av[i], N, ix.id_stride, bitmask) >> 5]; // an empty slot maps somewhere inside the filter too
            });
            static_for<0, LAL>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const bool c = av[i] != ROW_EMPTY && !(vword[i] & (1u << (vis_bit_of(av[i], N, ix.id_stride, bitmask) & 31u))); // entries past kwin hold only empty slots
                const u64 cm = __ballot(c);
                if (c) s_cl[T + (u32)__popcll(cm & lt_mask)] = (u64)av[i] | ((u64)(u32)(i * 64 + lane) << 32);
                T += (u32)__popcll(cm);
                // L2 warm-up: a candidate that is evaluated now is expanded a few rounds later, and its adjacency row is then the
                // FIRST of the round's two dependent HBM round trips.  One dword per 128-byte line of that row, requested now (a lane
                // per candidate: two load instructions per window entry, on a chip a small launch leaves idle), turns that trip
                // into an L2 / Infinity Cache hit.  The values are folded into `warm` AFTER step 3 (loads complete in order, so by
                // then they have arrived with the code rows and nothing waits for them on their own); `warm` is only ever written
                // out under a condition that cannot hold, so the loads survive the optimizer.
                if (PREFETCH_ADJ) {
                    const u32 *arow = lv.adj_vec + (u64)(c ? an[i] : 0u) * M;
                    wv[i] = arow[0];
                    wv[LAL + i] = arow[M > 32 ? 32 : 0];
                }
            });
            __builtin_amdgcn_wave_barrier();

            // ---- 3. similarities of every candidate: 4 rows per pass, PBL passes in flight, no lane ever masked off ----------
            spec_row_dots<ENG, CH, GL, PBL>(s_cl, s_spec, T, qreg, ix, qmag, lig, grp);
            if (PREFETCH_ADJ) {
#pragma unroll
                for (int i = 0; i < 2 * LAL; i++) warm ^= wv[i];
            }
            __builtin_amdgcn_wave_barrier();

            // ---- 4. commit in pop order: walk_kernel's consume loop with the similarities read from LDS --------------------
            // Unrolled over the window so that an entry's adjacency row and key stay in the registers step 1 loaded them into
            // (the runtime loop read them back from LDS: three more dependent LDS round trips per pop for a lone wave).
            bool window_ok = true;
            static_for<0, LAL>([&](auto ic) {
                constexpr int wi = decltype(ic)::value;
                if ((u32)wi < kwin && window_ok && !failed) { // wave-uniform
                    const u64 sp_all = s_spec[wi * 64 + lane]; // issued with the filter word below: one LDS wait for both
                    pool.pop_head(lane);
                    npool--;
                    if (lane == 0) s_res[npop] = wkey[wi];
                    npop++;
                    n_exp++;
                    adj_bytes += (u64)slots * 4;
                    const int limit = (int)wa.ef - (int)npop;     // future pops still allowed
                    const int ahead = (int)kwin - 1 - wi;         // window entries still waiting at pool positions 0..ahead-1

                    const u32 nb_vec = av[wi], nb_node = an[wi];
                    const bool valid = nb_vec != ROW_EMPTY;
                    const u32 bit = vis_bit_of(nb_vec, N, ix.id_stride, bitmask);
                    const u32 word = bit >> 5, msk = 1u << (bit & 31);
                    const bool pre = valid && (s_vis[word] & msk);
                    const bool cand = valid && !pre;
                    if (__any(cand)) { // else nothing new: the next window entry is certainly the next pop
                        u32 old = 0;
                        if (cand) old = atomicOr(&s_vis[word], msk);
                        u64 m = vis_alias_winners(__ballot(cand), bit, __ballot(cand && (old & msk)));
                        const bool win = __builtin_amdgcn_inverse_ballot_w64(m);
                        n_evals += (u64)__popcll(m);
                        if (__any(win && (sp_all >> 32) != 0ull)) failed = true; // zero denominator -> CalculationError
                        else {
                            const u32 keyv = (u32)sp_all;
                            // one vector compare screens every winner against the entry that closes the poppable part of the pool
                            // (position limit - 1): below it a key has at least `limit` entries above it and the loop would only
                            // rank it to reject it.  The bar only rises while winners go in, so the screen is conservative.
                            const u64 bar = limit > 0 ? pool.peek_dyn((u32)(limit - 1)) : ~0ull;
                            m = __ballot(win && pack_key(keyv, nb_node) > bar);
                            while (m) { // winners in slot order (vector_store.rs:1161-1171)
                                const int l = __ffsll((long long)m) - 1;
                                m &= m - 1;
                                const u64 kk = pack_key(readlane_u32(keyv, l), readlane_u32(nb_node, l));
                                const int pos = pool.rank_of(kk);
                                if (pos < limit) {
                                    pool.insert_at(kk, pos, lane);
                                    if (npool < (u32)(64 * R)) npool++;
                                    if (pos < ahead) window_ok = false; // landed ahead of a prefetched entry: the window is stale
                                }
                            }
                        }
                    }
                }
            });
            if (failed) break;
            __builtin_amdgcn_wave_barrier();
        }
        if (failed) { status = COS_ERR_CALCULATION; break; }

        // keep the best `keep`, sorted descending (vector_store.rs:1194-1201)
        __builtin_amdgcn_wave_barrier();
        u64 rk[R];
        sort_popped_list<R>(rk, s_res, npop, lane);
        // npop >= 1: walk_lat_applicable refuses ef == 0, and with ef >= 1 the first round pops the start node
        write_level_list<R>(rk, npop < wa.keep ? npop : wa.keep, ix, lv, wa, qi, out_slot, lane);
        if (level > 0) { // descend through the best hit's child link (vector_store.rs:382-385)
            const u32 best = (u32)readlane_u64(rk[0], 0);
            entry = lv.child[best];
        }
    }

    if (warm == 0x9E3779B9u && wa.keep == 0xFFFFFFFFu) wa.out_status[qi] = (int32_t)warm; // keep is 100 / 64: never true, but not provably — keeps the warm-up loads alive
    if (lane == 0) {
        wa.out_status[qi] = status;
        write_walk_stats(wa.out_stats, qi, n_evals, n_exp, adj_bytes, n_rounds);
    }
}

size_t walk_lat_smem_bytes(const IndexDev &ix, u32 ef) {
    return (size_t)LAL * 64 * 8 * 2 + (size_t)ef * 8 + (size_t)walk_mmax(ix) * 8 + 16;
}

template <int ENG, int CH>
hipError_t launch_lat_r(const IndexDev &ix, const WalkArgs &wa, u32 la, hipStream_t st) {
    const size_t smem = walk_lat_smem_bytes(ix, wa.ef);
    dim3 grid(wa.B), block(64);
    const bool warm = tune_or(TUNE_WALK_LAT_WARM, 1) != 0; // experiments: 0 = off
    if (warm) {
        if (wa.ef <= 64) hipLaunchKernelGGL((walk_lat_kernel<ENG, CH, 1, true>), grid, block, smem, st, ix, wa, la);
        else hipLaunchKernelGGL((walk_lat_kernel<ENG, CH, 4, true>), grid, block, smem, st, ix, wa, la);
    } else {
        if (wa.ef <= 64) hipLaunchKernelGGL((walk_lat_kernel<ENG, CH, 1, false>), grid, block, smem, st, ix, wa, la);
        else hipLaunchKernelGGL((walk_lat_kernel<ENG, CH, 4, false>), grid, block, smem, st, ix, wa, la);
    }
    return hipGetLastError();
}

template <int ENG>
hipError_t launch_lat_ch(const IndexDev &ix, const WalkArgs &wa, u32 ch, u32 la, hipStream_t st) {
    switch (ch) {
    case 1: return launch_lat_r<ENG, 1>(ix, wa, la, st);
    case 2: return launch_lat_r<ENG, 2>(ix, wa, la, st);
    case 3: return launch_lat_r<ENG, 3>(ix, wa, la, st);
    case 4: return launch_lat_r<ENG, 4>(ix, wa, la, st);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

namespace cosdev {

hipError_t launch_walk_lat(int eng, const IndexDev &ix, const WalkArgs &wa, hipStream_t st) {
    // window size: 4 (profiles/archive/r02_latency_walk_sweep_first_version_window4_vs_8.jsonl: an 8-entry window needs 24 % fewer rounds but only 3.9
    // of its 8 entries are consumed before it goes stale, and the wasted evaluations cost more issue time than the rounds save; the
    // kernel has been unrolled for at most LAL = 4 since); tuning knob walk_lat_la = 1..4 narrows it per launch (experiments)
    const u32 la_env = (u32)std::max<long long>(0, tune_or(TUNE_WALK_LAT_LA, 0));
    u32 la = la_env ? la_env : 4u;
    if (la > (u32)LAL) la = LAL;
    const u32 ch = (ix.nchunks + GL - 1) / GL;
    if (eng == ENG_U8) return launch_lat_ch<ENG_U8>(ix, wa, ch, la, st);
    if (eng == ENG_Q2) return launch_lat_ch<ENG_Q2>(ix, wa, ch, la, st);
    return hipErrorInvalidValue;
}

} // namespace cosdev
