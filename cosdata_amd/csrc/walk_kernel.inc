// walk_kernel.inc — the HNSW walk kernel (ann_search / traverse_find_nearest, vector_store.rs:256-402, 1112-1204), textually included
// by kernels_walk.hip; the rules it shares with the other walk kernels are in walk_common.h.
// The row level directly under the level table reads table columns for the neighbours that have a node one level up (LevelDev::adj_up,
// `UPT` below): u8 codes only — quaternary codes walk that level as they did, every winner from its code row.
//
// kernels_walk_pair.hip includes this text a second time with WALK_PAIR defined: the same walk as walk_pair_kernel, a workgroup of TWO
// waves that walk two neighbours of the sorted order (the last range of an ordered launch).  Each wave walks its own query exactly as
// below — own pool, filter, popped list, window; what `PAIR` adds is a small LDS cache of integer dots per query that the PARTNER
// fills: every code row a wave fetches is dotted with both queries, and a winner whose row the partner has already fetched costs one
// LDS read instead of the row.  Everything of it sits under `if constexpr (PAIR)`: walk_kernel's instantiations compile to what they were.
#ifdef WALK_PAIR
#define WALK_KERNEL_NAME walk_pair_kernel
#define WALK_PAIR_PARAM , const WalkPairArgs pa
constexpr bool PAIR = true;
#else
#define WALK_KERNEL_NAME walk_kernel
#define WALK_PAIR_PARAM
constexpr bool PAIR = false;
#endif
constexpr u32 PAIR_HASH = 0x9E3779B1u; // the cache's slot of vector row r: the top WalkPairArgs::cache_bits bits of r * PAIR_HASH
constexpr int PB = 4; // code rows in flight per lane group before the dots are consumed
constexpr int LA = 4; // lookahead window: adjacency rows prefetched per round
// G = 64 path: code rows in flight per wave = template parameter PB64.  An expansion discovers ~7 new neighbours on average:
// with 4 rows in flight that is two dependent HBM round trips per pop, with 8 it is one.  Measured on c2 (profiles/
// r02_c2_launch_shape_sweep_pb8.jsonl): 8 is faster at every launch size (+6 % at ef 64, +2 % at ef 256), so 8 is the default where
// the variant exists and the registers allow it: round 3's evaluation block holds the kernel at 80 VGPRs = 6 waves per SIMD for ef <= 64
// (amdgpu_waves_per_eu below; 7 waves spilled inside the loops and measured 7 % slower — round 6: the headline instantiation, u8 / one
// chunk pass / reference filter, fits 72 VGPRs = 7 waves without scratch and is asked to), 96 = 5 waves up to ef 256, and above that the
// widest pool takes the 4-row variant (walk_pb_policy).

// ------------------------------------------------------------------------------------------------
// walk kernel
// ------------------------------------------------------------------------------------------------
struct WalkSmem {
    u32 *vis;     // visited filter words (REF mode)
    u64 *res;     // popped (key, node) list, ef entries
    u32 *wl_vec;  // winners of the current expansion: vector rows
    u32 *wl_node; //                                     node indices
    u32 *win_vec; // lookahead window: prefetched adjacency rows [LA][64]
    u32 *win_node;
    float *win_mag; // ... and the neighbours' norms where the level has them beside its adjacency (LevelDev::adj_mag)
    float *qf;    // F32 engine: the query vector
};

template <int ENG, int CH, int R, bool G64, bool EXACT, int PB64 = 4>
// (a pair wave's LDS — 10.5 KB with a 512-entry cache — caps the resident waves at 14 per CU: its registers are not what decides, 4 waves per SIMD are asked for)
__global__ __launch_bounds__(PAIR ? 128 : 64) __attribute__((amdgpu_waves_per_eu(PAIR ? 4 : CH >= 3 ? (R <= 4 ? (CH == 3 ? 4 : 3) : (CH == 3 ? 3 : 2)) : (R == 1 ? ((ENG == ENG_U8 && CH == 1 && G64 && !EXACT) ? 7 : 6) : (R <= 4 ? 5 : 4)), 8))) void WALK_KERNEL_NAME(const IndexDev ix, const WalkArgs wa WALK_PAIR_PARAM) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
#ifndef WALK_PAIR
    constexpr WalkPairArgs pa{}; // (never read: every use is under `if constexpr (PAIR)`)
#endif
    const int lane = PAIR ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
    u32 wv = 0; // pair: the wave of the workgroup (wave-uniform, in an SGPR)
    if constexpr (PAIR) wv = uniform_u32(threadIdx.x >> 6);
    const u32 slot = PAIR ? blockIdx.x * 2u + wv : blockIdx.x; // position in the launch's order: a pair's waves take two neighbours
    if (slot >= wa.B) return;
    const u32 qi = wa.q_order ? wa.q_order[slot] : slot; // split walk: locality order (engine_types.h)
    const bool resume = wa.phase != 0u && wa.level_first < ix.num_layers; // a level range below the top: entry node from the range above
    if (resume && wa.out_status[qi] != COS_OK) return;                   // failed in the levels above: nothing below is read
                                                                         // (pair: no barrier anywhere, the partner walks alone)

    const u32 Mmax = wa.smem_mmax; // the widest row among the levels of THIS launch (launch_walk_r)
    WalkSmem sm;
    {
        unsigned char *p = smem_raw;
        if constexpr (PAIR) p += wv * pa.wave_bytes; // every wave of a pair has walk_kernel's layout to itself, its dot cache behind it
        sm.vis = (u32 *)p;      p += (size_t)Mmax * 8;
        sm.res = (u64 *)p;      p += (size_t)wa.ef * 8;
        sm.wl_vec = (u32 *)p;   p += 64 * 4;
        sm.wl_node = (u32 *)p;  p += 64 * 4;
        sm.win_vec = (u32 *)p;  // window region: smem_win_bytes (a launch of table levels only holds just the merge scratch here: win_node / win_mag
        sm.win_node = (u32 *)(p + LA * 64 * 4);  // are then never dereferenced)
        sm.win_mag = (float *)(p + 2 * LA * 64 * 4);
        p += wa.smem_win_bytes;
        p = (unsigned char *)(((size_t)p + 15) & ~(size_t)15);
        sm.qf = (float *)p;
    }

    const u32 qrow = wa.q_rows ? wa.q_rows[qi] : qi;
    const u32 self_id = wa.self_ids ? wa.self_ids[qi] * ix.id_stride : COS_QUERY_ID; // self_ids are vector rows
    const uint8_t *qcode = wa.qcodes + (u64)qrow * ix.row_stride;
    const float qmag = wa.qmags[qrow];
    const u32 N = ix.n;
    const u32 L = ix.num_layers;
    const u32 metric = ix.metric;
    constexpr bool exact = EXACT; // compile-time: the REF kernels carry none of the hash-set code
    // EXACT mode: this query's bitset (one bit per node of the level being walked; all-zero between levels) and the undo log
    // of the words it set, so the filter is cleared by touching only what the level touched (no per-launch memset)
    u32 *vis = exact ? wa.vis_bits + (u64)qi * wa.vis_words_per_query : sm.vis;
    u32 *vlog = exact ? wa.vis_log + (u64)qi * wa.vis_log_cap : nullptr;

    // ---- engine set-up -------------------------------------------------------------------------
    constexpr bool FLOAT_ENG = ENG == ENG_F32 || ENG == ENG_F16; // ordered f32 chains instead of integer chunk dots
    constexpr bool TABLE_OK = ENG == ENG_U8 || ENG == ENG_Q2; // level tables exist for u8 and quaternary codes (walk_operands.hip, cos_ensure_level_table)
    const int G = (ENG == ENG_F32) ? 8 : (ENG == ENG_F16 ? 1 : (int)ix.G); // f32: eight lanes per row, one per accumulator chain
    const int lig = lane & (G - 1);  // lane in group
    const int grp = lane / G;        // group index
    const int RP = 64 / G;           // rows per pass
    uint4 qreg[CH];
    if constexpr (!FLOAT_ENG) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            u32 chunk = (u32)lig + (u32)c * (u32)G;
            qreg[c] = chunk < ix.nchunks ? *(const uint4 *)(qcode + (u64)chunk * 16) : make_uint4(0, 0, 0, 0);
        }
    } else if constexpr (ENG == ENG_F16) {
        const __half *qh = (const __half *)qcode;
        for (u32 i = lane; i < ix.dim; i += 64) sm.qf[i] = __half2float(qh[i]);
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int c = 0; c < CH; c++) qreg[c] = make_uint4(0, 0, 0, 0);
    } else {
        const float *qg = (const float *)qcode;
        for (u32 i = lane; i < (u32)(ix.row_stride / 4); i += 64) sm.qf[i] = qg[i];
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int c = 0; c < CH; c++) qreg[c] = make_uint4(0, 0, 0, 0);
    }

    // G = 64 evaluation block: byte offset of this lane's 16-byte chunk inside a code row, per chunk pass; lanes past the last
    // chunk point at chunk 0 (their query register is zero, so what they read does not matter)
    u32 loff64[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const u32 chunk = (u32)lane + (u32)c * 64u;
        loff64[c] = (chunk < ix.nchunks ? chunk : 0u) * 16u;
    }

    // Pair: the partner's query chunk beside qreg, and the two dot caches — 8-byte entries (vector row << 32 | integer dot), read and
    // written whole, so a tag never pairs with another row's dot.  A wave fills ITS cache with the empty tag before its first probe
    // (LDS arrives uninitialised); an insert of the partner's that the fill wipes is only a lost hit.  Entries never go stale: queries
    // and rows are fixed for the launch and a dot does not depend on the level.
    uint4 qreg2[CH];
    u32 partner = 0; // wave-uniform: the neighbour in the order exists (odd B: the last wave has none)
    u64 *cache_mine = nullptr, *cache_partner = nullptr;
    u32 cache_shift = 0;
    u64 n_hits = 0, n_rows = 0; // winners served by the cache / by a fetched code row
    if constexpr (PAIR) {
        static_assert(!PAIR || (!FLOAT_ENG && G64 && !EXACT), "the pair walk exists on the one-row-per-pass path with the reference filter");
        cache_mine = (u64 *)(smem_raw + wv * pa.wave_bytes + pa.cache_off);
        cache_partner = (u64 *)(smem_raw + (wv ^ 1u) * pa.wave_bytes + pa.cache_off);
        cache_shift = 32u - pa.cache_bits;
        for (u32 i = (u32)lane; i < (1u << pa.cache_bits); i += 64u)
            __hip_atomic_store(&cache_mine[i], (u64)ROW_EMPTY << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        partner = (slot ^ 1u) < wa.B ? 1u : 0u;
#pragma unroll
        for (int c = 0; c < CH; c++) qreg2[c] = make_uint4(0, 0, 0, 0);
        if (partner) {
            const u32 qi2 = wa.q_order ? wa.q_order[slot ^ 1u] : (slot ^ 1u);
            const uint8_t *qcode2 = wa.qcodes + (u64)(wa.q_rows ? wa.q_rows[qi2] : qi2) * ix.row_stride;
#pragma unroll
            for (int c = 0; c < CH; c++) {
                const u32 chunk = (u32)lig + (u32)c * (u32)G;
                if (chunk < ix.nchunks) qreg2[c] = *(const uint4 *)(qcode2 + (u64)chunk * 16);
            }
        }
    }

    u64 n_evals = 0, n_exp = 0, adj_bytes = 0, n_rounds = 0, n_tab = 0;
    const u32 merge_min = uniform_u32(wa.merge_min); // table levels: winners from which an expansion takes the ranked merge (0 = never)
    int32_t status = COS_OK;
    u32 entry = uniform_u32(resume ? wa.entry0[qi] : ix.lv[L].root_idx);
    const int level_first = wa.phase ? (int)wa.level_first : (int)L, level_last = wa.phase ? (int)wa.level_last : 0;
    u32 order_key = wa.key_n; // split walk: depth-first position of the best node of level_last

    // distance of ONE row computed by group 0 (entry node); result valid in every lane
    auto single_distance = [&](u32 row, float &sim_out) -> bool {
        float dotf;
        if constexpr (!FLOAT_ENG) {
            dotf = (float)int_row_dot_group0<ENG, CH>(qreg, ix.codes + (u64)row * ix.row_stride, ix.nchunks, lig, grp, G); // integer dot `as f32` (RNE)
        } else if constexpr (ENG == ENG_F16) {
            float d = f16_lane_dot(ix.codes + (u64)row * ix.row_stride, sm.qf, ix.dim);
            dotf = __uint_as_float(readlane_u32(__float_as_uint(d), 0));
        } else {
            float d = f32_oct_dot((const float *)(ix.codes + (u64)row * ix.row_stride), sm.qf, ix.dim, lane & 7);
            dotf = __uint_as_float(readlane_u32(__float_as_uint(d), 0));
        }
        bool bad;
        sim_out = cosine_or_dot(metric, dotf, qmag, uniform_f32(ix.mags[row]), bad);
        return !bad;
    };

    for (int level = level_first; level >= level_last; level--) {
        const LevelDev lv = ix.lv[level];
        const u32 M = lv.M;
        const u32 slots = M < ix.shortlist ? M : ix.shortlist;
        const u32 bitmask = 64u * M - 1u;
        const u32 out_slot = L - (u32)level;
        u32 nlog = 0; // EXACT mode: entries of the undo log (wave-uniform)
        // table level (WalkArgs::tab): this query's row of precomputed similarities, columns of this level
        const bool tab_level = TABLE_OK && wa.tab != nullptr && (u32)level >= wa.tab_level_min;
        const float *tabq = wa.tab + (u64)qi * wa.tab_stride + wa.tab_col0[level];
        const float *tabm = wa.tab_mags + wa.tab_col0[level]; // |v| of the level's nodes, by node index

        // fresh visited filter, pre-seeded with the query / new-node id (vector_store.rs:266-271, :807)
        if (!exact) {
            vis_clear<64>(sm.vis, M, lane);
            if (lane == 0 && wa.no_self_seed == 0u) vis_set_bit(sm.vis, self_id & bitmask);
        }

        Pool<R> pool;
        pool.clear();
        u32 npool = 0, npop = 0;
        u32 res_lo = 0, res_hi = 0; // R == 1: the popped (key, node) list, entry i in lane i

        // start node (vector_store.rs:1144-1148)
        {
            const u32 erow = uniform_u32(lv.node_vec ? lv.node_vec[entry] : entry);
            float s0;
            if (tab_level) { // the table holds the integer dot `as f32`: the same product and quotient as single_distance
                bool bad;
                // (nested table, LevelDev::adj_tab: the start node's column from the level's node -> column array, once per level)
                u32 ecol = entry;
                if constexpr (ENG == ENG_U8 && CH == 1 && R <= 4) {
                    if (lv.adj_tab != nullptr) ecol = uniform_u32(lv.tab_col[entry]);
                }
                s0 = cosine_or_dot(metric, uniform_f32(tabq[ecol]), qmag, uniform_f32(tabm[ecol]), bad);
                if (bad) { status = COS_ERR_CALCULATION; break; }
            } else if (!single_distance(erow, s0)) { status = COS_ERR_CALCULATION; break; }
            if (lane == 0) {
                if (!exact) vis_set_bit(sm.vis, vis_bit_of(erow, N, ix.id_stride, bitmask));
                else {
                    atomicOr(&vis[entry >> 5], 1u << (entry & 31));
                    vlog[0] = entry >> 5;
                }
            }
            pool.insert_at(pack_key(metric_key(metric, s0), entry), 0, lane);
            npool = 1;
            if (exact) nlog = 1;
        }

        u32 failed = 0; // wave-uniform flags are u32 and lane sets u64 ballots: a bool that crosses a branch is kept as a lane mask
                        // and merged with exec-mask arithmetic at every join, a bool that is voted on is first turned into 0 / 1
        u32 lev_evals = 1; // distance evaluations of this level, the entry node's included
        const u32 log2M = (u32)__ffs((int)M) - 1u; // M is a power of two (cos_params)
        const u64 slotmask = slots >= 64u ? ~0ull : ((1ull << slots) - 1ull); // lanes that hold a scanned slot
        // Lookahead window: the adjacency rows of the next LA pool entries are fetched together (independent
        // loads, one latency); entry i+1 of the window is consumed only while it is still provably the next pop,
        // i.e. while no candidate has been inserted ahead of it.  Most pops of a walk discover nothing new
        // (3-4 evaluations per pop on average), so this collapses chains of dependent HBM round trips.
        // The rounds of a level, compiled TWICE: for a table level (no row is ever fetched: the evaluation blocks are not in its
        // instruction stream) and for a row level (no table gather) — `tab_level` is uniform for the level, the branch is taken once.
        // ... and a row level a THIRD time where it is the level directly under the table and has LevelDev::adj_up (UPT): u8 codes on the
        // one-row-per-pass path, every CH, both filters, both metrics.  Quaternary codes keep the AMAG variant.  The variant is taken once
        // per level, so every other level runs the instruction stream it ran before.
        // ... and a table level a second time where the launch reads the NESTED table (LevelDev::adj_tab, `NEST`): u8 codes only.  The window
        // loads adj_tab where it loaded adj_node, and an expansion splits the word into node and column; everything after the gather is the
        // same code.  Taken once per level, like UPT.
        auto level_rounds = [&](auto tabc, auto cosc, auto amagc, auto upc, auto nestc) __attribute__((always_inline)) {
        constexpr bool TAB = decltype(tabc)::value;
        constexpr bool NEST = decltype(nestc)::value && TAB && ENG == ENG_U8 && CH == 1 && R <= 4; // nb_node arrives as node | column << tab_bits
        const u32 nest_bits = NEST ? lv.tab_bits : 0u;
        constexpr bool COSINE = decltype(cosc)::value;       // table levels of a cosine index: the metric tests fold away
        constexpr bool AMAG = decltype(amagc)::value && G64 && !FLOAT_ENG; // row levels, one-row-per-pass path: norms beside the adjacency
        constexpr bool UPT = decltype(upc)::value && AMAG && !TAB && ENG == ENG_U8; // ... and table columns for the neighbours with a node one level up
        const u32 metric_t = COSINE ? 0u : metric;
        // The level under the table stages FOUR values per slot (row, node, norm, node one level up) for a window of LA - 1 entries in the
        // LDS the other row levels use for three values of LA entries: 4 x 3 = 3 x 4 arrays of 64 words.  A fourth array of LA entries
        // is 1 KB more per wave, and LDS is what caps the resident waves of the flagship's lower range (6.5 KB per wave at M0 256, ef 112:
        // 24 waves per CU; 7.5 KB: 21) — on all its levels, for the sake of one.  A shorter window changes when adjacency rows are
        // fetched, never what is popped (tests/test_commit_equivalence.py runs the model at windows of 1, 4 and 8).
        constexpr int LAW = UPT ? LA - 1 : LA;
        u32 *const w_vec = sm.win_vec, *const w_node = UPT ? sm.win_vec + LAW * 64 : sm.win_node, *const w_up = sm.win_vec + 3 * LAW * 64;
        float *const w_mag = UPT ? (float *)(sm.win_vec + 2 * LAW * 64) : sm.win_mag;
        // the level under the table: this query's table columns of the level ABOVE (level + 1 = tab_level_min <= L)
        const float *tabu = UPT ? wa.tab + (u64)qi * wa.tab_stride + wa.tab_col0[UPT ? level + 1 : 0] : nullptr;
        while (npool > 0 && npop < wa.ef) {
            n_rounds++;
            u32 kwin = npool < (u32)LAW ? npool : (u32)LAW;
            if (kwin > wa.ef - npop) kwin = wa.ef - npop;
            // the window lives in LDS so the consume loop below is a runtime loop (small code, no extra VGPRs)
            // All loads of the window are issued before the first value is looked at, and none is predicated: a pool position past
            // the window holds a real node or the empty key (node 0) — its row is fetched and never looked at; lanes past `slots`
            // read the last slot and are masked when the entry is consumed (slotmask).  Rounds 1-2 wrote `v = load; nn = level == 0
            // ? v : load2; LDS store` inside a per-entry `if`: the generated code waited for every load (s_waitcnt vmcnt(0)) before
            // issuing the next entry's — up to eight DEPENDENT round trips per round where the comment above promised one.
            // A TABLE level keeps the window in registers (round 5): its instruction stream has no row buffers, so the eight registers
            // are free, the consume loop is unrolled over the four entries, and an expansion saves the LDS round trip of reading
            // its entry back (plus the four staging writes of the round).
            u32 wv_[LA], wn_[LA];
            {
                const u32 slot_l = (u32)lane < slots ? (u32)lane : slots - 1u;
                // two copies of the block (level 0 has no node indices of its own): merged into one, the compiler waited for the
                // first group of loads before it issued the second
                auto fetch_stage = [&](auto bothc) {
                    constexpr bool BOTH = decltype(bothc)::value;
                    float wm_[LA];
                    u32 wu_[LA];
                    static_for<0, LAW>([&](auto ic) {
                        constexpr int i = decltype(ic)::value;
                        const u32 nd = pool.template peek_node<i>();
                        const u64 off = ((u64)nd << log2M) + slot_l;
                        wv_[i] = lv.adj_vec[off];
                        if constexpr (BOTH) wn_[i] = NEST ? lv.adj_tab[off] : lv.adj_node[off];
                        if constexpr (!TAB && AMAG && !UPT) wm_[i] = lv.adj_mag[(u64)nd * lv.mag_stride + slot_l]; // (slot_l < slots = mag_stride)
                        if constexpr (UPT) { // norm and node one level up in ONE 8-byte load through ONE pointer (LevelDev::adj_up says why)
                            const uint2 mu = ((const uint2 *)lv.adj_up)[(u64)nd * lv.mag_stride + slot_l];
                            wm_[i] = __uint_as_float(mu.x);
                            wu_[i] = mu.y;
                        }
                    });
                    if constexpr (!TAB) {
                        static_for<0, LAW>([&](auto ic) {
                            constexpr int i = decltype(ic)::value;
                            w_vec[i * 64 + lane] = wv_[i];
                            w_node[i * 64 + lane] = BOTH ? wn_[i] : wv_[i];
                            if constexpr (AMAG) w_mag[i * 64 + lane] = wm_[i];
                            if constexpr (UPT) w_up[i * 64 + lane] = wu_[i];
                        });
                    }
                };
                if (TAB || level != 0) fetch_stage(std::true_type{}); // (a table level is never level 0)
                else fetch_stage(std::false_type{});
            }
            u32 stop = 0; // wave-uniform: the window went stale or the level failed
            auto consume = [&](u32 wi, u32 nb_vec, u32 nb_node, float nb_mag, u32 nb_up) __attribute__((always_inline)) {
                // the window entry being consumed IS the pool's head (that is what "still provably the next pop" means): the
                // popped list takes it from lane 0's register — until round 4 the window's keys made a detour through LDS
                if constexpr (R == 1) { // ef <= 64: the popped list is one entry per lane, lane npop takes the head by v_writelane
                    const u64 hd = pool.head();
                    res_lo = writelane_dyn(res_lo, (u32)hd, (int)npop);
                    res_hi = writelane_dyn(res_hi, (u32)(hd >> 32), (int)npop);
                } else if (lane == 0) sm.res[npop] = pool.e[0];
                pool.pop_head(lane);
                npool--;
                npop++;
                const int limit = (int)wa.ef - (int)npop; // future pops still allowed
                const int ahead = (int)kwin - 1 - (int)wi; // window entries still waiting at pool positions 0..ahead-1
                u32 window_ok = 1;
                // nested table: the word is node | column << nest_bits.  The exact filter needs the node now; the reference filter tests
                // the vector row, so there the word stays ONE register through the filter: the column leaves it for the two gathers and
                // dies, then the node replaces it.
                const u32 nb_word = nb_node;
                if constexpr (NEST && EXACT) nb_node = nb_word & ((1u << nest_bits) - 1u);

                // neighbour slots in slot order, one per lane (vector_store.rs:1161-1171): nb_vec / nb_node
                const u64 vmask = ballot64(nb_vec != ROW_EMPTY) & slotmask;
                u64 wmask; // the expansion's winners: unvisited neighbours, as a lane set
                if (!exact) {
                    u32 bit = vis_bit_of(nb_vec, N, 1u, bitmask);
                    if (ix.id_stride != 1u) { // wave-uniform branch (the empty asm keeps it one): v_mul_lo_u32 is a quarter-rate instruction
                        asm volatile("");
                        bit = vis_bit_of(nb_vec, N, ix.id_stride, bitmask);
                    }
                    const u32 word = bit >> 5, msk = 1u << (bit & 31);
                    u32 seen = sm.vis[word]; // unpredicated (an empty slot's word is in range too); the asm keeps the load out of an `if (valid)`
                    asm volatile("" : "+v"(seen));
                    const u64 cmask = vmask & ballot64((seen & msk) == 0u);
                    wmask = cmask; // (nothing new: the next window entry is certainly the next pop)
                    if (cmask) {
                    u32 old = 0;
                    if (__builtin_amdgcn_inverse_ballot_w64(cmask)) old = atomicOr(&sm.vis[word], msk);
                    wmask = vis_alias_winners(cmask, bit, cmask & ballot64((old & msk) != 0u));
                    }
                } else {
                    u32 w = 0;
                    if (__builtin_amdgcn_inverse_ballot_w64(vmask)) w = __hip_atomic_load(&vis[nb_node >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    wmask = vmask & ballot64(((w >> (nb_node & 31)) & 1u) == 0u);
                    if (__builtin_amdgcn_inverse_ballot_w64(wmask)) {
                        atomicOr(&vis[nb_node >> 5], 1u << (nb_node & 31));                          // fire and forget
                        vlog[nlog + (u32)__popcll(wmask & ((1ull << lane) - 1ull))] = nb_node >> 5;  // undo log, in slot order
                    }
                    nlog += (u32)__popcll(wmask);
                }
                if (wmask) { // an expansion that discovers nothing costs nothing more
                const bool win = __builtin_amdgcn_inverse_ballot_w64(wmask);
                const int W = __popcll(wmask);
                lev_evals += (u32)W;
                // Winners whose similarity sits in a lane of `leadmask`, key and node index beside it, go into the pool in lane = slot
                // order.  One vector compare first screens them against the entry that closes the poppable part of the pool
                // (position limit - 1): a key below it has at least `limit` entries above it, the loop would rank it only to
                // reject it.  The bar can only rise while winners go in, so the screen is conservative and the loop's own test stays.
                auto insert_serial = [&](u64 pm, u32 keyv, u32 nodev) { // pm: the winners that passed the screen
                    while (pm) {
                        const int p = __ffsll((long long)pm) - 1;
                        pm = clear_bit_u64(pm, p);
                        const u64 kk = pack_key(readlane_u32(keyv, p), readlane_u32(nodev, p));
                        const int pos = pool.rank_of(kk);
                        if (pos < limit) {
                            pool.insert_at(kk, pos, lane);
                            npool = npool + 1u < (u32)(64 * R) ? npool + 1u : (u32)(64 * R);
                            window_ok = pos < ahead ? 0u : window_ok;
                        }
                    }
                };
                auto commit = [&](u64 leadmask, u32 keyv, u32 nodev) {
                    const u64 bar = limit > 0 ? pool.peek_dyn((u32)(limit - 1)) : ~0ull;
                    insert_serial(leadmask & ballot64(pack_key(keyv, nodev) > bar), keyv, nodev);
                };
                // Ranked merge (round 6; table levels, pools of up to 256 keys): the serial insert above costs one rank + one pool shift
                // per winner (R = 4: ~45 wave-instructions each, and a table level of the metric's shard — M 64, ef 128 — finds a dozen
                // winners per expansion).  Here every winner that passes the screen is ranked against the pool AND against the other
                // winners with one broadcast + R + 1 compares, the same compares count for every pool entry the winners below it, and
                // pool and winners then move to their final positions in ONE permutation through LDS (the lookahead window's LDS: a
                // table level keeps its window in registers).  Same pool afterwards as the serial loop leaves in the positions that can
                // still be popped (< limit): a winner the loop would refuse (rank >= limit) lands behind them, where nothing is ever
                // popped from; `npool` may count such entries, the window never reaches them (kwin <= limit).  window_ok: a winner
                // lands ahead of a waiting window entry iff fewer than `ahead` POOL entries beat it (the first such winner in slot order has
                // only smaller winners before it, so the serial loop sees the same rank).
                auto commit_merge = [&](u64 leadmask, u32 keyv, u32 nodev) {
                    const u64 bar = limit > 0 ? pool.peek_dyn((u32)(limit - 1)) : ~0ull;
                    const u64 mykey = pack_key(keyv, nodev);
                    const u64 pm = leadmask & ballot64(mykey > bar);
                    const u32 Wp = (u32)__popcll(pm);
                    if (Wp < merge_min) { insert_serial(pm, keyv, nodev); return; }
                    u32 below[R]; // per pool entry: the winners below it
#pragma unroll
                    for (int r = 0; r < R; r++) below[r] = 0u;
                    u32 posv = 0u;   // winners' lanes: pool entries above the winner ...
                    u32 abovev = 0u; // ... and winners above it: posv + abovev = its place in the merged order
                    u32 minrank = ~0u;
                    u64 m = pm;
                    while (m) {
                        const int p = __ffsll((long long)m) - 1;
                        m = clear_bit_u64(m, p);
                        const u64 kk = pack_key(readlane_u32(keyv, p), readlane_u32(nodev, p));
                        u32 rank = 0;
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            const bool gt = pool.e[r] > kk;
                            rank += (u32)__popcll(ballot64(gt));
                            below[r] += gt ? 1u : 0u;
                        }
                        minrank = rank < minrank ? rank : minrank;
                        abovev += kk > mykey ? 1u : 0u; // (lanes outside pm count garbage: never used)
                        posv = writelane_dyn(posv, rank, p);
                    }
                    window_ok = (int)minrank < ahead ? 0u : window_ok;
                    // the permutation: a key whose place is past the pool's end goes to the spare slot behind it (LDS the integer
                    // engines do not use: walk_smem_bytes' 16 bytes of slack) instead of being predicated off
                    u64 *mg = (u64 *)sm.win_vec; // 64 * R keys (R <= 4: the 2 KB of win_vec + win_node)
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        u32 np = (u32)lane * R + r + (Wp - below[r]);
                        np = np < (u32)(64 * R) ? np : (u32)(64 * R);
                        mg[np] = pool.e[r];
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(pm)) {
                        u32 np = posv + abovev;
                        np = np < (u32)(64 * R) ? np : (u32)(64 * R);
                        mg[np] = mykey;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int r = 0; r < R; r++) pool.e[r] = mg[(u32)lane * R + r];
                    npool = npool + Wp < (u32)(64 * R) ? npool + Wp : (u32)(64 * R);
                };
                if constexpr (TAB) {
                    // Table level: the integer dot of (query, node) was computed ahead of the walk for every node of the level
                    // (launch_level_table: exact on the i8 MFMA, converted like `as f32`), so an expansion's winners cost two
                    // 4-byte gathers issued together (the dot; the node's norm from a few KB that stay in L2) and ONE vector
                    // quotient — the product and the division of the row levels (cosine.rs:223-235) — and no code row is
                    // fetched or dotted.
                    float simv = 0.0f, magv = 1.0f;
                    if constexpr (NEST) {
                        const u32 nb_col = nb_word >> nest_bits;
                        if (win) { simv = tabq[nb_col]; magv = tabm[nb_col]; }
                        if constexpr (!EXACT) nb_node = nb_word & ((1u << nest_bits) - 1u);
                    } else if (win) { simv = tabq[nb_node]; magv = tabm[nb_node]; }
                    bool badl;
                    // u8 codes: both norms are roots of integer sums (>= 1 when not 0): the quotient needs no scaling
                    simv = cosine_or_dot<ENG == ENG_U8>(metric_t, simv, qmag, magv, badl);
                    if (wmask & ballot64(badl)) failed = 1;
                    else if constexpr (R <= 4) {
                        if (merge_min != 0u) commit_merge(wmask, metric_key(metric_t, simv), nb_node);
                        else commit(wmask, metric_key(metric_t, simv), nb_node);
                    } else commit(wmask, metric_key(metric_t, simv), nb_node);
                } else if constexpr (G64 && !FLOAT_ENG) {
                    // One code row per wave pass (64 lanes x 16 B cover the row): the winner's row index is wave-uniform, so it
                    // is taken straight from the owning lane with v_readlane and the row base lives in SGPRs (the load is the
                    // saddr + 32-bit lane offset form: no vector address arithmetic).  PB64 rows are in flight before the dots;
                    // their PB64 dot vectors are summed TOGETHER (wave_reduce_rows: 18 VALU for 8 rows), row p of the block
                    // landing in the lanes of group p — until late in round 3 the block reduced row by row (4 dependent DPP adds + 4 v_readlane + a
                    // select per row) and fetched |v| and the node index with one predicated scalar-indexed load per row: 24 VALU
                    // and 32 SALU per evaluation of the 38 + 36 the whole walk spent (profiles/archive/r03_mid_round_pmc_sq_instruction_mix_rocprofv3.txt).
                    // Lanes past the row's last chunk re-read chunk 0 against a zero query register instead of being masked off.
                    float magw = 1.0f; // |v| of every winner of the expansion, in the winner's own lane: it came with the adjacency
                                       // row (LevelDev::adj_mag), or one vector gather from mags[]
                    if constexpr (AMAG) magw = nb_mag;
                    else if (win) magw = ix.mags[nb_vec];
                    u64 m = wmask;
                    if constexpr (UPT) {
                        // The level under the table: a winner that has a node one level up (nb_up) was dotted with this query by the
                        // table GEMM — tabu[nb_up] is the integer dot `as f32` the row block below would compute (both are exact) — so
                        // it costs one 4-byte gather instead of a code row; its norm is in the lane already.  These winners (tmask) are
                        // committed BEFORE the row winners (rmask), not in slot order.  That cannot change a result:
                        //   * keys are unique (the node index is the low word), so pool and winners have one descending order;
                        //   * the entries that can still be popped afterwards are the top `limit` of pool + winners whatever the order
                        //     of insertion (insert_serial refuses exactly the keys with `limit` larger ones before them, and an entry
                        //     pushed past position limit - 1 by a later insert is one the other order would have refused or pushed too);
                        //   * window_ok falls iff SOME winner is inserted with fewer than `ahead` entries above it at that moment; the
                        //     LARGEST winner has only pool entries above it whenever it goes in (every other winner is below it), and no
                        //     winner can have fewer entries above it than the largest has pool entries above it — so the flag falls iff
                        //     fewer than `ahead` POOL entries beat the largest winner, in any order (commit_merge relies on the same).
                        // tests/test_walk_up_table_model.py checks the three on the pool model of tests/test_commit_equivalence.py.
                        const u64 tmask = wmask & ballot64(nb_up != ADJ_UP_NONE);
                        if (tmask) {
                            float dotv = 0.0f;
                            if (__builtin_amdgcn_inverse_ballot_w64(tmask)) dotv = tabu[nb_up];
                            bool badl;
                            const float sim = cosine_or_dot<ENG == ENG_U8>(metric, dotv, qmag, magw, badl);
                            if (tmask & ballot64(badl)) failed = 1;
                            else commit(tmask, metric_key(metric, sim), nb_node);
                            n_tab += (u64)__popcll(tmask);
                            m = wmask & ~tmask;
                        }
                    }
                    if constexpr (PAIR) {
                        // Pair: every winner left reads ITS cache at its row's slot.  A hit is the integer dot the partner computed from
                        // the same row and this query's chunk — `(float)` of it is the value the row block below would form — so the hits
                        // (hmask) are committed like tmask above, before the row winners: table winners, cache hits, rows.  The three
                        // points of the comment above hold for any split of an expansion's winners into groups committed one after the
                        // other (tests/test_walk_pair_model.py).
                        if (m && !failed) {
                            u64 ent = 0;
                            if (__builtin_amdgcn_inverse_ballot_w64(m))
                                ent = __hip_atomic_load(&cache_mine[(nb_vec * PAIR_HASH) >> cache_shift], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            const u64 hmask = m & ballot64((u32)(ent >> 32) == nb_vec);
                            if (hmask) {
                                const float dotv = (float)(u32)ent;
                                bool badl;
                                const float sim = cosine_or_dot<ENG == ENG_U8>(metric, dotv, qmag, magw, badl);
                                if (hmask & ballot64(badl)) failed = 1;
                                else commit(hmask, metric_key(metric, sim), nb_node);
                                n_hits += (u64)__popcll(hmask);
                                m &= ~hmask;
                            }
                        }
                        if (!failed) n_rows += (u64)__popcll(m);
                    }
                    while (m && !failed) {
                        u32 lsel = 0;  // landing lane of winner p of this block <- 4 * (the lane that owns the winner): a ds_bpermute address
                        u32 tot = 0;   // landing lanes: the winner's integer dot
                        u32 tot2 = 0;  // pair: the PARTNER's integer dot with the same row
                        u64 leadmask = 0; // first lane of the landing group of every winner of this block
                        // A block of up to NP winners, row p landing in lanes p*(64/NP)...: the rows are fetched together, dotted,
                        // and the NP partial-sum vectors reduced at once.  The dots of rows a short block does not have are
                        // skipped by real branches (the empty asm keeps the compiler from turning them into 5 VALU + a select each).
                        auto eval_block = [&](auto npc) {
                            constexpr int NP = decltype(npc)::value;
                            constexpr int LS = 64 / NP;
                            uint4 buf[NP][CH];
                            int cnt = 0;
                            static_for<0, NP>([&](auto pc) {
                                constexpr int p = decltype(pc)::value;
                                if (m) {
                                    const int l = __ffsll((long long)m) - 1;
                                    m = clear_bit_u64(m, l);
                                    const uint8_t *rp = row_ptr_scalar(ix.codes, readlane_u32(nb_vec, l), (u32)ix.row_stride);
                                    lsel = writelane_u32<p * LS>(lsel, (u32)l << 2);
#pragma unroll
                                    for (int c = 0; c < CH; c++) {
                                        u32 lo = loff64[c];
                                        asm("" : "+v"(lo)); // keeps the zero-extension in this block: saddr + 32-bit voffset addressing
                                        buf[p][c] = *(const uint4 *)(rp + lo);
                                    }
                                    cnt++;
                                }
                            });
                            u32 acc[NP];
                            static_for<0, NP>([&](auto pc) {
                                constexpr int p = decltype(pc)::value;
                                acc[p] = 0;
                                if (p < cnt) {
                                    asm volatile("");
#pragma unroll
                                    for (int c = 0; c < CH; c++) acc[p] = chunk_dot<ENG>(qreg[c], buf[p][c], acc[p]);
                                }
                            });
                            tot = wave_reduce_rows<NP>(acc);
                            if constexpr (PAIR) {
                                if (partner) { // the rows are in registers: the partner's dots cost the v_dot4 and one more reduce (the range is bound by the fabric)
                                    u32 acc2[NP];
                                    static_for<0, NP>([&](auto pc) {
                                        constexpr int p = decltype(pc)::value;
                                        acc2[p] = 0;
                                        if (p < cnt) {
                                            asm volatile("");
#pragma unroll
                                            for (int c = 0; c < CH; c++) acc2[p] = chunk_dot<ENG>(qreg2[c], buf[p][c], acc2[p]);
                                        }
                                    });
                                    tot2 = wave_reduce_rows<NP>(acc2);
                                }
                            }
                            constexpr u64 firsts = NP == 8 ? 0x0101010101010101ull : 0x0001000100010001ull;
                            leadmask = cnt == NP ? firsts : firsts & ((1ull << (cnt * LS)) - 1ull);
                        };
                        if constexpr (PB64 == 8) {
                            if (__popcll(m) > 4) eval_block(std::integral_constant<int, 8>{});
                            else eval_block(std::integral_constant<int, 4>{});
                        } else {
                            eval_block(std::integral_constant<int, 4>{});
                        }
                        // |v| and node index of the block's winners move to the landing lanes (two ds_bpermute)
                        const float magv = __uint_as_float((u32)__builtin_amdgcn_ds_bpermute((int)lsel, (int)__float_as_uint(magw)));
                        const u32 nodev = (u32)__builtin_amdgcn_ds_bpermute((int)lsel, (int)nb_node);
                        if constexpr (PAIR) {
                            if (partner) { // the row's id comes to the landing lane too, and (row, partner's dot) goes into the partner's cache
                                const u32 rowv = (u32)__builtin_amdgcn_ds_bpermute((int)lsel, (int)nb_vec);
                                if (__builtin_amdgcn_inverse_ballot_w64(leadmask))
                                    __hip_atomic_store(&cache_partner[(rowv * PAIR_HASH) >> cache_shift], ((u64)rowv << 32) | (u64)tot2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                        const float dotv = (float)tot; // integer dot `as f32` (RNE)
                        // one vector epilogue for the whole block
                        bool badl;
                        const float sim = cosine_or_dot<ENG == ENG_U8>(metric, dotv, qmag, magv, badl);
                        if (leadmask & ballot64(badl)) { failed = 1; break; }
                        commit(leadmask, metric_key(metric, sim), nodev);
                    }
                } else {
                // compact winners (slot order) into LDS
                if (win) {
                    const int rank = __popcll(wmask & ((1ull << lane) - 1ull));
                    sm.wl_vec[rank] = nb_vec;
                    sm.wl_node[rank] = nb_node;
                }

                // evaluate winners: RP rows per pass, PB passes in flight
                for (int base = 0; base < W; base += RP * PB) {
                    u32 prow[PB];
                    float pmag[PB];
                    uint4 buf[PB][CH];
                    float fdot[PB];
#pragma unroll
                    for (int p = 0; p < PB; p++) {
                        if (base + p * RP >= W) break; // wave-uniform
                        const int my = base + p * RP + grp;
                        const bool v = my < W;
                        prow[p] = v ? sm.wl_vec[my] : 0u;
                        pmag[p] = 1.0f;
                        if (v) pmag[p] = ix.mags[prow[p]];
                        if constexpr (!FLOAT_ENG) {
#pragma unroll
                            for (int c = 0; c < CH; c++) {
                                u32 chunk = (u32)lig + (u32)c * (u32)G;
                                buf[p][c] = make_uint4(0, 0, 0, 0);
                                if (v && chunk < ix.nchunks) buf[p][c] = *(const uint4 *)(ix.codes + (u64)prow[p] * ix.row_stride + (u64)chunk * 16);
                            }
                        }
                    }
                    if constexpr (FLOAT_ENG) {
                        // every lane group runs the uniform-trip-count dot; groups without a winner read row 0 and are ignored
#pragma unroll
                        for (int p = 0; p < PB; p++) {
                            if (base + p * RP >= W) break;
                            if constexpr (ENG == ENG_F32)
                                fdot[p] = f32_oct_dot((const float *)(ix.codes + (u64)prow[p] * ix.row_stride), sm.qf, ix.dim, lane & 7);
                            else
                                fdot[p] = f16_lane_dot(ix.codes + (u64)prow[p] * ix.row_stride, sm.qf, ix.dim);
                        }
                    }
#pragma unroll
                    for (int p = 0; p < PB; p++) {
                        if (base + p * RP >= W) break; // wave-uniform
                        float dotf;
                        if constexpr (!FLOAT_ENG) {
                            u32 acc = 0;
#pragma unroll
                            for (int c = 0; c < CH; c++) acc = chunk_dot<ENG>(qreg[c], buf[p][c], acc);
                            acc = group_reduce_add_u32(acc, G);
                            dotf = (float)acc;
                        } else {
                            dotf = fdot[p];
                        }
                        // this pass's rows in winner order: the first lane of every group holds its row's key
                        const int mine = base + p * RP + grp;
                        const bool leadg = lig == 0 && mine < W;
                        bool badl;
                        const float sim = cosine_or_dot(metric, dotf, qmag, pmag[p], badl);
                        if (ballot64(mine < W && badl)) { failed = 1; break; }
                        const u32 mynode = leadg ? sm.wl_node[mine] : 0u;
                        commit(ballot64(leadg), metric_key(metric, sim), mynode);
                    }
                    if (failed) break;
                }
                }
                stop = failed | (window_ok ^ 1u);
                }
            };
            if constexpr (TAB) {
                static_for<0, LA>([&](auto ic) __attribute__((always_inline)) {
                    constexpr int i = decltype(ic)::value;
                    if ((u32)i < kwin && !stop) consume((u32)i, wv_[i], wn_[i], 1.0f, ADJ_UP_NONE);
                });
            } else {
                for (u32 wi = 0; wi < kwin && !stop; wi++)
                    consume(wi, w_vec[wi * 64 + lane], w_node[wi * 64 + lane], AMAG ? w_mag[wi * 64 + lane] : 1.0f, UPT ? w_up[wi * 64 + lane] : ADJ_UP_NONE);
            }
            if (failed) break;
        }
        };
        if (tab_level) {
            bool nest = false;
            // Rows of one chunk pass and pools of up to 256 keys only (WalkPlan::table_nested follows): every further copy of the rounds
            // moves the scalar spills of the kernel around, and in the instantiations of two to four passes that cost a VGPR (96 -> 97 at
            // CH 2, R 8: a wave per SIMD); so it did at R 8 with the exact filter (84 -> 85).  Rows of fewer than 64 chunks take ONE copy
            // for both metrics for the same reason (two copies: 72 -> 73 VGPRs at R 4).
            if constexpr (ENG == ENG_U8 && CH == 1 && R <= 4) {
                if (lv.adj_tab != nullptr) { // the nested table (uniform for the level: the branch is taken once)
                    if (G64 && metric == 0u) level_rounds(std::true_type{}, std::integral_constant<bool, G64>{}, std::false_type{}, std::false_type{}, std::true_type{});
                    else level_rounds(std::true_type{}, std::false_type{}, std::false_type{}, std::false_type{}, std::true_type{});
                    nest = true;
                }
            }
            if (!nest) {
                if (metric == 0u) level_rounds(std::true_type{}, std::true_type{}, std::false_type{}, std::false_type{}, std::false_type{});
                else level_rounds(std::true_type{}, std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{});
            }
        } else {
            bool done = false;
            if constexpr (G64 && !FLOAT_ENG) {
                if (lv.adj_mag != nullptr) { // (uniform for the level: the branch is taken once)
                    bool up = false;
                    if constexpr (ENG == ENG_U8) {
                        if (lv.adj_up != nullptr && wa.tab != nullptr && (u32)level + 1u == wa.tab_level_min) { // the level under the table
                            level_rounds(std::false_type{}, std::false_type{}, std::true_type{}, std::true_type{}, std::false_type{});
                            up = true;
                        }
                    }
                    if (!up) level_rounds(std::false_type{}, std::false_type{}, std::true_type{}, std::false_type{}, std::false_type{});
                    done = true;
                }
            }
            if (!done) level_rounds(std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{});
        }
        n_exp += npop;
        adj_bytes += (u64)npop * slots * 4; // what an expansion reads: the scanned slots of the row (min(M, shortlist_size))
        n_evals += lev_evals;
        if (tab_level) n_tab += lev_evals; // (the level under the table has added its table winners itself)
        if (exact) {
            // undo: zero exactly the words this level set (whole words belong to this query), leaving the bitset all-zero
            // for the next level / launch.  One wave owns the filter and its vector-memory operations reach L2 in issue
            // order, so waiting for the outstanding ones (no cache write-back fence) orders set -> clear -> next test.
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_s_waitcnt(0);
            for (u32 i = lane; i < nlog; i += 64) {
                const u32 w = __hip_atomic_load(&vlog[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&vis[w], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_s_waitcnt(0);
        }
        if (failed) { status = COS_ERR_CALCULATION; break; }

        // keep the best `keep`, sorted descending (vector_store.rs:1194-1201)
        u64 rk[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const u32 e = (u32)lane * R + r;
            if constexpr (R == 1) rk[r] = e < npop ? pack_key(res_hi, res_lo) : 0ull;
            else rk[r] = e < npop ? sm.res[e] : 0ull;
        }
        bitonic_sort_desc<R>(rk, lane);
        u32 cnt = npop < wa.keep ? npop : wa.keep;
        // npop == 0 only if ef == 0: fall back to the entry node's own distance (vector_store.rs:329-380)
        if (npop == 0) {
            const u32 erow = uniform_u32(lv.node_vec ? lv.node_vec[entry] : entry);
            float s0;
            if (!single_distance(erow, s0)) { status = COS_ERR_CALCULATION; break; }
            rk[0] = lane == 0 ? pack_key(metric_key(metric, s0), entry) : 0ull;
            cnt = 1;
        }
        // write_level_list (walk_common.h), written out: through the helper walk_kernel<ENG_U8, 1, 4, false, false> takes 74 VGPRs
        // instead of 71 and loses its seventh wave per SIMD
        const u64 obase = level_list_base(ix, wa, qi, out_slot);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const u32 e = (u32)lane * R + r;
            if (e < cnt) {
                const u32 nd = (u32)rk[r];
                const u32 vrow = lv.node_vec ? lv.node_vec[nd] : nd;
                wa.out_ids[obase + e] = vrow == N ? COS_ROOT_ID : vrow * ix.id_stride;
                wa.out_sims[obase + e] = metric_key_inv(metric, (u32)(rk[r] >> 32));
                if (wa.out_nodes) wa.out_nodes[obase + e] = nd;
            }
        }
        if (lane == 0) wa.out_counts[(u64)qi * (L + 1) + out_slot] = cnt;
        // descend through the best hit's child link (vector_store.rs:382-385)
        if (level > 0) {
            const u32 best = (u32)readlane_u64(rk[0], 0);
            entry = uniform_u32(lv.child[best]);
            if (wa.phase != 0u && level == level_last) order_key = uniform_u32(wa.order_rank[best]);
        }
    }

    if (lane == 0) {
        wa.out_status[qi] = status;
        if (wa.phase != 0u && level_last > 0) {
            wa.entry0[qi] = entry;
            wa.order_key[qi] = status == COS_OK ? order_key : wa.key_n;
            wa.order_iota[qi] = qi;
        }
        if (wa.out_stats) {
            const bool add = resume; // the counters of the levels above are already there
            wa.out_stats[(u64)qi * 4 + 0] = n_evals + (add ? wa.out_stats[(u64)qi * 4 + 0] : 0ull);
            wa.out_stats[(u64)qi * 4 + 1] = n_exp + (add ? wa.out_stats[(u64)qi * 4 + 1] : 0ull);
            wa.out_stats[(u64)qi * 4 + 2] = adj_bytes + (add ? wa.out_stats[(u64)qi * 4 + 2] : 0ull);
            wa.out_stats[(u64)qi * 4 + 3] = n_rounds + (add ? wa.out_stats[(u64)qi * 4 + 3] : 0ull);
        }
        if (wa.out_stats2) { // the split of a launch's counters the roofline report wants: the last level range on its own, table evaluations
            if (resume || wa.phase == 0u) {
                wa.out_stats2[(u64)qi * 4 + 0] = n_evals;
                wa.out_stats2[(u64)qi * 4 + 1] = n_exp;
                wa.out_stats2[(u64)qi * 4 + 2] = adj_bytes;
            }
            wa.out_stats2[(u64)qi * 4 + 3] = n_tab + (resume ? wa.out_stats2[(u64)qi * 4 + 3] : 0ull);
        }
        if constexpr (PAIR) {
            if (pa.out_pair) {
                pa.out_pair[(u64)qi * 2 + 0] = n_hits;
                pa.out_pair[(u64)qi * 2 + 1] = n_rows;
            }
        }
    }
}
