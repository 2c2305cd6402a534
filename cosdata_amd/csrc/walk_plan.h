// walk_plan.h — the launch policy of a dense HNSW walk, decided once: which kernel walks, whether the walk is split and locality-ordered,
// whether the level-table GEMM runs (and what it waits for), which levels read norms beside the adjacency, which stream and chain the
// walk joins, and what has to be prepared for all that.  Plain integer logic: no HIP, no handle, no global — every knob arrives resolved
// in WalkPlanIn, so the rules can be checked on a CPU (tests/cxx/walk_plan_check.cpp against tests/golden/walk_plan_cases.txt).
// engine.hip plans in get_workspace (cos_walk_plan_in, walk_operands.hip, fills the inputs), prepares what the plan wants, settles it against what exists and
// launches from it; builder.hip's walks take their kernel from the same function.
//
// The level-table GEMM of a chained big launch (round 7).  The query-resident GEMM (kernels_scan.hip level_table_areg) is a queue of
// work items — (row group of 256 queries, stripe of column tiles), table_gemm_items() of them — that its workgroups claim from one
// counter, so one table can be computed by several launches.  Where the GEMM is gated behind the previous chained walk
// (table_waits_for_sort) and tuning knob walk_table_early_wgs is not 0, engine.hip issues it as TWO launches over one counter:
//   * an EARLY part of WalkPlan::table_early_wgs workgroups that waits for the previous chained walk's END OF UPPER RANGE
//     (cos_index::chain_upper_ev, recorded between the upper range and the order sort, when the chip is empty for ~60 us);
//   * a LATE part, the full-width grid, that waits for the previous walk's completion (cos_index::chain_ev) and drains what is left of
//     the queue — or reads one word per workgroup and leaves.
// Both go out on the caller's stream, so the late part starts when the early one has left, and the early one leaves when the queue is
// empty: the early part computes the whole table on its few CUs and the late part is an empty launch.  No setting of the knob beat the
// single launch behind chain_last_range_ev on the 12.5M x 1024 shard, so table_early_wgs = 0 is the default; an arrangement in which
// the late part works BESIDE the early one (the early part on a stream of its own) was measured too and is not in the tree
// (profiles/r07_table_early_wgs_sweep.jsonl).
#pragma once
#include <algorithm>
#include <cstdint>

namespace cosdev {

constexpr int WALK_PLAN_MAX_LEVELS = 16;                    // = MAX_LEVELS (device_common.h; engine_internal.h asserts these four)
constexpr int WALK_PLAN_ENG_U8 = 0, WALK_PLAN_ENG_Q2 = 1;   // = ENG_U8, ENG_Q2
constexpr uint32_t WALK_PLAN_FAST_MAX_EF = 1024u;           // = WALK_FAST_MAX_EF (engine_types.h)

// The norms beside the adjacency (LevelDev::adj_mag), invalidated by a root replaced on a live graph, are refilled by the first launch
// of ADJ_MAG_REFILL_MIN_B queries but only read by launches of ADJ_MAG_USE_MIN_B: the two disagree, so a launch in between
// pays for a refill it does not use.
constexpr uint32_t ADJ_MAG_REFILL_MIN_B = 1024u, ADJ_MAG_USE_MIN_B = 4096u;

enum class WalkKernel : uint8_t {
    General,    // walk_general_kernel (kernels_walk_general.hip): every level from rows, one launch, arrival order
    Throughput, // walk_kernel (walk_kernel.inc): one wave per query
    Lat1,       // walk_lat_kernel: one wave per query, small launches
    Lat4        // walk_lat4_kernel: four waves per query, one client batch
};

struct WalkPlanIn {
    // engine and row shape
    int eng;
    uint32_t storage; // COS_STORAGE_* (0 = u8)
    uint32_t nchunks, G;
    // graph shape
    uint32_t num_layers, M[WALK_PLAN_MAX_LEVELS], shortlist, visited_mode, mdim;
    // the launch
    uint32_t B, ef;
    bool chain;        // false: a chunk of a pipelined host call (its chunks co-run)
    bool no_self_seed; // delete_embedding's walks (WalkArgs::no_self_seed)
    // the knobs, resolved
    uint32_t lat_max_B, lat4_max_B; // cos_index_set_latency_mode / _waves after the walk_lat / walk_lat4 overrides (0 = never)
    bool small_table_tk;            // tuning knob walk_small_table_tk
    uint32_t adj_mag_mode;          // tuning knob walk_adj_mag: 0 never | 1 by the rule below | 2 at every ef and launch size
    uint32_t table_min_B;           // cos_index_set_walk_table's min_queries after its override (0 = no table)
    uint32_t order_min_B, chain_min_B, side_min_B;
    long long table_after_sort;     // tuning knob walk_table_after_sort: 0 never | 1 tables of 2^30 entries or more | 2 always
    // what exists before anything is prepared
    bool table_supported;           // the engine has a level table at all (level_table_eng_supported)
    bool adj_mag_valid;             // WalkOperands::have_adj_mag() (engine.hip sets it again after the refill, before it settles the plan)
    // the two-part level-table GEMM (header comment)
    uint32_t table_early_wgs;       // tuning knob walk_table_early_wgs, resolved (0 = one launch)
    bool table_queue;               // the table comes from the query-resident GEMM, whose work items can be shared by two launches
    uint32_t n_cus;                 // compute units of the device (0 = 256): sizes the GEMM's work items
    // the row level under the table reads table columns for neighbours with a node one level up (WalkPlan::up_table_level)
    uint32_t up_table_mode;         // tuning knob walk_up_table, resolved: 0 never | 1 by the rule below | 2 at every ef and launch size
    // the throughput kernel reads the nested table, one column per vector (WalkPlan::table_nested, table_nested.h)
    uint32_t table_nested_mode;     // tuning knob walk_table_nested, resolved: 0 never | 1, 2 wherever the handle has the nested operand (the knob's two
                                    // values differ in which graphs get one: walk_operands.hip ensure_nested_table)
};

// What preparation left, for the second step: no table operand for this graph and rule, no room for a workspace's table (out of
// memory, over the budget), no order key level, short order buffers.
struct WalkHave {
    uint32_t table_level_min, table_cols; // the handle's operand for the current key (0 = none)
    bool table_buffer;                    // the workspace's table holds B rows
    uint32_t n_order_keys, order_level0;  // key levels of the locality order and the first (highest) of them
    bool order_buffers;                   // the workspace's order buffers hold B queries
    uint32_t adj_up_level;                // the level whose LevelDev::adj_up is filled for this graph and table rule (0 = none)
    // the nested operand of the same table levels, with LevelDev::adj_tab filled for it (0 = none): its columns, and whether
    // LevelDev::adj_up holds columns of THAT table (a launch on the per-level table cannot read them, and the other way round)
    uint32_t nested_cols;
    bool adj_up_nested;
};

struct WalkPlan {
    WalkKernel kernel;
    bool ordered;              // the walk is cut after every order key level and the levels below run in locality order (throughput kernel)
    bool use_table;            // the level-table GEMM runs and the walk reads it
    bool table_waits_for_sort; // ... behind the previous chained launch's order sort (cos_index::chain_last_range_ev)
    uint32_t table_early_wgs;  // ... as two launches over one queue: workgroups of the early part (0 = one launch; header comment)
    uint32_t use_adj_mag;      // bit l: level l reads its winners' norms beside the adjacency
    bool refill_adj_mag;       // the norms are refilled first
    bool chained;              // the walk takes its place in the walk chain
    bool side_stream;          // the walk runs on the workspace's low-priority stream
    bool prepare_order, prepare_table; // what the above needs: order buffers + ranks, table operand + buffer
    uint32_t table_level_min, table_cols, cut_after_level; // of this launch (0 without a table / unsplit): cos_index_last_walk_split
    // The row level directly under the table (0 = none): its walk reads tab[q][tab_col0[l + 1] + adj_up] — one line — instead of the
    // code row — eight lines at 1024 dims — for every winner that has a node one level up (LevelDev::adj_up; a quarter of them where a
    // level holds a quarter of the nodes of the level below).  The GEMM computed that integer dot anyway.  Settled only (the table's
    // lowest level is known after preparation), throughput kernel, u8 codes on the one-row-per-pass path (G = 64).
    uint32_t up_table_level;
    // The table is the nested one (table_nested.h): one GEMM column per vector of the lowest table level instead of one per (level, node),
    // table_cols = that level's nodes; the table levels read LevelDev::adj_tab.  Settled only, like up_table_level: throughput kernel, u8
    // codes, no metadata schema, and the handle has the operand (WalkHave::nested_cols).  The four-wave kernel keeps the per-level table.
    bool table_nested;
};

// Work items of the query-resident level-table GEMM: a row group of 256 queries x a stripe of table_gemm_stripe_tiles() column tiles of
// 64 nodes.
//   * shared = false, a GEMM that is ONE full-width launch (not gated: c2's 20 903 columns): one item per workgroup — the partition of
//     the fixed grid it replaces, n_cus / row groups contiguous column groups per row group.  No workgroup restarts its staging
//     pipeline or reloads its query rows (finer items cost c2 0.14 ms per step: DESIGN.md §0.1);
//   * shared = true, a gated GEMM (table_waits_for_sort), whose queue two launches may share and whose workgroups are placed one by one
//     into the previous walk's draining lower range: about 24 items per workgroup of a full-width launch, so that late workgroups
//     find the rest of the work evenly spread; at least 2 and at most 64 tiles, so that the 256 query rows a workgroup reloads when
//     its row group changes (256 x K bytes from L2) stay small against the item's MFMAs.  12.5M x 1024 shard (65 161 columns x 32 768
//     queries): 21 tiles = 1 344 columns, 6 272 items.
inline uint32_t table_gemm_stripe_tiles(uint32_t B, uint32_t cols, uint32_t n_cus, bool shared) {
    const uint32_t n_tiles = (cols + 63u) / 64u, row_groups = (B + 255u) / 256u, cus = n_cus ? n_cus : 256u;
    if (!shared) {
        const uint32_t groups = std::max(1u, cus / std::max(1u, std::min(row_groups, cus)));
        return std::max(1u, (n_tiles + groups - 1u) / groups);
    }
    const uint64_t units = (uint64_t)n_tiles * row_groups;
    return (uint32_t)std::min<uint64_t>(64u, std::max<uint64_t>(2u, units / (24ull * cus)));
}
inline uint32_t table_gemm_items(uint32_t B, uint32_t cols, uint32_t n_cus, bool shared) {
    const uint32_t n_tiles = (cols + 63u) / 64u, st = table_gemm_stripe_tiles(B, cols, n_cus, shared);
    return (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (uint64_t)((n_tiles + st - 1u) / st) * ((B + 255u) / 256u));
}

// more than 64 scanned slots per node on some level: walk_general_kernel's graphs (it gathers the norms: no LevelDev::adj_mag)
inline bool walk_rows_over_64_slots(const WalkPlanIn &in) {
    for (uint32_t l = 0; l <= in.num_layers; l++)
        if (std::min(in.M[l], in.shortlist) > 64u) return true;
    return false;
}

// the launches walk_kernel and the latency kernels cannot hold (cos_index_create's domain checks follow this)
inline bool walk_general_needed(const WalkPlanIn &in) {
    if (in.ef > WALK_PLAN_FAST_MAX_EF) return true;
    // code rows wider than walk_kernel's chunk passes: u8 above 4096 dims (four passes of 64 lanes x 16 B), SubByte above 64 chunks
    if (in.nchunks != 0u && in.G != 0u && (in.nchunks + in.G - 1u) / in.G > (in.storage == 0u /* COS_STORAGE_U8 */ ? 4u : 1u)) return true;
    return walk_rows_over_64_slots(in);
}

// the launches both latency kernels take: reference filter, u8 / quaternary codes of <= 64 chunks, 1 <= ef <= 256, at most max_B queries
inline bool walk_latency_domain(const WalkPlanIn &in, uint32_t max_B) {
    if (max_B == 0 || in.B > max_B) return false;
    if (in.visited_mode != 0) return false;
    if (in.eng != WALK_PLAN_ENG_U8 && in.eng != WALK_PLAN_ENG_Q2) return false;
    if (in.nchunks == 0 || in.nchunks > 64u) return false; // rows of <= 4 passes of LAT_ROW_LANES chunks
    if (in.ef == 0 || in.ef > 256) return false;
    return true;
}

// Which fast kernel walks an unsplit launch inside their domain (!walk_general_needed).
// table_available: the launch can have a level table.  With the table (u8 codes) the throughput kernel beats the one-wave latency
// kernel at every launch size (1M x 768, ms per launch at ef 64 / 256: 256 queries 0.77 / 2.20 against 0.99 / 2.37; 1 024 queries
// 0.84 / 2.33 against 1.13 / 2.57; 2 048 queries 0.95 / 2.58 against 1.50 / 2.91) and the four-wave kernel up to ef 64 (0.77
// against 0.82 with the table, 0.88 without); above ef 64 the four-wave kernel with the table stays ahead on one client batch
// (1.73 against 2.20 at ef 256).  profiles/r04_single_batch_probe.jsonl, r04_mid_size_probe.jsonl.  Round 6 (r06_single_batch_probe.jsonl): one
// client batch with the automatic table — ef 64 0.642 / 0.643 ms (throughput / four waves), ef 128 1.017 / 1.148, ef 256 1.747 / 1.658.
inline WalkKernel walk_fast_kernel(const WalkPlanIn &in, bool table_available) {
    if (in.no_self_seed) return WalkKernel::Throughput; // the unseeded filter exists in the throughput kernel only
    // the four-wave kernel's s_first is sized 64 * Mmax words: keep the workgroup's LDS small
    const bool lat4 = walk_latency_domain(in, in.lat4_max_B) && std::max(in.M[0], in.M[in.num_layers]) <= 64u;
    if (table_available && in.small_table_tk && in.eng == WALK_PLAN_ENG_U8)
        return in.ef > 128u && lat4 ? WalkKernel::Lat4 : WalkKernel::Throughput; // (round 6: the 128-key pool + ranked merge moved the crossover from ef 64 to 128)
    if (lat4) return WalkKernel::Lat4;
    if (walk_latency_domain(in, in.lat_max_B)) return WalkKernel::Lat1;
    return WalkKernel::Throughput;
}

// The plan of one launch.  have == nullptr: what the launch wants, taking for granted that whatever it asks to be prepared will be
// there; with `have`: the same rules downgraded to what preparation left (never more than the first step asked for).
inline WalkPlan walk_plan(const WalkPlanIn &in, const WalkHave *have = nullptr) {
    WalkPlan p{};
    // (a launch outside the fast kernels' domain walks every level from rows, in one launch, in arrival order)
    const bool general = walk_general_needed(in);
    // Big launches walk in locality order (kernels_order.hip).  Beam widths above 256 keep the single launch: the cut costs the tail
    // of one more launch, a fixed ~3 % of the walk whatever the ef, while what the order saves shrinks as the walk turns from
    // memory-bound to bound by its own serial work (c2: +16 % at ef 64, +3.6 % at 128, +2.6 % at 256, +1 % at 512; nothing measurable
    // at ef 512 on the uniform corpus or on a 12.5M shard: profiles/archive/r03_order_probe_*.jsonl and the two
    // r03_final_bench_default_* lines, taken with and without this rule).
    p.ordered = !general && in.order_min_B && in.B >= in.order_min_B && in.ef <= 256u && (!have || (have->n_order_keys > 0 && have->order_buffers));
    // Which kernel walks decides whether the level table is worth its GEMM: the throughput kernel (from table_min_B queries on, and
    // where it takes the four-wave kernel's small launches) and the four-wave latency kernel (one client batch, u8 codes only) read
    // it, the one-wave latency kernel does not.
    bool table = !general && in.table_min_B && (have ? have->table_level_min != 0 && have->table_buffer : in.table_supported);
    const bool table_size = in.B >= in.table_min_B || in.B <= in.lat4_max_B;
    if (general) p.kernel = WalkKernel::General;
    else if (p.ordered) {
        p.kernel = WalkKernel::Throughput;
        table = table && table_size;
    } else {
        const WalkKernel with_table = walk_fast_kernel(in, true);
        table = table && ((with_table == WalkKernel::Lat4 && in.eng == WALK_PLAN_ENG_U8) || (with_table == WalkKernel::Throughput && table_size));
        p.kernel = table ? with_table : walk_fast_kernel(in, false);
    }
    p.use_table = table;
    p.chained = in.chain && in.B >= in.chain_min_B;
    if (have && table) {
        p.table_level_min = have->table_level_min;
        p.table_cols = have->table_cols;
        // (rows of one chunk pass, u8 up to 1024 dims, and ef up to 256: walk_kernel has the nested rounds in those instantiations only — walk_kernel.inc says why)
        if (p.kernel == WalkKernel::Throughput && in.table_nested_mode != 0 && in.eng == WALK_PLAN_ENG_U8 && in.mdim == 0u && have->nested_cols != 0u &&
            in.G != 0u && in.nchunks <= in.G && in.ef <= 256u) {
            p.table_nested = true;
            p.table_cols = have->nested_cols;
        }
        // Only a GEMM long enough to outlast the previous walk's upper range blocks its sort (engine_internal.h, chain_last_range_ev): the
        // shard's 65 161 columns x 32 768 queries (3.1 ms alone; gate: 33.3 -> 32.6 ms per step) do, c2's 20 903 (0.85 ms; 6.22 -> 6.29) do not
        // (profiles/r06_inflight_probe.txt)
        p.table_waits_for_sort = p.chained && (in.table_after_sort == 2 || (in.table_after_sort == 1 && (uint64_t)p.table_cols * in.B >= (1ull << 30)));
        // ... and only such a GEMM is worth two launches: the early part runs under the previous walk's lower range (header comment)
        if (p.table_waits_for_sort && in.table_queue)
            p.table_early_wgs = std::min(in.table_early_wgs, table_gemm_items(in.B, p.table_cols, in.n_cus, true));
    }
    if (have && p.ordered) p.cut_after_level = have->order_level0;
    // Norms beside the adjacency cost two more lines per window entry and save one line per winner: they pay while an expansion still
    // finds several winners, i.e. while the level's filter (64 x M bits) is not saturated by the ef pops of the level.
    // Measured (profiles/r06_adjmag_probe_*.jsonl): 1M x 768, M0 64 — ef 64: 7.8 evaluations per expansion, lower range 2.64 -> 2.42 ms;
    // ef 256: 2.35 per expansion, 5.10 -> 5.31 ms; 12.5M x 1024, M0 256 / M 64, ef 128: 9.8 per expansion, 26.5 -> 24.3 ms.
    // ... and while the launch is bound by bandwidth at all: one client batch is a chain of dependent round trips per query, where two more
    // loads and an LDS round trip per window entry only add latency (single batch of c2: 407 k QPS without, 396 k with).
    if (in.adj_mag_valid && in.adj_mag_mode != 0)
        for (uint32_t l = 0; l <= in.num_layers; l++)
            if (in.adj_mag_mode == 2 || (in.ef <= 2u * in.M[l] && in.B >= ADJ_MAG_USE_MIN_B)) p.use_adj_mag |= 1u << l;
    // (a root replaced on a live graph; small launches keep their gathers until a big one pays for the refill)
    p.refill_adj_mag = !in.adj_mag_valid && in.B >= ADJ_MAG_REFILL_MIN_B;
    // The level under the table takes its winners' norms from the window (adj_mag) and their columns from the same window (adj_up):
    // it follows adj_mag's rule — the extra window array costs what adj_mag's costs and pays under the same conditions.  Mode 2 drops
    // the launch-size condition of that rule for this one level (tests: a few hundred queries), not its need for valid norms.
    if (have && p.use_table && p.kernel == WalkKernel::Throughput && in.up_table_mode != 0 && in.eng == WALK_PLAN_ENG_U8 && in.G == 64u &&
        in.mdim == 0u && have->table_level_min >= 2u && have->adj_up_level == have->table_level_min - 1u && have->adj_up_nested == p.table_nested) {
        const uint32_t l = have->table_level_min - 1u;
        if (in.up_table_mode == 2 && in.adj_mag_valid && in.adj_mag_mode != 0) p.use_adj_mag |= 1u << l;
        if ((p.use_adj_mag >> l) & 1u) p.up_table_level = l;
    }
    p.side_stream = in.side_min_B && in.B >= in.side_min_B;
    p.prepare_order = p.ordered;
    p.prepare_table = p.use_table;
    return p;
}

} // namespace cosdev
