// walk_operands.h — the decisions behind the arrays a dense handle derives from its resident graph for the walk alone: the locality-order
// ranks, the level table's per-level and nested operands, and beside the adjacency the norms (LevelDev::adj_mag), the node one level up
// (adj_up) and the packed node | column word (adj_tab).  Which levels the table takes, which level carries the order key, the depth-first
// rank, which level wants adj_up, and the one state every operand keeps.  Plain integer logic: no HIP, no handle, every knob arrives
// resolved (walk_operands.hip builds, owns and drops the arrays from it; tests/cxx/walk_operands_check.cpp checks it on a CPU).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/cosdata_hip.h"
#include "walk_plan.h"

namespace cosdev {

// What changed about the resident graph, for cos_graph_changed (walk_operands.hip): the one call that invalidates.
//   LEVELS     a level's nodes or the vectors under them: upload, build, append
//   ROOT       the root's code row and norm were replaced on the levels as they are
//   ADJACENCY  neighbour slots changed under unchanged nodes: delete, a build or append that failed half way
enum class GraphChange : uint8_t { LEVELS, ROOT, ADJACENCY };
// ... and which changes an operand falls with (OperandState::follows)
constexpr uint8_t FOLLOWS_LEVELS = 1u << (int)GraphChange::LEVELS;
constexpr uint8_t FOLLOWS_ROOT = FOLLOWS_LEVELS | 1u << (int)GraphChange::ROOT;
constexpr uint8_t FOLLOWS_ADJACENCY = FOLLOWS_ROOT | 1u << (int)GraphChange::ADJACENCY;

// One operand of the current graph: built for key K, went without for key K (an optimisation that did not fit the device's memory or
// that this graph cannot have: same results, and not tried again for K until the graph changes), or invalid.  OperandState{FOLLOWS_...}.
struct OperandState {
    enum Kind : uint8_t { INVALID, BUILT, WITHOUT };
    uint8_t follows;
    Kind kind = INVALID;
    uint64_t key = 0;
    bool valid() const { return kind != INVALID; }
    bool built(uint64_t k = 0) const { return kind == BUILT && key == k; }
    bool without(uint64_t k = 0) const { return kind == WITHOUT && key == k; }
    void settle(bool built_, uint64_t k = 0) { kind = built_ ? BUILT : WITHOUT; key = k; }
    void invalidate() { kind = INVALID; key = 0; }
    void graph_changed(GraphChange c) { if ((follows >> (int)c) & 1u) invalidate(); }
};

// ---- which levels the level table takes ---------------------------------------------------------------------------------------------
constexpr uint32_t WALK_TABLE_MAX_COLS = 1u << 20; // of one level under the automatic rule, of all levels together always
// keys of a handle's table sets: the automatic rule's per-level bound under TABLE_KEY_AUTO, or the explicit max_cols; the nested set of
// the same levels (table_nested.h) carries TABLE_KEY_NESTED on top
constexpr uint64_t TABLE_KEY_AUTO = 1ull << 63, TABLE_KEY_NESTED = 1ull << 62;

struct LevelShape { // the levels of a graph as the rules below see them
    uint32_t num_layers;
    uint32_t n[WALK_PLAN_MAX_LEVELS];                                      // nodes of every level
    bool node_table[WALK_PLAN_MAX_LEVELS], adj_node[WALK_PLAN_MAX_LEVELS]; // its node -> vector row array / node-index adjacency is resident
};
struct TableRule {
    uint64_t key;
    uint32_t level_min, cols;                // the table holds the levels level_min ... num_layers, cols nodes together (0, 0 = no table)
    uint32_t col0[WALK_PLAN_MAX_LEVELS];     // first column of a table level, level by level from the top
};

// Which levels pay.  A table column costs one GEMM column per launch (~2.6 ps per query and column at K = 1024), a level walked
// from rows costs ~0.11 ns per evaluation, and a level's walk evaluates 0.2-0.4 x ef x M rows per query: a level of n nodes pays
// while n < ~40 x that.  Measured on both ends — 1M x 768 at ef 64, M 32: level 4 (3 917 nodes) pays, level 3 (15 570) does not;
// one 12.5M x 1024 shard at ef 128, M 64: level 5 (12 225) +24 % QPS, level 4 (48 870) another +17 %, both far above a fixed
// 8 192 columns (profiles/r04_c4_table_cols_probe.jsonl) — the automatic rule is n_level <= c x ef_search x neighbors_count, level
// by level from the top; an explicit max_cols caps the columns of all table levels together instead.  Round 4-5: c = 8 up to ef 64
// and 6 above: the wider pools of ef > 64 make a walk spend its time ranking and inserting, so a row it does not fetch saves less
// (1M x 768, M 32: at ef 64 level 3 = 7.6 x ef x M pays, 7.53 -> 7.13 ms per 32 768 queries; at ef 256 level 2 = 7.7 x ef x M
// costs 5.4 ms of GEMM and saves nothing, level 3 = 1.9 x pays; profiles/r04_table_level_rule_probe.jsonl).
// Round 6 (profiles/r06_rule_probe_*.jsonl): what decides is how many rows an expansion still evaluates, i.e. how far the level's
// filter (64 x M bits) is from saturation after ef pops — ef relative to M, not ef alone.  12.5M x 1024 with M 64: level 4 (48 870
// nodes) at ef 80 / 96 / 112 (9.5 / 8.0 / 6.8 x ef x M) +25 % / +25 % / +25 % QPS, 14 evaluations per expansion; 1M x 768 with M 32:
// level 2 (62 869 nodes) at ef 128 / 256 (15.3 / 7.7 x) -20 % / -15 %, 3-5 evaluations per expansion.  c = 10 up to ef = 1.5 M, 8 up
// to 2 M, 6 above (M 32: the old rule — 8 up to ef 64, 6 above — except c = 10 up to ef 48).
inline uint64_t table_rule_c(uint32_t ef_search, uint32_t neighbors_count) {
    return 2u * ef_search <= 3u * neighbors_count ? 10u : (ef_search <= 2u * neighbors_count ? 8u : 6u);
}
// max_cols: cos_index_set_walk_table after its override, COS_WALK_TABLE_AUTO = the automatic rule; rule_c: tuning knob walk_table_rule_c,
// negative = the measured c above
inline TableRule table_rule(const LevelShape &g, uint32_t ef_search, uint32_t neighbors_count, uint32_t max_cols, long long rule_c) {
    TableRule r{};
    const bool automatic = max_cols == COS_WALK_TABLE_AUTO;
    const uint64_t c = rule_c >= 0 ? (uint64_t)rule_c : table_rule_c(ef_search, neighbors_count);
    const uint64_t per_level = automatic ? std::min<uint64_t>(c * ef_search * neighbors_count, WALK_TABLE_MAX_COLS) : (uint64_t)WALK_TABLE_MAX_COLS;
    const uint64_t total_cap = automatic ? (uint64_t)WALK_TABLE_MAX_COLS : (uint64_t)max_cols;
    r.key = automatic ? (TABLE_KEY_AUTO | per_level) : (uint64_t)max_cols;
    for (uint32_t l = g.num_layers; l >= 1; l--) { // level 0 (every vector) never takes part
        if (!g.node_table[l] || g.n[l] == 0 || g.n[l] > per_level || (uint64_t)r.cols + g.n[l] > total_cap) break;
        r.col0[l] = r.cols;
        r.cols += g.n[l];
        r.level_min = l;
    }
    return r;
}

// ---- which levels carry the order keys, and a level's rank --------------------------------------------------------------------------
// Key levels (the walk is cut AFTER each of them): by default ONE, the lowest level whose code rows take at most 64 MB — a
// quarter of the 256 MB memory-side cache, so the levels walked in arrival order stay cache-resident whatever the order, and the
// key is as fine as that allows (c2: level 2, 62 500 nodes x 768 B = 48 MB, levels 1 and 0 walked in order; a 12.5M x 1024
// shard: level 4, 48 829 nodes).  Every further cut costs the tail of one more launch (~0.3 ms per 32768 queries) and measured
// slower: profiles/archive/r03_locality_probe_split_levels.jsonl (cuts after 1 | 2 | 3 | 4 | 3,1 | 4,1 | 5,1 | 4,2,1 | 5,3,1).
// COS_WALK_SPLIT=a,b,.. overrides (split_mask: bit l = cut after level l, negative = the default; "0" = no split): descending,
// distinct, usable levels; one that is not is skipped, not an error.
inline std::vector<uint32_t> order_key_levels(const LevelShape &g, uint64_t row_stride, long long split_mask) {
    const uint32_t num_layers = g.num_layers;
    auto usable = [&](uint32_t l) { return l >= 1 && l <= num_layers && g.n[l] > 1 && g.n[l] <= (1u << 20) && g.adj_node[l]; };
    std::vector<uint32_t> want, levels;
    if (split_mask >= 0) {
        for (uint32_t l = num_layers; l >= 1; l--)
            if ((split_mask >> l) & 1) want.push_back(l);
    } else {
        for (uint32_t l = 1; l <= num_layers; l++)
            if (usable(l) && (uint64_t)g.n[l] * row_stride <= (64ull << 20)) { want.push_back(l); break; }
    }
    uint32_t prev = num_layers + 1;
    for (uint32_t l : want) {
        if (!usable(l) || l >= prev) continue;
        levels.push_back(l);
        prev = l;
    }
    return levels;
}

// Every node of a key level -> its position in a depth-first order of that level's graph (WalkArgs::order_rank).  Consecutive positions
// are graph neighbours or a short backtrack apart, so queries whose best key-level nodes have close positions walk the same region of
// the levels below — a one-dimensional locality order that needs nothing but the graph (the vectors' geometry is in its edges).
// adj: [n][M] node indices, an empty slot holds a value >= n.  From the root (the last node of every level: where every walk of the
// level starts) in slot order, then from every node not reached yet in index order.
inline std::vector<uint32_t> order_rank_dfs(const uint32_t *adj, uint32_t n, uint32_t M) {
    std::vector<uint32_t> rank(n, 0u), stack;
    std::vector<uint8_t> seen(n, 0);
    uint32_t next = 0;
    auto dfs_from = [&](uint32_t start) {
        stack.push_back(start);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            stack.pop_back();
            if (seen[v]) continue;
            seen[v] = 1;
            rank[v] = next++;
            const uint32_t *row = &adj[(size_t)v * M];
            for (uint32_t j = M; j-- > 0;) { // pushed last = visited first: slot order
                const uint32_t u = row[j];
                if (u < n && !seen[u]) stack.push_back(u);
            }
        }
    };
    if (n) dfs_from(n - 1);
    for (uint32_t v = 0; v < n; v++) if (!seen[v]) dfs_from(v);
    return rank;
}

// ---- which level wants LevelDev::adj_up ---------------------------------------------------------------------------------------------
// The ONE level that can use it: the row level directly under the current level table (level >= 1), on a graph whose norms beside the
// adjacency are there (the walk takes both from the same window), u8 codes on the one-row-per-pass path; 0 = none.
inline uint32_t adj_up_wanted_level(uint32_t table_level_min, int eng, uint32_t G, bool adj_mag, bool up_table_knob) {
    return adj_mag && table_level_min >= 2u && eng == WALK_PLAN_ENG_U8 && G == 64u && up_table_knob ? table_level_min - 1u : 0u;
}

} // namespace cosdev
