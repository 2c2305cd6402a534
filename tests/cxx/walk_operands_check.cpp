// walk_operands_check.cpp — the decisions behind the walk's per-graph operands (cosdata_amd/csrc/walk_operands.h): which levels the level
// table takes, which levels carry the order keys, the depth-first rank of a level, which level wants adj_up, and the operand state.
// Known answers from the measurements the rule's comment records, and restatements in this file's own words on random inputs.  No GPU,
// no input file.
//   g++ -std=c++17 -I cosdata_amd/csrc tests/cxx/walk_operands_check.cpp -o check && ./check
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <random>

#include "walk_operands.h"

using namespace cosdev;

static unsigned bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { bad++; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

constexpr uint32_t WALK_TABLE_AUTO = COS_WALK_TABLE_AUTO;
struct TableRuleIn { // table_rule's arguments
    LevelShape g;
    uint32_t ef_search, neighbors_count, max_cols;
    long long rule_c;
};
static TableRule table_rule(const TableRuleIn &in) { return table_rule(in.g, in.ef_search, in.neighbors_count, in.max_cols, in.rule_c); }
static TableRuleIn rule_in(std::initializer_list<uint32_t> n_from_level0, uint32_t ef, uint32_t M, uint32_t max_cols = WALK_TABLE_AUTO, long long c = -1) {
    TableRuleIn in{};
    uint32_t l = 0;
    for (uint32_t n : n_from_level0) {
        in.g.n[l] = n;
        in.g.node_table[l] = in.g.adj_node[l] = l != 0; // level 0 keeps no node -> vector row array (a node index is the row)
        l++;
    }
    in.g.num_layers = l - 1;
    in.ef_search = ef;
    in.neighbors_count = M;
    in.max_cols = max_cols;
    in.rule_c = c;
    return in;
}

// The two measured graphs.  1M x 768, neighbors_count 32: levels 4 / 3 / 2 hold 3 917 / 15 570 / 62 869 nodes (the rule's comment).  One
// 12.5M x 1024 shard, neighbors_count 64: levels 5 / 4 hold 12 225 / 48 870 nodes.  ONLY these five sizes are measured: every other level
// below is made up, a quarter / four times its neighbour, so of the assertions that follow the level_min and the bounds rest on
// measurements, the sums in `cols` and `col0` partly on the made-up sizes (they check the arithmetic, not a recorded figure).
#define C2_LEVELS {1000001u, 251476u, 62869u, 15570u, 3917u, 980u}
#define C4_LEVELS {12500001u, 3127680u, 781920u, 195480u, 48870u, 12225u, 3056u, 764u, 191u, 48u}

static void known_answers() {
    // neighbors_count 32, ef 64: c = 8, per-level bound 16 384: level 4 and level 3 in, level 2 out
    TableRule r = table_rule(rule_in(C2_LEVELS, 64, 32));
    CHECK(table_rule_c(64, 32) == 8 && r.key == (TABLE_KEY_AUTO | 16384u), "M 32 ef 64: c %llu key %llx", (unsigned long long)table_rule_c(64, 32), (unsigned long long)r.key);
    CHECK(r.level_min == 3 && r.cols == 980u + 3917u + 15570u, "M 32 ef 64: level_min %u cols %u", r.level_min, r.cols);
    CHECK(r.col0[5] == 0 && r.col0[4] == 980u && r.col0[3] == 980u + 3917u, "M 32 ef 64: first columns, from the top");
    const uint64_t key64 = r.key;
    // ef 128: c = 6, 24 576: level 2 still out
    r = table_rule(rule_in(C2_LEVELS, 128, 32));
    CHECK(table_rule_c(128, 32) == 6 && r.key == (TABLE_KEY_AUTO | 24576u) && r.level_min == 3, "M 32 ef 128: level_min %u", r.level_min);
    // ef 256: c = 6, 49 152: level 2 (7.7 x ef x M, costs 5.4 ms of GEMM and saves nothing) out
    r = table_rule(rule_in(C2_LEVELS, 256, 32));
    CHECK(r.key == (TABLE_KEY_AUTO | 49152u) && r.level_min == 3, "M 32 ef 256: level_min %u", r.level_min);
    // ef 48 = 1.5 M: c = 10, 15 360: level 3 (15 570) no longer fits
    r = table_rule(rule_in(C2_LEVELS, 48, 32));
    CHECK(table_rule_c(48, 32) == 10 && r.key == (TABLE_KEY_AUTO | 15360u) && r.level_min == 4 && r.cols == 980u + 3917u, "M 32 ef 48: level_min %u", r.level_min);
    CHECK(r.key != key64, "rules that choose other levels have other keys");
    CHECK(table_rule_c(49, 32) == 8 && table_rule_c(65, 32) == 6, "c changes right above 1.5 M and 2 M");
    // neighbors_count 64, ef 80 / 96 / 112: c = 10 / 10 / 8, level 5 and level 4 both in, level 3 out
    const uint32_t efs[3] = {80, 96, 112};
    const uint64_t cs[3] = {10, 10, 8};
    for (int i = 0; i < 3; i++) {
        r = table_rule(rule_in(C4_LEVELS, efs[i], 64));
        CHECK(table_rule_c(efs[i], 64) == cs[i] && r.key == (TABLE_KEY_AUTO | cs[i] * efs[i] * 64u), "M 64 ef %u: c", efs[i]);
        CHECK(r.level_min == 4 && r.cols == 48u + 191u + 764u + 3056u + 12225u + 48870u, "M 64 ef %u: level_min %u cols %u", efs[i], r.level_min, r.cols);
    }
    r = table_rule(rule_in(C4_LEVELS, 128, 64)); // ef 128 = 2 M: c = 8, 65 536 (level 4: another +17 %)
    CHECK(r.level_min == 4, "M 64 ef 128: level_min %u", r.level_min);
    // the knob overrides c
    r = table_rule(rule_in(C2_LEVELS, 64, 32, WALK_TABLE_AUTO, 40));
    CHECK(r.key == (TABLE_KEY_AUTO | 81920u) && r.level_min == 2, "c = 40: level 2 in");
    r = table_rule(rule_in(C2_LEVELS, 64, 32, WALK_TABLE_AUTO, 0));
    CHECK(r.key == TABLE_KEY_AUTO && r.level_min == 0 && r.cols == 0, "c = 0: no table");

    // explicit max_cols: caps the columns of all levels together, a level alone may hold up to 2^20; the key is max_cols itself
    r = table_rule(rule_in(C2_LEVELS, 64, 32, 20467));
    CHECK(r.key == 20467u && r.level_min == 3 && r.cols == 20467u, "max_cols 20467: level_min %u", r.level_min);
    r = table_rule(rule_in(C2_LEVELS, 64, 32, 20466));
    CHECK(r.key == 20466u && r.level_min == 4 && r.cols == 4897u, "max_cols 20466: level_min %u", r.level_min);
    CHECK(table_rule(rule_in(C2_LEVELS, 999, 32, 20466)).key == 20466u && table_rule(rule_in(C2_LEVELS, 999, 32, 20466)).level_min == 4, "explicit: ef plays no part");
    r = table_rule(rule_in(C2_LEVELS, 64, 32, 979));
    CHECK(r.level_min == 0 && r.cols == 0, "max_cols below the top level: no table");
    r = table_rule(rule_in(C2_LEVELS, 64, 32, 0));
    CHECK(r.key == 0 && r.level_min == 0 && r.cols == 0, "max_cols 0: no table");
    r = table_rule(rule_in(C2_LEVELS, 64, 32, 1u << 20));
    CHECK(r.level_min == 1 && r.cols == 251476u + 62869u + 15570u + 3917u + 980u, "max_cols 2^20: every level above 0");
    CHECK((key64 & TABLE_KEY_AUTO) && !(r.key & TABLE_KEY_AUTO) && !(key64 & TABLE_KEY_NESTED) && (key64 | TABLE_KEY_NESTED) != key64 && (r.key | TABLE_KEY_NESTED) != key64,
          "automatic, explicit and nested keys are apart");
    // a level without a node table ends the range
    TableRuleIn in = rule_in(C2_LEVELS, 64, 32);
    in.g.node_table[4] = false;
    r = table_rule(in);
    CHECK(r.level_min == 5 && r.cols == 980u, "no node table on level 4: level 5 alone");
    in.g.node_table[5] = false;
    CHECK(table_rule(in).level_min == 0, "no node table on the top level: no table");
    in = rule_in(C2_LEVELS, 64, 32);
    in.g.n[4] = 0;
    CHECK(table_rule(in).level_min == 5, "an empty level ends the range");
    // the 2^20 caps of the automatic rule: a level alone, and all levels together
    r = table_rule(rule_in({5000000u, 1048577u, 100u}, 1024, 256));
    CHECK(r.key == (TABLE_KEY_AUTO | (1u << 20)) && r.level_min == 2 && r.cols == 100u, "a level above 2^20 nodes is out whatever ef x M");
    r = table_rule(rule_in({5000000u, 600000u, 448576u}, 1024, 256));
    CHECK(r.level_min == 1 && r.cols == (1u << 20), "2^20 columns together fit");
    r = table_rule(rule_in({5000000u, 600000u, 448577u}, 1024, 256));
    CHECK(r.level_min == 2 && r.cols == 448577u, "2^20 + 1 columns together do not");
}

// The rule once more, in other words: of all the lowest levels L for which every level from L to the top has a node table, is not empty,
// is small enough on its own and fits with the others, the table starts at the LOWEST.
static void rule_against_restatement() {
    std::mt19937_64 rng(777);
    for (int it = 0; it < 4000; it++) {
        TableRuleIn in{};
        in.g.num_layers = 1 + rng() % 15;
        uint64_t n = 1 + rng() % 4;
        for (uint32_t l = in.g.num_layers + 1; l-- > 0;) { // from the top: every level about 2-5 times the one above, some out of line
            in.g.n[l] = (uint32_t)std::min<uint64_t>(n, 3000000u);
            in.g.node_table[l] = l != 0 && rng() % 23 != 0;
            if (rng() % 37 == 0) in.g.n[l] = 0;
            n = n * (2 + rng() % 4) + rng() % 3;
        }
        const uint32_t Ms[5] = {8, 16, 32, 64, 256};
        in.neighbors_count = Ms[rng() % 5];
        in.ef_search = 1 + rng() % (6 * in.neighbors_count);
        in.max_cols = rng() % 3 ? WALK_TABLE_AUTO : (uint32_t)(rng() % ((1u << 20) + 1));
        in.rule_c = rng() % 5 ? -1 : (long long)(rng() % 50);
        const TableRule got = table_rule(in);

        const bool automatic = in.max_cols == WALK_TABLE_AUTO;
        const double ratio = (double)in.ef_search / in.neighbors_count;
        const uint64_t c = in.rule_c >= 0 ? (uint64_t)in.rule_c : ratio <= 1.5 ? 10 : ratio <= 2.0 ? 8 : 6;
        uint64_t alone = 1u << 20, together = 1u << 20, key;
        if (automatic) {
            alone = std::min<uint64_t>(alone, c * in.ef_search * in.neighbors_count);
            key = 0x8000000000000000ull + alone;
        } else {
            together = in.max_cols;
            key = in.max_cols;
        }
        uint32_t want_min = 0, want_cols = 0;
        for (uint32_t L = 1; L <= in.g.num_layers && want_min == 0; L++) {
            uint64_t sum = 0;
            bool ok = true;
            for (uint32_t l = L; l <= in.g.num_layers; l++) {
                ok = ok && in.g.node_table[l] && in.g.n[l] != 0 && in.g.n[l] <= alone;
                sum += in.g.n[l];
            }
            if (ok && sum <= together) { want_min = L; want_cols = (uint32_t)sum; }
        }
        CHECK(got.key == key && got.level_min == want_min && got.cols == want_cols, "case %d: level_min %u cols %u key %llx, expected %u %u %llx", it, got.level_min,
              got.cols, (unsigned long long)got.key, want_min, want_cols, (unsigned long long)key);
        uint32_t c0 = 0;
        for (uint32_t l = in.g.num_layers; want_min && l >= want_min; l--) {
            CHECK(got.col0[l] == c0, "case %d: level %u starts at column %u, expected %u", it, l, got.col0[l], c0);
            c0 += in.g.n[l];
        }
    }
}

static void order_levels() {
    // default: the lowest usable level whose code rows fit 64 MiB — 1M x 768: level 2 (62 869 x 768 B = 46 MiB; level 1: 184 MiB)
    LevelShape g = rule_in(C2_LEVELS, 64, 32).g;
    bool *adj = g.adj_node;
    adj[0] = true;
    std::vector<uint32_t> lv = order_key_levels(g, 768, -1);
    CHECK(lv == std::vector<uint32_t>({2u}), "default key level of 1M x 768");
    CHECK(order_key_levels(g, 1072, -1) == std::vector<uint32_t>({3u}), "62 869 x 1 072 B = 64.3 MiB: level 3");
    CHECK(order_key_levels(g, 1056, -1) == std::vector<uint32_t>({2u}), "62 869 x 1 056 B = 63.3 MiB: level 2");
    adj[2] = false;
    CHECK(order_key_levels(g, 768, -1) == std::vector<uint32_t>({3u}), "a level without its node adjacency is not usable");
    adj[2] = true;
    // the override: bit l = cut after level l; descending, distinct, usable; level 0 and levels above the top are no key levels
    CHECK(order_key_levels(g, 768, (1 << 3) | (1 << 1)) == std::vector<uint32_t>({3u, 1u}), "cuts after 3 and 1");
    CHECK(order_key_levels(g, 768, 0).empty() && order_key_levels(g, 768, 1).empty(), "\"0\": no split");
    CHECK(order_key_levels(g, 768, (1 << 9) | (1 << 5) | 1) == std::vector<uint32_t>({5u}), "levels outside the graph are skipped");
    adj[3] = false;
    CHECK(order_key_levels(g, 768, (1 << 4) | (1 << 3) | (1 << 2)) == std::vector<uint32_t>({4u, 2u}), "an unusable level is skipped, not an error");
    const LevelShape tiny = rule_in({3000000u, 2000000u, 1u}, 64, 32).g;
    CHECK(order_key_levels(tiny, 16, -1).empty() && order_key_levels(tiny, 16, 6).empty(), "a level of one node or of more than 2^20 carries no key");
    // adj_up: the level under the table, u8 rows of one pass, norms beside the adjacency there, knob on
    CHECK(adj_up_wanted_level(4, WALK_PLAN_ENG_U8, 64, true, true) == 3 && adj_up_wanted_level(2, WALK_PLAN_ENG_U8, 64, true, true) == 1, "adj_up: level_min - 1");
    CHECK(adj_up_wanted_level(1, WALK_PLAN_ENG_U8, 64, true, true) == 0 && adj_up_wanted_level(0, WALK_PLAN_ENG_U8, 64, true, true) == 0, "adj_up: never level 0");
    CHECK(adj_up_wanted_level(4, WALK_PLAN_ENG_Q2, 64, true, true) == 0 && adj_up_wanted_level(4, WALK_PLAN_ENG_U8, 32, true, true) == 0 &&
          adj_up_wanted_level(4, WALK_PLAN_ENG_U8, 64, false, true) == 0 && adj_up_wanted_level(4, WALK_PLAN_ENG_U8, 64, true, false) == 0, "adj_up: engine, G, norms, knob");
}

// The rank against a recursive depth-first walk: a node's rank is the number of nodes entered before it.
static void check_rank(const std::vector<uint32_t> &adj, uint32_t n, uint32_t M, const char *what) {
    const std::vector<uint32_t> got = order_rank_dfs(adj.data(), n, M);
    std::vector<uint32_t> want(n, 0xFFFFFFFFu);
    uint32_t entered = 0;
    std::function<void(uint32_t)> enter = [&](uint32_t v) {
        want[v] = entered++;
        for (uint32_t j = 0; j < M; j++) {
            const uint32_t u = adj[(size_t)v * M + j];
            if (u < n && want[u] == 0xFFFFFFFFu) enter(u);
        }
    };
    enter(n - 1);
    for (uint32_t v = 0; v < n; v++)
        if (want[v] == 0xFFFFFFFFu) enter(v);
    CHECK(got.size() == n && got[n - 1] == 0, "%s: the last node has rank 0", what);
    std::vector<uint32_t> hits(n, 0);
    for (uint32_t r : got)
        if (r < n) hits[r]++;
    CHECK(std::all_of(hits.begin(), hits.end(), [](uint32_t h) { return h == 1; }), "%s: the rank is no permutation", what);
    CHECK(got == want, "%s: the rank differs from the recursive walk", what);
}
static void ranks() {
    std::mt19937 rng(4242);
    for (int it = 0; it < 60; it++) {
        const uint32_t n = 2 + rng() % 3000, M = 1u << (rng() % 6), parts = 1 + rng() % 4; // nodes v with equal v % parts: one component
        std::vector<uint32_t> adj((size_t)n * M);
        for (uint32_t v = 0; v < n; v++)
            for (uint32_t j = 0; j < M; j++) {
                const uint32_t dice = rng() % 10;
                uint32_t u = (uint32_t)(rng() % n) / parts * parts + v % parts;
                if (dice < 3) u = 0xFFFFFFFFu;          // an empty slot
                else if (dice == 3) u = n + rng() % 7;  // out of range
                adj[(size_t)v * M + j] = u;
            }
        check_rank(adj, n, M, "random");
    }
    check_rank({1u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u}, 2, 2, "n = 2");
    check_rank({0xFFFFFFFFu, 0xFFFFFFFFu}, 2, 1, "n = 2, no edge");
    const std::vector<uint32_t> none = order_rank_dfs(std::vector<uint32_t>(5 * 4, 0xFFFFFFFFu).data(), 5, 4);
    CHECK(none == std::vector<uint32_t>({1u, 2u, 3u, 4u, 0u}), "every slot empty: the root, then index order");
    check_rank(std::vector<uint32_t>(5 * 4, 0xFFFFFFFFu), 5, 4, "every slot empty");
}

static void states() {
    const GraphChange changes[3] = {GraphChange::LEVELS, GraphChange::ROOT, GraphChange::ADJACENCY};
    // what falls with what: the ranks with the levels; the table sets also with the root; the arrays beside the adjacency with everything
    const struct { uint8_t follows; bool drops[3]; } kinds[3] = {{FOLLOWS_LEVELS, {true, false, false}}, {FOLLOWS_ROOT, {true, true, false}}, {FOLLOWS_ADJACENCY, {true, true, true}}};
    const uint64_t K = TABLE_KEY_AUTO | 16384u, K2 = TABLE_KEY_AUTO | 24576u;
    for (const auto &kind : kinds)
        for (int c = 0; c < 3; c++) {
            OperandState s{kind.follows};
            CHECK(!s.valid() && !s.built(K) && !s.without(K), "a new state is invalid");
            s.settle(true, K);
            CHECK(s.valid() && s.built(K) && !s.without(K) && !s.built(K2) && !s.without(K2), "built for K, not for another key");
            s.graph_changed(changes[c]);
            CHECK(s.valid() == !kind.drops[c] && s.built(K) == !kind.drops[c], "follows %u, change %d: built -> %s", kind.follows, c, kind.drops[c] ? "invalid" : "built");
            s.settle(false, K);
            CHECK(s.valid() && s.without(K) && !s.built(K) && !s.without(K2) && !s.built(K2), "went without for K");
            s.graph_changed(changes[c]);
            CHECK(s.without(K) == !kind.drops[c] && s.valid() == !kind.drops[c], "follows %u, change %d: went-without is remembered until invalidated", kind.follows, c);
        }
    // an ensure function's use: one attempt per (graph, key), whatever its outcome
    OperandState s{FOLLOWS_ROOT};
    unsigned attempts = 0;
    auto ensure = [&](uint64_t key, bool fits) {
        if (s.built(key) || s.without(key)) return;
        attempts++;
        s.settle(fits, key);
    };
    for (int i = 0; i < 5; i++) ensure(K, false);
    CHECK(attempts == 1 && s.without(K), "no retry for the same key");
    s.graph_changed(GraphChange::ADJACENCY);
    ensure(K, false);
    CHECK(attempts == 1, "a change the operand does not follow: no retry");
    ensure(K2, true);
    CHECK(attempts == 2 && s.built(K2), "another key: one attempt");
    s.graph_changed(GraphChange::ROOT);
    ensure(K2, true);
    CHECK(attempts == 3 && s.built(K2), "after the graph changed: again");
    s.invalidate();
    CHECK(!s.valid() && !s.built(K2), "invalidate");
    OperandState unkeyed{FOLLOWS_ADJACENCY}; // operands without a key (ranks, norms) use key 0
    unkeyed.settle(false);
    CHECK(unkeyed.valid() && unkeyed.without() && !unkeyed.built(), "key 0");
}

int main() {
    known_answers();
    rule_against_restatement();
    order_levels();
    ranks();
    states();
    printf("%s %u failed checks\n", bad ? "FAIL" : "OK", bad);
    return bad ? 1 : 0;
}
