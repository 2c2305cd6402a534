// table_nested_check.cpp — the nested column order of the level table and the packed adjacency word (cosdata_amd/csrc/table_nested.h), and
// the plan's flag for it (walk_plan.h, WalkPlan::table_nested), on random nested level structures.  No GPU, no input file.
//   g++ -std=c++17 -I cosdata_amd/csrc tests/cxx/table_nested_check.cpp -o check && ./check
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>

#include "table_nested.h"
#include "walk_plan.h"

using namespace cosdev;

static unsigned bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { bad++; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// a random graph skeleton: level l holds a random subset of level l - 1's vectors in a random node order, the root (vector N) last on every level
struct Levels {
    std::vector<uint32_t> n;
    std::vector<std::vector<uint32_t>> node_vec, child; // child[l][j] = node of level l - 1 with the same vector
};
static Levels random_levels(std::mt19937 &rng, uint32_t L, uint32_t N, uint32_t shrink) {
    Levels g;
    g.n.assign(L + 1, 0);
    g.node_vec.resize(L + 1);
    g.child.resize(L + 1);
    std::vector<uint32_t> vecs(N);
    std::iota(vecs.begin(), vecs.end(), 0u);
    for (uint32_t l = 0; l <= L; l++) {
        if (l > 0) {
            std::shuffle(vecs.begin(), vecs.end(), rng);
            vecs.resize(std::max<size_t>(0, vecs.size() / shrink));
        }
        std::vector<uint32_t> order = vecs;
        std::shuffle(order.begin(), order.end(), rng); // node order unrelated to the level below
        order.push_back(N);                            // the root
        g.node_vec[l] = order;
        g.n[l] = (uint32_t)order.size();
        if (l > 0) {
            std::vector<uint32_t> pos(N + 1, 0u); // vector -> node of the level below
            for (uint32_t i = 0; i < g.n[l - 1]; i++) pos[g.node_vec[l - 1][i]] = i;
            g.child[l].resize(g.n[l]);
            for (uint32_t j = 0; j < g.n[l]; j++) g.child[l][j] = pos[order[j]];
        }
    }
    return g;
}

static void check_structure(std::mt19937 &rng, uint32_t L, uint32_t N, uint32_t shrink, uint32_t lmin, uint32_t M) {
    const Levels g = random_levels(rng, L, N, shrink);
    NestedTable t;
    const bool ok = table_nested_columns(lmin, L, g.n, g.child, &t);
    CHECK(ok, "L %u N %u lmin %u: no nested table", L, N, lmin);
    if (!ok) return;
    CHECK(t.cols == g.n[lmin] && t.level_min == lmin && t.level_top == L, "shape");
    // the vector of every column, through the lowest level
    std::vector<uint32_t> col_vec(t.cols);
    for (uint32_t c = 0; c < t.cols; c++) col_vec[c] = g.node_vec[lmin][t.col_node[c]];
    for (uint32_t l = lmin; l <= L; l++) {
        const std::vector<uint32_t> &col = t.col[l - lmin];
        CHECK(col.size() == g.n[l], "level %u: %zu columns for %u nodes", l, col.size(), g.n[l]);
        // level l's columns are exactly [0, n_l): a permutation of the prefix
        std::vector<uint32_t> seen(g.n[l], 0);
        for (uint32_t c : col) {
            CHECK(c < g.n[l], "level %u: column %u outside [0, %u)", l, c, g.n[l]);
            if (c < g.n[l]) seen[c]++;
        }
        CHECK(std::all_of(seen.begin(), seen.end(), [](uint32_t s) { return s == 1; }), "level %u: columns are no permutation of the prefix", l);
        for (uint32_t j = 0; j < g.n[l]; j++) CHECK(col_vec[col[j]] == g.node_vec[l][j], "level %u node %u: column %u holds another vector", l, j, col[j]);
        if (l == L)
            for (uint32_t j = 0; j < g.n[l]; j++) CHECK(col[j] == j, "top level keeps its own order");
        // every word of adj_tab decodes to the adj_node entry and to the column of that node's vector; the empty marker stays
        const uint32_t bits = t.node_bits[l - lmin];
        CHECK(bits == table_nested_bits(g.n[l] - 1) && bits + table_nested_bits(t.cols - 1) <= 32, "level %u: %u node bits", l, bits);
        std::uniform_int_distribution<uint32_t> pick(0, g.n[l] - 1);
        for (uint32_t s = 0; s < 4 * M; s++) {
            const uint32_t node = s % 7 == 3 ? 0xFFFFFFFFu : pick(rng);
            const uint32_t word = node < g.n[l] ? table_nested_pack(node, col[node], bits) : node; // what fill_adj_tab_kernel writes
            if (node >= g.n[l]) { CHECK(word == 0xFFFFFFFFu, "empty marker"); continue; }
            const uint32_t dn = word & ((1u << bits) - 1u), dc = word >> bits;                        // what walk_kernel.inc reads
            CHECK(dn == node && dc == col[node] && col_vec[dc] == g.node_vec[l][node], "level %u: word %08x -> node %u column %u", l, word, dn, dc);
        }
    }
    // one table level: the nested order is the level's own
    if (lmin == L)
        for (uint32_t c = 0; c < t.cols; c++) CHECK(t.col_node[c] == c, "one level: identity");
}

int main() {
    std::mt19937 rng(12345);
    check_structure(rng, 5, 20000, 4, 1, 32);
    check_structure(rng, 5, 20000, 4, 3, 32);
    check_structure(rng, 5, 6000, 4, 5, 16);  // one table level
    check_structure(rng, 6, 3000, 3, 2, 16);
    check_structure(rng, 9, 70000, 4, 1, 64); // 15 + 15 bits on the lowest level, levels of a single node at the top
    check_structure(rng, 4, 300, 100, 1, 8);  // top levels of one node (the root alone): 0 node bits
    {
        // the bit rule: 65 536 nodes on the lowest table level fit (16 + 16), 65 537 do not (17 + 17) and the graph keeps the per-level table
        std::vector<uint32_t> n = {0, 65536, 1};
        std::vector<std::vector<uint32_t>> child(3);
        child[2] = {65535};
        NestedTable t;
        CHECK(table_nested_columns(1, 2, n, child, &t) && t.node_bits[0] == 16 && t.node_bits[1] == 0, "16 + 16 bits must fit");
        n[1] = 65537;
        child[2] = {65536};
        CHECK(!table_nested_columns(1, 2, n, child, &t), "17 + 17 bits must fall back");
        // ... and so do levels that are not nested: two nodes with one child, a child out of range, an empty level
        n = {0, 8, 3};
        child[2] = {7, 2, 2};
        CHECK(!table_nested_columns(1, 2, n, child, &t), "shared child");
        child[2] = {7, 2, 8};
        CHECK(!table_nested_columns(1, 2, n, child, &t), "child out of range");
        child[2] = {7, 2, 5};
        CHECK(table_nested_columns(1, 2, n, child, &t) && t.col[0][7] == 0 && t.col[0][2] == 1 && t.col[0][5] == 2 && t.col[0][0] == 3, "hand case");
        n = {0, 8, 0};
        child[2] = {};
        CHECK(!table_nested_columns(1, 2, n, child, &t), "empty level");
    }
    {
        // the plan: settled from WalkHave only, throughput kernel + u8 + no schema + knob; table_cols follows; the level under the table
        // reads adj_up only in the form that matches the launch's table; a default-initialised input plans as before
        WalkPlanIn in{};
        in.eng = WALK_PLAN_ENG_U8; in.G = 64; in.nchunks = 64; in.num_layers = 9;
        for (uint32_t l = 0; l <= 9; l++) in.M[l] = l ? 64u : 256u;
        in.shortlist = 64; in.B = 32768; in.ef = 112; in.chain = true; in.chain_min_B = 16384; in.small_table_tk = true;
        in.adj_mag_mode = 1; in.adj_mag_valid = true; in.up_table_mode = 1; in.table_min_B = 8192; in.order_min_B = 8192; in.side_min_B = 4096;
        in.table_after_sort = 1; in.table_supported = true; in.table_queue = true; in.n_cus = 256;
        WalkHave have{};
        have.table_level_min = 4; have.table_cols = 65161; have.table_buffer = true; have.n_order_keys = 1; have.order_level0 = 4; have.order_buffers = true;
        have.adj_up_level = 3; have.nested_cols = 48822; have.adj_up_nested = true;
        WalkPlan p = walk_plan(in, &have);
        CHECK(!p.table_nested && p.table_cols == 65161 && p.up_table_level == 0, "knob 0: per-level table, and adj_up in the other form is not read");
        CHECK(!walk_plan(in).table_nested, "never wanted, only settled");
        in.table_nested_mode = 1;
        p = walk_plan(in, &have);
        CHECK(p.table_nested && p.table_cols == 48822 && p.table_level_min == 4 && p.up_table_level == 3 && p.table_waits_for_sort, "flagship launch");
        have.adj_up_nested = false;
        CHECK(walk_plan(in, &have).up_table_level == 0, "adj_up holds node indices: not read under the nested table");
        have.adj_up_nested = true;
        have.nested_cols = 0;
        p = walk_plan(in, &have);
        CHECK(!p.table_nested && p.table_cols == 65161, "no operand: per-level table");
        have.nested_cols = 48822;
        WalkPlanIn q2 = in; q2.eng = WALK_PLAN_ENG_Q2;
        CHECK(!walk_plan(q2, &have).table_nested, "quaternary codes keep the per-level table");
        WalkPlanIn wide = in; wide.nchunks = 96;
        CHECK(!walk_plan(wide, &have).table_nested, "rows of two chunk passes keep the per-level table");
        WalkPlanIn beam = in; beam.ef = 300;
        CHECK(walk_plan(beam, &have).use_table && !walk_plan(beam, &have).table_nested, "beams above 256 keep the per-level table");
        WalkPlanIn md = in; md.mdim = 3;
        CHECK(!walk_plan(md, &have).table_nested, "a metadata schema keeps the per-level table");
        WalkPlanIn one = in; one.B = 256; one.ef = 256; one.lat4_max_B = 256; one.lat_max_B = 2048; one.M[0] = 64; // one client batch above ef 128: four-wave kernel
        p = walk_plan(one, &have);
        CHECK(p.kernel == WalkKernel::Lat4 && p.use_table && !p.table_nested && p.table_cols == 65161, "the four-wave kernel keeps the per-level table");
    }
    printf("%s %u failed checks\n", bad ? "FAIL" : "OK", bad);
    return bad ? 1 : 0;
}
