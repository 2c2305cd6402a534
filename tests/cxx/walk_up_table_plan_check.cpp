// walk_up_table_plan_check.cpp — replays tests/golden/walk_up_table_plan_cases.txt through walk_plan.h: which level, if any, reads table
// columns for the neighbours that have a node one level up (WalkPlan::up_table_level), and what that does to WalkPlan::use_adj_mag.
// A second checker beside walk_plan_check.cpp, whose 44 recorded columns predate the field (its golden file stays byte for byte: with
// WalkPlanIn::up_table_mode = 0 and WalkHave::adj_up_level = 0, which is what it passes, the plan is what it was).  The launch is the
// flagship shape unless a column says otherwise (u8, 9 layers, M 64 / 256, shortlist 64, table and order from 8192 queries); the expected
// values are worked out by hand in the golden file.
//   g++ -std=c++17 -I cosdata_amd/csrc tests/cxx/walk_up_table_plan_check.cpp -o check && ./check tests/golden/walk_up_table_plan_cases.txt
#include <cstdio>

#include "walk_plan.h"

using namespace cosdev;

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s walk_up_table_plan_cases.txt\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    char line[512];
    unsigned n = 0, bad = 0, lineno = 0;
    while (fgets(line, sizeof(line), f)) {
        lineno++;
        if (line[0] == '#' || line[0] == '\n') continue;
        unsigned long long v[14];
        int got = 0, off = 0, adv = 0;
        while (got < 14 && sscanf(line + off, "%llu%n", &v[got], &adv) == 1) { off += adv; got++; }
        if (got != 14) return fprintf(stderr, "line %u: %d fields, expected 14\n", lineno, got), 2;
        WalkPlanIn in{};
        in.eng = (int)v[0]; in.storage = 0; in.G = (uint32_t)v[1]; in.nchunks = in.G;
        in.num_layers = 9;
        for (uint32_t l = 0; l <= in.num_layers; l++) in.M[l] = l == 0 ? 256u : 64u;
        in.shortlist = 64;
        in.B = (uint32_t)v[2]; in.ef = (uint32_t)v[3];
        in.chain = true; in.chain_min_B = 16384;
        in.lat_max_B = (uint32_t)v[4]; in.lat4_max_B = 0; in.small_table_tk = true;
        in.adj_mag_mode = (uint32_t)v[5]; in.adj_mag_valid = v[6] != 0;
        in.up_table_mode = (uint32_t)v[7];
        in.table_min_B = (uint32_t)v[8]; in.order_min_B = 8192; in.side_min_B = 4096; in.table_after_sort = 1;
        in.table_supported = true; in.table_queue = true; in.n_cus = 256;
        WalkHave have{};
        have.table_level_min = (uint32_t)v[9]; have.table_cols = 65161; have.table_buffer = true;
        have.n_order_keys = 1; have.order_level0 = 4; have.order_buffers = true;
        have.adj_up_level = (uint32_t)v[10];
        const WalkPlan p = walk_plan(in, &have), want = walk_plan(in);
        const unsigned long long out[3] = {(unsigned long long)p.kernel, p.up_table_level, p.use_adj_mag};
        static const char *const names[3] = {"kernel", "up_table_level", "use_adj_mag"};
        bool ok = true;
        for (int k = 0; k < 3; k++)
            if (out[k] != v[11 + k]) {
                fprintf(stderr, "line %u: %s = %llu, expected %llu\n", lineno, names[k], out[k], v[11 + k]);
                ok = false;
            }
        // the level is settled, never wanted (the table's lowest level is known after preparation); it is the level under the table, a
        // row level >= 1 that reads its norms beside the adjacency in this plan, and only the throughput kernel with a table has one
        const uint32_t l = p.up_table_level;
        if (want.up_table_level != 0 ||
            (l != 0 && (!p.use_table || p.kernel != WalkKernel::Throughput || l + 1 != p.table_level_min || l != have.adj_up_level || !((p.use_adj_mag >> l) & 1u) ||
                        in.up_table_mode == 0 || !in.adj_mag_valid))) {
            fprintf(stderr, "line %u: up_table_level %u breaks its rule (first step %u)\n", lineno, l, want.up_table_level);
            ok = false;
        }
        // mode 0 is the plan as it was: the same as never having the array
        WalkPlanIn in0 = in;
        in0.up_table_mode = 0;
        WalkHave have0 = have;
        have0.adj_up_level = 0;
        const WalkPlan a = walk_plan(in0, &have), b = walk_plan(in, &have0);
        if (a.up_table_level != 0 || b.up_table_level != 0 || a.use_adj_mag != b.use_adj_mag || a.kernel != p.kernel || a.use_table != p.use_table) {
            fprintf(stderr, "line %u: knob 0 / no array do not give the earlier plan\n", lineno);
            ok = false;
        }
        n++;
        bad += !ok;
    }
    fclose(f);
    printf("%s %u cases, %u differ\n", bad || !n ? "FAIL" : "OK", n, bad);
    return bad || !n ? 1 : 0;
}
