// walk_plan_check.cpp — replays tests/golden/walk_plan_cases.txt (the launch decisions recorded at the commit before walk_plan.h existed,
// scripts/gen_walk_plan_cases.cpp) through walk_plan.h.  Every line must give the recorded decisions; and the first step (what the launch
// wants prepared) must cover what the settled plan uses without asking for more than that commit prepared.
//   g++ -std=c++17 -I cosdata_amd/csrc tests/cxx/walk_plan_check.cpp -o walk_plan_check && ./walk_plan_check tests/golden/walk_plan_cases.txt
#include <cstdio>
#include <cstring>

#include "walk_plan.h"

using namespace cosdev;

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s walk_plan_cases.txt\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    char line[1024];
    unsigned n = 0, bad = 0, lineno = 0;
    while (fgets(line, sizeof(line), f)) {
        lineno++;
        if (line[0] == '#' || line[0] == '\n') continue;
        unsigned long long v[44];
        int got = 0, off = 0, adv = 0;
        while (got < 44 && sscanf(line + off, "%llu%n", &v[got], &adv) == 1) { off += adv; got++; }
        if (got != 44) return fprintf(stderr, "line %u: %d fields, expected 44\n", lineno, got), 2;
        WalkPlanIn in{};
        in.eng = (int)v[0]; in.storage = (uint32_t)v[1]; in.nchunks = (uint32_t)v[2]; in.G = (uint32_t)v[3];
        in.num_layers = (uint32_t)v[4];
        if (in.num_layers >= (uint32_t)WALK_PLAN_MAX_LEVELS) return fprintf(stderr, "line %u: num_layers %u\n", lineno, in.num_layers), 2;
        for (uint32_t l = 0; l <= in.num_layers; l++) in.M[l] = (uint32_t)(l == 0 ? v[6] : v[5]);
        in.shortlist = (uint32_t)v[7]; in.visited_mode = (uint32_t)v[8]; in.mdim = (uint32_t)v[9];
        in.B = (uint32_t)v[10]; in.ef = (uint32_t)v[11]; in.chain = v[12] != 0; in.no_self_seed = v[13] != 0;
        in.lat_max_B = (uint32_t)v[14]; in.lat4_max_B = (uint32_t)v[15]; in.small_table_tk = v[16] != 0; in.adj_mag_mode = (uint32_t)v[17];
        in.table_min_B = (uint32_t)v[18]; in.order_min_B = (uint32_t)v[19]; in.chain_min_B = (uint32_t)v[20]; in.side_min_B = (uint32_t)v[21];
        in.table_after_sort = (long long)v[22]; in.table_supported = v[23] != 0; in.adj_mag_valid = v[24] != 0;
        WalkHave have{};
        have.table_level_min = (uint32_t)v[25]; have.table_cols = (uint32_t)v[26]; have.table_buffer = v[27] != 0;
        have.n_order_keys = (uint32_t)v[28]; have.order_level0 = (uint32_t)v[29]; have.order_buffers = v[30] != 0;
        const WalkPlan p = walk_plan(in, &have), want = walk_plan(in);
        const unsigned long long out[11] = {(unsigned long long)p.kernel, p.ordered, p.use_table, p.table_waits_for_sort, p.use_adj_mag, p.refill_adj_mag,
                                            p.chained, p.side_stream, p.table_level_min, p.table_cols, p.cut_after_level};
        static const char *const names[11] = {"kernel", "ordered", "use_table", "table_waits_for_sort", "use_adj_mag", "refill_adj_mag",
                                              "chained", "side_stream", "table_level_min", "table_cols", "cut_after_level"};
        bool ok = true;
        for (int k = 0; k < 11; k++)
            if (out[k] != v[31 + k]) {
                fprintf(stderr, "line %u: %s = %llu, recorded %llu\n", lineno, names[k], out[k], v[31 + k]);
                ok = false;
            }
        // preparation: never less than the launch uses, never more than was prepared before
        if ((p.ordered && !want.prepare_order) || (p.use_table && !want.prepare_table) || (want.prepare_order && !v[42]) || (want.prepare_table && !v[43]) ||
            p.prepare_order != p.ordered || p.prepare_table != p.use_table || want.refill_adj_mag != p.refill_adj_mag) {
            fprintf(stderr, "line %u: prepares order %d table %d, uses %d %d, recorded preparation %llu %llu\n", lineno, want.prepare_order,
                    want.prepare_table, p.ordered, p.use_table, v[42], v[43]);
            ok = false;
        }
        n++;
        bad += !ok;
    }
    fclose(f);
    printf("%s %u cases, %u differ\n", bad || !n ? "FAIL" : "OK", n, bad);
    return bad || !n ? 1 : 0;
}
