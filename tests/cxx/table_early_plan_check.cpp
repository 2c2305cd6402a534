// table_early_plan_check.cpp — replays tests/golden/table_early_plan_cases.txt through walk_plan.h: where the level-table GEMM of a
// launch is issued as two launches over one queue of work items (WalkPlan::table_early_wgs), how many workgroups its early part gets,
// and how many work items the queue holds.  The launch is the flagship shape otherwise (u8 x 1024 dims, 9 layers, M 64 / 256, ef 112,
// table and order from 8192 queries, chain from `chain_min_B`); the expected values are worked out by hand in the golden file.
//   g++ -std=c++17 -I cosdata_amd/csrc tests/cxx/table_early_plan_check.cpp -o check && ./check tests/golden/table_early_plan_cases.txt
#include <cstdio>

#include "walk_plan.h"

using namespace cosdev;

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s table_early_plan_cases.txt\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    char line[512];
    unsigned n = 0, bad = 0, lineno = 0;
    while (fgets(line, sizeof(line), f)) {
        lineno++;
        if (line[0] == '#' || line[0] == '\n') continue;
        unsigned long long v[12];
        if (sscanf(line, "%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9],
                   &v[10], &v[11]) != 12)
            return fprintf(stderr, "line %u: expected 12 fields\n", lineno), 2;
        WalkPlanIn in{};
        in.eng = WALK_PLAN_ENG_U8; in.storage = 0; in.nchunks = 64; in.G = 64;
        in.num_layers = 9;
        for (uint32_t l = 0; l <= in.num_layers; l++) in.M[l] = l == 0 ? 256u : 64u;
        in.shortlist = 64; in.ef = 112;
        in.lat_max_B = 2048; in.lat4_max_B = 512; in.small_table_tk = true; in.adj_mag_mode = 1;
        in.table_min_B = 8192; in.order_min_B = 8192; in.side_min_B = 4096;
        in.table_supported = true; in.adj_mag_valid = true;
        in.B = (uint32_t)v[0]; in.chain = v[2] != 0; in.chain_min_B = (uint32_t)v[3]; in.table_after_sort = (long long)v[4];
        in.table_queue = v[5] != 0; in.table_early_wgs = (uint32_t)v[6]; in.n_cus = (uint32_t)v[7];
        WalkHave have{};
        have.table_level_min = 4; have.table_cols = (uint32_t)v[1]; have.table_buffer = true;
        have.n_order_keys = 1; have.order_level0 = 4; have.order_buffers = true;
        const WalkPlan p = walk_plan(in, &have), want = walk_plan(in);
        const unsigned long long got[4] = {p.use_table, p.table_waits_for_sort, p.table_early_wgs, table_gemm_items(in.B, have.table_cols, in.n_cus, p.table_waits_for_sort)};
        static const char *const names[4] = {"use_table", "table_waits_for_sort", "table_early_wgs", "items"};
        bool ok = true;
        for (int k = 0; k < 4; k++)
            if (got[k] != v[8 + k]) {
                fprintf(stderr, "line %u: %s = %llu, expected %llu\n", lineno, names[k], got[k], v[8 + k]);
                ok = false;
            }
        // the early part exists only for a gated GEMM, never has more workgroups than the queue has items, and is settled, not wanted
        if ((p.table_early_wgs && !p.table_waits_for_sort) || p.table_early_wgs > got[3] || want.table_early_wgs != 0) {
            fprintf(stderr, "line %u: early part of %u workgroups, gated %d, %llu items, first step %u\n", lineno, p.table_early_wgs, p.table_waits_for_sort, got[3],
                    want.table_early_wgs);
            ok = false;
        }
        n++;
        bad += !ok;
    }
    fclose(f);
    printf("%s %u cases, %u differ\n", bad || !n ? "FAIL" : "OK", n, bad);
    return bad || !n ? 1 : 0;
}
