// walk_pair_plan_check.cpp — walk_pair_plan.h on a CPU (tests/test_walk_pair_plan.py builds and runs it): the flagship's launch walks
// its last range in pairs, and every condition of the pair kernel's domain, taken away alone, sends the launch back to walk_kernel.
#include <cstdio>

#include "walk_pair_plan.h"

using namespace cosdev;

static int failures = 0;
#define CHECK(what, got, want)                                                              \
    do {                                                                                    \
        const unsigned g_ = (got), w_ = (want);                                             \
        if (g_ != w_) { printf("FAIL %s: got %u, want %u\n", what, g_, w_); failures++; }   \
    } while (0)

int main() {
    // the 12.5M x 1024 shard: M0 256 / M 64, ef 112, 32 768 queries, table levels >= 4, cut after level 4
    WalkPlanIn in{};
    in.eng = WALK_PLAN_ENG_U8;
    in.nchunks = 64, in.G = 64;
    in.num_layers = 9;
    for (int l = 0; l <= 9; l++) in.M[l] = l ? 64u : 256u;
    in.shortlist = 64;
    in.B = 32768, in.ef = 112;
    WalkPlan p{};
    p.kernel = WalkKernel::Throughput;
    p.ordered = true;
    p.use_table = true;
    p.table_level_min = 4;
    p.use_adj_mag = 0xFu;
    WalkPairIn pi{1u, 512u, 3u, 12500000u};
    CHECK("flagship", walk_pair_plan(in, p, pi), 512u);
    { WalkPairIn q = pi; q.mode = 0; CHECK("knob 0", walk_pair_plan(in, p, q), 0u); }
    { WalkPlanIn i = in; i.B = WALK_PAIR_MIN_B - 1; CHECK("small launch, rule", walk_pair_plan(i, p, pi), 0u); }
    { WalkPairIn q = pi; q.n_vectors = 1000000; CHECK("a launch dense in the corpus, rule", walk_pair_plan(in, p, q), 0u); }
    { WalkPairIn q = pi; q.n_vectors = 32768u * WALK_PAIR_MIN_ROWS_PER_QUERY; CHECK("at the density threshold", walk_pair_plan(in, p, q), 512u); }
    { WalkPairIn q = pi; q.n_vectors = 1000000; q.mode = 2; CHECK("a dense launch, always", walk_pair_plan(in, p, q), 512u); }
    { WalkPlanIn i = in; i.B = 301; WalkPairIn q = pi; q.mode = 2; CHECK("small launch, always", walk_pair_plan(i, p, q), 512u); }
    { WalkPlanIn i = in; i.B = 1; WalkPairIn q = pi; q.mode = 2; CHECK("one query", walk_pair_plan(i, p, q), 0u); }
    { WalkPlan x = p; x.ordered = false; CHECK("not ordered", walk_pair_plan(in, x, pi), 0u); }
    { WalkPlan x = p; x.kernel = WalkKernel::General; CHECK("general kernel", walk_pair_plan(in, x, pi), 0u); }
    { WalkPlanIn i = in; i.eng = WALK_PLAN_ENG_Q2; CHECK("quaternary codes", walk_pair_plan(i, p, pi), 0u); }
    { WalkPlanIn i = in; i.nchunks = 96; CHECK("two chunk passes", walk_pair_plan(i, p, pi), 0u); }
    { WalkPlanIn i = in; i.nchunks = 16, i.G = 16; CHECK("rows of fewer than 64 lanes", walk_pair_plan(i, p, pi), 0u); }
    { WalkPlanIn i = in; i.nchunks = 63; CHECK("1000 dimensions", walk_pair_plan(i, p, pi), 512u); }
    { WalkPlanIn i = in; i.ef = 256; CHECK("ef 256", walk_pair_plan(i, p, pi), 512u); }
    { WalkPlanIn i = in; i.ef = 257; CHECK("ef 257", walk_pair_plan(i, p, pi), 0u); }
    { WalkPlanIn i = in; i.visited_mode = 1; CHECK("exact filter", walk_pair_plan(i, p, pi), 0u); }
    { WalkPlanIn i = in; i.mdim = 5; CHECK("metadata schema", walk_pair_plan(i, p, pi), 0u); }
    { WalkPlan x = p; x.use_adj_mag = 0xBu; CHECK("a level gathers its norms", walk_pair_plan(in, x, pi), 0u); }
    { WalkPlan x = p; x.table_level_min = 3; CHECK("a table level in the last range", walk_pair_plan(in, x, pi), 0u); }
    { WalkPlan x = p; x.use_table = false; x.table_level_min = 0; CHECK("no table", walk_pair_plan(in, x, pi), 512u); }
    { WalkPairIn q = pi; q.cache_entries = 256; CHECK("256 entries", walk_pair_plan(in, p, q), 256u); }
    { WalkPairIn q = pi; q.cache_entries = 1024; CHECK("1024 entries", walk_pair_plan(in, p, q), 1024u); }
    { WalkPairIn q = pi; q.cache_entries = 500; CHECK("not a power of two", walk_pair_plan(in, p, q), 0u); }
    { WalkPairIn q = pi; q.cache_entries = 32; CHECK("too few entries", walk_pair_plan(in, p, q), 0u); }
    { WalkPairIn q = pi; q.cache_entries = 8192; CHECK("too many entries", walk_pair_plan(in, p, q), 0u); }
    { WalkPairIn q = pi; q.cache_entries = 4096; CHECK("4096 entries: two waves of 39 KB", walk_pair_plan(in, p, q), 0u); }
    { WalkPairIn q = pi; q.cache_entries = 2048; CHECK("2048 entries", walk_pair_plan(in, p, q), 2048u); }
    { WalkPlanIn i = in; i.ef = 256; WalkPairIn q = pi; q.cache_entries = 2048; CHECK("2048 entries at ef 256", walk_pair_plan(i, p, q), 2048u); }
    // the two waves' LDS: M0 2048 is 16 KB of filter per wave, 2 x (19 664 + 16 384) bytes do not fit 64 KB, 2 x (19 664 + 8 192) do
    { WalkPlanIn i = in; i.M[0] = 2048; WalkPairIn q = pi; q.cache_entries = 2048; CHECK("a wide level 0 and 2048 entries", walk_pair_plan(i, p, q), 0u); }
    { WalkPlanIn i = in; i.M[0] = 2048; WalkPairIn q = pi; q.cache_entries = 1024; CHECK("a wide level 0 and 1024 entries", walk_pair_plan(i, p, q), 1024u); }
    CHECK("cache offset of the flagship's wave", walk_pair_cache_off(256, 112), 6544u);
    if (failures) return 1;
    printf("OK 32 cases\n");
    return 0;
}
