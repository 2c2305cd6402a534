// walk_lat_storages_check.cpp — the host arithmetic behind binary / octal codes and f16 / f32 rows in the latency kernels, on a CPU
// (tests/test_walk_lat_storages_plan.py builds and runs it): the domain rule and its row-width limits, the kernel the plan then
// picks, the f16 tile's bank-conflict-free row stride, and the LDS of both kernels at the corners of the domain.
#include <cstdio>

#include "walk_plan.h"

using namespace cosdev;

static int failures = 0, cases = 0;
#define CHECK(cond, what) do { cases++; if (!(cond)) { printf("FAIL %s\n", what); failures++; } } while (0)

static WalkPlanIn launch(int eng, uint32_t nchunks, uint32_t dim, uint32_t B, uint32_t ef) {
    WalkPlanIn in{};
    in.eng = eng, in.storage = 1u /* not u8 */, in.nchunks = nchunks, in.G = nchunks ? 64u : 1u, in.dim = dim;
    for (int l = 0; l <= 4; l++) in.M[l] = l ? 32u : 64u;
    in.num_layers = 4, in.shortlist = 64, in.B = B, in.ef = ef;
    in.lat_st_max_B = 2048, in.lat4_st_max_B = 512;
    return in;
}

int main() {
    for (int e : {WALK_PLAN_ENG_Q1, WALK_PLAN_ENG_Q3, WALK_PLAN_ENG_F32, WALK_PLAN_ENG_F16}) {
        const bool flt = e == WALK_PLAN_ENG_F32 || e == WALK_PLAN_ENG_F16;
        const uint32_t nch = flt ? 0u : 64u, dim = flt ? WALK_LAT_FLOAT_MAX_DIM : (e == WALK_PLAN_ENG_Q1 ? 8192u : 2048u); // at the width limit
        CHECK(walk_plan(launch(e, nch, dim, 256, 256)).kernel == WalkKernel::Lat4, "one client batch: four waves");
        CHECK(walk_plan(launch(e, nch, dim, 513, 64)).kernel == WalkKernel::Lat1, "above the four-wave size: one wave");
        CHECK(walk_plan(launch(e, nch, dim, 2049, 64)).kernel == WalkKernel::Throughput, "above both sizes");
        CHECK(walk_plan(launch(e, nch, dim, 256, 257)).kernel == WalkKernel::Throughput, "ef 257");
        { WalkPlanIn i = launch(e, nch, dim, 256, 64); i.visited_mode = 1; CHECK(walk_plan(i).kernel == WalkKernel::Throughput, "exact filter"); }
        { WalkPlanIn i = launch(e, nch, dim, 256, 64); i.M[0] = 128; CHECK(walk_plan(i).kernel == WalkKernel::Lat1, "rows of 128 slots: four waves decline"); }
        { WalkPlanIn i = launch(e, nch, dim, 256, 64); i.lat_st_max_B = i.lat4_st_max_B = 0; i.lat_max_B = 2048, i.lat4_max_B = 512;
          CHECK(walk_plan(i).kernel == WalkKernel::Throughput, "the limits of u8 / quaternary codes do not route these storages (the recorded plan cases)"); }
        if (flt) CHECK(walk_plan(launch(e, 0, dim + 1, 256, 64)).kernel == WalkKernel::Throughput, "float row over the limit");
        else CHECK(walk_plan(launch(e, 65, dim + 1, 256, 64)).kernel == WalkKernel::General, "code row over 64 chunks");
        CHECK(walk_latency_default_max_B(e, true, 512) <= walk_latency_default_max_B(e, false, 2048) && walk_latency_default_max_B(e, false, 2048) <= 2048,
              "defaults: nothing above the largest measured launch");
    }
    CHECK(!walk_latency_storages_domain(launch(WALK_PLAN_ENG_U8, 48, 768, 256, 64), 2048), "u8 codes answer to walk_latency_domain");
    CHECK(walk_latency_default_max_B(WALK_PLAN_ENG_Q1, false, 2048) == 0 && walk_latency_default_max_B(WALK_PLAN_ENG_Q2, true, 512) == 512, "binary: never; quaternary: as ever");

    // the f16 tiles: an odd row stride puts one column's words of the rows in different banks (64 banks, or 32 per half wave)
    const uint32_t tiles[2][2] = {{LAT_F16_TILE_ROWS, LAT_F16_TILE_DIMS}, {LAT4_F16_TILE_ROWS, LAT4_F16_TILE_DIMS}};
    for (auto &t : tiles) {
        const uint32_t rw = lat_f16_row_words(t[1]);
        bool clash = false;
        for (uint32_t banks : {32u, 64u})
            for (uint32_t j = 0; j < rw; j++) {
                uint64_t seen = 0;
                for (uint32_t r = 0; r < (t[0] < banks ? t[0] : banks); r++) { const uint32_t b = (r * rw + j) % banks; clash |= (seen >> b) & 1u; seen |= 1ull << b; }
            }
        CHECK(!clash && rw % 2 == 1 && rw * 2 > t[1] && lat_f16_tile_bytes(t[0], t[1]) == t[0] * rw * 4, "f16 tile stride");
        CHECK(64 % t[0] == 0 && t[1] % 8 == 0 && 64 % (t[1] / 8) == 0 && t[0] % (64 / (t[1] / 8)) == 0, "tile shape the loader assumes");
    }
    CHECK(walk_lat_lds_bytes(WALK_PLAN_ENG_Q3, 2048, 64, 64) == 4096 + 512 + 512 + 16 && walk_lat4_lds_bytes(WALK_PLAN_ENG_U8, 768, 256, 256, 64, 1) == 29216 + 16, "LDS: the integer engines add nothing to what the kernels asked for before");
    CHECK(walk_lat_lds_bytes(WALK_PLAN_ENG_F32, 100, 33, 64) - walk_lat_lds_bytes(WALK_PLAN_ENG_U8, 0, 33, 64) == 400 &&
              walk_lat_lds_bytes(WALK_PLAN_ENG_F16, 7, 64, 64) - walk_lat_lds_bytes(WALK_PLAN_ENG_U8, 0, 64, 64) == 32 + 16640, "one wave: query (+ tile)");
    CHECK(walk_lat4_lds_bytes(WALK_PLAN_ENG_F16, 100, 64, 64, 64, 1) - walk_lat4_lds_bytes(WALK_PLAN_ENG_U8, 0, 64, 64, 64, 1) == 400 + 4 * 4224, "f16, four waves");
    CHECK(walk_lat_lds_bytes(WALK_PLAN_ENG_F16, WALK_LAT_FLOAT_MAX_DIM, 256, 256) <= 65536 && walk_lat4_lds_bytes(WALK_PLAN_ENG_F16, WALK_LAT_FLOAT_MAX_DIM, 256, 256, 64, 1) <= 65536,
          "ef 256, the widest rows: under the 64 KB a workgroup gets without asking for more");
    printf("%s %d checks\n", failures ? "FAIL" : "OK", cases);
    return failures != 0;
}
