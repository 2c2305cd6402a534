// Stand-alone check of cosdata_amd/csrc/flat_plan.h (driven by tests/test_flat_plan.py, built with -fsanitize=address,undefined): the
// chunk schedule of the exhaustive scans, their unfused chunks, pool widths, limits, buffer sizes and the choice of the scoring kernel.
// The expected values are the hand-written lines of tests/golden/flat_plan_cases.txt (argv[1]), never taken from the header; what holds
// for every schedule — the chunks tile [0, n) in order, none is empty, only the first of a fused attempt is unfused — is checked on each.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "flat_plan.h"

namespace fp = flat_plan;

static int failures = 0;
static int line_no = 0;
#define EXPECT(cond)                                                                       \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::printf("FAIL %s:%d (cases line %d): %s\n", __FILE__, __LINE__, line_no, #cond); \
            failures++;                                                                    \
        }                                                                                  \
    } while (0)

struct Run { // `count` chunks of `nc` rows
    uint64_t nc, count;
    bool fused;
};

// "16384u 4194304f*2 284288f"
static bool parse_runs(std::istringstream &in, std::vector<Run> &runs) {
    std::string tok;
    while (in >> tok) {
        Run r{0, 1, false};
        char kind = 0;
        const int got = std::sscanf(tok.c_str(), "%" SCNu64 "%c*%" SCNu64, &r.nc, &kind, &r.count);
        if (got < 2 || (kind != 'u' && kind != 'f')) return false;
        r.fused = kind == 'f';
        runs.push_back(r);
    }
    return !runs.empty();
}

static void expect_schedule(const fp::Scan &plan, int attempt, const std::vector<Run> &runs) {
    fp::Schedule s = plan.schedule(attempt);
    fp::Chunk c{0, 0, false};
    uint64_t covered = 0, chunks = 0;
    size_t run = 0;
    uint64_t in_run = 0;
    while (s.next(c)) {
        if (c.n0 != covered || c.nc == 0 || (c.fused && (c.n0 == 0 || !plan.fused(attempt))) || (!c.fused && c.n0 > 0 && plan.fused(attempt))) {
            std::printf("FAIL cases line %d: chunk %" PRIu64 " = (%u, %u, %d) after %" PRIu64 " rows\n", line_no, chunks, c.n0, c.nc, (int)c.fused, covered);
            failures++;
            return;
        }
        if (run >= runs.size() || runs[run].nc != c.nc || runs[run].fused != c.fused) {
            std::printf("FAIL cases line %d: chunk %" PRIu64 " = %u%c, expected %s\n", line_no, chunks, c.nc, c.fused ? 'f' : 'u',
                        run >= runs.size() ? "the end" : (std::to_string(runs[run].nc) + (runs[run].fused ? "f" : "u")).c_str());
            failures++;
            return;
        }
        if (++in_run == runs[run].count) { run++; in_run = 0; }
        covered += c.nc;
        chunks++;
        if (chunks > (1u << 26)) break; // (no case comes near it: a schedule that does not end fails here)
    }
    EXPECT(covered == plan.n);
    EXPECT(run == runs.size() && in_run == 0);
    EXPECT(!s.next(c)); // the end stays the end
}

static bool kernel_of(const std::string &name, fp::ScanKernel &k) {
    if (name == "tile") k = fp::ScanKernel::TILE;
    else if (name == "planes") k = fp::ScanKernel::RESIDENT_PLANES;
    else if (name == "u8") k = fp::ScanKernel::RESIDENT_U8;
    else return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: flat_plan_check tests/golden/flat_plan_cases.txt\n");
        return 2;
    }
    std::ifstream file(argv[1]);
    if (!file) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    int cases = 0;
    std::string line;
    while (std::getline(file, line)) {
        line_no++;
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string what, colon, name;
        in >> what;
        bool parsed = true;
        cases++;
        if (what == "code" || what == "brute") {
            uint32_t n = 0, B = 0, k = 0;
            int knob = 0, attempt = 0;
            fp::ScanKernel kernel = fp::ScanKernel::TILE;
            std::vector<Run> runs;
            in >> n >> B >> k >> knob >> attempt;
            if (what == "code") parsed = (bool)(in >> name) && kernel_of(name, kernel);
            parsed = parsed && (bool)(in >> colon) && colon == ":" && parse_runs(in, runs);
            if (parsed) expect_schedule(what == "code" ? fp::code_scan(n, B, k, knob != 0, kernel) : fp::brute_scan(n, B, k, knob != 0), attempt, runs);
        } else if (what == "chunk") {
            uint32_t B = 0, n = 0, want = 0;
            parsed = (bool)(in >> name >> B >> n >> want) && (name == "code" || name == "brute");
            if (parsed) EXPECT((name == "code" ? fp::code_unfused_chunk(B, n) : fp::brute_unfused_chunk(B, n)) == want);
        } else if (what == "width") {
            uint32_t need = 0, want = 0;
            parsed = (bool)(in >> need >> want);
            if (parsed) EXPECT(fp::flat_pool_width(need) == want);
        } else if (what == "top_k") {
            uint32_t top_k = 0;
            int32_t want = 0;
            parsed = (bool)(in >> top_k >> want);
            if (parsed) EXPECT(fp::check_code_top_k(top_k) == want);
            if (parsed && want == 0) EXPECT(fp::code_pool(top_k) >= 5 * top_k && fp::code_pool(top_k) <= 1024);
        } else if (what == "k") {
            uint32_t k = 0, n = 0;
            int32_t want = 0;
            parsed = (bool)(in >> k >> n >> want);
            if (parsed) EXPECT(fp::check_brute_k(k, n) == want);
            if (parsed && want == 0) EXPECT(fp::brute_pool(k) >= 2 * k && fp::brute_pool(k) <= 1024);
        } else if (what == "segments") {
            uint32_t B = 0, rows = 0, want = 0;
            parsed = (bool)(in >> B >> rows >> want);
            if (parsed) EXPECT(fp::select_segments(B, rows) == want);
        } else if (what == "stride") {
            uint32_t rows = 0;
            uint64_t want = 0;
            parsed = (bool)(in >> rows >> want);
            if (parsed) EXPECT(fp::score_stride(rows) == want);
        } else if (what == "kernel") {
            uint64_t row_bytes = 0;
            int knob_tile = 0, planes_ok = 0, u8_ok = 0, knob_fp4 = 0, want_fp4 = 0;
            uint32_t want_kdims = 0;
            std::string want_kernel;
            fp::ScanKernel want = fp::ScanKernel::TILE;
            parsed = (bool)(in >> name >> row_bytes >> knob_tile >> planes_ok >> u8_ok >> knob_fp4 >> colon >> want_kdims >> want_kernel >> want_fp4) && colon == ":" &&
                     kernel_of(want_kernel, want) && (name == "u8" || name == "q1" || name == "q2" || name == "q3");
            if (parsed) {
                const int eng = name == "u8" ? fp::U8 : name == "q1" ? fp::Q1 : name == "q2" ? fp::Q2 : fp::Q3;
                const uint32_t kdims = fp::code_kdims(eng, row_bytes);
                const fp::ScanKernel got = fp::fused_kernel(eng, kdims, row_bytes, knob_tile != 0, planes_ok != 0, u8_ok != 0);
                EXPECT(kdims == want_kdims);
                EXPECT(got == want);
                EXPECT(fp::scan_fp4(got, eng, knob_fp4 != 0) == (want_fp4 != 0));
            }
        } else
            parsed = false;
        if (!parsed) {
            std::printf("FAIL cases line %d: cannot read \"%s\"\n", line_no, line.c_str());
            failures++;
        }
    }
    EXPECT(cases >= 80); // a truncated file is no pass
    // ---- the constants ----
    EXPECT(fp::FLAT_SEED == 16384);
    EXPECT(fp::flat_growth(64) == 8 && fp::flat_growth(128) == 4 && fp::flat_growth(1024) == 4);
    EXPECT(fp::flat_app_cap(64) == 4096 && fp::flat_app_cap(128) == 4096 && fp::flat_app_cap(1024) == 32768);
    EXPECT(fp::fused_cap(fp::ScanKernel::TILE) == (1ull << 22) && fp::fused_cap(fp::ScanKernel::RESIDENT_PLANES) == (1ull << 31) &&
           fp::fused_cap(fp::ScanKernel::RESIDENT_U8) == (1ull << 31));
    EXPECT(fp::OK == 0 && fp::INVALID == 3 && fp::UNIMPLEMENTED == 4);
    // the sizes each caller derives: the brute force by its unfused chunk, the code scan by the first chunk of the attempt
    {
        const fp::Scan b = fp::brute_scan(100000, 32768, 10, false);
        EXPECT(b.P == 64 && b.unfused == 8192 && b.seed == 8192 && b.first(0) == 8192 && b.first(1) == 8192 && b.fused(0) && !b.fused(1));
        const fp::Scan c = fp::code_scan(40000, 2, 204, false, fp::ScanKernel::TILE);
        EXPECT(c.P == 1024 && c.growth() == 4 && c.app_cap() == 32768 && c.first(0) == 16384 && c.first(1) == 40000 && c.fused(0) && !c.fused(1));
        const fp::Scan s = fp::code_scan(16384, 2, 10, false, fp::ScanKernel::TILE);
        EXPECT(!s.fused(0) && s.first(0) == 16384);
        const fp::Scan e = fp::code_scan(0, 2, 10, false, fp::ScanKernel::TILE); // no rows: no chunk
        fp::Schedule es = e.schedule(0);
        fp::Chunk c0{0, 0, false};
        EXPECT(!es.next(c0));
    }
    // ---- the brute force's margin rule: safe = the pool is not full, or the P-th GEMM score lies more than 2 * bound under the k-th ----
    {
        const double u = 1.0 / 16777216.0;
        // the bound, restated by hand: 2 * ((dim + dim / 8 + 32) + 8) * 2^-24 (tests/near_copies.py margin_bound states the same)
        EXPECT(fp::brute_margin_bound(64) == 2.0 * 112 * u && fp::brute_margin_bound(65) == 2.0 * 113 * u && fp::brute_margin_bound(96) == 2.0 * 148 * u);
        EXPECT(fp::brute_margin_bound(97) == 2.0 * 149 * u && fp::brute_margin_bound(100) == 2.0 * 152 * u && fp::brute_margin_bound(768) == 2.0 * 904 * u);
        EXPECT(fp::brute_margin_bound(1) == 2.0 * 41 * u);
        const float b96 = (float)fp::brute_margin_bound(96); // 296 * 2^-24: exact in f32
        EXPECT(!fp::brute_margin_safe(0.75f, 0.75f, 96, true));                              // equal scores
        EXPECT(!fp::brute_margin_safe(0.75f, 0.75f - 2.0f * b96, 96, true));                 // a gap of exactly 2 * bound is not "more than"
        EXPECT(fp::brute_margin_safe(0.75f, 0.75f - 2.0f * b96 - 0x1p-24f, 96, true));       // one ulp (of 0.5 .. 1) more is
        EXPECT(!fp::brute_margin_safe(0.5f, 0.75f, 96, true));                               // (a P-th score above the k-th: never)
        EXPECT(fp::brute_margin_safe(-0.25f, -0.5f, 96, true));                              // negative scores: the same subtraction
        EXPECT(!fp::brute_margin_safe(-0.25f, -0.25f - b96, 96, true));
        EXPECT(fp::brute_margin_safe(1e-3f, -1e-3f, 96, true) && !fp::brute_margin_safe(1e-5f, -1e-5f, 96, true)); // across zero
        EXPECT(fp::brute_margin_safe(0.75f, 0.75f, 96, false));                              // a pool that is not full holds every row
        EXPECT(fp::brute_margin_safe(__builtin_nanf(""), 0.0f, 96, false));
        const float nan = __builtin_nanf(""), inf = __builtin_inff();
        EXPECT(!fp::brute_margin_safe(nan, 0.0f, 96, true) && !fp::brute_margin_safe(1.0f, nan, 96, true) && !fp::brute_margin_safe(-nan, -nan, 96, true));
        EXPECT(!fp::brute_margin_safe(inf, 0.0f, 96, true) && !fp::brute_margin_safe(1.0f, -inf, 96, true) && !fp::brute_margin_safe(inf, -inf, 96, true));
        // the same two scores are safe at a short dim and not at a long one
        EXPECT(fp::brute_margin_safe(0.5f, 0.5f - 1e-4f, 64, true) && !fp::brute_margin_safe(0.5f, 0.5f - 1e-4f, 1024, true));
        // k = P / 2 exactly: the pool's width does not enter the rule beyond "full" — the caller reads ranks k and P of a pool of
        // brute_pool(k) keys, and at k = 32, 64, ..., 512 that pool is exactly 2k wide
        for (uint32_t k = 32; k <= 512; k *= 2) EXPECT(fp::brute_pool(k) == 2 * k && fp::brute_pool(k + 1) == (k == 512 ? 0u : 4 * k));
        static_assert(fp::brute_margin_safe(1.0f, 0.0f, 4096, true) && !fp::brute_margin_safe(1.0f, 1.0f, 1, true), "the rule is a constant expression");
        EXPECT(fp::BRUTE_EXACT_NEVER == 0 && fp::BRUTE_EXACT_BY_RULE == 1 && fp::BRUTE_EXACT_ALWAYS == 2);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
