// Stand-alone check of cosdata_amd/csrc/level_grow_plan.h (driven by tests/test_level_grow_plan.py, built with -fsanitize=address,undefined):
// where the new nodes of an append go on every level of the base graph (tail: the root) and of the pseudo-root component (tail: the pseudo
// nodes), their child links, and the renumbering of an old index.
// The expected values are the hand-written lines of tests/golden/level_grow_plan_cases.txt (argv[1]), never taken from the header.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "level_grow_plan.h"

namespace mg = level_grow_plan;

static int failures = 0;
static int line_no = 0;
#define EXPECT(cond)                                                                       \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::printf("FAIL %s:%d (cases line %d): %s\n", __FILE__, __LINE__, line_no, #cond); \
            failures++;                                                                    \
        }                                                                                  \
    } while (0)

static bool word(std::istringstream &in, const char *want) {
    std::string w;
    return (bool)(in >> w) && w == want;
}
template <typename T> static bool numbers(std::istringstream &in, size_t count, std::vector<T> &out) {
    out.clear();
    for (size_t i = 0; i < count; i++) {
        uint64_t v = 0;
        if (!(in >> v)) return false;
        out.push_back((T)v);
    }
    return true;
}

static bool plan_case(std::istringstream &in) {
    uint32_t levels = 0, n_new = 0;
    std::vector<uint32_t> tails;
    std::vector<uint8_t> comp, lvl;
    if (!(in >> levels) || levels == 0 || levels > 16 || !word(in, "tails") || !numbers(in, levels, tails) || !word(in, "new") || !(in >> n_new) || !word(in, "comp") ||
        !numbers(in, n_new, comp) || !word(in, "lvl") || !numbers(in, n_new, lvl) || !word(in, ":"))
        return false;
    const std::vector<mg::LevelPlan> plan = mg::plan_levels(tails, n_new, comp.data(), lvl.data());
    EXPECT(plan.size() == levels);
    for (uint32_t l = 0; l < levels; l++) {
        if (l > 0 && !word(in, "|")) return false;
        uint32_t add = 0;
        if (!(in >> add)) return false;
        const bool have = l < plan.size();
        if (have) {
            EXPECT(plan[l].tail_first == tails[l]);
            EXPECT(plan[l].add == add);
            EXPECT(plan[l].who.size() == add && plan[l].index.size() == add && plan[l].child.size() == add);
        }
        for (uint32_t k = 0; k < add; k++) {
            std::string tok;
            if (!(in >> tok)) return false;
            unsigned who = 0, index = 0, child = 0;
            char dash = 0;
            const bool leaf = std::sscanf(tok.c_str(), "%u,%u,%c", &who, &index, &dash) == 3 && dash == '-';
            if (!leaf && std::sscanf(tok.c_str(), "%u,%u,%u", &who, &index, &child) != 3) return false;
            if (leaf != (l == 0)) return false;
            if (!have || k >= plan[l].who.size() || k >= plan[l].index.size() || k >= plan[l].child.size()) continue;
            EXPECT(plan[l].who[k] == who);
            EXPECT(plan[l].index[k] == index);
            EXPECT(plan[l].child[k] == (leaf ? mg::NONE : child));
        }
    }
    std::string rest;
    return !(in >> rest);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: level_grow_plan_check tests/golden/level_grow_plan_cases.txt\n");
        return 2;
    }
    std::ifstream file(argv[1]);
    if (!file) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    int plans = 0, remaps = 0, tails = 0;
    std::string line;
    while (std::getline(file, line)) {
        line_no++;
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string what;
        in >> what;
        bool parsed = true;
        if (what == "plan") {
            parsed = plan_case(in);
            plans++;
        } else if (what == "remap") {
            uint32_t idx = 0, tail_first = 0, add = 0, want = 0;
            parsed = (bool)(in >> idx >> tail_first >> add >> want);
            if (parsed) EXPECT(mg::remap_index(idx, tail_first, add) == want);
            remaps++;
        } else if (what == "tail") {
            uint32_t count = 0, want = 0;
            std::vector<uint32_t> ids;
            parsed = (bool)(in >> count) && word(in, ":") && numbers(in, count, ids) && word(in, ":") && (bool)(in >> want);
            if (parsed) EXPECT(mg::tail_first(ids.data(), count) == want);
            tails++;
        } else
            parsed = false;
        if (!parsed) {
            std::printf("FAIL cases line %d: cannot read \"%s\"\n", line_no, line.c_str());
            failures++;
        }
    }
    EXPECT(plans >= 9 && remaps >= 9 && tails >= 5); // a truncated file is no pass
    EXPECT(mg::PSEUDO_LO == 0xFFFFFFFFu - 257u && mg::NONE == 0xFFFFFFFFu);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
