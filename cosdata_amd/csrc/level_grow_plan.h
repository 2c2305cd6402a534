// level_grow_plan.h — the host-only part of growing a graph's levels in front of a tail (builder.hip: cos_index_append,
// cos_index_append_meta).  A level keeps its nodes in ascending id, and what an append adds lies above every resident id but below the
// level's TAIL: the root on the base graph (one node, the last), the pseudo nodes on the pseudo-root component (ids >= u32::MAX - 257,
// the pseudo root first among them; the node table ends in the same tail).  So the new nodes go between the old nodes and that tail.
// What follows from it is plain integer work: where the tail starts, how many nodes a level gains, the node index of every new node on
// every level it reaches, its child link one level down, and the rule that renumbers an old index.  Plain C++17, no HIP header and no
// handle, so that a stand-alone program can check it (tests/cxx/level_grow_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace level_grow_plan {

constexpr uint32_t PSEUDO_LO = 0xFFFFFEFEu; // the pseudo root's id; every pseudo node's id is at or above it (engine_types.h: builder.hip ties the two)
constexpr uint32_t NONE = 0xFFFFFFFFu;      // an empty slot: never renumbered

// first index of an ascending id list that holds a pseudo node (n when there is none)
inline uint32_t tail_first(const uint32_t *ids, uint32_t n) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < PSEUDO_LO) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// an index into an array whose tail moved up by `add`: the tail's entries follow it, everything below stays (the device kernel applies
// the same rule to every stored index: grow_tail_kernel, kernels_link.hip)
inline uint32_t remap_index(uint32_t idx, uint32_t tail_first, uint32_t add) { return idx != NONE && idx >= tail_first ? idx + add : idx; }

struct LevelPlan {
    uint32_t tail_first = 0;     // first tail node of the level before the growth = node index of the first new node
    uint32_t add = 0;            // new nodes of the level
    std::vector<uint32_t> who;   // [add] position of the new node in the call's arrays, ascending
    std::vector<uint32_t> index; // [add] its node index on this level after the growth (tail_first + rank)
    std::vector<uint32_t> child; // [add] its node index one level down after THAT level's growth (level 0: unused, NONE)
};

// tails[l] = tail_first of level l before the growth (base graph: the root's index, nodes - 1).  in_graph[i] == 0: a row that is on no
// level (the component's Base replicas — all-zero metadata dimensions —, recorded in the node table only; the base graph has none).
// New node i is on the levels 0..max_levels[i].
inline std::vector<LevelPlan> plan_levels(const std::vector<uint32_t> &tails, uint32_t n_new, const uint8_t *in_graph, const uint8_t *max_levels) {
    std::vector<LevelPlan> out(tails.size());
    for (std::size_t l = 0; l < tails.size(); l++) {
        LevelPlan &P = out[l];
        P.tail_first = tails[l];
        uint32_t below = 0; // rank among the new nodes of level l - 1
        for (uint32_t i = 0; i < n_new; i++) {
            if (!in_graph[i]) continue;
            if (max_levels[i] >= l) {
                P.who.push_back(i);
                P.index.push_back(P.tail_first + P.add);
                P.child.push_back(l == 0 ? NONE : out[l - 1].tail_first + below);
                P.add++;
            }
            if (l > 0 && (uint32_t)max_levels[i] + 1 >= l) below++;
        }
    }
    return out;
}

} // namespace level_grow_plan
