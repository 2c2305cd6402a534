// table_nested.h — the nested column order of the throughput walk's level table and the packed adjacency word of its table levels.
// Plain integer logic: no HIP, no handle (walk_operands.hip ensure_nested_table fills the device arrays from it; tests/cxx/table_nested_check.cpp
// checks it on a CPU).
//
// The levels of an HNSW graph are nested: every node of level l + 1 has a child on level l (LevelDev::child), the same vector.  A table
// with one column per (level, node) therefore repeats, for every level above the lowest table level, dots that the lowest level's columns
// already hold.  The nested table has ONE column per node of the lowest table level, ordered by the highest level the vector reaches:
// first the nodes of the top level in their own order, then the nodes that reach one level less in the order of that level, and so on
// down to the nodes that exist on the lowest table level only.  The nodes of level l then occupy exactly the columns [0, n_l), in some
// permutation, so a level's gathers stay as dense in cache lines as its own slice of the per-level table was, and a lower level touches
// again the lines the levels above it used.
//
// A table level's walk needs, for every neighbour, its node index (pool key, filter, output) AND its column.  Both come in the one word
// the walk loaded anyway: LevelDev::adj_tab holds node | column << node_bits where LevelDev::adj_node holds the node, node_bits =
// bits(n_l - 1).  That fits while bits(n_l - 1) + bits(columns - 1) <= 32 on every table level (12.5M x 1024 shard: 16 + 16); a graph
// that does not fit keeps the per-level table.
#pragma once
#include <cstdint>
#include <vector>

namespace cosdev {

// columns the nested table must save over the per-level one before a handle builds it by default (tuning knob walk_table_nested = 1):
// a second operand and a second adjacency array are not worth a GEMM that is a few microseconds either way
constexpr uint32_t TABLE_NESTED_MIN_SAVED_COLS = 4096u;

constexpr uint32_t TABLE_NESTED_NONE = 0xFFFFFFFFu;

inline uint32_t table_nested_bits(uint32_t v) { // bits needed to hold the values 0 ... v
    uint32_t b = 0;
    for (; v; v >>= 1) b++;
    return b;
}

// the word of LevelDev::adj_tab: `node` below 2^node_bits, the empty marker of adj_node (any value >= n) is kept as it is
inline uint32_t table_nested_pack(uint32_t node, uint32_t col, uint32_t node_bits) { return node | (col << node_bits); }

struct NestedTable {
    uint32_t level_min = 0, level_top = 0, cols = 0;
    std::vector<std::vector<uint32_t>> col; // [level - level_min][node of the level] -> column
    std::vector<uint32_t> node_bits;        // [level - level_min] bits(n_level - 1)
    std::vector<uint32_t> col_node;         // [column] -> node of level_min
};

// n[l], child[l] for level_min <= l <= level_top (child[l][j] = node of level l - 1; child[level_min] is not read).  false = no nested
// table for this graph: a level is empty, a child link is out of range or shared by two nodes (the levels are not nested), or a packed
// word would not fit 32 bits.
inline bool table_nested_columns(uint32_t level_min, uint32_t level_top, const std::vector<uint32_t> &n, const std::vector<std::vector<uint32_t>> &child,
                                 NestedTable *out) {
    if (level_min == 0 || level_top < level_min || n.size() <= level_top || child.size() <= level_top) return false;
    NestedTable t;
    t.level_min = level_min;
    t.level_top = level_top;
    t.cols = n[level_min];
    const uint32_t nl = level_top - level_min + 1;
    t.col.resize(nl);
    t.node_bits.resize(nl);
    for (uint32_t l = level_min; l <= level_top; l++) {
        if (n[l] == 0 || n[l] > t.cols) return false;
        t.node_bits[l - level_min] = table_nested_bits(n[l] - 1u);
        if (t.node_bits[l - level_min] + table_nested_bits(t.cols - 1u) > 32u) return false;
    }
    std::vector<uint32_t> &top = t.col[nl - 1];
    top.resize(n[level_top]);
    for (uint32_t j = 0; j < n[level_top]; j++) top[j] = j;
    for (uint32_t l = level_top; l > level_min; l--) {
        const std::vector<uint32_t> &up = t.col[l - level_min];
        std::vector<uint32_t> &dn = t.col[l - 1 - level_min];
        if (child[l].size() != n[l] || n[l - 1] < n[l]) return false;
        dn.assign(n[l - 1], TABLE_NESTED_NONE);
        for (uint32_t j = 0; j < n[l]; j++) {
            const uint32_t c = child[l][j];
            if (c >= n[l - 1] || dn[c] != TABLE_NESTED_NONE) return false;
            dn[c] = up[j];
        }
        uint32_t next = n[l]; // the nodes that level l - 1 adds, in its own order
        for (uint32_t i = 0; i < n[l - 1]; i++)
            if (dn[i] == TABLE_NESTED_NONE) dn[i] = next++;
    }
    t.col_node.assign(t.cols, 0u);
    for (uint32_t i = 0; i < t.cols; i++) t.col_node[t.col[0][i]] = i;
    *out = std::move(t);
    return true;
}

} // namespace cosdev
