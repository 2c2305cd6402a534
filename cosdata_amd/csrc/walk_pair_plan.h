// walk_pair_plan.h — whether the last level range of a launch is walked by walk_pair_kernel (kernels_walk_pair.hip: two sorted
// neighbours per workgroup, sharing integer dots through LDS) instead of walk_kernel.  Decided after walk_plan.h has settled the launch
// and on top of it; plain integer logic like walk_plan.h (no HIP, no handle, no global), checked by tests/cxx/walk_pair_plan_check.cpp.
#pragma once
#include "walk_plan.h"

namespace cosdev {

// Rule 1, a disclosed heuristic with two measured points, both on 32 768-query launches (profiles/walk_pair_probe_*.jsonl):
//   * launches of fewer than WALK_PAIR_MIN_B queries have too few neighbours per region of the graph for a partner's rows to be the own ones;
//   * the launch must be SPARSE in the corpus, WALK_PAIR_MIN_ROWS_PER_QUERY vectors per query or more.  Where it is dense (1M x 768:
//     30 vectors per query) the locality order already finds the neighbours' rows in an L2 — fabric reads are 0.64 of the algorithmic
//     bytes, the lower range is not bound by the fabric — and the pair kernel's fewer resident waves cost more than its hits save
//     (0.29 of the evaluations hit, the step 0.7 % slower).  Where it is sparse (12.5M x 1024: 381 per query) every row crosses the
//     fabric once per query that wants it, and a pair saves what one of its waves fetches for both (ef 112: the step 2.9 % faster;
//     ef 64, the pair kernel switched on by hand with knob 2 — the rule selects it there too —: 4.1 %).  The threshold is the geometric
//     middle of the two measured ends; nothing between them was measured, so n / B stands in for "bound by the fabric" on those two shapes only.
constexpr uint32_t WALK_PAIR_MIN_B = 8192u, WALK_PAIR_MIN_ROWS_PER_QUERY = 128u;
constexpr uint32_t WALK_PAIR_CACHE_MIN = 64u, WALK_PAIR_CACHE_MAX = 2048u; // entries per query (8 bytes each), a power of two
constexpr uint32_t WALK_PAIR_MAX_LDS = 64u << 10;                          // dynamic LDS of one workgroup (two waves) without raising the kernel's limit

// LDS of one wave of the pair kernel: where its dot cache starts (walk_kernel's layout for the integer engines — filter 8 x mmax, popped
// list 8 x ef, winners 512, window 3 x 4 x 64 x 4, 16 bytes of slack — rounded up to 16) and where it ends.  mmax: the widest neighbour
// row among the levels of the last range.  launch_walk_pair lays the wave out with these and checks them against walk_smem_bytes.
inline uint32_t walk_pair_cache_off(uint32_t mmax, uint32_t ef) { return ((mmax * 8u + ef * 8u + 512u + 3072u + 15u) & ~15u) + 16u; }
inline uint32_t walk_pair_wave_bytes(uint32_t mmax, uint32_t ef, uint32_t cache_entries) { return walk_pair_cache_off(mmax, ef) + cache_entries * 8u; }

struct WalkPairIn {
    uint32_t mode;          // tuning knob walk_pair, resolved: 0 never | 1 by the rule below | 2 at every launch size (tests)
    uint32_t cache_entries; // tuning knob walk_pair_cache, resolved
    uint32_t last_first;    // the highest level of the launch's last range (the level under the last order key level)
    uint32_t n_vectors;     // vectors of the graph
};

// -> cache entries per query, 0 = walk_kernel walks the last range as before.
// The pair kernel's domain: a split, ordered walk by the throughput kernel; u8 codes of one chunk pass on the one-row-per-pass path
// (G = 64, at most 1024 dimensions); pools of up to 256 keys; reference filter; no metadata schema; every level of the last range a
// row level that reads its norms beside the adjacency.
inline uint32_t walk_pair_plan(const WalkPlanIn &in, const WalkPlan &p, const WalkPairIn &pi) {
    if (pi.mode == 0u) return 0u;
    if (pi.mode == 1u && (in.B < WALK_PAIR_MIN_B || (uint64_t)in.B * WALK_PAIR_MIN_ROWS_PER_QUERY > pi.n_vectors)) return 0u;
    if (!p.ordered || p.kernel != WalkKernel::Throughput) return 0u;
    if (in.eng != WALK_PLAN_ENG_U8 || in.G != 64u || in.nchunks == 0u || in.nchunks > 64u) return 0u;
    if (in.ef == 0u || in.ef > 256u || in.visited_mode != 0u || in.mdim != 0u || in.no_self_seed) return 0u;
    if (in.B < 2u || pi.last_first >= in.num_layers) return 0u;
    if (p.use_table && p.table_level_min <= pi.last_first) return 0u;
    for (uint32_t l = 0; l <= pi.last_first; l++)
        if (!((p.use_adj_mag >> l) & 1u)) return 0u;
    const uint32_t c = pi.cache_entries;
    uint32_t mmax = 1u;
    for (uint32_t l = 0; l <= pi.last_first; l++) mmax = std::max(mmax, in.M[l]);
    if (mmax > 4096u) return 0u;
    if (c < WALK_PAIR_CACHE_MIN || c > WALK_PAIR_CACHE_MAX || (c & (c - 1u)) != 0u) return 0u;
    if (2u * walk_pair_wave_bytes(mmax, in.ef, c) > WALK_PAIR_MAX_LDS) return 0u; // (the two waves' LDS must fit: otherwise walk_kernel, like everything outside the domain)
    return c;
}

} // namespace cosdev
