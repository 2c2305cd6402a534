// kernels_walk_pair.hip — walk_pair_kernel: the throughput walk (walk_kernel.inc, compiled here a second time under WALK_PAIR) for the
// LAST level range of a locality-ordered launch, two queries per workgroup.
//
// A big launch holds several queries per region of the graph (the 12.5M x 1024 shard: 32 768 queries over 12 500 clusters), sorted
// neighbours evaluate almost the same code rows, and the lower range is bound by the bytes of those rows.  A workgroup here is two waves
// that walk q_order[2b] and q_order[2b + 1], each exactly as walk_kernel walks it; every code row a wave fetches is dotted with BOTH
// queries and the partner's integer dot goes into the partner's LDS cache, where the partner's winners look before they fetch a row.
// The cached integer is the one the row block would compute, so every key, list and result keeps its bits; what changes is how many
// rows cross the fabric.  No barrier: a wave that returns early leaves its partner walking alone.
//
// Domain (walk_pair_plan.h decides): u8 codes, one chunk pass of 64 lanes, pools of up to 256 keys, reference filter, eight rows in
// flight.  A translation unit of its own, so that walk_kernel's instantiations (kernels_walk.hip) keep their registers.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_types.h"
#include "walk_common.h"
#include "walk_pair_plan.h"

using namespace cosdev;

namespace {

#define WALK_PAIR 1
#include "walk_kernel.inc"

} // namespace

namespace cosdev {

size_t walk_smem_bytes(const IndexDev &ix, u32 ef, int eng, u32 mmax, u32 win_bytes); // kernels_walk.hip

// wa: the last range of an ordered launch (phase 1, q_order dealt in units of two: launch_walk_order).  cache_entries: a power of two,
// WALK_PAIR_CACHE_MIN..WALK_PAIR_CACHE_MAX entries of 8 bytes per query (walk_pair_plan has checked that the two waves' LDS fits).
// Always eight rows in flight, and the pool width follows ef alone: tuning knobs walk_pb and walk_r2, which launch_walk_r honours, are
// not read here.  Results do not depend on either, but with one of them set an A/B of walk_pair compares different instantiations.
hipError_t launch_walk_pair(const IndexDev &ix, const WalkArgs &wa_in, u32 cache_entries, u64 *out_pair, hipStream_t st) {
    if (wa_in.B == 0) return hipSuccess;
    if (cache_entries < WALK_PAIR_CACHE_MIN || cache_entries > WALK_PAIR_CACHE_MAX || (cache_entries & (cache_entries - 1u)) != 0u) return hipErrorInvalidValue;
    if (ix.G != 64u || ix.nchunks > 64u || wa_in.ef == 0u || wa_in.ef > 256u || ix.visited_mode != 0u) return hipErrorInvalidValue;
    WalkArgs wa = wa_in;
    wa.merge_min = 0u; // (a table level in this range — none where the plan sends a launch here — takes the serial insert: same pool)
    const u32 lf = wa.phase ? wa.level_first : ix.num_layers, ll = wa.phase ? wa.level_last : 0u;
    u32 mmax = 1;
    for (u32 l = ll; l <= lf; l++) mmax = std::max(mmax, ix.lv[l].M);
    wa.smem_mmax = mmax;
    wa.smem_win_bytes = (u32)(LA * 64 * 4 * 3);
    WalkPairArgs pa{};
    pa.cache_off = walk_pair_cache_off(mmax, wa.ef);
    pa.wave_bytes = walk_pair_wave_bytes(mmax, wa.ef, cache_entries);
    if (pa.cache_off < walk_smem_bytes(ix, wa.ef, ENG_U8, mmax, wa.smem_win_bytes)) return hipErrorInvalidValue; // (walk_pair_plan.h restates walk_kernel's layout)
    pa.cache_bits = (u32)__builtin_ctz(cache_entries);
    pa.out_pair = out_pair;
    const size_t smem = (size_t)pa.wave_bytes * 2;
    if (smem > WALK_PAIR_MAX_LDS) return hipErrorInvalidValue;
    const dim3 grid((wa.B + 1u) / 2u), block(128);
    if (wa.ef <= 64) hipLaunchKernelGGL((walk_pair_kernel<ENG_U8, 1, 1, true, false, 8>), grid, block, smem, st, ix, wa, pa);
    else if (wa.ef <= 128) hipLaunchKernelGGL((walk_pair_kernel<ENG_U8, 1, 2, true, false, 8>), grid, block, smem, st, ix, wa, pa);
    else hipLaunchKernelGGL((walk_pair_kernel<ENG_U8, 1, 4, true, false, 8>), grid, block, smem, st, ix, wa, pa);
    return hipGetLastError();
}

} // namespace cosdev
