// merge_plan.h — the host-only part of the S-way merge of per-shard lists (kernels_misc.hip: cos_merge_topk_*, cos_merge_lists_*):
// which kernel sorts the S * k keys of a query and how wide it is.  Plain C++17, no HIP header and no handle, so that a stand-alone
// program can check it (tests/cxx/merge_plan_check.cpp).
#pragma once
#include <cstdint>

namespace merge_plan {

// cos_status values of include/cosdata_hip.h, restated so that the header stands alone (kernels_misc.hip asserts that they agree)
constexpr int32_t OK = 0, INVALID = 3, UNIMPLEMENTED = 4;

constexpr uint32_t WAVE_MAX_KEYS = 1024; // merge_topk_kernel<R>: one wave per query, R = 1, 2, 4, 8, 16 keys per lane in registers
constexpr uint32_t LDS_MAX_KEYS = 8192;  // merge_lists_lds_kernel<N>: one workgroup per query, N = 2048, 4096, 8192 keys (8 bytes each) in LDS
constexpr uint32_t LDS_THREADS = 256;    // ... of this many threads

enum class Kind { WAVE, LDS, REFUSED };
struct Plan {
    Kind kind;
    uint32_t width;  // WAVE: R, keys per lane; LDS: N, keys in LDS; REFUSED: 0
    int32_t status;  // OK, or what the entry point returns
    uint64_t keys;   // S * k
    uint32_t lds_bytes() const { return kind == Kind::LDS ? width * 8u : 0u; }
};

// max_keys: WAVE_MAX_KEYS for cos_merge_topk_* (the entry points that never leave the wave kernel), LDS_MAX_KEYS for cos_merge_lists_*
inline Plan plan(uint32_t S, uint32_t k, uint32_t max_keys) {
    const uint64_t keys = (uint64_t)S * (uint64_t)k; // S and k are any u32: the product does not fit 32 bits
    if (S == 0 || k == 0) return {Kind::REFUSED, 0u, INVALID, keys};
    if (keys > (uint64_t)max_keys) return {Kind::REFUSED, 0u, UNIMPLEMENTED, keys};
    if (keys <= WAVE_MAX_KEYS) {
        uint32_t R = 1;
        while ((uint64_t)R * 64u < keys) R *= 2;
        return {Kind::WAVE, R, OK, keys};
    }
    uint32_t N = 2 * WAVE_MAX_KEYS;
    while ((uint64_t)N < keys) N *= 2;
    return {Kind::LDS, N, OK, keys};
}

} // namespace merge_plan
