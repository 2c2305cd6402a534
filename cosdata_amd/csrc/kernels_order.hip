// kernels_order.hip — the locality order of a big search launch (engine_types.h, WalkArgs::phase).
//
// Between the two launches of a split walk: the launch's queries are sorted by ORDER KEY (written by the upper-level phase: the
// depth-first position of the best node found on the key level) and dealt to the XCDs in contiguous runs.  gfx950 hands workgroup b of a grid to XCD b % 8, and each
// XCD has its own 4 MB L2: with the queries in arrival order every XCD walks the whole graph and no row is found twice in an L2;
// sorted and dealt, the ~600 waves resident on one XCD walk neighbouring regions.  The per-query walk is untouched — the order
// only decides when and where a query's workgroup runs (scripts/locality_probe.py: 11.7 -> 9.6 ms per 32768-query launch with
// an oracle key, every result identical).
//
// Not a reference interface: the reference answers one query per rayon task (indexes/mod.rs:260-272) and has no launch to order.
#include <hipcub/hipcub.hpp>

#include "engine_internal.h"

namespace cosdev {

// num_xcd: the device's XCD count (hipDeviceAttributeNumberOfXccs, read at cos_index_create; MI355X: 8 XCDs x 32 CUs)
// unit: queries per workgroup of the launch that reads q_order — 1 (walk_kernel), or 2 (walk_pair_kernel: workgroup b walks q_order[2b]
// and q_order[2b + 1], which must be neighbours in the sorted order).  The U = B / unit whole units are dealt; what is left of an odd
// launch goes to the workgroup behind them.
__global__ void deal_to_xcds_kernel(const u32 *__restrict__ sorted, u32 B, u32 num_xcd, u32 unit, u32 *__restrict__ q_order) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 U = B / unit;
    if (b > U) return;
    if (b == U) { // (unit 1: nothing is left)
        for (u32 i = U * unit; i < B; i++) q_order[i] = sorted[i];
        return;
    }
    // XCD x receives workgroups x, x + num_xcd, ...: U / num_xcd of them, one more for x < U % num_xcd.  Its run of the sorted order
    // starts after the runs of the XCDs before it.
    const u32 q = U / num_xcd, r = U % num_xcd, x = b % num_xcd, j = b / num_xcd;
    const u32 src = x * q + (x < r ? x : r) + j;
    for (u32 k = 0; k < unit; k++) q_order[b * unit + k] = sorted[src * unit + k];
}

hipError_t walk_order_reserve(WalkOrder &o, u32 B) {
    if (B <= o.cap) return hipSuccess;
    o.cap = 0; // (a failure at any array leaves an order for no query: launch_walk_order refuses, the next reservation starts over)
    hipError_t e;
    for (DevArr<u32> *a : {&o.entry0, &o.order_key, &o.keys_sorted, &o.iota, &o.vals_sorted, &o.q_order})
        if ((e = a->alloc(B)) != hipSuccess) return e;
    size_t bytes = 0;
    if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, o.order_key.p, o.keys_sorted.p, o.iota.p, o.vals_sorted.p, (int)B, 0, 32, (hipStream_t)0)) != hipSuccess)
        return e;
    if ((e = o.tmp.alloc(bytes)) != hipSuccess) return e;
    o.cap = B;
    return hipSuccess;
}

// order_key[0..B) / iota[0..B) (both written by the upper-level phase; keys <= key_max) -> q_order[0..B), all on `st`
hipError_t launch_walk_order(WalkOrder &o, u32 B, u32 key_max, u32 num_xcd, hipStream_t st, u32 unit) {
    if (B > o.cap || unit == 0u) return hipErrorInvalidValue;
    int end_bit = 1;
    while (end_bit < 32 && (key_max >> end_bit)) end_bit++; // radix passes over the bits the keys have
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, o.order_key.p, o.keys_sorted.p, o.iota.p, o.vals_sorted.p, (int)B, 0, end_bit, st);
    if (e != hipSuccess) return e;
    if (bytes > o.tmp.cap) return hipErrorOutOfMemory; // sized for cap >= B items: cannot happen unless the library's sizing is not monotonic
    bytes = o.tmp.cap;
    e = hipcub::DeviceRadixSort::SortPairs(o.tmp.p, bytes, o.order_key.p, o.keys_sorted.p, o.iota.p, o.vals_sorted.p, (int)B, 0, end_bit, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(deal_to_xcds_kernel, dim3((B / unit + 1u + 255u) / 256u), dim3(256), 0, st, o.vals_sorted.p, B, num_xcd ? num_xcd : 1u, unit, o.q_order.p);
    return hipGetLastError();
}

} // namespace cosdev
