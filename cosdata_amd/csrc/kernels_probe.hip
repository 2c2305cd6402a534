// kernels_probe.hip — empirical HBM ceilings for the roofline report ("measure an empirical
// peak with a device copy/triad kernel and report fraction of both").  Two access patterns:
//   kind 0  streaming read  : every byte of the buffer once, 16 B per lane, fully coalesced
//   kind 1  streaming copy  : read + write (the classic "copy" figure; bytes counted both ways)
//   kind 2  random row gather: one wave fetches one row of row_bytes at a pseudo-random index, GATHER_INFLIGHT
//                              rows in flight per wave — the access pattern of the HNSW walk (one quantized
//                              vector per distance evaluation), i.e. the practical ceiling for walk_kernel.
// Diagnostic only: not on the search path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_internal.h"

namespace {

__global__ __launch_bounds__(256) void stream_read_kernel(const uint4 *__restrict__ src, u64 n16, u32 *__restrict__ sink) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u32 acc = 0;
    for (; i + 3 * stride < n16; i += 4 * stride) { // 4 independent 16 B loads in flight per lane
        const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
    }
    for (; i < n16; i += stride) {
        const uint4 a = src[i];
        acc ^= a.x ^ a.y ^ a.z ^ a.w;
    }
    if (acc == 0x9E3779B9u) sink[0] = acc; // keeps the loads alive without a store per thread
}

__global__ __launch_bounds__(256) void stream_copy_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, u64 n16) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        dst[i] = a;
        dst[i + stride] = b;
        dst[i + 2 * stride] = c;
        dst[i + 3 * stride] = d;
    }
    for (; i < n16; i += stride) dst[i] = src[i];
}

__device__ __forceinline__ u32 mix32(u32 x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

constexpr int GATHER_INFLIGHT = 8;

// one wave per "query": rows_per_wave rows, GATHER_INFLIGHT outstanding; lanes*16 B cover a row (row_bytes <= 1024)
__global__ __launch_bounds__(256) void row_gather_kernel(const uint8_t *__restrict__ base, u32 n_rows, u32 row_bytes, u32 rows_per_wave,
                                                         u32 *__restrict__ sink) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const bool active = lane * 16u < row_bytes;
    u32 acc = 0;
    for (u32 it = 0; it < rows_per_wave; it += GATHER_INFLIGHT) {
        uint4 v[GATHER_INFLIGHT];
#pragma unroll
        for (int j = 0; j < GATHER_INFLIGHT; j++) {
            const u32 r = mix32(wave * 0x9E3779B1u + it + j) % n_rows;
            v[j] = active ? *reinterpret_cast<const uint4 *>(base + (u64)r * row_bytes + lane * 16u) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < GATHER_INFLIGHT; j++) acc ^= v[j].x ^ v[j].y ^ v[j].z ^ v[j].w;
    }
    if (acc == 0x9E3779B9u) sink[1] = acc;
}

} // namespace

extern "C" int32_t cos_hbm_probe(int32_t device, uint32_t kind, uint64_t buffer_bytes, uint32_t row_bytes, uint32_t iters, double *out_gbps) {
    if (!out_gbps || kind > 2 || buffer_bytes < (1ull << 20) || iters == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (kind == 2 && (row_bytes == 0 || row_bytes > 1024 || row_bytes % 16 != 0)) return cos_fail(COS_ERR_INVALID, "row_bytes must be a multiple of 16, <= 1024");
    HIP_TRY(hipSetDevice(device));
    struct Run { // stream and events of one probe; declared before the buffers, so they outlive them
        hipStream_t st = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Run() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (st) (void)hipStreamDestroy(st);
        }
    } run;
    hipStream_t &st = run.st;
    hipEvent_t &e0 = run.e0, &e1 = run.e1;
    DevArr<uint8_t> buf, dst;
    DevArr<u32> sink;
    buffer_bytes &= ~0xFFFull;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(buf.alloc(buffer_bytes));
    HIP_TRY(sink.alloc(16));
    HIP_TRY(hipMemsetAsync(buf, 0x5A, buffer_bytes, st));
    if (kind == 1) {
        HIP_TRY(dst.alloc(buffer_bytes));
        HIP_TRY(hipMemsetAsync(dst, 0, buffer_bytes, st));
    }
    const u64 n16 = buffer_bytes / 16;
    const u32 n_rows = kind == 2 ? (u32)std::min<u64>(buffer_bytes / row_bytes, 0xFFFFFFFFull) : 0;
    const u32 rows_per_wave = 4096, gather_waves = 32768; // 128 M row fetches per launch
    double bytes_per_launch = 0;
    auto launch = [&]() {
        if (kind == 0) {
            hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 32), dim3(256), 0, st, (const uint4 *)buf.p, n16, sink.p);
            bytes_per_launch = (double)buffer_bytes;
        } else if (kind == 1) {
            hipLaunchKernelGGL(stream_copy_kernel, dim3(256 * 32), dim3(256), 0, st, (const uint4 *)buf.p, (uint4 *)dst.p, n16);
            bytes_per_launch = 2.0 * (double)buffer_bytes;
        } else {
            hipLaunchKernelGGL(row_gather_kernel, dim3(gather_waves / 4), dim3(256), 0, st, buf.p, n_rows, row_bytes, rows_per_wave, sink.p);
            bytes_per_launch = (double)gather_waves * rows_per_wave * row_bytes;
        }
    };
    launch(); // warm-up (TLB, clocks)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e0, st));
    for (u32 i = 0; i < iters; i++) launch();
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *out_gbps = bytes_per_launch * iters / ((double)ms * 1e-3) / 1e9;
    return COS_OK;
}
