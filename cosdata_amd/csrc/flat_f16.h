// flat_f16.h — what the f16 scans share: kernels_flat_f16.hip (cos_flat_search_f16_batch, every row), kernels_flat_f16_masked.hip
// (cos_flat_search_f16_masked_batch, each query's live rows) and kernels_flat_f16_dot.hip (cos_flat_search_f16_dot_batch, the
// dot-product metric, masked or not).  The tile geometry, the fragment helpers of the scan kernels, the handle's workspace, the
// re-score launch and the masked calls' prepare step; each scan kernel and its host flow stay in their own file.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include "engine_internal.h"
#include "flat_scan.h"

namespace cosdev {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

constexpr int F_ROWS = 64, F_PAN = 256;                 // stored rows per tile, dims per k panel
constexpr int F_LDP = F_PAN * 2 + 16;                   // bytes per row of a panel in LDS: 528 = 132 dwords, conflict-free ds_read_b128
constexpr int F_NP = F_ROWS * (F_PAN / 8) / 256;        // 16-byte pieces per thread and panel: 8
constexpr size_t F16_SCAN_LDS = (size_t)2 * F_ROWS * F_LDP; // 67 584 B
constexpr int F_MAX_NPAN = 4;                           // resident fragments: up to 1024 dims
static_assert(F_ROWS == (int)flat_plan::F16_TILE_ROWS, "flat_plan.h sizes the tile lists by this tile");

// the first `keep` halves of a piece survive, the rest become +0.0 (keep >= 2 * words: unchanged)
__device__ __forceinline__ u32 keep_word(u32 w, int keep) { return keep >= 2 ? w : keep == 1 ? (w & 0xFFFFu) : 0u; }
__device__ __forceinline__ i32x4 keep_halves(i32x4 v, int keep) {
    v[0] = (int)keep_word((u32)v[0], keep);
    v[1] = (int)keep_word((u32)v[1], keep - 2);
    v[2] = (int)keep_word((u32)v[2], keep - 4);
    v[3] = (int)keep_word((u32)v[3], keep - 6);
    return v;
}

// (accumulators in VGPRs, fragments used straight from AccVGPRs: both translation units are compiled with
// -mllvm -amdgpu-mfma-vgpr-form=1, kernels_scan.hip areg_mfma has the story)
__device__ __forceinline__ void mfma16(f32x16 &acc, const i32x4 &a, const i32x4 &b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}
__device__ __forceinline__ void mfma8(f32x16 &acc, const i32x2 &a, const i32x2 &b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x8f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), acc, 0, 0, 0);
}

// the query's f16 code widened into LDS (exact): what f16_lane_dot multiplies the stored halves with
__device__ __forceinline__ void stage_f16_query(float *qf, const uint8_t *__restrict__ qrow, u32 dim) {
    for (u32 i = threadIdx.x; i < dim; i += blockDim.x) qf[i] = __half2float(((const __half *)qrow)[i]);
    __syncthreads();
}

// the pool's rows again in the reference's order, sorted (kernels_flat_f16.hip f16_rescore): empty keys stay empty and sort last
hipError_t launch_f16_rescore(u32 P, const uint8_t *qh, u64 row_stride, const float *qmags, u32 B, const uint8_t *codes, const float *mags, u32 dim,
                              const u64 *pool, u64 *sorted, hipStream_t st);

// a masked call's device buffers (kernels_flat_f16_masked.hip f16m_prepare writes all but the first four): grow-only
struct FlatF16MaskBufs {
    DevArr<u32> user, qmask, blk_off, blk_masks; // uploaded: the masks in use [G][words], [B] -> mask, the masks of query block b
    DevArr<u32> eff, uni, live;                  // [G][words] effective words, [words] their OR, [G] live rows
    DevArr<u64> tile_bits;                       // [G][ceil(tiles / 64)]: bit t = tile t holds a live row of mask g
    DevArr<u32> lists, list_len;                 // [blocks][tiles] the live tiles of a query block, ascending; [blocks] how many
    std::vector<u32> h_blk_off, h_blk_masks;     // what blk_off / blk_masks are uploaded from: alive until the stream has read them
};
// the same buffers as a call's kernels take them (f16_mask_prepare below fills it)
struct F16MaskDev {
    ScanMask sm;                 // the effective words and [B] -> mask
    const u32 *uni, *live;       // [words] the OR of the effective words, [G] live rows
    const u64 *tile_bits;        // [G][tb_stride]
    u32 tb_stride;
    const u32 *lists, *list_len; // [blocks][tiles], [blocks]
    u32 tiles, blocks;
};

}  // namespace cosdev

// Per-index workspace of the two f16 calls, beside FlatWs: grow-only, sized and indexed by each call's own P, released with it
struct FlatF16Ws {
    std::mutex mu; // the scan runs on the index's own stream: one call at a time
    DevArr<float> q, qm, qrm, os, scores;
    DevArr<uint8_t> qc;
    DevArr<u32> flags /*[zero-norm, overflow, queries flagged]*/, appcnt, oi, oc, qflag;
    DevArr<u64> pool, sorted, thr, app, part;
    cosdev::FlatF16MaskBufs mask;           // the masked call's; empty until one is made
    bool zn_valid = false, zn_zero = false; // "a stored vector has a zero norm" for the current rows (the unmasked call's screen)
    u32 zn_n = 0;
    DevArr<u32> xmax; // the dot-metric call's: bits of the largest norm of the stored f16 rows, rounded up (kernels_flat_f16_dot.hip);
    bool xmax_valid = false; // cached like zn_*: the workspace goes with every upload and append
    u32 xmax_n = 0;
    std::vector<hipEvent_t> evs;
    hipError_t event(size_t i, hipEvent_t *out) {
        while (evs.size() <= i) {
            hipEvent_t ev = nullptr;
            hipError_t e = hipEventCreate(&ev);
            if (e != hipSuccess) return e;
            evs.push_back(ev);
        }
        *out = evs[i];
        return hipSuccess;
    }
    ~FlatF16Ws() {
        for (hipEvent_t ev : evs) (void)hipEventDestroy(ev);
    }
};
// the handle's workspace, created on first use (kernels_flat_f16.hip)
FlatF16Ws *cos_flat_f16_ws(cos_index *ix);
// a masked call's prepare step (kernels_flat_f16_masked.hip): `used` / `qmask` of the call's MaskPlan -> effective words, live counts,
// tile bits and each query block's list of live tiles, all enqueued on st
hipError_t f16_mask_prepare(cos_index *ix, FlatF16Ws *W, const cos_scan_mask *mask, const std::vector<u32> &used, bool skip_deleted,
                            const std::vector<u32> &qmask, u32 B, hipStream_t st, cosdev::F16MaskDev &out);
