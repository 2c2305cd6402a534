// kernels_walk.hip — gfx950 kernels of the dense search path:
//   quantize_rows  : ScalarQuantization::quantize           (quantization/scalar.rs:10-52)
//   walk           : ann_search / traverse_find_nearest     (vector_store.rs:256-402, 1112-1204)
// (what ends the search — dedup, 5k cut, exact rerank — is kernels_finalize.hip)
// One wavefront (64 lanes) owns one query: 64 lanes <-> the <=64 neighbour slots of an expansion
// (level_0_neighbors_count = shortlist_size = 64, config.toml:21,32).  HBM-bound gather work:
// adjacency rows and code rows are read with coalesced 16-byte-per-lane loads; the candidate pool
// lives in registers, the visited filter and the popped list in LDS.  No MFMA here by design.
//
// Compile with -ffp-contract=off: the reference's arithmetic order (fused only where AVX2 FMA is
// used, x86_64.rs:418-444) is reproduced with explicit __fmaf_rn / __fmul_rn / __fadd_rn.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "engine_types.h"
#include "tuning.h"
#include "walk_common.h"
#include "walk_plan.h"

using namespace cosdev;

namespace {

// ------------------------------------------------------------------------------------------------
// quantize_rows: one wave per row.  Writes the DEVICE code layout:
//   U8  : dim bytes, zero padded to a multiple of 16
//   Q2  : per 64-dim chunk 16 bytes = [plane0 (MSB as quantize_to_u8_bits stores it) 8 B | plane1 8 B]
//   F32 : dim floats, zero padded to a multiple of 16 bytes
// ------------------------------------------------------------------------------------------------
template <int ENG>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const float *__restrict__ x, u64 x_stride, u32 n, u32 dim, float lo,
                                                            float hi, uint8_t *__restrict__ codes, u64 row_stride,
                                                            float *__restrict__ mags, float *__restrict__ raw_mags, u32 *__restrict__ code_sums) {
    const int lane = threadIdx.x & 63;
    const u32 row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    const float *xr = x + (u64)row * x_stride;
    uint8_t *cr = codes + (u64)row * row_stride;
    float rn = 0.0f;
    const bool need_seq = (raw_mags != nullptr) || (ENG != ENG_U8);
    if (need_seq) rn = seq_norm_wave(xr, dim, lane); // wave-uniform branch; every lane gets the value
    if (raw_mags && lane == 0) raw_mags[row] = rn;
    if constexpr (ENG == ENG_U8) {
        u32 ss = 0, sum = 0; // (sum: the level-table GEMM's recentring term of a query, engine.hip run_search)
        for (u32 i = lane; i < (u32)row_stride; i += 64) {
            uint8_t q = 0;
            if (i < dim) {
                float c = rust_min(rust_max(xr[i], lo), hi);
                float v = __fmul_rn(__fdiv_rn(__fsub_rn(c, lo), __fsub_rn(hi, lo)), 255.0f);
                q = rust_f32_as_u8(v);
            }
            cr[i] = q;
            ss += (u32)q * (u32)q;
            sum += (u32)q;
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) ss += (u32)__shfl_xor((int)ss, m, 64);
        if (lane == 0) mags[row] = sqrtf((float)ss); // (sum::<u32>() as f32).sqrt()
        if (code_sums) { // wave-uniform
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) sum += (u32)__shfl_xor((int)sum, m, 64);
            if (lane == 0) code_sums[row] = sum;
        }
    } else if constexpr (ENG == ENG_Q2) {
        const u32 nch = (u32)(row_stride / 16);
        for (u32 c = 0; c < nch; c++) {
            u32 i = c * 64 + lane;
            u32 lvl = 0;
            if (i < dim) lvl = rust_f32_as_usize_low2(floorf(__fdiv_rn(__fadd_rn(xr[i], 1.0f), 0.5f))); // step = 2/4
            u64 p0 = __ballot((lvl >> 1) & 1u); // plane 0 = MSB (common.rs:230-233)
            u64 p1 = __ballot(lvl & 1u);
            if (lane == 0) {
                *(u64 *)(cr + (u64)c * 16) = p0;
                *(u64 *)(cr + (u64)c * 16 + 8) = p1;
            }
        }
        if (lane == 0) mags[row] = rn; // norm of the ORIGINAL vector (scalar.rs:31-32)
    } else if constexpr (ENG == ENG_Q1) {
        // binary: one plane, level = floor((x+1)/1.0) & 1 (common.rs:226-275 with resolution 1); 128 dims per 16 B chunk
        const u32 nch = (u32)(row_stride / 16);
        for (u32 c = 0; c < 2 * nch; c++) {
            const u32 i = c * 64 + lane;
            u32 lvl = 0;
            if (i < dim) lvl = rust_f32_as_usize_low(floorf(__fdiv_rn(__fadd_rn(xr[i], 1.0f), 1.0f)), 1u);
            const u64 p0 = __ballot(lvl & 1u);
            if (lane == 0) *(u64 *)(cr + (u64)c * 8) = p0;
        }
        if (lane == 0) mags[row] = rn;
    } else if constexpr (ENG == ENG_Q3) {
        // octal: three planes, MSB first; 32 dims per 16 B chunk [p0 | p1 | p2 | 0]; one ballot covers two chunks
        const u32 nch = (u32)(row_stride / 16);
        for (u32 c = 0; c < nch; c += 2) {
            const u32 i = c * 32 + lane;
            u32 lvl = 0;
            if (i < dim) lvl = rust_f32_as_usize_low(floorf(__fdiv_rn(__fadd_rn(xr[i], 1.0f), 0.25f)), 7u); // step = 2/8
            const u64 p0 = __ballot((lvl >> 2) & 1u), p1 = __ballot((lvl >> 1) & 1u), p2 = __ballot(lvl & 1u);
            if (lane == 0) {
                *(uint4 *)(cr + (u64)c * 16) = make_uint4((u32)p0, (u32)p1, (u32)p2, 0u);
                if (c + 1 < nch) *(uint4 *)(cr + (u64)(c + 1) * 16) = make_uint4((u32)(p0 >> 32), (u32)(p1 >> 32), (u32)(p2 >> 32), 0u);
            }
        }
        if (lane == 0) mags[row] = rn;
    } else if constexpr (ENG == ENG_F16) {
        __half *ch = (__half *)cr;
        for (u32 i = lane; i < (u32)(row_stride / 2); i += 64) ch[i] = i < dim ? __float2half_rn(xr[i]) : __float2half_rn(0.0f); // f16::from_f32 (RNE)
        if (lane == 0) mags[row] = rn; // norm of the ORIGINAL vector (scalar.rs:41)
    } else {
        float *cf = (float *)cr;
        for (u32 i = lane; i < (u32)(row_stride / 4); i += 64) cf[i] = i < dim ? xr[i] : 0.0f;
        if (lane == 0) mags[row] = rn;
    }
}

#include "walk_kernel.inc"

} // namespace

// ------------------------------------------------------------------------------------------------
// host-side launchers (called from engine.hip)
// ------------------------------------------------------------------------------------------------
namespace cosdev {

hipError_t launch_quantize_rows(int eng, const float *x, u64 x_stride, u32 n, u32 dim, float lo, float hi, uint8_t *codes,
                                u64 row_stride, float *mags, float *raw_mags, hipStream_t st, u32 *code_sums) {
    if (n == 0) return hipSuccess;
    dim3 block(256), grid((n + 3) / 4);
    switch (eng) {
    case ENG_U8: hipLaunchKernelGGL(quantize_rows_kernel<ENG_U8>, grid, block, 0, st, x, x_stride, n, dim, lo, hi, codes, row_stride, mags, raw_mags, code_sums); break;
    case ENG_Q2: hipLaunchKernelGGL(quantize_rows_kernel<ENG_Q2>, grid, block, 0, st, x, x_stride, n, dim, lo, hi, codes, row_stride, mags, raw_mags, code_sums); break;
    case ENG_F32: hipLaunchKernelGGL(quantize_rows_kernel<ENG_F32>, grid, block, 0, st, x, x_stride, n, dim, lo, hi, codes, row_stride, mags, raw_mags, code_sums); break;
    case ENG_F16: hipLaunchKernelGGL(quantize_rows_kernel<ENG_F16>, grid, block, 0, st, x, x_stride, n, dim, lo, hi, codes, row_stride, mags, raw_mags, code_sums); break;
    case ENG_Q1: hipLaunchKernelGGL(quantize_rows_kernel<ENG_Q1>, grid, block, 0, st, x, x_stride, n, dim, lo, hi, codes, row_stride, mags, raw_mags, code_sums); break;
    case ENG_Q3: hipLaunchKernelGGL(quantize_rows_kernel<ENG_Q3>, grid, block, 0, st, x, x_stride, n, dim, lo, hi, codes, row_stride, mags, raw_mags, code_sums); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// LDS of one walk_kernel wave (walk_kernel.inc, WalkSmem): filter | popped list | winners | window | f32 / f16 query
size_t walk_smem_bytes(const IndexDev &ix, u32 ef, int eng, u32 mmax, u32 win_bytes) {
    size_t b = (size_t)mmax * 8 + (size_t)ef * 8 + 64 * 4 * 2 + (size_t)win_bytes;
    b = (b + 15) & ~(size_t)15;
    if (eng == ENG_F32) b += (size_t)ix.row_stride;
    if (eng == ENG_F16) b += ((size_t)ix.dim * 4 + 15) & ~(size_t)15;
    return b + 16;
}

// rows in flight per wave on the G = 64 u8 path (see PB64 above); tuning knob walk_pb = 4|8 overrides the default (experiments).
// The widest pool (ef > 256: 16 VGPRs of pool) with eight row buffers needs 110 VGPRs = 4 waves per SIMD; with four it fits 5 waves
// without spills and measured 3.3 % faster (c2 at ef 512: 50.9 vs 52.6 ms per 32768 queries, profiles/archive/r03_order_probe_c2_ef512_pb4.jsonl).
// The UPPER range of a split walk (tuning knob walk_pb_upper = 4|8 overrides): with the level table that range is almost all table
// levels, which fetch no rows (c2: 91 M table evaluations against 2 M row evaluations), and the four-buffer variant leaves more waves
// per SIMD.  Measured in round 5 (profiles/r05_candidates_walk_pb_upper.txt, c2): ef 64 2.798 against 2.799 ms (nothing: 8 stays),
// ef 256 10.47 against 11.33 ms per 32 768 queries (+4.4 % QPS on the whole step): four buffers above ef 64.
static int walk_pb_policy(u32 B, u32 ef, bool upper_range_of_a_split_walk) {
    const int forced = (int)tune_or(TUNE_WALK_PB, 0), forced_upper = (int)tune_or(TUNE_WALK_PB_UPPER, 0);
    if (upper_range_of_a_split_walk && (forced_upper == 4 || forced_upper == 8)) return forced_upper;
    if (forced == 4 || forced == 8) return forced;
    if (upper_range_of_a_split_walk && ef > 64u) return 4;
    return ef > 256u ? 4 : 8;
}

// Table levels (walk_kernel.inc, commit_merge): winners past the screen from which an expansion takes the ranked merge instead of
// the serial insert.  Tuning knob walk_merge_min overrides (0 = never merge).  Defaults measured in round 6
// (profiles/r06_merge_probe_*.jsonl): one key per lane (ef <= 64) the serial insert is a dozen instructions and only a big batch
// of winners pays for the permutation; from two keys per lane on the merge wins from three winners.
static u32 walk_merge_min_policy(u32 ef) {
    const long long forced = tune_or(TUNE_WALK_MERGE_MIN, -1);
    if (forced >= 0) return (u32)std::min<long long>(forced, 65);
    return ef <= 64u ? 4u : 3u;
}

template <int ENG, int CH, bool G64>
static hipError_t launch_walk_r(const IndexDev &ix, const WalkArgs &wa_in, hipStream_t st) {
    WalkArgs wa = wa_in;
    wa.merge_min = wa.tab != nullptr ? walk_merge_min_policy(wa.ef) : 0u;
    // the LDS of a wave follows the levels THIS launch walks: the filter is as wide as their widest row, and a launch of table levels only
    // (the upper range of a split walk whose cut level is in the table) needs no window staging — just the ranked merge's scratch.  On the
    // metric's shard (M0 256, ef 112) that is 2.9 KB per wave instead of 6.6: the upper range's 60-register waves were capped at 6 per
    // SIMD by LDS, and that range is bound by the gathers in flight (fewer resident waves = proportionally slower:
    // profiles/r06_pad_probe_c4shard.jsonl) — now 8.
    const u32 lf = wa.phase ? wa.level_first : ix.num_layers, ll = wa.phase ? wa.level_last : 0u;
    u32 mmax = 1;
    for (u32 l = ll; l <= lf; l++) mmax = std::max(mmax, ix.lv[l].M);
    constexpr bool TABLE_ENG = ENG == ENG_U8 || ENG == ENG_Q2;
    const bool all_tab = TABLE_ENG && wa.tab != nullptr && ll >= wa.tab_level_min && tune_or(TUNE_WALK_UPPER_LDS_PAD, 0) >= 0;
    wa.smem_mmax = mmax;
    size_t pad = 0;
    // experiment knob: extra (unused) dynamic LDS per wave on the upper range of a split walk = fewer resident waves per CU (negative: the
    // full layout even for table-only launches)
    if (wa.phase != 0u && wa.level_last >= 1u) pad = (size_t)std::max<long long>(0, std::min<long long>(tune_or(TUNE_WALK_UPPER_LDS_PAD, 0), 48 << 10));
    dim3 grid(wa.B), block(64);
    const bool exact = ix.visited_mode != 0;
    constexpr bool HAS_PB8 = ENG == ENG_U8 && G64 && CH == 1; // the headline path (u8, 513..1024 dims)
    const bool pb8 = HAS_PB8 && walk_pb_policy(wa.B, wa.ef, wa.phase != 0u && wa.level_last >= 1u) == 8;
#define WALK(R_)                                                                                                          \
    do {                                                                                                                  \
        wa.smem_win_bytes = (all_tab && (R_) <= 4) ? (u32)(((64 * (R_) + 1) * 8 + 15) & ~15) : (u32)(LA * 64 * 4 * 3);         \
        const size_t smem = walk_smem_bytes(ix, wa.ef, ENG, mmax, wa.smem_win_bytes) + pad;                                \
        if constexpr (HAS_PB8) {                                                                                          \
            if (pb8) {                                                                                                    \
                if (exact) hipLaunchKernelGGL((walk_kernel<ENG, CH, R_, G64, true, 8>), grid, block, smem, st, ix, wa);   \
                else hipLaunchKernelGGL((walk_kernel<ENG, CH, R_, G64, false, 8>), grid, block, smem, st, ix, wa);        \
                break;                                                                                                    \
            }                                                                                                             \
        }                                                                                                                 \
        if (exact) hipLaunchKernelGGL((walk_kernel<ENG, CH, R_, G64, true>), grid, block, smem, st, ix, wa);              \
        else hipLaunchKernelGGL((walk_kernel<ENG, CH, R_, G64, false>), grid, block, smem, st, ix, wa);                   \
    } while (0)
    if (wa.ef <= 64) WALK(1);
    else if (wa.ef <= 128 && tune_or(TUNE_WALK_R2, 1) != 0) WALK(2); // round 6: the metric's shard runs at ef 128 — half the pool registers, half the insert
    else if (wa.ef <= 256) WALK(4);
    else if (wa.ef <= 512) WALK(8);
    else if (wa.ef <= 1024) WALK(16); // round 5: a pool of 64 x 16 keys per wave (103 VGPRs, no scratch: 4 waves per SIMD)
    else return hipErrorInvalidValue;
#undef WALK
    return hipGetLastError();
}

// kernels_walk_lat.hip, kernels_walk_lat4.hip, kernels_walk_general.hip
hipError_t launch_walk_lat(int eng, const IndexDev &ix, const WalkArgs &wa, hipStream_t st);
hipError_t launch_walk_lat4(int eng, const IndexDev &ix, const WalkArgs &wa, hipStream_t st);
hipError_t launch_walk_general(int eng, const IndexDev &ix, const WalkArgs &wa, hipStream_t st);

// `kernel` is the launch plan's choice (walk_plan.h): nothing is decided here
hipError_t launch_walk(int eng, const IndexDev &ix, const WalkArgs &wa, WalkKernel kernel, hipStream_t st) {
    if (wa.B == 0) return hipSuccess;
    if (kernel == WalkKernel::General) return launch_walk_general(eng, ix, wa, st);
    if (kernel == WalkKernel::Lat4) return launch_walk_lat4(eng, ix, wa, st);
    if (kernel == WalkKernel::Lat1) return launch_walk_lat(eng, ix, wa, st);
    const u32 ch = (eng == ENG_F32 || eng == ENG_F16) ? 1 : (ix.nchunks + ix.G - 1) / ix.G;
    switch (eng) {
    case ENG_U8:
        if (ch == 1) return ix.G == 64 ? launch_walk_r<ENG_U8, 1, true>(ix, wa, st) : launch_walk_r<ENG_U8, 1, false>(ix, wa, st);
        if (ch == 2) return launch_walk_r<ENG_U8, 2, true>(ix, wa, st);
        if (ch == 3) return launch_walk_r<ENG_U8, 3, true>(ix, wa, st); // 2049..3072 dimensions (round 6: three chunk passes)
        if (ch == 4) return launch_walk_r<ENG_U8, 4, true>(ix, wa, st); // 3073..4096 dimensions (four; wider rows: walk_general_kernel)
        return hipErrorInvalidValue;
    case ENG_Q2:
        if (ch == 1) return ix.G == 64 ? launch_walk_r<ENG_Q2, 1, true>(ix, wa, st) : launch_walk_r<ENG_Q2, 1, false>(ix, wa, st);
        return hipErrorInvalidValue;
    case ENG_Q1:
        if (ch == 1) return ix.G == 64 ? launch_walk_r<ENG_Q1, 1, true>(ix, wa, st) : launch_walk_r<ENG_Q1, 1, false>(ix, wa, st);
        return hipErrorInvalidValue;
    case ENG_Q3:
        if (ch == 1) return ix.G == 64 ? launch_walk_r<ENG_Q3, 1, true>(ix, wa, st) : launch_walk_r<ENG_Q3, 1, false>(ix, wa, st);
        return hipErrorInvalidValue;
    case ENG_F32: return launch_walk_r<ENG_F32, 1, false>(ix, wa, st);
    case ENG_F16: return launch_walk_r<ENG_F16, 1, false>(ix, wa, st);
    default: return hipErrorInvalidValue;
    }
}

} // namespace cosdev
