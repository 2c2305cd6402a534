// Shared between kernels_flat.hip (host flow, tile kernel) and kernels_scan.hip (query-resident scan kernels).
#pragma once
#include <hip/hip_runtime.h>

#include "engine_types.h"
#include "flat_plan.h"

namespace cosdev {

// Threshold-filtered epilogue (FUSED): instead of writing the [B][chunk] score matrix to HBM for a second kernel to select from
// (10 GB written + 10 GB re-read per 256 x 10M scan against 1.9 GB of codes), every score is compared with its query's current
// SEL-th best key and only the rare survivors are appended to app[B][cap] through a per-query counter.  A reciprocal-based
// estimate (4 VALU ops) screens the elements; the exact IEEE quotient — the value that is ranked — is formed only for those
// within 4e-6 of the threshold or above it, so results are identical to the unfused path.
// Row masks of a masked scan (cos_flat_search_masked_batch, cos_bruteforce_topk_masked): query q may only be given rows whose bit is set
// in mask qmask[q].  The masks are the call's EFFECTIVE ones — the caller's allow-lists AND NOT the handle's deleted set, padding bits
// cleared — built once per call (launch_scan_mask_build).  Only the MASKED instantiations of the kernels read them; bits == nullptr
// is the unmasked call, which launches the unmasked instantiations.
struct ScanMask {
    const u32 *bits;  // [G][words]: bit (r % 32) of word r / 32 = row r is live
    const u32 *qmask; // [B] -> mask index
    u32 words;        // ceil(n / 32)
};
// The test sits where a candidate is about to be kept (a pool, the append buffer, the staging area of the query-resident kernels): a
// pool only ever holds live rows, so a query's threshold is the one of its live rows and the appends per chunk do not grow.
template <bool MASKED>
__device__ __forceinline__ bool scan_live(const ScanMask &m, u32 q, u32 row) {
    if constexpr (!MASKED) return true;
    else return ((m.bits[(u64)m.qmask[q] * m.words + (row >> 5)] >> (row & 31u)) & 1u) != 0u;
}

struct FusedOut {
    const u64 *thr;   // [B] SEL-th best (key) so far; 0 = pool not full yet, everything passes
    u64 *app;         // [B][cap]
    u32 *app_cnt;     // [B]
    u32 cap;
    const uint8_t *qdigits; // bit-plane codes (binary, quaternary, octal): [B][kdims] pre-expanded query digits (expand_digits_kernel)
    ScanMask m;       // masked instantiations only
};


// query-resident scan of bit-plane codes (kernels_scan.hip): eng = ENG_Q1 (binary), ENG_Q2 (quaternary) or ENG_Q3 (octal); kdims = the
// dims multiplied, a multiple of 64 (a 16-byte chunk of a row holds 128, 64 or 32 of them)
bool flat_scan_supported(u32 kdims);
// the same per storage: octal codes of 16 digit chunks (993..1024 dims) stay on the tile kernel — their i8 kernel holds 256 AccVGPRs of
// query fragments and six raw dwords per staged chunk, spills, and measured slower than the tile kernel
bool flat_scan_supported(int eng, u32 kdims);
// queries' planes -> permuted digit bytes [B][kdims] (the layout the scan kernel multiplies)
// (fp4, binary and quaternary: the operands as e2m1 nibbles for the scaled MFMA — flat_scan_q2_fp4 — instead of i8 digits; the buffer is
// half as long.  Octal digits 5 and 7 have no e2m1 code: i8 only)
hipError_t launch_flat_scan_expand_queries(int eng, const uint8_t *qcodes, u64 row_stride, u32 B, u32 kdims, uint8_t *digits, hipStream_t st, bool fp4);
hipError_t launch_flat_scan(int eng, u32 kdims, u32 n_cus, hipStream_t st, const uint8_t *qdig, const float *qmags, u32 B, const uint8_t *codes,
                            const float *mags, u64 row_stride, u32 n0, u32 nc, u32 metric, const FusedOut &fo, bool fp4);

// the same for u8 codes (flat_scan_u8_areg): qcodes = the queries' code rows [B][kdims], qsums / csums = code sums; rows must be exactly kdims bytes
hipError_t launch_flat_scan_u8(u32 kdims, u32 n_cus, hipStream_t st, const uint8_t *qcodes, const u32 *qsums, const float *qmags, u32 B, const uint8_t *codes,
                               const u32 *csums, const float *mags, u64 row_stride, u32 n0, u32 nc, u32 metric, const FusedOut &fo);

// Survivor pools wider than 64 keys (kernels_flat_wide.hip): P = 64 * R keys per query, R = 2, 4, 8, 16, kept sorted (descending) as
// pool[B][P].  The scan kernels are the same at every width: they read thr[q] (the P-th best key, 0 while the pool is not full) and
// append to app[B][cap].  R = 1 stays on the kernels of kernels_flat.hip.
// FLAT_SEED, the fused schedule of a pool of P keys (flat_growth, flat_app_cap) and the pool widths (flat_pool_width) are host numbers:
// flat_plan.h, with the rest of what a scan decides between its launches
using flat_plan::FLAT_SEED;
using flat_plan::flat_app_cap;
using flat_plan::flat_growth;
using flat_plan::flat_pool_width;
// score chunk [B][nc] -> per-segment top P (part[B][S][P]) -> merged into pool[B][P]; thr[q] = the pool's P-th best.  m.bits set: rows
// outside a query's mask are skipped
hipError_t launch_flat_select_wide(u32 R, const float *d_scores, u64 s_stride, u32 B, u32 n0, u32 nc, u64 *d_part, u32 S, u64 *d_pool, u64 *d_thr,
                                   hipStream_t st, const ScanMask &m);
// fold of the fused scan's append buffer (entries past `cap` were dropped: *d_overflow |= 1), new thresholds, counters cleared
hipError_t launch_flat_append_wide(u32 R, const u64 *d_app, u32 *d_appcnt, u32 cap, u32 B, u64 *d_pool, u64 *d_thr, u32 *d_overflow, hipStream_t st);
// exact re-score against the raw rows, sort, top k.  brute = false: the best min(have, ncand_max) of the pool, out_counts set (code scan);
// brute = true: every survivor, ~0 / 0.0 where there is none, out_counts unused (brute force)
hipError_t launch_flat_rerank_wide(u32 R, bool brute, const float *Q, u64 q_stride, const float *qmags, u32 B, const float *X, u64 x_stride,
                                   const float *xmags, u32 dim, const u64 *d_pool, u32 ncand_max, u32 k, u32 id_base, u32 *out_ids, float *out_scores,
                                   u32 *out_counts, hipStream_t st);

// the walk's level table as a query-resident GEMM (kernels_scan.hip): tab[q][c] = (f32) exact integer dot; u8 or quaternary codes.
// Its workgroups claim work items from *queue (zeroed before the first launch over it); wgs = workgroups of this launch, 0 = full width
bool level_table_areg_supported(int eng, u64 row_stride);
hipError_t launch_level_table_areg(int eng, u32 n_cus, hipStream_t st, const uint8_t *qcodes, const u32 *qsums, u32 B, const uint8_t *tcodes,
                                   const u32 *tcsums, u64 row_stride, u32 ncols, float *tab, u64 tab_stride, u32 *queue, u32 wgs, bool shared);

} // namespace cosdev
