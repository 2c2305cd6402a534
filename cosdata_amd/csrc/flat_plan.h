// flat_plan.h — the host-only part of the two exhaustive scans (kernels_flat.hip: cos_flat_search_batch over the quantized codes,
// cos_bruteforce_topk over the f32 rows): the limits, the survivor pool's width, the chunk schedule of an attempt, the buffer sizes
// that follow from it, the kernel that scores a fused chunk of the code scan and the rule that says when the brute force's pool can be
// trusted (brute_margin_safe).  Every number a scan decides before or between its launches.  Plain C++17, no HIP header and no handle, so that a stand-alone program can check it (tests/cxx/flat_plan_check.cpp).
#pragma once
#include <cstdint>

namespace flat_plan {

// cos_status values of include/cosdata_hip.h and the storage engines of device_common.h, restated so that the header stands alone
// (kernels_flat.hip asserts that they agree)
constexpr int32_t OK = 0, INVALID = 3, UNIMPLEMENTED = 4;
constexpr int U8 = 0, Q2 = 1, Q1 = 4, Q3 = 5; // ENG_U8, ENG_Q2 (quaternary), ENG_Q1 (binary), ENG_Q3 (octal)

// ---- survivor pools: P = 64, 128, ..., 1024 keys per query (kernels_flat_wide.hip from 128 up) ----
constexpr uint32_t FLAT_SEED = 16384; // candidates that go through the score matrix first and seed every query's threshold (every width)
// Fused schedule of a pool of P keys: a chunk `growth` times the size of everything seen lets ~growth * P keys per query through (a key
// passes with probability P / seen while the threshold stands), and the append buffer holds eight times that:
//   P = 64        growth 8, cap 64 P = 4096 keys (32 KB per query)
//   P = 128..1024 growth 4, cap 32 P        keys (256 P bytes per query: 32 KB .. 256 KB)
constexpr uint32_t flat_growth(uint32_t P) { return P == 64 ? 8u : 4u; }
constexpr uint32_t flat_app_cap(uint32_t P) { return P == 64 ? 4096u : 32u * P; }
// smallest pool width (64, 128, ..., 1024) that holds `need` keys; 0 when none does
inline uint32_t flat_pool_width(uint32_t need) {
    for (uint32_t P = 64; P <= 1024; P *= 2)
        if (need <= P) return P;
    return 0;
}

// ---- limits ----
// brute force: the f32 MFMA GEMM only generates candidates, so the pool holds at least 2k of them (and is trusted only under the margin
// rule below); k in [1, min(512, n)]
constexpr uint32_t BRUTE_MAX_K = 512, BRUTE_POOL_FACTOR = 2;
inline int32_t check_brute_k(uint32_t k, uint32_t n) { return k == 0 || k > BRUTE_MAX_K || k > n ? INVALID : OK; }
inline uint32_t brute_pool(uint32_t k) { return flat_pool_width(BRUTE_POOL_FACTOR * k); }

// ---- brute force: when the pool that the GEMM's ranking cut can be trusted ----
// The pool holds the P best rows by the GEMM's score g; the answer is the k best by the reference-order score e.  With
// |g - e| <= bound for every row: a row outside a FULL pool has g <= g_P (the pool's P-th score), so e <= g_P + bound, and the k best
// of the pool have e >= g_k - bound.  When g_P + bound < g_k - bound, k rows of the pool beat every row outside it in the exact order
// too, and the exact top k lies in the pool: the query is SAFE.  A pool that is not full holds every (live) row and is always safe.
// Otherwise — more than P - k rows within 2 * bound of the k-th score: copies, scaled copies, boilerplate documents — the pool may
// have dropped rows of the answer, and the call scores every row of that query in the reference's order instead (kernels_flat.hip,
// the exact path).  Scores that are not finite are never safe.
//
// The bound.  u = 2^-24.  Both scores divide by the SAME f32 denominator D = fl(|q| * |x|) (the norms the handle keeps): their
// difference is that of the two f32 dots over D, plus one rounding of each quotient.
//   GEMM dot       one k-ordered chain of dim fused steps (v_mfma_f32_32x32x2_f32): |err| <= dim u S, S = sum |x_i q_i| —
//                  which holds for dim correctly rounded operations in ANY order
//   reference dot  eight chains of dim / 8 fused steps, a pairwise tree of 3, a scalar tail of up to 7 unfused multiply-adds: the
//                  model of tests/odd_dims.py bound_a, |err| <= (dim / 8 + 16) u S
//   two quotients  |g|, |e| <= ~1: 2 u each with the product |q| * |x| rounded once more — 8 u for both, an absolute term
// With S <= |x| |q| (Cauchy-Schwarz) and S / D ~ 1: |g - e| <= ((dim + dim / 8 + 32) + 8) u, the extra 16 u being slack for the chain
// ends.  That figure assumes round-to-nearest at every step and D equal to the true |x| |q|.  Neither is documented: the MFMA's
// internal rounding of its two-term step is not stated by the ISA guide (a truncating step errs by 2 u, not u), and the handle's
// norms are sequential f32 sums whose relative error (up to dim u / 2 each) scales S / D.  The bound therefore takes TWICE the figure —
// a truncating chain, or S / D up to 2 — and the rule twice the bound.  On Gaussian-mixture corpora the k-th and P-th scores are
// hundreds of bounds apart (tests/test_oracle_near_copies.py), so ordinary data never leaves the MFMA path.
// constexpr: the kernel that flags the queries calls the same function (a constexpr function is host and device code under hipcc).
constexpr double brute_margin_bound(uint32_t dim) { return 2.0 * (double)((dim + dim / 8 + 32) + 8) * (1.0 / 16777216.0); }
constexpr bool brute_margin_safe(float kth, float pth, uint32_t dim, bool pool_full) {
    if (!pool_full) return true;
    const double a = (double)kth, b = (double)pth;
    if (!(a - a == 0.0) || !(b - b == 0.0)) return false; // NaN or inf
    return a - b > 2.0 * brute_margin_bound(dim);
}
// tuning knob flat_brute_exact: which queries take the exact path
enum BruteExact : int { BRUTE_EXACT_NEVER = 0, BRUTE_EXACT_BY_RULE = 1, BRUTE_EXACT_ALWAYS = 2 };
// code scan: the pool holds the 5 * top_k candidates of the exact rerank; top_k in [1, 204]
constexpr uint32_t CODE_MAX_TOP_K = 204, CODE_POOL_FACTOR = 5;
inline int32_t check_code_top_k(uint32_t top_k) { return top_k == 0 || top_k > CODE_MAX_TOP_K ? UNIMPLEMENTED : OK; }
inline uint32_t code_pool(uint32_t top_k) { return flat_pool_width(CODE_POOL_FACTOR * top_k); }

// ---- which kernel scores a fused chunk of the code scan ----
enum class ScanKernel {
    RESIDENT_PLANES, // query-resident scan of bit-plane codes (kernels_scan.hip flat_scan_q2_*)
    RESIDENT_U8,     // query-resident scan of u8 codes (flat_scan_u8_areg)
    TILE,            // flat_codes_gemm_i8, 256 x 128 tiles: every storage and row length
};
constexpr bool bit_planes(int eng) { return eng == Q1 || eng == Q2 || eng == Q3; }
// dims the GEMM multiplies, a multiple of 64: a 16-byte chunk of a row holds 128 binary, 64 quaternary or 32 octal dims
inline uint32_t code_kdims(int eng, uint64_t row_stride) {
    if (eng == U8) return (uint32_t)((row_stride + 63) / 64 * 64);
    const uint32_t chunk_k = eng == Q1 ? 128u : eng == Q3 ? 32u : 64u;
    return ((uint32_t)(row_stride / 16) * chunk_k + 63) / 64 * 64;
}
// planes_supported / u8_supported: flat_scan_supported(eng, kdims) / flat_scan_supported(kdims) of flat_scan.h.  The u8 kernel wants
// rows of exactly kdims bytes.  Tuning knob flat_tile_kernel = 1: the tile kernel always
inline ScanKernel fused_kernel(int eng, uint32_t kdims, uint64_t row_stride, bool knob_tile_kernel, bool planes_supported, bool u8_supported) {
    if (knob_tile_kernel) return ScanKernel::TILE;
    if (bit_planes(eng)) return planes_supported ? ScanKernel::RESIDENT_PLANES : ScanKernel::TILE;
    return eng == U8 && row_stride == (uint64_t)kdims && u8_supported ? ScanKernel::RESIDENT_U8 : ScanKernel::TILE;
}
// e2m1 digits on the scaled MFMA instead of i8 digits (tuning knob flat_fp4).  Octal digits (0..7) have no e2m1 form: i8 always
inline bool scan_fp4(ScanKernel kernel, int eng, bool knob_fp4) { return kernel == ScanKernel::RESIDENT_PLANES && eng != Q3 && knob_fp4; }
// cap on a fused chunk: the tile kernels' grid (and their event granularity) like 4 M; a query-resident kernel is persistent and pays
// ~35 us of prologue per launch, so it takes everything that is left once the growth rule allows it
constexpr uint64_t TILE_CHUNK_CAP = 1ull << 22, RESIDENT_CHUNK_CAP = 1ull << 31;
constexpr uint64_t fused_cap(ScanKernel kernel) { return kernel == ScanKernel::TILE ? TILE_CHUNK_CAP : RESIDENT_CHUNK_CAP; }

// ---- unfused chunks: the [B][chunk] score matrix stays within score_bytes; whole tiles of 128 candidates, at least one, at most n ----
inline uint32_t unfused_chunk(uint32_t widest, uint64_t score_bytes, uint32_t B, uint32_t n) {
    uint64_t chunk = (score_bytes / B / 4) / 128 * 128;
    if (chunk > widest) chunk = widest;
    if (chunk < 128) chunk = 128;
    return chunk < n ? (uint32_t)chunk : n;
}
inline uint32_t brute_unfused_chunk(uint32_t B, uint32_t n) { return unfused_chunk(1u << 18, 1ull << 30, B, n); } // <= 1 GiB of scores
inline uint32_t code_unfused_chunk(uint32_t B, uint32_t n) { return unfused_chunk(1u << 20, 1ull << 31, B, n); }  // <= 2 GiB

// ---- buffers that follow from the widest unfused chunk they serve ----
// segments per query of the selection over a score chunk: enough waves to fill 256 CUs x 8, at least 4096 candidates per segment
inline uint32_t select_segments(uint32_t B, uint32_t n_chunk) {
    uint32_t S = (4096 + B - 1) / B;
    const uint32_t max_s = (n_chunk + 4095) / 4096;
    if (S > max_s) S = max_s;
    if (S > 64) S = 64;
    return S ? S : 1;
}
// floats per query of the score matrix
inline uint64_t score_stride(uint32_t widest) { return ((uint64_t)widest + 63) & ~63ull; }

// ---- the chunk schedule of one attempt ----
// Attempt 0 of a fused scan: the seed chunk goes through the score matrix + segmented selection and seeds every query's threshold; every
// later chunk is `growth` times everything seen before it (capped) and the scoring kernel appends only what beats the threshold.  An
// append-buffer overflow (an adversarially ordered corpus) repeats the call as attempt 1: unfused chunks only, so the result never
// depends on the shortcut.  Tuning knob flat_unfused = 1, or n <= FLAT_SEED: attempt 0 is unfused already.
struct Chunk {
    uint32_t n0, nc; // rows [n0, n0 + nc)
    bool fused;
};
// the chunks cover [0, n) exactly once, in order
struct Schedule {
    uint32_t n, first /*the first chunk; unfused attempt: every chunk*/, growth;
    bool fused;
    uint64_t cap;
    uint32_t n0 = 0;
    bool next(Chunk &c) {
        if (n0 >= n || first == 0) return false;
        c.n0 = n0;
        c.fused = fused && n0 > 0;
        uint64_t nc = c.fused ? (uint64_t)n0 * growth : first;
        if (c.fused && nc > cap) nc = cap;
        if (nc > (uint64_t)(n - n0)) nc = n - n0;
        c.nc = (uint32_t)nc;
        n0 += c.nc;
        return true;
    }
};

// one call's scan
struct Scan {
    uint32_t n, B, P;       // rows, queries, survivor pool per query
    uint32_t seed, unfused; // first chunk of a fused attempt; every chunk of an unfused one
    uint64_t cap;           // on a fused chunk
    bool allow_fused;
    uint32_t growth() const { return flat_growth(P); }
    uint32_t app_cap() const { return flat_app_cap(P); }
    bool fused(int attempt) const { return allow_fused && attempt == 0; }
    uint32_t first(int attempt) const { return fused(attempt) ? seed : unfused; }
    Schedule schedule(int attempt) const { return Schedule{n, first(attempt), growth(), fused(attempt), cap}; }
};
// brute force: the seed is no wider than an unfused chunk (the score matrix is sized by it); always the tile GEMM
inline Scan brute_scan(uint32_t n, uint32_t B, uint32_t k, bool knob_unfused) {
    const uint32_t chunk = brute_unfused_chunk(B, n);
    return Scan{n, B, brute_pool(k), FLAT_SEED < chunk ? FLAT_SEED : chunk, chunk, TILE_CHUNK_CAP, !knob_unfused && n > FLAT_SEED};
}
// code scan: the score matrix is sized per attempt by its first chunk
inline Scan code_scan(uint32_t n, uint32_t B, uint32_t top_k, bool knob_unfused, ScanKernel kernel) {
    return Scan{n, B, code_pool(top_k), FLAT_SEED, code_unfused_chunk(B, n), fused_cap(kernel), !knob_unfused && n > FLAT_SEED};
}

} // namespace flat_plan
