// lat_dots_host.h — plain host models of what the latency kernels' evaluation blocks (cosdata_amd/csrc/walk_common.h: spec_f32_dots,
// spec_f16_dots, spec_row_dots, float_row_dot_wave, int_row_dot_group0) must leave behind, and the inputs they are checked on.
// No HIP: tests/cxx/lat_dots_selftest.cpp (host compiler) pins the models to the oracle bit for bit, tests/cxx/lat_dots_check.hip
// compares the device functions with them.  Compile with -ffp-contract=off: every fused step below is an explicit std::fmaf.
//   * f32: dot_product_f32_simd (x86_64.rs:418-444) — eight fmaf chains from +0.0, chain c over the elements 8s + c, the tree
//     ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)), an unfused sequential tail;
//   * f16: dot_product_f16 (dot_product.rs:13-19) — ONE chain of unfused f32(a) * f32(b), folded from -0.0;
//   * binary / octal: dot_product.rs:21-33 / :64-90 over plane-major rows, and the 16-byte chunk layout of DESIGN.md §3;
//   * the parked word: cosine_or_dot + metric_key — den = |q| * |v|, bad = den == 0, the IEEE quotient, the total-order key
//     (complemented for metrics 1 and 2), bad in bit 32.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ldm {

enum Storage : int { ST_F32 = 0, ST_F16 = 1, ST_BIN = 2, ST_OCT = 3 };
inline const char *storage_name(int st) { return st == ST_F32 ? "f32" : st == ST_F16 ? "f16" : st == ST_BIN ? "binary" : "octal"; }

// the sweep of both programs
inline std::vector<uint32_t> sweep_dims(int st) {
    switch (st) {
    case ST_F32: return {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 100, 255, 256, 257, 1027, 2047, 2048};
    case ST_F16: return {1, 2, 7, 8, 9, 63, 64, 65, 71, 127, 128, 129, 135, 136, 1027, 2047, 2048};
    case ST_BIN: return {1, 127, 128, 129, 2048, 2049, 4097, 6145, 8192}; // 1, 1, 1, 2, 16, 17, 33, 49, 64 chunks
    default: return {1, 31, 32, 33, 512, 513, 1025, 1537, 2048};          // the same chunk counts, 32 dims each
    }
}
constexpr uint32_t TABLE_ROWS = 512;                                 // rows of the synthetic table
constexpr uint32_t ZERO_ROWS[3] = {3, 200, 400};                     // zero contents, norm 0 (never the last row: its bytes must tell)
constexpr uint32_t N_QUERIES = 3, ZERO_QUERY = 2;                    // queries 0 and 1 are ordinary, query 2 is all zero (norm 0)
// f16 rows that carry one kind of special code each, at special_positions(); row R16_NEG is negative in every element
enum : uint32_t { R16_SUBNORMAL = 8, R16_PINF = 9, R16_NINF = 10, R16_NAN = 11, R16_NZERO = 12, R16_MAX = 13, R16_NEG = 14 };

inline uint32_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
inline float float_of(uint32_t b) { float v; std::memcpy(&v, &b, 4); return v; }

// half -> float by bit manipulation: subnormals normalised, inf and NaN carried (a NaN's payload moves up, its quiet bit is set as
// the hardware conversions set it)
inline float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u;
    uint32_t m = h & 1023u;
    if (e == 0) {
        if (m == 0) return float_of(s);
        int k = 0;
        while (!(m & 0x400u)) { m <<= 1; k++; }
        return float_of(s | (uint32_t)(127 - 14 - k) << 23 | (m & 0x3FFu) << 13);
    }
    if (e == 31) return float_of(s | 0x7F800000u | (m ? 0x00400000u : 0u) | m << 13);
    return float_of(s | (e + 112u) << 23 | m << 13);
}

// ---- the three dot rules -------------------------------------------------------------------------------------------------------------
inline float dot_f32(const float *a, const float *b, uint32_t n) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const uint32_t steps = n / 8;
    for (uint32_t i = 0; i < steps; i++)
        for (int c = 0; c < 8; c++) s[c] = std::fmaf(a[8 * i + c], b[8 * i + c], s[c]);
    const float s01 = s[0] + s[1], s23 = s[2] + s[3], s45 = s[4] + s[5], s67 = s[6] + s[7];
    const float lo = s01 + s23, hi = s45 + s67;
    float r = lo + hi;
    for (uint32_t i = steps * 8; i < n; i++) { const float p = a[i] * b[i]; r = r + p; }
    return r;
}
inline float dot_f16(const uint16_t *a, const uint16_t *b, uint32_t n) {
    float acc = -0.0f;
    for (uint32_t i = 0; i < n; i++) { const float p = half_to_float(a[i]) * half_to_float(b[i]); acc = acc + p; }
    return acc;
}
// plane-major rows (plane 0 first, as stored), pb bytes per plane
inline uint32_t dot_binary(const uint8_t *x, const uint8_t *y, uint32_t pb) {
    uint32_t d = 0;
    for (uint32_t i = 0; i < pb; i++) d += (uint32_t)__builtin_popcount(x[i] & y[i]);
    return d;
}
inline uint32_t dot_octal(const uint8_t *x, const uint8_t *y, uint32_t pb) { // digit = p2 << 2 | p1 << 1 | p0 on the planes as stored
    uint32_t d = 0;
    for (uint32_t i = 0; i < pb; i++)
        for (int bit = 0; bit < 8; bit++) {
            const uint32_t xv = ((x[2 * pb + i] >> bit) & 1u) << 2 | ((x[pb + i] >> bit) & 1u) << 1 | ((x[i] >> bit) & 1u);
            const uint32_t yv = ((y[2 * pb + i] >> bit) & 1u) << 2 | ((y[pb + i] >> bit) & 1u) << 1 | ((y[i] >> bit) & 1u);
            d += xv * yv;
        }
    return d;
}

// ---- deliberately wrong orders: what the inputs must tell from the rules above ---------------------------------------------------
enum : int { F32_ONE_CHAIN = 0, F32_UNFUSED_STEPS = 1, F32_FUSED_TAIL = 2, F32_LEFT_FOLD = 3, F32_VARIANTS = 4 };
inline const char *f32_variant_name(int v) { return v == 0 ? "one_chain" : v == 1 ? "unfused_steps" : v == 2 ? "fused_tail" : "left_fold"; }
inline float dot_f32_variant(int v, const float *a, const float *b, uint32_t n) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const uint32_t steps = n / 8;
    float r;
    if (v == F32_ONE_CHAIN) { // the body as one sequential fused chain
        r = 0.f;
        for (uint32_t i = 0; i < steps * 8; i++) r = std::fmaf(a[i], b[i], r);
    } else {
        for (uint32_t i = 0; i < steps; i++)
            for (int c = 0; c < 8; c++) {
                if (v == F32_UNFUSED_STEPS) { const float p = a[8 * i + c] * b[8 * i + c]; s[c] = s[c] + p; }
                else s[c] = std::fmaf(a[8 * i + c], b[8 * i + c], s[c]);
            }
        if (v == F32_LEFT_FOLD) {
            r = s[0];
            for (int c = 1; c < 8; c++) r = r + s[c];
        } else {
            const float s01 = s[0] + s[1], s23 = s[2] + s[3], s45 = s[4] + s[5], s67 = s[6] + s[7];
            const float lo = s01 + s23, hi = s45 + s67;
            r = lo + hi;
        }
    }
    for (uint32_t i = steps * 8; i < n; i++) {
        if (v == F32_FUSED_TAIL) r = std::fmaf(a[i], b[i], r);
        else { const float p = a[i] * b[i]; r = r + p; }
    }
    return r;
}
// the dims at which a variant is another computation: one chain and the left fold from the first full step on (one step: eight
// products, summed in another order); unfused steps from the second step on (fmaf(a, b, +0.0) is the rounded product); a fused tail
// with a tail element that meets a sum (a first tail element added to the +0.0 of an empty body is the rounded product either way)
inline bool f32_variant_applies(int v, uint32_t n) {
    const uint32_t steps = n / 8, tail = n % 8;
    switch (v) {
    case F32_ONE_CHAIN: case F32_LEFT_FOLD: return steps >= 1;
    case F32_UNFUSED_STEPS: return steps >= 2;
    default: return tail >= 2 || (tail >= 1 && steps >= 1);
    }
}
enum : int { F16_PLUS_ZERO = 0, F16_FUSED = 1, F16_EIGHT_CHAINS = 2, F16_VARIANTS = 3 };
inline const char *f16_variant_name(int v) { return v == 0 ? "plus_zero_start" : v == 1 ? "fused_steps" : "eight_chains"; }
inline float dot_f16_variant(int v, const uint16_t *a, const uint16_t *b, uint32_t n) {
    if (v == F16_EIGHT_CHAINS) { // element i on chain i % 8, the f32 rule's tree
        float s[8];
        for (int c = 0; c < 8; c++) s[c] = -0.0f;
        for (uint32_t i = 0; i < n; i++) { const float p = half_to_float(a[i]) * half_to_float(b[i]); s[i % 8] = s[i % 8] + p; }
        const float s01 = s[0] + s[1], s23 = s[2] + s[3], s45 = s[4] + s[5], s67 = s[6] + s[7];
        const float lo = s01 + s23, hi = s45 + s67;
        return lo + hi;
    }
    float acc = v == F16_PLUS_ZERO ? 0.0f : -0.0f;
    for (uint32_t i = 0; i < n; i++) {
        if (v == F16_FUSED) acc = std::fmaf(half_to_float(a[i]), half_to_float(b[i]), acc);
        else { const float p = half_to_float(a[i]) * half_to_float(b[i]); acc = acc + p; }
    }
    return acc;
}
// +0.0 start: another result wherever every product is -0.0 (row R16_NEG against the zero query), at every dim.  Eight chains: from
// four elements on ((p0+p1)+(p2+p3) against ((p0+p1)+p2)+p3; up to three elements both orders are p0+p1+p2 left to right).  Fused
// steps: NEVER another result — the product of two f16 values has at most 22 significant bits and an exponent >= -48, so it is exact
// in f32 and fmaf(a, b, acc) rounds the same real number as acc + a * b; the self-test asserts that equality instead.
inline bool f16_variant_applies(int v, uint32_t n) { return v == F16_PLUS_ZERO ? n >= 1 : v == F16_EIGHT_CHAINS ? n >= 4 : false; }

// ---- the parked word -----------------------------------------------------------------------------------------------------------------
inline uint32_t total_order_key(float v) { const uint32_t b = bits_of(v); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
inline uint64_t parked_word(uint32_t metric, float dot, float qmag, float mag) {
    bool bad = false;
    float sim = dot;
    if (metric == 0u) {
        const float den = qmag * mag;
        bad = den == 0.0f;
        sim = dot / den;
    }
    const uint32_t k = total_order_key(sim);
    return (uint64_t)((metric == 1u || metric == 2u) ? ~k : k) | (bad ? 1ull << 32 : 0ull);
}
inline float key_value(uint32_t metric, uint32_t key) { // the similarity a key stands for
    const uint32_t k = (metric == 1u || metric == 2u) ? ~key : key;
    return float_of((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// Two f32 patterns agree: the same bits, or both NaN with the same sign (a NaN's payload is the platform's; its sign decides at which
// end of f32::total_cmp it sorts — dot_engines.h x86_div)
inline bool same_f32(uint32_t a, uint32_t b) {
    const bool an = (a & 0x7FFFFFFFu) > 0x7F800000u, bn = (b & 0x7FFFFFFFu) > 0x7F800000u;
    if (an || bn) return an && bn && (a >> 31) == (b >> 31);
    return a == b;
}
// ... two parked words: the same flag, and keys that stand for agreeing similarities
inline bool same_word(uint32_t metric, uint64_t a, uint64_t b) {
    return (a >> 32) == (b >> 32) && same_f32(bits_of(key_value(metric, (uint32_t)a)), bits_of(key_value(metric, (uint32_t)b)));
}

// ---- layout ------------------------------------------------------------------------------------------------------------------------------
inline uint32_t plane_bytes(uint32_t dim) { return (dim + 7) / 8; }
inline uint32_t ref_bytes(int st, uint32_t dim) { return st == ST_F32 ? dim * 4 : st == ST_F16 ? dim * 2 : st == ST_BIN ? plane_bytes(dim) : 3 * plane_bytes(dim); }
inline uint32_t n_chunks(int st, uint32_t dim) { return st == ST_BIN ? (dim + 127) / 128 : st == ST_OCT ? (dim + 31) / 32 : 0; }
inline uint32_t row_stride(int st, uint32_t dim) { return st == ST_F32 ? (dim * 4 + 15) & ~15u : st == ST_F16 ? (dim * 2 + 15) & ~15u : n_chunks(st, dim) * 16; }
// reference layout -> device layout: float rows padded with zeros to 16 bytes; binary: the plane itself; octal: chunk k =
// [plane 0 | plane 1 | plane 2 | 0], four bytes (32 dims) each.  dev: row_stride bytes, zero-filled here.
inline void to_device_layout(int st, uint32_t dim, const uint8_t *ref, uint8_t *dev) {
    std::memset(dev, 0, row_stride(st, dim));
    if (st != ST_OCT) { std::memcpy(dev, ref, ref_bytes(st, dim)); return; }
    const uint32_t pb = plane_bytes(dim);
    for (uint32_t p = 0; p < 3; p++)
        for (uint32_t b = 0; b < pb; b++) dev[(size_t)(b / 4) * 16 + p * 4 + (b % 4)] = ref[(size_t)p * pb + b];
}

// ---- inputs: one deterministic function of (storage, dim, row, seed) ---------------------------------------------------------------------
struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() >> 33) % n; }
};
inline Rng rng_for(int st, uint32_t dim, uint32_t row, uint32_t seed) {
    Rng r{((uint64_t)st << 56) ^ ((uint64_t)dim << 40) ^ ((uint64_t)seed << 32) ^ row};
    r.next();
    return r;
}
// where an f16 row of one special kind carries its special code: one element in the first, a middle and the last tile of the
// dimension at both tile widths of spec_f16_dots (64 and 128 dims)
inline std::vector<uint32_t> special_positions(uint32_t dim) {
    std::vector<uint32_t> pos;
    for (uint32_t td : {64u, 128u}) {
        const uint32_t nt = (dim + td - 1) / td;
        for (uint32_t t : {0u, nt / 2, nt - 1}) {
            const uint32_t n = dim - t * td < td ? dim - t * td : td;
            pos.push_back(t * td + (t * 7 + 3) % n);
        }
    }
    return pos;
}
constexpr uint32_t SEED_TABLE = 0, SEED_QUERY = 1;
// One row in the REFERENCE layout.  seed SEED_TABLE: row `row` of the table; SEED_QUERY: query `row`.
//   f32: mixed signs, exponents uniform over 20 binades (2^-10 .. 2^9), random significands — neighbouring products differ by up to
//        2^38, so every rounding of a partial sum is at another bit and a wrong order shows; the tail elements behind a body of eight
//        or more full steps sit in the top two binades: a tail product far below the body's sum is absorbed whether it was rounded first or not,
//        and a fused tail would pass;
//   f16: the same over the binades 2^-10 .. 2^9 of f16; the special rows above;
//   binary / octal: random bits in the dims of the row, zero bits behind them (as the quantizer leaves them).
inline std::vector<uint8_t> gen_row(int st, uint32_t dim, uint32_t row, uint32_t seed) {
    std::vector<uint8_t> out(ref_bytes(st, dim), 0);
    const bool table = seed == SEED_TABLE;
    if (table ? (row == ZERO_ROWS[0] || row == ZERO_ROWS[1] || row == ZERO_ROWS[2]) : row == ZERO_QUERY) return out;
    Rng r = rng_for(st, dim, row, seed);
    if (st == ST_F32) {
        for (uint32_t i = 0; i < dim; i++) {
            const uint64_t z = r.next();
            const uint32_t e = dim >= 64 && i >= dim / 8 * 8 ? 135u + (uint32_t)((z >> 40) & 1u) : 117u + (uint32_t)((z >> 40) % 20u);
            const uint32_t b = (uint32_t)(z >> 63) << 31 | e << 23 | (uint32_t)(z & 0x7FFFFFu);
            std::memcpy(&out[(size_t)i * 4], &b, 4);
        }
    } else if (st == ST_F16) {
        std::vector<uint16_t> h(dim);
        for (uint32_t i = 0; i < dim; i++) {
            const uint64_t z = r.next();
            h[i] = (uint16_t)((uint32_t)(z >> 63) << 15 | (5u + (uint32_t)((z >> 40) % 20u)) << 10 | (uint32_t)(z & 0x3FFu));
            if (table && row == R16_NEG) h[i] |= 0x8000u;
        }
        if (table && row >= R16_SUBNORMAL && row <= R16_MAX) {
            uint32_t k = 0;
            for (uint32_t p : special_positions(dim)) {
                switch (row) {
                case R16_SUBNORMAL: h[p] = (uint16_t)((k & 1u) << 15 | (k == 0 ? 1u : k == 1 ? 0x3FFu : 1u + r.below(0x3FFu))); break;
                case R16_PINF: h[p] = 0x7C00u; break;
                case R16_NINF: h[p] = 0xFC00u; break;
                // quiet NaNs, of ONE sign per row (negative at odd dims): which of two NaN operands an addition hands on is the
                // platform's choice, so only a row whose NaNs agree in sign has a sign to compare
                case R16_NAN: h[p] = (dim & 1u) ? 0xFE01u : 0x7E00u; break;
                case R16_NZERO: h[p] = 0x8000u; break;
                default: h[p] = (uint16_t)((k & 1u) << 15 | 0x7BFFu); break; // +-65504
                }
                k++;
            }
        }
        std::memcpy(out.data(), h.data(), (size_t)dim * 2);
    } else {
        const uint32_t pb = plane_bytes(dim), planes = st == ST_BIN ? 1 : 3;
        for (uint32_t p = 0; p < planes; p++)
            for (uint32_t b = 0; b < pb; b++) {
                uint8_t v = (uint8_t)r.next();
                if (b == pb - 1 && dim % 8) v &= (uint8_t)((1u << (dim % 8)) - 1u);
                out[(size_t)p * pb + b] = v;
            }
    }
    return out;
}
// The norm that stands beside a row (Storage::*::mag): sqrt of the sequential unfused sum of squares from -0.0 (scalar.rs:31-45) over
// the row's elements, an f16 element that is not finite counting as 1 and a zero as 2^-24 (the norm of such a row is the raw vector's,
// whose elements quantized to these codes: positive, and only the zero rows may be flagged).  Code rows carry the RAW vector's norm, which the codes do not determine: any positive number serves,
// here sqrt(1 + dot(row, row)) / 4.  0 for the zero rows and the zero query.
inline float row_mag(int st, uint32_t dim, const uint8_t *ref, bool zero_row) {
    if (zero_row) return 0.0f;
    if (st == ST_BIN) return std::sqrt((float)(1u + dot_binary(ref, ref, plane_bytes(dim)))) * 0.25f;
    if (st == ST_OCT) return std::sqrt((float)(1u + dot_octal(ref, ref, plane_bytes(dim)))) * 0.25f;
    float acc = -0.0f;
    for (uint32_t i = 0; i < dim; i++) {
        float v;
        if (st == ST_F32) std::memcpy(&v, ref + (size_t)i * 4, 4);
        else { uint16_t h; std::memcpy(&h, ref + (size_t)i * 2, 2); v = half_to_float(h); if (!std::isfinite(v)) v = 1.0f; if (v == 0.0f) v = 0x1p-24f; }
        const float p = v * v;
        acc = acc + p;
    }
    return std::sqrt(acc);
}
// the model's dot of two reference-layout rows, as the f32 the kernels hand to cosine_or_dot (integer dots `as f32`)
inline float model_dot(int st, uint32_t dim, const uint8_t *q, const uint8_t *row) {
    if (st == ST_F32) return dot_f32((const float *)q, (const float *)row, dim);
    if (st == ST_F16) return dot_f16((const uint16_t *)q, (const uint16_t *)row, dim);
    return (float)(st == ST_BIN ? dot_binary(q, row, plane_bytes(dim)) : dot_octal(q, row, plane_bytes(dim)));
}

} // namespace ldm
