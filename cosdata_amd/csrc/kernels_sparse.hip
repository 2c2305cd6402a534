// kernels_sparse.hip — learned-sparse (SPLADE-style) inverted index search.
//   SparseAnnQueryBasic::sequential_search          models/sparse_ann_query.rs:68-147
//   InvertedIndexNode::quantize                     models/inverted_index.rs:168-172
//   InvertedIndex::search_internal / finalize_sparse_ann_results (raw-value rerank)   indexes/inverted/mod.rs:278-381
// The reference keeps, per dimension, one list of vector ids per QUANTIZED value (key); a query dimension with quantized value qq
// adds qq * key to every vector of every key list it visits (all keys when qq is above the early-termination threshold, the
// upper keys otherwise).  The caller hands the lists over as CSR — dims[T] ascending, key_off[T][2^bits + 1], vec_ids; the device
// keeps one id-sorted (id, key) list per dimension and accumulates in LDS tiles of the vector-id space (below): HBM-bound streaming
// of the postings, no MFMA (integer adds).  Sums are exact u32 -> atomic adds in any order give the reference's value.  The reference returns the survivors of
// select_nth_unstable in hash-map order; here (as in the oracle) they are ordered by similarity descending, larger id first.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "engine_internal.h"
#include "postings_update.h"
#include "sparse_fold_plan.h"
#include "topk_select.h"

using namespace cosdev;

namespace {

constexpr u32 SEL = 64; // candidates a call keeps per query on the narrow path: top_k * reranking_factor <= 64
// A call that keeps more runs the wide instantiation R = 2, 4, 8 or 16 (cos_sparse_set_max_candidates): pools, partial results and
// the finish kernel hold 64 * R keys.  R = 1 is the narrow path; its kernels are not touched by the wide ones.
constexpr u32 SEL_MAX = 1024;

struct SparseDev {
    const u32 *dims;      // [T]
    const u64 *key_off;   // [T][Q + 1]
    const u32 *vec_ids;   // postings
    const u64 *row_off;   // raw vectors (rerank): [n + 1]
    const u32 *raw_dims;
    const float *raw_vals;
    u32 T, Q, n, bits;
    float upper;
};

// Rust `as u8` / `as u32` on f32 (saturating, NaN -> 0) and f32::clamp; host and device
__host__ __device__ __forceinline__ u32 f32_as_u8(float v) { return !(v == v) || v <= 0.0f ? 0u : (v >= 255.0f ? 255u : (u32)(int)v); }
__host__ __device__ __forceinline__ u32 f32_as_u32(float v) { return !(v == v) || v <= 0.0f ? 0u : (v >= 4294967296.0f ? 0xFFFFFFFFu : (u32)v); }
// InvertedIndexNode::quantize, inverted_index.rs:168-172: one correctly rounded division, one multiplication (this file is built with
// -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt: the device runs the host's two f32 operations)
__host__ __device__ __forceinline__ u32 sparse_quantize(float value, float upper, u32 bits) {
    const u32 quantization = (1u << bits) - 1u;
    const float max_val = (float)quantization;
    float t = (value / upper) * max_val;
    t = t < 0.0f ? 0.0f : (t > max_val ? max_val : t); // clamp keeps NaN
    const u32 q = f32_as_u8(t);
    return q < quantization ? q : quantization;
}

// ---- device layout ----------------------------------------------------------------------------------------------------------
// The caller's CSR keeps, per dimension, one list per key (the reference's map key -> Vec<vec_id>).  On the device every dimension
// is ONE list sorted by vector id, the key of a posting next to it (m_ids u32 + m_keys u8 = 5 B per posting): the vector-id space
// can then be cut into tiles whose accumulators live in LDS, exactly like the BM25 kernel (kernels_hybrid.hip) —
//   * no [B][n] accumulator array in HBM at all (round 2: 268 M scattered global atomics into 410 MB + 512 MB cleared and scanned
//     per 256-query batch = 10.3 ms, 0.013 of the HBM roof on the postings);
//   * a term's early termination (keys below k0 are not visited) is a compare on the key byte.
// Sums are exact u32 adds (qq * key), so the order in which a tile's terms and postings arrive is irrelevant: LDS atomic adds,
// no barrier between terms.  A vector is a result as soon as any visited list holds it, also with similarity 0 (key 0, or a query
// value that quantizes to 0): those rare postings set a bit in a per-tile flag word instead.
constexpr u32 STILE = POSTINGS_TILE; // vector ids per LDS accumulator tile (32 KB of u32)
constexpr u32 SDIR_MIN = 256;    // dimensions with more postings get a tile directory; shorter lists are scanned whole per tile
constexpr u32 SNO_DIR = POSTINGS_NONE;
constexpr int SPU = 8;           // postings per thread per chunk
constexpr u32 SLICES = 256;      // (tile, term) slices a block resolves up front (LDS table); beyond that they are looked up on the way

struct STerm { // one resolved query term (host: find_node, quantize, early-termination rule)
    u64 begin, end; // the dimension's posting list in m_ids / m_keys
    u32 dir;        // row in the tile directory, SNO_DIR for short lists
    u32 qq_k0;      // quantized query value | first visited key << 8
};

struct SCursor { // block-uniform
    u32 tile, t;
    u64 base, e; // postings [base, min(base + SPU * 256, e)) of term t's slice of the tile
    bool valid;
};

// ---- what the tile kernels share ---------------------------------------------------------------------------------------------
// postings [b, e) of query term t that fall into `tile`: the directory's range for a long list, the whole list for a short one
__device__ __forceinline__ void slice_lookup(const STerm *__restrict__ qt, u32 t, const u32 *__restrict__ tile_dir, u32 n_tiles, u32 tile, u64 &b, u64 &e) {
    const u32 dr = qt[t].dir;
    b = qt[t].begin;
    e = qt[t].end;
    if (dr != SNO_DIR) {
        const u32 *row = tile_dir + (u64)dr * (n_tiles + 1);
        e = b + row[tile + 1];
        b = b + row[tile];
    }
}
// wave 0, one lane per term (nt <= 64): the step counts of the slices of sl_n[0 .. nt) -> exclusive prefix st_pre[0 .. nt],
// [nt] = total; the tile's step counter back to 0
template <u32 STEP>
__device__ __forceinline__ void step_prefix(const u32 *sl_n, u32 nt, u32 *st_pre, u32 *st_ctr, int lane) {
    u32 ns = 0;
    if ((u32)lane < nt) ns = (sl_n[lane] + STEP - 1u) / STEP;
    u32 incl = ns;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
        const u32 o = (u32)__shfl_up((int)incl, dd, 64);
        if (lane >= dd) incl += o;
    }
    if ((u32)lane < nt) st_pre[lane] = incl - ns;
    if ((u32)lane == nt - 1u) st_pre[nt] = incl;
    if (lane == 0) *st_ctr = 0u;
}
// Flush of a tile whose similarity-0 hits are flag bits: wave w scans slots [w * 2048, (w + 1) * 2048) of the tile, 64 at a time.
// This takes one slot: its key ((similarity + 1) << 32 | id, 0 = not reached), the accumulator cleared.
__device__ __forceinline__ u64 take_flagged_slot(u32 *acc, const u32 *zflag, u32 d0, u32 slot) {
    const u32 a = acc[slot];
    const u32 fw = zflag[slot >> 5];
    acc[slot] = 0u;
    const bool reached = a != 0u || ((fw >> (slot & 31u)) & 1u);
    return reached ? (((u64)a + 1ull) << 32 | (u64)(d0 + slot)) : 0ull;
}
// a block that has nothing to visit writes an empty segment of 64 * R keys (the finish kernel reads every split)
template <int R>
__device__ __forceinline__ void write_empty_segment(u64 *out) {
    if constexpr (R == 1) {
        if (threadIdx.x < SEL) out[threadIdx.x] = 0ull;
    } else
        for (u32 i = threadIdx.x; i < SEL * R; i += blockDim.x) out[i] = 0ull;
}
// A block's four wave pools (each sorted, blocked layout) -> ONE sorted segment of the block's best 64 * R keys in out[]: the finish
// kernel then folds `splits` segments per query, not 4 * splits, and part[] stays a quarter of the size.
//   R > 1: the LDS networks of topk_select.h over the accumulator tile `acc`, dead after the block's last flush and exactly
//          4 * 1024 u64: the merge costs no LDS, so no occupancy (wpool is not touched and may be null).
//   R = 1: through wpool; wave 0 folds the three other pools into its own key by key, with the fold(key) of its flushes.
template <int R, typename Fold>
__device__ __forceinline__ void block_merge_pools(const Pool<R> &pool, u64 (*wpool)[SEL], u32 *acc, u64 *__restrict__ out, int wave, int lane, Fold fold) {
    if constexpr (R == 1) {
        wpool[wave][lane] = pool.e[0];
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < 4; w++) fold(wpool[w][lane]);
            out[lane] = pool.e[0];
        }
    } else {
        constexpr u32 N = 64u * R;
        u64 *buf = reinterpret_cast<u64 *>(acc);
        static_assert(4u * N * 8u <= STILE * 4u, "the four pools are staged in the accumulator tile");
        __syncthreads(); // every wave is done with the tile
#pragma unroll
        for (int r = 0; r < R; r++) buf[(u32)wave * N + (u32)lane * R + r] = pool.e[r];
        __syncthreads();
        for (u32 p = threadIdx.x; p < 2u * N; p += blockDim.x) { // pools (0, 1) and (2, 3), as fold_reversed
            u64 *a = buf + (p / N) * 2u * N;
            const u32 i = p % N;
            const u64 x = a[i], y = a[2u * N - 1u - i];
            a[i] = x > y ? x : y;
        }
        lds_bitonic_merge_desc<N>(buf, 2, 2 * N);
        fold_reversed<N>(buf, buf + 2 * N);
        lds_bitonic_merge_desc<N>(buf, 1, 0);
        for (u32 i = threadIdx.x; i < N; i += blockDim.x) out[i] = buf[i];
    }
}

// grid = B * splits blocks, heaviest query first: block (q, s) owns the tiles s, s + splits, ...; every wave keeps a private pool
// of the best SEL * R keys ((similarity + 1) << 32 | id) it has flushed, the block's four pools are merged into part[q][s][64 * R].
// R = 1 is the narrow kernel; R = 2, 4, 8, 16 are the wide instantiations of the unpacked layout.
template <int R>
__global__ __launch_bounds__(256) void sparse_tile_kernel(const u32 *__restrict__ m_ids, const uint8_t *__restrict__ m_keys, const STerm *__restrict__ terms,
                                                          const u32 *__restrict__ qt_off, u32 n, const u32 *__restrict__ tile_dir,
                                                          const u32 *__restrict__ order, u32 splits, u64 *__restrict__ part /*[B][splits][64 * R]*/) {
    static_assert(R == 1 || R == 2 || R == 4 || R == 8 || R == 16, "narrow or a wide instantiation");
    __shared__ alignas(R == 1 ? 4 : 16) u32 acc[STILE + 64]; // [STILE + lane] = the lane's dummy slot for postings that do not count (one per lane: same-address LDS atomics serialise)
    __shared__ u32 zflag[STILE / 32];
    __shared__ u64 wpool[4][SEL]; // (R == 1 only: the wide merge is staged in acc)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u32 q = order[blockIdx.x / splits];
    const u32 split = blockIdx.x % splits;
    const u32 t0 = qt_off[q], nt = qt_off[q + 1] - t0;
    const u32 n_tiles = (n + STILE - 1) / STILE;
    u64 *out = part + ((u64)q * splits + split) * (SEL * R);
    if (nt == 0 || split >= n_tiles) { // nothing to visit
        write_empty_segment<R>(out);
        return;
    }
    for (u32 i = threadIdx.x; i < STILE; i += blockDim.x) acc[i] = 0u;
    for (u32 i = threadIdx.x; i < STILE / 32; i += blockDim.x) zflag[i] = 0u;
    const STerm *qt = terms + t0;
    Pool<R> pool;
    pool.clear();
    u64 thr = 0ull;

    // __ballot, as this kernel always voted; pool_fold_lanes' ballot64 is the same vote in fewer instructions, but switching is a change to time
    auto fold_keys = [&](u64 key) { pool_fold_mask<R>(pool, thr, key, __ballot(key > thr), lane); };
    auto slice_global = [&](u32 tile, u32 t, u64 &b, u64 &e) { slice_lookup(qt, t, tile_dir, n_tiles, tile, b, e); };
    // The (tile, term) slices of this block, resolved once, all lookups in flight together: a chunk used to start with two
    // DEPENDENT global loads (the term's directory row, then its two entries) that nothing overlapped — with ~900 postings per slice
    // the kernel spent more time finding its slices than streaming them (0.95 ms per 256-query batch, 0.14 of the HBM roof).
    __shared__ u64 sl_b[SLICES];
    __shared__ u32 sl_n[SLICES], sl_w[SLICES]; // slice = [sl_b, sl_b + sl_n); a list has < 2^32 postings (cos_sparse_create)
    const u32 my_tiles = (n_tiles - split + splits - 1) / splits;
    const bool tabled = (u64)my_tiles * nt <= SLICES;
    if (tabled)
        for (u32 p = threadIdx.x; p < my_tiles * nt; p += blockDim.x) {
            u64 b, e;
            slice_global(split + (p / nt) * splits, p % nt, b, e);
            sl_b[p] = b;
            sl_n[p] = (u32)(e - b);
            if (p < nt) sl_w[p] = qt[p].qq_k0;
        }
    auto slice = [&](u32 tile, u32 t, u64 &b, u64 &e) {
        if constexpr (R == 1) {
            if (tabled) {
                const u32 p = ((tile - split) / splits) * nt + t;
                b = sl_b[p];
                e = b + sl_n[p];
            } else
                slice_global(tile, t, b, e);
        } else { // through locals: written straight into a cursor's fields, the two branches end as one store to a selected
                 // address and the cursors move to scratch memory (the narrow kernel carries 40 B of it)
            u64 bb, ee;
            if (tabled) {
                const u32 p = ((tile - split) / splits) * nt + t;
                bb = sl_b[p];
                ee = bb + sl_n[p];
            } else
                slice_global(tile, t, bb, ee);
            b = bb;
            e = ee;
        }
    };
    auto advance = [&](const SCursor &c) -> SCursor {
        SCursor nx = c;
        if (c.base + (u64)SPU * 256 < c.e) { nx.base = c.base + (u64)SPU * 256; return nx; }
        if (c.t + 1 < nt) nx.t = c.t + 1;
        else { nx.t = 0; nx.tile = c.tile + splits; }
        nx.valid = nx.tile < n_tiles;
        if (nx.valid) slice(nx.tile, nx.t, nx.base, nx.e);
        return nx;
    };
    // every load is issued unconditionally (masked lanes read posting 0 and drop it): a fixed number of loads per chunk lets the
    // compiler wait for exactly the older chunk while the newer one stays in flight (see bm25_score_kernel)
    auto fetch = [&](const SCursor &c, u32 (&iv)[SPU], u32 (&kv)[SPU]) -> u32 {
        u32 mask = 0;
#pragma unroll
        for (int u = 0; u < SPU; u++) {
            const u64 i = c.base + threadIdx.x + (u64)u * 256;
            const bool in = c.valid && i < c.e;
            const u64 ii = in ? i : 0ull;
            iv[u] = m_ids[ii];
            kv[u] = m_keys[ii];
            mask |= (in ? 1u : 0u) << u;
        }
        return mask;
    };
    auto apply = [&](const SCursor &c, const SCursor &nx, const u32 (&iv)[SPU], const u32 (&kv)[SPU], const u32 mask) {
        const u32 d0 = c.tile * STILE;
        const u32 w_t = tabled ? sl_w[c.t] : qt[c.t].qq_k0;
        const u32 qq = w_t & 255u, k0 = w_t >> 8;
#pragma unroll
        for (int u = 0; u < SPU; u++) {
            const u32 slot = iv[u] - d0; // a short list's postings of other tiles wrap to >= STILE
            if (((mask >> u) & 1u) && slot < STILE && kv[u] >= k0) {
                const u32 w = qq * kv[u];
                if (w) atomicAdd(&acc[slot], w);
                else atomicOr(&zflag[slot >> 5], 1u << (slot & 31u));
            }
        }
        const bool tile_done = !nx.valid || nx.tile != c.tile;
        if (tile_done) {
            __syncthreads();
            for (u32 s0 = (u32)wave * (STILE / 4); s0 < (u32)(wave + 1) * (STILE / 4); s0 += 64) fold_keys(take_flagged_slot(acc, zflag, d0, s0 + (u32)lane));
            __syncthreads(); // everybody has read the flag words of its slots
            for (u32 i = threadIdx.x; i < STILE / 32; i += blockDim.x) zflag[i] = 0u;
            __syncthreads();
        }
    };

    __syncthreads(); // the slice table
    // ---- stepped path (the usual case: the table holds every slice of the block and a query has <= 64 terms) --------------------
    // A tile's slices average ~900 postings, so the block-wide chunks below (2048 posting slots per (tile, term)) ran 43 % full and
    // the kernel was instruction-bound (135 lane-instructions per posting, profiles/archive/r03_sparse_tile_kernel_sq_counters_*.txt).  Here every WAVE
    // pulls STEPS — 512 consecutive postings of one slice — from a per-tile counter in LDS: a slice of L postings is ceil(L / 512)
    // steps, waves never wait for each other inside a tile (LDS atomic adds commute), a long slice spreads over the four waves, and
    // the next step's postings are in flight while the current one is applied.
    if (tabled && nt <= 64u) {
        __shared__ u32 st_pre[65]; // exclusive prefix of the tile's per-term step counts; [nt] = total
        __shared__ u32 st_ctr;
        constexpr u32 STEP = 64u * SPU;
        for (u32 ti = 0; ti < my_tiles; ti++) {
            const u32 tile = split + ti * splits, d0 = tile * STILE;
            if (wave == 0) step_prefix<STEP>(sl_n + ti * nt, nt, st_pre, &st_ctr, lane); // this tile's slices
            __syncthreads();
            const u32 total = st_pre[nt];
            // which slice does step k belong to: one lane per term tests its range, a ballot finds it (no dependent LDS chain)
            const u32 my_lo = (u32)lane < nt ? st_pre[lane] : 0xFFFFFFFFu, my_hi = (u32)lane < nt ? st_pre[lane + 1] : 0u;
            auto pull = [&]() -> u32 {
                u32 k = 0;
                if (lane == 0) k = atomicAdd(&st_ctr, 1u);
                return readlane_u32(k, 0);
            };
            struct Step { u64 base; u32 len, w; bool valid; };
            auto locate = [&](u32 k) -> Step {
                Step sp;
                sp.valid = k < total;
                sp.base = 0; sp.len = 0; sp.w = 0;
                if (sp.valid) {
                    const u64 m = __ballot(k >= my_lo && k < my_hi);
                    const u32 t = (u32)(__ffsll((long long)m) - 1);
                    const u32 p = ti * nt + t;
                    const u32 done = (k - readlane_u32(my_lo, (int)t)) * STEP, left = sl_n[p] - done;
                    sp.base = sl_b[p] + done;
                    sp.len = left < STEP ? left : STEP;
                    sp.w = sl_w[t];
                }
                return sp;
            };
            // The posting arrays carry STEP entries of padding (cos_sparse_create), so a step's 8 loads per lane are one base address
            // plus compile-time offsets, never clamped; lanes past the step's end read something and drop it below.
            auto fetch_s = [&](const Step &sp, u32 (&iv)[SPU], u32 (&kv)[SPU]) {
                const u32 *ip = m_ids + sp.base + lane;
                const uint8_t *kp = m_keys + sp.base + lane;
#pragma unroll
                for (int u = 0; u < SPU; u++) {
                    iv[u] = ip[u * 64];
                    kv[u] = kp[u * 64];
                }
            };
            // Branch-free: every lane issues its ds_add — a posting that does not count (past the step's end, another tile of a short
            // list, a key below the term's first visited key) adds 0 to the lane's dummy slot behind the tile.  The block-chunk version spent
            // ~70 instructions per posting slot on exec-mask bookkeeping around two predicated atomics (89 lane-instructions per posting,
            // profiles/archive/r03_sparse_tile_kernel_sq_counters_wave_steps.txt).  Weight-0 postings (key 0, or a query value that
            // quantizes to 0) are rare: one wave-level test per step.
            auto apply_s = [&](const Step &sp, const u32 (&iv)[SPU], const u32 (&kv)[SPU]) {
                const u32 qq = sp.w & 255u, k0 = sp.w >> 8;
                bool zero_any = false;
#pragma unroll
                for (int u = 0; u < SPU; u++) {
                    const u32 slot = iv[u] - d0; // a short list's postings of other tiles wrap to >= STILE
                    const bool ok = (u32)lane + (u32)u * 64u < sp.len && slot < STILE && kv[u] >= k0;
                    const u32 w = __umul24(qq, kv[u]); // both < 256: the full-rate 24-bit multiply
                    atomicAdd(&acc[ok ? slot : STILE + (u32)lane], ok ? w : 0u);
                    zero_any |= ok && w == 0u;
                }
                if (__any(zero_any)) {
#pragma unroll
                    for (int u = 0; u < SPU; u++) {
                        const u32 slot = iv[u] - d0;
                        if ((u32)lane + (u32)u * 64u < sp.len && slot < STILE && kv[u] >= k0 && qq * kv[u] == 0u) atomicOr(&zflag[slot >> 5], 1u << (slot & 31u));
                    }
                }
            };
            u32 ia[SPU], ib[SPU], ka[SPU], kb[SPU];
            Step sa = locate(pull()), sb;
            if (sa.valid) fetch_s(sa, ia, ka);
            while (sa.valid) { // ping-pong between the two register sets
                sb = locate(pull());
                if (sb.valid) fetch_s(sb, ib, kb);
                apply_s(sa, ia, ka);
                if (!sb.valid) break;
                sa = locate(pull());
                if (sa.valid) fetch_s(sa, ia, ka);
                apply_s(sb, ib, kb);
            }
            __syncthreads();
            for (u32 s0 = (u32)wave * (STILE / 4); s0 < (u32)(wave + 1) * (STILE / 4); s0 += 64) fold_keys(take_flagged_slot(acc, zflag, d0, s0 + (u32)lane));
            __syncthreads(); // everybody has read the flag words of its slots
            for (u32 i = threadIdx.x; i < STILE / 32; i += blockDim.x) zflag[i] = 0u;
            // (the next tile's prefix barrier orders these stores before its first atomic)
        }
        block_merge_pools<R>(pool, wpool, acc, out, wave, lane, fold_keys);
        return;
    }
    // ---- block-wide chunks: queries of more than 64 terms, or more (tile, term) slices than the table holds ----------------------
    SCursor cur;
    cur.tile = split; cur.t = 0; cur.valid = true;
    slice(cur.tile, 0, cur.base, cur.e);
    u32 ia[SPU], ib[SPU], ka[SPU], kb[SPU];
    u32 ma = fetch(cur, ia, ka), mb;
    __syncthreads();
    for (;;) { // ping-pong between the two register sets
        const SCursor n1 = advance(cur);
        mb = fetch(n1, ib, kb);
        apply(cur, n1, ia, ka, ma);
        if (!n1.valid) break;
        const SCursor n2 = advance(n1);
        ma = fetch(n2, ia, ka);
        apply(n1, n2, ib, kb, mb);
        if (!n2.valid) break;
        cur = n2;
    }
    block_merge_pools<R>(pool, wpool, acc, out, wave, lane, fold_keys);
}

// ---- packed layout (cos_sparse::packed: the default wherever vector ids fit 24 bits; tuning knob sparse_layout = 0 keeps the other) ----
// One u32 per posting, key << 24 | (vector id + 1), instead of a u32 id + a u8 key: 4 B instead of 5 B of HBM traffic per posting,
// one load instead of two, and the apply step of a posting shrinks from ~19 to ~9 instructions:
//   * a step's postings are fetched through a buffer descriptor whose num_records is the step's own length — a lane past the step's
//     end reads 0 = "vector id -1", which is outside every tile — so there is no `lane + 64 u < len` mask;
//   * slot = min((p - (d0 + 1)) & 0xFFFFFF, STILE + lane): postings of other tiles (a short list is scanned whole per tile) and the
//     out-of-range zeros wrap to a huge value and land on a dummy slot behind the tile; no compare, no select;
//   * COUNTED blocks (the usual case): a posting adds qq * key + 2^22, so a slot's high 10 bits count the postings that reached the
//     vector and the low 22 bits hold the similarity — "visited with similarity 0" needs no flag word and no second pass.  The
//     host checks per query that neither field can overflow (sum over its terms of multiplicity x qq x (Q - 1) < 2^22, at most
//     1023 touches; `multiplicity` = how often one vector id occurs in the dimension's list, 1 unless the caller's CSR repeats ids);
//     other queries run the same steps with the flag words of the unpacked kernel.
// Vector ids need 24 bits: n_vectors <= SPK_MAX_N, larger collections keep the unpacked layout.  Queries of more than 64 terms are
// walked in groups of 64 terms (the step directory is one lane per term); slices the LDS table does not hold are looked up on the way.
constexpr u32 SPK_CNT = 1u << 22;
constexpr u32 SPK_SUM = SPK_CNT - 1u;
constexpr u32 SPK_MAX_N = (1u << 24) - 2u * STILE;
constexpr u32 SPK_COUNTED = 0x80000000u; // bit of order[]: this query's blocks may count touches in the accumulator

template <bool COUNTED, int PU /* postings per lane per step */, int R = 1 /* pool of 64 * R keys per wave */>
__device__ __forceinline__ void sparse_packed_body(const u32 *__restrict__ m_pk, const STerm *__restrict__ qt, const u32 nt, const u32 n_tiles,
                                                   const u32 *__restrict__ tile_dir, const u32 split, const u32 splits, u64 *__restrict__ out, u32 *acc,
                                                   u32 *zflag, u64 (*wpool)[SEL], u64 *sl_b, u32 *sl_n, u32 *sl_w, u32 *st_pre, u32 *st_ctr) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr u32 STEP = 64u * PU;
    for (u32 i = threadIdx.x; i < STILE / 4; i += blockDim.x) reinterpret_cast<uint4 *>(acc)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (!COUNTED)
        for (u32 i = threadIdx.x; i < STILE / 32; i += blockDim.x) zflag[i] = 0u;
    Pool<R> pool;
    pool.clear();
    u64 thr = 0ull;
    auto insert_keys = [&](u64 key) { pool_fold_lanes<R>(pool, thr, key, lane); };
    // The (tile, term) slices are resolved into the LDS table a WINDOW at a time, all lookups of a window in flight together: TB tiles
    // x all nt terms when nt <= SLICES (one window for the whole block in the usual case), one tile x SLICES terms otherwise.
    const u32 my_tiles = (n_tiles - split + splits - 1) / splits;
    const u32 TW = nt < SLICES ? nt : SLICES;
    const u32 TB = nt < SLICES ? (SLICES / nt < my_tiles ? SLICES / nt : my_tiles) : 1u;
    const u32 dummy4 = (STILE + (u32)lane) * 4u; // byte address of the lane's dummy slot
    char *accb = reinterpret_cast<char *>(acc);
    for (u32 ti0 = 0; ti0 < my_tiles; ti0 += TB) {
        const u32 tbn = my_tiles - ti0 < TB ? my_tiles - ti0 : TB;
        for (u32 tw0 = 0; tw0 < nt; tw0 += TW) {
            const u32 twn = nt - tw0 < TW ? nt - tw0 : TW;
            __syncthreads(); // the previous window is done with the table
            for (u32 p = threadIdx.x; p < tbn * twn; p += blockDim.x) {
                const u32 tile = split + (ti0 + p / twn) * splits, t = tw0 + p % twn;
                u64 b, e;
                slice_lookup(qt, t, tile_dir, n_tiles, tile, b, e);
                sl_b[p] = b;
                sl_n[p] = (u32)(e - b);
                if (p < twn) sl_w[p] = qt[t].qq_k0;
            }
            const u32 groups = (twn + 63u) >> 6;
            for (u32 tj = 0; tj < tbn; tj++) {
                const u32 tile = split + (ti0 + tj) * splits, d0 = tile * STILE;
                const u32 d1 = d0 + 1u; // a posting holds vector id + 1 in its low 24 bits
                for (u32 g = 0; g < groups; g++) {
                    const u32 tb = g << 6, ng = twn - tb < 64u ? twn - tb : 64u;
                    const u32 row0 = tj * twn + tb; // table row of the group's first term
                    __syncthreads(); // the table; the previous group's directory is no longer read; the previous tile's flush
                    if (wave == 0) step_prefix<STEP>(sl_n + row0, ng, st_pre, st_ctr, lane); // this group's slices of the tile
                    __syncthreads();
                    const u32 total = uniform_u32(st_pre[ng]);
                    const u32 my_lo = (u32)lane < ng ? st_pre[lane] : 0xFFFFFFFFu, my_hi = (u32)lane < ng ? st_pre[lane + 1] : 0u;
                    auto pull = [&]() -> u32 {
                        u32 k = 0;
                        if (lane == 0) k = atomicAdd(st_ctr, 1u);
                        return readlane_u32(k, 0);
                    };
                    struct Step { u32 base_lo, base_hi, len, w; bool valid; };
                    auto locate = [&](u32 k) -> Step {
                        Step sp;
                        sp.valid = k < total;
                        sp.base_lo = 0; sp.base_hi = 0; sp.len = 0; sp.w = 0;
                        if (sp.valid) {
                            const u64 m = ballot64(k >= my_lo && k < my_hi);
                            const u32 tl = (u32)(__ffsll((long long)m) - 1);
                            const u32 done = (k - readlane_u32(my_lo, (int)tl)) * STEP, left = sl_n[row0 + tl] - done;
                            const u64 b = sl_b[row0 + tl] + done;
                            // wave-uniform by construction; say so (values that arrive through a vector load count as divergent)
                            sp.base_lo = uniform_u32((u32)b);
                            sp.base_hi = uniform_u32((u32)(b >> 32));
                            sp.len = uniform_u32(left < STEP ? left : STEP);
                            sp.w = uniform_u32(sl_w[tb + tl]);
                        }
                        return sp;
                    };
                    auto fetch_p = [&](const Step &sp, u32 (&pv)[PU]) {
                        const u32 *bp = m_pk + ((u64)sp.base_hi << 32 | sp.base_lo);
                        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)bp, (short)0, (int)(sp.len * 4u), 0x00020000);
#pragma unroll
                        for (int u = 0; u < PU; u++) pv[u] = (u32)__builtin_amdgcn_raw_buffer_load_b32(rsrc, ((u32)lane + (u32)u * 64u) * 4u, 0, 0);
                    };
                    // a posting: slot = its id relative to the tile (other tiles' postings and the zeros past the step's end wrap to >=
                    // STILE and fall on the lane's dummy slot behind the tile through the min), weight = qq * key
                    auto apply_p = [&](const Step &sp, const u32 (&pv)[PU]) {
                        const u32 qq = sp.w & 255u, k0 = sp.w >> 8;
                        if (COUNTED) {
                            auto one = [&](u32 p, bool keyed) {
                                const u32 rel = p - d1;
                                // (rel & 0xFFFFFF) * 4, the slot's byte address, and qq * (rel >> 24) as ONE full-rate instruction each
                                // (left alone the compiler shifts and masks for the first and picks the quarter-rate v_mul_lo_u32 for the second)
                                u32 at, w;
                                asm("v_mul_u32_u24 %0, %1, 4" : "=v"(at) : "v"(rel));
                                asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(w) : "v"(rel), "s"(qq));
                                if (keyed) at = (rel >> 24) >= k0 ? at : dummy4;
                                at = min(at, dummy4);
                                atomicAdd(reinterpret_cast<u32 *>(accb + at), w | SPK_CNT);
                            };
                            if (sp.len == STEP) { // a full step: no tests at all
                                if (k0 == 0u) {
#pragma unroll
                                    for (int u = 0; u < PU; u++) one(pv[u], false);
                                } else {
#pragma unroll
                                    for (int u = 0; u < PU; u++) one(pv[u], true);
                                }
                            } else {
#pragma unroll
                                for (int u = 0; u < PU; u++)
                                    if ((u32)u * 64u < sp.len) one(pv[u], true);
                                // every path consumes the whole register set: a load still in flight into a register the next
                                // iteration reuses would make the loop head wait for ALL loads, the prefetched step's included
                                asm volatile("" ::"v"(pv[PU - 1]));
                            }
                        } else {
                            bool zero_any = false;
#pragma unroll
                            for (int u = 0; u < PU; u++) {
                                const u32 rel = pv[u] - d1, key = rel >> 24, slot = rel & 0xFFFFFFu;
                                const bool ok = slot < STILE && key >= k0;
                                const u32 w = __umul24(qq, key);
                                atomicAdd(reinterpret_cast<u32 *>(accb + (ok ? slot * 4u : dummy4)), ok ? w : 0u);
                                zero_any |= ok && w == 0u;
                            }
                            if (__any(zero_any)) {
#pragma unroll
                                for (int u = 0; u < PU; u++) {
                                    const u32 rel = pv[u] - d1, key = rel >> 24, slot = rel & 0xFFFFFFu;
                                    if (slot < STILE && key >= k0 && qq * key == 0u) atomicOr(&zflag[slot >> 5], 1u << (slot & 31u));
                                }
                            }
                        }
                    };
                    // Two steps per iteration, no exit in the middle: a step behind the last one has length 0 — eight out-of-range loads,
                    // no memory traffic, nothing applied.  Every fetch is issued and every register set consumed on every path, so the
                    // wait for the older step's postings always leaves exactly the newer step's eight loads in flight (a load that
                    // some path leaves pending makes the loop head wait for ALL loads, the prefetched step's included).
                    u32 pa[PU], pb[PU];
                    Step sa = locate(pull()), sb;
                    fetch_p(sa, pa);
                    while (sa.valid) { // ping-pong between the two register sets
                        sb = locate(pull());
                        fetch_p(sb, pb);
                        apply_p(sa, pa);
                        sa = locate(pull());
                        fetch_p(sa, pa);
                        apply_p(sb, pb);
                    }
                }
                if (tw0 + TW < nt) continue; // more term windows of this tile to come (TB == 1 then)
                __syncthreads();             // every wave's adds to the tile are done
                // flush: wave w scans slots [w * 2048, (w + 1) * 2048) of the tile into its pool and clears them
                if (COUNTED) {
                    for (u32 s0 = (u32)wave * (STILE / 4); s0 < (u32)(wave + 1) * (STILE / 4); s0 += 256) {
                        const u32 slot = s0 + (u32)lane * 4u;
                        const uint4 a4 = *reinterpret_cast<const uint4 *>(&acc[slot]);
                        *reinterpret_cast<uint4 *>(&acc[slot]) = make_uint4(0u, 0u, 0u, 0u);
                        const u32 thr_hi = (u32)(thr >> 32);
                        const u32 a[4] = {a4.x, a4.y, a4.z, a4.w};
                        bool c[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) c[j] = a[j] != 0u && (a[j] & SPK_SUM) + 1u >= thr_hi;
                        if (__any(c[0] | c[1] | c[2] | c[3])) {
#pragma unroll
                            for (int j = 0; j < 4; j++) insert_keys(c[j] ? ((u64)((a[j] & SPK_SUM) + 1u) << 32 | (u64)(d0 + slot + (u32)j)) : 0ull);
                        }
                    }
                } else {
                    for (u32 s0 = (u32)wave * (STILE / 4); s0 < (u32)(wave + 1) * (STILE / 4); s0 += 64) insert_keys(take_flagged_slot(acc, zflag, d0, s0 + (u32)lane));
                    zflag[(u32)wave * (STILE / 128) + (u32)lane] = 0u; // the flag words of this wave's own slots (nobody else reads them)
                }
                // (the next group's barrier orders the cleared slots before the next tile's first add)
            }
        }
    }
    block_merge_pools<R>(pool, wpool, acc, out, wave, lane, insert_keys);
}

// grid / blocks / pools as sparse_tile_kernel; order[i] = query | SPK_COUNTED
template <int PU>
__global__ __launch_bounds__(256) void sparse_packed_kernel(const u32 *__restrict__ m_pk, const STerm *__restrict__ terms, const u32 *__restrict__ qt_off, u32 n,
                                                            const u32 *__restrict__ tile_dir, const u32 *__restrict__ order, u32 splits,
                                                            u64 *__restrict__ part /*[B][splits][64]*/) {
    __shared__ __attribute__((aligned(16))) u32 acc[STILE + 64];
    __shared__ u32 zflag[STILE / 32];
    __shared__ u64 wpool[4][SEL];
    __shared__ u64 sl_b[SLICES];
    __shared__ u32 sl_n[SLICES], sl_w[SLICES];
    __shared__ u32 st_pre[65];
    __shared__ u32 st_ctr;
    const u32 oq = order[blockIdx.x / splits];
    const u32 q = oq & ~SPK_COUNTED;
    const u32 split = blockIdx.x % splits;
    const u32 t0 = qt_off[q], nt = qt_off[q + 1] - t0;
    const u32 n_tiles = (n + STILE - 1) / STILE;
    u64 *out = part + ((u64)q * splits + split) * SEL;
    if (nt == 0 || split >= n_tiles) { // nothing to visit
        write_empty_segment<1>(out);
        return;
    }
    if (oq & SPK_COUNTED) sparse_packed_body<true, PU>(m_pk, terms + t0, nt, n_tiles, tile_dir, split, splits, out, acc, zflag, wpool, sl_b, sl_n, sl_w, st_pre, &st_ctr);
    else sparse_packed_body<false, PU>(m_pk, terms + t0, nt, n_tiles, tile_dir, split, splits, out, acc, zflag, wpool, sl_b, sl_n, sl_w, st_pre, &st_ctr);
}

// the same scan with pools of 64 * R keys per wave (R = 2, 4, 8, 16), eight postings per lane and step
template <int R>
__global__ __launch_bounds__(256) void sparse_wide_packed_kernel(const u32 *__restrict__ m_pk, const STerm *__restrict__ terms, const u32 *__restrict__ qt_off, u32 n,
                                                                 const u32 *__restrict__ tile_dir, const u32 *__restrict__ order, u32 splits,
                                                                 u64 *__restrict__ part /*[B][splits][64 * R]*/) {
    static_assert(R == 2 || R == 4 || R == 8 || R == 16, "wide instantiations");
    __shared__ __attribute__((aligned(16))) u32 acc[STILE + 64];
    __shared__ u32 zflag[STILE / 32];
    __shared__ u64 sl_b[SLICES];
    __shared__ u32 sl_n[SLICES], sl_w[SLICES];
    __shared__ u32 st_pre[65];
    __shared__ u32 st_ctr;
    const u32 oq = order[blockIdx.x / splits];
    const u32 q = oq & ~SPK_COUNTED;
    const u32 split = blockIdx.x % splits;
    const u32 t0 = qt_off[q], nt = qt_off[q + 1] - t0;
    const u32 n_tiles = (n + STILE - 1) / STILE;
    u64 *out = part + ((u64)q * splits + split) * (SEL * R);
    if (nt == 0 || split >= n_tiles) { // nothing to visit
        write_empty_segment<R>(out);
        return;
    }
    if (oq & SPK_COUNTED) sparse_packed_body<true, 8, R>(m_pk, terms + t0, nt, n_tiles, tile_dir, split, splits, out, acc, zflag, nullptr, sl_b, sl_n, sl_w, st_pre, &st_ctr);
    else sparse_packed_body<false, 8, R>(m_pk, terms + t0, nt, n_tiles, tile_dir, split, splits, out, acc, zflag, nullptr, sl_b, sl_n, sl_w, st_pre, &st_ctr);
}

// finalize_sparse_ann_results' key of candidate v: dp over the QUERY pairs in order, f32 multiply then add (the caller sorts by
// total_cmp descending)
__device__ __forceinline__ u64 raw_rerank_key(const SparseDev &ix, u32 v, const u32 *__restrict__ q_dims, const float *__restrict__ q_vals,
                                              const u32 *__restrict__ q_off, u32 q) {
    const u64 b = ix.row_off[v], e = ix.row_off[v + 1];
    float dp = 0.0f;
    for (u32 i = q_off[q]; i < q_off[q + 1]; i++) {
        const u32 d = q_dims[i];
        u64 lo = b, hi = e;
        while (lo < hi) { const u64 mid = lo + (hi - lo) / 2; if (ix.raw_dims[mid] < d) lo = mid + 1; else hi = mid; }
        if (lo < e && ix.raw_dims[lo] == d) dp = __fadd_rn(dp, __fmul_rn(ix.raw_vals[lo], q_vals[i]));
    }
    return pack_key(simkey(dp), v);
}

// What sparse_finish_kernel and sparse_record_kernel share: the best 64 keys of a query's S segment pools, lane l the l-th, and how many
// of them are candidates (select_nth + truncate(k * reranking_factor))
__device__ __forceinline__ u64 narrow_merge_cut(const u64 *__restrict__ part, u32 S, u32 q, u32 k_with_reranking, int lane, u32 &ncand) {
    Pool<1> pool;
    pool.clear();
    u64 thr = 0ull;
    for (u32 sgm = 0; sgm < S; sgm++) pool_fold_lanes<1>(pool, thr, part[((u64)q * S + sgm) * SEL + lane], lane);
    const u32 have = (u32)__popcll(__ballot(pool.e[0] != 0ull));
    ncand = have < k_with_reranking ? have : k_with_reranking;
    return pool.e[0];
}

// one wave per query: merge the segment pools, optional raw-value rerank, write the top k
__global__ __launch_bounds__(64) void sparse_finish_kernel(const SparseDev ix, const u64 *__restrict__ part, u32 S, const u32 *__restrict__ q_dims,
                                                           const float *__restrict__ q_vals, const u32 *__restrict__ q_off, u32 top_k, u32 k_with_reranking,
                                                           int rerank, u32 *__restrict__ out_ids, float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    u32 ncand;
    const u64 mine = narrow_merge_cut(part, S, q, k_with_reranking, lane, ncand);
    if (!rerank) {
        const u32 nout = ncand < top_k ? ncand : top_k;
        if ((u32)lane < nout) {
            out_ids[(u64)q * top_k + lane] = (u32)mine;
            out_scores[(u64)q * top_k + lane] = (float)((u32)(mine >> 32) - 1u); // `similarity as f32`
        }
        if (lane == 0) out_counts[q] = nout;
        return;
    }
    u64 res[1] = {0ull};
    if ((u32)lane < ncand) {
        res[0] = raw_rerank_key(ix, (u32)mine, q_dims, q_vals, q_off, q);
    }
    bitonic_sort_desc<1>(res, lane);
    const u32 nout = ncand < top_k ? ncand : top_k;
    if ((u32)lane < nout) {
        out_ids[(u64)q * top_k + lane] = (u32)res[0];
        out_scores[(u64)q * top_k + lane] = simkey_inv((u32)(res[0] >> 32));
    }
    if (lane == 0) out_counts[q] = nout;
}

// What sparse_wide_finish_kernel<R> and sparse_wide_record_kernel<R> share: best[64 R] <- the best keys of the query's S sorted segments,
// descending; returns the number of candidates among them.  Ends behind a barrier.
template <u32 N>
__device__ __forceinline__ u32 wide_merge_cut(u64 *best, u32 *s_ncand, const u64 *__restrict__ seg, u32 S, u32 k_with_reranking) {
    for (u32 i = threadIdx.x; i < N; i += blockDim.x) best[i] = seg[i];
    __syncthreads();
    for (u32 sgm = 1; sgm < S; sgm++) {
        const u64 *other = seg + (u64)sgm * N;
        if (other[0] <= best[N - 1]) continue; // block-uniform: the segment's best key does not make the cut (an empty segment never does)
        __syncthreads();                       // everybody has read best[N - 1]
        fold_reversed<N>(best, other);
        lds_bitonic_merge_desc<N>(best, 1, 0);
    }
    // select_nth + truncate(k * reranking_factor): the filled entries come first
    if (threadIdx.x == 0) *s_ncand = k_with_reranking < N ? k_with_reranking : N;
    __syncthreads();
    for (u32 i = threadIdx.x; i < k_with_reranking && i < N; i += blockDim.x)
        if (best[i] == 0ull && (i == 0u || best[i - 1] != 0ull)) *s_ncand = i;
    __syncthreads();
    return *s_ncand;
}

// The wide finish, one block of 256 threads per query: the S sorted segments of 64 * R keys are folded into the best 64 * R one
// after the other (fold_reversed + lds_bitonic_merge_desc of topk_select.h: log2(64 R) rounds in 8 KB of LDS at R = 16), cut to k * reranking_factor,
// re-scored four candidates per thread at R = 16 and sorted again in LDS.  Same arithmetic and order as sparse_finish_kernel.
template <int R>
__global__ __launch_bounds__(256) void sparse_wide_finish_kernel(const SparseDev ix, const u64 *__restrict__ part, u32 S, const u32 *__restrict__ q_dims,
                                                                 const float *__restrict__ q_vals, const u32 *__restrict__ q_off, u32 top_k, u32 k_with_reranking,
                                                                 int rerank, u32 *__restrict__ out_ids, float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    static_assert(R == 2 || R == 4 || R == 8 || R == 16, "wide instantiations");
    constexpr u32 N = 64u * R;
    __shared__ u64 best[N];
    __shared__ u32 s_ncand;
    const u32 q = blockIdx.x;
    const u32 ncand = wide_merge_cut<N>(best, &s_ncand, part + (u64)q * S * N, S, k_with_reranking), nout = ncand < top_k ? ncand : top_k;
    if (!rerank) {
        for (u32 i = threadIdx.x; i < nout; i += blockDim.x) {
            const u64 mine = best[i];
            out_ids[(u64)q * top_k + i] = (u32)mine;
            out_scores[(u64)q * top_k + i] = (float)((u32)(mine >> 32) - 1u); // `similarity as f32`
        }
        if (threadIdx.x == 0) out_counts[q] = nout;
        return;
    }
    for (u32 c = threadIdx.x; c < N; c += blockDim.x) { // (every thread rewrites the entries it read)
        u64 res = 0ull;
        if (c < ncand) {
            res = raw_rerank_key(ix, (u32)best[c], q_dims, q_vals, q_off, q);
        }
        best[c] = res;
    }
    lds_bitonic_sort_desc<N>(best);
    for (u32 i = threadIdx.x; i < nout; i += blockDim.x) {
        out_ids[(u64)q * top_k + i] = (u32)best[i];
        out_scores[(u64)q * top_k + i] = simkey_inv((u32)(best[i] >> 32));
    }
    if (threadIdx.x == 0) out_counts[q] = nout;
}

// ---- the handle as one shard of a collection (cos_shardset_sparse_search_batch) -------------------------------------
// A vector's quantized similarity depends on the query and its own postings only, and global id = id_base + local id with increasing
// bases keeps "larger id first": the collection's best C = k * max(reranking_factor, 1) lie inside the union of every shard's best C.
// The record form of the two finish kernels stops behind the cut at C and leaves, per query, a RECORD of fixed stride W = 64 * R slots
// (sparse_fold_plan.h: Layout):
//   rec_keys  [B][W] u64  pack_key(similarity + 1, id_base + local id), descending; 0 in the slots behind the query's count
//   rec_counts[B]    u32  candidates of the query in this shard, min(touched vectors, C)
//   rec_raw   [B][W] u32  simkey(raw-value dot product) of the candidate in the same slot — the score half of raw_rerank_key — when
//                         the call reranks (not written, not part of the record, otherwise)
// No sort by raw score and no cut to top_k here: which candidates are re-ranked at all is the collection's decision
// (sparse_fold_rerank_kernel).
struct SparseRecord {
    u64 *keys;
    u32 *counts, *raw;
    u32 id_base;
};

__global__ __launch_bounds__(64) void sparse_record_kernel(const SparseDev ix, const u64 *__restrict__ part, u32 S, const u32 *__restrict__ q_dims,
                                                           const float *__restrict__ q_vals, const u32 *__restrict__ q_off, u32 k_with_reranking, int rerank,
                                                           const SparseRecord rec) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    u32 ncand;
    const u64 mine = narrow_merge_cut(part, S, q, k_with_reranking, lane, ncand);
    const bool cand = (u32)lane < ncand;
    rec.keys[(u64)q * SEL + lane] = cand ? pack_key((u32)(mine >> 32), rec.id_base + (u32)mine) : 0ull;
    if (rerank) rec.raw[(u64)q * SEL + lane] = cand ? (u32)(raw_rerank_key(ix, (u32)mine, q_dims, q_vals, q_off, q) >> 32) : 0u;
    if (lane == 0) rec.counts[q] = ncand;
}

template <int R>
__global__ __launch_bounds__(256) void sparse_wide_record_kernel(const SparseDev ix, const u64 *__restrict__ part, u32 S, const u32 *__restrict__ q_dims,
                                                                 const float *__restrict__ q_vals, const u32 *__restrict__ q_off, u32 k_with_reranking,
                                                                 int rerank, const SparseRecord rec) {
    static_assert(R == 2 || R == 4 || R == 8 || R == 16, "wide instantiations");
    constexpr u32 N = 64u * R;
    __shared__ u64 best[N];
    __shared__ u32 s_ncand;
    const u32 q = blockIdx.x;
    const u32 ncand = wide_merge_cut<N>(best, &s_ncand, part + (u64)q * S * N, S, k_with_reranking);
    for (u32 c = threadIdx.x; c < N; c += blockDim.x) {
        const u64 mine = best[c];
        const bool cand = c < ncand;
        rec.keys[(u64)q * N + c] = cand ? pack_key((u32)(mine >> 32), rec.id_base + (u32)mine) : 0ull;
        if (rerank) rec.raw[(u64)q * N + c] = cand ? (u32)(raw_rerank_key(ix, (u32)mine, q_dims, q_vals, q_off, q) >> 32) : 0u;
    }
    if (threadIdx.x == 0) rec.counts[q] = ncand;
}

// any W <= min(N, 1024) keys at the front of buf, W a power of two >= 64 known at run time (block-uniform) -> sorted
template <u32 N, u32 W = sparse_fold_plan::MIN_STRIDE>
__device__ __forceinline__ void lds_sort_front_desc(u64 *buf, u32 w) {
    if (w == W) lds_bitonic_sort_desc<W>(buf);
    else if constexpr (2 * W <= N && 2 * W <= sparse_fold_plan::MAX_CANDIDATES) lds_sort_front_desc<N, 2 * W>(buf, w);
}

// The collection's answer from the S gathered records of a query; one workgroup of 256 threads per query, N >= S * W keys in LDS
// (sparse_fold_plan.h decides N).  gathered = [S][shard_words] words, every record laid out as above (counts_off / raw_off in words).
//   1. the S * W quantized keys sorted descending: the first C = k_with_reranking of them are the collection's candidates — the order
//      of the u64 keys (similarity, then the larger global id) is the single handle's;
//   2. without a rerank that is the answer;
//   3. with one, the C-th key is the cut: every thread reads its gathered slots again and a slot whose key makes the cut appends
//      pack_key(its raw score, its global id) to a compact list at the front of the same LDS (keys are unique: at most C pass), which is
//      sorted and cut to top_k.
// The count is min(min(candidates of all shards, C), top_k) from the records' counts, never from a key being non-zero: the raw key of a
// NaN dot product with id 0 is 0 (sparse_finish_kernel counts by ncand too).
template <u32 N>
__global__ __launch_bounds__(256) void sparse_fold_rerank_kernel(const u32 *__restrict__ gathered, u32 S, u64 shard_words, u64 counts_off, u64 raw_off, u32 W,
                                                                 u32 top_k, u32 k_with_reranking, int rerank, u32 *__restrict__ out_ids,
                                                                 float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    static_assert(N >= sparse_fold_plan::MIN_KEYS && N <= sparse_fold_plan::MAX_KEYS && (N & (N - 1)) == 0, "fold widths");
    __shared__ u64 buf[N]; // nothing else: 64 KB at N = 8192
    const u32 q = blockIdx.x, SW = S * W; // SW <= N (the host's plan)
    const u32 wshift = 31u - (u32)__clz((int)W);
    auto slot_key = [&](u32 i) { return reinterpret_cast<const u64 *>(gathered + (u64)(i >> wshift) * shard_words)[(u64)q * W + (i & (W - 1u))]; };
    for (u32 i = threadIdx.x; i < N; i += blockDim.x) buf[i] = i < SW ? slot_key(i) : 0ull;
    u32 total = 0; // block-uniform, at most S * W
    for (u32 s = 0; s < S; s++) total += gathered[(u64)s * shard_words + counts_off + q];
    lds_bitonic_sort_desc<N>(buf);
    const u32 ncand = total < k_with_reranking ? total : k_with_reranking, nout = ncand < top_k ? ncand : top_k;
    if (!rerank) {
        for (u32 i = threadIdx.x; i < nout; i += blockDim.x) {
            const u64 mine = buf[i];
            out_ids[(u64)q * top_k + i] = (u32)mine;
            out_scores[(u64)q * top_k + i] = (float)((u32)(mine >> 32) - 1u); // `similarity as f32`
        }
        if (threadIdx.x == 0) out_counts[q] = nout;
        return;
    }
    // fewer than C candidates in the whole collection: every one of them passes (a filled slot's key is at least 1 << 32)
    const u64 cut = total >= k_with_reranking ? buf[k_with_reranking - 1u] : 1ull;
    // The sorted keys are dead once the cut is read: the compact list takes buf[0 .. W) and, with two shards or more (W < N), the last
    // key's words count its entries.  One shard's record is the collection's cut already: slot i is entry i, and W may equal N.
    u32 *fill = reinterpret_cast<u32 *>(&buf[N - 1]);
    __syncthreads(); // everybody has read the cut
    for (u32 i = threadIdx.x; i < W; i += blockDim.x) buf[i] = 0ull;
    if (threadIdx.x == 0 && S > 1) *fill = 0u;
    __syncthreads();
    for (u32 i = threadIdx.x; i < SW; i += blockDim.x) {
        const u64 key = slot_key(i);
        if (key >= cut) {
            const u32 at = S > 1 ? atomicAdd(fill, 1u) : i;
            const u32 raw = (gathered + (u64)(i >> wshift) * shard_words + raw_off)[(u64)q * W + (i & (W - 1u))];
            if (at < W) buf[at] = pack_key(raw, (u32)key); // (at < C <= W always: the guard keeps a malformed record inside the list)
        }
    }
    lds_sort_front_desc<N>(buf, W);
    for (u32 i = threadIdx.x; i < nout; i += blockDim.x) {
        out_ids[(u64)q * top_k + i] = (u32)buf[i];
        out_scores[(u64)q * top_k + i] = simkey_inv((u32)(buf[i] >> 32));
    }
    if (threadIdx.x == 0) out_counts[q] = nout;
}

} // namespace

struct cos_sparse {
    int32_t device = 0;
    u32 bits = 0, T = 0, n = 0, n_tiles = 0;
    u32 dir_rows = 0;            // rows of d_tile_dir
    u64 raw_nnz = 0, removed = 0; // pairs of the raw CSR; postings removed by cos_sparse_delete since create
    float upper = 1.0f;
    bool have_raw = false;
    // host side of a query's preparation: find_node, the early-termination rule, posting counts
    std::vector<u32> h_dims;    // [T] ascending
    std::vector<u64> h_key_off; // [T][Q + 1] (the caller's CSR offsets: list begin/end and the postings a term visits from key k0 on)
    std::vector<u32> h_dir;     // [T] row in the tile directory or SNO_DIR
    std::vector<u32> h_mult;    // [T] how often one vector id occurs in the dimension's list at most (1 unless the caller's CSR repeats ids)
    bool packed = false;        // device layout: one u32 per posting (d_pk) instead of d_ids + d_keys
    u32 max_cand = SEL;         // widest top_k * max(reranking_factor, 1) a search keeps: 64, 128, 256, 512 or 1024 (cos_sparse_set_max_candidates)
    // device: one id-sorted list per dimension (same offsets as the caller's CSR: list t = [key_off[t][0], key_off[t][Q]))
    DevArr<u32> d_ids;
    DevArr<uint8_t> d_keys;
    DevArr<u32> d_pk; // packed layout: key << 24 | (vector id + 1)
    DevArr<u32> d_tile_dir; // [rows][n_tiles + 1], offsets relative to the list's begin
    DevArr<u32> d_raw_dims;
    DevArr<u64> d_row_off;
    DevArr<float> d_raw_vals;
    // grow-only workspace of cos_sparse_search_batch (no allocation on the query path once warm); `mu` serialises callers
    std::mutex mu;
    DevBuf w_in, w_part, w_oi, w_os, w_oc; // (bytes) w_in: the batch's resolved tables, one image (SparseImage); w_o*: the host entry point's results
    PinArr<unsigned char> h_in;            // pinned staging of w_in: written by the host resolution, read by the launch's one copy
    // ev0 / ev1 bracket the kernels of the most recent batch on the stream they ran on; ev1 is what the next batch (and destroy) waits for
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool stats_pending = false; // last.kernel_ms is still to be read from the events
    cos_sparse_search_stats last{};
    ~cos_sparse() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// scan + finish of a call that keeps more than 64 candidates per query: the instantiation R, pools and segments of 64 * R keys
template <int R>
static hipError_t sparse_launch_wide(const cos_sparse *s, const SparseDev &dev, u32 B, u32 splits, const STerm *terms, const u32 *qt_off, const u32 *order,
                                     u64 *part, const u32 *qd, const float *qv, const u32 *qo, u32 top_k, u32 kwr, int rerank, u32 *oi, float *os, u32 *oc,
                                     hipStream_t st, const SparseRecord *rec) {
    if (s->packed)
        hipLaunchKernelGGL(sparse_wide_packed_kernel<R>, dim3(B * splits), dim3(256), 0, st, s->d_pk.p, terms, qt_off, s->n, s->d_tile_dir.p, order, splits, part);
    else
        hipLaunchKernelGGL(sparse_tile_kernel<R>, dim3(B * splits), dim3(256), 0, st, s->d_ids.p, s->d_keys.p, terms, qt_off, s->n, s->d_tile_dir.p, order, splits, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (rec) hipLaunchKernelGGL(sparse_wide_record_kernel<R>, dim3(B), dim3(256), 0, st, dev, part, splits, qd, qv, qo, kwr, rerank, *rec);
    else hipLaunchKernelGGL(sparse_wide_finish_kernel<R>, dim3(B), dim3(256), 0, st, dev, part, splits, qd, qv, qo, top_k, kwr, rerank, oi, os, oc);
    return hipGetLastError();
}

extern "C" int32_t cos_sparse_destroy(cos_sparse *s) {
    if (!s) return COS_OK;
    (void)hipSetDevice(s->device);
    if (s->ev1) (void)hipEventSynchronize(s->ev1); // a batch of cos_sparse_search_batch_device may still be reading the workspace
    delete s;
    return COS_OK;
}

extern "C" int32_t cos_sparse_create(int32_t device, uint32_t quantization_bits, float values_upper_bound, const uint32_t *dims, uint32_t n_dims,
                                     const uint64_t *key_offsets, const uint32_t *vec_ids, uint32_t n_vectors, const uint64_t *row_offsets,
                                     const uint32_t *raw_dims, const float *raw_vals, cos_sparse **out) {
    if (!dims || !key_offsets || !vec_ids || !out || n_dims == 0 || n_vectors == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (quantization_bits < 1 || quantization_bits > 8) return cos_fail(COS_ERR_INVALID, "quantization_bits must be in [1, 8] (keys are u8)");
    const u32 Q = 1u << quantization_bits;
    for (u32 t = 0; t < n_dims; t++) {
        if (t && dims[t] <= dims[t - 1]) return cos_fail(COS_ERR_INVALID, "dimension indices must be strictly ascending");
        for (u32 k = 0; k < Q; k++)
            if (key_offsets[(size_t)t * (Q + 1) + k] > key_offsets[(size_t)t * (Q + 1) + k + 1]) return cos_fail(COS_ERR_INVALID, "key offsets of dimension %u decrease", dims[t]);
        if (t && key_offsets[(size_t)t * (Q + 1)] != key_offsets[(size_t)(t - 1) * (Q + 1) + Q]) return cos_fail(COS_ERR_INVALID, "posting ranges of consecutive dimensions must be contiguous");
    }
    if (key_offsets[0] != 0) return cos_fail(COS_ERR_INVALID, "the first posting list must start at offset 0");
    const u64 nnz = key_offsets[(size_t)(n_dims - 1) * (Q + 1) + Q];
    for (u64 p = 0; p < nnz; p++)
        if (vec_ids[p] >= n_vectors) return cos_fail(COS_ERR_INVALID, "posting %llu names vector %u of %u", (unsigned long long)p, vec_ids[p], n_vectors);
    if ((row_offsets != nullptr) != (raw_dims != nullptr) || (raw_dims != nullptr) != (raw_vals != nullptr)) return cos_fail(COS_ERR_INVALID, "raw CSR: all three arrays or none");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return cos_fail(COS_ERR_NO_DEVICE, "no HIP device visible; the GPU path has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    cos_sparse *s = new cos_sparse();
    s->device = device; s->bits = quantization_bits; s->T = n_dims; s->n = n_vectors; s->upper = values_upper_bound;
    s->n_tiles = (n_vectors + STILE - 1) / STILE;
    s->h_dims.assign(dims, dims + n_dims);
    s->h_key_off.assign(key_offsets, key_offsets + (size_t)n_dims * (Q + 1));
    // device layout: per dimension the Q key lists merged into one list sorted by vector id ((id, key) pairs; a stable order among
    // equal ids is irrelevant, the sums commute), and a tile directory for the long lists
    constexpr size_t PAD = 64 * SPU; // one step of padding behind the last posting: the kernel's loads are never clamped
    std::vector<u32> m_ids((size_t)nnz + PAD, 0u);
    std::vector<uint8_t> m_keys((size_t)nnz + PAD, 0);
    std::vector<u32> tile_dir;
    s->h_dir.assign(n_dims, SNO_DIR);
    s->h_mult.assign(n_dims, 1u);
    // the one-word-per-posting layout and its kernel (sparse_packed_kernel) wherever vector ids fit 24 bits — measured in round 5:
    // 0.453 ms against 0.540 ms per 256-query batch, 256 / 256 queries identical to the oracle (profiles/r05_candidates_sparse.txt);
    // tuning knob sparse_layout = 0 keeps the (u32 id, u8 key) layout (the parity tests run both)
    s->packed = tune_or(TUNE_SPARSE_LAYOUT, 1) != 0 && n_vectors <= SPK_MAX_N;
    std::vector<u64> tmp;
    u32 rows = 0;
    const u32 nt1 = s->n_tiles + 1;
    for (u32 t = 0; t < n_dims; t++) {
        const uint64_t *ko = key_offsets + (size_t)t * (Q + 1);
        const u64 b = ko[0], e = ko[Q];
        tmp.clear();
        for (u32 k = 0; k < Q; k++)
            for (u64 p = ko[k]; p < ko[k + 1]; p++) tmp.push_back((u64)vec_ids[p] << 8 | k);
        std::sort(tmp.begin(), tmp.end());
        for (u64 p = b; p < e; p++) { m_ids[p] = (u32)(tmp[p - b] >> 8); m_keys[p] = (uint8_t)(tmp[p - b] & 255u); }
        u32 run = 0, mult = 1;
        for (u64 p = b; p < e; p++) {
            run = p > b && m_ids[p] == m_ids[p - 1] ? run + 1 : 1;
            mult = std::max(mult, run);
        }
        s->h_mult[t] = mult;
        if (e - b > SDIR_MIN) {
            if (e - b > 0xFFFFFFFFull) { cos_sparse_destroy(s); return cos_fail(COS_ERR_UNIMPLEMENTED, "dimension %u holds more than 2^32 postings", dims[t]); }
            s->h_dir[t] = rows++;
            s->dir_rows = rows;
            tile_dir.resize((size_t)rows * nt1);
            u32 *row = tile_dir.data() + (size_t)(rows - 1) * nt1;
            u64 p = b;
            for (u32 tile = 0; tile <= s->n_tiles; tile++) {
                const u64 first = (u64)tile * STILE;
                while (p < e && m_ids[p] < first) p++;
                row[tile] = (u32)(p - b);
            }
        }
    }
    auto up = [&](auto &dst, const void *src, size_t count) -> hipError_t {
        hipError_t e = dst.alloc(count);
        return e == hipSuccess && count ? hipMemcpy(dst, src, count * sizeof(*dst.p), hipMemcpyHostToDevice) : e;
    };
    hipError_t e = hipSuccess;
    if (s->packed) {
        std::vector<u32> m_pk((size_t)nnz + 1, 0u);
        for (u64 p = 0; p < nnz; p++) m_pk[p] = (u32)m_keys[p] << 24 | (m_ids[p] + 1u);
        e = up(s->d_pk, m_pk.data(), m_pk.size());
    } else {
        e = up(s->d_ids, m_ids.data(), m_ids.size());
        if (e == hipSuccess) e = up(s->d_keys, m_keys.data(), m_keys.size());
    }
    if (e == hipSuccess) e = up(s->d_tile_dir, tile_dir.data(), tile_dir.size());
    if (e == hipSuccess && row_offsets) {
        const u64 rnnz = row_offsets[n_vectors];
        e = up(s->d_row_off, row_offsets, (size_t)n_vectors + 1);
        if (e == hipSuccess) e = up(s->d_raw_dims, raw_dims, (size_t)rnnz);
        if (e == hipSuccess) e = up(s->d_raw_vals, raw_vals, (size_t)rnnz);
        s->have_raw = true;
        s->raw_nnz = rnnz;
    }
    if (e == hipSuccess) e = hipEventCreate(&s->ev0);
    if (e == hipSuccess) e = hipEventCreate(&s->ev1);
    if (e != hipSuccess) { cos_sparse_destroy(s); HIP_TRY(e); }
    *out = s;
    return COS_OK;
}

// InvertedIndex::insert for a whole collection (indexes/inverted/mod.rs + models/inverted_index.rs:176-200): the vectors are taken in
// id order and every (dimension, value) pair pushes the id to the END of the list of (dimension, quantize(value)) — so the CSR this
// produces is what the host's tree holds after inserting ids 0 .. n-1.  Host code, no device.
extern "C" int32_t cos_sparse_build_csr(uint32_t quantization_bits, float values_upper_bound, uint32_t n_vectors, const uint64_t *row_offsets,
                                        const uint32_t *raw_dims, const float *raw_vals, uint32_t *out_dims, uint64_t *out_key_offsets,
                                        uint32_t *out_vec_ids, uint32_t *n_dims) {
    if (!row_offsets || !raw_dims || !raw_vals || !n_dims || n_vectors == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (quantization_bits < 1 || quantization_bits > 8) return cos_fail(COS_ERR_INVALID, "quantization_bits must be in [1, 8] (keys are u8)");
    const u32 Q = 1u << quantization_bits;
    const u64 nnz = row_offsets[n_vectors];
    for (u32 v = 0; v < n_vectors; v++)
        if (row_offsets[v + 1] < row_offsets[v]) return cos_fail(COS_ERR_INVALID, "row offsets decrease at vector %u", v);
    std::vector<u32> dims(raw_dims, raw_dims + nnz);
    std::sort(dims.begin(), dims.end());
    dims.erase(std::unique(dims.begin(), dims.end()), dims.end());
    const u32 T = (u32)dims.size();
    const bool sizes_only = !out_dims && !out_key_offsets && !out_vec_ids;
    if (sizes_only) { *n_dims = T; return COS_OK; }
    if (!out_dims || !out_key_offsets || !out_vec_ids) return cos_fail(COS_ERR_INVALID, "all three output arrays or none");
    if (*n_dims < T) { *n_dims = T; return cos_fail(COS_ERR_INVALID, "%u distinct dimensions, room for fewer", T); }
    *n_dims = T;
    std::vector<u64> count((size_t)T * Q, 0);
    std::vector<u32> slot(nnz);
    for (u64 p = 0; p < nnz; p++) {
        const u32 t = (u32)(std::lower_bound(dims.begin(), dims.end(), raw_dims[p]) - dims.begin());
        slot[p] = t * Q + sparse_quantize(raw_vals[p], values_upper_bound, quantization_bits);
        count[slot[p]]++;
    }
    std::vector<u64> cursor((size_t)T * Q);
    u64 run = 0;
    for (u32 t = 0; t < T; t++) {
        for (u32 k = 0; k < Q; k++) {
            out_key_offsets[(size_t)t * (Q + 1) + k] = run;
            cursor[(size_t)t * Q + k] = run;
            run += count[(size_t)t * Q + k];
        }
        out_key_offsets[(size_t)t * (Q + 1) + Q] = run;
        out_dims[t] = dims[t];
    }
    for (u32 v = 0; v < n_vectors; v++) // id order = push order
        for (u64 p = row_offsets[v]; p < row_offsets[v + 1]; p++) out_vec_ids[cursor[slot[p]]++] = v;
    return COS_OK;
}

// cos_sparse_build_csr + cos_sparse_create in one call; keep_raw != 0 also uploads the raw vectors for the raw-value rerank
// (their dims must then ascend within a row, finalize_sparse_ann_results' lookup is a binary search)
extern "C" int32_t cos_sparse_create_from_vectors(int32_t device, uint32_t quantization_bits, float values_upper_bound, uint32_t n_vectors,
                                                  const uint64_t *row_offsets, const uint32_t *raw_dims, const float *raw_vals, int32_t keep_raw,
                                                  cos_sparse **out) {
    if (!out) return cos_fail(COS_ERR_INVALID, "null argument");
    *out = nullptr;
    u32 T = 0;
    int32_t rc = cos_sparse_build_csr(quantization_bits, values_upper_bound, n_vectors, row_offsets, raw_dims, raw_vals, nullptr, nullptr, nullptr, &T);
    if (rc) return rc;
    const u32 Q = 1u << quantization_bits;
    std::vector<u32> dims(std::max(T, 1u)), ids((size_t)std::max<u64>(row_offsets[n_vectors], 1));
    std::vector<uint64_t> ko((size_t)std::max(T, 1u) * (Q + 1));
    rc = cos_sparse_build_csr(quantization_bits, values_upper_bound, n_vectors, row_offsets, raw_dims, raw_vals, dims.data(), ko.data(), ids.data(), &T);
    if (rc) return rc;
    if (T == 0) return cos_fail(COS_ERR_INVALID, "no postings");
    return cos_sparse_create(device, quantization_bits, values_upper_bound, dims.data(), T, ko.data(), ids.data(), n_vectors,
                             keep_raw ? row_offsets : nullptr, keep_raw ? raw_dims : nullptr, keep_raw ? raw_vals : nullptr, out);
}

// ---- the search in two parts: host resolution into pinned staging, then copy + kernels on a stream --------------------------------
// what the resolution of one batch leaves for its launch (the tables themselves are in the handle's staging)
struct SparseBatch {
    u32 B = 0, nq = 0, top_k = 0, kwr = 0, R = 1, splits = 1;
    int rerank = 0;
    size_t bytes = 0; // of the staging image
};
// One image, one copy: [STerm x nq (a query pair resolves to at most one term) | q_dims nq | q_vals nq | q_offsets B + 1 | qt_off B + 1 | order B]
struct SparseImage {
    size_t qd, qv, qo, qt_off, order, bytes;
    SparseImage(u32 B, u32 nq) {
        qd = (size_t)nq * sizeof(STerm);
        qv = qd + (size_t)nq * 4;
        qo = qv + (size_t)nq * 4;
        qt_off = qo + ((size_t)B + 1) * 4;
        order = qt_off + ((size_t)B + 1) * 4;
        bytes = order + (size_t)B * 4;
    }
};

// the handle's previous batch has left the staging and the workspace (its end event; a never-recorded event is complete), and its
// kernel time is settled while both events still belong to it
static int32_t sparse_wait_previous(cos_sparse *s) {
    HIP_TRY(hipEventSynchronize(s->ev1));
    if (s->stats_pending) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        s->last.kernel_ms = ms;
        s->stats_pending = false;
    }
    return COS_OK;
}

// limits of a call, in the order cos_sparse_search_batch has always checked them (the caller holds s->mu for max_cand)
static int32_t sparse_admit(const cos_sparse *s, u32 B, u32 top_k, u32 reranking_factor) {
    if (B >= SPK_COUNTED) return cos_fail(COS_ERR_INVALID, "batch of %u queries", B);
    const bool rerank = reranking_factor != 0;
    if (rerank && !s->have_raw) return cos_fail(COS_ERR_NOT_READY, "raw-value rerank needs the raw sparse vectors (cos_sparse_create row_offsets / raw_dims / raw_vals)");
    const u64 kwr64 = (u64)top_k * (rerank ? reranking_factor : 1u);
    if (kwr64 > s->max_cand) return cos_fail(COS_ERR_UNIMPLEMENTED, "top_k x reranking_factor must be <= %u", s->max_cand);
    return COS_OK;
}

// Host resolution (sparse_ann_query.rs:80-125): find_node, quantize, which keys a term visits, the launch order — written into the
// handle's pinned staging.  The caller holds s->mu (cos_sparse_insert / cos_sparse_delete replace the host tables this reads, absolute
// list offsets included, cos_sparse_set_max_candidates the width the call is held to) and the previous batch has been waited for.
static int32_t sparse_resolve(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 top_k,
                              float early_terminate_threshold, u32 reranking_factor, SparseBatch &sb) {
    int32_t rc = sparse_admit(s, B, top_k, reranking_factor);
    if (rc) return rc;
    const bool rerank = reranking_factor != 0;
    const u32 kwr = (u32)((u64)top_k * (rerank ? reranking_factor : 1u));
    // the variant is the call's, not the handle's: up to 64 candidates run the narrow kernels whatever the handle allows
    u32 R = 1;
    while (SEL * R < kwr) R *= 2;
    for (u32 b = 0; b < B; b++)
        if (q_offsets[b + 1] < q_offsets[b]) return cos_fail(COS_ERR_INVALID, "query offsets decrease");
    const u32 nq = q_offsets[B], Q = 1u << s->bits;
    const SparseImage im(B, nq);
    HIP_TRY(s->h_in.grow(im.bytes));
    unsigned char *h = s->h_in;
    STerm *terms = (STerm *)h;
    u32 *qt_off = (u32 *)(h + im.qt_off), *order = (u32 *)(h + im.order);
    if (nq) {
        memcpy(h + im.qd, q_dims, (size_t)nq * 4);
        memcpy(h + im.qv, q_vals, (size_t)nq * 4);
    }
    memcpy(h + im.qo, q_offsets, ((size_t)B + 1) * 4);
    const float qf = (float)Q;
    float etv = qf * early_terminate_threshold;
    etv = etv > 255.0f ? 255.0f : etv;
    const u32 early_terminate_value = f32_as_u8(etv), low_threshold = f32_as_u32(early_terminate_threshold * qf);
    u32 n_terms = 0;
    std::vector<u64> weight(B, 0);
    std::vector<uint8_t> counted(B, 0);
    u64 visited = 0;
    qt_off[0] = 0;
    for (u32 b = 0; b < B; b++) {
        u64 sum_bound = 0, touch_bound = 0; // packed layout: may this query's blocks count touches next to the sum (sparse_packed_body)?
        for (u32 i = q_offsets[b]; i < q_offsets[b + 1]; i++) {
            auto it = std::lower_bound(s->h_dims.begin(), s->h_dims.end(), q_dims[i]);
            if (it == s->h_dims.end() || *it != q_dims[i]) continue;
            const u32 t = (u32)(it - s->h_dims.begin());
            const u32 qq = sparse_quantize(q_vals[i], s->upper, s->bits);
            const u32 k0 = qq > low_threshold ? 0u : early_terminate_value;
            if (k0 >= Q) continue;
            const u64 *ko = s->h_key_off.data() + (size_t)t * (Q + 1);
            if (ko[Q] == ko[0]) continue;
            terms[n_terms++] = STerm{ko[0], ko[Q], s->h_dir[t], qq | k0 << 8};
            weight[b] += ko[Q] - ko[0];
            visited += ko[Q] - ko[k0];
            sum_bound += (u64)s->h_mult[t] * qq * (Q - 1u);
            touch_bound += s->h_mult[t];
        }
        counted[b] = sum_bound < SPK_CNT && touch_bound <= 1023u;
        qt_off[b + 1] = n_terms;
    }
    for (u32 b = 0; b < B; b++) order[b] = b;
    std::stable_sort(order, order + B, [&](u32 a, u32 c) { return weight[a] > weight[c]; }); // heaviest query first
    if (s->packed)
        for (u32 b = 0; b < B; b++)
            if (counted[order[b]]) order[b] |= SPK_COUNTED;
    sb.B = B;
    sb.nq = nq;
    sb.top_k = top_k;
    sb.kwr = kwr;
    sb.R = R;
    sb.rerank = rerank ? 1 : 0;
    // blocks: enough to fill the chip several times over, at most one per tile
    sb.splits = std::max<u32>(1u, std::min<u32>(s->n_tiles, (4096u + B - 1) / B));
    sb.bytes = im.bytes;
    s->last.postings_visited = visited;
    s->last.posting_bytes = visited * 4;
    s->last.blocks = B * sb.splits;
    return COS_OK;
}

// Launch: one copy of the staging image, then scan + finish, all on `st`; results to device pointers.  The two events bracket the
// kernels on the stream they run on.  Nothing here synchronises.  With `rec` the record form of the finish kernel runs behind the same
// scan and the three result pointers are not used.
static int32_t sparse_launch(cos_sparse *s, const SparseBatch &sb, u32 *d_oi, float *d_os, u32 *d_oc, hipStream_t st, const SparseRecord *rec = nullptr) {
    const u32 B = sb.B, R = sb.R, splits = sb.splits, Q = 1u << s->bits;
    const SparseImage im(B, sb.nq);
    HIP_TRY(s->w_in.grow(im.bytes));
    HIP_TRY(s->w_part.grow((size_t)B * splits * SEL * R * 8));
    unsigned char *d = s->w_in.p;
    const STerm *d_terms = (const STerm *)d;
    const u32 *d_qd = (const u32 *)(d + im.qd), *d_qo = (const u32 *)(d + im.qo), *d_qt_off = (const u32 *)(d + im.qt_off), *d_order = (const u32 *)(d + im.order);
    const float *d_qv = (const float *)(d + im.qv);
    u64 *d_part = s->w_part.as<u64>();
    HIP_TRY(hipMemcpyAsync(d, s->h_in.p, im.bytes, hipMemcpyHostToDevice, st));
    SparseDev dev{nullptr, nullptr, nullptr, s->d_row_off, s->d_raw_dims, s->d_raw_vals, s->T, Q, s->n, s->bits, s->upper};
    HIP_TRY(hipEventRecord(s->ev0, st));
    if (R > 1) {
        auto wide = R == 2 ? sparse_launch_wide<2> : R == 4 ? sparse_launch_wide<4> : R == 8 ? sparse_launch_wide<8> : sparse_launch_wide<16>;
        HIP_TRY(wide(s, dev, B, splits, d_terms, d_qt_off, d_order, d_part, d_qd, d_qv, d_qo, sb.top_k, sb.kwr, sb.rerank, d_oi, d_os, d_oc, st, rec));
    } else {
        // eight postings per lane and step; sixteen measured the same (0.447 against 0.453 ms) and was dropped
        if (s->packed)
            hipLaunchKernelGGL(sparse_packed_kernel<8>, dim3(B * splits), dim3(256), 0, st, s->d_pk.p, d_terms, d_qt_off, s->n, s->d_tile_dir.p, d_order, splits, d_part);
        else
            hipLaunchKernelGGL(sparse_tile_kernel<1>, dim3(B * splits), dim3(256), 0, st, s->d_ids.p, s->d_keys.p, d_terms, d_qt_off, s->n, s->d_tile_dir.p, d_order, splits,
                               d_part);
        HIP_TRY(hipGetLastError());
        if (rec) hipLaunchKernelGGL(sparse_record_kernel, dim3(B), dim3(64), 0, st, dev, d_part, splits, d_qd, d_qv, d_qo, sb.kwr, sb.rerank, *rec);
        else hipLaunchKernelGGL(sparse_finish_kernel, dim3(B), dim3(64), 0, st, dev, d_part, splits, d_qd, d_qv, d_qo, sb.top_k, sb.kwr, sb.rerank, d_oi, d_os, d_oc);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->ev1, st));
    s->stats_pending = true;
    return COS_OK;
}

// both parts, for a caller that holds s->mu (cos_sparse_search_batch_device, and the fused hybrid call through cosdev::sparse_search_locked)
static int32_t sparse_search_on_stream(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 top_k,
                                       float early_terminate_threshold, u32 reranking_factor, u32 *d_oi, float *d_os, u32 *d_oc, hipStream_t st) {
    HIP_TRY(hipSetDevice(s->device));
    int32_t rc = sparse_wait_previous(s);
    if (rc) return rc;
    SparseBatch sb;
    rc = sparse_resolve(s, q_dims, q_vals, q_offsets, B, top_k, early_terminate_threshold, reranking_factor, sb);
    if (rc) return rc;
    return sparse_launch(s, sb, d_oi, d_os, d_oc, st);
}

namespace cosdev {
std::mutex &sparse_mutex(cos_sparse *s) { return s->mu; }
int32_t sparse_device(const cos_sparse *s) { return s->device; }
void sparse_limits(const cos_sparse *s, u32 *max_candidates, bool *have_raw, u32 *batch_bound) {
    *max_candidates = s->max_cand;
    *have_raw = s->have_raw;
    *batch_bound = SPK_COUNTED;
}
int32_t sparse_search_locked(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 top_k,
                             float early_terminate_threshold, u32 reranking_factor, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts, hipStream_t st) {
    return sparse_search_on_stream(s, q_dims, q_vals, q_offsets, B, top_k, early_terminate_threshold, reranking_factor, d_out_ids, d_out_scores, d_out_counts, st);
}

void sparse_shape(const cos_sparse *s, u32 *bits, float *upper, u32 *n) {
    *bits = s->bits;
    *upper = s->upper;
    *n = s->n;
}

static_assert(sparse_fold_plan::OK == COS_OK && sparse_fold_plan::INVALID == COS_ERR_INVALID && sparse_fold_plan::UNIMPLEMENTED == COS_ERR_UNIMPLEMENTED,
              "sparse_fold_plan.h restates cos_status");
static_assert(sparse_fold_plan::MIN_STRIDE == SEL && sparse_fold_plan::MAX_CANDIDATES == SEL_MAX, "sparse_fold_plan.h restates the pool widths");

int32_t sparse_record_locked(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 top_k,
                             float early_terminate_threshold, u32 reranking_factor, u32 id_base, u32 *d_record, hipStream_t st) {
    HIP_TRY(hipSetDevice(s->device));
    int32_t rc = sparse_wait_previous(s);
    if (rc) return rc;
    SparseBatch sb;
    rc = sparse_resolve(s, q_dims, q_vals, q_offsets, B, top_k, early_terminate_threshold, reranking_factor, sb); // (sparse_admit's rules first)
    if (rc) return rc;
    const sparse_fold_plan::Layout lay = sparse_fold_plan::layout(B, sb.kwr, sb.rerank != 0);
    if (lay.stride != SEL * sb.R) return cos_fail(COS_ERR_INVALID, "record stride %u against a pool of %u keys", lay.stride, SEL * sb.R);
    const SparseRecord rec{reinterpret_cast<u64 *>(d_record), d_record + lay.counts, d_record + lay.raw, id_base};
    return sparse_launch(s, sb, nullptr, nullptr, nullptr, st, &rec);
}

int32_t sparse_fold_rerank(const u32 *d_gathered, u32 S, u32 B, u32 top_k, u32 reranking_factor, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts,
                           hipStream_t st) {
    const bool rerank = reranking_factor != 0;
    const u64 C = (u64)top_k * (rerank ? reranking_factor : 1u);
    const sparse_fold_plan::Plan fp = sparse_fold_plan::plan(S, C);
    if (fp.status) return cos_fail(fp.status, "%u shards x %llu candidates: the fold holds at most %u keys per query", S, (unsigned long long)C, sparse_fold_plan::MAX_KEYS);
    const sparse_fold_plan::Layout lay = sparse_fold_plan::layout(B, C, rerank);
#define LAUNCH(N)                                                                                                                                          \
    hipLaunchKernelGGL(sparse_fold_rerank_kernel<N>, dim3(B), dim3(sparse_fold_plan::THREADS), 0, st, d_gathered, S, (u64)lay.words, (u64)lay.counts, (u64)lay.raw, \
                       lay.stride, top_k, (u32)C, rerank ? 1 : 0, d_out_ids, d_out_scores, d_out_counts)
    switch (fp.N) {
    case 256: LAUNCH(256); break;
    case 512: LAUNCH(512); break;
    case 1024: LAUNCH(1024); break;
    case 2048: LAUNCH(2048); break;
    case 4096: LAUNCH(4096); break;
    default: LAUNCH(8192); break; // (the plan refuses above)
    }
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    return COS_OK;
}
} // namespace cosdev

extern "C" int32_t cos_sparse_search_batch_device(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, uint32_t B,
                                                  uint32_t top_k, float early_terminate_threshold, uint32_t reranking_factor, uint32_t *d_out_ids,
                                                  float *d_out_scores, uint32_t *d_out_counts, void *stream) {
    if (!s || !q_dims || !q_vals || !q_offsets || !d_out_ids || !d_out_scores || !d_out_counts || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> guard(s->mu);
    return sparse_search_on_stream(s, q_dims, q_vals, q_offsets, B, top_k, early_terminate_threshold, reranking_factor, d_out_ids, d_out_scores, d_out_counts,
                                   (hipStream_t)stream);
}

extern "C" int32_t cos_sparse_search_batch(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, uint32_t B, uint32_t top_k,
                                           float early_terminate_threshold, uint32_t reranking_factor, uint32_t *out_ids, float *out_scores,
                                           uint32_t *out_counts) {
    if (!s || !q_dims || !q_vals || !q_offsets || !out_ids || !out_scores || !out_counts || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> guard(s->mu);
    int32_t rc = sparse_admit(s, B, top_k, reranking_factor); // (before the device is touched, as ever)
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->w_oi.grow((size_t)B * top_k * 4));
    HIP_TRY(s->w_os.grow((size_t)B * top_k * 4));
    HIP_TRY(s->w_oc.grow((size_t)B * 4));
    // the host entry point launches where it always has: the default stream; its copies back wait for the kernels
    rc = sparse_search_on_stream(s, q_dims, q_vals, q_offsets, B, top_k, early_terminate_threshold, reranking_factor, s->w_oi.as<u32>(), s->w_os.as<float>(),
                                 s->w_oc.as<u32>(), 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_ids, s->w_oi.p, (size_t)B * top_k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_scores, s->w_os.p, (size_t)B * top_k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, s->w_oc.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    // The finish kernels write a query's first `count` entries only: what lies behind them in the result buffers is whatever the
    // device memory held.  The caller gets defined values there (no id, score 0), so that two calls on the same state return the
    // same arrays byte for byte, not only the same answers.
    for (u32 q = 0; q < B; q++)
        for (u32 i = std::min(out_counts[q], top_k); i < top_k; i++) {
            out_ids[(size_t)q * top_k + i] = 0xFFFFFFFFu;
            out_scores[(size_t)q * top_k + i] = 0.0f;
        }
    return sparse_wait_previous(s); // (complete already: settles kernel_ms)
}

extern "C" int32_t cos_sparse_layout(cos_sparse *s, uint32_t *packed) {
    if (!s || !packed) return cos_fail(COS_ERR_INVALID, "null argument");
    *packed = s->packed ? 1u : 0u;
    return COS_OK;
}

extern "C" int32_t cos_sparse_set_max_candidates(cos_sparse *s, uint32_t max_candidates) {
    if (!s) return cos_fail(COS_ERR_INVALID, "null argument");
    if (max_candidates == 0 || max_candidates > SEL_MAX) return cos_fail(COS_ERR_INVALID, "max_candidates must be in [1, %u]", SEL_MAX);
    u32 w = SEL;
    while (w < max_candidates) w *= 2;
    std::lock_guard<std::mutex> guard(s->mu);
    s->max_cand = w; // the workspace follows the calls (grow-only): narrowing the setting frees nothing
    return COS_OK;
}

extern "C" int32_t cos_sparse_max_candidates(cos_sparse *s, uint32_t *out) {
    if (!s || !out) return cos_fail(COS_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> guard(s->mu);
    *out = s->max_cand;
    return COS_OK;
}

extern "C" int32_t cos_sparse_last_stats(cos_sparse *s, cos_sparse_search_stats *out) {
    if (!s || !out) return cos_fail(COS_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> guard(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const int32_t rc = sparse_wait_previous(s); // a batch left on a stream by cos_sparse_search_batch_device: its time exists once it has run
    if (rc) return rc;
    *out = s->last;
    return COS_OK;
}

// ------------------------------------------------------------------------------------------------
// Updates of the resident postings: cos_sparse_insert / cos_sparse_delete / cos_sparse_stats / cos_sparse_download.
//   InvertedIndex::insert / InvertedIndexRoot::insert / InvertedIndexNode::insert    indexes/inverted/mod.rs:72-89, models/inverted_index.rs:273-289, :176-201
//   InvertedIndex::mark_embedding_as_deleted / InvertedIndexRoot::delete / Node::delete   mod.rs:91-108, inverted_index.rs:291-306, :205-222
//   VersionedVec::delete (first entry that equals the id) and the iterator that skips tombstones   models/versioned_vec.rs:131-154, :251-275
//
// The postings never go back through the host.  The host owns the dimension table and the per-(dimension, key) counts (h_dims,
// h_key_off: O(T * Q)) and sees the update itself; the device turns the vector-major update into dimension-major order (stable
// radix sort by dimension slot: ids arrive ascending), streams old list + new postings of every dimension into NEW arrays
// (postings_merge_kernel<SparseMerge<PACKED>>, postings_update.h), or the surviving postings of every list (sparse_compact_kernel),
// and searches the tile directory of the new arrays (postings_tile_dir_kernel<SparseIds<PACKED>>).  A delete REMOVES the posting:
// the packed word has no spare bit at 8-bit keys, and a search cannot tell a tombstone from an absent posting (nothing of a list
// but its live entries enters a score).  Only when all of it is complete are the handle's pointers and host tables swapped: a
// call that fails before leaves the handle as it was.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr size_t SPAD_UNPACKED = 64 * SPU, SPAD_PACKED = 1; // padding behind the last posting (cos_sparse_create)

__device__ __forceinline__ u32 spk_word(u32 id, u32 key) { return key << 24 | (id + 1u); }

// vector id of posting p in either layout
template <bool PACKED>
struct SparseIds {
    const u32 *__restrict__ a; // ids or packed words
    __device__ __forceinline__ u32 operator()(u64 p) const { return PACKED ? (a[p] & 0xFFFFFFu) - 1u : a[p]; }
};

// the update's pairs as (vector id << 8 | key): InvertedIndexNode::quantize on the device
__global__ __launch_bounds__(256) void sparse_delta_kernel(const u32 *__restrict__ pair_id, const float *__restrict__ vals, u32 np, float upper, u32 bits,
                                                           u64 *__restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    out[i] = (u64)pair_id[i] << 8 | sparse_quantize(vals[i], upper, bits);
}

// the posting formats of postings_update.h: a vector id and a key byte in two arrays (unpacked) or one word (packed); the delta is
// `id << 8 | key` either way.  The registers hold the key on its own in both layouts; the packed stores leave it out.
template <bool PACKED>
struct SparseMerge {
    const u32 *__restrict__ old_a; // ids or packed words
    const uint8_t *__restrict__ old_keys;
    const u64 *__restrict__ delta;
    u32 *__restrict__ new_a;
    uint8_t *__restrict__ new_keys;
    struct P { u32 a, ky; };
    __device__ __forceinline__ P zero() const { return {0u, 0u}; }
    __device__ __forceinline__ P from_old(u64 p) const { return {old_a[p], PACKED ? 0u : (u32)old_keys[p]}; }
    __device__ __forceinline__ P from_delta(u64 p) const {
        const u64 v = delta[p];
        return {PACKED ? spk_word((u32)(v >> 8), (u32)v & 255u) : (u32)(v >> 8), (u32)v & 255u};
    }
    __device__ __forceinline__ void store4(u64 j, const P (&v)[4]) const {
        *reinterpret_cast<uint4 *>(new_a + j) = make_uint4(v[0].a, v[1].a, v[2].a, v[3].a);
        if (!PACKED) *reinterpret_cast<u32 *>(new_keys + j) = v[0].ky | v[1].ky << 8 | v[2].ky << 16 | v[3].ky << 24;
    }
    __device__ __forceinline__ void store1(u64 j, const P &v) const {
        new_a[j] = v.a;
        if (!PACKED) new_keys[j] = (uint8_t)v.ky;
    }
};

// one thread per (id, dimension, key) pair of a delete call whose key list holds something: lower bound on the id in the
// dimension's list, then the postings of that id in turn — the first one with the pair's key that nobody has claimed yet is
// claimed (the atomic OR on the flag word makes k pairs naming the same (id, dimension, key) claim k different postings)
template <bool PACKED>
__global__ __launch_bounds__(256) void sparse_claim_kernel(const u32 *__restrict__ a, const uint8_t *__restrict__ keys, const u32 *__restrict__ pair_id_key /* id, key */,
                                                           const u64 *__restrict__ pair_begin, const u32 *__restrict__ pair_len, u32 np,
                                                           u32 *__restrict__ flags, uint8_t *__restrict__ found) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const u32 id = pair_id_key[2 * i], key = pair_id_key[2 * i + 1];
    const u64 lo = pair_begin[i], hi = lo + pair_len[i];
    uint8_t hit = 0;
    const SparseIds<PACKED> ids{a};
    for (u64 p = postings_lower_bound(ids, lo, hi, id); p < hi && ids(p) == id; p++) {
        const u32 k = PACKED ? a[p] >> 24 : (u32)keys[p];
        if (k != key) continue;
        const u32 bit = 1u << (p & 31u);
        if (!(atomicOr(&flags[p >> 5], bit) & bit)) { hit = 1; break; }
    }
    found[i] = hit;
}

__global__ __launch_bounds__(256) void sparse_flag_count_kernel(const u32 *__restrict__ flags, u64 n_words, u32 *__restrict__ counts) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) counts[i] = (u32)__popc(flags[i]);
}

// stream compaction: posting p of the old arrays moves to p - (claimed postings before p); `before` = exclusive sum of the flag
// words' popcounts.  A thread reads 4 consecutive postings (one 16-byte load) and, when none of them goes and their destination
// is 16-byte aligned, stores them as one word; otherwise posting by posting (a wave's stores stay contiguous either way).
template <bool PACKED>
__global__ __launch_bounds__(256) void sparse_compact_kernel(const u32 *__restrict__ old_a, const uint8_t *__restrict__ old_keys, const u32 *__restrict__ flags,
                                                             const u32 *__restrict__ before, u64 nnz, u32 *__restrict__ new_a, uint8_t *__restrict__ new_keys) {
    const u64 p0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= nnz) return;
    const u32 w = flags[p0 >> 5], sh = (u32)(p0 & 31u);
    const u32 f = (w >> sh) & 15u;
    u64 o = p0 - ((u64)before[p0 >> 5] + (u64)__popc(w & ((1u << sh) - 1u)));
    if (p0 + 4 <= nnz) {
        const uint4 v = *reinterpret_cast<const uint4 *>(old_a + p0);
        const u32 kw = PACKED ? 0u : *reinterpret_cast<const u32 *>(old_keys + p0);
        if (f == 0u && (o & 3u) == 0u) {
            *reinterpret_cast<uint4 *>(new_a + o) = v;
            if (!PACKED) *reinterpret_cast<u32 *>(new_keys + o) = kw;
            return;
        }
        const u32 a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (!((f >> u) & 1u)) {
                new_a[o] = a[u];
                if (!PACKED) new_keys[o] = (uint8_t)(kw >> (8 * u));
                o++;
            }
        return;
    }
    for (u32 u = 0; p0 + u < nnz; u++)
        if (!((f >> u) & 1u)) {
            new_a[o] = old_a[p0 + u];
            if (!PACKED) new_keys[o] = old_keys[p0 + u];
            o++;
        }
}

// the posting arrays of a handle in the making: allocated with the padding the search kernels rely on, the padding zeroed
struct SparseArrays {
    DevArr<u32> a; // d_ids or d_pk
    DevArr<uint8_t> keys;
    hipError_t alloc(bool packed, u64 nnz) {
        const size_t pad = packed ? SPAD_PACKED : SPAD_UNPACKED;
        hipError_t e = a.alloc((size_t)nnz + pad);
        if (e == hipSuccess) e = hipMemsetAsync(a.p + nnz, 0, pad * 4, 0);
        if (e == hipSuccess && !packed) {
            e = keys.alloc((size_t)nnz + pad);
            if (e == hipSuccess) e = hipMemsetAsync(keys.p + nnz, 0, pad, 0);
        }
        return e;
    }
};

// tile directory of new arrays `d_a` whose lists are the rows of `key_off` ([T][Q + 1]): rows for those longer than SDIR_MIN
int32_t sparse_new_dir(bool packed, const u32 *d_a, const std::vector<u64> &key_off, u32 T, u32 Q, u32 n_tiles, std::vector<u32> &h_dir, u32 &rows_out,
                       DevArr<u32> &d_dir) {
    auto too_long = [](u32) { return cos_fail(COS_ERR_UNIMPLEMENTED, "a dimension would hold more than 2^32 postings"); };
    if (packed) return postings_build_dir(SparseIds<true>{d_a}, key_off.data(), Q + 1, Q, T, SDIR_MIN, n_tiles, 0, too_long, h_dir, rows_out, d_dir);
    return postings_build_dir(SparseIds<false>{d_a}, key_off.data(), Q + 1, Q, T, SDIR_MIN, n_tiles, 0, too_long, h_dir, rows_out, d_dir);
}

} // namespace

extern "C" int32_t cos_sparse_insert(cos_sparse *s, uint32_t m, const uint64_t *row_offsets, const uint32_t *raw_dims, const float *raw_vals,
                                     uint32_t *out_first_id) {
    if (!s) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (m == 0) {
        if (out_first_id) { std::lock_guard<std::mutex> g(s->mu); *out_first_id = s->n; }
        return COS_OK;
    }
    if (!row_offsets) return cos_fail(COS_ERR_INVALID, "bad argument");
    int32_t rc = postings_check_offsets(row_offsets, m, "row_offsets", "vector");
    if (rc) return rc;
    const u64 nd = row_offsets[m];
    if (nd && (!raw_dims || !raw_vals)) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (nd > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 2^31 - 1 pairs in one insert");
    const u32 np = (u32)nd;
    std::lock_guard<std::mutex> g(s->mu);
    const u32 Q = 1u << s->bits, n0 = s->n, T0 = s->T;
    if ((u64)n0 + m > 0xFFFFFFFFull) return cos_fail(COS_ERR_INVALID, "%u + %u vectors do not fit 32-bit ids", n0, m);
    const u32 n1 = n0 + m;
    if (s->packed && n1 > SPK_MAX_N)
        return cos_fail(COS_ERR_UNIMPLEMENTED, "%u vectors pass the packed layout's limit of %u (create the index with sparse_layout = 0)", n1, SPK_MAX_N);
    // ---- host: O(update + T * Q) ------------------------------------------------------------------------------------------------
    // the update's dimensions, the merged dimension table, per pair its slot in it
    std::vector<u32> ud(raw_dims, raw_dims + np);
    std::sort(ud.begin(), ud.end());
    ud.erase(std::unique(ud.begin(), ud.end()), ud.end());
    const u32 U = (u32)ud.size();
    MergedKeys mk = postings_merge_keys(s->h_dims, ud);
    std::vector<u32> &new_dims = mk.keys, &old_of = mk.old_of; // old_of[t] = index in the old table or POSTINGS_NONE
    std::vector<u32> ud_slot(U);
    if (new_dims.size() > 0xFFFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 2^32 - 1 dimensions");
    const u32 T1 = (u32)new_dims.size();
    for (u32 t = 0; t < T1; t++)
        if (mk.del_of[t] != POSTINGS_NONE) ud_slot[mk.del_of[t]] = t;
    std::vector<u32> h_slot(np), h_pid(np), cnt((size_t)T1 * Q, 0u), new_mult(T1, 1u), tmp;
    for (u32 t = 0; t < T1; t++)
        if (old_of[t] != POSTINGS_NONE) new_mult[t] = s->h_mult[old_of[t]];
    for (u32 i = 0; i < m; i++) {
        const u64 b = row_offsets[i], e = row_offsets[i + 1];
        bool ascending = true;
        for (u64 p = b; p < e; p++) {
            const u32 sl = ud_slot[std::lower_bound(ud.begin(), ud.end(), raw_dims[p]) - ud.begin()];
            h_slot[p] = sl;
            h_pid[p] = n0 + i;
            cnt[(size_t)sl * Q + sparse_quantize(raw_vals[p], s->upper, s->bits)]++;
            if (p > b && raw_dims[p] <= raw_dims[p - 1]) ascending = false;
        }
        if (ascending) continue;
        if (s->have_raw) return cos_fail(COS_ERR_INVALID, "the dimensions of vector %u do not ascend (the raw-value rerank searches them)", i);
        tmp.assign(h_slot.begin() + b, h_slot.begin() + e); // a dimension named twice: its id is pushed twice (h_mult feeds the COUNTED bound)
        std::sort(tmp.begin(), tmp.end());
        for (size_t a = 0, z; a < tmp.size(); a = z) {
            for (z = a + 1; z < tmp.size() && tmp[z] == tmp[a]; z++) {}
            new_mult[tmp[a]] = std::max(new_mult[tmp[a]], (u32)(z - a));
        }
    }
    // new per-key offsets; per new dimension where its old part and its delta part start
    std::vector<u64> new_ko((size_t)T1 * (Q + 1)), old_off((size_t)T1 + 1), del_off((size_t)T1 + 1);
    const u64 nnz0 = s->h_key_off[(size_t)(T0 - 1) * (Q + 1) + Q];
    {
        u64 run = 0, dpos = 0;
        u32 next_old = 0; // the old dimension at or behind new slot t
        for (u32 t = 0; t < T1; t++) {
            const u64 *oko = old_of[t] != POSTINGS_NONE ? s->h_key_off.data() + (size_t)old_of[t] * (Q + 1) : nullptr;
            old_off[t] = next_old < T0 ? s->h_key_off[(size_t)next_old * (Q + 1)] : nnz0;
            del_off[t] = dpos;
            const u64 begin = run;
            for (u32 k = 0; k < Q; k++) {
                new_ko[(size_t)t * (Q + 1) + k] = run;
                run += (oko ? oko[k + 1] - oko[k] : 0ull) + cnt[(size_t)t * Q + k];
                dpos += cnt[(size_t)t * Q + k];
            }
            new_ko[(size_t)t * (Q + 1) + Q] = run;
            if (run - begin > 0xFFFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "dimension %u would hold more than 2^32 postings", new_dims[t]);
            if (oko) next_old++;
        }
        old_off[T1] = nnz0;
        del_off[T1] = dpos;
    }
    const u64 nnz1 = nnz0 + np;
    const u32 n_tiles1 = (u32)(((u64)n1 + STILE - 1) / STILE);
    const u64 pieces = (nnz1 + MERGE_PIECE - 1) / MERGE_PIECE;
    if (pieces > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "too many postings for one merge launch");
    std::vector<u64> raw_off_tail;
    if (s->have_raw) {
        raw_off_tail.resize(m);
        for (u32 i = 0; i < m; i++) raw_off_tail[i] = s->raw_nnz + row_offsets[i + 1];
    }
    // ---- device: everything into locals; the handle's arrays are only read ------------------------------------------------------
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(0));
    DevArr<u64> d_delta;
    if (np) { // the delta in dimension-major order (uploads from host arrays are synchronous copies)
        DevArr<u32> d_slot, d_slot_sorted, d_pid;
        DevArr<float> d_vals;
        DevArr<u64> d_pairs;
        DevBuf d_tmp;
        HIP_TRY(d_slot.alloc(np)); HIP_TRY(d_slot_sorted.alloc(np)); HIP_TRY(d_pid.alloc(np)); HIP_TRY(d_vals.alloc(np));
        HIP_TRY(d_pairs.alloc(np)); HIP_TRY(d_delta.alloc(np));
        int end_bit = 1;
        while (end_bit < 32 && (1ull << end_bit) < T1) end_bit++;
        size_t sort_bytes = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_slot.p, d_slot_sorted.p, d_pairs.p, d_delta.p, (int)np, 0, end_bit, 0));
        HIP_TRY(d_tmp.alloc(sort_bytes));
        HIP_TRY(hipMemcpy(d_slot, h_slot.data(), (size_t)np * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_pid, h_pid.data(), (size_t)np * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_vals, raw_vals, (size_t)np * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(sparse_delta_kernel, dim3((np + 255) / 256), dim3(256), 0, 0, d_pid.p, d_vals.p, np, s->upper, s->bits, d_pairs.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, sort_bytes, d_slot.p, d_slot_sorted.p, d_pairs.p, d_delta.p, (int)np, 0, end_bit, 0)); // LSD radix sort: stable
        HIP_TRY(hipStreamSynchronize(0)); // the sort's inputs and workspace are locals of this block
    } else
        HIP_TRY(d_delta.alloc(1));
    SparseArrays na;
    DevArr<u64> d_old_off, d_del_off;
    HIP_TRY(na.alloc(s->packed, nnz1));
    HIP_TRY(d_old_off.alloc((size_t)T1 + 1)); HIP_TRY(d_del_off.alloc((size_t)T1 + 1));
    HIP_TRY(hipMemcpy(d_old_off, old_off.data(), ((size_t)T1 + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_del_off, del_off.data(), ((size_t)T1 + 1) * 8, hipMemcpyHostToDevice));
    if (pieces) {
        if (s->packed)
            hipLaunchKernelGGL(postings_merge_kernel<SparseMerge<true>>, dim3((u32)pieces), dim3(256), 0, 0,
                               SparseMerge<true>{s->d_pk.p, nullptr, d_delta.p, na.a.p, nullptr}, d_old_off.p, d_del_off.p, T1, nnz1);
        else
            hipLaunchKernelGGL(postings_merge_kernel<SparseMerge<false>>, dim3((u32)pieces), dim3(256), 0, 0,
                               SparseMerge<false>{s->d_ids.p, s->d_keys.p, d_delta.p, na.a.p, na.keys.p}, d_old_off.p, d_del_off.p, T1, nnz1);
        HIP_TRY(hipGetLastError());
    }
    std::vector<u32> new_dir;
    DevArr<u32> d_new_dir;
    u32 rows1 = 0;
    rc = sparse_new_dir(s->packed, na.a.p, new_ko, T1, Q, n_tiles1, new_dir, rows1, d_new_dir);
    if (rc) { (void)hipStreamSynchronize(0); return rc; }
    DevArr<u64> d_row_off;
    DevArr<u32> d_raw_dims;
    DevArr<float> d_raw_vals;
    if (s->have_raw) { // the raw CSR grows by the same rows: device-side copy of the old arrays + upload of the new rows
        const u64 r0 = s->raw_nnz;
        HIP_TRY(d_row_off.alloc((size_t)n1 + 1)); HIP_TRY(d_raw_dims.alloc((size_t)(r0 + np))); HIP_TRY(d_raw_vals.alloc((size_t)(r0 + np)));
        HIP_TRY(hipMemcpy(d_row_off, s->d_row_off, ((size_t)n0 + 1) * 8, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(d_row_off.p + n0 + 1, raw_off_tail.data(), (size_t)m * 8, hipMemcpyHostToDevice));
        if (r0) {
            HIP_TRY(hipMemcpy(d_raw_dims, s->d_raw_dims, (size_t)r0 * 4, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(d_raw_vals, s->d_raw_vals, (size_t)r0 * 4, hipMemcpyDeviceToDevice));
        }
        if (np) {
            HIP_TRY(hipMemcpy(d_raw_dims.p + r0, raw_dims, (size_t)np * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_raw_vals.p + r0, raw_vals, (size_t)np * 4, hipMemcpyHostToDevice));
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    // ---- everything is complete: swap, the old arrays are freed by the moves ----------------------------------------------------
    if (s->packed) s->d_pk = std::move(na.a);
    else { s->d_ids = std::move(na.a); s->d_keys = std::move(na.keys); }
    s->d_tile_dir = std::move(d_new_dir);
    if (s->have_raw) {
        s->d_row_off = std::move(d_row_off); s->d_raw_dims = std::move(d_raw_dims); s->d_raw_vals = std::move(d_raw_vals);
        s->raw_nnz += np;
    }
    s->h_dims.swap(new_dims);
    s->h_key_off.swap(new_ko);
    s->h_dir.swap(new_dir);
    s->h_mult.swap(new_mult);
    s->T = T1;
    s->n = n1;
    s->n_tiles = n_tiles1;
    s->dir_rows = rows1;
    if (out_first_id) *out_first_id = n0;
    return COS_OK;
}

extern "C" int32_t cos_sparse_delete(cos_sparse *s, const uint32_t *ids, const uint64_t *row_offsets, uint32_t m, const uint32_t *raw_dims,
                                     const float *raw_vals, uint64_t *out_removed) {
    if (!s) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (out_removed) *out_removed = 0;
    if (m == 0) return COS_OK;
    if (!ids || !row_offsets) return cos_fail(COS_ERR_INVALID, "bad argument");
    int32_t rc = postings_check_offsets(row_offsets, m, "row_offsets", "vector");
    if (rc) return rc;
    const u64 nd = row_offsets[m];
    if (nd && (!raw_dims || !raw_vals)) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (nd > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 2^31 - 1 pairs in one delete");
    std::lock_guard<std::mutex> g(s->mu);
    const u32 Q = 1u << s->bits, T = s->T;
    // (id, dimension, value) -> the key list on the host's tables; no node, no list for the key: left alone (inverted_index.rs:205-222)
    std::vector<u32> pair_ik, pair_len, pair_slot; // (id, key) interleaved; pair_slot = t * Q + key for the host's counts
    std::vector<u64> pair_begin;
    for (u32 i = 0; i < m; i++) {
        if (ids[i] >= s->n) continue;
        for (u64 p = row_offsets[i]; p < row_offsets[i + 1]; p++) {
            auto it = std::lower_bound(s->h_dims.begin(), s->h_dims.end(), raw_dims[p]);
            if (it == s->h_dims.end() || *it != raw_dims[p]) continue;
            const u32 t = (u32)(it - s->h_dims.begin());
            const u32 key = sparse_quantize(raw_vals[p], s->upper, s->bits);
            const u64 *ko = s->h_key_off.data() + (size_t)t * (Q + 1);
            if (ko[key + 1] == ko[key]) continue;
            pair_ik.push_back(ids[i]);
            pair_ik.push_back(key);
            pair_begin.push_back(ko[0]);
            pair_len.push_back((u32)(ko[Q] - ko[0])); // lists longer than 2^32 - 1 are refused by create and insert
            pair_slot.push_back(t * Q + key);
        }
    }
    const u32 np = (u32)pair_len.size();
    if (!np) return COS_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(0));
    const u64 nnz0 = s->h_key_off[(size_t)(T - 1) * (Q + 1) + Q];
    const u64 n_words = (nnz0 + 31) / 32;
    if ((n_words + 255) / 256 > 0x7FFFFFFFull || (nnz0 + 1023) / 1024 > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "too many postings for one launch");
    const u32 *old_a = s->packed ? s->d_pk.p : s->d_ids.p;
    DevArr<u32> d_ik, d_len, d_flags, d_before;
    DevArr<u64> d_begin;
    DevArr<uint8_t> d_found;
    HIP_TRY(d_ik.alloc((size_t)np * 2)); HIP_TRY(d_len.alloc(np)); HIP_TRY(d_begin.alloc(np)); HIP_TRY(d_found.alloc(np)); HIP_TRY(d_flags.alloc(n_words));
    HIP_TRY(hipMemcpy(d_ik, pair_ik.data(), (size_t)np * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, pair_len.data(), (size_t)np * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_begin, pair_begin.data(), (size_t)np * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d_flags, 0, n_words * 4, 0));
    // (the flags are the call's own: nothing of the handle is written before the swap)
    if (s->packed) hipLaunchKernelGGL(sparse_claim_kernel<true>, dim3((np + 255) / 256), dim3(256), 0, 0, old_a, (const uint8_t *)nullptr, d_ik.p, d_begin.p, d_len.p, np, d_flags.p, d_found.p);
    else hipLaunchKernelGGL(sparse_claim_kernel<false>, dim3((np + 255) / 256), dim3(256), 0, 0, old_a, s->d_keys.p, d_ik.p, d_begin.p, d_len.p, np, d_flags.p, d_found.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> found(np);
    HIP_TRY(hipMemcpy(found.data(), d_found, np, hipMemcpyDeviceToHost));
    // the per-key counts of the pairs the device found: postings_visited stays exact
    std::vector<u64> dec((size_t)T * Q, 0ull);
    u64 removed = 0;
    for (u32 i = 0; i < np; i++)
        if (found[i]) { dec[pair_slot[i]]++; removed++; }
    if (!removed) return COS_OK; // nothing found: nothing swapped
    std::vector<u64> new_ko((size_t)T * (Q + 1));
    {
        u64 run = 0;
        for (u32 t = 0; t < T; t++) {
            const u64 *ko = s->h_key_off.data() + (size_t)t * (Q + 1);
            for (u32 k = 0; k < Q; k++) {
                new_ko[(size_t)t * (Q + 1) + k] = run;
                const u64 have = ko[k + 1] - ko[k], d = dec[(size_t)t * Q + k];
                if (d > have) return cos_fail(COS_ERR_HIP, "delete found %llu postings in a key list of %llu", (unsigned long long)d, (unsigned long long)have);
                run += have - d;
            }
            new_ko[(size_t)t * (Q + 1) + Q] = run;
        }
    }
    const u64 nnz1 = nnz0 - removed;
    // exclusive sum of the flag words' popcounts, compaction into new arrays, their tile directory
    DevBuf d_tmp;
    SparseArrays na;
    HIP_TRY(d_before.alloc(n_words));
    size_t scan_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_before.p, d_before.p, (int)n_words, 0));
    HIP_TRY(d_tmp.alloc(scan_bytes));
    HIP_TRY(na.alloc(s->packed, nnz1));
    hipLaunchKernelGGL(sparse_flag_count_kernel, dim3((u32)((n_words + 255) / 256)), dim3(256), 0, 0, d_flags.p, n_words, d_before.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, scan_bytes, d_before.p, d_before.p, (int)n_words, 0));
    const dim3 grid((u32)((nnz0 + 1023) / 1024));
    if (s->packed) hipLaunchKernelGGL(sparse_compact_kernel<true>, grid, dim3(256), 0, 0, old_a, (const uint8_t *)nullptr, d_flags.p, d_before.p, nnz0, na.a.p, (uint8_t *)nullptr);
    else hipLaunchKernelGGL(sparse_compact_kernel<false>, grid, dim3(256), 0, 0, old_a, s->d_keys.p, d_flags.p, d_before.p, nnz0, na.a.p, na.keys.p);
    HIP_TRY(hipGetLastError());
    std::vector<u32> new_dir;
    DevArr<u32> d_new_dir;
    u32 rows1 = 0;
    rc = sparse_new_dir(s->packed, na.a.p, new_ko, T, Q, s->n_tiles, new_dir, rows1, d_new_dir);
    if (rc) { (void)hipStreamSynchronize(0); return rc; }
    HIP_TRY(hipDeviceSynchronize());
    if (s->packed) s->d_pk = std::move(na.a);
    else { s->d_ids = std::move(na.a); s->d_keys = std::move(na.keys); }
    s->d_tile_dir = std::move(d_new_dir);
    s->h_key_off.swap(new_ko);
    s->h_dir.swap(new_dir);
    s->dir_rows = rows1;
    s->removed += removed; // (h_mult stays: an upper bound is all the COUNTED proof needs)
    if (out_removed) *out_removed = removed;
    return COS_OK;
}

extern "C" int32_t cos_sparse_stats(cos_sparse *s, cos_sparse_index_stats *out) {
    if (!s || !out || out->struct_size != sizeof(cos_sparse_index_stats))
        return cos_fail(COS_ERR_INVALID, "bad argument (struct_size must be sizeof(cos_sparse_index_stats))");
    std::lock_guard<std::mutex> g(s->mu);
    const u32 Q = 1u << s->bits;
    out->n_vectors = s->n;
    out->n_dims = s->T;
    out->dir_rows = s->dir_rows;
    out->dir_tiles = s->n_tiles;
    out->packed = s->packed ? 1u : 0u;
    out->have_raw = s->have_raw ? 1u : 0u;
    out->reserved = 0;
    out->postings = s->h_key_off[(size_t)(s->T - 1) * (Q + 1) + Q];
    out->removed = s->removed;
    out->raw_pairs = s->raw_nnz;
    u64 bytes = (u64)s->d_ids.cap * 4 + s->d_keys.cap + (u64)s->d_pk.cap * 4 + (u64)std::max<size_t>(s->d_tile_dir.cap, 1) * 4; // postings + directory
    bytes += (u64)s->d_row_off.cap * 8 + (u64)s->d_raw_dims.cap * 4 + (u64)s->d_raw_vals.cap * 4;                                 // raw vectors
    for (const DevBuf *w : {&s->w_in, &s->w_part, &s->w_oi, &s->w_os, &s->w_oc}) bytes += w->cap; // search workspace
    out->device_bytes = bytes;
    return COS_OK;
}

extern "C" int32_t cos_sparse_download(cos_sparse *s, uint32_t *n_dims, uint64_t *n_postings, uint32_t *dims, uint64_t *key_offsets, uint32_t *vec_ids) {
    if (!s || !n_dims || !n_postings) return cos_fail(COS_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> g(s->mu);
    const u32 Q = 1u << s->bits, T = s->T;
    const u64 nnz = s->h_key_off[(size_t)(T - 1) * (Q + 1) + Q];
    const u32 cap_t = *n_dims;
    const u64 cap_p = *n_postings;
    *n_dims = T;
    *n_postings = nnz;
    if (!dims && !key_offsets && !vec_ids) return COS_OK; // first call: the sizes
    if (!dims || !key_offsets || !vec_ids) return cos_fail(COS_ERR_INVALID, "bad argument: all three arrays or none");
    if (cap_t < T || cap_p < nnz)
        return cos_fail(COS_ERR_INVALID, "arrays for %u dimensions / %llu postings, the index holds %u / %llu", cap_t, (unsigned long long)cap_p, T, (unsigned long long)nnz);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(0));
    // a persistence / test path: the id-sorted lists come back whole and are split by key on the host
    std::vector<u32> a((size_t)std::max<u64>(nnz, 1));
    std::vector<uint8_t> kb;
    HIP_TRY(hipMemcpy(a.data(), s->packed ? s->d_pk.p : s->d_ids.p, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    if (!s->packed) {
        kb.resize((size_t)std::max<u64>(nnz, 1));
        HIP_TRY(hipMemcpy(kb.data(), s->d_keys.p, (size_t)nnz, hipMemcpyDeviceToHost));
    }
    memcpy(dims, s->h_dims.data(), (size_t)T * 4);
    memcpy(key_offsets, s->h_key_off.data(), (size_t)T * (Q + 1) * 8);
    std::vector<u64> cursor(Q);
    for (u32 t = 0; t < T; t++) {
        const u64 *ko = s->h_key_off.data() + (size_t)t * (Q + 1);
        for (u32 k = 0; k < Q; k++) cursor[k] = ko[k];
        for (u64 p = ko[0]; p < ko[Q]; p++) {
            const u32 key = s->packed ? a[p] >> 24 : kb[p], id = s->packed ? (a[p] & 0xFFFFFFu) - 1u : a[p];
            if (key >= Q || cursor[key] >= ko[key + 1]) return cos_fail(COS_ERR_HIP, "the postings of dimension %u do not match the host's key counts", s->h_dims[t]);
            vec_ids[cursor[key]++] = id;
        }
    }
    return COS_OK;
}
