// kernels_hybrid.hip — BM25 scoring over CSR postings and reciprocal-rank fusion (config c5).
//   SparseAnnQueryBasic::search_bm25   models/sparse_ann_query.rs:149-233
//   get_idf                            models/sparse_ann_query.rs:298-302 (ln_1p on the HOST libm, like the reference)
//   RRF fusion of hybrid_search        api/vectordb/search/repo.rs:311-340
//
// BM25 is HBM-bound streaming work: every posting (8 B: doc id + stored tf) of every query term is read
// once, coalesced.  The reference's document-at-a-time heap merge is restated as a tiled term-at-a-time
// accumulation that produces bit-identical f32 sums: the doc-id space is cut into tiles of TILE ids; inside
// a tile the query's terms are applied in ASCENDING TERM-HASH order (the documented order, oracle/…bm25.c)
// with a workgroup barrier between terms, so each document's score is p0, then +p1, then +p2 … exactly like
// the sequential merge.  Postings of one term are distinct documents, so lanes never collide inside a term.
// The 512 result buckets (doc_id % 512, strictly-greater score wins, first seen = smallest id on ties) are
// an order-independent max over the key (score, ~doc_id): one 64-bit LDS/global atomic max.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>

#include "engine_internal.h"
#include "hybrid_plan.h"
#include "postings_update.h"
#include "topk_select.h"

using namespace cosdev;

namespace {

constexpr u32 BUCKETS = 512;  // sparse_ann_query.rs:154
constexpr u32 TILE = POSTINGS_TILE; // doc ids per LDS accumulator tile (32 KB of f32)
constexpr u32 MAX_QTERMS = 64;
constexpr u32 DIR_MIN = 256;  // posting lists longer than this get a tile directory; shorter ones are scanned whole per tile
constexpr u32 NO_DIR = POSTINGS_NONE;
constexpr int PU = 8;       // postings per thread per chunk

struct QueryTerms { // per query, terms ascending by hash, only those that have a posting list
    u64 begin[MAX_QTERMS];
    u64 end[MAX_QTERMS];
    float idf[MAX_QTERMS];
    u32 dir[MAX_QTERMS]; // row of the term in the tile directory, NO_DIR for short lists
    u32 n;
};

// UNTOUCHED marks a document no term has reached yet: a NaN bit pattern that tf * idf and the sums of such products cannot take
// (cos_bm25_create rejects non-finite stored term frequencies; idf is finite), so the accumulator itself says whether the first
// posting assigns (p0) or a later one adds (+ p1 ...).  It replaces a separate bitmap whose bits were set with LDS atomics: the
// postings of a dense term are consecutive documents, so up to 32 lanes of a wave hit the SAME bitmap word per instruction and the
// hardware serialises same-address atomics — that, not HBM or the barriers, held the kernel at ~1.2 ms per batch on c5 (a
// barrier-free variant with wave-owned 2048-document tiles measured the same 1.3 ms with the bitmap and 0.75 ms without it,
// against 0.66 ms for this one: dropped).
constexpr u32 UNTOUCHED = 0xFFFFFFFFu;

// TOMBSTONE_TF is the stored term frequency of a deleted posting (cos_bm25_delete; the reference overwrites the entry with u64::MAX,
// versioned_vec.rs:141-150, and its iterator skips it, :251-275): another NaN pattern, so no stored tf can take it (create and insert
// reject non-finite values) and it is distinct from UNTOUCHED.  The document id stays in place — the lists stay ascending for the
// tile directory and for the delete's own search — and the posting still counts in the list's length, which is what get_idf sees.
constexpr u32 TOMBSTONE_TF = 0x7FC0DEADu;

// apply one chunk (PU postings per lane, all of ONE term: distinct documents, so the PU read-modify-writes of a lane and those of
// the other lanes never touch the same slot and the reads can all be issued before the first write)
// TOMBS: the index holds tombstones (cos_bm25_delete marked at least one posting).  An index without any runs the instantiation
// without the test, the inner loop it had before deletes existed.
template <u32 N, bool TOMBS>
__device__ __forceinline__ void bm25_apply_chunk(float *acc, u32 d0, float idf, const u32 (&dv)[PU], const float (&tv)[PU], u32 mask) {
    float old[PU];
    bool ok[PU];
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const u32 slot = dv[u] - d0; // out of range (another tile of a short list) wraps to >= N
        ok[u] = ((mask >> u) & 1u) && dv[u] >= d0 && slot < N;
        old[u] = acc[slot & (N - 1)];
    }
#pragma unroll
    for (int u = 0; u < PU; u++) {
        if (ok[u] && (!TOMBS || __float_as_uint(tv[u]) != TOMBSTONE_TF)) { // a deleted posting adds nothing: one compare per posting
            const float p = __fmul_rn(tv[u], idf); // tf * head.idf
            acc[(dv[u] - d0) & (N - 1)] = __float_as_uint(old[u]) != UNTOUCHED ? __fadd_rn(old[u], p) : p;
        }
    }
}

// grid = B * splits blocks: block (q, s) owns the tiles s, s+splits, s+2*splits, ...
// Tile directory: for every posting list longer than DIR_MIN, tile_dir[row][t] = offset (relative to the list's begin) of the
// first posting whose doc id is >= t * TILE, t = 0 .. n_tiles.  It replaces the two ~17-step binary searches every
// (query, tile, term) step used to make — the kernel was latency-bound on them at 0.16 of the HBM roof.
//
// Software pipeline.  A block walks a flat sequence of CHUNKS — (tile, term, PU * 256 consecutive postings of the term's slice
// of the tile) — and always has the NEXT chunk's postings in flight (registers) while it applies the current one to the LDS
// accumulators, across term barriers and tile flushes alike.  Before, a thread's 4 loads were issued, waited for and applied, so
// a CU had ~16 KB in flight half of the time: 2.5 TB/s is what Little's law gives for that at ~1.5 us of loaded HBM latency
// (profiles/archive/r02_c5_hybrid_1M_tile_directory.json).  Now 2 x 16 KB per block, 4 blocks per CU.

struct Bm25Cursor { // block-uniform
    u32 tile, t;
    u64 base, e; // postings [base, min(base + PU * 256, e)) of term t's slice of the tile
    bool valid;
};

// BASED: the handle is one shard of a collection and holds its documents under LOCAL ids (a shard set's text half, shardset.hip): the
// bucket index and the key's id are formed from the GLOBAL id doc_base + local where a tile is flushed; nothing else differs.  A single
// handle runs the BASED = false instantiations, whose last argument is empty: the code they were before shard sets had a text half.
template <bool BASED> struct DocBase { u32 v; };
template <> struct DocBase<false> {};
template <bool TOMBS, bool BASED = false>
__global__ __launch_bounds__(256) void bm25_score_kernel(const u32 *__restrict__ docs, const float *__restrict__ tfs,
                                                         const QueryTerms *__restrict__ qts, u32 n_docs, const u32 *__restrict__ tile_dir,
                                                         u64 *__restrict__ buckets /*[B][512]*/, const u32 *__restrict__ order, u32 splits,
                                                         DocBase<BASED> doc_base) {
    __shared__ float acc[TILE]; // UNTOUCHED (a NaN pattern no score can take) until a term reaches the document
    __shared__ u64 lb[BUCKETS];
    // 1-D grid, heaviest queries first: block id -> (rank in the host's descending-postings order, split).  Query sizes are
    // heavy-tailed (a few Zipf-head terms decide everything), so the blocks of the heaviest queries must not be the last to start.
    const u32 q = order[blockIdx.x / splits];
    const u32 split = blockIdx.x % splits;
    const QueryTerms *qt = &qts[q];
    const u32 nt = qt->n;
    if (nt == 0) return;
    const u32 n_tiles = (n_docs + TILE - 1) / TILE;
    if (split >= n_tiles) return;
    for (u32 i = threadIdx.x; i < BUCKETS; i += blockDim.x) lb[i] = 0ull;
    for (u32 i = threadIdx.x; i < TILE; i += blockDim.x) acc[i] = __uint_as_float(UNTOUCHED);

    auto slice = [&](u32 tile, u32 t, u64 &b, u64 &e) { // term t's postings inside the tile
        const u32 dr = qt->dir[t];
        b = qt->begin[t];
        e = qt->end[t];
        if (dr != NO_DIR) { // straight from the directory
            const u32 *row = tile_dir + (u64)dr * (n_tiles + 1);
            e = b + row[tile + 1];
            b = b + row[tile];
        } // else: a short list is scanned whole and filtered by range (no search at all)
    };
    auto advance = [&](const Bm25Cursor &c) -> Bm25Cursor {
        Bm25Cursor n = c;
        if (c.base + (u64)PU * 256 < c.e) { n.base = c.base + (u64)PU * 256; return n; }
        if (c.t + 1 < nt) n.t = c.t + 1;
        else { n.t = 0; n.tile = c.tile + splits; }
        n.valid = n.tile < n_tiles;
        if (n.valid) slice(n.tile, n.t, n.base, n.e);
        return n;
    };
    // Every load is issued unconditionally (masked lanes read posting 0 and drop it): a fixed number of loads per chunk lets the
    // compiler wait for exactly the older chunk (s_waitcnt vmcnt(2 * PU)) while the newer one stays in flight; with predicated
    // loads it had to drain the queue (vmcnt(0)) before touching the current chunk.
    // The loaded registers are not touched here (the lane mask travels separately): any use would wait for the data.
    auto fetch = [&](const Bm25Cursor &c, u32 (&dv)[PU], float (&tv)[PU]) -> u32 {
        u32 mask = 0;
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const u64 i = c.base + threadIdx.x + (u64)u * 256;
            const bool in = c.valid && i < c.e;
            const u64 ii = in ? i : 0ull;
            dv[u] = docs[ii];
            tv[u] = tfs[ii];
            mask |= (in ? 1u : 0u) << u;
        }
        return mask;
    };
    // apply chunk c (registers dv/tv); nx = the chunk after it (already in flight)
    auto apply = [&](const Bm25Cursor &c, const Bm25Cursor &nx, const u32 (&dv)[PU], const float (&tv)[PU], const u32 mask) {
        const u32 d0 = c.tile * TILE;
        const float idf = qt->idf[c.t];
        bm25_apply_chunk<TILE, TOMBS>(acc, d0, idf, dv, tv, mask);
        const bool term_done = !nx.valid || nx.tile != c.tile || nx.t != c.t;
        const bool tile_done = !nx.valid || nx.tile != c.tile;
        if (term_done) __syncthreads(); // a document's score is p0, then + p1, then + p2 ... in term order
        if (tile_done) {
            for (u32 slot = threadIdx.x; slot < TILE; slot += blockDim.x) {
                const float v = acc[slot];
                if (__float_as_uint(v) != UNTOUCHED) {
                    u32 doc = d0 + slot;
                    if constexpr (BASED) doc += doc_base.v;
                    const u64 key = pack_key(simkey(v), ~doc); // larger score, then smaller doc id
                    atomicMax((unsigned long long *)&lb[doc % BUCKETS], (unsigned long long)key);
                    acc[slot] = __uint_as_float(UNTOUCHED);
                }
            }
            __syncthreads();
        }
    };

    Bm25Cursor cur;
    cur.tile = split; cur.t = 0; cur.valid = true;
    slice(cur.tile, 0, cur.base, cur.e);
    u32 da[PU], db[PU];
    float ta[PU], tb[PU];
    u32 ma = fetch(cur, da, ta), mb;
    __syncthreads();
    for (;;) { // ping-pong between the two register sets: no copies, so nothing waits on the chunk in flight
        const Bm25Cursor n1 = advance(cur);
        mb = fetch(n1, db, tb);
        apply(cur, n1, da, ta, ma);
        if (!n1.valid) break;
        const Bm25Cursor n2 = advance(n1);
        ma = fetch(n2, da, ta);
        apply(n1, n2, db, tb, mb);
        if (!n2.valid) break;
        cur = n2;
    }
    // a query's ~100 blocks all fold into the same 512 global buckets: look before the atomic (a stale read only costs a
    // redundant atomicMax, never a lost one) — a bucket's running maximum is raised ~ln(blocks) times, not `blocks` times
    for (u32 i = threadIdx.x; i < BUCKETS; i += blockDim.x) {
        const u64 v = lb[i];
        if (v && v > __hip_atomic_load(&buckets[(u64)q * BUCKETS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax((unsigned long long *)&buckets[(u64)q * BUCKETS + i], (unsigned long long)v);
    }
}

// What bm25_topk_kernel and bm25_fold_topk_kernel share, from a wave's 512 bucket keys on (lane l holds buckets 8l .. 8l + 7 as the
// scoring kernel left them, (score, ~doc id), 0 = empty): back to (score, doc id), count, sort by (score desc, larger id first), top k
__device__ __forceinline__ void bm25_buckets_topk(u64 (&k)[8], int lane, u32 q, u32 top_k, u32 *__restrict__ out_ids, float *__restrict__ out_scores,
                                                  u32 *__restrict__ out_counts) {
    u32 cnt = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const u64 v = k[r];
        k[r] = v ? pack_key((u32)(v >> 32), ~(u32)v) : 0ull; // back to (score, doc id)
        cnt += v != 0ull;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) cnt += (u32)__shfl_xor((int)cnt, m, 64);
    bitonic_sort_desc<8>(k, lane);
    const u32 n = cnt < top_k ? cnt : top_k;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const u32 e = (u32)lane * 8 + r;
        if (e < n) {
            out_ids[(u64)q * top_k + e] = (u32)k[r];
            out_scores[(u64)q * top_k + e] = simkey_inv((u32)(k[r] >> 32));
        }
    }
    if (lane == 0) out_counts[q] = n;
}

// one wave per query: 512 buckets -> sort by (score desc, larger id first) -> top k
__global__ __launch_bounds__(64) void bm25_topk_kernel(const u64 *__restrict__ buckets, u32 B, u32 top_k, u32 *__restrict__ out_ids,
                                                       float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    u64 k[8];
#pragma unroll
    for (int r = 0; r < 8; r++) k[r] = buckets[(u64)q * BUCKETS + (u32)lane * 8 + r];
    bm25_buckets_topk(k, lane, q, top_k, out_ids, out_scores, out_counts);
}

// The collection's buckets from its S shards' (shardset.hip): one wave per query; gathered[s][q][512] are the keys shard s's scoring
// kernel left, over GLOBAL ids, and the key is an order-independent maximum, so the collection's array is their element-wise u64
// maximum.  Lane l reads buckets 8l .. 8l + 7 of every shard's row — 64 contiguous bytes per lane, 4 KB per row and wave, as four
// 16-byte loads — and the rest is bm25_topk_kernel's.  The lists go where the caller points: the host's staging, or where rrf_kernel
// reads its second list set.
__global__ __launch_bounds__(64) void bm25_fold_topk_kernel(const u64 *__restrict__ gathered, u32 S, u32 B, u32 top_k, u32 *__restrict__ out_ids,
                                                            float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    const int lane = threadIdx.x;
    const u32 q = blockIdx.x;
    if (q >= B) return;
    u64 k[8];
#pragma unroll
    for (int r = 0; r < 8; r++) k[r] = 0ull;
    for (u32 s = 0; s < S; s++) {
        const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(gathered + ((u64)s * B + q) * BUCKETS + (u32)lane * 8);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const ulonglong2 v = row[r];
            k[2 * r] = k[2 * r] > v.x ? k[2 * r] : (u64)v.x;
            k[2 * r + 1] = k[2 * r + 1] > v.y ? k[2 * r + 1] : (u64)v.y;
        }
    }
    bm25_buckets_topk(k, lane, q, top_k, out_ids, out_scores, out_counts);
}

// RRF: one wave per query.  score(id) = [last occurrence in the FIRST list: 1/(rank+k+eps)] then += each occurrence in the SECOND list.
// The body both fusion kernels share, from the query's two rows on: gather into LDS, first-occurrence ownership, overwrite in the
// first list (insert()), add in the second, pack, bitonic sort, write-out.  ids: LDS, [nd + ns].
template <int R>
__device__ __forceinline__ void rrf_fuse_query(u32 *ids, const u32 *__restrict__ first_row, u32 nd, const u32 *__restrict__ second_row, u32 ns, u32 q, float kc,
                                               u32 top_k, u32 *__restrict__ out_ids, float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    const int lane = threadIdx.x;
    const u32 n = nd + ns;
    for (u32 i = lane; i < n; i += 64) ids[i] = i < nd ? first_row[i] : second_row[i - nd];
    __builtin_amdgcn_wave_barrier();
    u64 key[R];
    u32 cnt = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const u32 e = (u32)lane * R + r;
        key[r] = 0ull;
        if (e < n) {
            const u32 id = ids[e];
            bool first = true;
            for (u32 j = 0; j < e; j++) first &= ids[j] != id;
            if (first) { // the first occurrence owns the id
                float score = 0.0f;
                for (u32 j = 0; j < nd; j++)
                    if (ids[j] == id) score = __fdiv_rn(1.0f, __fadd_rn(__fadd_rn((float)j, kc), 1.1920929e-07f)); // insert() overwrites
                for (u32 j = nd; j < n; j++)
                    if (ids[j] == id) score = __fadd_rn(score, __fdiv_rn(1.0f, __fadd_rn(__fadd_rn((float)(j - nd), kc), 1.1920929e-07f)));
                key[r] = pack_key(simkey(score), id);
                cnt++;
            }
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) cnt += (u32)__shfl_xor((int)cnt, m, 64);
    bitonic_sort_desc<R>(key, lane);
    const u32 nout = cnt < top_k ? cnt : top_k;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const u32 e = (u32)lane * R + r;
        if (e < nout) {
            out_ids[(u64)q * top_k + e] = (u32)key[r];
            out_scores[(u64)q * top_k + e] = simkey_inv((u32)(key[r] >> 32));
        }
    }
    if (lane == 0) out_counts[q] = nout;
}

template <int R>
__global__ __launch_bounds__(64) void rrf_kernel(const u32 *__restrict__ dense_ids, const u32 *__restrict__ dense_counts, u32 dense_stride,
                                                 const u32 *__restrict__ sparse_ids, const u32 *__restrict__ sparse_counts, u32 sparse_stride, u32 B,
                                                 float kc, u32 top_k, u32 *__restrict__ out_ids, float *__restrict__ out_scores,
                                                 u32 *__restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32 *ids = (u32 *)smem_raw; // [nd + ns]
    const u32 q = blockIdx.x;
    if (q >= B) return;
    rrf_fuse_query<R>(ids, dense_ids + (u64)q * dense_stride, dense_counts[q], sparse_ids + (u64)q * sparse_stride, sparse_counts[q], q, kc, top_k, out_ids,
                      out_scores, out_counts);
}

// The three list sets of a mixed hybrid batch, each ids [n_x][stride] + counts [n_x]; a set without queries is null and never chosen.
struct RrfListSets {
    const u32 *dense_ids, *dense_counts, *sparse_ids, *sparse_counts, *bm25_ids, *bm25_counts;
};
// One wave per query of the request: slots[q] = (arm, row of its first list, row of its second list) chooses the two lists — (dense,
// sparse), (dense, BM25), (sparse, BM25) — and the rest is rrf_kernel's.  A count is held to the stride: the LDS holds 2 * stride ids.
template <int R>
__global__ __launch_bounds__(64) void rrf_mixed_kernel(const RrfListSets sets, const hybrid_plan::Slot *__restrict__ slots, u32 stride, u32 B, float kc, u32 top_k,
                                                       u32 *__restrict__ out_ids, float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32 *ids = (u32 *)smem_raw; // [2 * stride]
    const u32 q = blockIdx.x;
    if (q >= B) return;
    const hybrid_plan::Slot sl = slots[q];
    const bool first_sparse = sl.arm == hybrid_plan::SPARSE_BM25, second_sparse = sl.arm == hybrid_plan::DENSE_SPARSE;
    const u32 *fi = first_sparse ? sets.sparse_ids : sets.dense_ids, *fc = first_sparse ? sets.sparse_counts : sets.dense_counts;
    const u32 *si = second_sparse ? sets.sparse_ids : sets.bm25_ids, *sc = second_sparse ? sets.sparse_counts : sets.bm25_counts;
    const u32 nd = min(fc[sl.pos_first], stride), ns = min(sc[sl.pos_second], stride);
    rrf_fuse_query<R>(ids, fi + (u64)sl.pos_first * stride, nd, si + (u64)sl.pos_second * stride, ns, q, kc, top_k, out_ids, out_scores, out_counts);
}

} // namespace

struct cos_bm25 {
    int32_t device = 0;
    u32 n_terms = 0, documents_count = 0, max_doc = 0;
    long long max_id_ever = -1; // the largest document id the index has ever held (cos_bm25_insert's id rule); -1 = none
    u64 n_tombstones = 0;
    u32 dir_rows = 0, dir_tiles = 0; // shape of d_tile_dir: [dir_rows][dir_tiles + 1]
    std::vector<u32> term_hashes;
    std::vector<u64> offsets;
    DevArr<u32> d_docs;
    DevArr<float> d_tfs;
    std::vector<u32> dir_row; // [n_terms] row in the tile directory or NO_DIR
    DevArr<u32> d_tile_dir; // [rows][n_tiles + 1]
    // per-handle workspace of the search (grown on demand, reused across calls: no allocation on the query path)
    std::mutex mu;
    DevBuf d_qt;                  // QueryTerms[capB], followed by the launch order u32[capB] in the same allocation
    PinArr<unsigned char> h_qt;   // ... and its pinned host image
    DevArr<u64> d_buckets;
    DevArr<u32> d_ids, d_cnt;
    DevArr<float> d_sc;
    u32 capB = 0, cap_k = 0;
    hipStream_t stream = nullptr;
    // cos_hybrid_search_batch: dense half + fusion (second stream, buffers grown on demand)
    hipStream_t stream_dense = nullptr;
    hipEvent_t ev_sparse = nullptr;
    DevArr<float> d_hq, d_dsc;
    DevArr<u32> d_did, d_dcnt;
    // what goes back to the caller, side by side for ONE copy: [fused ids B x k | fused scores B x k | counts B | dense status B]
    DevArr<u32> d_ret;
    PinArr<u32> h_ret; // its pinned landing area
    ~cos_bm25() { // (cos_bm25_destroy has drained both streams)
        if (stream) (void)hipStreamDestroy(stream);
        if (stream_dense) (void)hipStreamDestroy(stream_dense);
        if (ev_sparse) (void)hipEventDestroy(ev_sparse);
    }
};

extern "C" int32_t cos_bm25_create(int32_t device, const uint32_t *term_hashes, const uint64_t *offsets, uint32_t n_terms, const uint32_t *doc_ids,
                                   const float *tfs, uint32_t documents_count, cos_bm25 **out) {
    if (!term_hashes || !offsets || !doc_ids || !tfs || !out || n_terms == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    *out = nullptr;
    for (u32 t = 1; t < n_terms; t++)
        if (term_hashes[t] <= term_hashes[t - 1]) return cos_fail(COS_ERR_INVALID, "term hashes must be strictly ascending");
    for (u64 i = 0; i < offsets[n_terms]; i++) // compute_bm25_term_frequency (indexes/tf_idf/mod.rs:362-371) of a count is always finite
        if (!std::isfinite(tfs[i])) return cos_fail(COS_ERR_INVALID, "stored term frequency %llu is not finite", (unsigned long long)i);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return cos_fail(COS_ERR_NO_DEVICE, "no HIP device visible; the GPU path has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    cos_bm25 *b = new cos_bm25();
    b->device = device;
    b->n_terms = n_terms;
    b->documents_count = documents_count;
    b->term_hashes.assign(term_hashes, term_hashes + n_terms);
    b->offsets.assign(offsets, offsets + n_terms + 1);
    const u64 nnz = offsets[n_terms];
    for (u32 t = 0; t < n_terms; t++)
        if (offsets[t + 1] > offsets[t]) b->max_doc = std::max(b->max_doc, doc_ids[offsets[t + 1] - 1]); // lists are doc-id ascending
    // tile directory of the long posting lists (one pass over their postings on the host)
    const u32 n_tiles = (b->max_doc + 1 + TILE - 1) / TILE;
    b->dir_row.assign(n_terms, NO_DIR);
    std::vector<u32> dir;
    u32 rows = 0;
    for (u32 t = 0; t < n_terms; t++) {
        const u64 lo = offsets[t], hi = offsets[t + 1];
        if (hi - lo <= DIR_MIN) continue;
        if (hi - lo > 0xFFFFFFFFull) { cos_bm25_destroy(b); return cos_fail(COS_ERR_UNIMPLEMENTED, "posting list of term %u too long", term_hashes[t]); }
        b->dir_row[t] = rows++;
        const size_t base = dir.size();
        dir.resize(base + n_tiles + 1);
        u64 p = lo;
        for (u32 tile = 0; tile <= n_tiles; tile++) {
            const u64 bound = (u64)tile * TILE;
            while (p < hi && doc_ids[p] < bound) p++;
            dir[base + tile] = (u32)(p - lo);
        }
        dir[base + n_tiles] = (u32)(hi - lo);
    }
    hipError_t e = b->d_docs.alloc(nnz);
    if (e == hipSuccess) e = b->d_tfs.alloc(nnz);
    if (e == hipSuccess) e = b->d_tile_dir.alloc(dir.size());
    if (e == hipSuccess) e = hipMemcpy(b->d_docs, doc_ids, nnz * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_tfs, tfs, nnz * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !dir.empty()) e = hipMemcpy(b->d_tile_dir, dir.data(), dir.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { cos_bm25_destroy(b); HIP_TRY(e); }
    if (nnz) b->max_id_ever = b->max_doc;
    b->dir_rows = rows;
    b->dir_tiles = n_tiles;
    *out = b;
    return COS_OK;
}

extern "C" int32_t cos_bm25_destroy(cos_bm25 *b) {
    if (!b) return COS_OK;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->stream_dense) (void)hipStreamSynchronize(b->stream_dense);
    delete b;
    return COS_OK;
}

// host side of a batch: sort each query's terms by hash, look the posting lists up, idf via libm log1pf
// (sparse_ann_query.rs:298-302) -> QueryTerms in pinned memory
//
// Two pieces, shared by a single handle and by the shards of a collection (bm25_set_score): a query term resolved against ONE handle's
// term table, and a handle's QueryTerms filled from resolved terms and an idf.  The idf is a statistic of the COLLECTION: a single handle
// is its own collection, a shard takes the sums over every shard.
struct Bm25Term { // one query term in one handle: its posting list, its row of the tile directory, the list's length (tombstones included)
    u64 begin, end;
    u32 dir, len;
};
static bool bm25_resolve_term(const cos_bm25 *b, u32 h, Bm25Term &r) {
    auto it = std::lower_bound(b->term_hashes.begin(), b->term_hashes.end(), h);
    if (it == b->term_hashes.end() || *it != h) return false; // no node / no term: skipped (:165-167)
    const size_t ti = (size_t)(it - b->term_hashes.begin());
    r.begin = b->offsets[ti];
    r.end = b->offsets[ti + 1];
    r.dir = b->dir_row[ti];
    r.len = (u32)(b->offsets[ti + 1] - b->offsets[ti]);
    return true;
}
// get_idf(documents_count, documents.len()) with the reference's u32 wrap, on the host libm
static float bm25_idf(u32 documents_count, u32 len) { return log1pf(((float)(u32)(documents_count - len) + 0.5f) / ((float)len + 0.5f)); }
static void bm25_push_term(QueryTerms &qt, const Bm25Term &r, float idf) { // the caller has checked qt.n < MAX_QTERMS
    qt.begin[qt.n] = r.begin;
    qt.end[qt.n] = r.end;
    qt.idf[qt.n] = idf;
    qt.dir[qt.n] = r.dir;
    qt.n++;
}
static void bm25_launch_order(cos_bm25 *b, u32 B);

static int32_t bm25_prepare(cos_bm25 *b, const uint32_t *q_terms, const uint32_t *q_offsets, u32 B) {
    QueryTerms *h_qt = b->h_qt.as<QueryTerms>();
    for (u32 q = 0; q < B; q++) {
        std::vector<u32> t(q_terms + q_offsets[q], q_terms + q_offsets[q + 1]);
        std::sort(t.begin(), t.end());
        QueryTerms &qt = h_qt[q];
        qt.n = 0;
        for (u32 h : t) {
            Bm25Term r;
            if (!bm25_resolve_term(b, h, r)) continue;
            if (qt.n == MAX_QTERMS) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than %u matching terms in query %u", MAX_QTERMS, q);
            bm25_push_term(qt, r, bm25_idf(b->documents_count, r.len));
        }
    }
    bm25_launch_order(b, B);
    return COS_OK;
}

static void bm25_launch_order(cos_bm25 *b, u32 B) {
    QueryTerms *h_qt = b->h_qt.as<QueryTerms>();
    // launch order: heaviest query (most postings) first; ties by index
    std::vector<std::pair<u64, u32>> w(B);
    for (u32 q = 0; q < B; q++) {
        u64 tot = 0;
        for (u32 t = 0; t < h_qt[q].n; t++) tot += h_qt[q].end[t] - h_qt[q].begin[t];
        w[q] = {~tot, q};
    }
    std::sort(w.begin(), w.end());
    u32 *order = (u32 *)(h_qt + b->capB);
    for (u32 q = 0; q < B; q++) order[q] = w[q].second;
}

static int32_t bm25_workspace(cos_bm25 *b, u32 B, u32 top_k) {
    if (!b->stream) HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    if (B > b->capB || top_k > b->cap_k) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        const u32 nb = std::max(B, b->capB), nk = std::max(top_k, b->cap_k);
        b->capB = b->cap_k = 0; // (a failure below leaves a workspace for no query: the next call allocates all of it again)
        HIP_TRY(b->d_qt.alloc((size_t)nb * (sizeof(QueryTerms) + 4)));
        HIP_TRY(b->h_qt.alloc((size_t)nb * (sizeof(QueryTerms) + 4)));
        HIP_TRY(b->d_buckets.alloc((size_t)nb * BUCKETS));
        HIP_TRY(b->d_ids.alloc((size_t)nb * nk));
        HIP_TRY(b->d_sc.alloc((size_t)nb * nk));
        HIP_TRY(b->d_cnt.alloc(nb));
        b->capB = nb;
        b->cap_k = nk;
    }
    return COS_OK;
}

// scoring into the handle's bucket array, enqueued on `st`.  BASED: as one shard of a collection, keyed by doc_base + local id
template <bool BASED>
static int32_t bm25_launch_score(cos_bm25 *b, u32 B, hipStream_t st, u32 doc_base) {
    const QueryTerms *d_qt = b->d_qt.as<QueryTerms>(), *h_qt = b->h_qt.as<QueryTerms>();
    HIP_TRY(hipMemcpyAsync(b->d_qt, h_qt, (size_t)B * sizeof(QueryTerms), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->d_qt.as<QueryTerms>() + b->capB, h_qt + b->capB, (size_t)B * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b->d_buckets, 0, (size_t)B * BUCKETS * 8, st));
    const u32 span = b->max_doc + 1; // doc ids are internal ids; the largest one bounds the tile count
    // launch shape: enough blocks that the heaviest query's share is small against the whole launch, few enough that a block's fixed
    // cost (512 buckets, 8192 accumulators to reset and fold per tile) stays small against its postings.  c5, 256 queries
    // (profiles/archive/r02_c5_bm25_*): 2048 blocks 0.72 ms, 4096 0.67, 8192 0.66, 16384 0.69, 32768 0.89.  COS_BM25_BLOCKS overrides (experiments).
    const u32 target_blocks = (u32)std::max<long long>(1, tune_or(TUNE_BM25_BLOCKS, 8192));
    const u32 n_tiles = (span + TILE - 1) / TILE;
    const u32 splits = std::max(1u, std::min(n_tiles, std::max(1u, target_blocks / B)));
    // an index that holds no tombstone (never the target of a delete that found something) keeps the kernel without the tombstone test
    const u32 *d_order = (const u32 *)(d_qt + b->capB);
    DocBase<BASED> base;
    if constexpr (BASED) base.v = doc_base;
    if (b->n_tombstones)
        hipLaunchKernelGGL((bm25_score_kernel<true, BASED>), dim3(B * splits), dim3(256), 0, st, b->d_docs, b->d_tfs, d_qt, span, b->d_tile_dir, b->d_buckets,
                           d_order, splits, base);
    else
        hipLaunchKernelGGL((bm25_score_kernel<false, BASED>), dim3(B * splits), dim3(256), 0, st, b->d_docs, b->d_tfs, d_qt, span, b->d_tile_dir, b->d_buckets,
                           d_order, splits, base);
    HIP_TRY(hipGetLastError());
    return COS_OK;
}

// scoring + bucket top-k enqueued on `st`; outputs are device pointers
static int32_t bm25_launch(cos_bm25 *b, u32 B, u32 top_k, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts, hipStream_t st) {
    int32_t rc = bm25_launch_score<false>(b, B, st, 0u);
    if (rc) return rc;
    hipLaunchKernelGGL(bm25_topk_kernel, dim3(B), dim3(64), 0, st, b->d_buckets, B, top_k, d_out_ids, d_out_scores, d_out_counts);
    HIP_TRY(hipGetLastError());
    return COS_OK;
}

extern "C" int32_t cos_bm25_search_batch_device(cos_bm25 *b, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B, uint32_t top_k,
                                                uint32_t *d_out_ids, float *d_out_scores, uint32_t *d_out_counts, void *stream) {
    if (!b || !q_terms || !q_offsets || !d_out_ids || !d_out_scores || !d_out_counts || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(b->device));
    std::lock_guard<std::mutex> g(b->mu);
    int32_t rc = bm25_workspace(b, B, top_k);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream)); // the pinned term table of the previous batch must have been consumed
    rc = bm25_prepare(b, q_terms, q_offsets, B);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : b->stream;
    rc = bm25_launch(b, B, top_k, d_out_ids, d_out_scores, d_out_counts, st);
    if (rc) return rc;
    if (st != b->stream) HIP_TRY(hipStreamSynchronize(st)); // caller's stream: the pinned table may be reused as soon as we return
    return COS_OK;
}

extern "C" int32_t cos_bm25_search_batch(cos_bm25 *b, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B, uint32_t top_k,
                                         uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (!b || !q_terms || !q_offsets || !out_ids || !out_scores || !out_counts || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(b->device));
    std::lock_guard<std::mutex> g(b->mu);
    int32_t rc = bm25_workspace(b, B, top_k);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    rc = bm25_prepare(b, q_terms, q_offsets, B);
    if (rc) return rc;
    rc = bm25_launch(b, B, top_k, b->d_ids, b->d_sc, b->d_cnt, b->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_ids, b->d_ids, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(out_scores, b->d_sc, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(out_counts, b->d_cnt, (size_t)B * 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return COS_OK;
}

extern "C" int32_t cos_rrf_fuse_batch(const uint32_t *dense_ids, const uint32_t *dense_counts, uint32_t dense_stride, const uint32_t *sparse_ids,
                                      const uint32_t *sparse_counts, uint32_t sparse_stride, uint32_t B, float fusion_constant_k, uint32_t top_k,
                                      uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (!dense_ids || !dense_counts || !sparse_ids || !sparse_counts || !out_ids || !out_scores || !out_counts || B == 0 || top_k == 0)
        return cos_fail(COS_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return cos_fail(COS_ERR_NO_DEVICE, "no HIP device visible; the GPU path has no CPU fallback");
    u32 maxn = 0;
    for (u32 q = 0; q < B; q++) {
        if (dense_counts[q] > dense_stride || sparse_counts[q] > sparse_stride) return cos_fail(COS_ERR_INVALID, "count exceeds stride (query %u)", q);
        maxn = std::max(maxn, dense_counts[q] + sparse_counts[q]);
    }
    if (maxn > 1024) return cos_fail(COS_ERR_UNIMPLEMENTED, "RRF lists longer than 1024 entries");
    DevArr<u32> d_d, d_dc, d_s, d_sc, d_oi, d_oc;
    DevArr<float> d_os;
    HIP_TRY(d_d.alloc((size_t)B * dense_stride));
    HIP_TRY(d_s.alloc((size_t)B * sparse_stride));
    HIP_TRY(d_dc.alloc(B));
    HIP_TRY(d_sc.alloc(B));
    HIP_TRY(d_oi.alloc((size_t)B * top_k));
    HIP_TRY(d_os.alloc((size_t)B * top_k));
    HIP_TRY(d_oc.alloc(B));
    HIP_TRY(hipMemcpy(d_d, dense_ids, (size_t)B * dense_stride * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_s, sparse_ids, (size_t)B * sparse_stride * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_dc, dense_counts, (size_t)B * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_sc, sparse_counts, (size_t)B * 4, hipMemcpyHostToDevice));
    const size_t smem = (size_t)std::max(maxn, 1u) * 4;
#define LAUNCH(R) hipLaunchKernelGGL(rrf_kernel<R>, dim3(B), dim3(64), smem, 0, d_d, d_dc, dense_stride, d_s, d_sc, sparse_stride, B, fusion_constant_k, top_k, d_oi, d_os, d_oc)
    if (maxn <= 64) LAUNCH(1);
    else if (maxn <= 128) LAUNCH(2);
    else if (maxn <= 256) LAUNCH(4);
    else if (maxn <= 512) LAUNCH(8);
    else LAUNCH(16);
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_ids, d_oi, (size_t)B * top_k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_scores, d_os, (size_t)B * top_k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, d_oc, (size_t)B * 4, hipMemcpyDeviceToHost));
    return COS_OK;
}


// ------------------------------------------------------------------------------------------------
// repo::hybrid_search (api/vectordb/search/repo.rs:168-341) in one call: the dense index and the BM25 index are each asked
// for top_k * 3 (:200, :240, :251) — here concurrently, on two streams of the same device — and the two lists are fused with
// RRF on the device; only the fused top_k crosses PCIe.
// ------------------------------------------------------------------------------------------------
extern "C" int32_t cos_hybrid_search_batch(cos_index *ix, cos_bm25 *b, const float *queries, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B,
                                           uint32_t top_k, float fusion_constant_k, uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (!ix || !b || !queries || !q_terms || !q_offsets || !out_ids || !out_scores || !out_counts || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ix->p.device != b->device) return cos_fail(COS_ERR_INVALID, "the dense index and the BM25 index live on different devices");
    const u32 k3 = 3 * top_k, maxn = 2 * k3;
    if (maxn > 1024) return cos_fail(COS_ERR_UNIMPLEMENTED, "top_k above 170: RRF lists longer than 1024 entries");
    HIP_TRY(hipSetDevice(b->device));
    std::lock_guard<std::mutex> g(b->mu);
    int32_t rc = bm25_workspace(b, B, k3);
    if (rc) return rc;
    hipStream_t sd = nullptr;
    rc = bm25_dense_stream(b, &sd);
    if (rc) return rc;
    if (!b->ev_sparse) HIP_TRY(hipEventCreateWithFlags(&b->ev_sparse, hipEventDisableTiming));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream_dense));
    const size_t dim = ix->p.dim;
    HIP_TRY(b->d_hq.grow((size_t)B * dim));
    HIP_TRY(b->d_did.grow((size_t)B * k3));
    HIP_TRY(b->d_dsc.grow((size_t)B * k3));
    HIP_TRY(b->d_dcnt.grow((size_t)B));
    const size_t nk = (size_t)B * top_k, ret_words = 2 * nk + 2 * (size_t)B;
    HIP_TRY(b->d_ret.grow(ret_words));
    HIP_TRY(b->h_ret.grow(ret_words));
    u32 *d_fid = b->d_ret, *d_fcnt = b->d_ret + 2 * nk;
    float *d_fsc = (float *)(b->d_ret + nk);
    int32_t *d_dst = (int32_t *)(b->d_ret + 2 * nk + B);
    // The dense half goes FIRST, on a stream of the highest priority: its walk is a chain of dependent rounds on a quarter of the chip's
    // wave slots (one workgroup per query), the sparse half is a bandwidth kernel of 8192 workgroups that fills whatever the walk
    // leaves free.  Until round 6 the sparse half was enqueued first: its workgroups held every CU until they drained and the dense
    // half's first dispatch (the query copy) waited for them — the two halves ran one after the other (c5: 2.55 ms per batch,
    // profiles/r06_final_kernel_trace_c5_rocprofv3.txt: a 256-workgroup copy of 0.52 ms beside a 0.57 ms bm25_score_kernel).
    HIP_TRY(hipMemcpyAsync(b->d_hq, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, sd));
    rc = cos_search_batch_device(ix, b->d_hq, B, k3, b->d_did, b->d_dsc, b->d_dcnt, d_dst, sd);
    if (rc) return rc;
    // sparse half on its stream, beside the walk; its host side (the term table of the batch) is prepared while the device already walks
    rc = bm25_prepare(b, q_terms, q_offsets, B);
    if (rc) return rc;
    rc = bm25_launch(b, B, k3, b->d_ids, b->d_sc, b->d_cnt, b->stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(b->ev_sparse, b->stream));
    // fusion once both lists are there
    HIP_TRY(hipStreamWaitEvent(sd, b->ev_sparse, 0));
    rc = rrf_fuse_device(b->d_did, b->d_dcnt, b->d_ids, b->d_cnt, k3, B, fusion_constant_k, top_k, d_fid, d_fsc, d_fcnt, sd);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(b->h_ret, b->d_ret, ret_words * 4, hipMemcpyDeviceToHost, sd)); // (until round 6: four pageable copies)
    HIP_TRY(hipStreamSynchronize(sd));
    const u32 *hr = b->h_ret;
    memcpy(out_ids, hr, nk * 4);
    memcpy(out_scores, hr + nk, nk * 4);
    memcpy(out_counts, hr + 2 * nk, (size_t)B * 4);
    const int32_t *status = (const int32_t *)(hr + 2 * nk + B);
    for (u32 q = 0; q < B; q++)
        if (status[q] != COS_OK) return cos_fail(status[q], "dense half: query %u failed with status %d (zero-norm vector -> DistanceError::CalculationError)", q, status[q]);
    return COS_OK;
}

// ------------------------------------------------------------------------------------------------
// The BM25 handle as one shard of a collection (shardset.hip: cos_shardset_bm25_search_batch, cos_shardset_hybrid_search_batch).
// Handle s holds the documents of shard s under local ids.  What makes the sharded answer the whole index's, bit for bit:
//   * idf: N = the sum of the shards' documents_count, len = the sum of the term's list lengths (tombstones included), through the
//     expression a single handle uses (bm25_idf);
//   * a document lives in one shard, and a term without a list there adds nothing to it: with the collection's idf the shard's kernel
//     adds the same products in the same (term-hash) order as the whole index's;
//   * the bucket key (score, ~GLOBAL id) is an order-independent maximum, so the collection's buckets are the element-wise maximum of
//     the shards' (bm25_fold_topk_kernel).
// ------------------------------------------------------------------------------------------------
namespace cosdev {
std::mutex &bm25_mutex(cos_bm25 *b) { return b->mu; }
int32_t bm25_device(const cos_bm25 *b) { return b->device; }
long long bm25_largest_id(const cos_bm25 *b) { return b->max_id_ever; }
hipStream_t bm25_stream(cos_bm25 *b) { return b->stream; }
const u64 *bm25_buckets(const cos_bm25 *b) { return b->d_buckets; }

int32_t bm25_dense_stream(cos_bm25 *b, hipStream_t *out) {
    if (!b->stream_dense) {
        int prio_low = 0, prio_high = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        HIP_TRY(hipStreamCreateWithPriority(&b->stream_dense, hipStreamNonBlocking, prio_high));
    }
    *out = b->stream_dense;
    return COS_OK;
}

int32_t bm25_set_score(cos_bm25 *const *hs, const u32 *doc_bases, u32 S, const uint32_t *q_terms, const uint32_t *q_offsets, u32 B) {
    u32 N = 0; // TFIDFIndexRoot::total_documents_count of the collection (u32 arithmetic, like a handle's own count)
    for (u32 s = 0; s < S; s++) {
        cos_bm25 *b = hs[s];
        HIP_TRY(hipSetDevice(b->device));
        int32_t rc = bm25_workspace(b, B, 1);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(b->stream)); // the pinned term table of the previous batch must have been consumed
        N += b->documents_count;
    }
    std::vector<Bm25Term> res(S);
    std::vector<char> has(S);
    for (u32 q = 0; q < B; q++) {
        std::vector<u32> t(q_terms + q_offsets[q], q_terms + q_offsets[q + 1]);
        std::sort(t.begin(), t.end());
        for (u32 s = 0; s < S; s++) hs[s]->h_qt.as<QueryTerms>()[q].n = 0;
        u32 matched = 0; // terms with a list in ANY shard: what the whole index's table would hold of this query
        for (u32 h : t) {
            u64 len = 0;
            bool any = false;
            for (u32 s = 0; s < S; s++) {
                has[s] = bm25_resolve_term(hs[s], h, res[s]);
                if (has[s]) { any = true; len += res[s].len; }
            }
            if (!any) continue;
            if (matched == MAX_QTERMS) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than %u matching terms in query %u", MAX_QTERMS, q);
            matched++;
            const float idf = bm25_idf(N, (u32)len);
            for (u32 s = 0; s < S; s++)
                if (has[s]) bm25_push_term(hs[s]->h_qt.as<QueryTerms>()[q], res[s], idf);
        }
    }
    for (u32 s = 0; s < S; s++) {
        cos_bm25 *b = hs[s];
        bm25_launch_order(b, B);
        HIP_TRY(hipSetDevice(b->device));
        int32_t rc = bm25_launch_score<true>(b, B, b->stream, doc_bases[s]);
        if (rc) return rc;
    }
    return COS_OK;
}

int32_t bm25_fold_topk(const u64 *d_gathered, u32 S, u32 B, u32 top_k, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts, hipStream_t st) {
    hipLaunchKernelGGL(bm25_fold_topk_kernel, dim3(B), dim3(64), 0, st, d_gathered, S, B, top_k, d_out_ids, d_out_scores, d_out_counts);
    HIP_TRY(hipGetLastError());
    return COS_OK;
}

int32_t rrf_fuse_device(const u32 *d_first_ids, const u32 *d_first_counts, const u32 *d_second_ids, const u32 *d_second_counts, u32 k3, u32 B,
                        float fusion_constant_k, u32 top_k, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts, hipStream_t st) {
    const u32 maxn = 2 * k3;
    if (maxn > 1024) return cos_fail(COS_ERR_UNIMPLEMENTED, "top_k above 170: RRF lists longer than 1024 entries");
    const size_t smem = (size_t)maxn * 4;
#define LAUNCH(R) hipLaunchKernelGGL(rrf_kernel<R>, dim3(B), dim3(64), smem, st, d_first_ids, d_first_counts, k3, d_second_ids, d_second_counts, k3, B, fusion_constant_k, top_k, d_out_ids, d_out_scores, d_out_counts)
    if (maxn <= 64) LAUNCH(1);
    else if (maxn <= 128) LAUNCH(2);
    else if (maxn <= 256) LAUNCH(4);
    else if (maxn <= 512) LAUNCH(8);
    else LAUNCH(16);
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    return COS_OK;
}

int32_t rrf_mixed_device(const u32 *d_dense_ids, const u32 *d_dense_counts, const u32 *d_sparse_ids, const u32 *d_sparse_counts, const u32 *d_bm25_ids,
                         const u32 *d_bm25_counts, const hybrid_plan::Slot *d_slots, u32 k3, u32 B, float fusion_constant_k, u32 top_k, u32 *d_out_ids,
                         float *d_out_scores, u32 *d_out_counts, hipStream_t st) {
    const RrfListSets sets{d_dense_ids, d_dense_counts, d_sparse_ids, d_sparse_counts, d_bm25_ids, d_bm25_counts};
    const size_t smem = (size_t)2 * k3 * 4;
#define LAUNCH(R) hipLaunchKernelGGL(rrf_mixed_kernel<R>, dim3(B), dim3(64), smem, st, sets, d_slots, k3, B, fusion_constant_k, top_k, d_out_ids, d_out_scores, d_out_counts)
    switch (hybrid_plan::rrf_keys_per_lane(2 * k3)) {
    case 0: return cos_fail(COS_ERR_UNIMPLEMENTED, "top_k above 170: RRF lists longer than 1024 entries");
    case 1: LAUNCH(1); break;
    case 2: LAUNCH(2); break;
    case 4: LAUNCH(4); break;
    case 8: LAUNCH(8); break;
    default: LAUNCH(16); break;
    }
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    return COS_OK;
}
} // namespace cosdev


// ------------------------------------------------------------------------------------------------
// repo::batch_hybrid_search (api/vectordb/search/repo.rs:343-555) in one call: every query names its arm, the three batch searches
// run side by side for top_k * 3, each over its own sub-batch only, and rrf_mixed_kernel fuses every query's two lists on the device.
// The host-only part (the split of arm[], the limits) is hybrid_plan.h.
// ------------------------------------------------------------------------------------------------
static_assert(hybrid_plan::OK == COS_OK && hybrid_plan::INVALID == COS_ERR_INVALID && hybrid_plan::UNIMPLEMENTED == COS_ERR_UNIMPLEMENTED &&
                  hybrid_plan::NOT_READY == COS_ERR_NOT_READY, "hybrid_plan.h restates cos_status");
static_assert(hybrid_plan::DENSE_SPARSE == COS_HYBRID_DENSE_SPARSE && hybrid_plan::DENSE_BM25 == COS_HYBRID_DENSE_BM25 &&
                  hybrid_plan::SPARSE_BM25 == COS_HYBRID_SPARSE_BM25, "hybrid_plan.h restates the arms");
static_assert(sizeof(hybrid_plan::Slot) == 12, "three words per query");
static_assert(hybrid_plan::MAX_LIST == BUCKETS, "a BM25 list is at most its buckets");

struct cos_hybrid {
    int32_t device = 0;
    std::mutex mu; // one call at a time; taken before the sparse handle's lock, that before the BM25 handle's
    // three non-blocking streams: the dense half (highest priority; the fusion and the copy back follow on it), the sparse half, the BM25 half
    hipStream_t st_dense = nullptr, st_sparse = nullptr, st_bm25 = nullptr;
    hipEvent_t ev_sparse = nullptr, ev_bm25 = nullptr;
    std::vector<hybrid_plan::Slot> slots; // the request's query_mapping (host)
    // what goes up in ONE copy: [dense queries n_dense x dim f32 | Slot x B] (the queries first: they keep the allocation's alignment), pinned image and device block
    PinArr<unsigned char> h_in;
    DevBuf d_in;
    // the three list sets [n_x][3 * top_k] + counts [n_x] (grow-only)
    DevArr<u32> d_did, d_dcnt, d_sid, d_scnt, d_bid, d_bcnt;
    DevArr<float> d_dsc, d_ssc, d_bsc;
    // what comes back in ONE copy: [fused ids B x k | fused scores B x k | counts B | dense status n_dense], device block and pinned landing area
    DevArr<u32> d_ret;
    PinArr<u32> h_ret;
    ~cos_hybrid() { // (cos_hybrid_destroy has drained the streams)
        if (st_dense) (void)hipStreamDestroy(st_dense);
        if (st_sparse) (void)hipStreamDestroy(st_sparse);
        if (st_bm25) (void)hipStreamDestroy(st_bm25);
        if (ev_sparse) (void)hipEventDestroy(ev_sparse);
        if (ev_bm25) (void)hipEventDestroy(ev_bm25);
    }
};

static int32_t hybrid_drain(cos_hybrid *h) {
    HIP_TRY(hipStreamSynchronize(h->st_sparse));
    HIP_TRY(hipStreamSynchronize(h->st_bm25));
    HIP_TRY(hipStreamSynchronize(h->st_dense));
    return COS_OK;
}

extern "C" int32_t cos_hybrid_destroy(cos_hybrid *h) {
    if (!h) return COS_OK;
    (void)hipSetDevice(h->device);
    if (h->st_dense && h->st_sparse && h->st_bm25) (void)hybrid_drain(h);
    delete h;
    return COS_OK;
}

extern "C" int32_t cos_hybrid_create(int32_t device, cos_hybrid **out) {
    if (!out) return cos_fail(COS_ERR_INVALID, "bad argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return cos_fail(COS_ERR_NO_DEVICE, "no HIP device visible; the GPU path has no CPU fallback");
    if (device < 0 || device >= ndev) return cos_fail(COS_ERR_INVALID, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));
    cos_hybrid *h = new cos_hybrid();
    h->device = device;
    int prio_low = 0, prio_high = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->st_dense, hipStreamNonBlocking, prio_high);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->st_sparse, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->st_bm25, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_sparse, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_bm25, hipEventDisableTiming);
    if (e != hipSuccess) { delete h; HIP_TRY(e); }
    *out = h;
    return COS_OK;
}

extern "C" int32_t cos_hybrid_search_mixed(cos_hybrid *h, cos_index *ix, cos_sparse *sp, cos_bm25 *bm, const cos_hybrid_request *rq, uint32_t *out_ids,
                                           float *out_scores, uint32_t *out_counts) {
    namespace hp = hybrid_plan;
    if (!h || !rq || !out_ids || !out_scores || !out_counts) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (rq->struct_size < sizeof(cos_hybrid_request)) return cos_fail(COS_ERR_INVALID, "cos_hybrid_request.struct_size %u, expected %zu", rq->struct_size, sizeof(cos_hybrid_request));
    const u32 B = rq->B, top_k = rq->top_k, rf = rq->sparse_reranking_factor;
    int32_t rc = hp::check_request(rq->struct_size, (u32)sizeof(cos_hybrid_request), B, top_k);
    if (rc == COS_ERR_UNIMPLEMENTED) return cos_fail(rc, "top_k above %u: every half is asked for 3 * top_k, BM25 keeps %u buckets and the fusion holds two such lists", hp::MAX_TOP_K, BUCKETS);
    if (rc || !rq->arm) return cos_fail(COS_ERR_INVALID, "bad argument (B %u, top_k %u)", B, top_k);
    const u32 k3 = hp::LIST_FACTOR * top_k;
    std::lock_guard<std::mutex> gh(h->mu);
    // ---- the request's query_mapping and everything that refuses it: nothing is enqueued before the last check ----
    try {
        h->slots.resize(B);
    } catch (const std::bad_alloc &) {
        return cos_fail(COS_ERR_INVALID, "batch of %u queries", B);
    }
    hp::Split n;
    u32 bad = 0;
    if (hp::split(rq->arm, B, h->slots.data(), n, &bad)) return cos_fail(COS_ERR_INVALID, "arm %u of query %u", (u32)rq->arm[bad], bad);
    if (hp::check_handles(n, ix != nullptr, sp != nullptr, bm != nullptr))
        return cos_fail(COS_ERR_INVALID, "a handle is NULL whose half has queries (dense %u, sparse %u, BM25 %u)", n.n_dense, n.n_sparse, n.n_bm25);
    if ((n.n_dense && !rq->dense_queries) || (n.n_sparse && (!rq->sparse_dims || !rq->sparse_vals || !rq->sparse_offsets)) || (n.n_bm25 && (!rq->bm25_terms || !rq->bm25_offsets)))
        return cos_fail(COS_ERR_INVALID, "the queries of a half that has some are NULL");
    if ((n.n_dense && ix->p.device != h->device) || (n.n_sparse && sparse_device(sp) != h->device) || (n.n_bm25 && bm->device != h->device))
        return cos_fail(COS_ERR_INVALID, "the indexes of a hybrid call live on the device of its cos_hybrid (%d)", h->device);
    if (n.n_sparse && !hp::offsets_ascend(rq->sparse_offsets, n.n_sparse)) return cos_fail(COS_ERR_INVALID, "sparse query offsets decrease");
    if (n.n_bm25 && !hp::offsets_ascend(rq->bm25_offsets, n.n_bm25)) return cos_fail(COS_ERR_INVALID, "BM25 query offsets decrease");
    std::unique_lock<std::mutex> gs, gb; // cos_hybrid -> cos_sparse -> cos_bm25, each held until the synchronise below
    if (n.n_sparse) {
        gs = std::unique_lock<std::mutex>(sparse_mutex(sp));
        hp::SparseLimits lim{};
        sparse_limits(sp, &lim.max_candidates, &lim.have_raw, &lim.batch_bound);
        rc = hp::check_sparse(n.n_sparse, top_k, rf, lim);
        if (rc == COS_ERR_NOT_READY) return cos_fail(rc, "raw-value rerank needs the raw sparse vectors (cos_sparse_create row_offsets / raw_dims / raw_vals)");
        if (rc == COS_ERR_UNIMPLEMENTED) return cos_fail(rc, "3 x top_k x reranking_factor must be <= %u (cos_sparse_set_max_candidates)", lim.max_candidates);
        if (rc) return cos_fail(rc, "sparse sub-batch of %u queries", n.n_sparse);
    }
    if (n.n_bm25) gb = std::unique_lock<std::mutex>(bm->mu);
    HIP_TRY(hipSetDevice(h->device));
    rc = hybrid_drain(h); // a call that failed half-way may have left work behind: the staging is free only now
    if (rc) return rc;
    // ---- buffers (grow-only; no allocation once warm) ----
    const size_t dim = n.n_dense ? ix->p.dim : 0;
    const size_t in_bytes = (size_t)B * sizeof(hp::Slot) + (size_t)n.n_dense * dim * 4;
    HIP_TRY(h->h_in.grow(in_bytes));
    HIP_TRY(h->d_in.grow(in_bytes));
    if (n.n_dense) { HIP_TRY(h->d_did.grow((size_t)n.n_dense * k3)); HIP_TRY(h->d_dsc.grow((size_t)n.n_dense * k3)); HIP_TRY(h->d_dcnt.grow(n.n_dense)); }
    if (n.n_sparse) { HIP_TRY(h->d_sid.grow((size_t)n.n_sparse * k3)); HIP_TRY(h->d_ssc.grow((size_t)n.n_sparse * k3)); HIP_TRY(h->d_scnt.grow(n.n_sparse)); }
    if (n.n_bm25) { HIP_TRY(h->d_bid.grow((size_t)n.n_bm25 * k3)); HIP_TRY(h->d_bsc.grow((size_t)n.n_bm25 * k3)); HIP_TRY(h->d_bcnt.grow(n.n_bm25)); }
    const size_t nk = (size_t)B * top_k, ret_words = 2 * nk + (size_t)B + n.n_dense;
    HIP_TRY(h->d_ret.grow(ret_words));
    HIP_TRY(h->h_ret.grow(ret_words));
    u32 *d_fid = h->d_ret, *d_fcnt = h->d_ret + 2 * nk;
    float *d_fsc = (float *)(h->d_ret + nk);
    int32_t *d_dst = (int32_t *)(h->d_ret + 2 * nk + B);
    if (n.n_bm25) {
        rc = bm25_workspace(bm, n.n_bm25, k3);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(bm->stream)); // the handle's own batches have consumed its pinned term table
        if (bm->stream_dense) HIP_TRY(hipStreamSynchronize(bm->stream_dense));
    }
    // ---- enqueue.  From here a failure drains the three streams before the locks go. ----
    auto fail = [&](int32_t code) { (void)hybrid_drain(h); return code; };
#define HYB_TRY(expr)                                                                                                                                  \
    do {                                                                                                                                               \
        const hipError_t _e = (expr);                                                                                                                  \
        if (_e != hipSuccess) return fail(cos_fail(COS_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__));                  \
    } while (0)
    // The dense half goes FIRST, on the stream of the highest priority, as in cos_hybrid_search_batch: its walk is a chain of
    // dependent rounds on a part of the chip, the two postings scans are bandwidth kernels that fill what it leaves free.  The mapping rides
    // in the same copy as the dense queries.
    const size_t q_bytes = (size_t)n.n_dense * dim * 4;
    if (n.n_dense) memcpy(h->h_in.p, rq->dense_queries, q_bytes);
    memcpy(h->h_in.p + q_bytes, h->slots.data(), (size_t)B * sizeof(hp::Slot));
    HYB_TRY(hipMemcpyAsync(h->d_in.p, h->h_in.p, in_bytes, hipMemcpyHostToDevice, h->st_dense));
    if (n.n_dense) {
        rc = cos_search_batch_device(ix, (const float *)h->d_in.p, n.n_dense, k3, h->d_did, h->d_dsc, h->d_dcnt, d_dst, h->st_dense);
        if (rc) return fail(rc);
    }
    // the sparse half next, on its stream: host resolution while the device already walks.  Sparse before BM25 in the SPARSE_BM25 arm: not measured.
    if (n.n_sparse) {
        rc = sparse_search_locked(sp, rq->sparse_dims, rq->sparse_vals, rq->sparse_offsets, n.n_sparse, k3, rq->sparse_early_terminate_threshold, rf, h->d_sid,
                                  h->d_ssc, h->d_scnt, h->st_sparse);
        if (rc) return fail(rc);
        HYB_TRY(hipEventRecord(h->ev_sparse, h->st_sparse));
    }
    if (n.n_bm25) {
        rc = bm25_prepare(bm, rq->bm25_terms, rq->bm25_offsets, n.n_bm25);
        if (rc) return fail(rc);
        rc = bm25_launch(bm, n.n_bm25, k3, h->d_bid, h->d_bsc, h->d_bcnt, h->st_bm25);
        if (rc) return fail(rc);
        HYB_TRY(hipEventRecord(h->ev_bm25, h->st_bm25));
    }
    // fusion once the halves that ran are there
    hipStream_t sf = h->st_dense;
    if (n.n_sparse) HYB_TRY(hipStreamWaitEvent(sf, h->ev_sparse, 0));
    if (n.n_bm25) HYB_TRY(hipStreamWaitEvent(sf, h->ev_bm25, 0));
    const hp::Slot *d_slots = (const hp::Slot *)(h->d_in.p + q_bytes);
    rc = rrf_mixed_device(n.n_dense ? h->d_did.p : nullptr, n.n_dense ? h->d_dcnt.p : nullptr, n.n_sparse ? h->d_sid.p : nullptr, n.n_sparse ? h->d_scnt.p : nullptr,
                          n.n_bm25 ? h->d_bid.p : nullptr, n.n_bm25 ? h->d_bcnt.p : nullptr, d_slots, k3, B, rq->fusion_constant_k, top_k, d_fid, d_fsc, d_fcnt, sf);
    if (rc) return fail(rc); // (2 * k3 <= 1024: checked above)
    HYB_TRY(hipMemcpyAsync(h->h_ret, h->d_ret, ret_words * 4, hipMemcpyDeviceToHost, sf));
    HYB_TRY(hipStreamSynchronize(sf));
#undef HYB_TRY
    const u32 *hr = h->h_ret;
    const int32_t *status = (const int32_t *)(hr + 2 * nk + B);
    for (u32 q = 0; q < B; q++) { // the first failing query in request order
        const hp::Slot &sl = h->slots[q];
        if (hp::arm_has_dense(sl.arm) && status[sl.pos_first] != COS_OK)
            return cos_fail(status[sl.pos_first], "dense half: query %u failed with status %d (zero-norm vector -> DistanceError::CalculationError)", q, status[sl.pos_first]);
    }
    for (u32 q = 0; q < B; q++) { // entries past a query's count are not written
        const u32 c = std::min(hr[2 * nk + q], top_k);
        memcpy(out_ids + (size_t)q * top_k, hr + (size_t)q * top_k, (size_t)c * 4);
        memcpy(out_scores + (size_t)q * top_k, hr + nk + (size_t)q * top_k, (size_t)c * 4);
        out_counts[q] = c;
    }
    return COS_OK;
}


// ------------------------------------------------------------------------------------------------
// Updates of the resident postings: cos_bm25_insert / cos_bm25_delete / cos_bm25_stats / cos_bm25_download.
//   TFIDFIndex::insert                     indexes/tf_idf/mod.rs:85-110   (documents_count += 1; (doc id, tf) to the END of every term's list)
//   TFIDFIndex::mark_embedding_as_deleted  indexes/tf_idf/mod.rs:112-141  (documents_count -= 1; the first entry with the id becomes a tombstone)
//   TFIDFIndexNode::insert / delete        models/tf_idf_index.rs:212-266
//   VersionedVec::push_sorted / delete     models/versioned_vec.rs:131-150, :205-222; the iterator that skips tombstones :251-275
//
// The postings never go back through the host.  The host owns the term table (term_hashes, offsets: O(n_terms)) and sees the
// update itself (O(size of the update)); the device turns the document-major update into term-major order (stable radix sort by
// term hash: ids arrive ascending, so every term's new postings come out ascending), streams old list + new postings of every term
// into NEW arrays (postings_merge_kernel<Bm25Merge>, postings_update.h: 8 B read + 8 B written per posting of the new array), and
// searches the tile directory of the new arrays (postings_tile_dir_kernel<Bm25Ids>).  Only then are the handle's pointers swapped
// and the old arrays freed: a call that fails before that point leaves the handle exactly as it was.
// ------------------------------------------------------------------------------------------------
namespace {

// delta in term-major order: perm = the stable sort's permutation of the update's postings
__global__ __launch_bounds__(256) void bm25_delta_gather_kernel(const u32 *__restrict__ perm, const u32 *__restrict__ pdocs, const float *__restrict__ ptfs,
                                                                u32 n, u32 *__restrict__ out_docs, float *__restrict__ out_tfs) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 s = perm[i];
    out_docs[i] = pdocs[s];
    out_tfs[i] = ptfs[s];
}

// the posting format of postings_update.h: a document id and a stored term frequency, in two arrays; the delta has the same shape
struct Bm25Ids {
    const u32 *__restrict__ docs;
    __device__ __forceinline__ u32 operator()(u64 p) const { return docs[p]; }
};
struct Bm25Merge {
    const u32 *__restrict__ old_docs;
    const float *__restrict__ old_tfs;
    const u32 *__restrict__ del_docs;
    const float *__restrict__ del_tfs;
    u32 *__restrict__ new_docs;
    float *__restrict__ new_tfs;
    struct P { u32 d; float f; };
    __device__ __forceinline__ P zero() const { return {0u, 0.0f}; }
    __device__ __forceinline__ P from_old(u64 p) const { return {old_docs[p], old_tfs[p]}; }
    __device__ __forceinline__ P from_delta(u64 p) const { return {del_docs[p], del_tfs[p]}; }
    __device__ __forceinline__ void store4(u64 j, const P (&v)[4]) const {
        *reinterpret_cast<uint4 *>(new_docs + j) = make_uint4(v[0].d, v[1].d, v[2].d, v[3].d);
        *reinterpret_cast<float4 *>(new_tfs + j) = make_float4(v[0].f, v[1].f, v[2].f, v[3].f);
    }
    __device__ __forceinline__ void store1(u64 j, const P &v) const { new_docs[j] = v.d; new_tfs[j] = v.f; }
};

// one thread per (document, term) pair of a delete call whose term has a list: lower-bound search for the id, mark the posting if it
// is there and not yet marked (the exchange makes two pairs naming the same posting count it once), count what was marked
__global__ __launch_bounds__(256) void bm25_tombstone_kernel(const u32 *__restrict__ docs, float *__restrict__ tfs, const u32 *__restrict__ pair_doc,
                                                             const u64 *__restrict__ pair_begin, const u32 *__restrict__ pair_len, u32 n_pairs,
                                                             u32 *__restrict__ marked) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const u64 lo = pair_begin[i], hi = lo + pair_len[i];
    const u32 doc = pair_doc[i];
    const u64 pos = postings_lower_bound(Bm25Ids{docs}, lo, hi, doc);
    if (pos < hi && docs[pos] == doc) {
        const u32 old = atomicExch(reinterpret_cast<unsigned int *>(tfs + pos), TOMBSTONE_TF);
        if (old != TOMBSTONE_TF) atomicAdd(marked, 1u);
    }
}

// updates wait for everything the handle has in flight (the caller holds b->mu): a search sees the index before or after, never between
int32_t bm25_quiesce(cos_bm25 *b) {
    HIP_TRY(hipSetDevice(b->device));
    if (!b->stream) HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->stream_dense) HIP_TRY(hipStreamSynchronize(b->stream_dense));
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_bm25_insert(cos_bm25 *b, const uint32_t *doc_ids, const uint64_t *doc_offsets, uint32_t m, const uint32_t *term_hashes,
                                   const float *tfs) {
    if (!b) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (m == 0) return COS_OK;
    if (!doc_ids || !doc_offsets) return cos_fail(COS_ERR_INVALID, "bad argument");
    int32_t rc = postings_check_offsets(doc_offsets, m, "doc_offsets", "document");
    if (rc) return rc;
    const u64 nd = doc_offsets[m];
    if (nd && (!term_hashes || !tfs)) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (nd > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 2^31 - 1 postings in one insert");
    for (u32 i = 1; i < m; i++)
        if (doc_ids[i] <= doc_ids[i - 1]) return cos_fail(COS_ERR_INVALID, "document ids must be strictly ascending (document %u)", i);
    for (u64 i = 0; i < nd; i++) // same rule and status as cos_bm25_create; it also keeps TOMBSTONE_TF out of the caller's hands
        if (!std::isfinite(tfs[i])) return cos_fail(COS_ERR_INVALID, "stored term frequency %llu is not finite", (unsigned long long)i);
    std::vector<u32> tmp;
    for (u32 i = 0; i < m; i++) { // term hashes distinct inside a document (process_text counts per hash: indexes/tf_idf/mod.rs:310-360)
        const u32 *h = term_hashes + doc_offsets[i];
        const size_t n = (size_t)(doc_offsets[i + 1] - doc_offsets[i]);
        bool ascending = true;
        for (size_t j = 1; j < n && ascending; j++) ascending = h[j] > h[j - 1];
        if (ascending) continue; // what cos_text_process hands out
        tmp.assign(h, h + n);
        std::sort(tmp.begin(), tmp.end());
        if (std::adjacent_find(tmp.begin(), tmp.end()) != tmp.end()) return cos_fail(COS_ERR_INVALID, "term hash repeated inside document %u", doc_ids[i]);
    }
    std::lock_guard<std::mutex> g(b->mu);
    if ((long long)doc_ids[0] <= b->max_id_ever)
        return cos_fail(COS_ERR_INVALID, "document id %u is not above the largest id the index has held (%lld)", doc_ids[0], b->max_id_ever);
    if ((u64)b->documents_count + m > 0xFFFFFFFFull) return cos_fail(COS_ERR_INVALID, "documents_count would pass 2^32 - 1");
    rc = bm25_quiesce(b);
    if (rc) return rc;
    if (nd == 0) { // documents without terms: counted, nothing to post
        b->documents_count += m;
        b->max_id_ever = doc_ids[m - 1];
        return COS_OK;
    }
    hipStream_t st = b->stream;
    const u32 n = (u32)nd;

    // 1. the delta in term-major order (uploads from host arrays are synchronous copies: an early return never leaves one in flight)
    std::vector<u32> h_pdocs(n), h_iota(n);
    u32 delta_max_doc = 0;
    for (u32 i = 0; i < m; i++) {
        for (u64 j = doc_offsets[i]; j < doc_offsets[i + 1]; j++) h_pdocs[j] = doc_ids[i];
        if (doc_offsets[i + 1] > doc_offsets[i]) delta_max_doc = doc_ids[i];
    }
    std::iota(h_iota.begin(), h_iota.end(), 0u);
    // (device allocations of the call are locals: whatever has not moved into the handle when the call leaves, by any path, is freed)
    DevArr<u32> d_keys, d_keys_sorted, d_iota, d_perm, d_pdocs, d_del_docs, d_uniq, d_counts, d_nruns;
    DevArr<float> d_ptfs, d_del_tfs;
    DevBuf d_tmp;
    HIP_TRY(d_keys.alloc(n)); HIP_TRY(d_keys_sorted.alloc(n)); HIP_TRY(d_iota.alloc(n)); HIP_TRY(d_perm.alloc(n));
    HIP_TRY(d_pdocs.alloc(n)); HIP_TRY(d_ptfs.alloc(n)); HIP_TRY(d_del_docs.alloc(n)); HIP_TRY(d_del_tfs.alloc(n));
    HIP_TRY(d_uniq.alloc(n)); HIP_TRY(d_counts.alloc(n)); HIP_TRY(d_nruns.alloc(1));
    size_t sort_bytes = 0, rle_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_keys.p, d_keys_sorted.p, d_iota.p, d_perm.p, (int)n, 0, 32, st));
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, rle_bytes, d_keys_sorted.p, d_uniq.p, d_counts.p, d_nruns.p, (int)n, st));
    size_t tmp_bytes = std::max(sort_bytes, rle_bytes);
    HIP_TRY(d_tmp.alloc(tmp_bytes));
    HIP_TRY(hipMemcpy(d_keys, term_hashes, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_iota, h_iota.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_pdocs, h_pdocs.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ptfs, tfs, (size_t)n * 4, hipMemcpyHostToDevice));
    size_t bytes = tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, bytes, d_keys.p, d_keys_sorted.p, d_iota.p, d_perm.p, (int)n, 0, 32, st)); // LSD radix sort: stable
    hipLaunchKernelGGL(bm25_delta_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_perm, d_pdocs, d_ptfs, n, d_del_docs, d_del_tfs);
    HIP_TRY(hipGetLastError());
    bytes = tmp_bytes;
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(d_tmp.p, bytes, d_keys_sorted.p, d_uniq.p, d_counts.p, d_nruns.p, (int)n, st));
    u32 U = 0;
    HIP_TRY(hipMemcpyAsync(&U, d_nruns, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (U == 0 || U > n) return cos_fail(COS_ERR_HIP, "run-length encoding of the update returned %u runs for %u postings", U, n);
    std::vector<u32> uniq(U), counts(U); // only the delta's distinct hashes and their counts come to the host
    HIP_TRY(hipMemcpyAsync(uniq.data(), d_uniq, (size_t)U * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, (size_t)U * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // 2. merge the two sorted term tables on the host: new hashes, and per new term where its old part and its delta part start
    const u32 T0 = b->n_terms;
    MergedKeys mk = postings_merge_keys(b->term_hashes, uniq);
    if (mk.keys.size() > 0xFFFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 2^32 - 1 terms");
    const u32 T = (u32)mk.keys.size();
    std::vector<u64> old_off((size_t)T + 1), del_off((size_t)T + 1), new_off((size_t)T + 1);
    {
        u32 i = 0; // the old term at or behind new slot t; a term that only the update has: an empty old part where it would stand
        u64 dpos = 0;
        for (u32 t = 0; t < T; t++) {
            old_off[t] = b->offsets[i];
            del_off[t] = dpos;
            new_off[t] = old_off[t] + dpos;
            if (mk.old_of[t] != POSTINGS_NONE) i++;
            if (mk.del_of[t] != POSTINGS_NONE) dpos += counts[mk.del_of[t]];
        }
        old_off[T] = b->offsets[T0];
        del_off[T] = dpos;
        new_off[T] = old_off[T] + dpos;
        if (dpos != n) return cos_fail(COS_ERR_HIP, "the update's run lengths add up to %llu, not %u", (unsigned long long)dpos, n);
    }
    const u64 nnz = new_off[T];

    // 3. new arrays and merge on the device; the old arrays are only read
    DevArr<u32> d_new_docs, d_new_dir;
    DevArr<float> d_new_tfs;
    DevArr<u64> d_old_off, d_del_off;
    HIP_TRY(d_new_docs.alloc(nnz)); HIP_TRY(d_new_tfs.alloc(nnz));
    HIP_TRY(d_old_off.alloc((size_t)T + 1)); HIP_TRY(d_del_off.alloc((size_t)T + 1));
    HIP_TRY(hipMemcpy(d_old_off, old_off.data(), ((size_t)T + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_del_off, del_off.data(), ((size_t)T + 1) * 8, hipMemcpyHostToDevice));
    const u64 pieces = (nnz + MERGE_PIECE - 1) / MERGE_PIECE;
    if (pieces > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "too many postings for one merge launch");
    hipLaunchKernelGGL(postings_merge_kernel<Bm25Merge>, dim3((u32)pieces), dim3(256), 0, st,
                       Bm25Merge{b->d_docs, b->d_tfs, d_del_docs, d_del_tfs, d_new_docs, d_new_tfs}, d_old_off.p, d_del_off.p, T, nnz);
    HIP_TRY(hipGetLastError());

    // 4. the new directory: a list crossing DIR_MIN gets a row, a larger largest id widens every row
    const u32 new_max_doc = std::max(b->max_doc, delta_max_doc);
    const u32 n_tiles = (u32)(((u64)new_max_doc + 1 + TILE - 1) / TILE);
    std::vector<u32> new_dir_row;
    u32 rows = 0;
    rc = postings_build_dir(Bm25Ids{d_new_docs}, new_off.data(), 1, 1, T, DIR_MIN, n_tiles, st,
                            [&](u32 t) { return cos_fail(COS_ERR_UNIMPLEMENTED, "posting list of term %u too long", mk.keys[t]); }, new_dir_row, rows, d_new_dir);
    if (rc) { (void)hipStreamSynchronize(st); return rc; } // (the merge may still be reading the handle's arrays)
    HIP_TRY(hipStreamSynchronize(st));

    // 5. everything is complete: swap, then free the old arrays.  The search workspace is reused as is.
    b->d_docs = std::move(d_new_docs); b->d_tfs = std::move(d_new_tfs); b->d_tile_dir = std::move(d_new_dir);
    b->term_hashes.swap(mk.keys);
    b->offsets.swap(new_off);
    b->dir_row.swap(new_dir_row);
    b->n_terms = T;
    b->max_doc = new_max_doc;
    b->max_id_ever = doc_ids[m - 1];
    b->documents_count += m;
    b->dir_rows = rows;
    b->dir_tiles = n_tiles;
    return COS_OK;
}

extern "C" int32_t cos_bm25_delete(cos_bm25 *b, const uint32_t *doc_ids, const uint64_t *doc_offsets, uint32_t m, const uint32_t *term_hashes) {
    if (!b) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (m == 0) return COS_OK;
    if (!doc_ids || !doc_offsets) return cos_fail(COS_ERR_INVALID, "bad argument");
    int32_t rc = postings_check_offsets(doc_offsets, m, "doc_offsets", "document");
    if (rc) return rc;
    const u64 nd = doc_offsets[m];
    if (nd && !term_hashes) return cos_fail(COS_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> g(b->mu);
    if (b->documents_count < m) return cos_fail(COS_ERR_INVALID, "delete of %u documents from an index that counts %u", m, b->documents_count);
    // term -> list on the host's term table (like bm25_prepare for queries); a term without a list is left alone (mod.rs:124-133)
    std::vector<u32> pair_doc, pair_len;
    std::vector<u64> pair_begin;
    for (u32 i = 0; i < m; i++)
        for (u64 j = doc_offsets[i]; j < doc_offsets[i + 1]; j++) {
            auto it = std::lower_bound(b->term_hashes.begin(), b->term_hashes.end(), term_hashes[j]);
            if (it == b->term_hashes.end() || *it != term_hashes[j]) continue;
            const size_t ti = (size_t)(it - b->term_hashes.begin());
            const u64 len = b->offsets[ti + 1] - b->offsets[ti];
            if (len == 0) continue;
            pair_doc.push_back(doc_ids[i]);
            pair_begin.push_back(b->offsets[ti]);
            pair_len.push_back((u32)len); // lists longer than 2^32 - 1 are refused by create and insert
        }
    if (pair_doc.size() > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 2^31 - 1 (document, term) pairs in one delete");
    const u32 np = (u32)pair_doc.size();
    rc = bm25_quiesce(b);
    if (rc) return rc;
    u32 marked = 0;
    if (np) {
        hipStream_t st = b->stream;
        DevArr<u32> d_pd, d_pl, d_marked;
        DevArr<u64> d_pb;
        HIP_TRY(d_pd.alloc(np)); HIP_TRY(d_pl.alloc(np)); HIP_TRY(d_pb.alloc(np)); HIP_TRY(d_marked.alloc(1));
        HIP_TRY(hipMemcpy(d_pd, pair_doc.data(), (size_t)np * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_pl, pair_len.data(), (size_t)np * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_pb, pair_begin.data(), (size_t)np * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(d_marked, 0, 4, st));
        // nothing of the handle has been written up to here; from the launch on the call can only fail with the device itself
        hipLaunchKernelGGL(bm25_tombstone_kernel, dim3((np + 255) / 256), dim3(256), 0, st, b->d_docs, b->d_tfs, d_pd, d_pb, d_pl, np, d_marked);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&marked, d_marked, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    b->documents_count -= m; // once per document, found or not (mod.rs:117-119)
    b->n_tombstones += marked;
    return COS_OK;
}

extern "C" int32_t cos_bm25_stats(cos_bm25 *b, cos_bm25_index_stats *out) {
    if (!b || !out || out->struct_size != sizeof(cos_bm25_index_stats)) return cos_fail(COS_ERR_INVALID, "bad argument (struct_size must be sizeof(cos_bm25_index_stats))");
    std::lock_guard<std::mutex> g(b->mu);
    const u64 nnz = b->offsets[b->n_terms];
    out->documents_count = b->documents_count;
    out->n_terms = b->n_terms;
    out->largest_doc_id = b->max_id_ever < 0 ? 0u : (u32)b->max_id_ever;
    out->dir_rows = b->dir_rows;
    out->dir_tiles = b->dir_tiles;
    out->reserved = 0;
    out->postings = nnz;
    out->tombstones = b->n_tombstones;
    u64 bytes = 2 * std::max<u64>(nnz, 1) * 4 + std::max<u64>((u64)b->dir_rows * (b->dir_tiles + 1), 1) * 4; // postings + directory
    bytes += (u64)b->capB * (sizeof(QueryTerms) + 4 + BUCKETS * 8 + 4) + 2 * (u64)b->capB * b->cap_k * 4;     // search workspace
    bytes += ((u64)b->d_hq.cap + b->d_did.cap + b->d_dsc.cap + b->d_dcnt.cap + b->d_ret.cap) * 4;                       // hybrid search buffers
    out->device_bytes = bytes;
    return COS_OK;
}

extern "C" int32_t cos_bm25_download(cos_bm25 *b, uint32_t *n_terms, uint64_t *n_postings, uint32_t *term_hashes, uint64_t *offsets, uint32_t *doc_ids,
                                     float *tfs, uint8_t *tombstones) {
    if (!b || !n_terms || !n_postings) return cos_fail(COS_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> g(b->mu);
    const u32 T = b->n_terms;
    const u64 nnz = b->offsets[T];
    const u32 cap_t = *n_terms;
    const u64 cap_p = *n_postings;
    *n_terms = T;
    *n_postings = nnz;
    if (!term_hashes && !offsets && !doc_ids && !tfs && !tombstones) return COS_OK; // first call: the sizes
    if (!term_hashes || !offsets || !doc_ids || !tfs || !tombstones) return cos_fail(COS_ERR_INVALID, "bad argument: all five arrays or none");
    if (cap_t < T || cap_p < nnz)
        return cos_fail(COS_ERR_INVALID, "arrays for %u terms / %llu postings, the index holds %u / %llu", cap_t, (unsigned long long)cap_p, T, (unsigned long long)nnz);
    int32_t rc = bm25_quiesce(b);
    if (rc) return rc;
    memcpy(term_hashes, b->term_hashes.data(), (size_t)T * 4);
    memcpy(offsets, b->offsets.data(), ((size_t)T + 1) * 8);
    HIP_TRY(hipMemcpy(doc_ids, b->d_docs, nnz * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tfs, b->d_tfs, nnz * 4, hipMemcpyDeviceToHost));
    for (u64 i = 0; i < nnz; i++) { // a tombstone leaves as a flag and a finite 0: the arrays are again what cos_bm25_create takes
        u32 bits;
        memcpy(&bits, &tfs[i], 4);
        tombstones[i] = bits == TOMBSTONE_TF;
        if (bits == TOMBSTONE_TF) tfs[i] = 0.0f;
    }
    return COS_OK;
}
