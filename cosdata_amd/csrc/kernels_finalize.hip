// kernels_finalize.hip — gfx950 kernels that end a dense search: what the walk (kernels_walk.hip) left per level becomes the answer.
//   finalize       : remove_duplicates_and_filter + finalize_ann_results
//                                                           (models/common.rs:381-412, vector_store.rs:404-445)
// Its own translation unit: none of it depends on the walk's instances, which take minutes to compile.
//
// Compile with -ffp-contract=off: the reference's arithmetic order (fused only where AVX2 FMA is
// used, x86_64.rs:418-444) is reproduced with explicit __fmaf_rn / __fmul_rn / __fadd_rn.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_types.h"
#include "exact_rerank.h"
#include "tuning.h"
#include "walk_common.h"

using namespace cosdev;

namespace {

// ------------------------------------------------------------------------------------------------
// finalize: one wave per query.
//   remove_duplicates_and_filter: first-seen dedup, drop root, sort desc by quantized score, keep 5k
//   finalize_ann_results: cs = dot_f32(q, raw) / (|q| * |raw|) in the reference order, sort desc, top k
// ------------------------------------------------------------------------------------------------
struct FinalizeArgs {
    const float *queries; // raw f32 [B][q_stride]
    u64 q_stride;
    const float *q_raw_mags; // [B] sqrt(seq sum q*q)
    const u32 *walk_ids;     // [B][L+1][100]
    const float *walk_sims;
    const u32 *walk_counts;  // [B][L+1]
    const int32_t *walk_status;
    u32 B, top_k;
    u32 *out_ids;     // [B][top_k] (id_base + local id)
    float *out_scores;
    u32 *out_counts;
    int32_t *out_status;
    u64 *out_rerank_rows; // [B]
    const u32 *q_order;   // optional [B]: workgroup -> query, the locality order the walk of this launch ended with (engine_types.h):
                          // neighbouring queries rerank many of the same raw rows
    u32 *slow_list;       // finalize_fast_kernel: [B] queries it leaves to finalize_list_kernel (more than FAST_CAP survivors) ...
    u32 *slow_count;      // ... and how many (zeroed before the launch)
};

// Small launches (one client batch: 256 workgroups on 256 CUs) rerank with NWV waves per query.  One wave streams its 5k raw rows
// (3 KB each at 768 dims) with ~8 KB in flight: ~24 dependent trips to memory for 50 rows, 60 for the 150 rows of a hybrid query's
// top_k x 3 (0.05 / 0.16 ms per batch: profiles/r06_final_kernel_trace_c5_rocprofv3.txt).  With NWV > 1 wave 0 selects the candidates
// as before, every wave then dots 8 of them per pass with the eight-lane chains of f32_oct_dot (the pair version's bits, dot_engines.h)
// and wave 0 sorts the keys the waves left in LDS: same lists, same bits.
// how many distinct nodes of a query are reranked: truncate(5 * k) (common.rs:409)
__host__ __device__ constexpr u32 rerank_cut(u32 top_k) { return 5u * top_k; }
// Sorted keys with the first of every run of equal keys flagged, `mine` of them in this lane: pos = where this lane's first one goes
// in the compacted list; returns how many of the list are candidates, the first `want`
__device__ __forceinline__ u32 kept_prefix(u32 mine, int lane, u32 want, u32 &pos) {
    u32 incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = (u32)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += t;
    }
    pos = incl - mine;
    const u32 total = readlane_u32(incl, 63);
    return total < want ? total : want;
}
// one lane's part of an answer: how many results the query has, its status, how many raw rows were reranked for them
__device__ __forceinline__ void answer_header(u32 *out_counts, int32_t *out_status, u64 *out_rerank_rows, u32 qi, int32_t status, u32 count, u32 rows) {
    out_counts[qi] = count;
    out_status[qi] = status;
    if (out_rerank_rows) out_rerank_rows[qi] = rows;
}
// one wave's LDS writes are done before any of its lanes reads them
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_wave_barrier(); }
// the exact rerank (exact_rerank.h) of candidates [0, ncand) by every wave of a wide workgroup: keys[j] = (score, id) of cand[j]
template <int NWV>
__device__ __forceinline__ void rerank_wide(const IndexDev &ix, const float *qf, const u32 *cand, u32 ncand, float mag_query, u64 *keys, int lane, int wave) {
    for (u32 base = (u32)wave * 8u; base < ncand; base += 8u * (u32)NWV) { // (wave-uniform bounds)
        const u32 my = base + (u32)(lane >> 3);
        const u32 id = my < ncand ? cand[my] : 0u;
        const u32 rrow = id / ix.id_stride; // raw embedding of an id = its base id (collection.rs:368-384)
        const float dp = f32_oct_dot(ix.raw + (u64)rrow * ix.raw_stride, qf, ix.dim, lane & 7);
        const u64 key = exact_key(dp, mag_query, ix.raw_mags[rrow], id, true);
        if ((lane & 7) == 0 && my < ncand) keys[my] = key;
    }
}

template <int FR, int NWV = 1>
__device__ __forceinline__ void finalize_one(const IndexDev &ix, const FinalizeArgs &fa, const u32 qi, unsigned char *smem_raw) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 L = ix.num_layers;
    const u32 metric = ix.metric;
    float *qf = (float *)smem_raw;                                   // dim floats (padded to 16 B)
    u32 *cand = (u32 *)(smem_raw + staged_query_bytes(ix.dim)); // 64*FR candidate ids
    u64 *wkeys = (u64 *)(cand + 64 * FR);                            // NWV > 1: 64*FR reranked keys, then [0] of the word behind them = ncand
    u32 *wmisc = (u32 *)(wkeys + 64 * FR);

    const int32_t wst = fa.walk_status[qi];
    if (wst != COS_OK) {
        if (tid == 0) answer_header(fa.out_counts, fa.out_status, fa.out_rerank_rows, qi, wst, 0u, 0u);
        return;
    }
    const float *q = fa.queries + (u64)qi * fa.q_stride;
    for (u32 i = tid; i < ix.dim; i += 64 * NWV) qf[i] = q[i];
    const float mag_query = fa.q_raw_mags[qi];
    if constexpr (NWV > 1) {
        if (wave != 0) { // the other waves wait for the candidates, rerank their share and are done
            __syncthreads();
            rerank_wide<NWV>(ix, qf, cand, wmisc[0], mag_query, wkeys, lane, wave);
            __syncthreads();
            return;
        }
    }

    // gather the concatenated per-level lists (top level first) as (key, id) pairs
    u64 k[FR];
#pragma unroll
    for (int r = 0; r < FR; r++) k[r] = 0ull;
    {
        u32 off = 0;
        for (u32 s = 0; s <= L; s++) {
            // a level list is sorted: entries past its first 5k+1 cannot reach the global top 5k (each is preceded by 5k
            // distinct better non-root nodes — one of the first 5k+1 may be the root, which is filtered), so only
            // min(count, 5k+1) entries per level take part in the sort.  Not so in a metadata collection: the pseudo nodes are
            // filtered as well, a list may hold any number of them ahead of its replicas (one per matching filter at cosine 1.0;
            // under the other metrics every pseudo node scores like the all-zero vector), and the whole list takes part
            // (launch_finalize sizes FR for it)
            u32 c = fa.walk_counts[(u64)qi * (L + 1) + s];
            if (ix.mdim == 0u && c > rerank_cut(fa.top_k) + 1u) c = rerank_cut(fa.top_k) + 1u;
            const u64 b = ((u64)qi * (L + 1) + s) * KEEP_SEARCH;
            // element index off + j  lives in lane (off+j)/FR, register (off+j)%FR
#pragma unroll
            for (int r = 0; r < FR; r++) {
                const u32 e = (u32)lane * FR + r;
                if (e >= off && e < off + c) {
                    const u32 j = e - off;
                    const u32 id = fa.walk_ids[b + j];
                    const float sv = fa.walk_sims[b + j];
                    // root filtered (common.rs:397); so are the pseudo nodes of a metadata collection (common.rs:400-402)
                    const bool drop = id == COS_ROOT_ID || (ix.mdim != 0u && id >= PSEUDO_LO && id <= PSEUDO_HI);
                    k[r] = drop ? 0ull : pack_key(metric_key(metric, sv), id);
                }
            }
            off += c;
        }
    }
    bitonic_sort_desc<FR>(k, lane);
    // duplicates of a node carry identical (score, id) keys and are adjacent after the sort: keep the first
    const u64 prev_last = shfl_up1_u64(k[FR - 1]);
    u32 keepbits = 0;
#pragma unroll
    for (int r = 0; r < FR; r++) {
        const u64 prev = (r == 0) ? (lane == 0 ? ~0ull : prev_last) : k[r > 0 ? r - 1 : 0];
        if (k[r] != 0ull && k[r] != prev) keepbits |= 1u << r;
    }
    u32 pos; // exclusive prefix of kept counts across lanes
    const u32 ncand = kept_prefix((u32)__popc(keepbits), lane, rerank_cut(fa.top_k), pos);
#pragma unroll
    for (int r = 0; r < FR; r++) {
        if (keepbits & (1u << r)) {
            if (pos < ncand) cand[pos] = (u32)k[r];
            pos++;
        }
    }
    const u32 nout = ncand < fa.top_k ? ncand : fa.top_k;
    if constexpr (NWV > 1) {
        if (lane == 0) wmisc[0] = ncand;
        __syncthreads();
        rerank_wide<NWV>(ix, qf, cand, ncand, mag_query, wkeys, lane, 0);
        __syncthreads();
        u64 rk[FR];
#pragma unroll
        for (int r = 0; r < FR; r++) {
            const u32 e = (u32)lane * FR + r;
            rk[r] = e < ncand ? wkeys[e] : 0ull;
        }
        bitonic_sort_desc<FR>(rk, lane);
#pragma unroll
        for (int r = 0; r < FR; r++) {
            const u32 e = (u32)lane * FR + r;
            if (e < nout) {
                fa.out_ids[(u64)qi * fa.top_k + e] = (u32)rk[r] + ix.id_base;
                fa.out_scores[(u64)qi * fa.top_k + e] = simkey_inv((u32)(rk[r] >> 32));
            }
        }
        if (lane == 0) answer_header(fa.out_counts, fa.out_status, fa.out_rerank_rows, qi, COS_OK, nout, ncand);
        return;
    }
    wave_sync();

    // exact rerank on raw f32 (vector_store.rs:404-445); 32 candidates per pass (one lane pair each)
    const int pair = lane >> 1;
    if (ncand <= 64) {
        // common case (5k <= 64): survivor j ends in lane j and one 64-key sort finishes the job
        u64 res[1] = {0ull};
        for (u32 base = 0; base < ncand; base += 32) {
            const u32 my = base + (u32)pair;
            const u32 id = my < ncand ? cand[my] : 0u;
            const u32 rrow = id / ix.id_stride; // raw embedding of an id = its base id (collection.rs:368-384)
            const float dp = f32_pair_dot(ix.raw + (u64)rrow * ix.raw_stride, qf, ix.dim, lane & 1);
            pair_keys_to_lanes(exact_key(dp, mag_query, ix.raw_mags[rrow], id, my < ncand), base, lane, res[0]);
        }
        bitonic_sort_desc<1>(res, lane);
        if ((u32)lane < nout) {
            fa.out_ids[(u64)qi * fa.top_k + lane] = (u32)res[0] + ix.id_base;
            fa.out_scores[(u64)qi * fa.top_k + lane] = simkey_inv((u32)(res[0] >> 32));
        }
    } else {
        u64 rk[FR];
#pragma unroll
        for (int r = 0; r < FR; r++) rk[r] = 0ull;
        for (u32 base = 0; base < ncand; base += 32) {
            const u32 my = base + (u32)pair;
            const u32 id = my < ncand ? cand[my] : 0u;
            const u32 rrow = id / ix.id_stride;
            const float dp = f32_pair_dot(ix.raw + (u64)rrow * ix.raw_stride, qf, ix.dim, lane & 1);
            const u64 key = exact_key(dp, mag_query, ix.raw_mags[rrow], id, true);
            // scatter into the blocked register layout: element my -> lane my/FR, reg my%FR
            for (u32 j = 0; j < 32 && base + j < ncand; j++) {
                const u64 kv = readlane_u64(key, (int)(2 * j));
                const u32 e = base + j;
                if ((u32)lane == e / FR) {
#pragma unroll
                    for (int r = 0; r < FR; r++)
                        if ((e % FR) == (u32)r) rk[r] = kv;
                }
            }
        }
        bitonic_sort_desc<FR>(rk, lane);
#pragma unroll
        for (int r = 0; r < FR; r++) {
            const u32 e = (u32)lane * FR + r;
            if (e < nout) {
                fa.out_ids[(u64)qi * fa.top_k + e] = (u32)rk[r] + ix.id_base;
                fa.out_scores[(u64)qi * fa.top_k + e] = simkey_inv((u32)(rk[r] >> 32));
            }
        }
    }
    if (lane == 0) answer_header(fa.out_counts, fa.out_status, fa.out_rerank_rows, qi, COS_OK, nout, ncand);
}

// grid = B: one wave per query (q_order: the launch's locality order)
template <int FR>
__global__ __launch_bounds__(64) void finalize_kernel(const IndexDev ix, const FinalizeArgs fa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    if (blockIdx.x >= fa.B) return;
    finalize_one<FR>(ix, fa, fa.q_order ? fa.q_order[blockIdx.x] : blockIdx.x, smem_raw);
}
template <int FR, int NWV>
__global__ __launch_bounds__(64 * NWV) void finalize_wide_kernel(const IndexDev ix, const FinalizeArgs fa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    if (blockIdx.x >= fa.B) return;
    finalize_one<FR, NWV>(ix, fa, fa.q_order ? fa.q_order[blockIdx.x] : blockIdx.x, smem_raw);
}
// the queries finalize_fast_kernel left over (slow_list / slow_count): a small fixed grid walks the list — nothing to do costs a
// launch of a few workgroups instead of B that look at a flag and leave (60 us per 32768-query launch)
template <int FR>
__global__ __launch_bounds__(64) void finalize_list_kernel(const IndexDev ix, const FinalizeArgs fa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const u32 n = *fa.slow_count;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        finalize_one<FR>(ix, fa, fa.slow_list[i], smem_raw);
        wave_sync(); // the next query rewrites the LDS buffers
    }
}

// ------------------------------------------------------------------------------------------------
// finalize_fast: the same result for the usual shape of a search (5 * top_k <= 64), at a fraction of the work.
// finalize_kernel sorts the first 5k + 1 entries of EVERY level list — 510 keys at ten levels, a 512-key bitonic network in 121
// VGPRs (4 waves per SIMD) — to keep the best 5k distinct ones.  But level 0's own list already holds 5k + 1 distinct nodes (at most
// one of them the root): an entry of any list below level 0's (5k + 1)-th key has 5k distinct non-root entries above it and can never
// be kept.  So: T = that key; the entries >= T of all lists — level 0's 5k + 1 and the few upper-level entries that are among the
// query's nearest (the same nodes at the same scores: duplicates) — are compacted into LDS, typically ~70 of them; up to 128 are sorted
// by a 128-key network (two keys per lane), deduplicated and reranked exactly as below.  More than 128 survivors (small graphs, tiny
// ef: level 0 has no (5k + 1)-th entry and nothing is screened) leave the query to finalize_list_kernel through slow_list.
// ------------------------------------------------------------------------------------------------
constexpr int FAST_CAP = 128;
template <int NWV>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(NWV == 1 ? 7 : 2, 8))) void finalize_fast_kernel(const IndexDev ix, const FinalizeArgs fa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (blockIdx.x >= fa.B) return;
    const u32 qi = fa.q_order ? fa.q_order[blockIdx.x] : blockIdx.x;
    const u32 L = ix.num_layers;
    const u32 metric = ix.metric;
    float *qf = (float *)smem_raw;                                                       // dim floats (padded to 16 B)
    u64 *surv = (u64 *)(smem_raw + staged_query_bytes(ix.dim));           // FAST_CAP survivor keys
    u32 *cand = (u32 *)(surv + FAST_CAP);                                                // 64 candidate ids, then one word: ncand (NWV > 1)

    const int32_t wst = fa.walk_status[qi];
    if (wst != COS_OK) {
        if (tid == 0) answer_header(fa.out_counts, fa.out_status, fa.out_rerank_rows, qi, wst, 0u, 0u);
        return;
    }
    const float *q = fa.queries + (u64)qi * fa.q_stride;
    for (u32 i = tid; i < ix.dim; i += 64 * NWV) qf[i] = q[i];
    const float mag_query = fa.q_raw_mags[qi];
    if constexpr (NWV > 1) { // (finalize_one: the other waves wait for the candidates and rerank their share; keys land where the survivors were)
        if (wave != 0) {
            __syncthreads();
            const u32 nc = cand[64];
            if (nc != 0xFFFFFFFFu) rerank_wide<NWV>(ix, qf, cand, nc, mag_query, surv, lane, wave);
            __syncthreads();
            return;
        }
    }

    const u32 want = rerank_cut(fa.top_k), per = want + 1u; // entries of a level that can matter
    // counts of every level in one load; the threshold from level 0's list (slot L)
    const u32 cnt_l = (u32)lane <= L ? fa.walk_counts[(u64)qi * (L + 1) + lane] : 0u;
    const u32 c0 = readlane_u32(cnt_l, (int)L);
    const u64 b0 = ((u64)qi * (L + 1) + L) * KEEP_SEARCH;
    u64 T = 0ull;
    if (c0 >= per) T = pack_key(metric_key(metric, uniform_f32(fa.walk_sims[b0 + want])), uniform_u32(fa.walk_ids[b0 + want]));
    // every level's first min(count, 5k + 1) entries, one per lane (5k + 1 <= 64): loads of all levels first, then the screen
    u32 n = 0;
    bool overflow = false;
    for (u32 s0 = 0; s0 <= L; s0 += 4) { // four levels' loads in flight
        u32 idv[4];
        float smv[4];
        u32 cc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const u32 s = s0 + (u32)u;
            u32 c = s <= L ? readlane_u32(cnt_l, (int)(s <= L ? s : L)) : 0u;
            c = c > per ? per : c;
            cc[u] = c;
            const u64 b = ((u64)qi * (L + 1) + (s <= L ? s : L)) * KEEP_SEARCH;
            const u32 j = (u32)lane < c ? (u32)lane : 0u;
            idv[u] = fa.walk_ids[b + j];
            smv[u] = fa.walk_sims[b + j];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const u32 id = idv[u];
            // root filtered (common.rs:397); so are the pseudo nodes of a metadata collection (common.rs:400-402)
            const bool drop = id == COS_ROOT_ID || (ix.mdim != 0u && id >= PSEUDO_LO && id <= PSEUDO_HI);
            const u64 key = pack_key(metric_key(metric, smv[u]), id);
            const u64 keep = ballot64((u32)lane < cc[u] && !drop && key >= T);
            const u32 nk = (u32)__popcll(keep);
            if (n + nk > (u32)FAST_CAP) { overflow = true; break; }
            if (__builtin_amdgcn_inverse_ballot_w64(keep)) surv[n + (u32)__popcll(keep & ((1ull << lane) - 1ull))] = key;
            n += nk;
        }
        if (overflow) break;
    }
    if (overflow) {
        if (lane == 0) fa.slow_list[atomicAdd(fa.slow_count, 1u)] = qi;
        if constexpr (NWV > 1) {
            if (lane == 0) cand[64] = 0xFFFFFFFFu;
            __syncthreads();
            __syncthreads();
        }
        return;
    }
    wave_sync();
    u64 k[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const u32 e = (u32)lane * 2u + (u32)r;
        k[r] = e < n ? surv[e] : 0ull;
    }
    bitonic_sort_desc<2>(k, lane);
    // duplicates of a node carry identical (score, id) keys and are adjacent after the sort: keep the first
    const u64 prev_last = shfl_up1_u64(k[1]);
    const bool keep0 = k[0] != 0ull && (lane == 0 || k[0] != prev_last), keep1 = k[1] != 0ull && k[1] != k[0];
    u32 pos;
    const u32 ncand = kept_prefix((keep0 ? 1u : 0u) + (keep1 ? 1u : 0u), lane, want, pos);
    if (keep0) { if (pos < ncand) cand[pos] = (u32)k[0]; pos++; }
    if (keep1) { if (pos < ncand) cand[pos] = (u32)k[1]; }
    const u32 nout = ncand < fa.top_k ? ncand : fa.top_k;
    u64 res[1] = {0ull};
    if constexpr (NWV > 1) {
        if (lane == 0) cand[64] = ncand;
        __syncthreads(); // (the survivors were read into registers before the sort: their LDS takes the reranked keys)
        rerank_wide<NWV>(ix, qf, cand, ncand, mag_query, surv, lane, 0);
        __syncthreads();
        res[0] = (u32)lane < ncand ? surv[lane] : 0ull;
    } else {
    wave_sync();

    // exact rerank on raw f32 (vector_store.rs:404-445); 32 candidates per pass (one lane pair each); survivor j ends in lane j and
    // one 64-key sort finishes the job (5k <= 64)
    const int pair = lane >> 1;
    for (u32 base = 0; base < ncand; base += 32) {
        const u32 my = base + (u32)pair;
        const u32 id = my < ncand ? cand[my] : 0u;
        const u32 rrow = id / ix.id_stride; // raw embedding of an id = its base id (collection.rs:368-384)
        const float dp = f32_pair_dot(ix.raw + (u64)rrow * ix.raw_stride, qf, ix.dim, lane & 1);
        pair_keys_to_lanes(exact_key(dp, mag_query, ix.raw_mags[rrow], id, my < ncand), base, lane, res[0]);
    }
    }
    bitonic_sort_desc<1>(res, lane);
    write_topk<1, false>(res, nout, fa.top_k, qi, ix.id_base, fa.out_ids, fa.out_scores, lane);
    if (lane == 0) answer_header(fa.out_counts, fa.out_status, fa.out_rerank_rows, qi, COS_OK, nout, ncand);
}

} // namespace

namespace cosdev {

hipError_t launch_finalize(const IndexDev &ix, const float *queries, u64 q_stride, const float *q_raw_mags, const u32 *walk_ids,
                           const float *walk_sims, const u32 *walk_counts, const int32_t *walk_status, u32 B, u32 top_k,
                           u32 *out_ids, float *out_scores, u32 *out_counts, int32_t *out_status, u64 *out_rerank_rows,
                           hipStream_t st, const u32 *q_order, u32 *slow_list /* [B + 1] scratch: count, then the list */) {
    if (B == 0) return hipSuccess;
    FinalizeArgs fa{queries, q_stride, q_raw_mags, walk_ids, walk_sims, walk_counts, walk_status, B, top_k,
                    out_ids, out_scores, out_counts, out_status, out_rerank_rows, q_order, nullptr, nullptr};
    // (metadata collections: whole lists, see finalize_one — 16 levels x 100 entries still fit the widest instance)
    const u32 per_level = ix.mdim != 0u ? (u32)KEEP_SEARCH : std::min<u32>(KEEP_SEARCH, rerank_cut(top_k) + 1u);
    const u32 total = (ix.num_layers + 1) * per_level;
    dim3 grid(B), block(64);
    // small launches: FIN_WAVES waves per query (finalize_one); tuning knob finalize_wide_max_b = the largest such launch (0 = never)
    constexpr int FIN_WAVES = 8;
    const bool wide = B <= (u32)std::max<long long>(0, tune_or(TUNE_FINALIZE_WIDE_MAX_B, 1024));
    // the screened kernel first (5k + 1 <= 64 entries per level list), then the general kernel over the list of queries it left;
    // tuning knob finalize_fast = 0 keeps the general kernel alone (experiments)
    const bool fast_on = tune_or(TUNE_FINALIZE_FAST, 1) != 0;
    bool listed = false;
    if (fast_on && slow_list && ix.mdim == 0u && rerank_cut(top_k) + 1u <= 64u && KEEP_SEARCH >= rerank_cut(top_k) + 1u) { // base collections: only the root is ever dropped
        fa.slow_list = slow_list + 1;
        fa.slow_count = slow_list;
        hipError_t e = hipMemsetAsync(slow_list, 0, 4, st);
        if (e != hipSuccess) return e;
        const size_t smem_f = staged_query_bytes(ix.dim) + (size_t)FAST_CAP * 8 + 64 * 4 + 16;
        if (wide) hipLaunchKernelGGL(finalize_fast_kernel<FIN_WAVES>, grid, dim3(64 * FIN_WAVES), smem_f, st, ix, fa);
        else hipLaunchKernelGGL(finalize_fast_kernel<1>, grid, block, smem_f, st, ix, fa);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        listed = true;
        grid = dim3(std::min<u32>(B, 2048u));
    }
#define FIN(FR_)                                                                                                   \
    do {                                                                                                           \
        const size_t smem = staged_query_bytes(ix.dim) + 64 * (FR_) * 4;                            \
        if (listed) hipLaunchKernelGGL(finalize_list_kernel<FR_>, grid, block, smem, st, ix, fa);                 \
        else if (wide) hipLaunchKernelGGL((finalize_wide_kernel<FR_, FIN_WAVES>), grid, dim3(64 * FIN_WAVES), smem + 64 * (FR_) * 8 + 16, st, ix, fa); \
        else hipLaunchKernelGGL(finalize_kernel<FR_>, grid, block, smem, st, ix, fa);                             \
    } while (0)
    if (total <= 64 * 4) FIN(4);
    else if (total <= 64 * 8) FIN(8);
    else if (total <= 64 * 16) FIN(16);
    else if (total <= 64 * 32) FIN(32);
    else return hipErrorInvalidValue;
#undef FIN
    return hipGetLastError();
}

} // namespace cosdev
