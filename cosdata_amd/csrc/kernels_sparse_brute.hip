// kernels_sparse_brute.hip — cos_sparse_bruteforce_topk: the exact top k of a learned-sparse query over the RAW rows of the handle
// (DESIGN.md §4.9.1).  The score is finalize_sparse_ann_results' (sparse_raw_dot, sparse_brute.h): dp over the query's pairs in the order
// given, one f32 multiply and one f32 add per shared dimension; a row is a candidate when it is live and shares a dimension; the order
// is that of pack_key(simkey(dp), id), the rerank's.  No posting list is read: the scan streams the raw CSR once per block of queries.
//
// Fast path (sparse_brute_scan_kernel<R>): queries whose dimensions strictly ascend, on rows whose dimensions strictly ascend.  A
// workgroup of 16 waves owns 16 queries (one per wave, its Pool<R> in registers, its dim -> value table in LDS) and the rows that
// START inside one span of the nonzeros, so workgroups are balanced by nonzeros whatever the rows' lengths.  The span goes through
// a 64 KB LDS buffer in tiles of up to 8188 nonzeros and 1024 rows, double-buffered in registers: two 16-byte loads of dims and of
// vals per thread, issued before the current tile is probed and stored to LDS behind it.  (A second LDS buffer would buy nothing: the
// next tile's bounds are only known behind the barrier that frees the first.)  A lane walks one row of the tile out of LDS and probes the table per nonzero: both
// sides ascend, so the hits arrive in query order and the running fadd(dp, fmul(x, qv)) has the rule's bits.  A row cut by a tile
// boundary carries (dp, hit) to the next tile through LDS; a row part of 128 nonzeros or more is probed by the whole wave, 64
// nonzeros at a time, and its hits are added in lane order.
// Slow path (sparse_brute_slow_kernel<R>): any other query — unsorted or repeated dimensions, more pairs than the table holds, a
// handle whose rows do not ascend.  One lane per row calls sparse_raw_dot: order-preserving by construction.
// Both leave one sorted segment of 64 R keys per (query, chunk); sparse_brute_finish_kernel<R> folds a query's segments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sparse_brute.h"
#include "topk_select.h"

using namespace cosdev;

namespace {

constexpr u32 SB_QB = 16;              // queries (= waves) per workgroup of the fast scan
constexpr u32 SB_THREADS = SB_QB * 64; // 1024
constexpr u32 SB_TAB = 256;            // table slots per query: a power of two >= 2 * SB_MAX_PAIRS
constexpr u32 SB_MAX_PAIRS = 128;      // pairs of a fast-path query
constexpr u32 SB_LOADS = 2;           // 16-byte loads of dims, and of vals, per thread and tile
constexpr u32 SB_BUF = 4 * SB_LOADS * SB_THREADS; // nonzeros of the LDS buffer
constexpr u32 SB_TILE = SB_BUF - 4;    // nonzeros of a tile: the buffer starts at the 16-byte boundary under the tile's first one
constexpr u32 SB_ROWS = SB_THREADS;    // rows of a tile: one thread prepares one row's bounds
constexpr u32 SB_LONG = 128;           // a row part this long is probed by the whole wave
constexpr u32 SB_EMPTY = 0xFFFFFFFFu;  // empty table slot (a query naming this dimension takes the slow path)
constexpr u32 SB_MAX_CHUNKS = 64;
static_assert(SB_TILE + 3 < SB_BUF, "a row part ends inside the buffer, and the nonzero behind it is still inside");
static_assert(SB_TAB >= 2 * SB_MAX_PAIRS && (SB_TAB & (SB_TAB - 1)) == 0, "open addressing at load <= 1/2");

struct SbQueries { // device pointers into the call's one image
    const u32 *dims;
    const float *vals;
    const u32 *off;  // [B + 1]
    const u32 *list; // [B]: the fast queries, then the slow ones
};

__device__ __forceinline__ u32 sb_hash(u32 d) { return (d * 2654435761u) >> 24; }
static_assert(SB_TAB == 256, "sb_hash keeps 8 bits");

// first row r in [lo, hi] with row_off[r] >= x (hi when there is none)
__device__ __forceinline__ u32 sb_lower_row(const u64 *__restrict__ row_off, u32 lo, u32 hi, u64 x) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2;
        if (row_off[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool sb_dead(const u32 *__restrict__ dead, u32 v) { return (dead[v >> 5] >> (v & 31u)) & 1u; }

// a wave's pool is a sorted segment already: position e = lane * R + r
template <int R>
__device__ __forceinline__ void sb_write_segment(const Pool<R> &pool, u64 *__restrict__ out, int lane) {
#pragma unroll
    for (int r = 0; r < R; r++) out[(u32)lane * R + r] = pool.e[r];
}

struct SbTileMeta { // written by the threads that find them, read by all behind a barrier
    u64 t1;        // the tile's end in the nonzeros
    u32 nrows;     // rows with a part (possibly empty) in the tile
    u32 cont_in;   // the first row began in an earlier tile
    u32 cont_out;  // the last row goes on in the next tile
};

template <int R>
__global__ __launch_bounds__(SB_THREADS) void sparse_brute_scan_kernel(const SparseBruteIndex ix, const SbQueries qs, u32 n_fast, u32 chunks, u64 span,
                                                                        u64 *__restrict__ part) {
    __shared__ u32 tab_dim[SB_QB][SB_TAB];
    __shared__ float tab_val[SB_QB][SB_TAB];
    __shared__ __attribute__((aligned(16))) u32 buf_d[SB_BUF];
    __shared__ __attribute__((aligned(16))) float buf_v[SB_BUF];
    __shared__ u32 s_lo[SB_ROWS], s_hi[SB_ROWS]; // a row's part of the tile, relative to the buffer's first nonzero
    __shared__ SbTileMeta meta;
    __shared__ float carry_dp[SB_QB];
    __shared__ u32 carry_hit[SB_QB];

    const u32 tid = threadIdx.x;
    const int lane = (int)(tid & 63u), wave = (int)(tid >> 6);
    const u32 chunk = blockIdx.x, qi = blockIdx.y * SB_QB + (u32)wave;
    const bool has_q = qi < n_fast;
    const u32 q = has_q ? qs.list[qi] : 0u;

    // the wave's table: every lane inserts its pairs (distinct dimensions: a slot is claimed once)
    for (u32 i = (u32)lane; i < SB_TAB; i += 64u) tab_dim[wave][i] = SB_EMPTY;
    __syncthreads();
    if (has_q) {
        const u32 b = qs.off[q], e = qs.off[q + 1];
        for (u32 i = b + (u32)lane; i < e; i += 64u) {
            const u32 d = qs.dims[i];
            u32 h = sb_hash(d);
            while (atomicCAS(&tab_dim[wave][h], SB_EMPTY, d) != SB_EMPTY) h = (h + 1u) & (SB_TAB - 1u);
            tab_val[wave][h] = qs.vals[i];
        }
    }

    // rows [r_first, r_end) start inside [chunk * span, (chunk + 1) * span); their nonzeros are [E0, E)
    const u64 s0 = (u64)chunk * span;
    const u32 r_first = sb_lower_row(ix.row_off, 0u, ix.n, s0), r_end = sb_lower_row(ix.row_off, r_first, ix.n, s0 + span);
    const u64 E = ix.row_off[r_end];

    Pool<R> pool;
    pool.clear();
    u64 thr = 0ull;

    // tile state, block-uniform: first row and first nonzero of the tile being prepared
    u32 ra = r_first;
    u64 t0 = r_first < r_end ? ix.row_off[r_first] : E;

    // thread tid prepares row ra + tid of the tile at (ra, t0): its part of the tile, and the tile's end
    auto prepare = [&](u32 ra_, u64 t0_) {
        const u64 tcap = t0_ + SB_TILE < E ? t0_ + SB_TILE : E;
        const u64 a0 = t0_ & ~3ull;
        const u32 r = ra_ + tid;
        if (r < r_end) {
            const u64 o0 = ix.row_off[r], o1 = ix.row_off[r + 1];
            if (o0 < tcap) { // the row has a part here (rows ascend: a prefix of the threads)
                const u64 lo = o0 > t0_ ? o0 : t0_, hi = o1 < tcap ? o1 : tcap;
                s_lo[tid] = (u32)(lo - a0);
                s_hi[tid] = (u32)(hi - a0);
                const bool next_in = tid + 1u < SB_ROWS && r + 1u < r_end && o1 < tcap;
                if (!next_in) { // the tile's last row
                    meta.nrows = tid + 1u;
                    meta.t1 = hi; // SB_ROWS rows that end before the cap end the tile early
                    meta.cont_out = o1 > tcap ? 1u : 0u;
                }
                if (tid == 0u) meta.cont_in = o0 < t0_ ? 1u : 0u;
            }
        }
    };
    // SB_LOADS coalesced 16-byte loads of dims and of vals per thread, kept in registers while the tile before is probed: the buffer
    // then holds nonzeros [a0, a0 + SB_BUF), those past the arrays' end as zeros
    uint4 ld[SB_LOADS];
    float4 lv[SB_LOADS];
    auto load_tile = [&](u64 t0_) {
#pragma unroll
        for (u32 c = 0; c < SB_LOADS; c++) {
            const u64 i = (t0_ & ~3ull) + 4ull * (tid + c * SB_THREADS);
            if (i + 4ull <= ix.nnz) {
                ld[c] = *reinterpret_cast<const uint4 *>(ix.raw_dims + i);
                lv[c] = *reinterpret_cast<const float4 *>(ix.raw_vals + i);
            } else {
                u32 d[4] = {0u, 0u, 0u, 0u};
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (i + (u64)j < ix.nnz) { d[j] = ix.raw_dims[i + j]; v[j] = ix.raw_vals[i + j]; }
                ld[c] = make_uint4(d[0], d[1], d[2], d[3]);
                lv[c] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (u32 c = 0; c < SB_LOADS; c++) {
            reinterpret_cast<uint4 *>(buf_d)[tid + c * SB_THREADS] = ld[c];
            reinterpret_cast<float4 *>(buf_v)[tid + c * SB_THREADS] = lv[c];
        }
    };

    // one nonzero of the wave's query: the slot of dimension d, or none
    auto probe = [&](u32 d, float &qv) -> bool {
        u32 h = sb_hash(d);
        for (;;) {
            const u32 e = tab_dim[wave][h];
            if (e == d) { qv = tab_val[wave][h]; return true; }
            if (e == SB_EMPTY) return false;
            h = (h + 1u) & (SB_TAB - 1u);
        }
    };

    bool live = t0 < E; // (rows behind E are empty: no candidates)
    if (live) {
        load_tile(t0);
        prepare(ra, t0);
        store_tile();
    }
    __syncthreads();
    while (live) { // block-uniform
        const u32 nrows = meta.nrows, cont_in = meta.cont_in, cont_out = meta.cont_out;
        const u64 t1 = meta.t1;
        const u32 ra_next = ra + nrows - cont_out;
        const bool more = t1 < E && ra_next < r_end;
        if (more) load_tile(t1); // in flight under the probes below
        if (has_q) {
            const u32 *bd = buf_d;
            const float *bv = buf_v;
            for (u32 j = 0; j < nrows; j += 64u) {
                const u32 i = j + (u32)lane;
                const bool mine = i < nrows;
                const u32 lo = mine ? s_lo[i] : 0u, hi = mine ? s_hi[i] : 0u;
                float dp = 0.0f;
                u32 hit = 0u;
                if (i == 0u && cont_in) { dp = carry_dp[wave]; hit = carry_hit[wave]; }
                const bool is_long = hi - lo >= SB_LONG;
                if (!is_long && lo < hi) {
                    // Most nonzeros meet an empty slot (a query fills a tenth of its table): that path is straight-line, the next
                    // nonzero's dimension is already on its way from LDS, and only an occupied slot enters the probe loop.
                    u32 d = bd[lo];
                    for (u32 p = lo; p < hi; p++) {
                        const u32 dn = bd[p + 1u]; // at most one behind the part: hi < SB_BUF
                        u32 h = sb_hash(d);
                        u32 e = tab_dim[wave][h];
                        if (e != SB_EMPTY) {
                            while (e != d && e != SB_EMPTY) {
                                h = (h + 1u) & (SB_TAB - 1u);
                                e = tab_dim[wave][h];
                            }
                            if (e == d) { dp = __fadd_rn(dp, __fmul_rn(bv[p], tab_val[wave][h])); hit = 1u; }
                        }
                        d = dn;
                    }
                }
                // long parts, one after the other by the whole wave: lane order is nonzero order, so the adds keep the rule's order
                for (u64 m = ballot64(is_long); m; m &= m - 1ull) {
                    const int l = __ffsll((long long)m) - 1;
                    const u32 llo = readlane_u32(lo, l), lhi = readlane_u32(hi, l);
                    float ldp = __uint_as_float(readlane_u32(__float_as_uint(dp), l));
                    u32 lhit = readlane_u32(hit, l);
                    for (u32 p0 = llo; p0 < lhi; p0 += 64u) {
                        const u32 p = p0 + (u32)lane;
                        float qv = 0.0f, prod = 0.0f;
                        bool h = false;
                        if (p < lhi) h = probe(bd[p], qv);
                        if (h) prod = __fmul_rn(bv[p], qv);
                        for (u64 hm = ballot64(h); hm; hm &= hm - 1ull) {
                            ldp = __fadd_rn(ldp, __uint_as_float(readlane_u32(__float_as_uint(prod), __ffsll((long long)hm) - 1)));
                            lhit = 1u;
                        }
                    }
                    if (lane == l) { dp = ldp; hit = lhit; }
                }
                u64 key = 0ull;
                if (mine) {
                    if (i == nrows - 1u && cont_out) { // the row goes on: its sum so far waits for the next tile
                        carry_dp[wave] = dp;
                        carry_hit[wave] = hit;
                    } else if (hit && !sb_dead(ix.dead, ra + i))
                        key = pack_key(simkey(dp), ra + i);
                }
                pool_fold_lanes<R>(pool, thr, key, lane);
            }
        }
        __syncthreads(); // everybody is done with the tile: its bounds and the buffer are free
        ra = ra_next;
        t0 = t1;
        live = more;
        if (live) {
            prepare(ra, t0);
            store_tile();
        }
        __syncthreads();
    }
    if (has_q) sb_write_segment<R>(pool, part + ((u64)q * chunks + chunk) * (64u * R), lane);
}

// one wave per (chunk of rows, slow query): a lane scores a row by the shared rule
template <int R>
__global__ __launch_bounds__(64) void sparse_brute_slow_kernel(const SparseBruteIndex ix, const SbQueries qs, u32 n_fast, u32 chunks, u64 *__restrict__ part) {
    const int lane = (int)threadIdx.x;
    const u32 chunk = blockIdx.x, q = qs.list[n_fast + blockIdx.y];
    const u32 r0 = (u32)((u64)ix.n * chunk / chunks), r1 = (u32)((u64)ix.n * (chunk + 1u) / chunks);
    const u32 qb = qs.off[q], qe = qs.off[q + 1];
    Pool<R> pool;
    pool.clear();
    u64 thr = 0ull;
    for (u32 base = r0; base < r1; base += 64u) {
        const u32 v = base + (u32)lane;
        u64 key = 0ull;
        if (v < r1 && !sb_dead(ix.dead, v)) {
            // candidacy: some query dimension is in the row (the rule's own lookups, without the arithmetic)
            const u64 b = ix.row_off[v], e = ix.row_off[v + 1];
            bool shares = false;
            for (u32 i = qb; i < qe && !shares; i++) {
                const u32 d = qs.dims[i];
                u64 lo = b, hi = e;
                while (lo < hi) { const u64 mid = lo + (hi - lo) / 2; if (ix.raw_dims[mid] < d) lo = mid + 1; else hi = mid; }
                shares = lo < e && ix.raw_dims[lo] == d;
            }
            if (shares) key = pack_key(simkey(sparse_raw_dot(ix.row_off, ix.raw_dims, ix.raw_vals, v, qs.dims, qs.vals, qs.off, q)), v);
        }
        pool_fold_lanes<R>(pool, thr, key, lane);
    }
    sb_write_segment<R>(pool, part + ((u64)q * chunks + chunk) * (64u * R), lane);
}

// one workgroup per query: the best 64 R keys of its `chunks` sorted segments (fold_reversed + lds_bitonic_merge_desc, a segment
// whose best key misses the cut is skipped), the first k of them written.  Slots behind the count are not written.
template <int R>
__global__ __launch_bounds__(256) void sparse_brute_finish_kernel(const u64 *__restrict__ part, u32 chunks, u32 k, u32 *__restrict__ out_ids,
                                                                  float *__restrict__ out_scores, u32 *__restrict__ out_counts) {
    constexpr u32 N = 64u * R;
    __shared__ u64 best[N];
    __shared__ u32 s_count;
    const u32 q = blockIdx.x;
    const u64 *seg = part + (u64)q * chunks * N;
    for (u32 i = threadIdx.x; i < N; i += blockDim.x) best[i] = seg[i];
    __syncthreads();
    for (u32 c = 1; c < chunks; c++) {
        const u64 *other = seg + (u64)c * N;
        if (other[0] <= best[N - 1]) continue; // block-uniform
        __syncthreads();
        fold_reversed<N>(best, other);
        lds_bitonic_merge_desc<N>(best, 1, 0);
    }
    if (threadIdx.x == 0) s_count = k; // k <= N
    __syncthreads();
    for (u32 i = threadIdx.x; i < k; i += blockDim.x)
        if (best[i] == 0ull && (i == 0u || best[i - 1] != 0ull)) s_count = i; // the filled entries come first
    __syncthreads();
    const u32 nout = s_count;
    for (u32 i = threadIdx.x; i < nout; i += blockDim.x) {
        out_ids[(u64)q * k + i] = (u32)best[i];
        out_scores[(u64)q * k + i] = simkey_inv((u32)(best[i] >> 32));
    }
    if (threadIdx.x == 0) out_counts[q] = nout;
}

template <int R>
hipError_t sb_launch(const SparseBruteIndex &ix, const SbQueries &qs, u32 B, u32 n_fast, u32 chunks, u64 span, u64 *part, u32 k, u32 *oi, float *os, u32 *oc) {
    if (n_fast) {
        hipLaunchKernelGGL(sparse_brute_scan_kernel<R>, dim3(chunks, (n_fast + SB_QB - 1) / SB_QB), dim3(SB_THREADS), 0, 0, ix, qs, n_fast, chunks, span, part);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (B - n_fast) {
        hipLaunchKernelGGL(sparse_brute_slow_kernel<R>, dim3(chunks, B - n_fast), dim3(64), 0, 0, ix, qs, n_fast, chunks, part);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sparse_brute_finish_kernel<R>, dim3(B), dim3(256), 0, 0, part, chunks, k, oi, os, oc);
    return hipGetLastError();
}

// may the fast path take the query?  Strictly ascending dimensions (so distinct), none equal to the empty marker, the table's load
bool sb_fast_query(const uint32_t *d, u32 np) {
    if (np > SB_MAX_PAIRS) return false;
    for (u32 i = 0; i < np; i++)
        if (d[i] == SB_EMPTY || (i && d[i] <= d[i - 1])) return false;
    return true;
}

} // namespace

namespace cosdev {

int32_t sparse_brute_topk(SparseBruteWs &ws, const SparseBruteIndex &ix, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 k,
                          uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (k > SPARSE_BRUTE_MAX_K) return cos_fail(COS_ERR_UNIMPLEMENTED, "k must be <= %u (the widest pool)", SPARSE_BRUTE_MAX_K);
    if (B > 0xFFFFu) return cos_fail(COS_ERR_INVALID, "batch of %u queries", B);
    for (u32 b = 0; b < B; b++)
        if (q_offsets[b + 1] < q_offsets[b]) return cos_fail(COS_ERR_INVALID, "query offsets decrease");
    const u32 nq = q_offsets[B];
    u32 R = 1;
    while (64u * R < k) R *= 2;
    // one image, one copy: [q_dims nq | q_vals nq | q_offsets B + 1 | list B]
    const size_t o_qv = (size_t)nq * 4, o_qo = o_qv + (size_t)nq * 4, o_list = o_qo + ((size_t)B + 1) * 4, bytes = o_list + (size_t)B * 4;
    HIP_TRY(ws.h_in.grow(bytes));
    unsigned char *h = ws.h_in;
    if (nq) {
        memcpy(h, q_dims, (size_t)nq * 4);
        memcpy(h + o_qv, q_vals, (size_t)nq * 4);
    }
    memcpy(h + o_qo, q_offsets, ((size_t)B + 1) * 4);
    u32 *list = (u32 *)(h + o_list);
    u32 n_fast = 0;
    std::vector<u32> slow;
    for (u32 b = 0; b < B; b++) {
        if (ix.rows_ascend && sb_fast_query(q_dims + q_offsets[b], q_offsets[b + 1] - q_offsets[b])) list[n_fast++] = b;
        else slow.push_back(b);
    }
    for (size_t i = 0; i < slow.size(); i++) list[n_fast + i] = slow[i];
    // chunks: enough workgroups to fill the chip a few times over, at least two tiles of nonzeros each, partial results within 64 MB
    const u32 qblocks = std::max<u32>(1u, (n_fast + SB_QB - 1) / SB_QB);
    u32 chunks = (u32)std::min<u64>(SB_MAX_CHUNKS, std::max<u64>(1ull, ix.nnz / (2ull * SB_TILE)));
    chunks = std::max<u32>(1u, std::min<u32>(chunks, std::max<u32>(1u, 1024u / qblocks)));
    while (chunks > 1u && (u64)B * chunks * 64u * R * 8u > (64ull << 20)) chunks /= 2u;
    const u64 span = ix.nnz / chunks + 1ull; // chunks * span > nnz: every row starts inside some chunk
    HIP_TRY(ws.w_in.grow(bytes));
    HIP_TRY(ws.w_part.grow((size_t)B * chunks * 64u * R * 8u));
    HIP_TRY(ws.w_oi.grow((size_t)B * k * 4));
    HIP_TRY(ws.w_os.grow((size_t)B * k * 4));
    HIP_TRY(ws.w_oc.grow((size_t)B * 4));
    if (!ws.ev0) HIP_TRY(hipEventCreate(&ws.ev0));
    if (!ws.ev1) HIP_TRY(hipEventCreate(&ws.ev1));
    unsigned char *d = ws.w_in.p;
    HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, 0));
    const SbQueries qs{(const u32 *)d, (const float *)(d + o_qv), (const u32 *)(d + o_qo), (const u32 *)(d + o_list)};
    auto launch = R == 1 ? sb_launch<1> : R == 2 ? sb_launch<2> : R == 4 ? sb_launch<4> : R == 8 ? sb_launch<8> : sb_launch<16>;
    HIP_TRY(hipEventRecord(ws.ev0, 0));
    HIP_TRY(launch(ix, qs, B, n_fast, chunks, span, ws.w_part.as<u64>(), k, ws.w_oi.as<u32>(), ws.w_os.as<float>(), ws.w_oc.as<u32>()));
    HIP_TRY(hipEventRecord(ws.ev1, 0));
    HIP_TRY(hipMemcpy(out_ids, ws.w_oi.p, (size_t)B * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_scores, ws.w_os.p, (size_t)B * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, ws.w_oc.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    // defined values behind a query's count, as cos_sparse_search_batch leaves them
    for (u32 q = 0; q < B; q++)
        for (u32 i = std::min(out_counts[q], k); i < k; i++) {
            out_ids[(size_t)q * k + i] = 0xFFFFFFFFu;
            out_scores[(size_t)q * k + i] = 0.0f;
        }
    HIP_TRY(hipEventSynchronize(ws.ev1));
    HIP_TRY(hipEventElapsedTime(&ws.kernel_ms, ws.ev0, ws.ev1));
    ws.queries = B;
    ws.slow_queries = B - n_fast;
    ws.blocks = chunks * ((n_fast + SB_QB - 1) / SB_QB) + chunks * (B - n_fast);
    ws.pool = 64u * R;
    ws.raw_bytes = ix.nnz * 8ull + ((u64)ix.n + 1ull) * 8ull;
    return COS_OK;
}

} // namespace cosdev
