// postings_update.h — what an insert into resident postings does the same way for every posting format (BM25: kernels_hybrid.hip,
// learned-sparse in both layouts: kernels_sparse.hip): the merge of old lists and delta into new arrays, the tile directory of
// the new arrays, and the host's share of both.  A format is a small struct passed to the kernels by value; the indexes keep what
// is theirs (the delta's order, the offsets arithmetic, deletes, streams, the swap).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "engine_internal.h"

namespace cosdev {

constexpr u32 MERGE_PIECE = 4096;          // postings of the OUTPUT per workgroup: 256 threads x 4 rounds x 4 postings
constexpr u32 POSTINGS_TILE = 8192;        // ids per LDS accumulator tile of the search kernels = per column of the tile directory
constexpr u32 POSTINGS_NONE = 0xFFFFFFFFu; // "no row" in a directory's row table, "no entry" in a merged key table

// first position in [lo, hi) whose id is >= key (the lists are id-sorted); ids(p) = id of posting p
template <typename Ids>
__device__ __forceinline__ u64 postings_lower_bound(const Ids ids, u64 lo, u64 hi, u32 key) {
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (ids(mid) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the list that owns posting j of the new array: the LAST t in [lo, hi] whose list starts at or before j (new_off(t) = old_off[t] +
// del_off[t]; an empty list shares its start with the list behind it and is passed over).  Needs new_off(lo) <= j.
__device__ __forceinline__ u32 merge_owner_of(const u64 *__restrict__ old_off, const u64 *__restrict__ del_off, u32 lo, u32 hi, u64 j) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (old_off[mid] + del_off[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// new list t = old list t, then the delta's postings of t (ids above every id of the old list: still ascending).
// old_off / del_off [T + 1]: where list t's old postings / delta postings start, both indexed by the NEW key table (a list that
// exists only in the update has an empty old part, an untouched list an empty delta part).  One workgroup per MERGE_PIECE postings
// of the OUTPUT, whatever the list lengths: a 400 000-posting list is 98 workgroups, 4096 one-posting lists are one.  A thread
// moves 4 consecutive output postings; when they come from one list and one source they are 4 consecutive source postings
// (global_load_dwordx4 where a posting's field is 4 bytes, the source only 4-byte aligned) and always one store4 (16 bytes per
// 4-byte field: the piece and the arrays are 16-byte aligned).
// Fmt: P = one posting in registers; from_old(p) / from_delta(p) read posting p of the old arrays / of the delta, zero() fills the
// slots past the end, store4(j, v) writes new postings j .. j + 3 (j a multiple of 4), store1(j, v) one posting of the tail.
template <typename Fmt>
__global__ __launch_bounds__(256) void postings_merge_kernel(const Fmt fmt, const u64 *__restrict__ old_off, const u64 *__restrict__ del_off, u32 T,
                                                             u64 nnz) {
    const u64 p0 = (u64)blockIdx.x * MERGE_PIECE;
    if (p0 >= nnz) return;
    const u64 p1 = p0 + MERGE_PIECE < nnz ? p0 + MERGE_PIECE : nnz;
    const u32 t_lo = merge_owner_of(old_off, del_off, 0, T - 1, p0); // block-uniform: the piece's first and last list bound every thread's search
    const u32 t_hi = merge_owner_of(old_off, del_off, t_lo, T - 1, p1 - 1);
    for (u64 j0 = p0 + (u64)threadIdx.x * 4; j0 < p1; j0 += 1024) {
        u32 t = merge_owner_of(old_off, del_off, t_lo, t_hi, j0);
        u64 ob = old_off[t], db = del_off[t];
        u64 ol = old_off[t + 1] - ob;
        const u64 ne = old_off[t + 1] + del_off[t + 1];
        u64 k = j0 - ob - db;
        typename Fmt::P v[4];
        if (j0 + 4 <= ne && k + 4 <= ol) { // one list, the old part: 4 consecutive postings of it
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = fmt.from_old(ob + k + u);
        } else if (j0 + 4 <= ne && k >= ol) { // one list, the delta part
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = fmt.from_delta(db + (k - ol) + u);
        } else { // a list boundary or the old/delta seam inside the 4: posting by posting
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const u64 j = j0 + u;
                v[u] = fmt.zero();
                if (j < nnz) {
                    while (j >= old_off[t + 1] + del_off[t + 1]) t++; // j < nnz = new_off(T): stops at t <= T - 1
                    ob = old_off[t];
                    db = del_off[t];
                    ol = old_off[t + 1] - ob;
                    k = j - ob - db;
                    v[u] = k < ol ? fmt.from_old(ob + k) : fmt.from_delta(db + (k - ol));
                }
            }
        }
        if (j0 + 4 <= nnz) fmt.store4(j0, v);
        else {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (j0 + u < nnz) fmt.store1(j0 + u, v[u]);
        }
    }
}

// tile_dir[row][t] = offset (from the list's begin) of the first posting with id >= t * POSTINGS_TILE, t = 0 .. n_tiles; the last
// column is the list's length.  One lower-bound search per entry; the same values the host passes of the create functions write.
template <typename Ids>
__global__ __launch_bounds__(256) void postings_tile_dir_kernel(const Ids ids, const u64 *__restrict__ row_begin, const u32 *__restrict__ row_len, u32 rows,
                                                                u32 n_tiles, u32 *__restrict__ tile_dir) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 width = (u64)n_tiles + 1;
    if (idx >= (u64)rows * width) return;
    const u32 row = (u32)(idx / width), t = (u32)(idx % width);
    const u64 lo = row_begin[row];
    const u32 len = row_len[row];
    tile_dir[idx] = t == n_tiles ? len : (u32)(postings_lower_bound(ids, lo, lo + len, t * POSTINGS_TILE) - lo); // t < n_tiles: t * TILE <= the largest id
}

// offsets[0 .. m] of an update call: start at 0 and never decrease.  `array` and `item` are the caller's nouns in the message.
inline int32_t postings_check_offsets(const uint64_t *offsets, u32 m, const char *array, const char *item) {
    if (offsets[0] != 0) return cos_fail(COS_ERR_INVALID, "%s[0] must be 0", array);
    for (u32 i = 0; i < m; i++)
        if (offsets[i + 1] < offsets[i]) return cos_fail(COS_ERR_INVALID, "%s must not decrease (%s %u)", array, item, i);
    return COS_OK;
}

// two-way merge of two strictly ascending key tables (the index's and the update's): the new table and, per new slot, the
// index of the key in either input or POSTINGS_NONE
struct MergedKeys {
    std::vector<u32> keys, old_of, del_of;
};
inline MergedKeys postings_merge_keys(const std::vector<u32> &old_keys, const std::vector<u32> &del_keys) {
    const size_t n_old = old_keys.size(), n_del = del_keys.size();
    MergedKeys m;
    m.keys.reserve(n_old + n_del); m.old_of.reserve(n_old + n_del); m.del_of.reserve(n_old + n_del);
    size_t i = 0, j = 0;
    while (i < n_old || j < n_del) {
        const bool take_old = j == n_del || (i < n_old && old_keys[i] <= del_keys[j]);
        const bool take_del = i == n_old || (j < n_del && del_keys[j] <= old_keys[i]);
        m.keys.push_back(take_old ? old_keys[i] : del_keys[j]);
        m.old_of.push_back(take_old ? (u32)i++ : POSTINGS_NONE);
        m.del_of.push_back(take_del ? (u32)j++ : POSTINGS_NONE);
    }
    return m;
}

// Tile directory of new arrays, searched on the device.  List t of T spans postings [off[t * stride], off[t * stride + span]);
// a list longer than min_len gets a row: dir_row[t] = its row or POSTINGS_NONE, d_dir = [rows][n_tiles + 1].  A list of more than
// 2^32 - 1 postings ends the call with what too_long(t) returns (the caller's message).  Runs on `st` and drains it before it
// returns: the two row tables are locals.
template <typename Ids, typename TooLong>
int32_t postings_build_dir(const Ids ids, const u64 *off, size_t stride, size_t span, u32 T, u32 min_len, u32 n_tiles, hipStream_t st, TooLong too_long,
                           std::vector<u32> &dir_row, u32 &rows_out, DevArr<u32> &d_dir) {
    std::vector<u64> row_begin;
    std::vector<u32> row_len;
    dir_row.assign(T, POSTINGS_NONE);
    for (u32 t = 0; t < T; t++) {
        const u64 b = off[(size_t)t * stride], e = off[(size_t)t * stride + span];
        if (e - b <= min_len) continue;
        if (e - b > 0xFFFFFFFFull) return too_long(t);
        dir_row[t] = (u32)row_begin.size();
        row_begin.push_back(b);
        row_len.push_back((u32)(e - b));
    }
    const u32 rows = (u32)row_begin.size();
    const u64 dir_words = (u64)rows * (n_tiles + 1);
    rows_out = rows;
    HIP_TRY(d_dir.alloc(dir_words));
    if (!rows) return COS_OK;
    if ((dir_words + 255) / 256 > 0x7FFFFFFFull) return cos_fail(COS_ERR_UNIMPLEMENTED, "tile directory too large for one launch");
    DevArr<u64> d_row_begin;
    DevArr<u32> d_row_len;
    HIP_TRY(d_row_begin.alloc(rows));
    HIP_TRY(d_row_len.alloc(rows));
    HIP_TRY(hipMemcpy(d_row_begin, row_begin.data(), (size_t)rows * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_row_len, row_len.data(), (size_t)rows * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(postings_tile_dir_kernel<Ids>, dim3((u32)((dir_words + 255) / 256)), dim3(256), 0, st, ids, d_row_begin.p, d_row_len.p, rows, n_tiles,
                       d_dir.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return COS_OK;
}

} // namespace cosdev
