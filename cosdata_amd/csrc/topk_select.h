// topk_select.h — keeping the best N keys of a stream: the pools, sorts and merges every selecting kernel shares (device only).
// The conventions, stated once:
//   * a key is a u64, (score key << 32 | id) wherever it comes from; 0 means "empty" and no real key is 0;
//   * every order is DESCENDING: the best key first, the empty entries last;
//   * a wave holds 64 * R keys R per lane in the blocked layout e = lane * R + r (position e of the sorted sequence), and memory
//     holds them as pool[e];
//   * `thr` is the pool's last key — what a new key has to beat — and 0 while the pool is not full;
//   * ties between equal scores are resolved by the key's low half (the larger id first): keys are unique, so the order of the
//     u64 keys is the whole rule.
// Register networks (one wave, cross-lane moves) come first, the LDS networks (one workgroup, any size) last.
// Checked on the device primitive by primitive, at every width the kernels instantiate, by tests/cxx/topk_select_check.hip (host models: tests/cxx/topk_check_host.h).
#pragma once
#include "device_common.h"

namespace cosdev {

// ---- bitonic networks in registers --------------------------------------------------------------------------------------------
// Bitonic sort of 64 * R keys: stage `size` makes runs of `size` keys, alternately descending / ascending (one descending run at
// size = 64 * R), by compare-exchange steps between partners stride = size / 2, .., 1 positions apart; empty entries sink to the
// end.  Fully unrolled: every register index is static.
template <int R>
__device__ __forceinline__ void bitonic_sort_desc(u64 (&k)[R], int lane) {
    constexpr int N = WAVE * R;
#pragma unroll
    for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= R) {
                const int lmask = stride / R;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    u64 other = shfl_xor_u64(k[r], lmask);
                    int e = lane * R + r;
                    bool desc = (e & size) == 0;
                    bool lower = (e & stride) == 0;
                    bool keepmax = (desc == lower);
                    u64 mx = k[r] > other ? k[r] : other;
                    u64 mn = k[r] > other ? other : k[r];
                    k[r] = keepmax ? mx : mn;
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if ((r & stride) == 0) {
                        int e = lane * R + r;
                        bool desc = (e & size) == 0;
                        u64 a = k[r], b = k[r | stride];
                        u64 mx = a > b ? a : b, mn = a > b ? b : a;
                        k[r] = desc ? mx : mn;
                        k[r | stride] = desc ? mn : mx;
                    }
                }
            }
        }
    }
}
// A bitonic sequence of 64 * R keys -> sorted: the sort's last stage (size = 64 * R, every direction "descending").  Its own text:
// written with the sort over one shared step, either the sorting or the merging kernels change (flat_select_merge_w<16> 1457 -> 1583
// instructions, flat_select_segments_w<16> 108 -> 132 VGPRs).
template <int R, int STRIDE>
__device__ __forceinline__ void bitonic_merge_step(u64 (&k)[R], int lane) {
    if constexpr (STRIDE >= R) {
        constexpr int lmask = STRIDE / R;
        const bool lower = (lane & lmask) == 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const u64 other = shfl_xor_u64(k[r], lmask);
            const u64 mx = k[r] > other ? k[r] : other, mn = k[r] > other ? other : k[r];
            k[r] = lower ? mx : mn;
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; r++) {
            if ((r & STRIDE) == 0) {
                const u64 a = k[r], b = k[r | STRIDE];
                k[r] = a > b ? a : b;
                k[r | STRIDE] = a > b ? b : a;
            }
        }
    }
    if constexpr (STRIDE > 1) bitonic_merge_step<R, STRIDE / 2>(k, lane);
}
template <int R>
__device__ __forceinline__ void bitonic_merge_desc(u64 (&k)[R], int lane) {
    bitonic_merge_step<R, WAVE * R / 2>(k, lane);
}
// pool, other: sorted -> pool = the best 64 * R of both, sorted (max(pool[e], other[P - 1 - e]) is bitonic and holds them)
template <int R>
__device__ __forceinline__ void merge_sorted_desc(u64 (&pool)[R], const u64 (&other)[R], int lane) {
#pragma unroll
    for (int r = 0; r < R; r++) { // position e of the reversed list = position P - 1 - e = (lane 63 - lane, register R - 1 - r)
        const u64 o = other[R - 1 - r];
        const u32 lo = (u32)__shfl((int)(u32)o, 63 - lane, WAVE), hi = (u32)__shfl((int)(u32)(o >> 32), 63 - lane, WAVE);
        const u64 rev = ((u64)hi << 32) | lo;
        pool[r] = pool[r] > rev ? pool[r] : rev;
    }
    bitonic_merge_desc<R>(pool, lane);
}

// ---- keys that enter one at a time: the sorted register pool ---------------------------------------------------------------------
// Replaces the reference's BinaryHeap (vector_store.rs:1125): only the best (ef - popped) entries
// can ever be popped, so a bounded sorted pool reproduces the pop sequence exactly.
template <int R>
struct Pool {
    u64 e[R];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int r = 0; r < R; r++) e[r] = 0;
    }
    __device__ __forceinline__ u64 head() const { return readlane_u64(e[0], 0); }
    // entry at sorted position I (wave-uniform result); static register index
    template <int I>
    __device__ __forceinline__ u64 peek() const { return readlane_u64(e[I % R], I / R); }
    // entry at sorted position pos, pos wave-uniform but only known at run time.  Every register's candidate is read with
    // v_readlane and the choice is made among SCALARS: selecting the vector register first (x = e[pos % R]) made the compiler
    // index the pool as an array and move it to scratch memory (40 B per lane, the ef 256 walk 35 % slower).
    __device__ __forceinline__ u64 peek_dyn(u32 pos) const {
        const int l = (int)(pos / (u32)R);
        const u32 rr = pos % (u32)R;
        u64 v = readlane_u64(e[0], l);
#pragma unroll
        for (int r = 1; r < R; r++) {
            const u64 t = readlane_u64(e[r], l);
            v = rr == (u32)r ? t : v;
        }
        return v;
    }
    // node index (low half) of the entry at sorted position I: one v_readlane
    template <int I>
    __device__ __forceinline__ u32 peek_node() const { return readlane_u32((u32)e[I % R], I / R); }
    __device__ __forceinline__ void pop_head(int lane) {
        // lane l <- lane l+1's first entry; lane 63 <- empty (bound_ctrl zero fill: two DPP moves, nothing else)
        const u64 nxt = ((u64)dpp_mov_z<0x130>((u32)(e[0] >> 32)) << 32) | dpp_mov_z<0x130>((u32)e[0]);
#pragma unroll
        for (int r = 0; r + 1 < R; r++) e[r] = e[r + 1];
        e[R - 1] = nxt;
    }
    // number of entries strictly greater than k (= insertion position); k is wave-uniform
    __device__ __forceinline__ int rank_of(u64 k) const {
        int p = 0;
#pragma unroll
        for (int r = 0; r < R; r++) p += __popcll(__ballot(e[r] > k));
        return p;
    }
    // insert wave-uniform key k at position p (entries >= p shift up by one, the last one drops)
    __device__ __forceinline__ void insert_at(u64 k, int p, int lane) {
        if constexpr (R == 1) {
            // one entry per lane: lanes above p take their lower neighbour's entry (two DPP moves + one compare + two selects),
            // lane p takes k by v_writelane (no compare against p, no broadcast of k into a VGPR pair)
            u32 lo = (u32)e[0], hi = (u32)(e[0] >> 32);
            const u32 slo = dpp_mov_z<0x138>(lo), shi = dpp_mov_z<0x138>(hi); // lane 0 has no lower neighbour and never shifts
            const bool up = lane > p;
            lo = up ? slo : lo;
            hi = up ? shi : hi;
            lo = writelane_dyn(lo, (u32)k, p);
            hi = writelane_dyn(hi, (u32)(k >> 32), p);
            e[0] = ((u64)hi << 32) | lo;
            return;
        }
        const int lp = p / R, rp = p % R;
        const u64 prev_last = dpp_wave_shr1_u64(e[R - 1], 0ull); // lane l <- lane l-1's last entry
#pragma unroll
        for (int r = R - 1; r >= 0; r--) {
            u64 src = (r == 0) ? prev_last : e[r > 0 ? r - 1 : 0];
            bool shift = (lane > lp) || (lane == lp && r > rp);
            bool ins = (lane == lp && r == rp);
            e[r] = ins ? k : (shift ? src : e[r]);
        }
    }
};

// The keys of the lanes named by `m` (a subset of the lanes whose key beats thr) go into the pool, lowest lane first; a key that
// an earlier insert has pushed below the bar is dropped.  thr follows the pool's last key.
template <int R>
__device__ __forceinline__ void pool_fold_mask(Pool<R> &pool, u64 &thr, u64 key, u64 m, int lane) {
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const u64 kk = readlane_u64(key, l);
        if (kk > thr) {
            pool.insert_at(kk, pool.rank_of(kk), lane);
            thr = readlane_u64(pool.e[R - 1], WAVE - 1);
        }
    }
}
// a wave's 64 keys (one per lane, 0 = none) folded into the pool
template <int R>
__device__ __forceinline__ void pool_fold_lanes(Pool<R> &pool, u64 &thr, u64 key, int lane) {
    pool_fold_mask<R>(pool, thr, key, ballot64(key > thr), lane);
}

// ---- keys that enter by the thousand: batches ---------------------------------------------------------------------------------------
// A single insert into a 64 * R pool costs ~6 R instructions; here what beats thr is compacted into an LDS batch of up to P = 64 * R
// keys, a full batch is sorted and merged with the pool: the cost per key is that of the sort divided by the batch, ~R log^2(P) / P.
// `count` keys, key i = load(i); pool sorted, thr as above on entry and exit.
// batch: P keys of LDS, this wave's own (the workgroup is one wave: the barriers only order the LDS traffic).
template <int R, typename Load>
__device__ __forceinline__ void fold_stream(u64 (&pool)[R], u64 &thr, u64 *batch, u32 count, Load load, int lane) {
    constexpr u32 P = WAVE * R;
    u32 cnt = 0; // keys in the batch (wave-uniform)
    auto flush = [&]() {
        __syncthreads();
        u64 b[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const u32 i = (u32)lane * R + r;
            b[r] = i < cnt ? batch[i] : 0ull;
        }
        __syncthreads();
        bitonic_sort_desc<R>(b, lane);
        merge_sorted_desc<R>(pool, b, lane);
        thr = readlane_u64(pool[R - 1], WAVE - 1);
        cnt = 0;
    };
    const u64 below = (1ull << lane) - 1ull;
    for (u32 c = 0; c < count; c += WAVE) {
        if (cnt + WAVE > P) flush(); // the batch may not take 64 more: every write below stays inside batch[P]
        const u64 key = c + lane < count ? load(c + (u32)lane) : 0ull;
        const bool in = key > thr;
        const u64 m = ballot64(in);
        if (in) batch[cnt + (u32)__popcll(m & below)] = key;
        cnt += (u32)__popcll(m);
    }
    if (cnt) flush();
}

// ---- the same networks over keys in LDS, run by a whole workgroup -------------------------------------------------------------------
// log2(N) rounds of one compare-exchange per thread and pair, where folding N keys into a register pool by single inserts would
// be N inserts of ~150 wave instructions each on one wave.
// `nseq` bitonic sequences of N keys, sequence j at buf + j * pitch -> each sorted.  Ends with a barrier.
template <u32 N>
__device__ __forceinline__ void lds_bitonic_merge_desc(u64 *buf, u32 nseq, u32 pitch) {
    for (u32 stride = N / 2; stride > 0; stride >>= 1) {
        __syncthreads();
        for (u32 p = threadIdx.x; p < nseq * (N / 2); p += blockDim.x) {
            u64 *b = buf + (p / (N / 2)) * pitch;
            const u32 j = p % (N / 2);
            const u32 i = ((j & ~(stride - 1u)) << 1) | (j & (stride - 1u)); // the pair (i, i + stride)
            const u64 x = b[i], y = b[i + stride];
            if (x < y) { b[i] = y; b[i + stride] = x; }
        }
    }
    __syncthreads();
}
// any N keys -> sorted (empty entries sink to the end).  Ends with a barrier.
template <u32 N>
__device__ __forceinline__ void lds_bitonic_sort_desc(u64 *buf) {
    for (u32 size = 2; size <= N; size <<= 1)
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (u32 j = threadIdx.x; j < N / 2; j += blockDim.x) {
                const u32 i = ((j & ~(stride - 1u)) << 1) | (j & (stride - 1u));
                const bool desc = (i & size) == 0u;
                const u64 x = buf[i], y = buf[i + stride];
                if ((x < y) == desc) { buf[i] = y; buf[i + stride] = x; }
            }
        }
    __syncthreads();
}
// best[i] = max(best[i], other[N - 1 - i]) for two sorted sequences is a bitonic sequence of the best N keys of both (the
// first half-cleaner of the merge network); lds_bitonic_merge_desc sorts it.  `other` may be LDS or global memory.
template <u32 N>
__device__ __forceinline__ void fold_reversed(u64 *best, const u64 *other) {
    for (u32 i = threadIdx.x; i < N; i += blockDim.x) {
        const u64 x = best[i], y = other[N - 1u - i];
        best[i] = x > y ? x : y;
    }
}

} // namespace cosdev
