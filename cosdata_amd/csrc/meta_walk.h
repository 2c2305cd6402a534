// meta_walk.h — what the two metadata walks (walk_meta_kernel, kernels_meta.hip; walk_meta_general_kernel,
// kernels_meta_general.hip) state once: the node kinds, the metadata dot, CosineSimilarity::calculate's dispatch over
// (node kind, query kind) and the merge of one filter walk's popped list into the level's candidate list.
//   CosineSimilarity::calculate, (node kind, query kind) arms           distance/cosine.rs:36-102
//   cosine_similarity_mdims                                             distance/cosine.rs:243-262
//   VectorData::replica_node_kind                                       models/types.rs:219-241
//   ann_search: -1.0 dropped, sorted descending, first 100 kept         vector_store.rs:293-311
// Every piece is inlined into its caller; the round structure of a kernel (windows, passes, rows in flight) is its own.
#pragma once
#include "walk_common.h"

namespace cosdev {

enum : int { KIND_BASE = 0, KIND_PSEUDO = 1, KIND_METADATA = 2 };

// dot_product_f32 in the order of dot_product_f32_simd (x86_64.rs:418-444) by ONE lane: 8 FMA chains over chunks of 8,
// ((s0+s1)+(s2+s3)) + ((s4+s5)+(s6+s7)), non-fused scalar tail.  a: query metadata dims (LDS), b: node mbits (global).
__device__ __forceinline__ float mdims_dot_ref(const float *__restrict__ a, const int32_t *__restrict__ b, u32 n) {
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = 0.0f;
    const u32 chunks = n >> 3;
    for (u32 c = 0; c < chunks; c++)
#pragma unroll
        for (int i = 0; i < 8; i++) s[i] = __fmaf_rn(a[c * 8 + i], (float)b[c * 8 + i], s[i]);
    float r = __fadd_rn(__fadd_rn(__fadd_rn(s[0], s[1]), __fadd_rn(s[2], s[3])), __fadd_rn(__fadd_rn(s[4], s[5]), __fadd_rn(s[6], s[7])));
    for (u32 i = chunks * 8; i < n; i++) r = __fadd_rn(r, __fmul_rn(a[i], (float)b[i]));
    return r;
}

// a query has no id (types.rs:227-236); a node being indexed has one: VectorData::replica_node_kind (types.rs:219-241)
__device__ __forceinline__ int meta_query_kind(float fmag, bool self_pseudo) {
    return fmag == 0.0f ? KIND_BASE : (self_pseudo ? KIND_PSEUDO : KIND_METADATA);
}

// CosineSimilarity::calculate's dispatch for (stored node, query with the filter in fq / fqi, both in LDS):
// returns 0 = the similarity is `sim`, 1 = the vector cosine decides, < 0 = -status.  Executed per LANE (its own node).
// k = the node's metadata row, ymag = its norm, nid = its id: loaded by the caller, TOGETHER with the node's vector row — loaded
// here they were one dependent trip to memory after the other.
__device__ __forceinline__ int meta_decide(const IndexDev &ix, const float *fq, const int32_t *fqi, u32 k, float ymag, u32 nid, float fmag, int xkind, float &sim) {
    if (ix.metric != 0u) return 1; // the other metrics never look at node kinds
    const u32 md = ix.mdim;
    const int ykind = ymag == 0.0f ? KIND_BASE : ((nid >= PSEUDO_LO && nid <= PSEUDO_HI) ? KIND_PSEUDO : KIND_METADATA);
    const int32_t *yb = ix.mbits + (u64)k * md;
    if (ykind == KIND_PSEUDO && xkind == KIND_METADATA) { // a metadata query strongly matches / mismatches a pseudo node
        bool eq = true;
        for (u32 j = 0; j < md; j++) eq &= yb[j] == fqi[j];
        sim = eq ? 1.0f : -1.0f;
        return 0;
    }
    if (ykind == KIND_PSEUDO && xkind == KIND_PSEUDO) { // two pseudo nodes (index time only): cosine_similarity_mdims (cosine.rs:243-262)
        const float dp = mdims_dot_ref(fq, yb, md);
        const float den = __fmul_rn(fmag, ymag);
        if (den == 0.0f) return -COS_ERR_CALCULATION;
        sim = __fdiv_rn(dp, den);
        return 0;
    }
    if (ykind == KIND_BASE && xkind == KIND_BASE) return 1;
    if (ykind == KIND_METADATA && xkind == KIND_METADATA) {
        const float dp = mdims_dot_ref(fq, yb, md);
        const float den = __fmul_rn(fmag, ymag);
        if (den == 0.0f) return -COS_ERR_CALCULATION;
        if (__fdiv_rn(dp, den) > 0.99f) return 1;
        sim = -1.0f;
        return 0;
    }
    if (ykind == KIND_BASE && xkind == KIND_METADATA) { sim = 0.0f; return 0; }
    return -COS_ERR_UNIMPLEMENTED; // the reference's unreachable!() arms (a Base-kind query under the pseudo root, ...)
}

// filter f's dimensions -> LDS, as i32 and as f32, by one wave
__device__ __forceinline__ void meta_stage_filter(const WalkArgs &wa, u32 f, u32 md, int32_t *fqi, float *fq, int lane) {
    for (u32 j = lane; j < md; j += 64) {
        const int32_t v = wa.f_dims[(u64)f * md + j];
        fqi[j] = v;
        fq[j] = (float)v;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
}

// One filter walk's result into the level's candidate list, by one wave: the popped list res[0, npop) sorted descending, first keep_n;
// entries with cosine exactly -1.0 are dropped (never at index time); merged into acc[0, nacc) (sorted descending, first keep_n kept).
// res (>= 128 entries, >= 64 * R) is dead afterwards: it doubles as the staging list.  Returns the new nacc.
template <int R, bool INDEXING>
__device__ __forceinline__ u32 meta_merge_walk(u64 *res, u64 *acc, u32 npop, u32 nacc, u32 keep_n, u32 metric, int lane) {
    u64 rk[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const u32 e = (u32)lane * R + r;
        rk[r] = e < npop ? res[e] : 0ull;
    }
    bitonic_sort_desc<R>(rk, lane);
    const u32 keepn = npop < keep_n ? npop : keep_n;
    const u32 minus1 = metric_key(metric, -1.0f);
    u64 mk[4]; // 256 >= 100 (so far) + 100 (this walk)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const u32 e = (u32)lane * 4 + r;
        mk[r] = e < nacc ? acc[e] : 0ull;
    }
    __builtin_amdgcn_wave_barrier();
    // the walk's survivors, compacted (they stay in descending order) into the staging list, then appended behind the
    // nacc entries already there and sorted together
    bool okf[R];
    u32 mine = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const u32 e = (u32)lane * R + r;
        okf[r] = e < keepn && (INDEXING || !(metric == 0u && (u32)(rk[r] >> 32) == minus1));
        mine += okf[r] ? 1u : 0u;
    }
    u32 incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = (u32)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += t;
    }
    const u32 nsurv = readlane_u32(incl, 63); // <= 100
    u32 pos = incl - mine;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (okf[r]) res[pos++] = rk[r];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const u32 e = (u32)lane * 4 + r;
        if (e >= nacc && e < nacc + nsurv) mk[r] = res[e - nacc];
    }
    bitonic_sort_desc<4>(mk, lane);
    nacc = nacc + nsurv < keep_n ? nacc + nsurv : keep_n;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const u32 e = (u32)lane * 4 + r;
        if (e < nacc) acc[e] = mk[r];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    return nacc;
}

// the level's list (acc[0, nacc), node indices) out: ids, similarities, the node indices for the link kernels at index time
template <bool INDEXING>
__device__ __forceinline__ void meta_write_level(const u64 *acc, u32 nacc, const IndexDev &ix, const LevelDev &lv, const WalkArgs &wa, u32 qi, u32 out_slot, int lane) {
    const u64 obase = ((u64)qi * (ix.num_layers + 1) + out_slot) * wa.keep;
    for (u32 e = lane; e < nacc; e += 64) {
        const u64 kv = acc[e];
        wa.out_ids[obase + e] = lv.node_id[(u32)kv];
        wa.out_sims[obase + e] = metric_key_inv(ix.metric, (u32)(kv >> 32));
        if (INDEXING && wa.out_nodes) wa.out_nodes[obase + e] = (u32)kv;
    }
    if (lane == 0) wa.out_counts[(u64)qi * (ix.num_layers + 1) + out_slot] = nacc;
}

// host side (engine_internal.h declares the same for engine.hip and builder.hip, which do not see the kernels' headers)
size_t walk_meta_smem_bytes(const IndexDev &ix, u32 ef, int eng);
size_t walk_meta_general_smem_bytes(const IndexDev &ix, u32 ef, int eng);
bool walk_meta_general_needed(int eng, const IndexDev &ix);
hipError_t launch_walk_meta_general(int eng, bool indexing, const IndexDev &ix, const WalkArgs &wa, hipStream_t st);

} // namespace cosdev
