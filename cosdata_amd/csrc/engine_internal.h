// engine_internal.h — host-side structures shared by engine.hip and builder.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cosdata_hip.h"
#include "engine_types.h"
#include "tuning.h"
#include "link_types.h"
#include "dev_mem.h"
#include "walk_plan.h"
#include "table_nested.h"
#include "walk_operands.h"

namespace hybrid_plan {
struct Slot; // hybrid_plan.h
}

namespace cosdev {
hipError_t launch_fill_i32(int32_t *p, u64 n, int32_t v, hipStream_t st);
hipError_t launch_edge_pairs(const u32 *adj_vec, const u32 *node_vec, u32 node0, u32 cn, u32 M, u32 *px, u32 *py, hipStream_t st);
hipError_t launch_edge_keys(const u32 *adj_vec, const float *sims, const int32_t *st_in, u32 node0, u32 cn, u32 M, u32 metric, int32_t *key, int32_t *fail, hipStream_t st);
hipError_t launch_low_cache(const u32 *adj_vec, const int32_t *key, u32 n, u32 M, int32_t kmin, int32_t kmax, uint8_t *low_idx, int32_t *low_key, hipStream_t st);
hipError_t launch_unlink(const LinkArgs &a, const u32 *dn, u32 *status, hipStream_t st);
hipError_t launch_index_pair_distances(int eng, const uint8_t *codes, const float *mags, u64 row_stride, u32 nchunks, u32 dim, u32 metric, const u32 *d_pair_x,
                                       const u32 *d_pair_y, u32 n_pairs, float *d_out, int32_t *d_status, hipStream_t st); // kernels_misc.hip
// a level's growth (cos_index_append: the tail is the root; cos_index_append_meta: the pseudo nodes): rows [tail_first, old_n) move up by
// `add`, the rows between are `fill`; of the copied values, remap_from becomes remap_to, any other at or above shift_from (the empty slot
// excepted) gains shift_add
hipError_t launch_grow_tail(const u32 *src, u32 *dst, u32 old_n, u32 tail_first, u32 add, u32 M, u32 fill, const GrowValues &v, hipStream_t st);
hipError_t launch_grow_tail_bytes(const uint8_t *src, uint8_t *dst, u32 old_n, u32 tail_first, u32 add, uint8_t fill, hipStream_t st);
hipError_t launch_fill_adj_mag(const u32 *adj_vec, const float *mags, float *adj_mag, u32 n, u32 M, u32 slots, hipStream_t st);
hipError_t launch_fill_adj_up(const u32 *adj_vec, const u32 *adj_node, const float *mags, const u32 *child_up, u32 n_up, u32 *up, AdjUp *adj_up, u32 n, u32 M, u32 slots,
                              hipStream_t st, const u32 *up_col = nullptr);
hipError_t launch_fill_adj_tab(const u32 *adj_node, const u32 *tab_col, u32 n, u32 M, u32 node_bits, u32 *adj_tab, hipStream_t st);
hipError_t launch_link_round(const LinkArgs &a, u32 maxM, const u32 *pend, const u32 *pcount, u32 *next, u32 *next_count, u32 *evq, u32 *evq_count,
                             u32 count_ub, u32 round, hipStream_t st);
hipError_t launch_quantize_rows(int eng, const float *x, u64 x_stride, u32 n, u32 dim, float lo, float hi, uint8_t *codes,
                                u64 row_stride, float *mags, float *raw_mags, hipStream_t st, u32 *code_sums = nullptr); // code_sums: [n] sums of the code bytes (u8 only)
hipError_t launch_walk(int eng, const IndexDev &ix, const WalkArgs &wa, WalkKernel kernel, hipStream_t st); // `kernel`: WalkPlan::kernel (walk_plan.h)
static_assert(WALK_PLAN_MAX_LEVELS == MAX_LEVELS && WALK_PLAN_ENG_U8 == ENG_U8 && WALK_PLAN_ENG_Q2 == ENG_Q2 && WALK_PLAN_FAST_MAX_EF == WALK_FAST_MAX_EF &&
              COS_STORAGE_U8 == 0u && COS_VISITED_REF == 0u, "walk_plan.h restates these");
hipError_t launch_walk_meta(int eng, const IndexDev &ix, const WalkArgs &wa, hipStream_t st);
hipError_t launch_walk_meta_index(int eng, const IndexDev &ix, const WalkArgs &wa, hipStream_t st);
hipError_t launch_finalize(const IndexDev &ix, const float *queries, u64 q_stride, const float *q_raw_mags, const u32 *walk_ids,
                           const float *walk_sims, const u32 *walk_counts, const int32_t *walk_status, u32 B, u32 top_k,
                           u32 *out_ids, float *out_scores, u32 *out_counts, int32_t *out_status, u64 *out_rerank_rows,
                           hipStream_t st, const u32 *q_order = nullptr, u32 *slow_list = nullptr);
// buffers of the locality order of one workspace's big launches (kernels_order.hip)
struct WalkOrder {
    u32 cap = 0;                // queries every array below holds (0 after a failed reservation)
    DevArr<u32> entry0;         // [cap] level-0 entry node per query
    DevArr<u32> order_key;      // [cap]
    DevArr<u32> keys_sorted;    // [cap]
    DevArr<u32> iota, vals_sorted, q_order; // [cap]
    DevBuf tmp;                 // radix sort scratch
};
hipError_t walk_order_reserve(WalkOrder &o, u32 B); // synchronous (re)allocation
hipError_t launch_walk_order(WalkOrder &o, u32 B, u32 key_max, u32 num_xcd, hipStream_t st, u32 unit = 1u); // unit: queries per workgroup of the range below
// the last range of an ordered launch, two sorted neighbours per workgroup (kernels_walk_pair.hip; walk_pair_plan.h decides)
hipError_t launch_walk_pair(const IndexDev &ix, const WalkArgs &wa, u32 cache_entries, u64 *out_pair, hipStream_t st);
// level table of the walk (kernels_flat.hip; WalkArgs::tab)
hipError_t launch_level_table_gather(const uint8_t *codes, const float *mags, u64 row_stride, const u32 *node_vec, u32 n, u32 col0,
                                     uint8_t *tcodes, float *tmags, hipStream_t st);
hipError_t launch_code_sums(const uint8_t *codes, u64 row_stride, u32 n, u32 *sums, hipStream_t st);
hipError_t launch_level_table(int eng, const uint8_t *qcodes, const float *qmags, const u32 *qsums, uint8_t *qdig, u32 B, const uint8_t *tcodes, const float *tmags,
                              const u32 *tcsums, u64 row_stride, u32 ncols, float *tab, u64 tab_stride, u32 n_cus, hipStream_t st, u32 *queue, u32 wgs, bool first, bool shared);
bool level_table_gemm_queue(int eng, u64 row_stride);   // the table comes from the query-resident GEMM (work items claimed from a queue)
bool level_table_eng_supported(int eng, u64 row_stride); // storages the level table exists for (kernels_flat.hip)
int32_t quantize_ref_layout(uint32_t storage, uint32_t res, uint32_t dim, const float *x, uint32_t n, void *codes, float *mags);
int32_t distance_ref_layout(uint32_t metric, uint32_t storage, uint32_t res, uint32_t dim, const void *x_codes, const float *x_mags, uint32_t nx,
                            const void *y_codes, const float *y_mags, uint32_t ny, const uint32_t *pair_x, const uint32_t *pair_y, uint32_t n_pairs,
                            float *out, int32_t *status);
} // namespace cosdev

using cosdev::u32;
using cosdev::u64;

int32_t cos_fail(int32_t code, const char *fmt, ...);
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) return cos_fail(COS_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// The learned-sparse handle as the fused hybrid call sees it (kernels_sparse.hip defines it, kernels_hybrid.hip holds its lock from the
// limit check to the call's one synchronisation).  sparse_limits and sparse_search_locked are for a caller that holds sparse_mutex.
namespace cosdev {
std::mutex &sparse_mutex(cos_sparse *s);
int32_t sparse_device(const cos_sparse *s);
void sparse_limits(const cos_sparse *s, u32 *max_candidates, bool *have_raw, u32 *batch_bound);
int32_t sparse_search_locked(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 top_k,
                             float early_terminate_threshold, u32 reranking_factor, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts, hipStream_t st);
// The learned-sparse handle as one shard of a collection (shardset.hip holds the lock of every attached handle, in shard order, from the
// limit checks to the call's synchronisation).  sparse_shape and sparse_record_locked are for a caller that holds sparse_mutex.
void sparse_shape(const cos_sparse *s, u32 *bits, float *upper, u32 *n);
// resolve + scan + the record form of the finish kernel on `st`: the handle's best top_k * max(reranking_factor, 1) candidates per query
// under global ids id_base + local id, laid out as sparse_fold_plan::layout says, into d_record (8-byte aligned).  sparse_admit's rules;
// one batch in flight per handle.
int32_t sparse_record_locked(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 top_k,
                             float early_terminate_threshold, u32 reranking_factor, u32 id_base, u32 *d_record, hipStream_t st);
// gathered [S][record words] -> the collection's lists [B][top_k] / [B] (sparse_fold_rerank_kernel<N>, N from sparse_fold_plan::plan), on `st`
int32_t sparse_fold_rerank(const u32 *d_gathered, u32 S, u32 B, u32 top_k, u32 reranking_factor, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts,
                           hipStream_t st);
// The BM25 handle as a shard set sees it (kernels_hybrid.hip defines it; shardset.hip holds the lock of every attached handle, in shard
// order, from the term lookup to the call's synchronisation).  Everything but bm25_mutex / bm25_device is for a caller that holds the locks.
std::mutex &bm25_mutex(cos_bm25 *b);
int32_t bm25_device(const cos_bm25 *b);
long long bm25_largest_id(const cos_bm25 *b); // the largest document id the handle has ever held, -1 = none
hipStream_t bm25_stream(cos_bm25 *b);         // the handle's scoring stream (after bm25_set_score)
const u64 *bm25_buckets(const cos_bm25 *b);   // [B][512] bucket keys of the last scoring
int32_t bm25_dense_stream(cos_bm25 *b, hipStream_t *out); // the stream cos_hybrid_search_batch walks on (highest priority; created on first use)
// One query batch over the S handles of a collection (handle s: local ids, global id = doc_bases[s] + local): every term is resolved in
// every handle's term table, its idf is the collection's, every handle's table goes into its own pinned staging and its scoring kernel
// onto its own stream, into its own bucket array, keyed by global ids.
int32_t bm25_set_score(cos_bm25 *const *hs, const u32 *doc_bases, u32 S, const uint32_t *q_terms, const uint32_t *q_offsets, u32 B);
// gathered [S][B][512] bucket keys -> their element-wise maximum -> the lists of bm25_topk_kernel, [B][top_k] / [B], on `st`
int32_t bm25_fold_topk(const u64 *d_gathered, u32 S, u32 B, u32 top_k, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts, hipStream_t st);
// rrf_kernel over two resident list sets of stride k3 = 3 * top_k, on `st`
int32_t rrf_fuse_device(const u32 *d_first_ids, const u32 *d_first_counts, const u32 *d_second_ids, const u32 *d_second_counts, u32 k3, u32 B,
                        float fusion_constant_k, u32 top_k, u32 *d_out_ids, float *d_out_scores, u32 *d_out_counts, hipStream_t st);
// rrf_mixed_kernel over the three resident list sets of a mixed hybrid batch (stride k3; a set without queries is NULL), d_slots[B] the
// request's query_mapping (hybrid_plan.h), on `st`
int32_t rrf_mixed_device(const u32 *d_dense_ids, const u32 *d_dense_counts, const u32 *d_sparse_ids, const u32 *d_sparse_counts, const u32 *d_bm25_ids,
                         const u32 *d_bm25_counts, const hybrid_plan::Slot *d_slots, u32 k3, u32 B, float fusion_constant_k, u32 top_k, u32 *d_out_ids,
                         float *d_out_scores, u32 *d_out_counts, hipStream_t st);
} // namespace cosdev

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
struct LevelHost {
    std::vector<u32> node_ids; // ascending, root last
    std::vector<u32> nbr_ids;  // [n][M] internal ids / COS_SLOT_EMPTY
    DevArr<u32> d_adj_vec, d_adj_node, d_node_vec, d_child;
    DevArr<u32> d_node_id, d_node_meta; // pseudo-root component only (metadata-filtered search)
    DevArr<float> d_adj_mag; // [n][min(M, shortlist)] norms of the scanned neighbour slots (LevelDev::adj_mag), valid while WalkOperands::have_adj_mag()
    DevArr<cosdev::AdjUp> d_adj_up; // same shape: the neighbours' norms and nodes one level up (LevelDev::adj_up); only level WalkOperands::adj_up_level() has it
    DevArr<u32> d_adj_tab;   // [n][M] node | nested-table column of every neighbour slot (LevelDev::adj_tab); the table levels of WalkOperands::nested_set() have it
    u32 n = 0, M = 0;
    u32 root_idx = 0;        // pseudo-root component: node index of the pseudo root (base graph: the root is the last node)
    bool host_valid = false; // node_ids/nbr_ids mirror the device arrays
    void release() { // the level's device arrays and host mirrors (M stays)
        d_adj_vec.reset(); d_adj_node.reset(); d_node_vec.reset(); d_child.reset();
        d_node_id.reset(); d_node_meta.reset(); d_adj_mag.reset(); d_adj_up.reset(); d_adj_tab.reset();
        n = 0;
        node_ids.clear();
        nbr_ids.clear();
        host_valid = false;
    }
};

// The link state of a graph's levels, base graph and pseudo-root component alike (builder.hip): the similarity key of every neighbour
// slot and every node's cached (lowest index, lowest similarity), prob_node.rs:108, which is history (remove_neighbor_by_id does not
// refresh it) and cannot be recomputed from the graph; the claim tags of the link rounds; and, for the component only, every node's
// ReplicaNodeKind (LinkLevelDev::kind; empty on the base graph).  4 bytes per neighbour slot and 9 (10) bytes per node of a level.
struct LinkLevels {
    DevBuf key[cosdev::MAX_LEVELS], low_idx[cosdev::MAX_LEVELS], low_key[cosdev::MAX_LEVELS], owner[cosdev::MAX_LEVELS], kind[cosdev::MAX_LEVELS];
    void release() {
        for (int l = 0; l < cosdev::MAX_LEVELS; l++) { key[l].reset(); low_idx[l].reset(); low_key[l].reset(); owner[l].reset(); kind[l].reset(); }
    }
    // level l for nl nodes of M slots, contents undefined (cos_index_restore_link_state computes them); no `kind`
    int32_t alloc_level(u32 l, u32 nl, u32 M);
    // ... allocated and filled for a level without edges: every slot empty (INT32_MIN), cached lowest = (0, MetricResult::min)
    // (prob_node.rs:140), claim tags 0; kinds [nl] (host) = the nodes' kinds, nullptr = none (base graph)
    int32_t init_level(u32 l, u32 nl, u32 M, u32 metric, const uint8_t *kinds, hipStream_t st);
    // out's level l = this level of old_n nodes grown in front of its tail: the nodes [tail_first, old_n) move up by `add`, the `add` new ones
    // between are filled as init_level fills them (kind: 2, a Metadata replica); the claim tags are zeroed for a new tag epoch.  Fresh
    // buffers: this level is only read.
    int32_t grow_level(u32 l, u32 old_n, u32 tail_first, u32 add, u32 M, u32 metric, LinkLevels &out, hipStream_t st) const;
    void swap_level(u32 l, LinkLevels &o) { key[l].swap(o.key[l]); low_idx[l].swap(o.low_idx[l]); low_key[l].swap(o.low_key[l]); owner[l].swap(o.owner[l]); kind[l].swap(o.kind[l]); }
};

// What cos_index_build leaves behind so that cos_index_append can CONTINUE it (builder.hip): the link state of every level, the RNG
// stream after the last level draw, and how many vectors the graph holds.  As large as the adjacency itself;
// cos_index_release_link_state frees it.
struct LinkState {
    LinkLevels lv;
    uint64_t rng = 0;
    u32 n_built = 0;
    bool valid = false;
    void release() { lv.release(); valid = false; }
};

// EXACT-mode visited filters of one stream (WalkArgs::vis_bits / vis_log).  The bitset is zeroed once, when it is
// (re)allocated; afterwards every walk level undoes its own bits.
struct VisTab {
    DevArr<u32> bits, log;
    bool zeroed = false; // cleared whenever `bits` is reallocated
};
// sizes/allocates the filter for B queries at beam width ef and fills wa.vis_*
int32_t vis_tab_prepare(VisTab &vt, const cos_index *ix, u32 B, u32 ef, hipStream_t st, cosdev::WalkArgs &wa);

struct Workspace {
    u32 capB = 0, cap_topk = 0;
    DevArr<uint8_t> q_codes;
    DevArr<float> q_mags, q_raw_mags;
    DevArr<u32> walk_ids, walk_counts;
    DevArr<float> walk_sims;
    DevArr<int32_t> walk_status;
    DevArr<u64> stats;          // [B][4]
    DevArr<u64> stats2;         // [B][4] WalkArgs::out_stats2
    DevArr<u64> pair_stats;     // [B][2] WalkPairArgs::out_pair (cos_index_last_pair_stats); last_pair_cache: the cache entries of the last launch, 0 = it did not walk in pairs
    u32 last_pair_cache = 0;
    DevArr<float> tab;          // level table of this workspace's big launches [capB][tab_stride] (WalkArgs::tab), grown on demand
    DevArr<u32> qsums;          // [capB] code sums of the queries (the table GEMM's recentring term; written by quantize_rows_kernel)
    DevArr<u32> tab_queue;      // [1] next work item of the table GEMM in flight (level_table_areg), zeroed before its first part
    DevArr<uint8_t> qdig;       // [capB][dims] quaternary codes: the queries' i8 digit rows (the table GEMM's resident operand)
    DevArr<u32> fin_flags;      // [capB + 1] finalize_fast_kernel -> finalize_list_kernel hand-over: count, then the queries (kernels_finalize.hip)
    DevArr<u64> rerank_rows;    // [B]
    VisTab vis; // EXACT mode visited filters
    cosdev::WalkOrder order; // locality order of big launches (cos_index::walk_order_min_B)
    // host-API staging (device)
    DevArr<float> d_queries;
    DevArr<u32> d_out_ids, d_out_counts;
    DevArr<float> d_out_scores;
    DevArr<int32_t> d_out_status;
    // filtered search (cos_search_filtered_batch): the batch's filters [dims | norms | offsets], grown on demand — until
    // round 6 three hipMalloc / hipFree pairs per call (a hipFree drains the device)
    DevArr<u32> f_buf;
    // timing: a ring of event quadruples (before prep | after prep | after walk | after finalize), one per launch, so a
    // run of launches can be summarised afterwards without synchronising between them (cos_index_timing_summary)
    // + the inner marks of a big launch's walk: [4] before / [5] after the level-table GEMM (caller's stream), [6] after the upper
    // level range, [7] after the order sort (walk stream), [8] before / [9] after the GEMM's late part (WalkPlan::table_early_wgs: then
    // [4] / [5] bracket the early part; both on the caller's stream, the waits in front of either part outside the brackets); last_plan
    // says which of them the last launch recorded
    static constexpr u32 EV_RING = 128;
    static constexpr u32 EV_PER = 10;
    std::vector<hipEvent_t> ev; // [EV_RING][EV_PER]
    u32 ev_count = 0;           // timed launches since timing was switched on (ring position = ev_count % EV_RING)
    hipEvent_t walk_done = nullptr; // recorded after this workspace's walk kernel (walk chain, see cos_index::chain_*)
    hipEvent_t last_range = nullptr; // recorded when this workspace's walk reaches its LAST level range (after the order sort; an unsplit walk: its start)
    hipEvent_t upper_done = nullptr; // recorded when this workspace's walk has finished its FIRST level range (before the order sort; an unsplit walk: its start)
    hipStream_t walk_stream = nullptr; // low-priority stream big walks run on (cos_index::walk_side_min_B), created on first use
    hipEvent_t prep_done = nullptr, walk_fin = nullptr; // caller's stream -> walk stream -> finalize stream
    u32 lastB = 0;
    bool timed = false;
    cosdev::WalkPlan last_plan{}; // of the last launch: whether it used the level table / was cut into level ranges, and where
    Workspace() = default;
    Workspace(const Workspace &) = delete;
    ~Workspace() { // (the caller has drained the device: cos_index_destroy)
        for (hipEvent_t e : {walk_done, walk_fin, last_range, upper_done, prep_done}) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (walk_stream) (void)hipStreamDestroy(walk_stream);
    }
};

// The pseudo-root component of a collection with a metadata schema: pseudo nodes + Metadata replicas, a graph of
// its own next to the base graph.  Node table = level 0 of the component, ascending replica id.
struct MetaGraph {
    u32 mdim = 0;                 // metadata dimensions per node (0 = the index has no metadata schema)
    std::vector<u32> node_ids;    // [n_meta] ascending
    DevArr<int32_t> d_mbits;      // [n_meta][mdim]
    DevArr<float> d_mmags;        // [n_meta]
    std::vector<LevelHost> lv;    // [num_layers + 1]
    // What cos_index_build_meta leaves behind so that cos_index_append_meta can CONTINUE it (builder.hip): the link state of the component's
    // levels and how many nodes the schedule has inserted.  Freed by cos_index_release_link_state and with the levels (an uploaded
    // component has none).
    struct Link {
        LinkLevels lv;
        u32 inserted = 0; // nodes inserted so far: pseudo nodes without the pseudo root + Metadata replicas
        bool valid = false;
        void release() { lv.release(); inserted = 0; valid = false; }
    } link;
};

// Device-side resources of ONE host-API call in flight (cos_search_batch, cos_ann_search_batch, cos_search_filtered_batch):
// s[0] is the call's stream on the simple path; big batches run as a chunk pipeline (engine.hip, search_host_pipelined):
// H2D of chunk i+1 on `sc` under the walk of chunk i on s[i & 1], finalize of chunk i on `sf` under the walk of chunk i+1.
struct HostPipe {
    static constexpr u32 MAX_CHUNKS = 4;
    hipStream_t s[2] = {nullptr, nullptr}, sc = nullptr, sf = nullptr;
    hipEvent_t ev_in[MAX_CHUNKS] = {}, ev_walk[MAX_CHUNKS] = {};
    char wkey[MAX_CHUNKS] = {}; // &wkey[i] = key of chunk i's Workspace in cos_index::ws
    DevArr<float> d_q;          // [B][dim] the call's queries
    DevArr<u32> d_ids, d_counts;
    DevArr<float> d_scores;
    DevArr<int32_t> d_status;
    HostPipe() = default;
    HostPipe(const HostPipe &) = delete;
    ~HostPipe() {
        for (hipEvent_t e : ev_in) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_walk) if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : {s[0], s[1], sc, sf}) if (st) (void)hipStreamDestroy(st);
    }
};
static constexpr u32 COS_MAX_HOST_PIPES = 32; // concurrent host-API calls served at once; further callers wait for a pipe

// One operand of the level-table GEMM: the code rows, norms and code sums of the table's nodes ([cols][row_stride] / [cols] / [cols]),
// level by level from the top, the first column of every level, and floats per query row of the table computed from it (cols padded to
// 32).  A NESTED set (table_nested.h; key = the per-level set's | TABLE_KEY_NESTED) has one column per node of level_min, col0 all
// zero, and per table level the node -> column array and the node bits of LevelDev::adj_tab's words.
struct TableSet : cosdev::TableRule { // key, level_min, cols, col0
    u64 stride = 0;
    u32 node_bits[cosdev::MAX_LEVELS] = {};
    DevArr<uint8_t> tcodes;
    DevArr<float> tmags;
    DevArr<u32> tcsums, tab_col[cosdev::MAX_LEVELS];
};

// Everything a dense handle derives from its resident graph for the walk alone (walk_operands.hip builds and drops it, walk_operands.h
// decides; DESIGN.md §5.1 has the table of what follows what).  Only LevelHost::d_adj_mag / d_adj_up / d_adj_tab live with their level.
// Guarded by cos_index::mu; only cos_graph_changed invalidates.
struct WalkOperands {
    // the order keys' tables: position of every node of a key level in a depth-first order of that level's graph, and the key
    // levels themselves, descending (empty = the graph has no level the order could use)
    DevArr<u32> d_order_rank[cosdev::MAX_LEVELS];
    std::vector<u32> order_levels;
    // the table sets of the current graph, one per key: ef_search changes re-select the table's levels while searches of the previous
    // ef may still be in flight, so nothing a launch may be reading is freed before the graph itself is replaced.  table_idx: the
    // per-level set of the current key; nested_idx: the nested set of the same levels that the throughput kernel's launches use, with
    // LevelHost::d_adj_tab filled for it (-1 = none: knob, rule, a graph whose words do not fit, out of memory)
    std::vector<TableSet> table_sets;
    int table_idx = -1, nested_idx = -1;
    // key of `table`: table_rule's; of `nested` and `adj_tab`: that | TABLE_KEY_NESTED; of `adj_up`: the level that holds the filled
    // array (always the table's level_min - 1), | ADJ_UP_NESTED where its entries hold columns of the nested table, not node indices.
    // `nested` only remembers "went without" (a built nested set is found in table_sets by its key); `table` is settled for a key with
    // or without a set (table_idx says which)
    cosdev::OperandState rank{cosdev::FOLLOWS_LEVELS}, table{cosdev::FOLLOWS_ROOT}, nested{cosdev::FOLLOWS_ROOT};
    cosdev::OperandState adj_mag{cosdev::FOLLOWS_ADJACENCY}, adj_up{cosdev::FOLLOWS_ADJACENCY}, adj_tab{cosdev::FOLLOWS_ADJACENCY};
    static constexpr u64 ADJ_UP_NESTED = 1ull << 32;
    const TableSet *table_set() const { return table_idx >= 0 ? &table_sets[(size_t)table_idx] : nullptr; }
    const TableSet *nested_set() const { return nested_idx >= 0 ? &table_sets[(size_t)nested_idx] : nullptr; }
    bool have_adj_mag() const { return adj_mag.kind == cosdev::OperandState::BUILT; }
    u32 adj_up_level() const { return adj_up.kind == cosdev::OperandState::BUILT ? (u32)adj_up.key : 0u; } // 0 = no level has LevelHost::d_adj_up
    bool adj_up_nested() const { return adj_up_level() != 0u && (adj_up.key & ADJ_UP_NESTED) != 0; }
    void drop_tables() { table.invalidate(); nested.invalidate(); adj_tab.invalidate(); table_idx = nested_idx = -1; }
};

struct cos_index {
    cos_params p;
    int eng = -1;
    u32 n = 0;
    bool have_vectors = false, have_root = false;
    const float *d_raw = nullptr; // the f32 table the kernels read: raw_own, or the caller's (COS_UPLOAD_BORROW_DEVICE)
    DevArr<float> raw_own;        // empty while the table is borrowed
    DevArr<float> d_raw_mags;
    DevArr<uint8_t> d_codes;
    DevArr<float> d_mags;
    DevArr<u32> d_deleted;        // [ceil(n / 32)] the deleted set: bit (r % 32) of word r / 32 = row r was given to cos_index_delete (kernels_flat.hip)
    u64 row_stride = 0;
    u32 nchunks = 0, G = 1;
    std::vector<float> root_raw;
    std::vector<LevelHost> lv;
    u32 id_stride = 1; // internal id of vector row r = r * id_stride (max_replica_per_node with a metadata schema, else 1)
    MetaGraph meta;
    hipStream_t own_stream = nullptr; // uploads / builder stream (exclusive entry points)
    std::mutex mu;                    // guards the workspace + thread-stream maps, the timing flag, ef_search and visited_mode
    std::map<void *, std::unique_ptr<Workspace>> ws;
    // host-API searches: a call leases one HostPipe (private streams + staging) for its duration from a bounded pool, so
    // concurrent callers neither serialise nor share buffers and a host that churns threads cannot grow device memory
    std::mutex pipe_mu;
    std::condition_variable pipe_cv;
    std::vector<std::unique_ptr<HostPipe>> pipes_all;
    std::vector<HostPipe *> pipes_free;
    std::atomic<int> host_calls_active{0};
    Workspace *last_ws = nullptr; // most recent batch (cos_index_last_stats with stream == NULL)
    // host-API request coalescing (cos_index_set_coalescing)
    std::mutex co_mu;
    std::condition_variable co_cv;
    std::vector<struct CoSlot *> co_slots; // pooled launches-in-assembly (engine.hip, CoSlot)
    struct CoSlot *co_open = nullptr;      // the slot new requests join
    u32 co_max_queries = 0, co_window_us = 0;
    u32 co_inflight = 0;                  // coalesced launches issued and not yet complete (co_mu)
    cos_coalescing_stats co_stats{};      // since the last cos_index_set_coalescing (co_mu)
    bool timing = false;
    // Walk chain: a launch big enough to fill the chip several times over (>= chain_min_B queries) gains nothing from sharing
    // it with ANOTHER stream's walk — two co-running walks only stretch each other — but its prologue/epilogue (quantize,
    // finalize: short kernels) do hide well under a neighbour's walk.  So big walks of different streams are ordered one after
    // the other with an event, while everything else of a launch stays free to overlap.
    std::mutex chain_mu;
    hipEvent_t chain_ev = nullptr; // walk_done of the most recent chained walk
    // ... and its last_range: the next launch's level-table GEMM waits for it.  Issued freely on the caller's stream the GEMM lands
    // next to the previous walk's UPPER range and order sort — and the sort's first kernel (32 workgroups) cannot be placed while the
    // GEMM's 450-register waves hold every SIMD: the chip ran the GEMM alone for 3 ms per step and the lower range waited
    // (profiles/r06_step_timeline_before.txt).  Behind this event the GEMM shares the chip with the HBM-bound lower range instead.
    hipEvent_t chain_last_range_ev = nullptr;
    // ... and its upper_done (round 7): between the upper range and the order sort the chip is empty for ~60 us.  The EARLY part of the
    // next launch's GEMM (WalkPlan::table_early_wgs workgroups; 0 by default) waits for this event, the LATE part for chain_ev (walk_plan.h).
    hipEvent_t chain_upper_ev = nullptr;
    // (Round 5 also chained the two level ranges of a split walk separately, so that the upper range of launch i+1 — table levels,
    // instruction issue — co-ran with the lower range of launch i — HBM.  Measured: 7.08 against 7.12 ms per step at ef 64, 17.34
    // against 17.27 at ef 256 (profiles/r05_phase_chain_probe.jsonl): both ranges are limited by the queries in flight, and two
    // co-running ranges share the wave slots.  Removed.)
    u32 chain_min_B = 16384;
    // launches of at least this many queries split their walk in two (upper levels | level 0) and run level 0 in locality order
    // (kernels_order.hip); 0 = never.  Env COS_WALK_ORDER_MIN_B.
    u32 walk_order_min_B = COS_WALK_ORDER_DEFAULT_MIN_B;
    u32 n_cus = 256; // hipDeviceAttributeMultiprocessorCount of the handle's device (persistent kernels launch one workgroup per CU)
    u32 num_xcd = 8; // hipDeviceAttributeNumberOfXccs of the handle's device (workgroup b of a grid runs on XCD b % num_xcd)
    // Level table (WalkArgs::tab): launches of at least walk_table_min_B queries over u8 codes precompute the similarities to every
    // node of the levels >= the table's level_min with one i8 MFMA GEMM; walk_table_max_cols picks the levels (walk_operands.h,
    // table_rule; 0 = no table).  Env COS_WALK_TABLE_COLS / COS_WALK_TABLE_MIN_B.
    u32 walk_table_max_cols = COS_WALK_TABLE_AUTO, walk_table_min_B = COS_WALK_TABLE_DEFAULT_MIN_B;
    size_t table_bytes_total = 0;    // tables held by this handle's workspaces (budget: get_workspace)
    WalkOperands ops;                // what the walk derives from the resident graph (walk_operands.hip; cos_graph_changed invalidates)
    LinkState link;                  // cos_index_build -> cos_index_append (builder.hip); dropped with the graph
    u32 walk_side_min_B = 4096; // launches of at least this many queries walk on the workspace's low-priority stream; 0 = never
    // launches of at most this many queries run the latency variant of the walk (kernels_walk_lat.hip) where it applies; 0 = never
    u32 lat_max_B = COS_LATENCY_MODE_DEFAULT_MAX_B;
    // ... and the smallest of them (one client batch) give every query four waves (kernels_walk_lat4.hip); 0 = never
    u32 lat4_max_B = COS_LATENCY_WAVES_DEFAULT_MAX_B;
    struct FlatWs *flat_ws = nullptr; // cos_flat_search_batch's buffers (kernels_flat.hip), created on first use under `mu`
    cos_brute_stats brute_last = {(u32)sizeof(cos_brute_stats), 0u, 0u, 0u}; // the last brute force of this handle (cos_index_last_brute_stats)
};


struct FlatWs;
void cos_flat_ws_release(cos_index *ix);
namespace cosdev {
// The single-index searches as one shard of a shard set runs them (shardset.hip): the operator's own kernels, refusals and zero-norm rule;
// the packed record [ids B*k | scores B*k | counts B] is left in d_record (device memory on the index's device, B * (2k + 1) words) and is
// complete when the call returns.  kernels_flat.hip (the first two), engine.hip.
int32_t flat_search_record(cos_index *ix, const float *queries, u32 B, u32 top_k, const cos_scan_mask *mask, u32 *d_record);
int32_t bruteforce_record(cos_index *ix, const float *queries, u32 B, u32 k, const cos_scan_mask *mask, u32 *d_record);
int32_t search_filtered_record(cos_index *ix, const float *queries, u32 B, const u32 *filter_offsets, const int8_t *filter_dims, u32 top_k, u32 *d_record);
} // namespace cosdev
// the deleted set (kernels_flat.hip), on `st`: a fresh all-live bitmap for n rows | grown from n0 to n1 rows, the new ones live | ids marked
hipError_t cos_deleted_reset(cos_index *ix, u32 n, hipStream_t st);
hipError_t cos_deleted_grow(cos_index *ix, u32 n0, u32 n1, hipStream_t st);
hipError_t cos_deleted_mark(cos_index *ix, const u32 *ids, u32 m, hipStream_t st);
void cos_coalesce_release(cos_index *ix);
cosdev::IndexDev cos_make_index_dev(const cos_index *ix);
cosdev::IndexDev cos_make_meta_dev(const cos_index *ix);
int32_t cos_set_device(const cos_index *ix);
// the walk's operands (walk_operands.hip); the caller holds ix->mu, cos_prepare_walk_plans takes it
inline bool cos_graph_ready(const cos_index *ix) {
    if (!ix->have_vectors || !ix->have_root) return false;
    for (auto &l : ix->lv) if (l.n == 0) return false;
    return true;
}
void cos_graph_changed(cos_index *ix, cosdev::GraphChange change); // the ONLY call that invalidates them
cosdev::WalkPlanIn cos_walk_plan_in(const cos_index *ix, u32 B, u32 ef); // the handle's shape and resolved knobs as walk_plan's inputs
u32 cos_walk_table_min_B(const cos_index *ix);   // cos_index_set_walk_table's min_queries after its override
int32_t cos_ensure_adj_mags(cos_index *ix);      // LevelHost::d_adj_mag of every level
int32_t cos_ensure_order_rank(cos_index *ix);    // order ranks
int32_t cos_ensure_level_table(cos_index *ix);   // per-level and nested table sets of the current key, LevelHost::d_adj_tab
int32_t cos_ensure_adj_up(cos_index *ix);        // LevelHost::d_adj_up of the level under the table (after cos_ensure_level_table)
int32_t cos_prepare_walk_plans(cos_index *ix);   // all of them, for a freshly committed graph
// An operand that is an optimisation and does not fit the device's memory: *without = true, the error is cleared, COS_OK (the caller goes
// without: same results); every other error is reported as HIP_TRY reports it
int32_t cos_or_go_without(hipError_t e, bool *without);
void cos_meta_free_levels(cos_index *ix); // device arrays + host lists of every level of the pseudo-root component
