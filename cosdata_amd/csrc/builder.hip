// builder.hip — vector_store::index_embeddings (vector_store.rs:714-1109) for a device-resident index.
//
// Batch-synchronous construction, entirely on the device: the ids of a batch run the reference's per-level walk
// (traverse_find_nearest with ef_construction, keep 64, visited pre-seeded with the new id) against the graph snapshot
// that precedes the batch — one wavefront per new vector, the same walk kernel the search path uses — then their edges are
// connected with the reference's exact edge semantics (create_node_edges / ProbNode::add_neighbor: replace-lowest slot,
// bidirectional accept-or-rollback, evictee drops its back edge, stale lowest cache) by the round-synchronous link kernels
// of kernels_link.hip.  The host only does bookkeeping: level draws, node numbering, the round loop.
// oracle/cosdata_oracle_hnsw.c:coso_index_build_rounds (ordered variant) is the CPU statement of the same schedule; the
// tests assert the two graphs are identical.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "engine_internal.h"
#include "level_grow_plan.h"

using namespace cosdev;

namespace {

constexpr u32 NONE = 0xFFFFFFFFu;
static_assert(level_grow_plan::PSEUDO_LO == PSEUDO_LO && level_grow_plan::NONE == ROW_EMPTY, "level_grow_plan.h restates these");

inline uint64_t splitmix64(uint64_t &st) {
    uint64_t z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline float rand_f32(uint64_t &st) { return (float)(splitmix64(st) >> 40) * (1.0f / 16777216.0f); }

inline int32_t total_key(float v) {
    int32_t b;
    memcpy(&b, &v, 4);
    b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
    return b;
}
inline float metric_min(u32 metric) { return metric == COS_METRIC_COSINE ? -1.0f : -INFINITY; } // types.rs:435-446
inline float metric_max(u32 metric) { return metric == COS_METRIC_COSINE ? 2.0f : INFINITY; }   // types.rs:448-457
inline int32_t order_key(u32 metric, float v) {
    const int32_t k = total_key(v);
    return (metric == COS_METRIC_EUCLIDEAN || metric == COS_METRIC_HAMMING) ? ~k : k;
}

} // namespace

// ---- LinkLevels (engine_internal.h): the one place a level's link state is allocated, initialised and grown -------------------------
int32_t LinkLevels::alloc_level(u32 l, u32 nl, u32 M) {
    HIP_TRY(key[l].alloc((size_t)nl * M * 4));
    HIP_TRY(low_idx[l].alloc(nl));
    HIP_TRY(low_key[l].alloc((size_t)nl * 4));
    HIP_TRY(owner[l].alloc((size_t)nl * 4));
    kind[l].reset();
    return COS_OK;
}

int32_t LinkLevels::init_level(u32 l, u32 nl, u32 M, u32 metric, const uint8_t *kinds, hipStream_t st) {
    if (int32_t rc = alloc_level(l, nl, M)) return rc;
    HIP_TRY(launch_fill_i32(key[l].as<int32_t>(), (u64)nl * M, INT32_MIN, st));
    HIP_TRY(hipMemsetAsync(low_idx[l].p, 0, nl, st));
    HIP_TRY(launch_fill_i32(low_key[l].as<int32_t>(), nl, order_key(metric, metric_min(metric)), st));
    HIP_TRY(hipMemsetAsync(owner[l].p, 0, (size_t)nl * 4, st));
    if (kinds) {
        HIP_TRY(kind[l].alloc(nl));
        HIP_TRY(hipMemcpy(kind[l].p, kinds, nl, hipMemcpyHostToDevice));
    }
    return COS_OK;
}

int32_t LinkLevels::grow_level(u32 l, u32 old_n, u32 tail_first, u32 add, u32 M, u32 metric, LinkLevels &out, hipStream_t st) const {
    const u32 nl = old_n + add;
    const GrowValues as_is; // keys and caches are similarities, not indices
    if (int32_t rc = out.alloc_level(l, nl, M)) return rc;
    HIP_TRY(launch_grow_tail(key[l].as<u32>(), out.key[l].as<u32>(), old_n, tail_first, add, M, (u32)INT32_MIN, as_is, st));
    HIP_TRY(launch_grow_tail(low_key[l].as<u32>(), out.low_key[l].as<u32>(), old_n, tail_first, add, 1, (u32)order_key(metric, metric_min(metric)), as_is, st));
    HIP_TRY(launch_grow_tail_bytes(low_idx[l].as<uint8_t>(), out.low_idx[l].as<uint8_t>(), old_n, tail_first, add, 0, st));
    HIP_TRY(hipMemsetAsync(out.owner[l].p, 0, (size_t)nl * 4, st)); // a new tag epoch (run_link_schedule starts at round 1)
    if (kind[l].p) {
        HIP_TRY(out.kind[l].alloc(nl));
        HIP_TRY(launch_grow_tail_bytes(kind[l].as<uint8_t>(), out.kind[l].as<uint8_t>(), old_n, tail_first, add, 2, st)); // every new node is a Metadata replica
    }
    return COS_OK;
}

namespace {

// generate_level_probs(4.0, L): 1 - 4^-n, n = L..0 (common.rs:421-429), and get_max_insert_level (common.rs:373-379) for one draw
std::vector<double> level_probs(u32 Ltop) {
    std::vector<double> pv(Ltop + 1);
    for (u32 k = 0; k <= Ltop; k++) {
        const int nn = (int)(Ltop - k);
        double r = 1.0, a = 4.0;
        for (int b = nn;;) { if (b & 1) r *= a; b /= 2; if (b == 0) break; a *= a; }
        pv[k] = 1.0 - 1.0 / r;
    }
    return pv;
}
inline uint8_t draw_level(uint64_t &rng, const std::vector<double> &pv, u32 Ltop) {
    const double x = (double)rand_f32(rng);
    u32 k = 0;
    while (k < Ltop && !(x >= pv[k])) k++;
    return (uint8_t)(Ltop - k);
}

// a failed build / append leaves the handle WITHOUT a graph (search returns NotReady) instead of a half-linked one
struct GraphGuard {
    cos_index *ix;
    bool armed = true;
    ~GraphGuard() {
        if (!armed) return;
        (void)hipStreamSynchronize(ix->own_stream);
        for (auto &l : ix->lv) l.release();
        ix->link.release();
        cos_graph_changed(ix, GraphChange::ADJACENCY);
        ix->have_root = false;
    }
};

// The batch size of a build or an append: the caller's or the graph's default, within what a claim tag's 13-bit batch position holds.
// The component's default is 1024 (the base graph's: 4096): every Metadata replica links to the same few pseudo nodes, the rounds of a
// batch run ~1.4 nodes each whatever its size, and a round costs what its PENDING list costs — 600 k nodes: 27 s at 4096, 16.4 s at
// 1024 or 256
constexpr u32 BASE_DEFAULT_BATCH = 4096u, COMPONENT_DEFAULT_BATCH = 1024u;
inline u32 batch_max(u32 batch_size, u32 graph_default) { return std::min<u32>(batch_size ? batch_size : graph_default, LINK_MAX_BATCH); }

// LinkArgs over a graph's level arrays and link state, base graph and component alike.  Level 0 of the base graph keeps neither a
// node-index adjacency nor a node -> vector row array (there a node index IS the vector row): adj_node = adj_vec, node_vec = nullptr.
// `kind` is the component's (nullptr on the base graph).
void fill_link_levels(const std::vector<LevelHost> &lv, const LinkLevels &ls, LinkArgs &la, u32 &maxM) {
    maxM = 0;
    for (u32 l = 0; l < (u32)lv.size(); l++) {
        const LevelHost &H = lv[l];
        LinkLevelDev &D = la.lv[l];
        D.adj_vec = H.d_adj_vec;
        D.adj_node = H.d_adj_node.p ? H.d_adj_node.p : H.d_adj_vec.p;
        D.node_vec = H.d_node_vec;
        D.key = ls.key[l].as<int32_t>();
        D.low_idx = ls.low_idx[l].as<uint8_t>();
        D.low_key = ls.low_key[l].as<int32_t>();
        D.owner = ls.owner[l].as<u32>();
        D.kind = ls.kind[l].as<uint8_t>();
        D.M = H.M;
        maxM = std::max(maxM, H.M);
    }
}

// ---- the link schedule of both graphs -----------------------------------------------------------------------------------------------
// What a graph tells the schedule about itself ...
struct LinkSchedule {
    const char *graph;          // which graph, for the build_profile line
    std::vector<LevelHost> &lv; // its levels: they already hold every item of the call (all slots empty, claim tags zero: a new tag epoch)
    LinkLevels &link;           // ... and their link state
    u32 first, count;           // items the schedule had inserted before this call (the batch-size rule continues there) | items of this call
    u32 md;                     // filter columns per item (0: the walk takes no filter)
    u32 Bmax;
};
// ... and what its `item` callback writes for item i of the call, into the batch's staging
struct BatchSlot {
    u32 &row, &self_id; // the walk's query: a vector row, and the id pre-inserted in its visited filter (vector_store.rs:807)
    u32 *me;            // [levels] the item's node index on every level it reaches; preset NONE
    int32_t *fdims;     // [md] the query's filter columns ...
    float &fmag;        // ... and their norm
};

// index_embeddings' batch loop: batches of min(Bmax, max(1, inserted / 4), left) items run the reference walk against the snapshot that
// precedes the batch, then the round-synchronous link kernels (kernels_link.hip) connect them.
//   item(i, BatchSlot)        fills the slot of item i, 0 <= i < count
//   walk(WalkArgs &, stream)  launches the graph's insertion walk for a batch: queries, outputs, ef and keep are set
//   fail(i, status)           -> cos_fail for item i, whose walk reported `status`
template <typename Item, typename Walk, typename Fail>
int32_t run_link_schedule(cos_index *ix, const LinkSchedule &s, Item item, Walk walk, Fail fail) {
    const u32 L1 = (u32)s.lv.size(), metric = ix->p.metric, md = s.md, Bmax = s.Bmax, total = s.first + s.count;
    hipStream_t st = ix->own_stream;
    LinkArgs la;
    memset(&la, 0, sizeof(la));
    u32 maxM = 0;
    fill_link_levels(s.lv, s.link, la, maxM);
    if (maxM > 256) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 256 neighbour slots per node");

    // ---- batch workspace (device) + pinned staging: a batch's staging is rewritten only after the synchronisation that ends the
    //      previous batch's round loop, so every upload runs asynchronously
    const u32 KEEP = (u32)KEEP_INDEX;
    DevBuf d_rows, d_self, d_foff, d_fdims, d_fmags, d_out_ids, d_out_nodes, d_out_sims, d_out_counts, d_status, d_me, d_pend[2], d_cnt, d_evq;
    PinArr<u32> h_rows, h_self, h_foff, h_me, h_pend, h_cnt;
    PinArr<int32_t> h_fdims, h_status;
    PinArr<float> h_fmags;
    const size_t pend_cap = (size_t)Bmax * L1;              // (level, batch position) entries
    const size_t evq_cap = pend_cap * 2 * KEEP;             // a node queues at most 2 evictions per candidate
    HIP_TRY(d_rows.alloc((size_t)Bmax * 4));
    HIP_TRY(d_self.alloc((size_t)Bmax * 4));
    HIP_TRY(d_out_ids.alloc((size_t)Bmax * L1 * KEEP * 4));
    HIP_TRY(d_out_nodes.alloc((size_t)Bmax * L1 * KEEP * 4));
    HIP_TRY(d_out_sims.alloc((size_t)Bmax * L1 * KEEP * 4));
    HIP_TRY(d_out_counts.alloc((size_t)Bmax * L1 * 4));
    HIP_TRY(d_status.alloc((size_t)Bmax * 4));
    HIP_TRY(d_me.alloc((size_t)Bmax * L1 * 4));
    HIP_TRY(d_pend[0].alloc(pend_cap * 4));
    HIP_TRY(d_pend[1].alloc(pend_cap * 4));
    HIP_TRY(d_cnt.alloc(4 * 4));                            // [0], [1]: pending counters (ping-pong); [2]: eviction queue length
    HIP_TRY(d_evq.alloc(evq_cap * 3 * 4));
    HIP_TRY(h_rows.alloc(Bmax));
    HIP_TRY(h_self.alloc(Bmax));
    HIP_TRY(h_me.alloc((size_t)Bmax * L1));
    HIP_TRY(h_pend.alloc(pend_cap));
    HIP_TRY(h_status.alloc(Bmax));
    HIP_TRY(h_cnt.alloc(4));
    HIP_TRY(h_fdims.alloc((size_t)Bmax * md));
    HIP_TRY(h_fmags.alloc(Bmax));
    if (md) { // one filter per query: its offsets are 0, 1, 2, ... whatever the batch
        HIP_TRY(d_foff.alloc(((size_t)Bmax + 1) * 4));
        HIP_TRY(d_fdims.alloc((size_t)Bmax * md * 4));
        HIP_TRY(d_fmags.alloc((size_t)Bmax * 4));
        HIP_TRY(h_foff.alloc((size_t)Bmax + 1));
        for (u32 b = 0; b <= Bmax; b++) h_foff[b] = b;
        HIP_TRY(hipMemcpyAsync(d_foff.p, h_foff.p, ((size_t)Bmax + 1) * 4, hipMemcpyHostToDevice, st));
    }

    la.L1 = L1;
    la.z_nodes = d_out_nodes.as<u32>();
    la.z_sims = d_out_sims.as<float>();
    la.z_counts = d_out_counts.as<u32>();
    la.me = d_me.as<u32>();
    la.metric = metric;
    la.kmin = order_key(metric, metric_min(metric));
    la.kmax = order_key(metric, metric_max(metric));

    u32 inserted = s.first, round = 0;
    u64 n_rounds = 0, n_batches = 0;
    const bool prof = cosdev::tune_or(cosdev::TUNE_BUILD_PROFILE, 0) != 0;
    double t_walk = 0, t_link = 0;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    u32 *cnt = d_cnt.as<u32>();
    while (inserted < total) {
        const double t0 = now();
        n_batches++;
        const u32 bs = std::min({Bmax, std::max(1u, inserted / 4u), total - inserted});
        // batch bookkeeping: the walks' queries, node index of every (batch item, level), initial pending list (all levels together)
        u32 np = 0;
        for (u32 b = 0; b < bs; b++) {
            u32 *me = h_me.p + (size_t)b * L1;
            std::fill(me, me + L1, NONE);
            item(inserted - s.first + b, BatchSlot{h_rows[b], h_self[b], me, h_fdims.p + (size_t)b * md, h_fmags[b]});
            for (u32 l = 0; l < L1; l++)
                if (me[l] != NONE) h_pend[np++] = (l << 16) | b;
        }
        HIP_TRY(hipMemcpyAsync(d_rows.p, h_rows.p, (size_t)bs * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_self.p, h_self.p, (size_t)bs * 4, hipMemcpyHostToDevice, st));
        if (md) {
            HIP_TRY(hipMemcpyAsync(d_fdims.p, h_fdims.p, (size_t)bs * md * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_fmags.p, h_fmags.p, (size_t)bs * 4, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(d_me.p, h_me.p, (size_t)bs * L1 * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_pend[0].p, h_pend.p, (size_t)np * 4, hipMemcpyHostToDevice, st));
        h_cnt[0] = np; h_cnt[1] = 0; h_cnt[2] = 0; h_cnt[3] = 0;
        HIP_TRY(hipMemcpyAsync(cnt, h_cnt.p, 16, hipMemcpyHostToDevice, st));
        // 1. the reference walk of every item against the snapshot that precedes the batch (one wave each)
        WalkArgs wa;
        memset(&wa, 0, sizeof(wa));
        wa.qcodes = ix->d_codes;
        wa.qmags = ix->d_mags;
        wa.q_rows = d_rows.as<u32>();
        wa.self_ids = d_self.as<u32>();
        wa.B = bs;
        wa.ef = ix->p.ef_construction;
        wa.keep = KEEP;
        wa.out_ids = d_out_ids.as<u32>();
        wa.out_sims = d_out_sims.as<float>();
        wa.out_nodes = d_out_nodes.as<u32>();
        wa.out_counts = d_out_counts.as<u32>();
        wa.out_status = d_status.as<int32_t>();
        if (md) {
            wa.f_dims = d_fdims.as<int32_t>();
            wa.f_mags = d_fmags.as<float>();
            wa.f_off = d_foff.as<u32>();
        }
        if (int32_t wrc = walk(wa, st)) return wrc;
        HIP_TRY(hipMemcpyAsync(h_status.p, d_status.p, (size_t)bs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st)); // a failed walk leaves its lower levels unwritten: never link from it
        for (u32 b = 0; b < bs; b++)
            if (h_status[b] != COS_OK) return fail(inserted - s.first + b, h_status[b]);
        t_walk += now() - t0;
        const double t1 = now();
        // 2. link rounds (kernels_link.hip).  Rounds are enqueued a few at a time; each reads the true pending count on the
        // device, so over-launching costs nothing but empty blocks.
        u32 pending_ub = np, cur = 0;
        while (pending_ub > 0) {
            const u32 chunk = pending_ub > 64 ? 2 : 4;
            for (u32 r = 0; r < chunk; r++) {
                if (++round > LINK_MAX_ROUND) { // claim tags would wrap: start a new tag epoch
                    for (u32 l = 0; l < L1; l++) HIP_TRY(hipMemsetAsync(s.link.owner[l].p, 0, (size_t)s.lv[l].n * 4, st));
                    round = 1;
                }
                HIP_TRY(launch_link_round(la, maxM, d_pend[cur].as<u32>(), cnt + cur, d_pend[cur ^ 1].as<u32>(), cnt + (cur ^ 1), d_evq.as<u32>(), cnt + 2,
                                          pending_ub, round, st));
                cur ^= 1;
                n_rounds++;
            }
            HIP_TRY(hipMemcpyAsync(h_cnt.p, cnt, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            pending_ub = h_cnt[cur]; // the list the next round would read
        }
        t_link += now() - t1;
        inserted += bs;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (prof)
        fprintf(stderr, "[cos_index_build] %s: items [%u, %u) batches=%llu link rounds=%llu walk %.2fs link %.2fs\n", s.graph, s.first, total,
                (unsigned long long)n_batches, (unsigned long long)n_rounds, t_walk, t_link);
    return COS_OK;
}

// The base graph's items are the vectors [first, ix->n): max_level is indexed by vector row - first; cursor[l] = the node index the next
// inserted vector takes on level l (nodes are in id order, the root last).
int32_t link_vectors(cos_index *ix, u32 first, const uint8_t *max_level, std::vector<u32> &cursor, u32 Bmax) {
    IndexDev dev = cos_make_index_dev(ix);
    VisTab vtab; // EXACT build mode: visited filters of the batch walks
    const LinkSchedule s{"base graph", ix->lv, ix->link.lv, first, ix->n - first, 0u, Bmax};
    return run_link_schedule(
        ix, s,
        [&](u32 i, BatchSlot o) {
            o.row = o.self_id = first + i;
            for (u32 l = 0; l <= max_level[i]; l++) o.me[l] = cursor[l]++;
        },
        [&](WalkArgs &wa, hipStream_t st) -> int32_t {
            if (dev.visited_mode == COS_VISITED_EXACT) {
                const int32_t vrc = vis_tab_prepare(vtab, ix, Bmax, wa.ef, st, wa);
                if (vrc) return vrc;
            }
            cosdev::WalkPlanIn pin = cos_walk_plan_in(ix, wa.B, wa.ef); // the handle's latency knobs; an insertion walk has no table and no order
            pin.table_min_B = pin.order_min_B = 0;
            HIP_TRY(launch_walk(ix->eng, dev, wa, cosdev::walk_plan(pin).kernel, st));
            return COS_OK;
        },
        [&](u32 i, int32_t status) { return cos_fail(status, "vector %u cannot be indexed (zero norm -> DistanceError::CalculationError)", first + i); });
}


// ---- the pseudo-root component of a collection with a metadata schema (cos_index_build_meta, cos_index_append_meta below) ----
// a failed build / growth leaves the handle WITHOUT the component (filtered search: NotReady) instead of a half-linked one
struct MetaGuard {
    cos_index *ix;
    bool armed = true;
    ~MetaGuard() { if (armed) { (void)hipStreamSynchronize(ix->own_stream); cos_meta_free_levels(ix); } }
};

// Metadata::from (types.rs:112-126) for rows of the node table: the norm of the metadata dimensions (sqrt of the sequential sum of
// squares) and the ReplicaNodeKind — 0 Base (all dimensions zero: the node lives under the main root, not here), 1 Pseudo, 2 Metadata
void meta_row_kinds(u32 n_nodes, const u32 *node_ids, const int32_t *mbits, u32 md, std::vector<float> &mmag, std::vector<uint8_t> &kind) {
    mmag.resize(n_nodes);
    kind.resize(n_nodes);
    for (u32 i = 0; i < n_nodes; i++) {
        float acc = -0.0f;
        for (u32 j = 0; j < md; j++) { const float x = (float)mbits[(size_t)i * md + j]; acc = acc + x * x; }
        mmag[i] = sqrtf(acc);
        kind[i] = mmag[i] == 0.0f ? 0 : (is_pseudo(node_ids[i]) ? 1 : 2);
    }
}

// The component's items are the nodes ord[0], ord[1], ... (positions in the caller's node_ids / mbits / mmag / max_levels), inserted by the
// schedule CONTINUED at ix->meta.link.inserted.  A node walks from the pseudo root with its OWN metadata dimensions as the query's filter
// (walk_meta_kernel<.., INDEXING>); its node index on a level is its place in the level's ascending id list.
int32_t link_component_nodes(cos_index *ix, const u32 *node_ids, const int32_t *mbits, const float *mmag, const uint8_t *max_levels, const std::vector<u32> &ord, u32 Bmax) {
    const u32 n = ix->n, md = ix->meta.mdim;
    IndexDev dev = cos_make_meta_dev(ix);
    dev.visited_mode = COS_VISITED_REF;
    const LinkSchedule s{"metadata component", ix->meta.lv, ix->meta.link.lv, ix->meta.link.inserted, (u32)ord.size(), md, Bmax};
    const int32_t rc = run_link_schedule(
        ix, s,
        [&](u32 i, BatchSlot o) {
            const u32 t = ord[i], id = node_ids[t];
            o.row = is_pseudo(id) ? n + 1 : id / ix->id_stride;
            o.self_id = id;
            std::copy(mbits + (size_t)t * md, mbits + (size_t)(t + 1) * md, o.fdims);
            o.fmag = mmag[t];
            for (u32 l = 0; l <= max_levels[t]; l++) {
                const std::vector<u32> &ids = ix->meta.lv[l].node_ids;
                o.me[l] = (u32)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin());
            }
        },
        [&](WalkArgs &wa, hipStream_t st) -> int32_t {
            HIP_TRY(launch_walk_meta_index(ix->eng, dev, wa, st));
            return COS_OK;
        },
        [&](u32 i, int32_t status) { return cos_fail(status, "node %u of the metadata component cannot be indexed (status %d)", node_ids[ord[i]], status); });
    if (rc) return rc;
    ix->meta.link.inserted += (u32)ord.size();
    return COS_OK;
}

// cos_index_append on a collection with a metadata schema: the pseudo nodes' vector moved from row n0 + 1 to row n1 + 1, and every level
// of the resident pseudo-root component names it in d_node_vec and d_adj_vec (the component keeps no adjacency-side norms:
// walk_meta_kernel gathers mags[], which moved with the row).  Nothing else of the component changes — node indices, ids, link state —
// so filtered search answers as before over the old replicas.  A failure drops the component.
int32_t meta_follow_vector_growth(cos_index *ix, u32 n0, u32 n1) {
    hipStream_t st = ix->own_stream;
    MetaGuard guard{ix};
    GrowValues v;
    v.remap_from = n0 + 1;
    v.remap_to = n1 + 1;
    for (LevelHost &H : ix->meta.lv) {
        if (H.n == 0) continue;
        DevArr<u32> adj_vec, node_vec;
        HIP_TRY(adj_vec.alloc((size_t)H.n * H.M));
        HIP_TRY(node_vec.alloc(H.n));
        HIP_TRY(launch_grow_tail(H.d_adj_vec, adj_vec, H.n, H.n, 0, H.M, ROW_EMPTY, v, st));
        HIP_TRY(launch_grow_tail(H.d_node_vec, node_vec, H.n, H.n, 0, 1, ROW_EMPTY, v, st));
        HIP_TRY(hipStreamSynchronize(st));
        adj_vec.swap(H.d_adj_vec);
        node_vec.swap(H.d_node_vec);
    }
    guard.armed = false;
    return COS_OK;
}

} // namespace

extern "C" int32_t cos_index_build(cos_index *ix, uint32_t batch_size) {
    if (!ix) return cos_fail(COS_ERR_INVALID, "null index");
    if (!ix->have_vectors) return cos_fail(COS_ERR_NOT_READY, "upload vectors before building");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 n = ix->n, Ltop = ix->p.num_layers, metric = ix->p.metric;
    const u32 Bmax = batch_max(batch_size, BASE_DEFAULT_BATCH);
    hipStream_t st = ix->own_stream;
    GraphGuard guard{ix};

    cos_graph_changed(ix, GraphChange::LEVELS); // (the builder's walks gather mags[]; the adjacency-side norms are written when the graph is committed)
    ix->link.release();
    // ---- root + level draws (same RNG stream as the oracle builders) ----------------------------
    uint64_t rng = ix->p.seed ? ix->p.seed : 0x1234567ull;
    std::vector<float> root(ix->p.dim);
    for (u32 i = 0; i < ix->p.dim; i++) root[i] = ix->p.range_lo + rand_f32(rng) * (ix->p.range_hi - ix->p.range_lo); // vector_store.rs:30-36
    rc = cos_index_set_root(ix, root.data());
    if (rc) return rc;
    const std::vector<double> pv = level_probs(Ltop);
    std::vector<uint8_t> max_level(n);
    for (u32 id = 0; id < n; id++) max_level[id] = draw_level(rng, pv, Ltop);

    // ---- level skeletons: nodes of a level in ascending id, root last; every slot empty ------------------------
    for (u32 l = 0; l <= Ltop; l++) {
        LevelHost &H = ix->lv[l];
        H.release();
        for (u32 id = 0; id < n; id++)
            if (max_level[id] >= l) H.node_ids.push_back(id * ix->id_stride); // internal id of vector row `id`
        H.node_ids.push_back(COS_ROOT_ID);
        const u32 nl = (u32)H.node_ids.size(), M = H.M;
        if (M > 256) return cos_fail(COS_ERR_UNIMPLEMENTED, "more than 256 neighbour slots per node");
        HIP_TRY(H.d_adj_vec.alloc((size_t)nl * M));
        HIP_TRY(hipMemsetAsync(H.d_adj_vec, 0xFF, (size_t)nl * M * 4, st));
        if (l > 0) {
            std::vector<u32> node_vec(nl), child(nl);
            const std::vector<u32> &D = ix->lv[l - 1].node_ids;
            for (u32 i = 0; i < nl; i++) {
                node_vec[i] = H.node_ids[i] == COS_ROOT_ID ? n : H.node_ids[i] / ix->id_stride;
                child[i] = (u32)(std::lower_bound(D.begin(), D.end(), H.node_ids[i]) - D.begin()); // same id one level down (vector_store.rs:897-903)
            }
            HIP_TRY(H.d_adj_node.alloc((size_t)nl * M));
            HIP_TRY(hipMemsetAsync(H.d_adj_node, 0xFF, (size_t)nl * M * 4, st));
            HIP_TRY(H.d_node_vec.alloc(nl));
            HIP_TRY(hipMemcpy(H.d_node_vec, node_vec.data(), (size_t)nl * 4, hipMemcpyHostToDevice));
            HIP_TRY(H.d_child.alloc(nl));
            HIP_TRY(hipMemcpy(H.d_child, child.data(), (size_t)nl * 4, hipMemcpyHostToDevice));
        }
        H.n = nl;
        rc = ix->link.lv.init_level(l, nl, M, metric, nullptr, st);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));

    std::vector<u32> cursor(Ltop + 1, 0); // first node of each level not yet inserted (nodes are in id order)
    rc = link_vectors(ix, 0, max_level.data(), cursor, Bmax);
    if (rc) return rc;
    guard.armed = false;
    ix->link.rng = rng;
    ix->link.n_built = n;
    ix->link.valid = true;
    if (int32_t rc2 = cos_prepare_walk_plans(ix)) return rc2; // the walk's operands of the new graph (walk_operands.hip), outside any search
    return COS_OK; // the id-format host copy is made on demand (cos_index_download_graph_level)
}

// The link state of an UPLOADED graph (cos_index_upload_graph_level, cos_index_load_reference_dir), as the reference has it after a
// reload: it persists every slot's similarity (serializer/hnsw/neighbors.rs:22-61) and recomputes a node's cached lowest slot when it
// deserializes the node (ProbNode::new_with_neighbors_and_versions, prob_node.rs:145-181).  Here the similarities are recomputed with
// the distance operator's kernel on the resident codes (the distance is symmetric in its bits), the caches follow the reload rule,
// and later appends draw their levels from the seed's stream advanced past the resident vectors (a graph built by the same-seed
// builder and uploaded continues with the draws a native build would make).  oracle: coso_index_restore_link_state.
extern "C" int32_t cos_index_restore_link_state(cos_index *ix) {
    if (!ix) return cos_fail(COS_ERR_INVALID, "null index");
    if (!ix->have_vectors || !ix->have_root) return cos_fail(COS_ERR_NOT_READY, "restore needs vectors, root and every graph level");
    for (auto &l : ix->lv) if (l.n == 0) return cos_fail(COS_ERR_NOT_READY, "restore needs vectors, root and every graph level");
    if (ix->id_stride != 1u || ix->meta.mdim != 0u) return cos_fail(COS_ERR_UNIMPLEMENTED, "link state of a collection with a metadata schema");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const u32 Ltop = ix->p.num_layers, metric = ix->p.metric;
    const int32_t kmin = order_key(metric, metric_min(metric)), kmax = order_key(metric, metric_max(metric));
    hipStream_t st = ix->own_stream;
    ix->link.release();
    struct Fail { cos_index *ix; bool armed = true; ~Fail() { if (armed) ix->link.release(); } } fail_guard{ix};
    constexpr u64 CHUNK_PAIRS = 1ull << 24; // 64 MB per pair array
    DevBuf px, py, sims, dst, d_fail;
    HIP_TRY(px.alloc(CHUNK_PAIRS * 4));
    HIP_TRY(py.alloc(CHUNK_PAIRS * 4));
    HIP_TRY(sims.alloc(CHUNK_PAIRS * 4));
    HIP_TRY(dst.alloc(CHUNK_PAIRS * 4));
    HIP_TRY(d_fail.alloc(4));
    HIP_TRY(hipMemsetAsync(d_fail.p, 0, 4, st));
    for (u32 l = 0; l <= Ltop; l++) {
        LevelHost &H = ix->lv[l];
        const u32 nl = H.n, M = H.M;
        rc = ix->link.lv.alloc_level(l, nl, M);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(ix->link.lv.owner[l].p, 0, (size_t)nl * 4, st));
        const u32 step = (u32)std::max<u64>(1, CHUNK_PAIRS / M);
        for (u32 n0 = 0; n0 < nl; n0 += step) {
            const u32 cn = std::min(step, nl - n0);
            HIP_TRY(launch_edge_pairs(H.d_adj_vec, l == 0 ? nullptr : H.d_node_vec, n0, cn, M, px.as<u32>(), py.as<u32>(), st));
            HIP_TRY(cosdev::launch_index_pair_distances(ix->eng, ix->d_codes, ix->d_mags, ix->row_stride, ix->nchunks, ix->p.dim, metric, px.as<u32>(), py.as<u32>(),
                                                       (u32)((u64)cn * M), sims.as<float>(), dst.as<int32_t>(), st));
            HIP_TRY(launch_edge_keys(H.d_adj_vec, sims.as<float>(), dst.as<int32_t>(), n0, cn, M, metric, ix->link.lv.key[l].as<int32_t>(), d_fail.as<int32_t>(), st));
        }
        HIP_TRY(launch_low_cache(H.d_adj_vec, ix->link.lv.key[l].as<int32_t>(), nl, M, kmin, kmax, ix->link.lv.low_idx[l].as<uint8_t>(), ix->link.lv.low_key[l].as<int32_t>(), st));
    }
    int32_t failed = 0;
    HIP_TRY(hipMemcpyAsync(&failed, d_fail.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (failed) return cos_fail(failed, "an edge of the uploaded graph has no similarity (zero norm -> DistanceError::CalculationError)");
    uint64_t rng = ix->p.seed ? ix->p.seed : 0x1234567ull;
    for (u64 i = 0; i < (u64)ix->p.dim + ix->n; i++) (void)rand_f32(rng); // the root's components, then one level draw per resident vector
    ix->link.rng = rng;
    ix->link.n_built = ix->n;
    ix->link.valid = true;
    fail_guard.armed = false;
    return COS_OK;
}

extern "C" int32_t cos_index_release_link_state(cos_index *ix) {
    if (!ix) return cos_fail(COS_ERR_INVALID, "null index");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ix->own_stream));
    ix->link.release();
    ix->meta.link.release(); // the pseudo-root component's (cos_index_build_meta): cos_index_append_meta then answers NotReady
    return COS_OK;
}

// vector_store::index_embeddings called AGAIN on a live index (vector_store.rs:714-780; index_embedding :782-975 per vector): m more
// vectors take the internal ids [n, n + m) (sequential: collection.rs:451-468) and are inserted into the resident graph by the
// schedule of cos_index_build CONTINUED at inserted = n — level draws from the same RNG stream, batches of min(batch, max(1,
// inserted / 4)) walking the snapshot that precedes them, the round-synchronous link kernels on the link state cos_index_build left
// (slot similarities and lowest caches of EVERY node: a new vector's back edges evict from old nodes' rows).  oracle/
// cosdata_oracle_hnsw.c: coso_index_append_vectors + coso_index_build_rounds_continue is the CPU statement; tests/test_gpu_append.py
// asserts identical graphs.  Exclusive like every graph change: no search in flight.
extern "C" int32_t cos_index_append(cos_index *ix, const float *raw, uint32_t m, uint32_t flags, uint32_t batch_size) {
    if (!ix || !raw || m == 0) return cos_fail(COS_ERR_INVALID, "null/empty vectors");
    if (!ix->have_vectors || !ix->have_root) return cos_fail(COS_ERR_NOT_READY, "append needs a built index");
    for (auto &l : ix->lv) if (l.n == 0) return cos_fail(COS_ERR_NOT_READY, "append needs a built index");
    if (!ix->link.valid || ix->link.n_built != ix->n)
        return cos_fail(COS_ERR_NOT_READY, "no link state to continue from: the graph was uploaded (not built by cos_index_build on this handle), its root "
                                           "was replaced, or cos_index_release_link_state freed it");
    if ((u64)ix->n + m >= 0xFFFFFFF0ull) return cos_fail(COS_ERR_INVALID, "too many vectors");
    if (ix->meta.mdim != 0u && (u64)ix->p.id_base + ((u64)ix->n + m) * ix->id_stride >= PSEUDO_LO)
        return cos_fail(COS_ERR_INVALID, "replica ids would run into the reserved id range");
    const bool borrow = (flags & COS_UPLOAD_BORROW_DEVICE) != 0;
    if (borrow != !ix->raw_own) // (an empty owner = the table is the caller's)
        return cos_fail(COS_ERR_INVALID, borrow ? "the index owns its raw rows: append host rows" : "the index borrows its raw rows: append with COS_UPLOAD_BORROW_DEVICE and the whole grown table");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 n0 = ix->n, n1 = n0 + m, Ltop = ix->p.num_layers, metric = ix->p.metric;
    const u32 Bmax = batch_max(batch_size, BASE_DEFAULT_BATCH);
    const u64 dim = ix->p.dim, rs = ix->row_stride;
    hipStream_t st = ix->own_stream;
    HIP_TRY(hipDeviceSynchronize()); // exclusive: whatever read the old arrays is done
    GraphGuard guard{ix};
    cos_graph_changed(ix, GraphChange::LEVELS);
    ix->link.valid = false; // until the append is complete
    cos_flat_ws_release(ix); // cached sums of the stored codes, scan buffers sized for the old corpus

    // ---- 1. the vector tables grow: rows [0, n0) stay, rows [n0, n1) are the new vectors, the root and the pseudo nodes' vector move behind them
    {
        DevArr<uint8_t> codes;
        DevArr<float> mags, raw_mags, new_raw;
        HIP_TRY(codes.alloc(((size_t)n1 + 2) * rs));
        HIP_TRY(mags.alloc((size_t)n1 + 2));
        HIP_TRY(raw_mags.alloc((size_t)n1 + 2));
        HIP_TRY(hipMemcpyAsync(codes, ix->d_codes, (size_t)n0 * rs, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(codes + (size_t)n1 * rs, ix->d_codes + (size_t)n0 * rs, 2 * rs, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(mags, ix->d_mags, (size_t)n0 * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(mags + n1, ix->d_mags + n0, 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(raw_mags, ix->d_raw_mags, (size_t)n0 * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync(raw_mags + n1, 0, 8, st));
        const float *new_rows;
        if (borrow) {
            new_rows = raw + (size_t)n0 * dim; // raw = the caller's whole grown table (device)
        } else {
            HIP_TRY(new_raw.alloc((size_t)n1 * dim));
            HIP_TRY(hipMemcpyAsync(new_raw, ix->d_raw, (size_t)n0 * dim * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(new_raw + (size_t)n0 * dim, raw, (size_t)m * dim * 4, hipMemcpyHostToDevice, st));
            new_rows = new_raw + (size_t)n0 * dim;
        }
        HIP_TRY(launch_quantize_rows(ix->eng, new_rows, dim, m, ix->p.dim, ix->p.range_lo, ix->p.range_hi, codes + (size_t)n0 * rs, rs, mags + n0, raw_mags + n0, st));
        HIP_TRY(cos_deleted_grow(ix, n0, n1, st)); // the deleted set follows the tables: the new rows are live
        HIP_TRY(hipStreamSynchronize(st));
        codes.swap(ix->d_codes);
        mags.swap(ix->d_mags);
        raw_mags.swap(ix->d_raw_mags);
        new_raw.swap(ix->raw_own); // (borrowed: both empty)
        ix->d_raw = borrow ? raw : ix->raw_own.p;
        ix->n = n1; // (the locals free the old arrays)
    }
    if (ix->meta.mdim != 0u) { // the resident pseudo-root component names the pseudo nodes' vector row
        rc = meta_follow_vector_growth(ix, n0, n1);
        if (rc) return rc;
    }

    // ---- 2. level draws of the new ids: the draws a full build would have given them
    uint64_t rng = ix->link.rng;
    const std::vector<double> pv = level_probs(Ltop);
    std::vector<uint8_t> max_level(m);
    for (u32 i = 0; i < m; i++) max_level[i] = draw_level(rng, pv, Ltop);

    // ---- 3. every level grows in front of its tail, which on the base graph is ONE node, the root: the new nodes (ascending id) go
    //         between the old nodes and the root, every slot empty (level_grow_plan.h, grow_tail_kernel — the component's rule with its
    //         pseudo tail).  What names the root follows it: its vector row n0 -> n1 is a remap; its node index is the SHIFT of every
    //         index at or above the tail, where the root is the only one — so adj_node and child say what the component's say.
    std::vector<u32> tails(Ltop + 1), cursor(Ltop + 1);
    for (u32 l = 0; l <= Ltop; l++) tails[l] = ix->lv[l].n - 1;
    const std::vector<uint8_t> in_graph(m, 1);
    const std::vector<level_grow_plan::LevelPlan> plan = level_grow_plan::plan_levels(tails, m, in_graph.data(), max_level.data());
    GrowValues root_row;
    root_row.remap_from = n0;
    root_row.remap_to = n1;
    for (u32 l = 0; l <= Ltop; l++) {
        LevelHost &H = ix->lv[l];
        const level_grow_plan::LevelPlan &P = plan[l];
        const u32 nl0 = H.n, tf = P.tail_first, add = P.add, nl1 = nl0 + add, M = H.M;
        cursor[l] = tf; // the first new node takes the root's old index
        H.node_ids.pop_back();
        for (u32 i : P.who) H.node_ids.push_back((n0 + i) * ix->id_stride); // internal id of vector row n0 + i
        H.node_ids.push_back(COS_ROOT_ID);
        H.host_valid = false;
        H.nbr_ids.clear();
        H.d_adj_mag.reset();
        H.d_adj_up.reset();
        DevArr<u32> adj_vec, adj_node, node_vec, child;
        LinkLevels link;
        std::vector<u32> rows(add); // the new nodes' vector rows (alive until the synchronisation below)
        for (u32 k = 0; k < add; k++) rows[k] = n0 + P.who[k];
        HIP_TRY(adj_vec.alloc((size_t)nl1 * M));
        HIP_TRY(launch_grow_tail(H.d_adj_vec, adj_vec, nl0, tf, add, M, ROW_EMPTY, root_row, st));
        if (l > 0) {
            GrowValues nodes_here, nodes_below; // what a stored index points into: this level | the level below
            nodes_here.shift_from = tf; nodes_here.shift_add = add;
            nodes_below.shift_from = plan[l - 1].tail_first; nodes_below.shift_add = plan[l - 1].add;
            HIP_TRY(adj_node.alloc((size_t)nl1 * M));
            HIP_TRY(node_vec.alloc(nl1));
            HIP_TRY(child.alloc(nl1));
            HIP_TRY(launch_grow_tail(H.d_adj_node, adj_node, nl0, tf, add, M, ROW_EMPTY, nodes_here, st));
            HIP_TRY(launch_grow_tail(H.d_node_vec, node_vec, nl0, tf, add, 1, ROW_EMPTY, root_row, st));
            HIP_TRY(launch_grow_tail(H.d_child, child, nl0, tf, add, 1, ROW_EMPTY, nodes_below, st));
            if (add) { // node -> vector row and node -> node one level down of the new nodes
                HIP_TRY(hipMemcpyAsync(node_vec + tf, rows.data(), (size_t)add * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(child + tf, P.child.data(), (size_t)add * 4, hipMemcpyHostToDevice, st));
            }
        }
        rc = ix->link.lv.grow_level(l, nl0, tf, add, M, metric, link, st);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        adj_vec.swap(H.d_adj_vec);
        adj_node.swap(H.d_adj_node);
        node_vec.swap(H.d_node_vec);
        child.swap(H.d_child);
        ix->link.lv.swap_level(l, link);
        H.n = nl1; // (the locals free the old arrays)
    }

    // ---- 4. the new vectors, batch by batch
    rc = link_vectors(ix, n0, max_level.data(), cursor, Bmax);
    if (rc) return rc;
    guard.armed = false;
    ix->link.rng = rng;
    ix->link.n_built = n1;
    ix->link.valid = true;
    if (int32_t rc2 = cos_prepare_walk_plans(ix)) return rc2;
    return COS_OK;
}

// delete_embedding (vector_store.rs:1206-1400) for the internal ids of `ids`, one after the other in the given order (the reference
// deletes inside a transaction one embedding at a time; a later delete's walk sees the graph the earlier ones left).  Per id: ONE walk
// launch for the vector's own code — every level, ef = 512, keep 100, nothing pre-inserted in the filters (:1232-1248) — then, per
// level where the walk's list holds the node, unlink_kernel: every neighbour drops its back edge, the node's slots are emptied.  A level
// on which a neighbour would be left without any neighbour (the reference links it again between the removals, :1305-1357) is run on
// the host in the reference's order over a small cache of the rows involved (rare: a node whose ONLY neighbour is the deleted one).
// The vector's rows stay in the tables; the node is unreachable (edges are symmetric by construction) and its id is never returned by a
// walk again.  Needs the link state (slot keys / lowest caches are kept consistent: a later append continues from them).
// oracle/cosdata_oracle_hnsw.c: coso_index_delete is the CPU statement; tests/test_gpu_append.py asserts identical graphs.
namespace {

struct RowCache { // host copies of the level rows a slow-path delete touches; written back at the end
    struct Row { std::vector<u32> adj; std::vector<int32_t> key; uint8_t low_idx; int32_t low_key; bool dirty = false; };
    cos_index *ix; u32 level; u32 M;
    std::map<u32, Row> rows;
    hipError_t err = hipSuccess;
    Row &get(u32 node) {
        auto it = rows.find(node);
        if (it != rows.end()) return it->second;
        Row &r = rows[node];
        LevelHost &H = ix->lv[level];
        r.adj.resize(M); r.key.resize(M);
        auto cp = [&](void *dst, const void *src, size_t n) { if (err == hipSuccess) err = hipMemcpy(dst, src, n, hipMemcpyDeviceToHost); };
        cp(r.adj.data(), (level == 0 ? H.d_adj_vec : H.d_adj_node) + (size_t)node * M, (size_t)M * 4);
        cp(r.key.data(), ix->link.lv.key[level].as<int32_t>() + (size_t)node * M, (size_t)M * 4);
        cp(&r.low_idx, ix->link.lv.low_idx[level].as<uint8_t>() + node, 1);
        cp(&r.low_key, ix->link.lv.low_key[level].as<int32_t>() + node, 4);
        return r;
    }
    hipError_t flush(const std::vector<u32> &node_vec /* node -> vector row (level 0: identity) */) {
        LevelHost &H = ix->lv[level];
        for (auto &kv : rows) {
            if (!kv.second.dirty || err != hipSuccess) continue;
            const u32 node = kv.first;
            Row &r = kv.second;
            auto cp = [&](void *dst, const void *src, size_t n) { if (err == hipSuccess) err = hipMemcpy(dst, src, n, hipMemcpyHostToDevice); };
            if (level == 0) cp(H.d_adj_vec + (size_t)node * M, r.adj.data(), (size_t)M * 4);
            else {
                std::vector<u32> av(M);
                for (u32 j = 0; j < M; j++) av[j] = r.adj[j] == NONE ? NONE : node_vec[r.adj[j]];
                cp(H.d_adj_node + (size_t)node * M, r.adj.data(), (size_t)M * 4);
                cp(H.d_adj_vec + (size_t)node * M, av.data(), (size_t)M * 4);
            }
            cp(ix->link.lv.key[level].as<int32_t>() + (size_t)node * M, r.key.data(), (size_t)M * 4);
            cp(ix->link.lv.low_idx[level].as<uint8_t>() + node, &r.low_idx, 1);
            cp(ix->link.lv.low_key[level].as<int32_t>() + node, &r.low_key, 4);
        }
        return err;
    }
};

// ProbNode::add_neighbor (prob_node.rs:210-283) on cached rows; returns the slot or -1
int add_neighbor_host(RowCache &rc, u32 self, u32 nbr, int32_t k, int32_t kmin, int32_t kmax) {
    RowCache::Row &r = rc.get(self);
    const u32 M = rc.M, li = r.low_idx;
    if (k <= r.low_key) return -1;
    const bool ok = r.adj[li] == NONE || k > r.key[li];
    u32 old = NONE;
    if (ok) { old = r.adj[li]; r.adj[li] = nbr; r.key[li] = k; }
    u32 nl = 0;
    int32_t nk = kmax;
    for (u32 j = 0; j < M; j++) {
        if (r.adj[j] == NONE) { nk = kmin; nl = j; break; }
        if (r.key[j] < nk) { nk = r.key[j]; nl = j; }
    }
    r.low_idx = (uint8_t)nl;
    r.low_key = nk;
    r.dirty = true;
    if (!ok) return -1;
    if (old != NONE) { // the evictee drops its back edge; its cache is NOT refreshed
        RowCache::Row &o = rc.get(old);
        for (u32 j = 0; j < M; j++) if (o.adj[j] == self) { o.adj[j] = NONE; o.key[j] = INT32_MIN; o.dirty = true; break; }
    }
    return (int)li;
}

} // namespace

extern "C" int32_t cos_index_delete(cos_index *ix, const uint32_t *ids, uint32_t m) {
    if (!ix || (!ids && m)) return cos_fail(COS_ERR_INVALID, "null argument");
    if (!ix->have_vectors || !ix->have_root) return cos_fail(COS_ERR_NOT_READY, "delete needs a built index");
    for (auto &l : ix->lv) if (l.n == 0) return cos_fail(COS_ERR_NOT_READY, "delete needs a built index");
    if (!ix->link.valid) return cos_fail(COS_ERR_NOT_READY, "no link state (the graph was uploaded, its root replaced, or cos_index_release_link_state freed it)");
    if (ix->id_stride != 1u || ix->meta.mdim != 0u) return cos_fail(COS_ERR_UNIMPLEMENTED, "delete on a collection with a metadata schema");
    for (u32 i = 0; i < m; i++) if (ids[i] >= ix->n) return cos_fail(COS_ERR_INVALID, "id %u is not a resident vector", ids[i]);
    if (m == 0) return COS_OK;
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize()); // exclusive: no search in flight
    const u32 Ltop = ix->p.num_layers, L1 = Ltop + 1, metric = ix->p.metric, KEEP = (u32)KEEP_SEARCH, EF = 512;
    hipStream_t st = ix->own_stream;
    // the deleted set records the intent, whether or not the walks below find the nodes (the masked exhaustive scans read it)
    HIP_TRY(cos_deleted_mark(ix, ids, m, st));
    LinkArgs la;
    memset(&la, 0, sizeof(la));
    u32 maxM = 0;
    fill_link_levels(ix->lv, ix->link.lv, la, maxM);
    la.L1 = L1;
    la.metric = metric;
    const int32_t kmin = order_key(metric, metric_min(metric)), kmax = order_key(metric, metric_max(metric));
    DevBuf d_row, d_out_ids, d_out_nodes, d_out_sims, d_out_counts, d_status, d_dn, d_ust, d_px, d_py, d_ds, d_dst;
    HIP_TRY(d_row.alloc(4));
    HIP_TRY(d_out_ids.alloc((size_t)L1 * KEEP * 4));
    HIP_TRY(d_out_nodes.alloc((size_t)L1 * KEEP * 4));
    HIP_TRY(d_out_sims.alloc((size_t)L1 * KEEP * 4));
    HIP_TRY(d_out_counts.alloc((size_t)L1 * 4));
    HIP_TRY(d_status.alloc(4));
    HIP_TRY(d_dn.alloc((size_t)L1 * 4));
    HIP_TRY(d_ust.alloc((size_t)L1 * 4));
    HIP_TRY(d_px.alloc((size_t)KEEP * 4));
    HIP_TRY(d_py.alloc((size_t)KEEP * 4));
    HIP_TRY(d_ds.alloc((size_t)KEEP * 4));
    HIP_TRY(d_dst.alloc((size_t)KEEP * 4));
    VisTab vtab;
    std::vector<u32> h_ids((size_t)L1 * KEEP), h_nodes((size_t)L1 * KEEP), h_counts(L1), h_dn(L1), h_ust(L1);
    std::vector<std::vector<u32>> node_vec(L1); // slow path only: node -> vector row, fetched once per level
    cos_graph_changed(ix, GraphChange::ADJACENCY);
    for (auto &l : ix->lv) { l.host_valid = false; l.nbr_ids.clear(); }

    for (u32 t = 0; t < m; t++) {
        const u32 id = ids[t];
        IndexDev dev = cos_make_index_dev(ix);
        for (u32 l = 0; l <= Ltop; l++) dev.lv[l].adj_mag = nullptr; // (removed slots would keep a stale norm: harmless, but not worth a refill per id)
        WalkArgs wa;
        memset(&wa, 0, sizeof(wa));
        HIP_TRY(hipMemcpyAsync(d_row.p, &id, 4, hipMemcpyHostToDevice, st));
        wa.qcodes = ix->d_codes;
        wa.qmags = ix->d_mags;
        wa.q_rows = d_row.as<u32>();
        wa.no_self_seed = 1u;
        if (dev.visited_mode == COS_VISITED_EXACT) {
            const int32_t vrc = vis_tab_prepare(vtab, ix, 1, EF, st, wa);
            if (vrc) return vrc;
        }
        wa.B = 1;
        wa.ef = EF;
        wa.keep = KEEP;
        wa.out_ids = d_out_ids.as<u32>();
        wa.out_sims = d_out_sims.as<float>();
        wa.out_nodes = d_out_nodes.as<u32>();
        wa.out_counts = d_out_counts.as<u32>();
        wa.out_status = d_status.as<int32_t>();
        cosdev::WalkPlanIn pin = cos_walk_plan_in(ix, 1, EF);
        pin.table_min_B = pin.order_min_B = 0;
        pin.no_self_seed = true; // (the throughput kernel: the latency kernels have no unseeded filter)
        HIP_TRY(launch_walk(ix->eng, dev, wa, cosdev::walk_plan(pin).kernel, st));
        int32_t wst = COS_OK;
        HIP_TRY(hipMemcpyAsync(&wst, d_status.p, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ids.data(), d_out_ids.p, h_ids.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_nodes.data(), d_out_nodes.p, h_nodes.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_counts.data(), d_out_counts.p, (size_t)L1 * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (wst != COS_OK) return cos_fail(wst, "vector %u cannot be walked for (zero norm -> DistanceError::CalculationError)", id);
        bool any = false;
        for (u32 l = 0; l <= Ltop; l++) { // list slot = num_layers - level
            const u32 slot = Ltop - l;
            h_dn[l] = NONE;
            for (u32 i = 0; i < h_counts[slot]; i++)
                if (h_ids[(size_t)slot * KEEP + i] == id) { h_dn[l] = h_nodes[(size_t)slot * KEEP + i]; any = true; break; }
        }
        if (!any) continue;
        HIP_TRY(hipMemcpyAsync(d_dn.p, h_dn.data(), (size_t)L1 * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_unlink(la, d_dn.as<u32>(), d_ust.as<u32>(), st));
        HIP_TRY(hipMemcpyAsync(h_ust.data(), d_ust.p, (size_t)L1 * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (u32 l = 0; l <= Ltop; l++) {
            if (h_ust[l] != 1u) continue;
            // ---- the reference's own order for this level (vector_store.rs:1277-1369)
            const LevelHost &H = ix->lv[l];
            const u32 M = H.M, slot = Ltop - l, node = h_dn[l];
            if (l > 0 && node_vec[l].empty()) {
                node_vec[l].resize(H.n);
                HIP_TRY(hipMemcpy(node_vec[l].data(), H.d_node_vec, (size_t)H.n * 4, hipMemcpyDeviceToHost));
            }
            auto vec_row = [&](u32 nd) { return l == 0 ? nd : node_vec[l][nd]; };
            std::vector<u32> res; // the walk's results minus the node (swap_remove :1277; the order is irrelevant: re-sorted below)
            for (u32 i = 0; i < h_counts[slot]; i++) if (h_nodes[(size_t)slot * KEEP + i] != node) res.push_back(h_nodes[(size_t)slot * KEEP + i]);
            RowCache cache{ix, l, M};
            RowCache::Row &dr = cache.get(node);
            for (u32 j = 0; j < M; j++) {
                const u32 x = dr.adj[j];
                if (x == NONE) continue;
                RowCache::Row &xr = cache.get(x);
                bool removed = false, empty = true;
                for (u32 k = 0; k < M; k++) if (xr.adj[k] == node) { xr.adj[k] = NONE; xr.key[k] = INT32_MIN; xr.dirty = true; removed = true; break; }
                for (u32 k = 0; k < M; k++) if (xr.adj[k] != NONE) { empty = false; break; }
                if (!(removed && empty)) continue;
                std::vector<u32> cand, px, py;
                for (u32 r : res) if (r != x) { cand.push_back(r); px.push_back(vec_row(x)); py.push_back(vec_row(r)); }
                std::vector<float> sims(cand.size());
                std::vector<int32_t> dst(cand.size());
                if (!cand.empty()) {
                    HIP_TRY(hipMemcpyAsync(d_px.p, px.data(), px.size() * 4, hipMemcpyHostToDevice, st));
                    HIP_TRY(hipMemcpyAsync(d_py.p, py.data(), py.size() * 4, hipMemcpyHostToDevice, st));
                    HIP_TRY(cosdev::launch_index_pair_distances(ix->eng, ix->d_codes, ix->d_mags, ix->row_stride, ix->nchunks, ix->p.dim, metric, d_px.as<u32>(), d_py.as<u32>(),
                                                               (u32)cand.size(), d_ds.as<float>(), d_dst.as<int32_t>(), st));
                    HIP_TRY(hipMemcpyAsync(sims.data(), d_ds.p, sims.size() * 4, hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipMemcpyAsync(dst.data(), d_dst.p, dst.size() * 4, hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                    for (int32_t e : dst) if (e != COS_OK) return cos_fail(e, "re-linking node %u after the delete of %u failed (DistanceError)", x, id);
                }
                std::vector<u32> ord(cand.size());
                for (u32 i = 0; i < ord.size(); i++) ord[i] = i;
                std::sort(ord.begin(), ord.end(), [&](u32 a, u32 b) { // descending; larger id (= node index) first on ties
                    const int32_t ka = order_key(metric, sims[a]), kb = order_key(metric, sims[b]);
                    return ka != kb ? ka > kb : cand[a] > cand[b];
                });
                u32 succ = 0; // create_node_edges (vector_store.rs:976-1074)
                for (u32 oi : ord) {
                    if (succ >= M) break;
                    const int32_t k = order_key(metric, sims[oi]);
                    const int r1 = add_neighbor_host(cache, x, cand[oi], k, kmin, kmax);
                    if (r1 < 0) continue;
                    const int r2 = add_neighbor_host(cache, cand[oi], x, k, kmin, kmax);
                    if (r2 >= 0) succ++;
                    else {
                        RowCache::Row &xr2 = cache.get(x);
                        if (xr2.adj[(u32)r1] == cand[oi]) { xr2.adj[(u32)r1] = NONE; xr2.key[(u32)r1] = INT32_MIN; xr2.dirty = true; } // remove_neighbor_by_index_and_id (an empty slot's key is EMPTY_KEY, like the link kernel leaves it)
                    }
                }
            }
            RowCache::Row &dr2 = cache.get(node);
            for (u32 j = 0; j < M; j++) { dr2.adj[j] = NONE; dr2.key[j] = INT32_MIN; }
            dr2.dirty = true;
            if (cache.err != hipSuccess) HIP_TRY(cache.err);
            HIP_TRY(cache.flush(node_vec[l]));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (int32_t rc2 = cos_prepare_walk_plans(ix)) return rc2; // the adjacency-side norms of the changed rows
    return COS_OK;
}

// ================================================================================================================================
// The pseudo-root component of a collection with a metadata schema, built on the device (rounds 1-2 took it from the
// oracle and uploaded it).
//   insert order: pseudo nodes, then the Metadata replicas of every embedding      api_service.rs:135-210, vector_store.rs:484-640
//   index_embedding for such a node: every level walked from the pseudo root with the node's OWN metadata dimensions as the
//   query's filter (walk_meta_kernel<.., INDEXING>), keep 64, its id pre-inserted in the visited filter
//   create_node_edges with the two refusal rules of vector_store.rs:1017-1041     (link_kernel, LinkLevelDev::kind)
// Same batch-synchronous schedule as cos_index_build — batches of min(Bmax, max(1, inserted / 4)) nodes walk the snapshot that
// precedes them, then the round-synchronous claim / link / evict kernels connect them; oracle/cosdata_oracle_hnsw.c:
// coso_meta_build_rounds is the CPU statement and tests/test_gpu_meta.py asserts identical graphs.  The level of every node comes
// from the caller (the reference draws it with thread_rng; pseudo nodes from pseudo_level_probs, metadata/mod.rs:182-209).
// ================================================================================================================================
extern "C" int32_t cos_index_build_meta(cos_index *ix, uint32_t n_nodes, const uint32_t *node_ids, const int32_t *mbits, const uint8_t *max_levels,
                                        uint32_t batch_size) {
    if (!ix || !node_ids || !mbits || !max_levels || n_nodes == 0) return cos_fail(COS_ERR_INVALID, "null/empty node table");
    u32 vmode;
    { std::lock_guard<std::mutex> g(ix->mu); vmode = ix->p.visited_mode; }
    if (vmode != COS_VISITED_REF) return cos_fail(COS_ERR_UNIMPLEMENTED, "the metadata component is built and searched with the reference's PerformantFixedSet filter only");
    int32_t rc = cos_index_upload_meta_nodes(ix, n_nodes, node_ids, mbits); // validates, uploads mbits / norms, drops the old levels
    if (rc) return rc;
    rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 n = ix->n, Ltop = ix->p.num_layers, L1 = Ltop + 1, metric = ix->p.metric, md = ix->meta.mdim;
    const u32 Bmax = batch_max(batch_size, COMPONENT_DEFAULT_BATCH);
    hipStream_t st = ix->own_stream;
    const std::vector<u32> &tab = ix->meta.node_ids;
    if (!std::binary_search(tab.begin(), tab.end(), PSEUDO_LO)) return cos_fail(COS_ERR_INVALID, "the node table has no pseudo root (u32::MAX - 257)");
    for (u32 i = 0; i < n_nodes; i++)
        if (max_levels[i] > Ltop) return cos_fail(COS_ERR_INVALID, "node %u: level %u above num_layers %u", node_ids[i], max_levels[i], Ltop);
    std::vector<float> mmag;
    std::vector<uint8_t> kind;
    meta_row_kinds(n_nodes, node_ids, mbits, md, mmag, kind);
    std::vector<u32> ord; // insertion order: pseudo nodes (ascending id, the root excluded), then the Metadata replicas (ascending id)
    for (int pass = 0; pass < 2; pass++)
        for (u32 i = 0; i < n_nodes; i++) {
            const bool ps = is_pseudo(node_ids[i]);
            if (node_ids[i] == PSEUDO_LO || ps != (pass == 0) || kind[i] == 0) continue;
            ord.push_back(i);
        }

    MetaGuard guard{ix}; // a failed build leaves the handle without the component (filtered search: NotReady)

    // ---- level skeletons: the root + every node whose level reaches l, ascending id; every slot empty; the link state beside them ------
    ix->meta.lv.resize(L1); // (the link state was released with the old levels by cos_index_upload_meta_nodes)
    for (u32 l = 0; l <= Ltop; l++) {
        LevelHost &H = ix->meta.lv[l];
        H.M = l == 0 ? ix->p.level0_neighbors_count : ix->p.neighbors_count;
        std::vector<u32> rows; // node-table rows of this level, ascending id (the table is ascending)
        for (u32 i = 0; i < n_nodes; i++)
            if (node_ids[i] == PSEUDO_LO || (kind[i] != 0 && max_levels[i] >= l)) rows.push_back(i);
        const u32 nl = (u32)rows.size(), M = H.M;
        H.node_ids.resize(nl);
        std::vector<u32> node_vec(nl), node_meta(nl), child(nl);
        std::vector<uint8_t> kd(nl);
        for (u32 i = 0; i < nl; i++) {
            const u32 id = node_ids[rows[i]];
            H.node_ids[i] = id;
            node_vec[i] = is_pseudo(id) ? n + 1 : id / ix->id_stride;
            node_meta[i] = rows[i];
            kd[i] = kind[rows[i]];
            if (id == PSEUDO_LO) { H.root_idx = i; kd[i] = 1; }
            if (l > 0) {
                const std::vector<u32> &D = ix->meta.lv[l - 1].node_ids;
                child[i] = (u32)(std::lower_bound(D.begin(), D.end(), id) - D.begin());
            }
        }
        auto up = [&](DevArr<u32> &dst, const std::vector<u32> &src) -> hipError_t {
            hipError_t e = dst.alloc(src.size());
            return e == hipSuccess ? hipMemcpy(dst, src.data(), src.size() * 4, hipMemcpyHostToDevice) : e;
        };
        HIP_TRY(H.d_adj_vec.alloc((size_t)nl * M));
        HIP_TRY(H.d_adj_node.alloc((size_t)nl * M));
        HIP_TRY(hipMemsetAsync(H.d_adj_vec, 0xFF, (size_t)nl * M * 4, st));
        HIP_TRY(hipMemsetAsync(H.d_adj_node, 0xFF, (size_t)nl * M * 4, st));
        HIP_TRY(up(H.d_node_vec, node_vec));
        HIP_TRY(up(H.d_node_id, H.node_ids));
        HIP_TRY(up(H.d_node_meta, node_meta));
        if (l > 0) HIP_TRY(up(H.d_child, child));
        H.n = nl;
        H.host_valid = false;
        rc = ix->meta.link.lv.init_level(l, nl, M, metric, kd.data(), st);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));

    rc = link_component_nodes(ix, node_ids, mbits, mmag.data(), max_levels, ord, Bmax);
    if (rc) return rc;
    ix->meta.link.valid = true; // kept for cos_index_append_meta until cos_index_release_link_state
    guard.armed = false;
    return COS_OK;
}

// index_embeddings on a LIVE collection with a metadata schema, the component's half (vector_store.rs:484-640; the embeddings themselves:
// cos_index_append).  The new replicas' ids lie above every resident replica's and below the pseudo range, so on every level — and in the
// node table — they go between the old replicas and the pseudo nodes: every array grows in front of its tail (grow_tail_kernel), the
// indices that point into a tail follow it (level_grow_plan.h), and the schedule of cos_index_build_meta continues at the number of nodes
// it has inserted.  oracle/cosdata_oracle_hnsw.c: coso_meta_build_rounds over the WHOLE table is the CPU statement when the earlier calls
// ended on one of its batch boundaries; tests/test_gpu_meta_append.py asserts identical graphs.
extern "C" int32_t cos_index_append_meta(cos_index *ix, uint32_t n_new, const uint32_t *node_ids, const int32_t *mbits, const uint8_t *max_levels,
                                         uint32_t batch_size) {
    if (!ix || !node_ids || !mbits || !max_levels || n_new == 0) return cos_fail(COS_ERR_INVALID, "null/empty node list");
    const u32 Ltop = ix->p.num_layers, L1 = Ltop + 1, metric = ix->p.metric, md = ix->meta.mdim;
    LinkLevels &ls = ix->meta.link.lv;
    bool resident = md != 0u && ix->have_vectors && ix->meta.lv.size() == L1 && ix->meta.link.valid;
    for (u32 l = 0; resident && l <= Ltop; l++) resident = ix->meta.lv[l].n != 0 && ls.key[l].p != nullptr;
    if (!resident)
        return cos_fail(COS_ERR_NOT_READY, "no component to continue: cos_index_build_meta has not built one on this handle (an uploaded component has no "
                                           "link state), or cos_index_release_link_state freed its link state");
    u32 vmode;
    { std::lock_guard<std::mutex> g(ix->mu); vmode = ix->p.visited_mode; }
    if (vmode != COS_VISITED_REF) return cos_fail(COS_ERR_INVALID, "the metadata component is built and searched with the reference's PerformantFixedSet filter only");
    std::vector<u32> &tab = ix->meta.node_ids;
    const u32 n_tab = (u32)tab.size(), tab_tail = level_grow_plan::tail_first(tab.data(), n_tab);
    if ((u64)n_tab + n_new >= 0xFFFFFFF0ull) return cos_fail(COS_ERR_INVALID, "too many nodes");
    for (u32 i = 0; i < n_new; i++) {
        const u32 id = node_ids[i];
        if (i && id <= node_ids[i - 1]) return cos_fail(COS_ERR_INVALID, "node ids must be strictly ascending");
        if (is_pseudo(id)) return cos_fail(COS_ERR_INVALID, "node %u lies in the pseudo nodes' id range", id);
        if (tab_tail > 0 && id <= tab[tab_tail - 1]) return cos_fail(COS_ERR_INVALID, "node %u is not above every resident replica id (%u)", id, tab[tab_tail - 1]);
        if (id / ix->id_stride >= ix->n) return cos_fail(COS_ERR_INVALID, "replica id %u has no resident vector (cos_index_append first)", id);
        if (max_levels[i] > Ltop) return cos_fail(COS_ERR_INVALID, "node %u: level %u above num_layers %u", id, max_levels[i], Ltop);
    }
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    const u32 Bmax = batch_max(batch_size, COMPONENT_DEFAULT_BATCH);
    hipStream_t st = ix->own_stream;
    HIP_TRY(hipDeviceSynchronize()); // exclusive: whatever read the old arrays is done

    std::vector<float> mmag;
    std::vector<uint8_t> kind;
    meta_row_kinds(n_new, node_ids, mbits, md, mmag, kind); // (no pseudo id among them: 0 Base or 2 Metadata)
    std::vector<u32> tails(L1);
    for (u32 l = 0; l <= Ltop; l++) tails[l] = ix->meta.lv[l].root_idx; // the pseudo root is the first pseudo node of every level
    const std::vector<level_grow_plan::LevelPlan> plan = level_grow_plan::plan_levels(tails, n_new, kind.data(), max_levels);

    // ---- 1. every array grows into a local; nothing of the handle changes before all of them are written ---------------------------
    struct Grown {
        DevArr<u32> adj_vec, adj_node, node_vec, node_id, node_meta, child;
        std::vector<u32> h_vec, h_id, h_meta; // the new nodes' entries (alive until the copies below have run)
    };
    std::vector<Grown> grown(L1);
    LinkLevels grown_link;
    DevArr<int32_t> new_mbits;
    DevArr<float> new_mmags;
    const GrowValues as_is;
    auto put = [&](u32 *dst, const std::vector<u32> &src) { return src.empty() ? hipSuccess : hipMemcpyAsync(dst, src.data(), src.size() * 4, hipMemcpyHostToDevice, st); };
    for (u32 l = 0; l <= Ltop; l++) {
        LevelHost &H = ix->meta.lv[l];
        Grown &G = grown[l];
        const level_grow_plan::LevelPlan &P = plan[l];
        const u32 nl0 = H.n, tf = P.tail_first, add = P.add, nl1 = nl0 + add, M = H.M;
        GrowValues nodes_here, table_rows, nodes_below; // what a stored index points into: this level | the node table | the level below
        nodes_here.shift_from = tf; nodes_here.shift_add = add;
        table_rows.shift_from = tab_tail; table_rows.shift_add = n_new;
        if (l > 0) { nodes_below.shift_from = plan[l - 1].tail_first; nodes_below.shift_add = plan[l - 1].add; }
        HIP_TRY(G.adj_vec.alloc((size_t)nl1 * M));
        HIP_TRY(G.adj_node.alloc((size_t)nl1 * M));
        HIP_TRY(G.node_vec.alloc(nl1));
        HIP_TRY(G.node_id.alloc(nl1));
        HIP_TRY(G.node_meta.alloc(nl1));
        HIP_TRY(launch_grow_tail(H.d_adj_vec, G.adj_vec, nl0, tf, add, M, ROW_EMPTY, as_is, st));
        HIP_TRY(launch_grow_tail(H.d_adj_node, G.adj_node, nl0, tf, add, M, ROW_EMPTY, nodes_here, st));
        HIP_TRY(launch_grow_tail(H.d_node_vec, G.node_vec, nl0, tf, add, 1, ROW_EMPTY, as_is, st));
        HIP_TRY(launch_grow_tail(H.d_node_id, G.node_id, nl0, tf, add, 1, ROW_EMPTY, as_is, st));
        HIP_TRY(launch_grow_tail(H.d_node_meta, G.node_meta, nl0, tf, add, 1, ROW_EMPTY, table_rows, st));
        rc = ls.grow_level(l, nl0, tf, add, M, metric, grown_link, st);
        if (rc) return rc;
        for (u32 k = 0; k < add; k++) {
            const u32 i = P.who[k];
            G.h_vec.push_back(node_ids[i] / ix->id_stride);
            G.h_id.push_back(node_ids[i]);
            G.h_meta.push_back(tab_tail + i); // the call's rows go into the node table in order, in front of its pseudo rows
        }
        HIP_TRY(put(G.node_vec + tf, G.h_vec));
        HIP_TRY(put(G.node_id + tf, G.h_id));
        HIP_TRY(put(G.node_meta + tf, G.h_meta));
        if (l > 0) {
            HIP_TRY(G.child.alloc(nl1));
            HIP_TRY(launch_grow_tail(H.d_child, G.child, nl0, tf, add, 1, ROW_EMPTY, nodes_below, st));
            HIP_TRY(put(G.child + tf, P.child));
        }
    }
    HIP_TRY(new_mbits.alloc(((size_t)n_tab + n_new) * md));
    HIP_TRY(new_mmags.alloc((size_t)n_tab + n_new));
    HIP_TRY(launch_grow_tail((const u32 *)ix->meta.d_mbits.p, (u32 *)new_mbits.p, n_tab, tab_tail, n_new, md, 0u, as_is, st));
    HIP_TRY(launch_grow_tail((const u32 *)ix->meta.d_mmags.p, (u32 *)new_mmags.p, n_tab, tab_tail, n_new, 1, 0u, as_is, st));
    HIP_TRY(hipMemcpyAsync(new_mbits + (size_t)tab_tail * md, mbits, (size_t)n_new * md * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(new_mmags + tab_tail, mmag.data(), (size_t)n_new * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));

    // ---- 2. commit: the grown arrays move in, the host lists follow ---------------------------------------------------------------
    MetaGuard guard{ix}; // from here on a failure drops the component, as a failed cos_index_build_meta does
    for (u32 l = 0; l <= Ltop; l++) {
        LevelHost &H = ix->meta.lv[l];
        Grown &G = grown[l];
        const level_grow_plan::LevelPlan &P = plan[l];
        G.adj_vec.swap(H.d_adj_vec);
        G.adj_node.swap(H.d_adj_node);
        G.node_vec.swap(H.d_node_vec);
        G.node_id.swap(H.d_node_id);
        G.node_meta.swap(H.d_node_meta);
        if (l > 0) G.child.swap(H.d_child);
        ls.swap_level(l, grown_link);
        H.node_ids.insert(H.node_ids.begin() + P.tail_first, G.h_id.begin(), G.h_id.end());
        H.n += P.add;
        H.root_idx = level_grow_plan::remap_index(H.root_idx, P.tail_first, P.add);
        H.host_valid = false;
        H.nbr_ids.clear();
    }
    new_mbits.swap(ix->meta.d_mbits);
    new_mmags.swap(ix->meta.d_mmags);
    tab.insert(tab.begin() + tab_tail, node_ids, node_ids + n_new);
    grown.clear(); // (frees the old arrays)
    grown_link.release();
    new_mbits.reset();
    new_mmags.reset();

    // ---- 3. the new Metadata replicas, batch by batch ------------------------------------------------------------------------------
    std::vector<u32> ord;
    for (u32 i = 0; i < n_new; i++) if (kind[i] != 0) ord.push_back(i);
    rc = link_component_nodes(ix, node_ids, mbits, mmag.data(), max_levels, ord, Bmax);
    if (rc) return rc;
    guard.armed = false;
    return COS_OK;
}
