// walk_operands.hip — builds, owns and drops what a dense handle derives from its resident graph for the walk alone (WalkOperands,
// engine_internal.h): the locality-order ranks, the level table's per-level and nested operands, and LevelHost::d_adj_mag / d_adj_up /
// d_adj_tab.  The decisions are walk_operands.h's; the only call that invalidates is cos_graph_changed.  Host code only.
//
// All of it is an optimisation: a handle short of device memory goes without (cos_or_go_without) and walks from rows and mags[] with the
// same results; that is remembered in the operand's state until the graph changes, not tried again per launch.
// Built when a graph is committed (cos_prepare_walk_plans: the end of cos_index_build / _append / _delete, the upload of a graph's last
// level, which is also how cos_index_load_reference_dir commits) instead of inside the first big search, where the host-side DFS and the
// device synchronisations ran under ix->mu and held up every concurrent searcher.  The calls in get_workspace (engine.hip) stay as a
// fall-back: knobs changed after the commit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_internal.h"

using namespace cosdev;

// What follows what.  The order ranks are a permutation of a level's nodes and the table sets hold gathered code rows, norms and code
// sums of the levels' nodes; the arrays beside the adjacency hold something per neighbour SLOT.
//   * LEVELS: other nodes, or other vectors under them — everything goes.
//   * ROOT: the root is a node of every level, so a table set holds a gathered COPY of its code row, norm and code sum, which a second
//     set_root on a live graph would leave stale (the row levels would use the new row), and the norms beside the adjacency hold the old
//     root's |v| wherever the root is a neighbour: tables and adjacency side go.  The ranks stay: the root is still the last node of its
//     level and no edge moved.
//   * ADJACENCY: a delete rewrites neighbour slots under unchanged nodes (a failed build or append leaves no levels at all).  The ranks
//     stay a permutation of the level's nodes and the table sets still hold the nodes' rows — tests/test_gpu_mutation_coherence.py
//     searches a warm handle with both after every delete, against a handle that never had them; the slot arrays go.
// Nothing is freed here: a table set of the old graph goes at the next cos_ensure_level_table after a device synchronise, a level's slot
// arrays with the level or at their next fill.
void cos_graph_changed(cos_index *ix, GraphChange change) {
    WalkOperands &o = ix->ops;
    for (OperandState *s : {&o.rank, &o.table, &o.nested, &o.adj_mag, &o.adj_up, &o.adj_tab}) s->graph_changed(change);
    if (!o.table.valid()) o.table_idx = o.nested_idx = -1;
}

int32_t cos_or_go_without(hipError_t e, bool *without) {
    *without = e == hipErrorOutOfMemory;
    if (*without) (void)hipGetLastError(); // (cleared)
    else HIP_TRY(e);
    return COS_OK;
}
// ... for a build or fill of operand `s` under `key` that failed with `e`: the device is drained, "went without" is remembered
static int32_t build_failed(OperandState &s, u64 key, hipError_t e) {
    (void)hipDeviceSynchronize();
    bool without;
    const int32_t rc = cos_or_go_without(e, &without);
    if (without) s.settle(false, key);
    else s.invalidate();
    return rc;
}
// the levels as walk_operands.h's rules see them
static LevelShape level_shape(const cos_index *ix) {
    LevelShape g{};
    g.num_layers = ix->p.num_layers;
    for (u32 l = 0; l <= g.num_layers; l++) {
        g.n[l] = ix->lv[l].n;
        g.node_table[l] = ix->lv[l].d_node_vec;
        g.adj_node[l] = ix->lv[l].d_adj_node;
    }
    return g;
}

// ------------------------------------------------------------------------------------------------
// knobs
// ------------------------------------------------------------------------------------------------
// a handle's value unless the tuning registry overrides it (experiments: 0 = off / never, 4294967295 = always)
static u32 knob_or(TuneKey k, u32 handle_value, long long cap = 0xFFFFFFFFll) {
    const long long env = tune_or(k, -1);
    return env >= 0 ? (u32)std::min(env, cap) : handle_value;
}
u32 cos_walk_table_min_B(const cos_index *ix) { return knob_or(TUNE_WALK_TABLE_MIN_B, ix->walk_table_min_B); }
// Workgroups of the early part of a gated level-table GEMM (walk_plan.h; tuning knob walk_table_early_wgs).  Measured on the 12.5M x 1024
// shard, 32 768 queries per step: DESIGN.md §8.1, profiles/r07_table_early_wgs_sweep.jsonl.
static constexpr long long WALK_TABLE_EARLY_WGS_DEFAULT = 0;
// The row level under the level table reads table columns for the neighbours that have a node one level up (walk_plan.h,
// WalkPlan::up_table_level; tuning knob walk_up_table).
static constexpr long long WALK_UP_TABLE_DEFAULT = 1;
// The throughput kernel's launches read the nested level table, one GEMM column per vector of the lowest table level (table_nested.h,
// ensure_nested_table; tuning knob walk_table_nested): 1 = on graphs where that saves TABLE_NESTED_MIN_SAVED_COLS columns or more.
static constexpr long long WALK_TABLE_NESTED_DEFAULT = 1;
static u32 knob_0_to_2(TuneKey k, long long dflt) { return (u32)std::min<long long>(std::max<long long>(tune_or(k, dflt), 0), 2); }

// the handle as walk_plan (walk_plan.h) sees it: shape, every knob resolved (the tuning registry's overrides included), a launch of B
// queries at beam width ef that takes part in the walk chain.  Caller holds ix->mu where the handle is shared.
WalkPlanIn cos_walk_plan_in(const cos_index *ix, u32 B, u32 ef) {
    WalkPlanIn in{};
    in.eng = ix->eng;
    in.storage = ix->p.storage;
    in.nchunks = ix->nchunks;
    in.G = ix->G;
    in.num_layers = ix->p.num_layers;
    for (u32 l = 0; l <= ix->p.num_layers; l++) in.M[l] = ix->lv[l].M;
    in.shortlist = ix->p.shortlist_size;
    in.visited_mode = ix->p.visited_mode;
    in.mdim = ix->meta.mdim;
    in.B = B;
    in.ef = ef;
    in.chain = true;
    in.lat_max_B = knob_or(TUNE_WALK_LAT, ix->lat_max_B);
    in.lat4_max_B = knob_or(TUNE_WALK_LAT4, ix->lat4_max_B);
    in.small_table_tk = tune_or(TUNE_WALK_SMALL_TABLE_TK, 1) != 0;
    in.adj_mag_mode = (u32)tune_or(TUNE_WALK_ADJ_MAG, 1);
    in.table_min_B = cos_walk_table_min_B(ix);
    in.order_min_B = ix->walk_order_min_B;
    in.chain_min_B = ix->chain_min_B;
    in.side_min_B = ix->walk_side_min_B;
    in.table_after_sort = tune_or(TUNE_WALK_TABLE_AFTER_SORT, 1);
    in.table_supported = level_table_eng_supported(ix->eng, ix->row_stride);
    in.adj_mag_valid = ix->ops.have_adj_mag();
    in.up_table_mode = knob_0_to_2(TUNE_WALK_UP_TABLE, WALK_UP_TABLE_DEFAULT);
    in.table_early_wgs = (u32)std::min<long long>(std::max<long long>(tune_or(TUNE_WALK_TABLE_EARLY_WGS, WALK_TABLE_EARLY_WGS_DEFAULT), 0), 0xFFFFFFFFll);
    in.table_queue = level_table_gemm_queue(ix->eng, ix->row_stride);
    in.n_cus = ix->n_cus;
    in.table_nested_mode = knob_0_to_2(TUNE_WALK_TABLE_NESTED, WALK_TABLE_NESTED_DEFAULT);
    return in;
}

// ------------------------------------------------------------------------------------------------
// order ranks
// ------------------------------------------------------------------------------------------------
// The tables behind the order keys of big launches (WalkArgs::order_rank; walk_operands.h: order_key_levels, order_rank_dfs).  Built on
// the host from the adjacency, once per graph: milliseconds for levels this small (<= 2^20 nodes).
int32_t cos_ensure_order_rank(cos_index *ix) {
    WalkOperands &o = ix->ops;
    if (o.rank.built()) return COS_OK;
    for (auto &r : o.d_order_rank) r.reset();
    o.order_levels = order_key_levels(level_shape(ix), ix->row_stride, tune_or(TUNE_WALK_SPLIT_LEVELS, -1));
    if (!o.order_levels.empty()) HIP_TRY(hipDeviceSynchronize()); // a build or an upload on another stream may still be writing the adjacency
    for (u32 kl : o.order_levels) {
        const LevelHost &H = ix->lv[kl];
        std::vector<u32> adj((size_t)H.n * H.M);
        HIP_TRY(hipMemcpy(adj.data(), H.d_adj_node, adj.size() * 4, hipMemcpyDeviceToHost));
        const std::vector<u32> rank = order_rank_dfs(adj.data(), H.n, H.M);
        HIP_TRY(o.d_order_rank[kl].alloc(H.n));
        HIP_TRY(hipMemcpy(o.d_order_rank[kl], rank.data(), (size_t)H.n * 4, hipMemcpyHostToDevice));
    }
    o.rank.settle(true);
    return COS_OK;
}

// ------------------------------------------------------------------------------------------------
// level table: the per-level set of the current key, its nested set, LevelHost::d_adj_tab
// ------------------------------------------------------------------------------------------------
static int find_table_set(const WalkOperands &o, u64 key) {
    for (size_t i = 0; i < o.table_sets.size(); i++)
        if (o.table_sets[i].key == key) return (int)i;
    return -1;
}

// `n` columns from col0 on: the rows rows[0 .. n) of the vector table (`rows`: device memory)
struct TableColumns { const u32 *rows; u32 n, col0; };

// The one build of a table set: code rows, norms and code sums of `cols` columns gathered on the device, block by block; for a nested
// set (`nt`) also the node -> column array and the node bits of its levels.  Synchronous; a failure leaves `t` to free what it holds.
static hipError_t build_table_set(const cos_index *ix, const TableRule &r, const std::vector<TableColumns> &blocks, const NestedTable *nt, TableSet &t) {
    static_cast<TableRule &>(t) = r;
    const u32 level_min = r.level_min, cols = r.cols;
    t.stride = ((u64)cols + 31) / 32 * 32;
    hipError_t e = t.tcodes.alloc((size_t)cols * ix->row_stride);
    if (e == hipSuccess) e = t.tmags.alloc(cols);
    if (e == hipSuccess) e = t.tcsums.alloc(cols);
    for (size_t b = 0; b < blocks.size() && e == hipSuccess; b++)
        e = launch_level_table_gather(ix->d_codes, ix->d_mags, ix->row_stride, blocks[b].rows, blocks[b].n, blocks[b].col0, t.tcodes, t.tmags, nullptr);
    if (e == hipSuccess) e = launch_code_sums(t.tcodes, ix->row_stride, cols, t.tcsums, nullptr);
    for (u32 l = level_min; nt && l <= nt->level_top && e == hipSuccess; l++) {
        const std::vector<u32> &col = nt->col[l - level_min];
        e = t.tab_col[l].alloc(col.size());
        if (e == hipSuccess) e = hipMemcpy(t.tab_col[l], col.data(), col.size() * 4, hipMemcpyHostToDevice);
        t.node_bits[l] = nt->node_bits[l - level_min];
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

// The per-level operand (WalkArgs::tab, cosdata_hip.h cos_index_set_walk_table): which levels it covers (walk_operands.h, table_rule) and
// their nodes' rows, level by level from the top.  Leaves WalkOperands::table_idx.
static int32_t ensure_per_level_table(cos_index *ix) {
    WalkOperands &o = ix->ops;
    const TableRule r = table_rule(level_shape(ix), ix->p.ef_search, ix->p.neighbors_count, knob_or(TUNE_WALK_TABLE_COLS, ix->walk_table_max_cols, 1ll << 20),
                                   tune_or(TUNE_WALK_TABLE_RULE_C, -1));
    if (o.table.valid() && o.table.key == r.key) return COS_OK; // settled for this (graph, key): a set, or none
    if (!o.table.valid()) { // a new graph: the old graph's sets go (graph changes are exclusive: no search is in flight)
        HIP_TRY(hipDeviceSynchronize());
        o.table_sets.clear();
    }
    // (from here on every path leaves a definite state for this (graph, key): a table, or "none" — which is also what an operand
    // that could not be allocated leaves, see below)
    o.table_idx = find_table_set(o, r.key); // built before for this graph (ef_search went back and forth)?
    o.table.settle(o.table_idx >= 0, r.key);
    if (o.table_idx >= 0 || r.level_min == 0 || !level_table_eng_supported(ix->eng, ix->row_stride)) return COS_OK; // u8 codes; quaternary codes of 128 ... 1024 dims
    HIP_TRY(hipDeviceSynchronize()); // a build or an upload on another stream may still be writing the levels
    std::vector<TableColumns> blocks;
    for (u32 l = ix->p.num_layers; l >= r.level_min; l--) blocks.push_back({ix->lv[l].d_node_vec, ix->lv[l].n, r.col0[l]});
    TableSet t;
    if (const hipError_t e = build_table_set(ix, r, blocks, nullptr, t); e != hipSuccess) {
        const int32_t rc = build_failed(o.table, r.key, e); // short of HBM the walk reads rows (same results) ...
        if (rc) o.drop_tables();                            // ... anything else is a real failure: reported, and retried by the next search
        return rc;
    }
    o.table_sets.push_back(std::move(t));
    o.table_idx = (int)o.table_sets.size() - 1;
    o.table.settle(true, r.key);
    return COS_OK;
}

// The NESTED operand of the current table levels (table_nested.h): one column per node of the lowest table level, in nested order, kept
// in table_sets beside the per-level set under a key of its own, and LevelDev::adj_tab of every table level filled for it.  Right after
// ensure_per_level_table.  Leaves WalkOperands::nested_idx: the set the throughput kernel's launches use, or -1 — the knob, a storage
// other than u8, a metadata schema, a graph whose packed words do not fit 32 bits or whose levels are not nested, too few columns saved
// (knob 1), out of memory: every launch then reads the per-level set exactly as before (same results either way).
static int32_t ensure_nested_table(cos_index *ix) {
    WalkOperands &o = ix->ops;
    const u32 mode = knob_0_to_2(TUNE_WALK_TABLE_NESTED, WALK_TABLE_NESTED_DEFAULT);
    o.nested_idx = -1;
    if (mode == 0 || o.table_idx < 0 || ix->eng != ENG_U8 || ix->meta.mdim != 0u) return COS_OK;
    if (ix->G == 0u || ix->nchunks > ix->G) return COS_OK; // rows of more than one chunk pass: walk_kernel's nested rounds do not exist there (walk_plan.h)
    const u32 lmin = o.table_set()->level_min, Ltop = ix->p.num_layers;
    if (mode == 1 && o.table_set()->cols - ix->lv[lmin].n < TABLE_NESTED_MIN_SAVED_COLS) return COS_OK;
    const u64 nkey = o.table_set()->key | TABLE_KEY_NESTED;
    if (o.nested.without(nkey)) return COS_OK;
    int idx = find_table_set(o, nkey);
    if (idx < 0) {
        HIP_TRY(hipDeviceSynchronize()); // a build or an upload on another stream may still be writing the levels
        std::vector<u32> n(Ltop + 1, 0u);
        std::vector<std::vector<u32>> child(Ltop + 1);
        for (u32 l = lmin; l <= Ltop; l++) {
            n[l] = ix->lv[l].n;
            if (l == lmin) continue;
            if (!ix->lv[l].d_child) { o.nested.settle(false, nkey); return COS_OK; }
            child[l].resize(n[l]);
            HIP_TRY(hipMemcpy(child[l].data(), ix->lv[l].d_child, (size_t)n[l] * 4, hipMemcpyDeviceToHost));
        }
        NestedTable nt;
        if (!table_nested_columns(lmin, Ltop, n, child, &nt)) { o.nested.settle(false, nkey); return COS_OK; }
        // the gather's index list: vector row of every column
        std::vector<u32> rows(nt.cols), node_vec(nt.cols);
        HIP_TRY(hipMemcpy(node_vec.data(), ix->lv[lmin].d_node_vec, (size_t)nt.cols * 4, hipMemcpyDeviceToHost));
        for (u32 c = 0; c < nt.cols; c++) rows[c] = node_vec[nt.col_node[c]];
        TableSet t;
        DevArr<u32> d_rows;
        hipError_t e = d_rows.alloc(nt.cols);
        if (e == hipSuccess) e = hipMemcpy(d_rows, rows.data(), (size_t)nt.cols * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = build_table_set(ix, TableRule{nkey, lmin, nt.cols, {}}, {{d_rows, nt.cols, 0u}}, &nt, t);
        if (e != hipSuccess) return build_failed(o.nested, nkey, e);
        o.table_sets.push_back(std::move(t));
        idx = (int)o.table_sets.size() - 1;
    }
    if (!o.adj_tab.built(nkey)) { // a new graph or key, or the adjacency changed under a table that stayed (cos_index_delete): refill
        if (o.adj_tab.without(nkey)) return COS_OK;
        HIP_TRY(hipDeviceSynchronize()); // (a launch in flight may still read the arrays that go; the adjacency may still be written)
        o.adj_tab.invalidate();
        for (u32 l = 0; l <= Ltop; l++) ix->lv[l].d_adj_tab.reset();
        const TableSet &t = o.table_sets[(size_t)idx];
        hipError_t e = hipSuccess;
        for (u32 l = lmin; l <= Ltop && e == hipSuccess; l++) {
            LevelHost &H = ix->lv[l];
            if (!H.d_adj_node) e = hipErrorInvalidValue;
            if (e == hipSuccess) e = H.d_adj_tab.alloc((size_t)H.n * H.M);
            if (e == hipSuccess) e = launch_fill_adj_tab(H.d_adj_node, t.tab_col[l], H.n, H.M, t.node_bits[l], H.d_adj_tab, ix->own_stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ix->own_stream);
        if (e != hipSuccess) {
            for (u32 l = 0; l <= Ltop; l++) ix->lv[l].d_adj_tab.reset();
            return build_failed(o.adj_tab, nkey, e);
        }
        o.adj_tab.settle(true, nkey);
    }
    o.nested_idx = idx;
    return COS_OK;
}

int32_t cos_ensure_level_table(cos_index *ix) {
    if (int32_t rc = ensure_per_level_table(ix)) return rc;
    return ensure_nested_table(ix);
}

// ------------------------------------------------------------------------------------------------
// beside the adjacency: norms, node one level up
// ------------------------------------------------------------------------------------------------
// LevelDev::adj_mag of every level: the norm of each scanned neighbour slot next to the adjacency.  Graph changes are exclusive (no
// search in flight).
int32_t cos_ensure_adj_mags(cos_index *ix) {
    WalkOperands &o = ix->ops;
    if (o.adj_mag.valid()) return COS_OK; // filled, or this graph goes without: the next graph change tries again
    if (!cos_graph_ready(ix) || ix->meta.mdim != 0u) return COS_OK; // (collections with a metadata schema keep the gathers: their walks are walk_meta_kernel's)
    if (walk_rows_over_64_slots(cos_walk_plan_in(ix, 0, 0))) return COS_OK; // (walk_general_kernel's indexes: it gathers the norms)
    HIP_TRY(hipDeviceSynchronize()); // a build or an upload on another stream may still be writing the adjacency
    for (u32 l = 0; l <= ix->p.num_layers; l++) ix->lv[l].d_adj_mag.reset();
    for (u32 l = 0; l <= ix->p.num_layers; l++) {
        LevelHost &H = ix->lv[l];
        const u32 slots = std::min(H.M, ix->p.shortlist_size);
        if (const hipError_t e = H.d_adj_mag.alloc((size_t)H.n * slots); e != hipSuccess) {
            for (u32 k = 0; k < l; k++) ix->lv[k].d_adj_mag.reset();
            return build_failed(o.adj_mag, 0, e);
        }
        HIP_TRY(launch_fill_adj_mag(H.d_adj_vec, ix->d_mags, H.d_adj_mag, H.n, H.M, slots, ix->own_stream));
    }
    HIP_TRY(hipStreamSynchronize(ix->own_stream));
    o.adj_mag.settle(true);
    return COS_OK;
}

// LevelDev::adj_up of the one level that can use it (walk_operands.h, adj_up_wanted_level).  Called where the table's operand is (a
// commit; get_workspace's fall-back after a knob changed).  When the table rule moves to another level the old array goes.
int32_t cos_ensure_adj_up(cos_index *ix) {
    WalkOperands &o = ix->ops;
    const u32 want = adj_up_wanted_level(o.table_idx >= 0 ? o.table_set()->level_min : 0u, ix->eng, ix->G, o.have_adj_mag(),
                                         tune_or(TUNE_WALK_UP_TABLE, WALK_UP_TABLE_DEFAULT) != 0);
    // With the nested table (ensure_nested_table has settled it) the entries hold the COLUMN of the node one level up, which is what the
    // throughput kernel — the array's only reader — then indexes the table with; a change of form refills like a change of level.
    const bool nested = o.nested_idx >= 0;
    const u64 key = want | (nested ? WalkOperands::ADJ_UP_NESTED : 0ull);
    if (want != 0u && (o.adj_up.built(key) || o.adj_up.without(want))) return COS_OK; // filled for this graph and rule, or known not to fit
    bool any = false;
    for (u32 l = 0; l <= ix->p.num_layers; l++) any = any || ix->lv[l].d_adj_up;
    if (any) {
        HIP_TRY(hipDeviceSynchronize()); // (the rule moved under running searches: a launch in flight may still read the array that goes)
        for (u32 l = 0; l <= ix->p.num_layers; l++) ix->lv[l].d_adj_up.reset();
    }
    o.adj_up.invalidate();
    if (want == 0u) return COS_OK;
    HIP_TRY(hipDeviceSynchronize()); // a build or an upload on another stream may still be writing the adjacency
    LevelHost &H = ix->lv[want];
    const LevelHost &U = ix->lv[want + 1];
    const u32 slots = std::min(H.M, ix->p.shortlist_size);
    if (!H.d_adj_node || !U.d_child || H.n == 0 || U.n == 0) return COS_OK;
    DevArr<u32> up; // node of level `want` -> node of the level above
    hipError_t e = H.d_adj_up.alloc((size_t)H.n * slots);
    if (e == hipSuccess) e = up.alloc(H.n);
    if (e != hipSuccess) {
        H.d_adj_up.reset();
        return build_failed(o.adj_up, want, e);
    }
    const u32 *up_col = nested ? o.nested_set()->tab_col[want + 1].p : nullptr;
    HIP_TRY(launch_fill_adj_up(H.d_adj_vec, H.d_adj_node, ix->d_mags, U.d_child, U.n, up, H.d_adj_up, H.n, H.M, slots, ix->own_stream, up_col));
    HIP_TRY(hipStreamSynchronize(ix->own_stream));
    o.adj_up.settle(true, key);
    return COS_OK;
}

int32_t cos_prepare_walk_plans(cos_index *ix) {
    std::lock_guard<std::mutex> g(ix->mu);
    if (int32_t rc = cos_ensure_adj_mags(ix)) return rc;
    if (ix->walk_order_min_B)
        if (int32_t rc = cos_ensure_order_rank(ix)) return rc;
    if (cos_walk_table_min_B(ix)) {
        if (int32_t rc = cos_ensure_level_table(ix)) return rc;
        if (int32_t rc = cos_ensure_adj_up(ix)) return rc;
    }
    return COS_OK;
}

// ------------------------------------------------------------------------------------------------
// the ABI entry points that set the table's knobs and report on the operands
// ------------------------------------------------------------------------------------------------
extern "C" int32_t cos_index_set_walk_table(cos_index *ix, uint32_t max_cols, uint32_t min_queries) {
    if (!ix) return cos_fail(COS_ERR_INVALID, "null argument");
    if (max_cols > (1u << 20) && max_cols != COS_WALK_TABLE_AUTO) return cos_fail(COS_ERR_INVALID, "max_cols must be <= 2^20 (or COS_WALK_TABLE_AUTO)");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->walk_table_max_cols = max_cols;
    ix->walk_table_min_B = min_queries;
    return COS_OK;
}

extern "C" int32_t cos_index_walk_table_info(cos_index *ix, uint32_t *out_level_min, uint32_t *out_cols) {
    if (!ix || !out_level_min || !out_cols) return cos_fail(COS_ERR_INVALID, "null argument");
    *out_level_min = *out_cols = 0;
    if (!cos_graph_ready(ix)) return cos_fail(COS_ERR_NOT_READY, "index needs vectors, root and every graph level");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    if (cos_walk_table_min_B(ix) == 0) return COS_OK;
    if ((rc = cos_ensure_level_table(ix))) return rc;
    const TableSet *t = ix->ops.nested_idx >= 0 ? ix->ops.nested_set() : ix->ops.table_set(); // what the next big launch computes
    if (t) *out_level_min = t->level_min, *out_cols = t->cols;
    return COS_OK;
}

extern "C" int32_t cos_index_walk_order_cuts(cos_index *ix, uint32_t *out_levels, uint32_t cap, uint32_t *out_n) {
    if (!ix || !out_n || (cap && !out_levels)) return cos_fail(COS_ERR_INVALID, "null argument");
    *out_n = 0;
    if (!cos_graph_ready(ix)) return cos_fail(COS_ERR_NOT_READY, "index needs vectors, root and every graph level");
    int32_t rc = cos_set_device(ix);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    if ((rc = cos_ensure_order_rank(ix))) return rc;
    for (u32 l : ix->ops.order_levels) {
        if (*out_n < cap) out_levels[*out_n] = l;
        (*out_n)++;
    }
    return COS_OK;
}
