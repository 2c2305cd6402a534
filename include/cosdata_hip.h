/*
 * cosdata_hip.h — C ABI of the MI355X-native ANN query engine for cosdata's dense/hybrid
 * search path (libcosdata_hip.so, hand-written HIP kernels for gfx950).
 *
 * The reference (cosdata/cosdata @ 2025-09-19) has no FFI/plugin seam; this header introduces
 * it at the L3<->L2 line of SURVEY.md §1.  Every entry point names the reference interface it
 * stands behind (paths relative to the reference root).  INTEGRATION.md shows the Rust
 * `extern "C"` block and the call sites a maintainer would redirect.
 *
 * Conventions
 *   - plain pointers and sizes, POD structs with an explicit struct_size; no C++/torch types;
 *   - every function returns a cos_status (0 = ok) and never unwinds or aborts across the ABI;
 *     cos_last_error_string() gives a per-thread message for the last non-zero status;
 *   - host buffers are borrowed for the duration of the call only; the library owns all device
 *     memory behind the opaque handle (exception: COS_UPLOAD_BORROW_DEVICE);
 *   - search entry points are thread-safe on a shared handle (the reference calls search from
 *     rayon workers, indexes/mod.rs:268-271); uploads/builds are exclusive;
 *   - internal ids follow the reference: vectors 0..n-1 (collection.rs:451-468, sequential),
 *     root = 0xFFFFFFFF (vector_store.rs:47), query = 0xFFFFFFFE (indexes/hnsw/mod.rs:398).
 */
#ifndef COSDATA_HIP_H
#define COSDATA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COS_ABI_VERSION 1u

/* models/types.rs:462-468 DistanceMetric */
typedef enum { COS_METRIC_COSINE = 0, COS_METRIC_EUCLIDEAN = 1, COS_METRIC_HAMMING = 2, COS_METRIC_DOT = 3 } cos_metric;
/* quantization/mod.rs:20-25 StorageType; SubByte carries its resolution separately */
typedef enum { COS_STORAGE_U8 = 0, COS_STORAGE_SUBBYTE = 1, COS_STORAGE_F16 = 2, COS_STORAGE_F32 = 3 } cos_storage;

typedef enum {
    COS_OK = 0,
    COS_ERR_STORAGE_MISMATCH = 1, /* DistanceError::StorageMismatch  -> WaCustomError::QuantizationMismatch */
    COS_ERR_CALCULATION = 2,      /* DistanceError::CalculationError (zero norm; cosine.rs:228-232)          */
    COS_ERR_INVALID = 3,          /* bad params / sizes / ordering of an upload                              */
    COS_ERR_UNIMPLEMENTED = 4,    /* arms the reference leaves `unimplemented!()` or not yet on the GPU      */
    COS_ERR_HIP = 5,              /* HIP runtime error (message has the hipError string)                     */
    COS_ERR_NOT_READY = 6,        /* search before vectors + graph are resident                              */
    COS_ERR_NO_DEVICE = 7         /* no usable gfx950 device: the product path never falls back to the CPU   */
} cos_status;

#define COS_ROOT_ID 0xFFFFFFFFu
#define COS_QUERY_ID 0xFFFFFFFEu
#define COS_SLOT_EMPTY 0xFFFFFFFDu /* a null neighbour pointer (prob_node.rs:97) in flat graph uploads */

/* visited-set semantics of the walk */
#define COS_VISITED_REF 0u   /* PerformantFixedSet replica (models/fixedset.rs): 64*M-bit lossy filter -> ID parity */
#define COS_VISITED_EXACT 1u /* exact visited set (recall mode; not ID-identical to the reference) */

/* upload flags */
#define COS_UPLOAD_DEFAULT 0u
#define COS_UPLOAD_BORROW_DEVICE 1u /* raw f32 pointer is device memory the caller keeps alive; no copy */

/* HNSWHyperParams (indexes/hnsw/types.rs:10-17) + the index fields search needs
 * (indexes/hnsw/mod.rs:59-78) + config.search.shortlist_size (config.toml:32). */
typedef struct {
    uint32_t struct_size; /* = sizeof(cos_params) */
    uint32_t abi_version; /* = COS_ABI_VERSION */
    uint32_t dim;
    uint32_t metric;     /* cos_metric */
    uint32_t storage;    /* cos_storage */
    uint32_t resolution; /* SubByte bits (1..3) */
    float range_lo, range_hi; /* values_range */
    uint32_t num_layers;             /* levels 0..num_layers */
    uint32_t neighbors_count;        /* M  (power of two, <= 256) */
    uint32_t level0_neighbors_count; /* M0 (power of two, <= 256) */
    uint32_t ef_construction;        /* <= 16384: up to 1024 the fast walk kernels, above it walk_general_kernel */
    uint32_t ef_search;              /* the same domain; cos_index_set_ef_search moves it on a live handle */
    uint32_t shortlist_size;         /* config.toml [search]: any; more than 64 scanned slots per node walk with walk_general_kernel */
    uint32_t visited_mode; /* COS_VISITED_* */
    int32_t device;        /* HIP device ordinal */
    uint32_t id_base;      /* shard support: global id of local vector 0; output ids = id_base + local id */
    uint32_t reserved;
    uint64_t seed;         /* GPU builder: level draws + root vector */
} cos_params;

typedef struct cos_index cos_index; /* opaque: one immutable device-resident index snapshot (one shard) */

/* Per-batch counters written by the kernels; the roofline's ALGORITHMIC bytes come from these. */
typedef struct {
    uint64_t evals;        /* distance evaluations (walk) */
    uint64_t expansions;   /* popped + expanded nodes */
    uint64_t adj_bytes;    /* sum over expansions of min(M_level, shortlist_size) * 4: the scanned slots of the row */
    uint64_t rerank_rows;  /* raw f32 rows gathered by the exact rerank */
    float walk_ms;         /* HIP-event time of the walk kernel of the last call on this stream (0 if timing off) */
    float finalize_ms;
    float prep_ms;
    uint32_t reserved;
} cos_search_stats;

/* ---- lifecycle ------------------------------------------------------------------------------ */
/* api_service.rs:26 init_hnsw_index_for_collection -> HNSWIndex::new (indexes/hnsw/mod.rs:81). */
int32_t cos_index_create(const cos_params *params, cos_index **out);
int32_t cos_index_destroy(cos_index *ix);
const char *cos_last_error_string(void);
int32_t cos_device_count(int32_t *out);
/* Diagnostic (not a reference interface): empirical HBM ceilings for the roofline report, SURVEY.md 8(d).
 * kind 0 = streaming read, 1 = streaming copy (read+write bytes), 2 = random gather of row_bytes-sized rows
 * (the walk's access pattern; row_bytes multiple of 16, <= 1024).  Allocates buffer_bytes (x2 for copy),
 * times `iters` launches with HIP events, returns GB/s (1e9 B/s). */
int32_t cos_hbm_probe(int32_t device, uint32_t kind, uint64_t buffer_bytes, uint32_t row_bytes, uint32_t iters,
                      double *out_gbps);

/* ---- data upload (host side of the snapshot; the Rust host walks its graph once) ------------ */
/* Collection::index_embeddings' raw f32 values (collection.rs:368, get_raw_emb_by_internal_id) for
 * internal ids [0,n).  The library quantizes them on the device with the index's StorageType
 * (ScalarQuantization::quantize, quantization/scalar.rs:10-52) and keeps raw for the exact rerank. */
int32_t cos_index_upload_vectors(cos_index *ix, const float *raw, uint32_t n, uint32_t flags);
/* Re-uploading vectors starts a new collection snapshot: the graph, the pseudo-root component AND the metadata schema
 * (cos_index_enable_metadata: mdim, max_replicas_per_node, the node table) are dropped — ids go back to id = vector row — so a host
 * that filters must call cos_index_enable_metadata again before cos_index_upload_meta_nodes / cos_index_build_meta. */
/* create_root_node's random vector (vector_store.rs:30-36), id u32::MAX. */
int32_t cos_index_set_root(cos_index *ix, const float *root_raw);
/* One HNSW level as flat arrays exported from ProbNode (prob_node.rs:97-109):
 * node_ids[n_nodes] ascending with COS_ROOT_ID last; nbr_ids[n_nodes][M_level] in SLOT ORDER,
 * COS_SLOT_EMPTY for null slots.  Level 0 must hold every vector.  Child links are implied
 * (same id one level down, vector_store.rs:897-903). */
int32_t cos_index_upload_graph_level(cos_index *ix, uint32_t level, uint32_t n_nodes, const uint32_t *node_ids,
                                     const uint32_t *nbr_ids);
int32_t cos_index_level_count(const cos_index *ix, uint32_t level, uint32_t *n_nodes);
int32_t cos_index_download_graph_level(const cos_index *ix, uint32_t level, uint32_t *node_ids, uint32_t *nbr_ids);
/* quantized codes in the REFERENCE layout (SubByte plane-major) + mags, rows [0,n] (row n = root) */
int32_t cos_index_download_codes(const cos_index *ix, void *codes, float *mags);
int32_t cos_index_download_root(const cos_index *ix, float *root_raw);

/* Load the graph of an index the reference server persisted (its `<collection>/dense_hnsw/` directory: {k}.index node records,
 * nodes.ptr, prop.data — models/serializer/hnsw/node.rs:19-101, neighbors.rs:22-61, latest_node.rs:18-44,
 * models/file_persist.rs:58-108) into the handle: every level's node ids and neighbour ids in slot order (as
 * cos_index_upload_graph_level would receive them) plus the root's stored code.  The raw vectors must already be resident
 * (cos_index_upload_vectors: the files hold only quantized codes, the exact rerank needs raw f32); root_ptr_offset =
 * HNSWIndexData.root_vec_ptr_offset (indexes/hnsw/mod.rs:47-57, kept in LMDB by the host).  COS_LOAD_VERIFY_CODES also
 * compares every stored Storage with the device's own quantization of the uploaded vector (StorageMismatch on a difference).
 * Collections with a metadata schema are refused (Unimplemented).  Format parity is UNPINNED: no reference-written file
 * exists in this image; see cosdata_amd/csrc/ref_index_reader.hip. */
#define COS_LOAD_DEFAULT 0u
#define COS_LOAD_VERIFY_CODES 1u
int32_t cos_index_load_reference_dir(cos_index *ix, const char *dense_hnsw_dir, uint32_t root_ptr_offset, uint32_t flags);
/* Host-only views of the same directory (no device needed): node count per level, then one level as the flat arrays
 * cos_index_upload_graph_level takes (node_ids ascending, root last; nbr_ids [n][M_level], COS_SLOT_EMPTY = null slot). */
int32_t cos_reference_dir_level_counts(const char *dense_hnsw_dir, uint32_t num_layers, uint32_t neighbors_count,
                                       uint32_t level0_neighbors_count, uint32_t *level_counts /* [num_layers + 1] */);
int32_t cos_reference_dir_read_level(const char *dense_hnsw_dir, uint32_t num_layers, uint32_t neighbors_count,
                                     uint32_t level0_neighbors_count, uint32_t level, uint32_t *node_ids, uint32_t *nbr_ids);

/* vector_store::index_embeddings (vector_store.rs:714) on the device: builds every level for the
 * uploaded vectors with the reference's edge semantics, batch-synchronously. */
int32_t cos_index_build(cos_index *ix, uint32_t batch_size);
/* vector_store::index_embeddings called AGAIN on a live index (vector_store.rs:714-780; index_embedding :782-975 per vector): m more
 * vectors take the internal ids [n, n + m) (sequential: collection.rs:451-468) and are inserted into the RESIDENT graph — no rebuild —
 * by the schedule of cos_index_build continued at inserted = n: level draws from the same RNG stream (the draws a full build would
 * have given these ids), batches of min(batch_size, max(1, inserted / 4)) walking the snapshot that precedes them, the link kernels on
 * the link state cos_index_build left on the handle (similarity of every neighbour slot + every node's cached lowest slot,
 * prob_node.rs:108).  The graph equals a full build's when the earlier build ended on one of its batch boundaries, and always the
 * oracle's coso_index_append_vectors + coso_index_build_rounds_continue.
 *   raw, flags = 0:                        HOST pointer to the m new rows [m][dim]; the index owns its raw rows
 *   raw, flags = COS_UPLOAD_BORROW_DEVICE: DEVICE pointer to the caller's WHOLE grown table [n + m][dim] (rows [0, n) unchanged), borrowed
 *                                          from now on — for an index whose rows were uploaded with the same flag
 * COS_ERR_NOT_READY: no graph, or no link state to continue from (the graph was uploaded, its root replaced, or the state released).
 * A collection with a metadata schema (cos_index_enable_metadata): the new rows take the ids (n + i) x max_replicas_per_node; their
 * replica nodes follow with cos_index_append_meta.
 * Exclusive like every graph change (no search in flight); a failed append leaves the handle without a graph. */
int32_t cos_index_append(cos_index *ix, const float *raw, uint32_t m, uint32_t flags, uint32_t batch_size /* 0 = 4096 */);
/* vector_store::delete_embedding (vector_store.rs:1206-1400) for the internal ids of `ids`, one after the other in the given order: per id
 * one walk for the vector's own code on every level (ef 512, keep 100, filters not pre-seeded, :1232-1248); on every level whose list
 * holds the node, its neighbours drop their back edges (remove_neighbor_by_id, prob_node.rs:285-306), a neighbour left without any
 * neighbour is linked again from the walk's results re-scored against it (:1305-1357), and the node's own slots are emptied.  The
 * vector's rows stay resident (ids are never reused, collection.rs:451-468); no walk reaches the node again (exhaustive scans —
 * cos_flat_search_batch, cos_bruteforce_topk — still see the row: use their masked forms with COS_SCAN_SKIP_DELETED; the id is recorded in
 * the handle's deleted set whether or not the walk found the node).
 * Needs the link state like cos_index_append; exclusive like every graph change.  oracle: coso_index_delete. */
int32_t cos_index_delete(cos_index *ix, const uint32_t *ids, uint32_t m);
/* The link state of an UPLOADED graph (cos_index_upload_graph_level, cos_index_load_reference_dir), as the reference has it after a reload:
 * slot similarities (persisted by the reference, serializer/hnsw/neighbors.rs:22-61; recomputed here on the resident codes) and every
 * node's cached lowest slot by the deserializer's rule (ProbNode::new_with_neighbors_and_versions, prob_node.rs:145-181: the first empty
 * slot, else the first strictly smallest similarity).  Afterwards cos_index_append / cos_index_delete work on the uploaded graph; appends
 * draw their levels from the seed's stream advanced past the resident vectors.  Every storage an index can have. */
int32_t cos_index_restore_link_state(cos_index *ix);
/* frees the link state (as large as the adjacency: 4 bytes per neighbour slot) of the base graph and of the pseudo-root component;
 * cos_index_append and cos_index_append_meta then return COS_ERR_NOT_READY */
int32_t cos_index_release_link_state(cos_index *ix);

/* ---- search --------------------------------------------------------------------------------- */
/* IndexOps::batch_search -> HNSWIndex::search_internal (indexes/mod.rs:260, indexes/hnsw/mod.rs:390):
 * quantize query -> ann_search (every level, ef_search) -> finalize_ann_results (exact f32 rerank).
 * queries [B][dim] raw f32; outputs [B][top_k] (internal id + id_base, cosine score), out_counts[B].
 * Like the reference's collect::<Result<_>>, any failing query fails the call (first error
 * returned); out_status[B] (optional) has the per-query cos_status. */
int32_t cos_search_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, uint32_t *out_ids,
                         float *out_scores, uint32_t *out_counts, int32_t *out_status);
/* Same, all pointers DEVICE memory, enqueued on `stream` (hipStream_t) without synchronising.
 * Statuses land in d_out_status[B] (required).  One in-flight batch per stream; concurrent host
 * threads use distinct streams. */
int32_t cos_search_batch_device(cos_index *ix, const float *d_queries, uint32_t B, uint32_t top_k, uint32_t *d_out_ids,
                                float *d_out_scores, uint32_t *d_out_counts, int32_t *d_out_status, void *stream);
/* ann_search's raw per-level output (vector_store.rs:256): ids/sims [B][(num_layers+1)][100],
 * counts [B][num_layers+1], top level first.  Host buffers. */
int32_t cos_ann_search_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t *out_ids, float *out_sims,
                             uint32_t *out_counts, int32_t *out_status);
/* Dynamic batching for the host API: concurrent cos_search_batch calls (rayon workers / request handlers) with
 * the same top_k are fused into one launch of up to max_queries queries.  The request that opens a launch issues it when it is
 * full, or — while fewer than two coalesced launches of the handle are in flight — window_us after its last arrival (at most 8
 * windows after its first); while two are in flight it keeps gathering and goes when one of them completes, so under load the
 * launches grow to what the callers offer and an idle device answers after one window.  Choose max_queries near HALF of what the
 * callers offer at once (64 callers x 256 queries: 8 192), so that two launches alternate — one on the device while the other is
 * copied in and out.  max_queries = 0 (default) turns it off.  Results are identical to un-coalesced calls.  Not a reference
 * interface. */
int32_t cos_index_set_coalescing(cos_index *ix, uint32_t max_queries, uint32_t window_us);
/* What the batching did since the last cos_index_set_coalescing (diagnostic; bench.py reports it next to the callers' rate). */
typedef struct cos_coalescing_stats {
    uint64_t launches;         /* coalesced launches issued */
    uint64_t queries;          /* queries they carried */
    uint64_t requests;         /* cos_search_batch calls they carried */
    uint64_t closed_full;      /* launches that left because max_queries was reached */
    uint64_t closed_quiet;     /* ... because window_us passed without an arrival */
    uint64_t closed_deadline;  /* ... because 8 windows passed since the first request */
    uint64_t solo_calls;       /* calls below max_queries that found every slot in flight and launched on their own */
} cos_coalescing_stats;
int32_t cos_index_coalescing_stats(cos_index *ix, cos_coalescing_stats *out);
int32_t cos_index_set_ef_search(cos_index *ix, uint32_t ef_search);
int32_t cos_index_set_visited_mode(cos_index *ix, uint32_t mode);
/* Latency mode.  A launch of at most max_queries queries (default COS_LATENCY_MODE_DEFAULT_MAX_B; 0 = never) runs the latency
 * variant of the walk where it applies (u8 / quaternary storage, ef <= 256, reference visited filter): the code rows of every
 * entry of the lookahead window are fetched speculatively in one go and committed in pop order.  Same results bit for bit;
 * it trades bandwidth (idle on a small launch) for dependent round trips.  The reference's caller submits one 256-query batch
 * at a time per worker (indexes/mod.rs:260-272); bigger launches (coalesced batches) keep the throughput kernel. */
/* Since round 4 a launch over u8 codes has a level table (cos_index_set_walk_table, on by default) and then takes the throughput kernel
 * at every size — with the table it is faster than the one-wave latency kernel from 256 to 2048 queries per launch — so this knob
 * now selects the kernel only for quaternary storage, or with the table switched off. */
#define COS_LATENCY_MODE_DEFAULT_MAX_B 2048u
int32_t cos_index_set_latency_mode(cos_index *ix, uint32_t max_queries);
/* Four waves per query (kernels_walk_lat4.hip) for the smallest launches — at most max_queries queries (default
 * COS_LATENCY_WAVES_DEFAULT_MAX_B: one or two client batches; 0 = never): every query gets a workgroup of four waves, each owning one
 * entry of the lookahead window for the speculative half of a round, and the commit is data-parallel over the window.  Same conditions
 * and same results, bit for bit, as the one-wave latency variant; it exists for the reference's literal unit of work, one
 * `query-batch = 256` per worker (indexes/mod.rs:260-272): 0.94 vs 1.05 ms per batch at ef 64, 1.87 vs 2.35 ms at ef 256 (1M x 768 u8);
 * from 1024 queries per launch on the one-wave kernel is faster (two of these workgroups fill a CU's registers). */
/* With a level table (u8, the default) the four-wave kernel is taken above ef_search 64 only (it reads the table too: 1.73 vs 2.20 ms
 * per batch at ef 256); up to ef 64 the throughput kernel with the table is faster (0.77 vs 0.82 ms). */
#define COS_LATENCY_WAVES_DEFAULT_MAX_B 512u
int32_t cos_index_set_latency_waves(cos_index *ix, uint32_t max_queries);
/* Locality order of big launches — at least min_queries queries (default COS_WALK_ORDER_DEFAULT_MIN_B; 0 = never).  Not a reference
 * interface: the reference answers each query on its own rayon task (indexes/mod.rs:260-272) and has no launch whose order could
 * matter; on the device the order decides which rows a query finds in cache.  Such a launch walks in two steps of the same kernel:
 * the levels from the top down to a KEY LEVEL in arrival order — the key level is the lowest level whose code rows take at most
 * 64 MB (1M x 768 u8: level 2; cos_index_walk_order_cuts reports it; COS_WALK_SPLIT overrides) — then the launch is sorted by the
 * position, in a depth-first order of the key level's graph, of the best node each query found there, and EVERY level below the
 * key level (not only level 0) runs with the sorted queries dealt to the XCDs in contiguous runs (workgroup b runs on XCD b % 8,
 * each XCD has its own L2), so the waves resident on an XCD walk neighbouring regions of the graph.  The rerank follows the same
 * order.  Every query's walk, and so every result, is bit for bit what it is without the order.
 * Applies at ef_search <= 256: wider beams are bound by their own serial work and the second launch's tail costs more than the order saves. */
#define COS_WALK_ORDER_DEFAULT_MIN_B 8192u
int32_t cos_index_set_walk_order(cos_index *ix, uint32_t min_queries);
/* The levels after which such a launch is cut (descending; the launch is re-sorted after each): by default ONE, the lowest level whose
 * code rows take at most 64 MB; none (*out_n = 0) if the graph has no level the order can use.  Diagnostic: bench.py reports it. */
int32_t cos_index_walk_order_cuts(cos_index *ix, uint32_t *out_levels, uint32_t cap, uint32_t *out_n);
/* Level table — launches of at least min_queries queries over u8 codes (default COS_WALK_TABLE_DEFAULT_MIN_B = every launch; 0 =
 * never).  With a table a launch takes the throughput kernel, except one client batch above ef_search 64, which takes the four-wave
 * latency kernel (it reads the table too); the one-wave latency kernel then only serves storages without a table.  Not a reference
 * interface.  The graph's top levels are small and walked by every query (1M vectors: levels >= 4 hold 5 300 nodes), so
 * for the levels >= L_t the launch first computes similarity(query, node) for EVERY node of those levels as one exact-integer i8 MFMA
 * GEMM (dot_product_u8's integer, the same `as f32` and the same division by |q| * |v|, cosine.rs:223-235), and the walk of those
 * levels reads the similarity (4 bytes) where it would have gathered and dotted a code row.  Which nodes a walk visits, the lossy
 * visited filter and every result are bit for bit what they are without the table.
 * L_t: with max_cols = COS_WALK_TABLE_AUTO (the default) a level takes part while it holds at most c x ef_search x neighbors_count
 * nodes (c = 8 up to ef_search 64, 6 above), level by level from the top (a level's walk evaluates a multiple of ef x M rows per
 * query; the table costs one GEMM column per node): 1M x 768 at ef 64 / M 32 -> levels >= 3 (20 903 columns); a 12.5M x 1024 shard at ef 128 / M 64 -> levels >= 4 (65 161
 * columns, +45 % QPS over a fixed 8 192).  An explicit max_cols caps the columns of all table levels together; 0 = no table.  The
 * operand follows ef_search (cos_index_set_ef_search rebuilds it on the next big launch).
 * The levels are nested (a node of level l + 1 is a node of level l), so the throughput kernel's table has ONE column per vector
 * of level L_t instead of one per (level, node) where that saves 4 096 columns or more (u8 codes up to 1024 dims, no metadata
 * schema, node index and column of a neighbour fit one 32-bit word; tuning knob walk_table_nested): the shard's 65 161 columns
 * become 48 822.  The four-wave kernel keeps the per-level table.  Same integers, same results.
 * A launch holds queries x columns x 4 bytes of table (32 768 x 20 928: 2.7 GB; 32 768 x 65 184: 8.5 GB — 32 768 x 48 832: 6.4 GB
 * with one column per vector); a handle's tables together
 * stay under 48 GiB (tuning knob walk_table_max_bytes): a launch whose workspace would exceed that walks without a table.
 * Device memory of the search side in general: every caller stream (cos_search_batch_device) and every host call in flight
 * (cos_search_batch: up to 32 leased pipes, a lone big call uses up to five workspaces) owns a workspace sized for its largest launch
 * — query codes, per-level result lists ((num_layers + 1) x 100 x 8 B per query: 8 KB at ten levels), statistics, the level table —
 * and keeps it until the handle is destroyed. */
#define COS_WALK_TABLE_DEFAULT_MIN_B 1u
#define COS_WALK_TABLE_DEFAULT_MAX_COLS 8192u /* kept for callers that want the round-4 mid-round default */
#define COS_WALK_TABLE_AUTO 0xFFFFFFFFu
int32_t cos_index_set_walk_table(cos_index *ix, uint32_t max_cols, uint32_t min_queries);
/* the table the next big launch would use: its lowest level and its columns (0, 0 = none; the nested table's columns where the
 * throughput kernel reads that one — a one-client-batch launch on the four-wave kernel then reports more).  Diagnostic: bench.py reports it. */
int32_t cos_index_walk_table_info(cos_index *ix, uint32_t *out_level_min, uint32_t *out_cols);
/* The last completed batch on `stream` split by dispatch, for the roofline report: a big launch is up to three
 * pieces of work with three different bounds — the level-table GEMM (MFMA), the level range above the cut (rows that stay in
 * L2 / the memory-side cache: a gather from cache) and the level range below it (HBM).  Times are HIP events on the streams the
 * kernels ran on (0 without cos_index_enable_timing); counters as in cos_search_stats. */
typedef struct {
    uint32_t struct_size;       /* in: sizeof(cos_walk_split) */
    uint32_t queries;
    uint32_t table_level_min;   /* 0 = the launch used no table */
    uint32_t table_cols;
    uint32_t cut_after_level;   /* 0 = the walk was one dispatch (everything is in `lower`) */
    uint32_t table_early_wgs;   /* workgroups of the GEMM's early part (tuning knob walk_table_early_wgs, clamped); 0 = the GEMM was one launch */
    float table_ms;             /* level-table GEMM: execution time, summed over its launches (the waits in front of them excluded) */
    float upper_ms, sort_ms, lower_ms;
    double table_int8_ops;      /* 2 * queries * cols * padded dims */
    uint64_t table_evals;       /* evaluations the table served (all of them above the cut) */
    uint64_t upper_evals, upper_expansions, upper_adj_bytes; /* levels above the cut, table evaluations included */
    uint64_t lower_evals, lower_expansions, lower_adj_bytes; /* levels below the cut (or the whole walk) */
} cos_walk_split;
int32_t cos_index_last_walk_split(cos_index *ix, void *stream, cos_walk_split *out);
/* The pair walk of the last completed batch on `stream` (tuning knob walk_pair: the levels below the cut of a big launch walked two
 * sorted neighbours per workgroup, which share their integer dots through LDS): how many of that range's evaluations found their dot
 * in the cache, how many fetched a code row, and the cache entries per query.  All three are 0 when the launch did not walk in pairs.
 * Hits depend on how the two waves of a workgroup interleave: they may differ from run to run, results never do. */
typedef struct {
    uint32_t struct_size;       /* in: sizeof(cos_pair_stats) */
    uint32_t cache_entries;
    uint64_t cache_hits, row_evals;
} cos_pair_stats;
int32_t cos_index_last_pair_stats(cos_index *ix, void *stream, cos_pair_stats *out);
/* counters + kernel times of the last completed batch on `stream` (NULL = the host API's stream).  A lone big cos_search_batch call
 * runs as up to four chunk launches (each with its own workspace): with stream == NULL the figures then describe the LAST chunk only
 * (about a quarter of the call's queries; cos_walk_split.queries says how many) — whether a call is chunked depends on what else is
 * in flight on the handle, so callers that want whole-batch counters use cos_search_batch_device on their own stream. */
int32_t cos_index_enable_timing(cos_index *ix, int32_t on);
int32_t cos_index_last_stats(cos_index *ix, void *stream, cos_search_stats *out);
/* HIP-event times of the (up to 128 most recent) launches enqueued on `stream` since cos_index_enable_timing(1):
 * sums / extremes per kernel, read after the fact so the measured launches are never synchronised in between. */
typedef struct {
    uint32_t launches;
    float prep_ms_sum, walk_ms_sum, finalize_ms_sum;
    float walk_ms_min, walk_ms_max;
} cos_timing_summary;
int32_t cos_index_timing_summary(cos_index *ix, void *stream, cos_timing_summary *out);

/* ---- metadata-filtered search ------------------------------------------------ */
/* Collections with a metadata schema index every embedding several times (metadata/mod.rs:128-146, vector_store.rs:484-640):
 * a Base replica under the main root and one Metadata replica per field combination under the PSEUDO root, next to the pseudo
 * nodes created with the index (api_service.rs:135-210).  A search with a Filter starts at the pseudo root and walks that second
 * component once per QueryFilterDimensions with one shared visited filter per level (indexes/hnsw/mod.rs:413-423,
 * vector_store.rs:273-313); the distance depends on the kinds of node and query (distance/cosine.rs:36-102).  Schema -> dimension
 * encoding (metadata/schema.rs, query_filtering.rs) stays on the host; the device takes the numeric form.
 * Ids: an embedding reserves max_replicas_per_node consecutive internal ids (collection.rs:445-468): vector row r has base id
 * r * max_replicas_per_node (also in the BASE graph from now on), replica i = base + i; pseudo root = u32::MAX - 257, pseudo
 * nodes follow it.  Returned ids are replica ids; scores are the exact cosine against the embedding's raw vector. */
int32_t cos_index_enable_metadata(cos_index *ix, uint32_t mdim /* <= 64 */, uint32_t max_replicas_per_node);
/* node table of the pseudo-root component: ascending replica ids (pseudo root and pseudo nodes last), mbits [n_nodes][mdim] */
int32_t cos_index_upload_meta_nodes(cos_index *ix, uint32_t n_nodes, const uint32_t *node_ids, const int32_t *mbits);
/* one level of the component, same conventions as cos_index_upload_graph_level (the pseudo root is on every level) */
int32_t cos_index_upload_meta_graph_level(cos_index *ix, uint32_t level, uint32_t n_nodes, const uint32_t *node_ids,
                                          const uint32_t *nbr_ids);
/* The component BUILT on the device instead of uploaded: index_embedding for the pseudo nodes (ascending id), then for the
 * Metadata replicas (ascending id) of the node table — every level walked from the pseudo root with the node's own metadata
 * dimensions as the filter, keep 64, then create_node_edges with the refusal rules of vector_store.rs:1017-1041 (a Metadata replica
 * links to a pseudo node only on an exact match; two Metadata replicas whose dimensions disagree are not linked) — in the same
 * batch-synchronous schedule as cos_index_build.  max_levels[n_nodes] = the level each node was drawn (the reference draws with
 * thread_rng: replicas from generate_level_probs, pseudo nodes from pseudo_level_probs, metadata/mod.rs:182-209); rows whose
 * metadata dimensions are all zero are Base replicas and stay out of the component.  Replaces the node table and every level. */
int32_t cos_index_build_meta(cos_index *ix, uint32_t n_nodes, const uint32_t *node_ids, const int32_t *mbits, const uint8_t *max_levels,
                             uint32_t batch_size /* 0 = 1024 */);
/* index_embeddings on a LIVE collection with a metadata schema (vector_store.rs:484-640, api_service.rs:135-210), in two calls:
 * cos_index_append adds the embeddings — their Base nodes take the ids (n + i) x max_replicas_per_node and join the base graph as on any
 * collection, and the resident component follows the vector table's growth (the pseudo nodes' vector moves from row n + 1 to row
 * n + m + 1), so filtered search keeps answering over the old replicas — then cos_index_append_meta adds their replica nodes to the
 * component.  node_ids: strictly ascending replica ids of RESIDENT embeddings (id / max_replicas_per_node < n), every one above every
 * replica id of the node table, none in the pseudo range; mbits [n_new][mdim]; max_levels [n_new] as in cos_index_build_meta.  A row
 * whose metadata dimensions are all zero is a Base replica: recorded in the node table, inserted nowhere.  The others are inserted by
 * the schedule of cos_index_build_meta CONTINUED at the number of nodes inserted so far: batches of min(batch_size, max(1, inserted / 4))
 * walk the snapshot that precedes them from the pseudo root with their own dimensions as the filter, then the link kernels run on the
 * link state cos_index_build_meta left on the handle.  The component equals one cos_index_build_meta over the whole table when the
 * earlier calls ended on a batch boundary of that build, and always what the same schedule gives from the resident component.
 *   COS_ERR_NOT_READY: no component built by cos_index_build_meta on this handle (it was uploaded, or never built), or
 *                      cos_index_release_link_state freed its link state.
 *   COS_ERR_INVALID:   one of the rules above is broken, a level is above num_layers, or the visited mode is not COS_VISITED_REF; the
 *                      handle is unchanged and searchable.
 * Exclusive like every graph change.  A failure after the arrays have grown drops the component, as a failed cos_index_build_meta does. */
int32_t cos_index_append_meta(cos_index *ix, uint32_t n_new, const uint32_t *node_ids, const int32_t *mbits, const uint8_t *max_levels,
                              uint32_t batch_size /* 0 = 1024 */);
/* the component back on the host: node count of a level; (node_ids ascending [n_l], nbr_ids [n_l][M_l], COS_SLOT_EMPTY = null slot) */
int32_t cos_index_meta_level_count(cos_index *ix, uint32_t level, uint32_t *out);
int32_t cos_index_download_meta_graph_level(cos_index *ix, uint32_t level, uint32_t *node_ids, uint32_t *nbr_ids);
/* HNSWIndex::search_internal with DenseSearchInput(query, Some(filter)): the filters of query b are rows
 * [filter_offsets[b], filter_offsets[b+1]) of filter_dims[][mdim] (values -1 / 0 / 1, filter_encoded_dimensions'
 * output).  Host buffers; error behaviour as cos_search_batch. */
int32_t cos_search_filtered_batch(cos_index *ix, const float *queries, uint32_t B, const uint32_t *filter_offsets,
                                  const int8_t *filter_dims, uint32_t top_k, uint32_t *out_ids, float *out_scores,
                                  uint32_t *out_counts, int32_t *out_status);
/* the filtered ann_search's per-level lists before finalisation (layout of cos_ann_search_batch) */
int32_t cos_ann_search_filtered_batch(cos_index *ix, const float *queries, uint32_t B, const uint32_t *filter_offsets,
                                      const int8_t *filter_dims, uint32_t *out_ids, float *out_sims, uint32_t *out_counts,
                                      int32_t *out_status);

/* ---- operators (L1 of SURVEY.md §1) --------------------------------------------------------- */
/* QuantizationMetric::quantize (models/types.rs:504) for n vectors; codes in the REFERENCE layout
 * (u8: dim bytes; SubByte: resolution planes x ceil(dim/8) bytes plane-major, plane 0 = MSB;
 * f16: dim x 2; f32: dim x 4), mags[n].  Host buffers. */
int32_t cos_quantize_batch(uint32_t storage, uint32_t resolution, uint32_t dim, float range_lo, float range_hi,
                           const float *x, uint32_t n, void *codes, float *mags);
size_t cos_code_bytes(uint32_t storage, uint32_t resolution, uint32_t dim);
/* "auto" quantization: HNSWIndex::sample_embedding + finalize_sampling (indexes/hnsw/mod.rs:202-351) over the
 * first sample_threshold embeddings: the range is the first of +-{.025,.05,.1,.2,.3,.4,.5} whose tail holds at
 * most clamp_margin_percent (config.toml:38, default 1.0) of all sampled values, else +-1.0.  Host buffer. */
int32_t cos_sample_values_range(const float *x, uint32_t n, uint32_t dim, float clamp_margin_percent, float *range_lo,
                                float *range_hi);
/* DistanceMetric::calculate (models/types.rs:469) for explicit (x_i, y_j) pairs of stored vectors
 * in the reference layout: out[p] = metric(x[pair_x[p]], y[pair_y[p]]); status[p] per pair. */
int32_t cos_distance_batch(uint32_t metric, uint32_t storage, uint32_t resolution, uint32_t dim, const void *x_codes,
                           const float *x_mags, uint32_t nx, const void *y_codes, const float *y_mags, uint32_t ny,
                           const uint32_t *pair_x, const uint32_t *pair_y, uint32_t n_pairs, float *out,
                           int32_t *status);
/* exact brute-force cosine top-k on the resident raw vectors (ground truth for recall@k):
 * MFMA f32 GEMM for candidate generation + reference-order re-score of the survivors.
 * k in [1, min(512, n)], anything else is COS_ERR_INVALID.  A query keeps a pool of P survivors, the smallest of
 * 64, 128, 256, 512, 1024 with 2k <= P (the GEMM's summation order differs from the reference's in the last ulp:
 * it only generates candidates).  The pool is trusted only where its P-th GEMM score lies more than twice a derived
 * error bound under its k-th (cosdata_amd/csrc/flat_plan.h brute_margin_safe); a query that fails the rule — more than
 * P - k rows within the scores' error of the k-th: copies and scaled copies of one vector — has every row scored in the
 * reference's order instead, n * dim fused multiply-adds on the vector units for that query, so the answer is the
 * reference's bit for bit on such corpora too.  cos_index_last_brute_stats says how many queries that was.
 * Device memory of a call beyond the score chunk, per query: 8 P bytes of pool,
 * up to 512 P bytes of per-segment partial pools (fewer for batches above 64 queries) and, above 16384 vectors, the
 * append buffer of the threshold-filtered scan: 32 KB at P = 64, 256 P bytes (32 KB .. 256 KB) at P >= 128. */
int32_t cos_bruteforce_topk(cos_index *ix, const float *queries, uint32_t B, uint32_t k, uint32_t *out_ids,
                            float *out_scores);
/* The last cos_bruteforce_topk / cos_bruteforce_topk_masked on this handle (a shard set's brute force counts as one per shard):
 * all zero before the first.  out->struct_size must be sizeof(cos_brute_stats) on entry, anything else is COS_ERR_INVALID. */
typedef struct cos_brute_stats {
    uint32_t struct_size;   /* in: sizeof(cos_brute_stats) */
    uint32_t queries;       /* B of the call */
    uint32_t exact_queries; /* queries answered by the exact path: those the margin rule flagged (every one with tuning knob
                             * flat_brute_exact = 2, none with 0) */
    uint32_t pool;          /* P */
} cos_brute_stats;
int32_t cos_index_last_brute_stats(cos_index *ix, cos_brute_stats *out);

/* Exhaustive search over the index's QUANTIZED codes as an exact-integer MFMA GEMM, then the reference's finalisation on the full candidate set: sort by quantized score (desc, larger id
 * first), keep 5k, exact f32 rerank (vector_store.rs:404-445), top-k.  The result is what
 * ann_search + finalize_ann_results would return if the walk visited every node: config c3's flat scan and
 * the exhaustive per-shard mode.  Host buffers.
 * Storages: UnsignedByte and SubByte of resolution 1 (binary), 2 (quaternary) and 3 (octal): their reference dots are integers, exact
 * in any summation order (dot_product_u8 / _binary / _quaternary / _octal), so the candidate set is the reference's bit for bit.
 * HalfPrecisionFP and FullPrecisionFP indexes: COS_ERR_UNIMPLEMENTED (their reference dots are order-dependent f32 chains; the handle
 * stays usable — cos_bruteforce_topk scans the raw rows of any index).  Cosine divides by the norms the quantizer keeps (SubByte: of the
 * original vector), and a zero norm among the queries or the stored vectors is COS_ERR_CALCULATION for the call.
 * top_k in [1, 204]; above that COS_ERR_UNIMPLEMENTED (the handle stays usable).  A query keeps a pool of P
 * survivors, the smallest of 64, 128, 256, 512, 1024 with 5 * top_k <= P: top_k <= 12 runs the 64-key kernels,
 * 13..25 P = 128, 26..51 P = 256, 52..102 P = 512, 103..204 P = 1024.  The index's workspace grows to the widest call
 * it has served and stays until the index is destroyed or its vectors are replaced; per query it holds 8 P bytes of pool,
 * up to 512 P bytes of per-segment partial pools (fewer for batches above 64 queries) and the append buffer of the
 * threshold-filtered scan: 32 KB at P = 64, 256 P bytes at P >= 128 (32 KB at top_k 13..25 up to 256 KB at
 * top_k 103..204: 64 MB for a 256-query call).  A call indexes the workspace by its own P: a narrow call after a wide
 * one returns the bits it returned before. */
typedef struct {
    float gemm_ms;          /* summed HIP-event time of the i8 MFMA GEMM launches */
    uint32_t gemm_launches;
    double int8_ops;        /* 2 * B * n * padded_dim (the dims multiplied: the stored row's dims rounded up to 64) */
    double code_bytes;      /* bytes of codes streamed from HBM (n * row bytes * query-tile rows) */
} cos_flat_stats;
int32_t cos_flat_search_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, uint32_t *out_ids,
                              float *out_scores, uint32_t *out_counts, cos_flat_stats *stats /* optional */);

/* The two exhaustive scans over a SUBSET of the rows: per-query allow-lists and / or the handle's deleted set.
 * Query q's live set is mask query_mask[q] AND NOT the deleted rows (COS_SCAN_SKIP_DELETED); its result is exactly what the unmasked
 * call returns on an index that holds only those rows, with the original ids — the reference's finalisation (sort by quantized score,
 * keep 5 * top_k, exact rerank, top_k) over the live rows, which dropping ids from an unmasked result cannot give.  The test is applied
 * inside the scan kernels where a candidate is about to be kept; the masks are read on the host once per call.
 *   out_counts[q] = min(top_k, live rows of q) (required in both calls); entries past the count are unspecified.  The brute force keeps
 *   its rule k in [1, min(512, n)]: k may exceed a query's live rows.
 *   Bits at and past n in a mask's last word are ignored.
 *   mask == NULL, or n_masks == 0 with flags == 0: the unmasked call — the same kernels, the same bits.
 *   Zero norms (cosine, code scan): COS_ERR_CALCULATION iff a query has zero norm or a row that is live for at least one query of the
 *   call has; a zero-norm row no query can see does not fail the call (the unmasked entry point keeps its rule).
 *   COS_ERR_INVALID: struct_size mismatch, unknown flags, bits == NULL with n_masks > 0, query_mask == NULL with n_masks > 1, a
 *   query_mask entry >= n_masks.  COS_ERR_UNIMPLEMENTED: f16 / f32 storage and top_k > 204 in the code scan, as in the unmasked call.
 *   The handle stays usable after every refusal.
 * The deleted set is a device bitmap on the handle, n / 8 bytes, always kept: cos_index_delete sets the bit of every id it is given
 * (whether or not its walk found the node; a repeated id is harmless), cos_index_append grows it (new rows are live), every upload
 * that replaces the vectors clears it. */
#define COS_SCAN_SKIP_DELETED 1u
typedef struct cos_scan_mask {
    uint32_t struct_size;        /* sizeof(cos_scan_mask) */
    uint32_t flags;              /* COS_SCAN_SKIP_DELETED: rows given to cos_index_delete are not returned */
    uint32_t n_masks;            /* 0 = no allow-list (every row, minus the deleted ones if flagged) */
    const uint32_t *bits;        /* HOST [n_masks][ceil(n / 32)]: bit (r % 32) of word r / 32 = ROW r (id - id_base) may be returned */
    const uint32_t *query_mask;  /* HOST [B] -> mask index; NULL = every query uses mask 0 (then n_masks must be 1) */
} cos_scan_mask;
int32_t cos_flat_search_masked_batch(cos_index *ix, const float *queries, uint32_t B, uint32_t top_k, const cos_scan_mask *mask,
                                     uint32_t *out_ids, float *out_scores, uint32_t *out_counts, cos_flat_stats *stats /* optional */);
int32_t cos_bruteforce_topk_masked(cos_index *ix, const float *queries, uint32_t B, uint32_t k, const cos_scan_mask *mask,
                                   uint32_t *out_ids, float *out_scores, uint32_t *out_counts);
/* rows in the deleted set; the set itself, HOST bits[ceil(n / 32)] in the layout of cos_scan_mask::bits (a set bit = deleted) */
int32_t cos_index_deleted_count(cos_index *ix, uint32_t *out);
int32_t cos_index_download_deleted(cos_index *ix, uint32_t *bits);

/* ---- hybrid (config c5) --------------------------------------------------------------------- */
typedef struct cos_bm25 cos_bm25;
/* TFIDFIndexRoot postings as CSR (models/tf_idf_index.rs, versioned_vec.rs:208-224): term hashes
 * ascending, offsets[T+1], (doc_id, stored tf) doc-id ascending within a term. */
int32_t cos_bm25_create(int32_t device, const uint32_t *term_hashes, const uint64_t *offsets, uint32_t n_terms,
                        const uint32_t *doc_ids, const float *tfs, uint32_t documents_count, cos_bm25 **out);
int32_t cos_bm25_destroy(cos_bm25 *b);
/* ---- updates of the resident postings ---------------------------------------------------------
 * The postings stay on the device: the host passes the update, the library keeps the term table.  Every call below takes the
 * handle's lock and waits for the handle's streams, so a search on another thread sees the index before or after an update, never
 * between.  Strong guarantee: a call that fails (bad argument, or hipErrorOutOfMemory while the new arrays are allocated) leaves
 * the handle exactly as it was, and usable.
 *
 * TFIDFIndex::insert (indexes/tf_idf/mod.rs:85-110; TFIDFIndexNode::insert models/tf_idf_index.rs:212-240, VersionedVec::push_sorted
 * models/versioned_vec.rs:205-222) for m documents in document-major form — what cos_text_process gives per document:
 * term_hashes / tfs [doc_offsets[i], doc_offsets[i+1]) belong to doc_ids[i].  (doc id, tf) goes to the END of each term's list, a new
 * term gets a list, documents_count += m.  doc_ids strictly ascending and all above every id the index has ever held, term hashes
 * distinct within a document, tfs finite (else COS_ERR_INVALID); m == 0 succeeds and does nothing.
 * Peak device memory during the call: old arrays + new arrays (8 B per posting each, plus the two tile directories) + the update
 * itself (about 40 B per posting of the update, the sort's workspace included) + 16 B per term. */
int32_t cos_bm25_insert(cos_bm25 *b, const uint32_t *doc_ids, const uint64_t *doc_offsets, uint32_t m, const uint32_t *term_hashes,
                        const float *tfs);
/* TFIDFIndex::mark_embedding_as_deleted (indexes/tf_idf/mod.rs:112-141; TFIDFIndexNode::delete models/tf_idf_index.rs:242-266,
 * VersionedVec::delete models/versioned_vec.rs:131-150) for m documents given with the term hashes of their text:
 * documents_count -= m (once per document, found or not; documents_count < m is COS_ERR_INVALID with nothing changed), and for
 * every (document, term) the entry of that term's list with this id becomes a tombstone: skipped by every search
 * (versioned_vec.rs:251-275), still counted in the list's length that get_idf sees, never compacted.  A term without a list, or a
 * list without the id (second delete), is left alone. */
int32_t cos_bm25_delete(cos_bm25 *b, const uint32_t *doc_ids, const uint64_t *doc_offsets, uint32_t m, const uint32_t *term_hashes);
typedef struct {
    uint32_t struct_size;     /* in: sizeof(cos_bm25_index_stats) */
    uint32_t documents_count; /* TFIDFIndexRoot::total_documents_count: what the idf uses */
    uint32_t n_terms;
    uint32_t largest_doc_id;  /* the largest document id the index has ever held (0 when it has held none) */
    uint32_t dir_rows;        /* lists long enough for a row of the tile directory */
    uint32_t dir_tiles;       /* tiles of 8192 document ids the directory spans */
    uint32_t reserved;
    uint64_t postings;        /* tombstones included */
    uint64_t tombstones;
    uint64_t device_bytes;    /* postings, tile directory and the search workspace */
} cos_bm25_index_stats;
int32_t cos_bm25_stats(cos_bm25 *b, cos_bm25_index_stats *out);
/* The index as the CSR cos_bm25_create takes, plus one flag per posting (1 = tombstone; its tf comes back as 0).  Two calls: with the
 * five arrays NULL, *n_terms / *n_postings receive the sizes; with the arrays (term_hashes[T], offsets[T+1], doc_ids / tfs /
 * tombstones [postings]) they carry the capacities in and the sizes out (too small: COS_ERR_INVALID, nothing written).  An index
 * that holds tombstones is restored by cos_bm25_create from these arrays followed by ONE cos_bm25_delete of the flagged (document,
 * term) pairs, with documents_count passed to create so that it ends right. */
int32_t cos_bm25_download(cos_bm25 *b, uint32_t *n_terms, uint64_t *n_postings, uint32_t *term_hashes, uint64_t *offsets,
                          uint32_t *doc_ids, float *tfs, uint8_t *tombstones);
/* SparseAnnQueryBasic::search_bm25 (models/sparse_ann_query.rs:149) for B queries given as
 * pre-hashed terms (CSR q_offsets[B+1] into q_terms); outputs [B][top_k]. */
int32_t cos_bm25_search_batch(cos_bm25 *b, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B,
                              uint32_t top_k, uint32_t *out_ids, float *out_scores, uint32_t *out_counts);
/* Same scoring with the results left in DEVICE memory (d_out_* : [B][top_k], [B][top_k], [B]) and the kernels enqueued on
 * `stream` (NULL = the handle's own stream, asynchronous): the BM25 half of a hybrid batch can run next to the dense half and
 * feed a fusion stage without a round trip through the host.  q_terms / q_offsets are host arrays (the term lookup and the
 * idf use host tables, like the reference's radix tree walk). */
int32_t cos_bm25_search_batch_device(cos_bm25 *b, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B, uint32_t top_k,
                                     uint32_t *d_out_ids, float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* RRF fusion of hybrid_search (api/vectordb/search/repo.rs:311-340) for B queries. */
int32_t cos_rrf_fuse_batch(const uint32_t *dense_ids, const uint32_t *dense_counts, uint32_t dense_stride,
                           const uint32_t *sparse_ids, const uint32_t *sparse_counts, uint32_t sparse_stride, uint32_t B,
                           float fusion_constant_k, uint32_t top_k, uint32_t *out_ids, float *out_scores,
                           uint32_t *out_counts);

/* repo::hybrid_search (api/vectordb/search/repo.rs:168-341) in one call: dense top_k*3 (walk + exact rerank) and BM25 top_k*3
 * run concurrently on two streams of the device both indexes live on, RRF fuses them there (fusion_constant_k: dtos.rs:10-12,
 * default 60); host buffers in, fused [B][top_k] out.  A failing dense query fails the call like cos_search_batch. */
int32_t cos_hybrid_search_batch(cos_index *ix, cos_bm25 *b, const float *queries, const uint32_t *q_terms, const uint32_t *q_offsets,
                                uint32_t B, uint32_t top_k, float fusion_constant_k, uint32_t *out_ids, float *out_scores,
                                uint32_t *out_counts);

/* ---- text -> BM25 terms (host code, no device needed) -------------------------- */
/* TFIDFIndex's text side: tokenize (indexes/tf_idf/mod.rs:288-308), STOPWORDS (:282-286), process_text (:310-360: tokens longer
 * than max_token_len bytes skipped, lowercase, stopwords, stem, xxhash32 seed 0, count per hash), compute_bm25_term_frequency
 * (:362-371), count_tokens (:373-389).  The stemmer is the reference's un-vendored git dependency: `stem` is the host's shim over
 * it — (ctx, token, token_len, out, out_cap) -> bytes written; NULL hashes the lowercased token unstemmed.  Terms come out by
 * ascending hash (the reference: FxHashMap order); *out_n = distinct terms (also set when cap is too small -> Invalid). */
typedef size_t (*cos_stem_fn)(void *ctx, const char *token, size_t token_len, char *out, size_t out_cap);
int32_t cos_text_process(const char *utf8, size_t len, uint32_t max_token_len, float average_document_length, float k1, float b,
                         cos_stem_fn stem, void *stem_ctx, uint32_t *out_hashes, float *out_tfs, uint32_t cap, uint32_t *out_n);
uint32_t cos_text_count_tokens(const char *utf8, size_t len, uint32_t max_token_len);
float cos_bm25_term_frequency(uint32_t count, uint32_t document_length, float average_document_length, float k1, float b);
uint32_t cos_xxhash32(const void *data, size_t len, uint32_t seed); /* twox-hash XxHash32 (indexes/tf_idf/mod.rs:343-345) */
/* The English Snowball stemmer ("Porter2") as a cos_stem_fn: pass it as `stem` to cos_text_process to get process_text's
 * `Stemmer::create()` + `stemmer.stem(&lower)` (indexes/tf_idf/mod.rs:317-340) without a host-side shim.  Restated from the
 * published algorithm the reference's git dependency (snowball-stemmer 0.1.0 @ dcbd7da, Cargo.lock:2571-2573) ports; pinned by
 * the algorithm's sample vocabulary, not by that crate (its source is not available).  ctx is ignored; returns the byte length
 * of the stem and writes at most out_cap bytes. */
size_t cos_stem_english(void *ctx, const char *token, size_t token_len, char *out, size_t out_cap);

/* ---- learned-sparse inverted index ----------------------------------------- */
typedef struct cos_sparse cos_sparse;
/* InvertedIndexRoot as CSR (models/inverted_index.rs): dims[n_dims] ascending; for dimension t and quantized key q in
 * [0, 2^bits) the vector ids vec_ids[key_offsets[t*(2^bits+1)+q] .. key_offsets[t*(2^bits+1)+q+1]) (one list per
 * (dimension, key), as InvertedIndexNode::insert files them, inverted_index.rs:176-200); posting ranges of consecutive
 * dimensions are contiguous.  Optional raw sparse vectors as CSR (row_offsets[n_vectors+1], dims ascending per row) for
 * finalize_sparse_ann_results' raw-value rerank; pass NULLs without it. */
int32_t cos_sparse_create(int32_t device, uint32_t quantization_bits, float values_upper_bound, const uint32_t *dims, uint32_t n_dims,
                          const uint64_t *key_offsets, const uint32_t *vec_ids, uint32_t n_vectors, const uint64_t *row_offsets,
                          const uint32_t *raw_dims, const float *raw_vals, cos_sparse **out);
/* InvertedIndex::insert for a whole collection (models/inverted_index.rs:168-200): vectors in id order, every (dimension, value) pair
 * pushes the id to the end of the list of (dimension, quantize(value)).  Host code, no device.  Call once with the three output arrays
 * NULL to get *n_dims (the posting count is row_offsets[n_vectors]), then with out_dims[*n_dims], out_key_offsets[*n_dims * (2^bits + 1)],
 * out_vec_ids[nnz]. */
int32_t cos_sparse_build_csr(uint32_t quantization_bits, float values_upper_bound, uint32_t n_vectors, const uint64_t *row_offsets,
                             const uint32_t *raw_dims, const float *raw_vals, uint32_t *out_dims, uint64_t *out_key_offsets,
                             uint32_t *out_vec_ids, uint32_t *n_dims);
/* cos_sparse_build_csr + cos_sparse_create; keep_raw != 0 keeps the raw vectors on the device for the raw-value rerank. */
int32_t cos_sparse_create_from_vectors(int32_t device, uint32_t quantization_bits, float values_upper_bound, uint32_t n_vectors,
                                       const uint64_t *row_offsets, const uint32_t *raw_dims, const float *raw_vals, int32_t keep_raw,
                                       cos_sparse **out);
int32_t cos_sparse_destroy(cos_sparse *s);
/* InvertedIndex::search_internal (indexes/inverted/mod.rs:278-331) -> SparseAnnQueryBasic::sequential_search
 * (models/sparse_ann_query.rs:68-147) for B queries given as CSR pairs (q_offsets[B+1] into q_dims / q_vals).
 * reranking_factor = 0: config.rerank_sparse_with_raw_values = false -> scores are the quantized similarities as f32;
 * otherwise the best top_k * reranking_factor candidates are re-scored with the raw values and sorted.
 * top_k * max(reranking_factor, 1) above the handle's cos_sparse_set_max_candidates (64 unless set) is COS_ERR_UNIMPLEMENTED and
 * leaves the handle usable.
 * Order: score descending, larger id first (the reference leaves the order of equal / unranked entries to its hash map). */
int32_t cos_sparse_search_batch(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, uint32_t B,
                                uint32_t top_k, float early_terminate_threshold, uint32_t reranking_factor, uint32_t *out_ids,
                                float *out_scores, uint32_t *out_counts);

/* Widest candidate set, top_k * max(reranking_factor, 1), a search on this handle may keep.  Default 64.
 * Accepted 1..1024, rounded up to 64, 128, 256, 512 or 1024; 0 or > 1024 -> COS_ERR_INVALID, handle unchanged.
 * Takes the handle's lock (a search on another thread runs before or after).  Kept across
 * cos_sparse_insert / cos_sparse_delete.
 * The setting only admits wider calls; every call picks its kernels by its own width: up to 64 candidates run exactly what a
 * default handle runs, (32 R, 64 R] candidates run the instantiation R = 2, 4, 8, 16 with pools of 64 R keys.  What a wide call
 * costs beside time is the grow-only workspace: B * splits * 64 R * 8 bytes of partial results (B * splits is about 4096 for
 * B <= 4096: 34 MB at R = 16), kept until the handle is destroyed. */
int32_t cos_sparse_set_max_candidates(cos_sparse *s, uint32_t max_candidates);
int32_t cos_sparse_max_candidates(cos_sparse *s, uint32_t *out);   /* the rounded value */

/* Figures of the most recent cos_sparse_search_batch on this handle: HIP-event time of its kernels, and the postings the
 * reference's traversal visits for that batch (sparse_ann_query.rs:92-125: every list of a term from its first visited key on;
 * 4 B each — SURVEY.md §8d counts algorithmic bytes, not what the device layout happens to read). */
typedef struct cos_sparse_stats {
    float kernel_ms;
    uint32_t blocks;
    uint64_t postings_visited;
    uint64_t posting_bytes;
} cos_sparse_search_stats; /* (the plain name cos_sparse_stats is the function further down: in C say `struct cos_sparse_stats`) */
int32_t cos_sparse_last_stats(cos_sparse *s, cos_sparse_search_stats *out);
/* Device layout of the handle's postings: 0 = a u32 id + a u8 key per posting (5 B), 1 = one packed u32 per posting
 * (key << 24 | id + 1; what cos_sparse_create builds whenever the collection holds fewer than 2^24 - 16384 vectors: measured in
 * round 5 at 0.453 ms against 0.540 ms per 256-query batch; tuning knob sparse_layout = 0 keeps the 5-byte layout).  Same results
 * either way; a tuning choice, not a reference interface. */
int32_t cos_sparse_layout(cos_sparse *s, uint32_t *packed);
/* ---- updates of the resident postings ---------------------------------------------------------
 * The postings stay on the device: the host passes the update, the library keeps the dimension table and the per-(dimension, key)
 * counts.  Every call below takes the handle's lock (the one cos_sparse_search_batch holds from the resolution of its terms to its
 * results) and waits for the device, so a search on another thread sees the index before or after an update, never between.
 * Strong guarantee: every allocation and kernel of a call completes before the handle's pointers and host tables are swapped; a
 * call that fails (bad argument, hipErrorOutOfMemory) leaves the handle exactly as it was, and usable.  Host work per call is
 * O(update + n_dims * 2^bits), never O(postings).
 *
 * InvertedIndex::insert (indexes/inverted/mod.rs:72-89; InvertedIndexRoot::insert models/inverted_index.rs:273-289,
 * InvertedIndexNode::insert :176-201) for m more vectors, which take the ids [n, n + m) (sequential, like cos_index_append);
 * *out_first_id (optional) = n before the call.  The pairs of vector i are raw_dims / raw_vals [row_offsets[i], row_offsets[i+1]):
 * every pair, zero values included, pushes the id to the END of the list of (dimension, quantize(value)); a dimension never seen
 * gets a list; a vector without pairs still takes an id.  row_offsets[0] == 0 and non-decreasing, n + m must fit 32 bits (else
 * COS_ERR_INVALID), at most 2^31 - 1 pairs per call; any f32 value is accepted (quantized as cos_sparse_build_csr quantizes it);
 * m == 0 succeeds and does nothing.  On a handle created with raw vectors the raw CSR grows by the same rows, and the dimensions of
 * a row must strictly ascend (the rerank's lookup is a binary search), else COS_ERR_INVALID.  On the packed layout
 * (cos_sparse_layout) n + m > 2^24 - 16384 is COS_ERR_UNIMPLEMENTED with the handle unchanged: a packed handle is not converted to
 * the unpacked layout; create the index with the tuning knob sparse_layout = 0 when it is meant to grow past that.
 * Peak device memory during the call: old + new posting arrays (4 B per posting packed, 5 B unpacked, each) + the two tile
 * directories + about 44 B per pair of the update (the sort's workspace included) + 16 B per dimension; with raw vectors also the
 * old and the new raw CSR (8 B per pair + 8 B per vector each). */
int32_t cos_sparse_insert(cos_sparse *s, uint32_t m, const uint64_t *row_offsets, const uint32_t *raw_dims, const float *raw_vals,
                          uint32_t *out_first_id);
/* InvertedIndex::mark_embedding_as_deleted (indexes/inverted/mod.rs:91-108; InvertedIndexRoot::delete models/inverted_index.rs:291-306,
 * InvertedIndexNode::delete :205-222, VersionedVec::delete models/versioned_vec.rs:131-154).  The pairs of ids[i] are raw_dims /
 * raw_vals [row_offsets[i], row_offsets[i+1]): what the host's raw embedding holds (delete_embedding passes raw_emb.sparse_values).
 * For every pair the FIRST posting of the id in the list of (dimension, quantize(value)) is removed; *out_removed (optional) =
 * postings actually removed.  Ids in any order; ids >= n, unknown dimensions, a key without a list and a list without the id
 * (second delete) are not errors: nothing is removed.  k pairs of one call that name the same (id, dimension, key) remove k such
 * postings.  A pair whose value quantizes to another key than the stored one removes nothing (the reference's rule).  Dimensions
 * are never dropped from the table, even when every list of one is empty; the raw rows of a deleted vector stay (only candidates
 * are ever reranked).  The reference marks a tombstone that every reader skips and nothing else of a list enters a score; here the
 * posting is removed (stream compaction into new arrays), which no search can tell apart — so a call streams the index once:
 * pass the ids of a transaction together.  A call that finds nothing swaps nothing.
 * Peak device memory during the call: old + new posting arrays + 1 B per 4 postings (claim flags and their prefix sums) + 21 B
 * per pair + the two tile directories. */
int32_t cos_sparse_delete(cos_sparse *s, const uint32_t *ids, const uint64_t *row_offsets, uint32_t m, const uint32_t *raw_dims,
                          const float *raw_vals, uint64_t *out_removed);
typedef struct {
    uint32_t struct_size; /* in: sizeof(cos_sparse_index_stats) */
    uint32_t n_vectors;   /* ids handed out so far: the next insert starts here */
    uint32_t n_dims;      /* dimensions in the table (those whose lists are all empty included) */
    uint32_t dir_rows;    /* lists long enough (> 256 postings) for a row of the tile directory */
    uint32_t dir_tiles;   /* tiles of 8192 vector ids the directory spans */
    uint32_t packed;      /* cos_sparse_layout */
    uint32_t have_raw;    /* raw vectors kept for the raw-value rerank */
    uint32_t reserved;
    uint64_t postings;    /* live postings (removed ones are gone) */
    uint64_t removed;     /* postings removed by cos_sparse_delete since create */
    uint64_t raw_pairs;   /* pairs of the raw CSR */
    uint64_t device_bytes; /* postings, tile directory, raw vectors and the search workspace */
} cos_sparse_index_stats;
int32_t cos_sparse_stats(cos_sparse *s, cos_sparse_index_stats *out);
/* The index as the CSR cos_sparse_create takes.  Two calls: with the three arrays NULL, *n_dims / *n_postings receive the sizes; with
 * the arrays (dims[T], key_offsets[T * (2^bits + 1)], vec_ids[postings]) they carry the capacities in and the sizes out (too small:
 * COS_ERR_INVALID, nothing written).  Ids ascend inside every (dimension, key) list — push order whenever the index was built by
 * inserts; a caller-chosen order inside a key list at create is not preserved (no score depends on it).  A persistence / test path:
 * the posting arrays are copied back and split by key on the host. */
int32_t cos_sparse_download(cos_sparse *s, uint32_t *n_dims, uint64_t *n_postings, uint32_t *dims, uint64_t *key_offsets,
                            uint32_t *vec_ids);

/* ---- hybrid search, all three arms, mixed per query --------------------------------------------
 * repo::batch_hybrid_search (api/vectordb/search/repo.rs:343-555) in one call: every query of the request names its own arm,
 * the queries are split into a dense, a learned-sparse and a BM25 sub-batch, the three batch searches run side by side on three
 * streams of one device, each for top_k * 3 and only for its own sub-batch (a DENSE_BM25 query costs no sparse work), and every
 * query's two lists are fused with RRF on the device; only the fused top_k crosses PCIe.  The library builds the reference's
 * query_mapping itself (:366-419): a query's lists are the next free rows of the sub-batches it joins, in request order.
 *
 * Lists: the FIRST and SECOND list of an arm are (dense, sparse), (dense, BM25) and (sparse, BM25).  The order matters: an id's
 * score from the first list is overwritten by a later occurrence of the id in the first list (`insert`), second-list scores
 * are added (:524-537).  score = 1 / (rank as f32 + fusion_constant_k + f32::EPSILON) in f32.  Output: fused score descending
 * (total_cmp), larger id first on ties, truncated to top_k; entries past out_counts[q] are NOT written.
 *
 * Shared id space: fusion is on the u32 ids the three searches return (dense ids include id_base).  The three indexes of a
 * collection share ONE internal id space — document id = vector id = id_base + dense internal id — as cos_hybrid_search_batch
 * already assumes; the library cannot check it.
 *
 * Sparse threshold: one per call.  batch_hybrid_search drops the per-query threshold and passes None, which becomes the
 * config default (:447, indexes/inverted/mod.rs:296-297).  The single-query hybrid_search (:168-341), which does take a
 * threshold, is this call with B = 1.
 *
 * Handles: a handle whose sub-batch is empty may be NULL; one that is needed and NULL, handles on different devices or on a
 * device other than h's are COS_ERR_INVALID.  Locks are taken in the order cos_hybrid -> cos_sparse -> cos_bm25 and each is held
 * until the call's one synchronisation, so searches and updates on the same handles from other threads run before or after.
 *
 * Refused before anything is enqueued, every handle staying usable: top_k > 170 (3 * top_k > 512: BM25 keeps 512 buckets per
 * query, the fusion holds two lists of at most 1024 ids together) -> COS_ERR_UNIMPLEMENTED; 3 * top_k * max(reranking_factor, 1)
 * above the sparse handle's cos_sparse_set_max_candidates -> COS_ERR_UNIMPLEMENTED; a rerank on a sparse handle without raw
 * vectors -> COS_ERR_NOT_READY; B == 0, top_k == 0, an arm above 2, decreasing offsets, a small struct_size -> COS_ERR_INVALID;
 * a sparse sub-batch at or above cos_sparse_search_batch's own bound on B is refused as that call refuses it.
 * A failing dense query (zero norm -> COS_ERR_CALCULATION) fails the call like cos_hybrid_search_batch: the status of the first
 * failing query in request order is returned, and the next call on the same handles answers. */
typedef struct cos_hybrid cos_hybrid;   /* streams, events, pinned staging and device buffers of the fused call; one call at a time */
int32_t cos_hybrid_create(int32_t device, cos_hybrid **out);
int32_t cos_hybrid_destroy(cos_hybrid *h);

enum { COS_HYBRID_DENSE_SPARSE = 0, COS_HYBRID_DENSE_BM25 = 1, COS_HYBRID_SPARSE_BM25 = 2 };

typedef struct cos_hybrid_request {
    uint32_t struct_size;               /* sizeof(cos_hybrid_request) */
    uint32_t B;                         /* queries of the request */
    const uint8_t *arm;                 /* [B] COS_HYBRID_* */
    const float *dense_queries;         /* [n_dense][dim]: vectors of the queries whose arm has a dense half, in query order */
    const uint32_t *sparse_dims;        /* CSR over the n_sparse queries whose arm has a sparse half, in query order: */
    const float *sparse_vals;           /*   pairs [sparse_offsets[i], sparse_offsets[i+1]) of sparse query i               */
    const uint32_t *sparse_offsets;     /*   [n_sparse + 1] */
    const uint32_t *bm25_terms;         /* CSR over the n_bm25 queries whose arm has a BM25 half, in query order: hashed terms */
    const uint32_t *bm25_offsets;       /*   [n_bm25 + 1] */
    float sparse_early_terminate_threshold; /* one per call, as cos_sparse_search_batch takes it */
    uint32_t sparse_reranking_factor;   /* 0 = no raw-value rerank */
    uint32_t top_k;
    float fusion_constant_k;            /* dtos.rs:10-12, default 60 */
} cos_hybrid_request;

/* n_dense, n_sparse and n_bm25 are what arm[] implies; the arrays of a half without queries may be NULL.  Host outputs:
 * out_ids / out_scores [B][top_k], out_counts [B]. */
int32_t cos_hybrid_search_mixed(cos_hybrid *h, cos_index *ix, cos_sparse *sp, cos_bm25 *bm, const cos_hybrid_request *rq,
                                uint32_t *out_ids, float *out_scores, uint32_t *out_counts);

/* cos_sparse_search_batch with the results left in DEVICE memory (d_out_ids / d_out_scores [B][top_k], d_out_counts [B]) and the
 * copies and kernels enqueued on `stream` (NULL = the default stream, where cos_sparse_search_batch launches) without
 * synchronising it: the sparse half of a hybrid batch runs beside the other halves and feeds the fusion without a round trip.
 * The query CSR is host memory (find_node, the quantization and the early-termination rule use host tables); it is resolved into
 * pinned staging the handle owns, so the caller's arrays are free as soon as the call returns.  One batch is in flight per handle:
 * a call waits for the handle's previous batch (an event) before it overwrites the staging or the workspace, and holds the
 * handle's lock while the host tables are read.  Same limits and statuses as cos_sparse_search_batch; cos_sparse_last_stats
 * afterwards waits for the batch and reports it. */
int32_t cos_sparse_search_batch_device(cos_sparse *s, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, uint32_t B,
                                       uint32_t top_k, float early_terminate_threshold, uint32_t reranking_factor,
                                       uint32_t *d_out_ids, float *d_out_scores, uint32_t *d_out_counts, void *stream);

/* ---- multi-GPU helper ----------------------------------------------------------------------- */
/* S-way merge of per-shard top-k lists gathered by the caller's RCCL all-gather
 * (SURVEY.md §8e): in [S][B][k] -> out [B][k], total_cmp desc, larger id first on ties.
 * All pointers device memory; enqueued on stream. */
int32_t cos_merge_topk_device(const uint32_t *d_ids, const float *d_scores, const uint32_t *d_counts, uint32_t S,
                              uint32_t B, uint32_t k, uint32_t *d_out_ids, float *d_out_scores,
                              uint32_t *d_out_counts, int32_t device, void *stream);

/* Same merge over S packed per-shard records, each B*(2k+1) 4-byte words laid out
 * [ids B*k | scores B*k (f32 bits) | counts B] — the layout that lets the caller exchange a shard's
 * whole result with ONE all-gather per batch instead of three. */
int32_t cos_merge_topk_packed_device(const uint32_t *d_packed, uint32_t S, uint32_t B, uint32_t k,
                                     uint32_t *d_out_ids, float *d_out_scores, uint32_t *d_out_counts,
                                     int32_t device, void *stream);

/* The same two merges for up to 8192 keys per query (8 shards x brute-force k 512 = 4096, 8 x flat top_k 204 = 1632), under the same
 * contract word for word: total_cmp score descending (+0.0 ahead of -0.0), larger id first; only the first counts[s][q] entries of a list
 * are read; the lists may be in any order; out_counts[q] = min(sum of counts, k); output slots past the count are not written.
 * S * k <= 1024 launches the kernel of cos_merge_topk_device (one wave per query, the keys in registers: the same bits); 1025 .. 8192 runs
 * one workgroup per query with the keys in 2048, 4096 or 8192 words of LDS; S * k > 8192 is COS_ERR_UNIMPLEMENTED with nothing written.
 * (cos_merge_topk_device / cos_merge_topk_packed_device keep refusing S * k > 1024.) */
int32_t cos_merge_lists_device(const uint32_t *d_ids, const float *d_scores, const uint32_t *d_counts, uint32_t S,
                               uint32_t B, uint32_t k, uint32_t *d_out_ids, float *d_out_scores,
                               uint32_t *d_out_counts, int32_t device, void *stream);
int32_t cos_merge_lists_packed_device(const uint32_t *d_packed, uint32_t S, uint32_t B, uint32_t k,
                                      uint32_t *d_out_ids, float *d_out_scores, uint32_t *d_out_counts,
                                      int32_t device, void *stream);

/* ---- sharded serving --------------------------------------------------------- */
/* A shard set = the S id-range shards of one collection (cos_index handles, cos_params.id_base = first id of the shard) plus
 * the exchange step between them: ONE all-gather of the packed per-shard records (RCCL over xGMI) and the S-way merge.
 * It stands behind the same caller as cos_search_batch — IndexOps::batch_search (indexes/mod.rs:260-272), a single process —
 * so the Rust host gets merged global top-k lists from one call.  Two deployments:
 *   - every shard in this process (n_local == world_size, unique_id NULL): communicators via ncclCommInitAll, the per-batch
 *     collective is a group of S ncclAllGather calls, one per device; cos_shardset_search_batch is the entry point;
 *   - one process per GPU (n_local == 1 < world_size): rank `first_rank` of a world_size communicator built from the
 *     ncclUniqueId one process obtained with cos_shardset_unique_id and handed to the others; the per-batch entry point is
 *     cos_shardset_exchange_device (all-gather + merge enqueued on the caller's stream).
 * Shards that share one device are exchanged with device copies (no communicator can span them). */
typedef struct cos_shardset cos_shardset;
#define COS_SHARDSET_UNIQUE_ID_BYTES 128
int32_t cos_shardset_unique_id(uint8_t *out /* [COS_SHARDSET_UNIQUE_ID_BYTES] */);
int32_t cos_shardset_create(cos_index *const *shards, uint32_t n_local, uint32_t first_rank, uint32_t world_size,
                            const uint8_t *unique_id, cos_shardset **out);
int32_t cos_shardset_destroy(cos_shardset *ss); /* the cos_index handles stay owned by the caller */
/* queries [B][dim] raw f32 (host) -> merged global top-k over every shard: out_ids [B][top_k] global internal ids,
 * out_scores exact cosine, out_counts [B].  Order: score desc by total_cmp, larger id first on ties.  Any failing query on
 * any shard fails the call (first error), like cos_search_batch.  Thread-safe; batches are serialised per shard set. */
int32_t cos_shardset_search_batch(cos_shardset *ss, const float *queries, uint32_t B, uint32_t top_k, uint32_t *out_ids,
                                  float *out_scores, uint32_t *out_counts);
/* Process-per-GPU exchange, all pointers DEVICE memory, enqueued on `stream`: d_packed_local = this shard's packed record
 * (B*(2*top_k+1) words, written by cos_search_batch_device on the same stream) -> d_gathered [world_size][words] ->
 * merged d_out_* on every rank.  Every rank must call it the same number of times in the same order. */
int32_t cos_shardset_exchange_device(cos_shardset *ss, const uint32_t *d_packed_local, uint32_t B, uint32_t top_k,
                                     uint32_t *d_gathered, uint32_t *d_out_ids, float *d_out_scores, uint32_t *d_out_counts,
                                     void *stream);
/* Both calls above merge with cos_merge_lists_packed_device: world_size * top_k <= 8192, otherwise COS_ERR_UNIMPLEMENTED.
 *
 * The other search operators of a cos_index on a shard set, in the shape of cos_shardset_search_batch: every shard runs the single-index
 * operator (its own kernels, refusals and zero-norm rule) and leaves its packed record on its device, ONE exchange, ONE merge on shard 0's
 * device, one copy back; under the set's lock, every shard in this process.  The first failing shard, in shard order, fails the call with
 * its status (the message names the shard); S * top_k <= 8192, otherwise COS_ERR_UNIMPLEMENTED.  The exhaustive operators block their host
 * thread (overflow retry, zero-norm read-back), so shards on different devices run from one host thread per device; shards that share a
 * device run in turn.  The outputs are those of cos_shardset_search_batch: global ids, out_counts[q] = min(sum of the shards' counts, top_k).
 *   cos_shardset_search_filtered_batch   cos_search_filtered_batch per shard (filters as there, one set for every shard): every shard is a
 *       ready metadata collection (COS_ERR_NOT_READY) with the same number of metadata dimensions (COS_ERR_INVALID) and
 *       id_base = first embedding x max_replicas.
 *   cos_shardset_flat_search_batch       cos_flat_search_batch / cos_flat_search_masked_batch per shard.  Exhaustive per-shard mode: the
 *       5 x top_k cut of the finalisation is applied PER SHARD, so the answer is the per-shard operator's answers under the merge rule — not
 *       the answer of one index over the whole corpus, whose single cut keeps 5 x top_k candidates in all.
 *   cos_shardset_bruteforce_topk         cos_bruteforce_topk / cos_bruteforce_topk_masked per shard; k in [1, min(512, rows of the smallest
 *       shard)] (COS_ERR_INVALID).  The exact re-score is per row and every shard keeps a pool of at least 2k, so over the id-range shards
 *       of a corpus this is the exact global top-k: ids and score bits of cos_bruteforce_topk on one index holding the whole corpus.
 * shard_masks: NULL, or [S] pointers, entry s NULL (shard s unmasked) or a cos_scan_mask over shard s's OWN rows (bit r = row r of that
 * shard, not a global id); COS_SCAN_SKIP_DELETED reads shard s's own deleted set.  Cutting a mask over global rows at the shard boundaries
 * is the host's work (Python: cosdata_amd.sharding.slice_row_masks). */
int32_t cos_shardset_search_filtered_batch(cos_shardset *ss, const float *queries, uint32_t B, const uint32_t *filter_offsets,
                                           const int8_t *filter_dims, uint32_t top_k, uint32_t *out_ids, float *out_scores,
                                           uint32_t *out_counts);
int32_t cos_shardset_flat_search_batch(cos_shardset *ss, const float *queries, uint32_t B, uint32_t top_k,
                                       const cos_scan_mask *const *shard_masks, uint32_t *out_ids, float *out_scores,
                                       uint32_t *out_counts);
int32_t cos_shardset_bruteforce_topk(cos_shardset *ss, const float *queries, uint32_t B, uint32_t k,
                                     const cos_scan_mask *const *shard_masks, uint32_t *out_ids, float *out_scores,
                                     uint32_t *out_counts);

/* The text half of the collection on a shard set.  cos_bm25 handle s holds the documents of shard s under LOCAL ids
 * 0 .. n_s - 1; the global id of a document is doc_bases[s] + local id (doc_bases == NULL: the dense shards' id_base).  The handles stay
 * owned by the caller, who inserts into and deletes from the owning shard's handle with local ids; attaching again replaces them;
 * shards == NULL detaches.  n_shards must equal the set's shard count, handle s must live on dense shard s's device, the bases must
 * strictly increase and doc_bases[s] + (largest id handle s has ever held) must stay below 2^32 - 1 and below doc_bases[s + 1] (a global
 * id names one document), else COS_ERR_INVALID (the id rules are checked again by every search: inserts move the largest id).  A set that
 * does not hold every shard in this process: COS_ERR_UNIMPLEMENTED. */
int32_t cos_shardset_attach_bm25(cos_shardset *ss, cos_bm25 *const *shards, uint32_t n_shards, const uint32_t *doc_bases);
/* cos_bm25_search_batch over the attached shards: ids (global), score bits and counts of ONE cos_bm25 handle created from the whole
 * collection's postings.  Per query term the idf comes from the collection — documents_count and list length summed over the shards,
 * tombstones included — looked up in every shard's term table per call; every shard scores its own documents with it into its 512
 * buckets per query, keyed by the GLOBAL id; ONE exchange brings the S bucket arrays to shard 0's device, one kernel takes their
 * element-wise maximum, sorts and cuts.  More than 64 of a query's terms with a list in ANY shard: COS_ERR_UNIMPLEMENTED, as the single
 * handle refuses 64 matching terms.  Nothing attached: COS_ERR_NOT_READY.  Locks: the set's, then every handle's in shard order, held
 * from the term lookup to the call's synchronisation — an update of a shard handle happens before or after a search, never inside. */
int32_t cos_shardset_bm25_search_batch(cos_shardset *ss, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B,
                                       uint32_t top_k, uint32_t *out_ids, float *out_scores, uint32_t *out_counts);
/* cos_hybrid_search_batch on the set: cos_shardset_search_batch for 3 * top_k and the call above for 3 * top_k, both merged lists left on
 * shard 0's device, RRF there, one copy back.  On every device the dense half is enqueued first.  top_k > 170 or S * 3 * top_k > 8192:
 * COS_ERR_UNIMPLEMENTED.  A failing dense query fails the call with the first failing shard's status. */
int32_t cos_shardset_hybrid_search_batch(cos_shardset *ss, const float *queries, const uint32_t *q_terms, const uint32_t *q_offsets,
                                         uint32_t B, uint32_t top_k, float fusion_constant_k,
                                         uint32_t *out_ids, float *out_scores, uint32_t *out_counts);

/* The learned-sparse half of the collection on a shard set.  cos_sparse handle s holds the vectors of shard s under
 * LOCAL ids 0 .. n_s - 1; the global id of a vector is vec_bases[s] + local id (vec_bases == NULL: the dense shards' id_base).  The rules
 * are those of cos_shardset_attach_bm25: the handles stay owned by the caller, who inserts into and deletes from the owning shard's
 * handle with local ids; attaching again replaces them; shards == NULL detaches; n_shards equals the set's shard count, handle s lives on
 * dense shard s's device, no handle twice, the bases strictly increase, vec_bases[s] + n_s stays <= vec_bases[s + 1] and below 2^32 - 1,
 * else COS_ERR_INVALID (checked again by every search: cos_sparse_insert moves n).  One rule more: quantization_bits and
 * values_upper_bound (its f32 bits) are the same on every handle, else COS_ERR_INVALID — a vector then has the quantized similarity in
 * its shard that it has in the whole collection.  A set that does not hold every shard in this process: COS_ERR_UNIMPLEMENTED. */
int32_t cos_shardset_attach_sparse(cos_shardset *ss, cos_sparse *const *shards, uint32_t n_shards, const uint32_t *vec_bases);
/* cos_sparse_search_batch over the attached shards: ids (global), score bits and counts of ONE cos_sparse handle created from the whole
 * collection.  With C = top_k * max(reranking_factor, 1): every shard runs its scan and leaves its best C candidates per query —
 * (quantized similarity, global id) keys and, for a rerank, each candidate's raw-value score — as one record on its device; ONE exchange
 * brings the S records to shard 0's device; one kernel cuts the S x C keys to the collection's best C by (similarity, larger id first),
 * re-ranks exactly those by raw score and cuts to top_k.  (A per-shard rerank followed by a merge would re-rank vectors the whole
 * collection never re-scores.)  Output slots past a query's count are not written.
 * Refused before anything is enqueued, the set and every handle staying usable: nothing attached -> COS_ERR_NOT_READY; a rerank while
 * a shard holds no raw vectors -> COS_ERR_NOT_READY; C above any shard's cos_sparse_set_max_candidates -> COS_ERR_UNIMPLEMENTED;
 * S x (64, 128, .. 1024: C rounded up) above 8192 -> COS_ERR_UNIMPLEMENTED; B at or above cos_sparse_search_batch's bound, decreasing
 * offsets, a broken id rule -> COS_ERR_INVALID.  Locks: the set's, then every sparse handle's in shard order, held to the call's
 * synchronisation — an update of a shard handle happens before or after a search, never inside. */
int32_t cos_shardset_sparse_search_batch(cos_shardset *ss, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets,
                                         uint32_t B, uint32_t top_k, float early_terminate_threshold, uint32_t reranking_factor,
                                         uint32_t *out_ids, float *out_scores, uint32_t *out_counts);
/* cos_hybrid_search_mixed on the set: the request is split as there; the dense sub-batch is cos_shardset_search_batch for 3 * top_k
 * (enqueued first on every device), the sparse sub-batch the call above for 3 * top_k with C = 3 * top_k * max(reranking_factor, 1), the
 * BM25 sub-batch cos_shardset_bm25_search_batch for 3 * top_k; the three list sets stay on shard 0's device, the fusion runs there, one
 * copy back.  Refusals: those of cos_hybrid_search_mixed, the widths of the three calls (S * 3 * top_k <= 8192 for a dense sub-batch),
 * and COS_ERR_NOT_READY for a half that has queries and nothing attached; a half without queries needs nothing attached.  Locks: the
 * set's, every sparse handle's in shard order, every BM25 handle's in shard order.  A failing dense query fails the call with the first
 * failing shard's status; the next call answers. */
int32_t cos_shardset_hybrid_search_mixed(cos_shardset *ss, const cos_hybrid_request *rq, uint32_t *out_ids, float *out_scores,
                                         uint32_t *out_counts);

/* ---- tuning knobs (experiments; NOT a reference interface) ------------------------------------------------------------------
 * Launch-policy knobs of the kernels — which of two implementations of one operator runs, launch sizes at which a policy
 * switches, prefetch depths.  None changes a result; the parity tests use them to compare implementations, the profiling
 * scripts to time them.  Names: cosdata_amd/csrc/tuning.h.  The library reads ONE environment variable,
 * COS_TUNING="name=value,name=value" (parsed once, on first use), so that an unmodified process can be steered under rocprofv3;
 * nothing else of the process environment influences a kernel.  A knob that is not set leaves the built-in, measured default.
 * Process-wide, thread-safe (relaxed atomics); knobs read at cos_index_create apply to handles created afterwards. */
int32_t cos_tuning_set(const char *name, int64_t value);
int32_t cos_tuning_clear(const char *name /* NULL = every knob */);
int32_t cos_tuning_get(const char *name, int64_t *out_value, int32_t *out_is_set);

#ifdef __cplusplus
}
#endif
#endif /* COSDATA_HIP_H */
