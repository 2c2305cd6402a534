// shardset.hip — sharded serving behind the C ABI (BASELINE north_star: "the index shards by vector-ID range
// across the 8 GPUs of one node with a final RCCL all-gather of per-shard top-k over xGMI").
//
// The caller of the reference's search path is ONE process: IndexOps::batch_search (indexes/mod.rs:260-272).  A cos_shardset
// gives that process one call that fans a query batch out to S resident shards (cos_index handles, id_base = first id of the
// shard), runs walk + exact rerank on every shard's GPU, exchanges the packed per-shard records [ids | scores | counts] with
// ONE all-gather and merges them (cos_merge_lists_packed_device, up to 8192 keys per query): cos_shardset_search_batch.  The filtered
// and the two exhaustive searches have the same shape (cos_shardset_search_filtered_batch, cos_shardset_flat_search_batch,
// cos_shardset_bruteforce_topk): every shard runs the single-index operator and leaves its record on its device.  Two deployments share the code:
//   * single process, S devices   (the Rust host):  ranks 0..S-1 are all local; communicators from ncclCommInitAll;
//     the per-launch collective is S grouped ncclAllGather calls, one per device stream;
//   * one process per GPU         (bench.py under torchrun): every process owns one local shard and joins a world-size
//     communicator built from a ncclUniqueId the host side distributes (cos_shardset_unique_id -> broadcast -> create);
//     cos_shardset_exchange_device is the per-launch exchange, enqueued on the caller's stream.
// Shards that share a device (S = 2 on one GPU: the single-device parity test) cannot form an RCCL communicator; their
// records are gathered with device-to-device copies instead — the same data movement, no other difference.
//
// RCCL is resolved at run time (dlopen of librccl.so.1) the first time a communicator is needed, so libcosdata_hip.so itself
// has no link-time dependency on it and single-GPU users never load it.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine_internal.h"
#include "flat_plan.h"
#include "hybrid_plan.h"
#include "merge_plan.h"
#include "sparse_fold_plan.h"

using namespace cosdev;

namespace {

struct RcclApi {
    void *handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
};

RcclApi *rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (api.handle) break;
        }
        if (!api.handle) { api.error = std::string("dlopen(librccl.so.1): ") + dlerror(); return; }
#define SYM(field, name)                                                                   \
    api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.handle, name));            \
    if (!api.field && api.error.empty()) api.error = std::string("librccl: missing symbol ") + name
        SYM(GetUniqueId, "ncclGetUniqueId");
        SYM(CommInitRank, "ncclCommInitRank");
        SYM(CommInitAll, "ncclCommInitAll");
        SYM(CommDestroy, "ncclCommDestroy");
        SYM(AllGather, "ncclAllGather");
        SYM(GroupStart, "ncclGroupStart");
        SYM(GroupEnd, "ncclGroupEnd");
        SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    });
    return &api;
}

#define RCCL_TRY(expr)                                                                                                        \
    do {                                                                                                                      \
        ncclResult_t _r = (expr);                                                                                             \
        if (_r != ncclSuccess) return cos_fail(COS_ERR_HIP, "%s: %s (%s:%d)", #expr, rccl()->GetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

struct LocalShard {
    cos_index *ix = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t done_text = nullptr; // the shard's BM25 buckets are complete (recorded on the attached handle's stream)
    hipStream_t stream_sp = nullptr; // the attached learned-sparse handle's scan and record run here, beside the walk
    hipEvent_t done_sp = nullptr;    // ... and this says that the record is complete
    ncclComm_t comm = nullptr;
    // per-shard device buffers, grown on demand
    DevArr<float> d_queries;
    DevArr<u32> d_packed;   // this shard's record [ids B*k | scores B*k | counts B]
    DevArr<u32> d_gathered; // [world][words]
    DevArr<u32> d_gathered_text; // [world][B * 1024]: every shard's B x 512 bucket keys (u64)
    DevArr<u32> d_record_sp;   // this shard's learned-sparse candidate record (sparse_fold_plan::Layout)
    DevArr<u32> d_gathered_sp; // [world][record words]
    DevArr<int32_t> d_status;
    LocalShard() = default;
    LocalShard(const LocalShard &) = delete;
    ~LocalShard() { // on the shard's device, its stream drained before anything is released
        (void)hipSetDevice(device);
        if (stream_sp) (void)hipStreamSynchronize(stream_sp);
        if (stream) (void)hipStreamSynchronize(stream);
        if (comm) (void)rccl()->CommDestroy(comm);
        d_queries.reset(); d_packed.reset(); d_gathered.reset(); d_gathered_text.reset(); d_record_sp.reset(); d_gathered_sp.reset(); d_status.reset();
        if (done) (void)hipEventDestroy(done);
        if (done_text) (void)hipEventDestroy(done_text);
        if (done_sp) (void)hipEventDestroy(done_sp);
        if (stream_sp) (void)hipStreamDestroy(stream_sp);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

} // namespace

struct cos_shardset {
    std::vector<LocalShard> sh;
    u32 first_rank = 0, world = 0;
    bool use_rccl = false;
    std::mutex mu; // one search at a time per shard set (the collectives of two batches must not interleave)
    // merge output on shard 0's device
    DevArr<u32> d_out_ids, d_out_counts;
    DevArr<float> d_out_scores;
    // the text half (cos_shardset_attach_bm25): handle s holds shard s's documents under local ids, global id = bm_base[s] + local
    std::vector<cos_bm25 *> bm;
    std::vector<u32> bm_base;
    // on shard 0's device: the collection's BM25 lists [B][k] after the fold; the fused lists of a hybrid call [ids | scores | counts]
    DevArr<u32> d_text_ids, d_text_counts, d_ret;
    DevArr<float> d_text_scores;
    PinArr<u32> h_ret;
    // the learned-sparse half (cos_shardset_attach_sparse): handle s holds shard s's vectors under local ids, global id = sp_base[s] + local
    std::vector<cos_sparse *> sp;
    std::vector<u32> sp_base;
    // on shard 0's device: the collection's learned-sparse lists [B][k] after the fold; a mixed hybrid request's query_mapping
    DevArr<u32> d_sp_ids, d_sp_counts;
    DevArr<float> d_sp_scores;
    DevArr<hybrid_plan::Slot> d_slots;
    PinArr<hybrid_plan::Slot> h_slots;
};

extern "C" int32_t cos_shardset_unique_id(uint8_t *out) {
    if (!out) return cos_fail(COS_ERR_INVALID, "null argument");
    RcclApi *r = rccl();
    if (!r->error.empty()) return cos_fail(COS_ERR_HIP, "RCCL unavailable: %s", r->error.c_str());
    ncclUniqueId id;
    RCCL_TRY(r->GetUniqueId(&id));
    static_assert(sizeof(id) == COS_SHARDSET_UNIQUE_ID_BYTES, "ncclUniqueId size");
    memcpy(out, &id, sizeof(id));
    return COS_OK;
}

extern "C" int32_t cos_shardset_destroy(cos_shardset *ss) {
    if (!ss) return COS_OK;
    // the shards first, each on its own device (~LocalShard), then the merge output on shard 0's
    const bool any = !ss->sh.empty();
    const int dev0 = any ? ss->sh[0].device : 0;
    ss->sh.clear();
    if (any) (void)hipSetDevice(dev0);
    ss->d_out_ids.reset(); ss->d_out_counts.reset(); ss->d_out_scores.reset();
    ss->d_text_ids.reset(); ss->d_text_counts.reset(); ss->d_text_scores.reset(); ss->d_ret.reset(); ss->h_ret.reset();
    ss->d_sp_ids.reset(); ss->d_sp_counts.reset(); ss->d_sp_scores.reset(); ss->d_slots.reset(); ss->h_slots.reset();
    delete ss;
    return COS_OK;
}

extern "C" int32_t cos_shardset_create(cos_index *const *shards, uint32_t n_local, uint32_t first_rank, uint32_t world_size, const uint8_t *unique_id,
                                       cos_shardset **out) {
    if (!shards || !out || n_local == 0) return cos_fail(COS_ERR_INVALID, "null/empty shard list");
    *out = nullptr;
    if (world_size == 0) world_size = n_local;
    if ((uint64_t)first_rank + n_local > world_size) return cos_fail(COS_ERR_INVALID, "ranks [%u, %u) exceed world size %u", first_rank, first_rank + n_local, world_size);
    if (n_local != world_size && n_local != 1) return cos_fail(COS_ERR_UNIMPLEMENTED, "a process holds either every shard or exactly one");
    if (n_local != world_size && !unique_id) return cos_fail(COS_ERR_INVALID, "a multi-process shard set needs the ncclUniqueId of cos_shardset_unique_id");
    for (u32 s = 0; s < n_local; s++) {
        if (!shards[s]) return cos_fail(COS_ERR_INVALID, "shard %u is null", s);
        if (shards[s]->p.dim != shards[0]->p.dim) return cos_fail(COS_ERR_INVALID, "shards disagree on dim");
    }
    cos_shardset *ss = new cos_shardset();
    ss->first_rank = first_rank;
    ss->world = world_size;
    ss->sh = std::vector<LocalShard>(n_local);
    bool distinct = true;
    for (u32 s = 0; s < n_local; s++) {
        ss->sh[s].ix = shards[s];
        ss->sh[s].device = shards[s]->p.device;
        for (u32 t = 0; t < s; t++) distinct &= ss->sh[t].device != ss->sh[s].device;
    }
    auto fail = [&](int32_t rc) { cos_shardset_destroy(ss); return rc; };
    for (LocalShard &s : ss->sh) {
        if (hipSetDevice(s.device) != hipSuccess || hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.done_text, hipEventDisableTiming) != hipSuccess ||
            hipStreamCreateWithFlags(&s.stream_sp, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&s.done_sp, hipEventDisableTiming) != hipSuccess)
            return fail(cos_fail(COS_ERR_HIP, "cannot create stream/event on device %d", s.device));
    }
    // RCCL communicators: needed whenever records cross a device boundary
    // (COS_SHARDSET_FORCE_RCCL=1: also for a world of one, so the RCCL call path can be exercised on a single-GPU box)
    const bool force = cosdev::tune_or(cosdev::TUNE_SHARDSET_FORCE_RCCL, 0) != 0 && world_size == 1;
    ss->use_rccl = (world_size > 1 && (n_local == 1 || distinct)) || force;
    if (ss->use_rccl) {
        RcclApi *r = rccl();
        if (!r->error.empty()) return fail(cos_fail(COS_ERR_HIP, "RCCL unavailable: %s", r->error.c_str()));
        if (n_local == world_size) {
            std::vector<int> devs(n_local);
            std::vector<ncclComm_t> comms(n_local);
            for (u32 s = 0; s < n_local; s++) devs[s] = ss->sh[s].device;
            ncclResult_t rr = r->CommInitAll(comms.data(), (int)n_local, devs.data());
            if (rr != ncclSuccess) return fail(cos_fail(COS_ERR_HIP, "ncclCommInitAll: %s", r->GetErrorString(rr)));
            for (u32 s = 0; s < n_local; s++) ss->sh[s].comm = comms[s];
        } else {
            ncclUniqueId id;
            memcpy(&id, unique_id, sizeof(id));
            if (hipSetDevice(ss->sh[0].device) != hipSuccess) return fail(cos_fail(COS_ERR_HIP, "hipSetDevice"));
            ncclResult_t rr = r->CommInitRank(&ss->sh[0].comm, (int)world_size, id, (int)first_rank);
            if (rr != ncclSuccess) return fail(cos_fail(COS_ERR_HIP, "ncclCommInitRank: %s", r->GetErrorString(rr)));
        }
    }
    *out = ss;
    return COS_OK;
}

// What one exchange moves: a record is `words` words per shard — the packed lists B (2k + 1) of the dense operators, or the B x 512 bucket
// keys of the text half, which leave straight from the attached handle's bucket array, or the candidate record of the learned-sparse half.
enum class Record { LISTS, BUCKETS, CANDIDATES };
static const u32 *record_src(cos_shardset *ss, u32 i, Record rec) {
    return rec == Record::LISTS        ? ss->sh[i].d_packed.p
           : rec == Record::CANDIDATES ? ss->sh[i].d_record_sp.p
                                       : reinterpret_cast<const u32 *>(cosdev::bm25_buckets(ss->bm[i]));
}
static u32 *record_dst(LocalShard &s, Record rec) {
    return rec == Record::LISTS ? s.d_gathered.p : rec == Record::CANDIDATES ? s.d_gathered_sp.p : s.d_gathered_text.p;
}
static hipEvent_t record_event(LocalShard &s, Record rec) { return rec == Record::LISTS ? s.done : rec == Record::CANDIDATES ? s.done_sp : s.done_text; }

// gathered[world][words] on every local shard's device <- every shard's record; enqueued on the shards' streams, each of which is
// already behind its own shard's record (it produced it, or waits for the event of the stream that did)
static int32_t exchange_local(cos_shardset *ss, size_t words, Record rec = Record::LISTS) {
    const u32 S = (u32)ss->sh.size();
    if (ss->use_rccl) {
        RcclApi *r = rccl();
        RCCL_TRY(r->GroupStart());
        for (u32 i = 0; i < S; i++) {
            LocalShard &s = ss->sh[i];
            ncclResult_t rr = r->AllGather(record_src(ss, i, rec), record_dst(s, rec), words, ncclUint32, s.comm, s.stream);
            if (rr != ncclSuccess) { (void)r->GroupEnd(); return cos_fail(COS_ERR_HIP, "ncclAllGather: %s", r->GetErrorString(rr)); }
        }
        RCCL_TRY(r->GroupEnd());
        return COS_OK;
    }
    // shards sharing a device (or a single shard): plain device copies into shard 0's gather buffer, ordered by events
    LocalShard &root = ss->sh[0];
    HIP_TRY(hipSetDevice(root.device));
    for (u32 s = 0; s < S; s++) {
        LocalShard &src = ss->sh[s];
        if (s) HIP_TRY(hipStreamWaitEvent(root.stream, record_event(src, rec), 0));
        u32 *dst = record_dst(root, rec) + (size_t)s * words;
        if (src.device == root.device)
            HIP_TRY(hipMemcpyAsync(dst, record_src(ss, s, rec), words * 4, hipMemcpyDeviceToDevice, root.stream));
        else // a mixed set (e.g. 3 shards on 2 GPUs): explicit peer copy, valid with or without peer access between the two devices
            HIP_TRY(hipMemcpyPeerAsync(dst, root.device, record_src(ss, s, rec), src.device, words * 4, root.stream));
    }
    return COS_OK;
}

namespace {
struct DrainAll { // every return path — a later shard's error, a failed grow, a failed exchange — leaves no walk or collective
    cos_shardset *ss; // of this batch queued on any shard's stream: the next call (or destroy) starts from idle streams
    std::vector<std::pair<int, hipStream_t>> text; // ... nor on a stream of an attached BM25 handle that the call has used
    ~DrainAll() {
        for (auto &t : text) { (void)hipSetDevice(t.first); (void)hipStreamSynchronize(t.second); }
        for (LocalShard &s : ss->sh) { // (the learned-sparse records first: the shards' streams wait for them)
            (void)hipSetDevice(s.device);
            (void)hipStreamSynchronize(s.stream_sp);
            (void)hipStreamSynchronize(s.stream);
        }
        (void)hipSetDevice(ss->sh[0].device);
    }
};

// the merge takes at most 8192 keys per query (merge_plan.h)
int32_t check_merge_width(u32 S, u32 top_k) {
    const merge_plan::Plan mp = merge_plan::plan(S, top_k, merge_plan::LDS_MAX_KEYS);
    if (mp.kind == merge_plan::Kind::REFUSED)
        return cos_fail(mp.status, "%u shards x top_k %u = %llu merged keys per query: at most %u", S, top_k, (unsigned long long)mp.keys, merge_plan::LDS_MAX_KEYS);
    return COS_OK;
}

// every shard's record is in its d_packed (events `done` recorded): ONE exchange, the merge on shard 0's device and the copies back, all
// enqueued on the shards' streams; the caller synchronises shard 0's
int32_t exchange_merge(cos_shardset *ss, u32 B, u32 top_k, size_t words) { // ... up to the merged lists in d_out_* on shard 0's device
    int32_t rc = exchange_local(ss, words);
    if (rc) return rc;
    LocalShard &root = ss->sh[0];
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(ss->d_out_ids.grow((size_t)B * top_k));
    HIP_TRY(ss->d_out_scores.grow((size_t)B * top_k));
    HIP_TRY(ss->d_out_counts.grow((size_t)B * top_k));
    return cos_merge_lists_packed_device(root.d_gathered, ss->world, B, top_k, ss->d_out_ids, ss->d_out_scores, ss->d_out_counts, root.device, root.stream);
}
int32_t exchange_merge_copy(cos_shardset *ss, u32 B, u32 top_k, size_t words, uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    int32_t rc = exchange_merge(ss, B, top_k, words);
    if (rc) return rc;
    LocalShard &root = ss->sh[0];
    HIP_TRY(hipMemcpyAsync(out_ids, ss->d_out_ids, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, root.stream));
    HIP_TRY(hipMemcpyAsync(out_scores, ss->d_out_scores, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, root.stream));
    HIP_TRY(hipMemcpyAsync(out_counts, ss->d_out_counts, (size_t)B * 4, hipMemcpyDeviceToHost, root.stream));
    return COS_OK;
}
// every shard: queries up, walk + exact rerank into its packed record (all shards run concurrently on their devices).  The walk runs on
// the shard's stream, or — the dense half of a hybrid call — on the stream the attached BM25 handle keeps for it (the one
// cos_hybrid_search_batch walks on), which the shard's stream then waits for.
int32_t enqueue_walks(cos_shardset *ss, const float *queries, u32 B, u32 top_k, size_t words, DrainAll *hybrid) {
    const u32 S = ss->world, dim = ss->sh[0].ix->p.dim;
    for (u32 i = 0; i < S; i++) {
        LocalShard &s = ss->sh[i];
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(s.d_queries.grow((size_t)B * dim));
        HIP_TRY(s.d_packed.grow(words));
        HIP_TRY(s.d_gathered.grow(words * S));
        HIP_TRY(s.d_status.grow((size_t)B));
        hipStream_t st = s.stream;
        if (hybrid) {
            if (int32_t rc = cosdev::bm25_dense_stream(ss->bm[i], &st)) return rc;
            hybrid->text.emplace_back(s.device, st);
        }
        HIP_TRY(hipMemcpyAsync(s.d_queries, queries, (size_t)B * dim * 4, hipMemcpyHostToDevice, st));
        int32_t rc = cos_search_batch_device(s.ix, s.d_queries, B, top_k, s.d_packed, reinterpret_cast<float *>(s.d_packed + (size_t)B * top_k),
                                             s.d_packed + 2 * (size_t)B * top_k, s.d_status, st);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(s.done, st));
        if (st != s.stream) HIP_TRY(hipStreamWaitEvent(s.stream, s.done, 0));
    }
    return COS_OK;
}

// per-shard statuses of the walks: like the reference's collect::<Result<_>>, one failing query on any shard fails the call
int32_t check_walk_statuses(cos_shardset *ss, u32 B) {
    LocalShard &root = ss->sh[0];
    std::vector<int32_t> status((size_t)B);
    for (LocalShard &s : ss->sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipMemcpyAsync(status.data(), s.d_status, (size_t)B * 4, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        for (u32 b = 0; b < B; b++)
            if (status[b] != COS_OK) {
                (void)hipSetDevice(root.device);
                (void)hipStreamSynchronize(root.stream);
                return cos_fail(status[b], "query %u failed on shard %u with status %d (zero-norm vector -> DistanceError::CalculationError)", b,
                                ss->first_rank + (u32)(&s - ss->sh.data()), status[b]);
            }
    }
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(hipStreamSynchronize(root.stream));
    return COS_OK;
}
} // namespace

extern "C" int32_t cos_shardset_search_batch(cos_shardset *ss, const float *queries, uint32_t B, uint32_t top_k, uint32_t *out_ids, float *out_scores,
                                             uint32_t *out_counts) {
    if (!ss || !queries || !out_ids || !out_scores || !out_counts || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ss->sh.size() != ss->world) return cos_fail(COS_ERR_INVALID, "cos_shardset_search_batch needs every shard in this process; a process-per-GPU job uses cos_shardset_exchange_device");
    if (int32_t wrc = check_merge_width(ss->world, top_k)) return wrc;
    std::lock_guard<std::mutex> g(ss->mu);
    const size_t words = (size_t)B * (2 * (size_t)top_k + 1);
    DrainAll drain_all{ss};
    // 1. every shard's walk
    int32_t rc = enqueue_walks(ss, queries, B, top_k, words, nullptr);
    if (rc) return rc;
    // 2. ONE exchange step, 3. merge on shard 0's device
    rc = exchange_merge_copy(ss, B, top_k, words, out_ids, out_scores, out_counts);
    if (rc) return rc;
    return check_walk_statuses(ss, B);
}

extern "C" int32_t cos_shardset_exchange_device(cos_shardset *ss, const uint32_t *d_packed_local, uint32_t B, uint32_t top_k, uint32_t *d_gathered,
                                                uint32_t *d_out_ids, float *d_out_scores, uint32_t *d_out_counts, void *stream) {
    if (!ss || !d_packed_local || !d_gathered || !d_out_ids || !d_out_scores || !d_out_counts || B == 0 || top_k == 0)
        return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ss->sh.size() != 1) return cos_fail(COS_ERR_INVALID, "cos_shardset_exchange_device is the process-per-GPU entry point (one local shard)");
    LocalShard &s = ss->sh[0];
    HIP_TRY(hipSetDevice(s.device));
    const size_t words = (size_t)B * (2 * (size_t)top_k + 1);
    hipStream_t st = (hipStream_t)stream;
    {
        std::lock_guard<std::mutex> g(ss->mu); // collectives of one communicator are issued in one order on every rank
        if (ss->use_rccl) RCCL_TRY(rccl()->AllGather(d_packed_local, d_gathered, words, ncclUint32, s.comm, st));
        else HIP_TRY(hipMemcpyAsync(d_gathered, d_packed_local, words * 4, hipMemcpyDeviceToDevice, st)); // world of one
    }
    return cos_merge_lists_packed_device(d_gathered, ss->world, B, top_k, d_out_ids, d_out_scores, d_out_counts, s.device, st);
}

// ---- the filtered and the exhaustive searches on a shard set ---------------------------------------------------------------------------
namespace {
enum class ShardOp { FILTERED, FLAT, BRUTE };
struct ShardOpArgs {
    ShardOp op;
    const float *queries;
    u32 B, top_k;
    const u32 *f_off = nullptr;                  // FILTERED
    const int8_t *f_dims = nullptr;
    const cos_scan_mask *const *masks = nullptr; // FLAT, BRUTE: NULL or [S], every entry NULL or a mask over that shard's own rows
};

// Every shard's operator (the single-index call's own kernels; each blocks its host thread until the shard's record is complete on the
// shard's device), one exchange, one merge, one copy back.  Shards on different devices run from one host thread per device, so that the
// devices work at once; the shards of one device run in turn.
int32_t shardset_run(cos_shardset *ss, const ShardOpArgs &a, uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    const u32 S = ss->world, B = a.B, top_k = a.top_k;
    const size_t words = (size_t)B * (2 * (size_t)top_k + 1);
    std::lock_guard<std::mutex> g(ss->mu);
    DrainAll drain_all{ss};
    for (LocalShard &s : ss->sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(s.d_packed.grow(words));
        HIP_TRY(s.d_gathered.grow(words * S));
    }
    std::vector<int32_t> rcs(S, COS_OK);
    std::vector<std::string> errs(S);
    auto run_shard = [&](u32 i) {
        LocalShard &s = ss->sh[i];
        const cos_scan_mask *m = a.masks ? a.masks[i] : nullptr;
        int32_t rc = a.op == ShardOp::FILTERED ? search_filtered_record(s.ix, a.queries, B, a.f_off, a.f_dims, top_k, s.d_packed)
                     : a.op == ShardOp::FLAT   ? flat_search_record(s.ix, a.queries, B, top_k, m, s.d_packed)
                                               : bruteforce_record(s.ix, a.queries, B, top_k, m, s.d_packed);
        if (rc == COS_OK && (hipSetDevice(s.device) != hipSuccess || hipEventRecord(s.done, s.stream) != hipSuccess))
            rc = cos_fail(COS_ERR_HIP, "cannot record an event on device %d", s.device);
        rcs[i] = rc;
        if (rc) errs[i] = cos_last_error_string(); // (the message belongs to the thread that ran the shard)
    };
    // the shards grouped by device, in shard order
    std::vector<std::vector<u32>> groups;
    for (u32 i = 0; i < S; i++) {
        size_t gi = 0;
        while (gi < groups.size() && ss->sh[groups[gi][0]].device != ss->sh[i].device) gi++;
        if (gi == groups.size()) groups.emplace_back();
        groups[gi].push_back(i);
    }
    auto run_group = [&](const std::vector<u32> &grp) {
        for (u32 i : grp) {
            run_shard(i);
            if (rcs[i]) break; // a failure ends the call: the device's later shards are not started
        }
    };
    if (groups.size() == 1) run_group(groups[0]);
    else {
        std::vector<std::thread> threads;
        for (size_t gi = 1; gi < groups.size(); gi++) threads.emplace_back(run_group, std::cref(groups[gi]));
        run_group(groups[0]);
        for (std::thread &t : threads) t.join();
    }
    for (u32 i = 0; i < S; i++) // the first failing shard, in shard order
        if (rcs[i]) return cos_fail(rcs[i], "shard %u: %s", ss->first_rank + i, errs[i].c_str());
    int32_t rc = exchange_merge_copy(ss, B, top_k, words, out_ids, out_scores, out_counts);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ss->sh[0].device));
    HIP_TRY(hipStreamSynchronize(ss->sh[0].stream));
    return COS_OK;
}

int32_t shardset_check(cos_shardset *ss, const void *queries, uint32_t B, uint32_t top_k, const void *o0, const void *o1, const void *o2, const char *name) {
    if (!ss || !queries || !o0 || !o1 || !o2 || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ss->sh.size() != ss->world) return cos_fail(COS_ERR_INVALID, "%s needs every shard in this process", name);
    return check_merge_width(ss->world, top_k);
}
} // namespace

extern "C" int32_t cos_shardset_search_filtered_batch(cos_shardset *ss, const float *queries, uint32_t B, const uint32_t *filter_offsets,
                                                      const int8_t *filter_dims, uint32_t top_k, uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (int32_t rc = shardset_check(ss, queries, B, top_k, out_ids, out_scores, out_counts, "cos_shardset_search_filtered_batch")) return rc;
    if (!filter_offsets || !filter_dims) return cos_fail(COS_ERR_INVALID, "bad argument");
    for (u32 i = 0; i < ss->world; i++) { // one schema: the filters are written once for every shard
        const u32 md = ss->sh[i].ix->meta.mdim;
        if (md == 0) return cos_fail(COS_ERR_NOT_READY, "shard %u is not a metadata collection", ss->first_rank + i);
        if (md != ss->sh[0].ix->meta.mdim)
            return cos_fail(COS_ERR_INVALID, "shard %u has %u metadata dimensions, shard %u has %u", ss->first_rank + i, md, ss->first_rank, ss->sh[0].ix->meta.mdim);
    }
    ShardOpArgs a{ShardOp::FILTERED, queries, B, top_k};
    a.f_off = filter_offsets;
    a.f_dims = filter_dims;
    return shardset_run(ss, a, out_ids, out_scores, out_counts);
}

extern "C" int32_t cos_shardset_flat_search_batch(cos_shardset *ss, const float *queries, uint32_t B, uint32_t top_k, const cos_scan_mask *const *shard_masks,
                                                  uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (int32_t rc = shardset_check(ss, queries, B, top_k, out_ids, out_scores, out_counts, "cos_shardset_flat_search_batch")) return rc;
    ShardOpArgs a{ShardOp::FLAT, queries, B, top_k};
    a.masks = shard_masks;
    return shardset_run(ss, a, out_ids, out_scores, out_counts);
}

extern "C" int32_t cos_shardset_bruteforce_topk(cos_shardset *ss, const float *queries, uint32_t B, uint32_t k, const cos_scan_mask *const *shard_masks,
                                                uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (int32_t rc = shardset_check(ss, queries, B, k, out_ids, out_scores, out_counts, "cos_shardset_bruteforce_topk")) return rc;
    for (u32 i = 0; i < ss->world; i++) // every shard must hold k rows: a short list would not be the single-index call's answer
        if (int32_t krc = flat_plan::check_brute_k(k, ss->sh[i].ix->n))
            return cos_fail(krc, "shard %u holds %u rows: k must be in [1, min(512, smallest shard)]", ss->first_rank + i, ss->sh[i].ix->n);
    ShardOpArgs a{ShardOp::BRUTE, queries, B, k};
    a.masks = shard_masks;
    return shardset_run(ss, a, out_ids, out_scores, out_counts);
}

// ---- the text half of the collection on a shard set: BM25 and dense + BM25 hybrid search ------------------------------------------------
// (the scheme and why it is the whole index's answer bit for bit: kernels_hybrid.hip, "The BM25 handle as one shard of a collection")
namespace {
constexpr size_t BUCKET_WORDS = 1024; // 512 u64 bucket keys per query

// the locks of every attached handle, in shard order, until the call has synchronised
struct TextLocks {
    std::vector<std::unique_lock<std::mutex>> held;
    explicit TextLocks(cos_shardset *ss) {
        for (cos_bm25 *b : ss->bm) held.emplace_back(cosdev::bm25_mutex(b));
    }
};

// global ids stay below 2^32 - 1 and inside their shard's range (inserts move the largest id, so every search asks again); locks held
int32_t check_text_ids(const std::vector<cos_bm25 *> &bm, const std::vector<u32> &base, u32 first_rank) {
    for (size_t s = 0; s < bm.size(); s++) {
        const long long largest = cosdev::bm25_largest_id(bm[s]);
        const u64 top = (u64)base[s] + (u64)(largest < 0 ? 0 : largest);
        if (top >= 0xFFFFFFFFull)
            return cos_fail(COS_ERR_INVALID, "BM25 shard %u: doc_base %u + largest id %lld does not fit below 2^32 - 1", first_rank + (u32)s, base[s], largest);
        if (s + 1 < bm.size() && largest >= 0 && top >= base[s + 1])
            return cos_fail(COS_ERR_INVALID, "BM25 shard %u: doc_base %u + largest id %lld reaches into the next shard (doc_base %u)", first_rank + (u32)s, base[s],
                            largest, base[s + 1]);
    }
    return COS_OK;
}

int32_t text_check(cos_shardset *ss, const void *q_terms, const void *q_offsets, u32 B, u32 top_k, const void *o0, const void *o1, const void *o2, const char *name) {
    if (!ss || !q_terms || !q_offsets || !o0 || !o1 || !o2 || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ss->sh.size() != ss->world) return cos_fail(COS_ERR_UNIMPLEMENTED, "%s needs every shard in this process", name);
    return COS_OK;
}

// every shard scores into its handle's buckets on the handle's stream; ONE exchange of the S bucket arrays; the fold on shard 0's device
// leaves the collection's lists in d_text_* ([B][top_k], [B]); everything enqueued, nothing synchronised
int32_t text_lists(cos_shardset *ss, DrainAll &drain, const uint32_t *q_terms, const uint32_t *q_offsets, u32 B, u32 top_k) {
    const u32 S = ss->world;
    const size_t words = (size_t)B * BUCKET_WORDS;
    LocalShard &root = ss->sh[0];
    for (LocalShard &s : ss->sh) { // (only the all-gather writes every shard's buffer; the copies fill shard 0's)
        if (!ss->use_rccl && &s != &root) continue;
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(s.d_gathered_text.grow(words * S));
    }
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(ss->d_text_ids.grow((size_t)B * top_k));
    HIP_TRY(ss->d_text_scores.grow((size_t)B * top_k));
    HIP_TRY(ss->d_text_counts.grow((size_t)B));
    int32_t rc = cosdev::bm25_set_score(ss->bm.data(), ss->bm_base.data(), S, q_terms, q_offsets, B);
    for (u32 i = 0; i < S; i++) // (whatever the call has launched before a failure is drained too)
        if (hipStream_t st = cosdev::bm25_stream(ss->bm[i])) drain.text.emplace_back(ss->sh[i].device, st);
    if (rc) return rc;
    for (u32 i = 0; i < S; i++) {
        LocalShard &s = ss->sh[i];
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipEventRecord(s.done_text, cosdev::bm25_stream(ss->bm[i])));
        HIP_TRY(hipStreamWaitEvent(s.stream, s.done_text, 0));
    }
    rc = exchange_local(ss, words, Record::BUCKETS);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(root.device));
    return cosdev::bm25_fold_topk(reinterpret_cast<const u64 *>(root.d_gathered_text.p), S, B, top_k, ss->d_text_ids, ss->d_text_scores, ss->d_text_counts, root.stream);
}
} // namespace

extern "C" int32_t cos_shardset_attach_bm25(cos_shardset *ss, cos_bm25 *const *shards, uint32_t n_shards, const uint32_t *doc_bases) {
    if (!ss) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ss->sh.size() != ss->world) return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_shardset_attach_bm25 needs every shard in this process");
    std::lock_guard<std::mutex> g(ss->mu);
    if (!shards) { // detach
        ss->bm.clear();
        ss->bm_base.clear();
        return COS_OK;
    }
    if (n_shards != ss->world) return cos_fail(COS_ERR_INVALID, "%u BM25 handles for a set of %u shards", n_shards, ss->world);
    std::vector<cos_bm25 *> bm(shards, shards + n_shards);
    std::vector<u32> base(n_shards);
    for (u32 s = 0; s < n_shards; s++) {
        if (!bm[s]) return cos_fail(COS_ERR_INVALID, "BM25 shard %u is null", s);
        for (u32 t = 0; t < s; t++)
            if (bm[t] == bm[s]) return cos_fail(COS_ERR_INVALID, "BM25 shards %u and %u are the same handle", t, s);
        if (cosdev::bm25_device(bm[s]) != ss->sh[s].device)
            return cos_fail(COS_ERR_INVALID, "BM25 shard %u lives on device %d, its dense shard on device %d", s, cosdev::bm25_device(bm[s]), ss->sh[s].device);
        base[s] = doc_bases ? doc_bases[s] : ss->sh[s].ix->p.id_base;
        if (s && base[s] <= base[s - 1]) return cos_fail(COS_ERR_INVALID, "doc_bases must strictly increase (shard %u: %u after %u)", s, base[s], base[s - 1]);
    }
    {
        std::vector<std::unique_lock<std::mutex>> held;
        for (cos_bm25 *b : bm) held.emplace_back(cosdev::bm25_mutex(b));
        if (int32_t rc = check_text_ids(bm, base, ss->first_rank)) return rc;
    }
    ss->bm.swap(bm);
    ss->bm_base.swap(base);
    return COS_OK;
}

extern "C" int32_t cos_shardset_bm25_search_batch(cos_shardset *ss, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B, uint32_t top_k,
                                                  uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (int32_t rc = text_check(ss, q_terms, q_offsets, B, top_k, out_ids, out_scores, out_counts, "cos_shardset_bm25_search_batch")) return rc;
    std::lock_guard<std::mutex> g(ss->mu);
    if (ss->bm.empty()) return cos_fail(COS_ERR_NOT_READY, "no BM25 shards attached (cos_shardset_attach_bm25)");
    TextLocks locks(ss);
    if (int32_t rc = check_text_ids(ss->bm, ss->bm_base, ss->first_rank)) return rc;
    DrainAll drain_all{ss};
    int32_t rc = text_lists(ss, drain_all, q_terms, q_offsets, B, top_k);
    if (rc) return rc;
    LocalShard &root = ss->sh[0];
    HIP_TRY(hipMemcpyAsync(out_ids, ss->d_text_ids, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, root.stream));
    HIP_TRY(hipMemcpyAsync(out_scores, ss->d_text_scores, (size_t)B * top_k * 4, hipMemcpyDeviceToHost, root.stream));
    HIP_TRY(hipMemcpyAsync(out_counts, ss->d_text_counts, (size_t)B * 4, hipMemcpyDeviceToHost, root.stream));
    HIP_TRY(hipStreamSynchronize(root.stream));
    return COS_OK;
}

extern "C" int32_t cos_shardset_hybrid_search_batch(cos_shardset *ss, const float *queries, const uint32_t *q_terms, const uint32_t *q_offsets, uint32_t B,
                                                    uint32_t top_k, float fusion_constant_k, uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    if (int32_t rc = text_check(ss, q_terms, q_offsets, B, top_k, out_ids, out_scores, out_counts, "cos_shardset_hybrid_search_batch")) return rc;
    if (!queries) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (top_k > 170) return cos_fail(COS_ERR_UNIMPLEMENTED, "top_k above 170: RRF lists longer than 1024 entries");
    const u32 k3 = 3 * top_k; // repo::hybrid_search asks both halves for top_k * 3
    if (int32_t wrc = check_merge_width(ss->world, k3)) return wrc;
    std::lock_guard<std::mutex> g(ss->mu);
    if (ss->bm.empty()) return cos_fail(COS_ERR_NOT_READY, "no BM25 shards attached (cos_shardset_attach_bm25)");
    TextLocks locks(ss);
    if (int32_t rc = check_text_ids(ss->bm, ss->bm_base, ss->first_rank)) return rc;
    LocalShard &root = ss->sh[0];
    const size_t words = (size_t)B * (2 * (size_t)k3 + 1), nk = (size_t)B * top_k, ret_words = 2 * nk + B;
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(ss->d_ret.grow(ret_words));
    HIP_TRY(ss->h_ret.grow(ret_words));
    DrainAll drain_all{ss};
    // 1. the dense half FIRST on every device (cos_hybrid_search_batch: the walk is a chain of dependent rounds, the scoring kernel fills
    //    whatever it leaves free), 2. the text half beside it, its host side prepared while the devices already walk
    int32_t rc = enqueue_walks(ss, queries, B, k3, words, &drain_all);
    if (rc) return rc;
    rc = text_lists(ss, drain_all, q_terms, q_offsets, B, k3);
    if (rc) return rc;
    // 3. the dense exchange and merge; both merged list sets are now on shard 0's device: RRF there, ONE copy back
    rc = exchange_merge(ss, B, k3, words);
    if (rc) return rc;
    u32 *d_fid = ss->d_ret, *d_fcnt = ss->d_ret + 2 * nk;
    float *d_fsc = reinterpret_cast<float *>(ss->d_ret + nk);
    rc = cosdev::rrf_fuse_device(ss->d_out_ids, ss->d_out_counts, ss->d_text_ids, ss->d_text_counts, k3, B, fusion_constant_k, top_k, d_fid, d_fsc, d_fcnt, root.stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ss->h_ret, ss->d_ret, ret_words * 4, hipMemcpyDeviceToHost, root.stream));
    rc = check_walk_statuses(ss, B); // (synchronises every shard's stream, shard 0's last)
    if (rc) return rc;
    const u32 *hr = ss->h_ret;
    memcpy(out_ids, hr, nk * 4);
    memcpy(out_scores, hr + nk, nk * 4);
    memcpy(out_counts, hr + 2 * nk, (size_t)B * 4);
    return COS_OK;
}

// ---- the learned-sparse half of the collection on a shard set, and the mixed hybrid call ------------------------------------------------
// (the scheme and why it is the whole index's answer bit for bit: kernels_sparse.hip, "The handle as one shard of a collection")
namespace {
// the locks of every attached learned-sparse handle, in shard order, until the call has synchronised (taken before any BM25 handle's)
struct SparseLocks {
    std::vector<std::unique_lock<std::mutex>> held;
    explicit SparseLocks(const std::vector<cos_sparse *> &sp) {
        for (cos_sparse *s : sp) held.emplace_back(cosdev::sparse_mutex(s));
    }
};

// a global id names one vector, and every shard quantizes alike (inserts move n, so every search asks again); locks held
int32_t check_sparse_ids(const std::vector<cos_sparse *> &sp, const std::vector<u32> &base, u32 first_rank) {
    u32 bits0 = 0;
    float upper0 = 0.0f;
    for (size_t s = 0; s < sp.size(); s++) {
        u32 bits = 0, n = 0;
        float upper = 0.0f;
        cosdev::sparse_shape(sp[s], &bits, &upper, &n);
        const u64 end = (u64)base[s] + n; // one past the shard's largest global id
        if (end >= 0xFFFFFFFFull)
            return cos_fail(COS_ERR_INVALID, "sparse shard %u: vec_base %u + %u vectors does not fit below 2^32 - 1", first_rank + (u32)s, base[s], n);
        if (s + 1 < sp.size() && end > base[s + 1])
            return cos_fail(COS_ERR_INVALID, "sparse shard %u: vec_base %u + %u vectors reaches into the next shard (vec_base %u)", first_rank + (u32)s, base[s], n,
                            base[s + 1]);
        if (s == 0) { bits0 = bits; upper0 = upper; }
        else if (bits != bits0 || memcmp(&upper, &upper0, 4) != 0)
            return cos_fail(COS_ERR_INVALID, "sparse shard %u: quantization_bits %u / values_upper_bound %g, shard %u has %u / %g", first_rank + (u32)s, bits, upper,
                            first_rank, bits0, upper0);
    }
    return COS_OK;
}

// what refuses a learned-sparse batch of B queries for top_k before anything is enqueued, in the order the single handle checks; locks held
int32_t check_sparse_limits(cos_shardset *ss, const uint32_t *q_offsets, u32 B, u32 top_k, u32 reranking_factor) {
    const u32 S = ss->world;
    const u64 C = (u64)top_k * (reranking_factor ? reranking_factor : 1u);
    u32 narrowest = 0xFFFFFFFFu;
    bool all_raw = true;
    for (cos_sparse *s : ss->sp) {
        u32 max_cand = 0, bound = 0;
        bool raw = false;
        cosdev::sparse_limits(s, &max_cand, &raw, &bound);
        if (B >= bound) return cos_fail(COS_ERR_INVALID, "batch of %u queries", B);
        narrowest = std::min(narrowest, max_cand);
        all_raw &= raw;
    }
    if (!hybrid_plan::offsets_ascend(q_offsets, B)) return cos_fail(COS_ERR_INVALID, "query offsets decrease");
    if (reranking_factor && !all_raw) return cos_fail(COS_ERR_NOT_READY, "raw-value rerank needs the raw sparse vectors on every shard");
    if (C > narrowest) return cos_fail(COS_ERR_UNIMPLEMENTED, "top_k x reranking_factor must be <= %u (the narrowest shard's cos_sparse_set_max_candidates)", narrowest);
    const sparse_fold_plan::Plan fp = sparse_fold_plan::plan(S, C);
    if (fp.status)
        return cos_fail(fp.status, "%u shards x %u candidate slots = %llu gathered keys per query: at most %u", S, sparse_fold_plan::record_stride(C),
                        (unsigned long long)fp.keys, sparse_fold_plan::MAX_KEYS);
    return COS_OK;
}

// every shard scans and writes its candidate record on its sparse stream; ONE exchange of the S records; the fold on shard 0's device
// leaves the collection's lists in d_ids / d_scores [B][top_k], d_counts [B]; everything enqueued, nothing synchronised
int32_t sparse_lists(cos_shardset *ss, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, u32 B, u32 top_k, float early_terminate_threshold,
                     u32 reranking_factor, u32 *d_ids, float *d_scores, u32 *d_counts) {
    const u32 S = ss->world;
    const u64 C = (u64)top_k * (reranking_factor ? reranking_factor : 1u);
    const sparse_fold_plan::Layout lay = sparse_fold_plan::layout(B, C, reranking_factor != 0);
    LocalShard &root = ss->sh[0];
    for (LocalShard &s : ss->sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(s.d_record_sp.grow(lay.words));
        if (ss->use_rccl || &s == &root) HIP_TRY(s.d_gathered_sp.grow(lay.words * S)); // (only the all-gather writes every shard's buffer)
    }
    for (u32 i = 0; i < S; i++) {
        LocalShard &s = ss->sh[i];
        int32_t rc = cosdev::sparse_record_locked(ss->sp[i], q_dims, q_vals, q_offsets, B, top_k, early_terminate_threshold, reranking_factor, ss->sp_base[i],
                                                  s.d_record_sp, s.stream_sp);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipEventRecord(s.done_sp, s.stream_sp));
        HIP_TRY(hipStreamWaitEvent(s.stream, s.done_sp, 0));
    }
    int32_t rc = exchange_local(ss, lay.words, Record::CANDIDATES);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(root.device));
    return cosdev::sparse_fold_rerank(root.d_gathered_sp, S, B, top_k, reranking_factor, d_ids, d_scores, d_counts, root.stream);
}

// h_ret = [ids B x k | scores B x k | counts B] -> the caller's arrays; entries past a query's count are not written
void copy_lists_out(const u32 *hr, u32 B, u32 top_k, uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    const size_t nk = (size_t)B * top_k;
    for (u32 q = 0; q < B; q++) {
        const u32 c = std::min(hr[2 * nk + q], top_k);
        memcpy(out_ids + (size_t)q * top_k, hr + (size_t)q * top_k, (size_t)c * 4);
        memcpy(out_scores + (size_t)q * top_k, hr + nk + (size_t)q * top_k, (size_t)c * 4);
        out_counts[q] = c;
    }
}
} // namespace

extern "C" int32_t cos_shardset_attach_sparse(cos_shardset *ss, cos_sparse *const *shards, uint32_t n_shards, const uint32_t *vec_bases) {
    if (!ss) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ss->sh.size() != ss->world) return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_shardset_attach_sparse needs every shard in this process");
    std::lock_guard<std::mutex> g(ss->mu);
    if (!shards) { // detach
        ss->sp.clear();
        ss->sp_base.clear();
        return COS_OK;
    }
    if (n_shards != ss->world) return cos_fail(COS_ERR_INVALID, "%u sparse handles for a set of %u shards", n_shards, ss->world);
    std::vector<cos_sparse *> sp(shards, shards + n_shards);
    std::vector<u32> base(n_shards);
    for (u32 s = 0; s < n_shards; s++) {
        if (!sp[s]) return cos_fail(COS_ERR_INVALID, "sparse shard %u is null", s);
        for (u32 t = 0; t < s; t++)
            if (sp[t] == sp[s]) return cos_fail(COS_ERR_INVALID, "sparse shards %u and %u are the same handle", t, s);
        if (cosdev::sparse_device(sp[s]) != ss->sh[s].device)
            return cos_fail(COS_ERR_INVALID, "sparse shard %u lives on device %d, its dense shard on device %d", s, cosdev::sparse_device(sp[s]), ss->sh[s].device);
        base[s] = vec_bases ? vec_bases[s] : ss->sh[s].ix->p.id_base;
        if (s && base[s] <= base[s - 1]) return cos_fail(COS_ERR_INVALID, "vec_bases must strictly increase (shard %u: %u after %u)", s, base[s], base[s - 1]);
    }
    {
        SparseLocks locks(sp);
        if (int32_t rc = check_sparse_ids(sp, base, ss->first_rank)) return rc;
    }
    ss->sp.swap(sp);
    ss->sp_base.swap(base);
    return COS_OK;
}

extern "C" int32_t cos_shardset_sparse_search_batch(cos_shardset *ss, const uint32_t *q_dims, const float *q_vals, const uint32_t *q_offsets, uint32_t B,
                                                    uint32_t top_k, float early_terminate_threshold, uint32_t reranking_factor, uint32_t *out_ids,
                                                    float *out_scores, uint32_t *out_counts) {
    if (!ss || !q_dims || !q_vals || !q_offsets || !out_ids || !out_scores || !out_counts || B == 0 || top_k == 0) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (ss->sh.size() != ss->world) return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_shardset_sparse_search_batch needs every shard in this process");
    std::lock_guard<std::mutex> g(ss->mu);
    if (ss->sp.empty()) return cos_fail(COS_ERR_NOT_READY, "no sparse shards attached (cos_shardset_attach_sparse)");
    SparseLocks locks(ss->sp);
    if (int32_t rc = check_sparse_ids(ss->sp, ss->sp_base, ss->first_rank)) return rc;
    if (int32_t rc = check_sparse_limits(ss, q_offsets, B, top_k, reranking_factor)) return rc;
    LocalShard &root = ss->sh[0];
    const size_t nk = (size_t)B * top_k, ret_words = 2 * nk + B;
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(ss->d_ret.grow(ret_words));
    HIP_TRY(ss->h_ret.grow(ret_words));
    DrainAll drain_all{ss};
    int32_t rc = sparse_lists(ss, q_dims, q_vals, q_offsets, B, top_k, early_terminate_threshold, reranking_factor, ss->d_ret, reinterpret_cast<float *>(ss->d_ret + nk),
                              ss->d_ret + 2 * nk);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ss->h_ret, ss->d_ret, ret_words * 4, hipMemcpyDeviceToHost, root.stream));
    HIP_TRY(hipStreamSynchronize(root.stream));
    copy_lists_out(ss->h_ret, B, top_k, out_ids, out_scores, out_counts);
    return COS_OK;
}

extern "C" int32_t cos_shardset_hybrid_search_mixed(cos_shardset *ss, const cos_hybrid_request *rq, uint32_t *out_ids, float *out_scores, uint32_t *out_counts) {
    namespace hp = hybrid_plan;
    if (!ss || !rq || !out_ids || !out_scores || !out_counts) return cos_fail(COS_ERR_INVALID, "bad argument");
    if (rq->struct_size < sizeof(cos_hybrid_request)) return cos_fail(COS_ERR_INVALID, "cos_hybrid_request.struct_size %u, expected %zu", rq->struct_size, sizeof(cos_hybrid_request));
    const u32 B = rq->B, top_k = rq->top_k, rf = rq->sparse_reranking_factor;
    int32_t rc = hp::check_request(rq->struct_size, (u32)sizeof(cos_hybrid_request), B, top_k);
    if (rc == COS_ERR_UNIMPLEMENTED) return cos_fail(rc, "top_k above %u: every half is asked for 3 * top_k, BM25 keeps %u buckets and the fusion holds two such lists", hp::MAX_TOP_K, hp::MAX_LIST);
    if (rc || !rq->arm) return cos_fail(COS_ERR_INVALID, "bad argument (B %u, top_k %u)", B, top_k);
    if (ss->sh.size() != ss->world) return cos_fail(COS_ERR_UNIMPLEMENTED, "cos_shardset_hybrid_search_mixed needs every shard in this process");
    const u32 k3 = hp::LIST_FACTOR * top_k, S = ss->world;
    std::lock_guard<std::mutex> g(ss->mu);
    // ---- the request's query_mapping and everything that refuses it: nothing is enqueued before the last check ----
    LocalShard &root = ss->sh[0];
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(ss->h_slots.grow(B)); // (no stream of the set is busy: every call drains them)
    hp::Split n;
    u32 bad = 0;
    if (hp::split(rq->arm, B, ss->h_slots, n, &bad)) return cos_fail(COS_ERR_INVALID, "arm %u of query %u", (u32)rq->arm[bad], bad);
    if ((n.n_dense && !rq->dense_queries) || (n.n_sparse && (!rq->sparse_dims || !rq->sparse_vals || !rq->sparse_offsets)) || (n.n_bm25 && (!rq->bm25_terms || !rq->bm25_offsets)))
        return cos_fail(COS_ERR_INVALID, "the queries of a half that has some are NULL");
    if (n.n_bm25 && !hp::offsets_ascend(rq->bm25_offsets, n.n_bm25)) return cos_fail(COS_ERR_INVALID, "BM25 query offsets decrease");
    if (n.n_dense)
        if (int32_t wrc = check_merge_width(S, k3)) return wrc;
    if (n.n_sparse && ss->sp.empty()) return cos_fail(COS_ERR_NOT_READY, "no sparse shards attached (cos_shardset_attach_sparse)");
    if (n.n_bm25 && ss->bm.empty()) return cos_fail(COS_ERR_NOT_READY, "no BM25 shards attached (cos_shardset_attach_bm25)");
    // the set's lock -> every sparse handle's -> every BM25 handle's; a half without queries takes none
    SparseLocks sparse_locks(n.n_sparse ? ss->sp : std::vector<cos_sparse *>());
    if (n.n_sparse) {
        if ((rc = check_sparse_ids(ss->sp, ss->sp_base, ss->first_rank))) return rc;
        if ((rc = check_sparse_limits(ss, rq->sparse_offsets, n.n_sparse, k3, rf))) return rc;
    }
    std::vector<std::unique_lock<std::mutex>> text_locks;
    if (n.n_bm25) {
        for (cos_bm25 *b : ss->bm) text_locks.emplace_back(cosdev::bm25_mutex(b));
        if ((rc = check_text_ids(ss->bm, ss->bm_base, ss->first_rank))) return rc;
    }
    // ---- buffers on shard 0's device (grow-only) ----
    const size_t words = (size_t)n.n_dense * (2 * (size_t)k3 + 1), nk = (size_t)B * top_k, ret_words = 2 * nk + B;
    HIP_TRY(ss->d_slots.grow(B));
    HIP_TRY(ss->d_ret.grow(ret_words));
    HIP_TRY(ss->h_ret.grow(ret_words));
    if (n.n_sparse) {
        HIP_TRY(ss->d_sp_ids.grow((size_t)n.n_sparse * k3));
        HIP_TRY(ss->d_sp_scores.grow((size_t)n.n_sparse * k3));
        HIP_TRY(ss->d_sp_counts.grow((size_t)n.n_sparse));
    }
    DrainAll drain_all{ss};
    // 1. the dense sub-batch FIRST on every device (beside a BM25 half: on the stream the attached handle keeps for the walk, as in
    //    cos_shardset_hybrid_search_batch), 2. the sparse records, 3. the BM25 buckets, each with its exchange and fold
    if (n.n_dense && (rc = enqueue_walks(ss, rq->dense_queries, n.n_dense, k3, words, n.n_bm25 ? &drain_all : nullptr))) return rc;
    if (n.n_sparse && (rc = sparse_lists(ss, rq->sparse_dims, rq->sparse_vals, rq->sparse_offsets, n.n_sparse, k3, rq->sparse_early_terminate_threshold, rf, ss->d_sp_ids,
                                         ss->d_sp_scores, ss->d_sp_counts)))
        return rc;
    if (n.n_bm25 && (rc = text_lists(ss, drain_all, rq->bm25_terms, rq->bm25_offsets, n.n_bm25, k3))) return rc;
    if (n.n_dense && (rc = exchange_merge(ss, n.n_dense, k3, words))) return rc;
    // 4. the three list sets are on shard 0's device: the fusion there, ONE copy back
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(hipMemcpyAsync(ss->d_slots, ss->h_slots, (size_t)B * sizeof(hp::Slot), hipMemcpyHostToDevice, root.stream));
    u32 *d_fid = ss->d_ret, *d_fcnt = ss->d_ret + 2 * nk;
    float *d_fsc = reinterpret_cast<float *>(ss->d_ret + nk);
    rc = cosdev::rrf_mixed_device(n.n_dense ? ss->d_out_ids.p : nullptr, n.n_dense ? ss->d_out_counts.p : nullptr, n.n_sparse ? ss->d_sp_ids.p : nullptr,
                                  n.n_sparse ? ss->d_sp_counts.p : nullptr, n.n_bm25 ? ss->d_text_ids.p : nullptr, n.n_bm25 ? ss->d_text_counts.p : nullptr, ss->d_slots, k3, B,
                                  rq->fusion_constant_k, top_k, d_fid, d_fsc, d_fcnt, root.stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ss->h_ret, ss->d_ret, ret_words * 4, hipMemcpyDeviceToHost, root.stream));
    if (n.n_dense) {
        if ((rc = check_walk_statuses(ss, n.n_dense))) return rc; // (synchronises every shard's stream, shard 0's last)
    } else {
        HIP_TRY(hipStreamSynchronize(root.stream));
    }
    copy_lists_out(ss->h_ret, B, top_k, out_ids, out_scores, out_counts);
    return COS_OK;
}
