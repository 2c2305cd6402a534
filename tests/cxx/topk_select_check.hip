// topk_select_check.hip — device check of cosdata_amd/csrc/topk_select.h: every register network, Pool<R>, fold_stream<R> and the LDS
// networks, at the widths the kernels instantiate, against the models of topk_check_host.h (cases and verifiers are there).
// Test infrastructure: compiled and run by tests/test_gpu_topk_select.py (hipcc --offload-arch=gfx950 -I cosdata_amd/csrc).
// One workgroup per case, so a primitive at one width is one launch.  Exit status: 0 every case matched (one OK line), 1 mismatch,
// 2 HIP error (returns at the first one and launches nothing further).
#include <hip/hip_runtime.h>

#include "topk_check_host.h"
#include "topk_select.h"

using cosdev::u32;
using cosdev::u64;
using namespace tkc;

// ---- the wrappers ------------------------------------------------------------------------------------------------------------------------
enum { NET_SORT, NET_MERGE, NET_MERGE_SORTED };
template <int R, int NET>
__global__ __launch_bounds__(64) void reg_network_kernel(const u64 *in, u64 *out) { // in [cases][P] (NET_MERGE_SORTED: [cases][2 P]), out [cases][P]
    constexpr u32 P = 64 * R;
    const int lane = threadIdx.x;
    const u64 *src = in + (size_t)blockIdx.x * (NET == NET_MERGE_SORTED ? 2 * P : P);
    u64 k[R];
#pragma unroll
    for (int r = 0; r < R; r++) k[r] = src[lane * R + r];
    if constexpr (NET == NET_SORT) cosdev::bitonic_sort_desc<R>(k, lane);
    if constexpr (NET == NET_MERGE) cosdev::bitonic_merge_desc<R>(k, lane);
    if constexpr (NET == NET_MERGE_SORTED) {
        u64 other[R];
#pragma unroll
        for (int r = 0; r < R; r++) other[r] = src[P + lane * R + r];
        cosdev::merge_sorted_desc<R>(k, other, lane);
    }
#pragma unroll
    for (int r = 0; r < R; r++) out[(size_t)blockIdx.x * P + lane * R + r] = k[r];
}

// one wave replays the operations [case_off[c], case_off[c + 1]) and dumps the whole pool, the result and thr after each
template <int R>
__global__ __launch_bounds__(64) void pool_kernel(const PoolOp *ops, const u32 *case_off, const u64 *waves, u64 *out_pool, u64 *out_scalar) {
    constexpr u32 P = 64 * R;
    const int lane = threadIdx.x;
    cosdev::Pool<R> pool;
    pool.clear();
    u64 thr = 0;
    const u32 o0 = case_off[blockIdx.x], o1 = case_off[blockIdx.x + 1];
    for (u32 o = o0; o < o1; o++) {
        const u32 op = cosdev::uniform_u32(ops[o].op), arg = cosdev::uniform_u32(ops[o].arg);
        const u64 key = ((u64)cosdev::uniform_u32((u32)(ops[o].key >> 32)) << 32) | cosdev::uniform_u32((u32)ops[o].key);
        u64 res = 0;
        switch (op) {
        case OP_INSERT_AT: pool.insert_at(key, (int)arg, lane); break;
        case OP_POP_HEAD: pool.pop_head(lane); break;
        case OP_RANK_OF: res = (u64)pool.rank_of(key); break;
        case OP_HEAD: res = pool.head(); break;
        case OP_PEEK_DYN: res = pool.peek_dyn(arg); break;
        case OP_PEEK:
            res = arg == 0 ? pool.template peek<0>() : arg == 1 ? pool.template peek<R - 1>() : arg == 2 ? pool.template peek<R>() : pool.template peek<P - 1>();
            break;
        case OP_PEEK_NODE:
            res = arg == 0   ? pool.template peek_node<0>()
                  : arg == 1 ? pool.template peek_node<R - 1>()
                  : arg == 2 ? pool.template peek_node<R>()
                             : pool.template peek_node<P - 1>();
            break;
        case OP_FOLD_LANES: cosdev::pool_fold_lanes<R>(pool, thr, waves[(size_t)arg * 64 + lane], lane); break;
        case OP_FOLD_MASK: cosdev::pool_fold_mask<R>(pool, thr, waves[(size_t)arg * 64 + lane], key, lane); break;
        default: break;
        }
#pragma unroll
        for (int r = 0; r < R; r++) out_pool[(size_t)o * P + lane * R + r] = pool.e[r];
        if (lane == 0) {
            out_scalar[(size_t)o * 2] = res;
            out_scalar[(size_t)o * 2 + 1] = thr;
        }
    }
}

// desc[c] = {offset of stream 1, its count, offset of stream 2, its count or ~0 for "one call only"}
template <int R>
__global__ __launch_bounds__(64) void fold_stream_kernel(const u64 *keys, const uint4 *desc, u64 *out_pool, u64 *out_thr) {
    constexpr u32 P = 64 * R;
    __shared__ u64 batch[P];
    const int lane = threadIdx.x;
    const uint4 d = desc[blockIdx.x];
    const u32 cnt1 = cosdev::uniform_u32(d.y), cnt2 = cosdev::uniform_u32(d.w);
    u64 pool[R];
#pragma unroll
    for (int r = 0; r < R; r++) pool[r] = 0;
    u64 thr = 0;
    const u64 *s1 = keys + d.x, *s2 = keys + d.z;
    cosdev::fold_stream<R>(pool, thr, batch, cnt1, [&](u32 i) { return s1[i]; }, lane);
    if (cnt2 != 0xFFFFFFFFu) cosdev::fold_stream<R>(pool, thr, batch, cnt2, [&](u32 i) { return s2[i]; }, lane); // thr carried over
#pragma unroll
    for (int r = 0; r < R; r++) out_pool[(size_t)blockIdx.x * P + lane * R + r] = pool[r];
    if (lane == 0) out_thr[blockIdx.x] = thr;
}

enum { LDS_SORT, LDS_FOLD_MERGE, LDS_FOLD_MERGE_GLOBAL, LDS_MERGE_TWO };
template <u32 N, int NET>
__global__ void lds_network_kernel(const u64 *in, u64 *out) {
    constexpr u32 N_IN = NET == LDS_SORT ? N : 2 * N, N_OUT = NET == LDS_MERGE_TWO ? 2 * N : N;
    constexpr u32 N_BUF = NET == LDS_SORT || NET == LDS_FOLD_MERGE_GLOBAL ? N : NET == LDS_FOLD_MERGE ? 2 * N : 4 * N;
    __shared__ u64 buf[N_BUF];
    const u64 *src = in + (size_t)blockIdx.x * N_IN;
    u64 *dst = out + (size_t)blockIdx.x * N_OUT;
    if constexpr (NET == LDS_SORT) {
        for (u32 i = threadIdx.x; i < N; i += blockDim.x) buf[i] = src[i];
        cosdev::lds_bitonic_sort_desc<N>(buf);
        for (u32 i = threadIdx.x; i < N; i += blockDim.x) dst[i] = buf[i];
    } else if constexpr (NET == LDS_MERGE_TWO) { // as block_merge_pools: sequence j at buf + j * 2N
        for (u32 i = threadIdx.x; i < 2 * N; i += blockDim.x) buf[(i / N) * 2 * N + i % N] = src[i];
        cosdev::lds_bitonic_merge_desc<N>(buf, 2, 2 * N);
        for (u32 i = threadIdx.x; i < 2 * N; i += blockDim.x) dst[i] = buf[(i / N) * 2 * N + i % N];
    } else { // best in LDS; other in LDS (block_merge_pools) or in global memory (sparse_wide_finish_kernel)
        for (u32 i = threadIdx.x; i < N_BUF; i += blockDim.x) buf[i] = src[i];
        __syncthreads();
        if constexpr (NET == LDS_FOLD_MERGE) cosdev::fold_reversed<N>(buf, buf + N);
        else cosdev::fold_reversed<N>(buf, src + N);
        cosdev::lds_bitonic_merge_desc<N>(buf, 1, 0);
        for (u32 i = threadIdx.x; i < N; i += blockDim.x) dst[i] = buf[i];
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

struct DevBuf { // freed on every way out of a run
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
template <typename T>
static int upload(DevBuf &d, const std::vector<T> &h) {
    CK(hipMalloc(&d.p, h.size() * sizeof(T) + 16));
    if (!h.empty()) CK(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
template <typename T>
static int download(std::vector<T> &h, const DevBuf &d) {
    CK(hipDeviceSynchronize());
    if (!h.empty()) CK(hipMemcpy(h.data(), d.p, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}
#define TRY(x) do { if ((x) != 0) return 2; } while (0)

static size_t g_cases = 0;
static Report g_rep;

// a primitive whose cases are flat arrays of n_in keys in and n_out keys out; launch(cases, in, out) starts its one launch
template <typename Launch>
static int run_seq(const char *prim, const char *wname, u32 width, const std::vector<SeqCase> &cases, size_t n_in, size_t n_out, Launch launch) {
    std::vector<u64> h_in, h_out(cases.size() * n_out, 0xDEADBEEFDEADBEEFull);
    for (const SeqCase &c : cases) {
        if (c.in.size() != n_in || c.want.size() != n_out) return fprintf(stderr, "%s %s=%u case '%s': wrong size\n", prim, wname, width, c.name.c_str()), 1;
        h_in.insert(h_in.end(), c.in.begin(), c.in.end());
    }
    DevBuf d_in, d_out;
    TRY(upload(d_in, h_in));
    TRY(upload(d_out, h_out));
    launch((u32)cases.size(), (const u64 *)d_in.p, (u64 *)d_out.p);
    CK(hipGetLastError());
    TRY(download(h_out, d_out));
    size_t bad = 0;
    for (size_t c = 0; c < cases.size(); c++) bad += verify_seq(prim, wname, width, cases[c], &h_out[c * n_out], g_rep);
    g_cases += cases.size();
    return bad ? 1 : 0;
}

template <int R>
static int run_register_networks() {
    constexpr u32 P = 64 * R;
    int rc = run_seq("bitonic_sort_desc", "R", R, sort_cases(P, 1), P, P,
                     [](u32 n, const u64 *in, u64 *out) { hipLaunchKernelGGL((reg_network_kernel<R, NET_SORT>), dim3(n), dim3(64), 0, 0, in, out); });
    if (rc == 2) return 2;
    int rc2 = run_seq("bitonic_merge_desc", "R", R, bitonic_cases(P, R, 2), P, P,
                      [](u32 n, const u64 *in, u64 *out) { hipLaunchKernelGGL((reg_network_kernel<R, NET_MERGE>), dim3(n), dim3(64), 0, 0, in, out); });
    if (rc2 == 2) return 2;
    int rc3 = run_seq("merge_sorted_desc", "R", R, merge_sorted_cases(P, 3), 2 * P, P,
                      [](u32 n, const u64 *in, u64 *out) { hipLaunchKernelGGL((reg_network_kernel<R, NET_MERGE_SORTED>), dim3(n), dim3(64), 0, 0, in, out); });
    if (rc3 == 2) return 2;
    return rc | rc2 | rc3;
}

template <int R>
static int run_pool() {
    constexpr u32 P = 64 * R;
    const std::vector<PoolCase> cases = pool_cases(R, 4);
    std::vector<PoolOp> h_ops;
    std::vector<u32> h_off(1, 0u);
    std::vector<u64> h_waves;
    for (const PoolCase &c : cases) {
        const u32 slot0 = (u32)(h_waves.size() / 64);
        for (PoolOp o : c.ops) {
            if (o.op == OP_FOLD_LANES || o.op == OP_FOLD_MASK) o.arg += slot0;
            h_ops.push_back(o);
        }
        h_off.push_back((u32)h_ops.size());
        h_waves.insert(h_waves.end(), c.waves.begin(), c.waves.end());
    }
    std::vector<u64> h_pool(h_ops.size() * P, 0xDEADBEEFDEADBEEFull), h_scalar(h_ops.size() * 2, 0xDEADBEEFDEADBEEFull);
    DevBuf d_ops, d_off, d_waves, d_pool, d_scalar;
    TRY(upload(d_ops, h_ops));
    TRY(upload(d_off, h_off));
    TRY(upload(d_waves, h_waves));
    TRY(upload(d_pool, h_pool));
    TRY(upload(d_scalar, h_scalar));
    hipLaunchKernelGGL(pool_kernel<R>, dim3((u32)cases.size()), dim3(64), 0, 0, (const PoolOp *)d_ops.p, (const u32 *)d_off.p, (const u64 *)d_waves.p, (u64 *)d_pool.p,
                       (u64 *)d_scalar.p);
    CK(hipGetLastError());
    TRY(download(h_pool, d_pool));
    TRY(download(h_scalar, d_scalar));
    size_t bad = 0;
    for (size_t c = 0; c < cases.size(); c++) bad += verify_pool(R, cases[c], &h_pool[(size_t)h_off[c] * P], &h_scalar[(size_t)h_off[c] * 2], g_rep);
    g_cases += cases.size();
    return bad ? 1 : 0;
}

template <int R>
static int run_fold_stream() {
    constexpr u32 P = 64 * R;
    const std::vector<StreamCase> cases = stream_cases(P, 5);
    std::vector<u64> h_keys;
    std::vector<uint4> h_desc;
    for (const StreamCase &c : cases) {
        uint4 d;
        d.x = (u32)h_keys.size();
        d.y = (u32)c.s1.size();
        h_keys.insert(h_keys.end(), c.s1.begin(), c.s1.end());
        d.z = (u32)h_keys.size();
        d.w = c.twice ? (u32)c.s2.size() : 0xFFFFFFFFu;
        h_keys.insert(h_keys.end(), c.s2.begin(), c.s2.end());
        h_desc.push_back(d);
    }
    std::vector<u64> h_pool(cases.size() * P, 0xDEADBEEFDEADBEEFull), h_thr(cases.size(), 0xDEADBEEFDEADBEEFull);
    DevBuf d_keys, d_desc, d_pool, d_thr;
    TRY(upload(d_keys, h_keys));
    TRY(upload(d_desc, h_desc));
    TRY(upload(d_pool, h_pool));
    TRY(upload(d_thr, h_thr));
    hipLaunchKernelGGL(fold_stream_kernel<R>, dim3((u32)cases.size()), dim3(64), 0, 0, (const u64 *)d_keys.p, (const uint4 *)d_desc.p, (u64 *)d_pool.p, (u64 *)d_thr.p);
    CK(hipGetLastError());
    TRY(download(h_pool, d_pool));
    TRY(download(h_thr, d_thr));
    size_t bad = 0;
    for (size_t c = 0; c < cases.size(); c++) bad += verify_stream(R, cases[c], &h_pool[c * P], h_thr[c], g_rep);
    g_cases += cases.size();
    return bad ? 1 : 0;
}

template <u32 N>
static int run_lds_networks() {
    int rc = 0;
    for (u32 threads : LDS_THREADS) {
        const std::string tn = fmt("/threads=%llu", threads);
        auto named = [&](std::vector<SeqCase> c) {
            for (SeqCase &x : c) x.name += tn;
            return c;
        };
        int r = run_seq("lds_bitonic_sort_desc", "N", N, named(sort_cases(N, 6)), N, N,
                        [&](u32 n, const u64 *in, u64 *out) { hipLaunchKernelGGL((lds_network_kernel<N, LDS_SORT>), dim3(n), dim3(threads), 0, 0, in, out); });
        if (r == 2) return 2;
        rc |= r;
        r = run_seq("fold_reversed+lds_bitonic_merge_desc(1),other_in_lds", "N", N, named(merge_sorted_cases(N, 7)), 2 * N, N,
                    [&](u32 n, const u64 *in, u64 *out) { hipLaunchKernelGGL((lds_network_kernel<N, LDS_FOLD_MERGE>), dim3(n), dim3(threads), 0, 0, in, out); });
        if (r == 2) return 2;
        rc |= r;
        r = run_seq("fold_reversed+lds_bitonic_merge_desc(1),other_in_global", "N", N, named(merge_sorted_cases(N, 7)), 2 * N, N,
                    [&](u32 n, const u64 *in, u64 *out) { hipLaunchKernelGGL((lds_network_kernel<N, LDS_FOLD_MERGE_GLOBAL>), dim3(n), dim3(threads), 0, 0, in, out); });
        if (r == 2) return 2;
        rc |= r;
        r = run_seq("lds_bitonic_merge_desc(2)", "N", N, named(two_seq_cases(N, 8)), 2 * N, 2 * N,
                    [&](u32 n, const u64 *in, u64 *out) { hipLaunchKernelGGL((lds_network_kernel<N, LDS_MERGE_TWO>), dim3(n), dim3(threads), 0, 0, in, out); });
        if (r == 2) return 2;
        rc |= r;
    }
    return rc;
}

int main() {
    int rc = 0, r;
#define STEP(call) do { r = (call); if (r == 2) return 2; rc |= r; } while (0)
    STEP(run_register_networks<1>());
    STEP(run_register_networks<2>());
    STEP(run_register_networks<4>());
    STEP(run_register_networks<8>());
    STEP(run_register_networks<16>());
    STEP(run_pool<1>());
    STEP(run_pool<2>());
    STEP(run_pool<4>());
    STEP(run_pool<8>());
    STEP(run_pool<16>());
    STEP(run_fold_stream<2>());
    STEP(run_fold_stream<4>());
    STEP(run_fold_stream<8>());
    STEP(run_fold_stream<16>());
    STEP(run_lds_networks<128>());
    STEP(run_lds_networks<256>());
    STEP(run_lds_networks<512>());
    STEP(run_lds_networks<1024>());
    if (rc) {
        printf("MISMATCH (%d printed, see stderr)\n", g_rep.printed);
        return 1;
    }
    printf("OK topk_select.h: %zu cases — bitonic_sort_desc, bitonic_merge_desc, merge_sorted_desc, Pool at R = 1, 2, 4, 8, 16; fold_stream at R = 2, 4, 8, 16; "
           "the LDS networks at N = 128, 256, 512, 1024 with 256 and 192 threads — every key where the model puts it\n",
           g_cases);
    return 0;
}
