// exact_rerank_check.hip — device check of cosdata_amd/csrc/exact_rerank.h: a miniature rerank built only from that header and
// dot_engines.h, against a host model of the rule written here (vector_store.rs:404-445: eight fused chains, their pairwise tree,
// an unfused tail, |q| * |x| as a product of its own, x86's negative NaN for 0/0, keys ordered as (simkey, id)).
// Test infrastructure: compiled and run by tests/test_gpu_exact_rerank.py with the library's floating-point flags.
// One workgroup per case.  Exit status: 0 every case matched (one OK line), 1 mismatch, 2 HIP error (returns at the first one and
// launches nothing further).  Everything compared is a u64 key or the bits of an output word: exact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "exact_rerank.h"

using cosdev::u32;
using cosdev::u64;

// ---- the miniature ---------------------------------------------------------------------------------------------------------------------
struct Case { // rows [nrows][dim] at x_off (stride = dim: rows are only 4-byte aligned), the query at q_off, candidates at c_off
    u32 dim, ncand, x_off, q_off, m_off, c_off;
    float mq;
};
constexpr int LDS_R = 4, LDS_WAVES = 4; // the LDS form: up to 256 candidates, four waves

// the pair passes: 32 candidates per pass, candidate j ends in lane j, one 64-key sort (ncand <= 64)
__global__ __launch_bounds__(64) void pair_rerank_kernel(const Case *cases, const float *f, const u32 *cand, u64 *out /*[cases][64]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *qf = (float *)smem_raw;
    const Case c = cases[blockIdx.x];
    const int lane = threadIdx.x;
    for (u32 i = lane; i < c.dim; i += 64) qf[i] = f[c.q_off + i];
    __syncthreads();
    u64 res[1] = {0ull};
    for (u32 base = 0; base < c.ncand; base += 32) {
        const u32 my = base + (u32)(lane >> 1);
        const u32 id = my < c.ncand ? cand[c.c_off + my] : 0u;
        const float dp = cosdev::f32_pair_dot(f + c.x_off + (u64)id * c.dim, qf, c.dim, lane & 1);
        cosdev::pair_keys_to_lanes(cosdev::exact_key(dp, c.mq, f[c.m_off + id], id, my < c.ncand), base, lane, res[0]);
    }
    cosdev::bitonic_sort_desc<1>(res, lane);
    out[(size_t)blockIdx.x * 64 + lane] = res[0];
}
// the LDS form: every wave dots 8 candidates per pass with the oct dot, keys to LDS, wave 0 sorts them
__global__ __launch_bounds__(64 * LDS_WAVES) void lds_rerank_kernel(const Case *cases, const float *f, const u32 *cand, u64 *out /*[cases][64 LDS_R]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const Case c = cases[blockIdx.x];
    float *qf = (float *)smem_raw;
    u64 *keys = (u64 *)(smem_raw + cosdev::staged_query_bytes(c.dim));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (u32 i = tid; i < c.dim; i += 64 * LDS_WAVES) qf[i] = f[c.q_off + i];
    __syncthreads();
    for (u32 base = (u32)wave * 8u; base < c.ncand; base += 8u * LDS_WAVES) {
        const u32 my = base + (u32)(lane >> 3);
        const u32 id = my < c.ncand ? cand[c.c_off + my] : 0u;
        const float dp = cosdev::f32_oct_dot(f + c.x_off + (u64)id * c.dim, qf, c.dim, lane & 7);
        const u64 key = cosdev::exact_key(dp, c.mq, f[c.m_off + id], id, true);
        if ((lane & 7) == 0 && my < c.ncand) keys[my] = key;
    }
    __syncthreads();
    if (wave != 0) return;
    u64 rk[LDS_R];
#pragma unroll
    for (int r = 0; r < LDS_R; r++) {
        const u32 e = (u32)lane * LDS_R + r;
        rk[r] = e < c.ncand ? keys[e] : 0ull;
    }
    cosdev::bitonic_sort_desc<LDS_R>(rk, lane);
#pragma unroll
    for (int r = 0; r < LDS_R; r++) out[(size_t)blockIdx.x * 64 * LDS_R + lane * LDS_R + r] = rk[r];
}
// sorted[q][64 R] -> write_topk
template <int R, bool FILL>
__global__ __launch_bounds__(64) void write_topk_kernel(const u64 *sorted, const u32 *nout, u32 k, u32 id_base, u32 *out_ids, float *out_scores) {
    const int lane = threadIdx.x;
    u64 res[R];
#pragma unroll
    for (int r = 0; r < R; r++) res[r] = sorted[(size_t)blockIdx.x * 64 * R + lane * R + r];
    cosdev::write_topk<R, FILL>(res, nout[blockIdx.x], k, blockIdx.x, id_base, out_ids, out_scores, lane);
}

// ---- the host model --------------------------------------------------------------------------------------------------------------------
static u32 bits(float v) { u32 b; memcpy(&b, &v, 4); return b; }
static float from_bits(u32 b) { float v; memcpy(&v, &b, 4); return v; }
static u32 host_simkey(float v) { const u32 b = bits(v); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
static float host_dot(const float *q, const float *x, u32 dim) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const u32 chunks = dim / 8;
    for (u32 c = 0; c < chunks; c++)
        for (int j = 0; j < 8; j++) s[j] = std::fmaf(q[8 * c + j], x[8 * c + j], s[j]);
    volatile float lo = (s[0] + s[1]) + (s[2] + s[3]), hi = (s[4] + s[5]) + (s[6] + s[7]);
    volatile float r = lo + hi;
    for (u32 i = chunks * 8; i < dim; i++) { // unfused: the product is rounded before it is added
        volatile float p = q[i] * x[i];
        r = r + p;
    }
    return r;
}
static u64 host_key(const float *q, const float *x, u32 dim, float mq, float xm, u32 id) {
    const float dp = host_dot(q, x, dim);
    volatile float den = mq * xm;
    float cs = dp / den;
    if (dp == 0.0f && den == 0.0f) cs = from_bits(0xFFC00000u); // 0/0 on x86: the negative NaN, last under total_cmp
    return ((u64)host_simkey(cs) << 32) | id;
}
static float host_norm(const float *x, u32 dim) { // sqrt of the sequential, unfused sum of squares
    volatile float acc = -0.0f;
    for (u32 i = 0; i < dim; i++) { volatile float p = x[i] * x[i]; acc = acc + p; }
    return std::sqrt(acc);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
struct DevBuf { // freed on every way out
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
template <typename T>
static int upload(DevBuf &d, const std::vector<T> &h) {
    CK(hipMalloc(&d.p, h.size() * sizeof(T) + 64));
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

static u32 g_rng = 12345u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return (float)((int)(g_rng >> 8) - (1 << 23)) / (float)(1 << 23); }

static int run_rerank(size_t &n_cases) {
    const u32 dims[] = {1, 7, 8, 9, 63, 64, 65, 72, 255, 256, 257, 264};
    const u32 counts[] = {0, 1, 31, 32, 33, 63, 64};
    std::vector<Case> cases;
    std::vector<float> f;
    std::vector<u32> cand;
    std::vector<std::vector<u64>> want;
    auto add = [&](u32 dim, u32 ncand, bool zero_query) {
        Case c{};
        c.dim = dim; c.ncand = ncand;
        const u32 nrows = std::max(ncand, 1u);
        c.x_off = (u32)f.size();
        for (u32 i = 0; i < nrows * dim; i++) f.push_back(rnd());
        if (nrows >= 3) {
            for (u32 i = 0; i < dim; i++) f[c.x_off + 1 * dim + i] = 0.0f;                  // a zero row: 0/0, ranks last
            for (u32 i = 0; i < dim; i++) f[c.x_off + 2 * dim + i] = f[c.x_off + i];        // rows 0 and 2 score alike: id 2 first
        }
        c.q_off = (u32)((f.size() + 3) / 4 * 4);
        f.resize(c.q_off);
        for (u32 i = 0; i < dim; i++) f.push_back(zero_query ? 0.0f : rnd());
        c.m_off = (u32)f.size();
        for (u32 r = 0; r < nrows; r++) f.push_back(host_norm(&f[c.x_off + r * dim], dim));
        c.mq = host_norm(&f[c.q_off], dim);
        c.c_off = (u32)cand.size();
        for (u32 j = 0; j < ncand; j++) cand.push_back(ncand - 1 - j);
        std::vector<u64> w;
        for (u32 j = 0; j < ncand; j++) w.push_back(host_key(&f[c.q_off], &f[c.x_off + j * dim], dim, c.mq, f[c.m_off + j], j));
        std::sort(w.begin(), w.end(), [](u64 a, u64 b) { return a > b; });
        cases.push_back(c);
        want.push_back(w);
    };
    for (u32 i = 0; i < 12; i++) {
        add(dims[i], counts[i % 7], false);
        add(dims[i], counts[(i + 3) % 7], false);
    }
    add(72, 65, false); add(257, 65, false); add(9, 130, false); add(264, 130, false); // more than 64: the LDS form only
    add(65, 33, true);                                                                  // a zero query: every score 0/0, ids descending
    // what the model itself must show before it judges the device
    for (size_t c = 0; c < cases.size(); c++) {
        const std::vector<u64> &w = want[c];
        if (cases[c].ncand < 3) continue;
        if ((u32)w.back() != 1u && cases[c].mq != 0.0f) return fprintf(stderr, "model: case %zu: the zero row is not last\n", c), 1;
        if ((w.back() >> 32) != (u64)host_simkey(from_bits(0xFFC00000u))) return fprintf(stderr, "model: case %zu: last key is not the negative NaN\n", c), 1;
        if (cases[c].mq == 0.0f) continue; // (a zero query: every score alike, the ids simply descend)
        const size_t p2 = std::find_if(w.begin(), w.end(), [](u64 k) { return (u32)k == 2u; }) - w.begin();
        if (p2 + 1 >= w.size() || (u32)w[p2 + 1] != 0u || (w[p2] >> 32) != (w[p2 + 1] >> 32)) return fprintf(stderr, "model: case %zu: equal scores, larger id not first\n", c), 1;
    }
    f.resize(f.size() + 16, 0.0f);
    DevBuf d_cases, d_f, d_cand, d_pair, d_lds;
    std::vector<u64> h_pair(cases.size() * 64, 0xDEADBEEFDEADBEEFull), h_lds(cases.size() * 64 * LDS_R, 0xDEADBEEFDEADBEEFull);
    cand.push_back(0u);
    TRY(upload(d_cases, cases)); TRY(upload(d_f, f)); TRY(upload(d_cand, cand)); TRY(upload(d_pair, h_pair)); TRY(upload(d_lds, h_lds));
    const size_t smem = cosdev::staged_query_bytes(264);
    hipLaunchKernelGGL(pair_rerank_kernel, dim3((u32)cases.size()), dim3(64), smem, 0, (const Case *)d_cases.p, (const float *)d_f.p, (const u32 *)d_cand.p, (u64 *)d_pair.p);
    CK(hipGetLastError());
    TRY(download(h_pair, d_pair));
    hipLaunchKernelGGL(lds_rerank_kernel, dim3((u32)cases.size()), dim3(64 * LDS_WAVES), smem + 64 * LDS_R * 8, 0, (const Case *)d_cases.p, (const float *)d_f.p,
                       (const u32 *)d_cand.p, (u64 *)d_lds.p);
    CK(hipGetLastError());
    TRY(download(h_lds, d_lds));
    int bad = 0;
    for (size_t c = 0; c < cases.size(); c++) {
        const std::vector<u64> &w = want[c];
        for (u32 e = 0; e < 64 * LDS_R; e++) {
            const u64 exp = e < w.size() ? w[e] : 0ull;
            if (h_lds[c * 64 * LDS_R + e] != exp && bad++ < 10)
                fprintf(stderr, "oct dot / LDS form: dim %u ncand %u position %u: %016llx, model %016llx\n", cases[c].dim, cases[c].ncand, e, h_lds[c * 64 * LDS_R + e], exp);
            if (cases[c].ncand <= 64 && e < 64 && h_pair[c * 64 + e] != exp && bad++ < 10) // (the pair kernel of a larger case sorts garbage: not looked at)
                fprintf(stderr, "pair dot / pair passes: dim %u ncand %u position %u: %016llx, model %016llx\n", cases[c].dim, cases[c].ncand, e, h_pair[c * 64 + e], exp);
        }
    }
    n_cases += cases.size();
    return bad ? 1 : 0;
}

template <int R, bool FILL>
static int run_write_topk(u32 k, size_t &n_cases) {
    constexpr u32 P = 64 * R, ID_BASE = 1000u, UNTOUCHED = 0xDEADBEEFu;
    const u32 have[3] = {k - 3, k, k + 5}; // fewer keys than k, exactly k, more
    std::vector<u64> sorted(3 * P, 0ull);
    std::vector<u32> nout(3), ids(3 * k, UNTOUCHED), sc(3 * k, UNTOUCHED);
    for (u32 q = 0; q < 3; q++) {
        for (u32 e = 0; e < have[q] && e < P; e++) sorted[q * P + e] = ((u64)host_simkey(1.0f - 0.001f * (float)e - (float)q) << 32) | (7u * (P - e) + q);
        nout[q] = FILL ? k : std::min(have[q], k);
    }
    DevBuf d_sorted, d_nout, d_ids, d_sc;
    TRY(upload(d_sorted, sorted)); TRY(upload(d_nout, nout)); TRY(upload(d_ids, ids)); TRY(upload(d_sc, sc));
    hipLaunchKernelGGL((write_topk_kernel<R, FILL>), dim3(3), dim3(64), 0, 0, (const u64 *)d_sorted.p, (const u32 *)d_nout.p, k, ID_BASE, (u32 *)d_ids.p, (float *)d_sc.p);
    CK(hipGetLastError());
    TRY(download(ids, d_ids)); TRY(download(sc, d_sc));
    int bad = 0;
    for (u32 q = 0; q < 3; q++)
        for (u32 e = 0; e < k; e++) {
            const u64 key = sorted[q * P + e];
            u32 want_id = UNTOUCHED, want_sc = UNTOUCHED;
            if (e < nout[q]) {
                const u32 sk = (u32)(key >> 32);
                want_id = key ? (u32)key + ID_BASE : 0xFFFFFFFFu;
                want_sc = key ? ((sk & 0x80000000u) ? (sk ^ 0x80000000u) : ~sk) : bits(0.0f);
            }
            if ((ids[q * k + e] != want_id || sc[q * k + e] != want_sc) && bad++ < 10)
                fprintf(stderr, "write_topk<%d, %d> k %u query %u entry %u: id %08x score %08x, model %08x %08x\n", R, (int)FILL, k, q, e, ids[q * k + e], sc[q * k + e], want_id, want_sc);
        }
    n_cases += 3;
    return bad ? 1 : 0;
}

int main() {
    int rc = 0, r;
    size_t n = 0;
#define STEP(call) do { r = (call); if (r == 2) return 2; rc |= r; } while (0)
    STEP(run_rerank(n));
    STEP((run_write_topk<1, false>(10, n)));
    STEP((run_write_topk<1, true>(32, n)));
    STEP((run_write_topk<2, false>(100, n)));
    STEP((run_write_topk<2, true>(100, n)));
    STEP((run_write_topk<4, false>(204, n)));
    STEP((run_write_topk<4, true>(250, n)));
    if (rc) {
        printf("MISMATCH (see stderr)\n");
        return 1;
    }
    printf("OK exact_rerank.h: %zu cases — pair and oct dot, pair passes and the LDS form against the host model at 12 dimensions, write_topk at R = 1, 2, 4, both forms\n", n);
    return 0;
}
