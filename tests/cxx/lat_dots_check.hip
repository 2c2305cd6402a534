// lat_dots_check.hip — device check of the latency kernels' evaluation blocks (walk_common.h), value by value against the host models of
// lat_dots_host.h (which tests/test_lat_dots_model.py pins to the oracle):
//   stage_float_query<ENG, 64> / <ENG, 256> + float_row_dot_wave<ENG>, spec_f32_dots<4>, spec_f16_dots<64, 128> / <32, 64>,
//   int_row_dot_group0<ENG, CH> and spec_row_dots<ENG, CH, 16, 8> for ENG_Q1 / ENG_Q3 and CH = 1 .. 4.
// One workgroup per case, called as the two kernels call them: a 64-thread probe lays its LDS out as walk_lat_kernel does (ef 256, rows
// of 256 slots) and a 256-thread probe as walk_lat4_kernel does (ef 256, pool of 256, rows of 64 slots) — both at their largest — and
// there the LAST wave evaluates, on the last row tile.  A case is (metric, query, T): cl[] holds T rows of a 512-row table (repeats inside
// a block and across blocks, the table's last row, a zero row) at T distinct positions of the 256 slots; spec[] is pre-filled with a
// sentinel that every other slot must still hold.  T = 0 .. 256 at one dim per storage, the block edges at the others; cosine and dot
// product everywhere, metric id 1 (whose key metric_key complements) at the full-T dim.
// Test infrastructure: compiled and run by tests/test_gpu_lat_dots.py with the library's flags for kernels_walk_lat*.hip.
// Exit status: 0 every word matched (one OK line with the words compared per storage), 1 mismatch, 2 HIP error (returns at the first
// one and launches nothing further).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "lat_dots_host.h"
#include "walk_common.h"
#include "walk_plan.h"

using namespace cosdev;

constexpr u64 SENTINEL = 0xA5A5A5A5DEADBEEFull;
constexpr u32 SLOTS = 256, PROBE_EF = 256, LAT_MMAX = 256, LAT4_MMAX = 64, LAT4_CAP = 256;

struct Case { u32 metric, query, T, single_row; };

// ENG / CH as the kernels instantiate them; NT = 64: walk_lat_kernel's layout, NT = 256: walk_lat4_kernel's (E = 1)
template <int ENG, int CH, int NT>
__global__ __launch_bounds__(NT) void probe_kernel(IndexDev ix, const Case *cases, const u64 *cl_all, const uint8_t *qcodes, const float *qmags, u64 *spec_out, u32 *single_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr bool FLOAT_ENG = ENG == ENG_F32 || ENG == ENG_F16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Case cs = cases[blockIdx.x];
    ix.metric = cs.metric;
    u64 *s_spec, *s_cl;
    float *s_q = nullptr;
    u32 *tile = nullptr;
    if constexpr (NT == 64) { // kernels_walk_lat.hip
        s_spec = (u64 *)smem_raw;
        s_cl = s_spec + 4 * 64;
        if constexpr (FLOAT_ENG) {
            const u32 own = (u32)(4 * 64 * 8 * 2) + PROBE_EF * 8u + LAT_MMAX * 8u;
            s_q = (float *)(smem_raw + ((own + 15u) & ~15u));
            tile = (u32 *)((unsigned char *)s_q + lat_float_query_bytes(ENG, ix.dim));
        }
    } else { // kernels_walk_lat4.hip
        unsigned char *p = smem_raw;
        p += (size_t)2 * LAT4_CAP * 8; // pools
        p += (size_t)PROBE_EF * 8;     // popped list
        p += (size_t)4 * 64 * 8;       // winners
        s_cl = (u64 *)p;   p += (size_t)4 * 64 * 8;
        s_spec = (u64 *)p; p += (size_t)4 * 64 * 8;
        p += (size_t)64 * LAT4_MMAX * 4; // claim table
        p += (size_t)2 * LAT4_MMAX * 4;  // filter
        p += (size_t)4 * 4;              // flags
        p += 16;                         // hand-over words
        if constexpr (FLOAT_ENG) {
            s_q = (float *)(smem_raw + (((u32)(p - smem_raw) + 15u) & ~15u));
            tile = (u32 *)((unsigned char *)s_q + lat_float_query_bytes(ENG, ix.dim)) + (size_t)wave * (lat_f16_tile_bytes(LAT4_F16_TILE_ROWS, LAT4_F16_TILE_DIMS) / 4u);
        }
    }
    for (u32 i = tid; i < SLOTS; i += NT) {
        s_cl[i] = cl_all[(size_t)blockIdx.x * SLOTS + i];
        s_spec[i] = SENTINEL;
    }
    const uint8_t *qcode = qcodes + (u64)cs.query * ix.row_stride;
    const float qmag = qmags[cs.query];
    const int lig = lane & (LAT_ROW_LANES - 1), grp = lane / LAT_ROW_LANES;
    uint4 qreg[CH];
    if constexpr (FLOAT_ENG) {
        stage_float_query<ENG, NT>(s_q, qcode, ix, tid);
    } else {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const u32 chunk = (u32)lig + (u32)c * (u32)LAT_ROW_LANES;
            qreg[c] = chunk < ix.nchunks ? *(const uint4 *)(qcode + (u64)chunk * 16) : make_uint4(0, 0, 0, 0);
        }
    }
    __syncthreads();
    if (wave == NT / 64 - 1) {
        const uint8_t *row_ptr = ix.codes + (u64)cs.single_row * ix.row_stride;
        u32 single;
        if constexpr (FLOAT_ENG) single = __float_as_uint(float_row_dot_wave<ENG>(row_ptr, s_q, ix.dim, lane));
        else single = int_row_dot_group0<ENG, CH>(qreg, row_ptr, ix.nchunks, lig, grp, LAT_ROW_LANES);
        if (lane == 63) single_out[blockIdx.x] = single; // "the dot in every lane": the last one tells
        if constexpr (ENG == ENG_F32) spec_f32_dots<4>(s_cl, s_spec, cs.T, s_q, ix, qmag, lane);
        else if constexpr (ENG == ENG_F16) {
            if constexpr (NT == 64) spec_f16_dots<(int)LAT_F16_TILE_ROWS, (int)LAT_F16_TILE_DIMS>(s_cl, s_spec, cs.T, s_q, tile, ix, qmag, lane);
            else spec_f16_dots<(int)LAT4_F16_TILE_ROWS, (int)LAT4_F16_TILE_DIMS>(s_cl, s_spec, cs.T, s_q, tile, ix, qmag, lane);
        } else spec_row_dots<ENG, CH, LAT_ROW_LANES, 8>(s_cl, s_spec, cs.T, qreg, ix, qmag, lig, grp);
    }
    __syncthreads();
    for (u32 i = tid; i < SLOTS; i += NT) spec_out[(size_t)blockIdx.x * SLOTS + i] = s_spec[i];
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define TRY(x) do { if ((x) != 0) return 2; } while (0)

struct DevBuf { // freed on every way out of a run
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
template <typename T>
static int upload(DevBuf &d, const std::vector<T> &h) {
    CK(hipMalloc(&d.p, h.size() * sizeof(T)));
    CK(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

static int g_printed = 0;
static size_t g_bad = 0;
static void mismatch(const char *what, int st, u32 dim, int nt, const Case &c, u32 pos, u64 got, u64 want) {
    g_bad++;
    if (g_printed++ < 12)
        fprintf(stderr, "MISMATCH %s: storage %s dim %u threads %d metric %u query %u T %u position %u: device %016llx model %016llx\n", what, ldm::storage_name(st), dim, nt,
                c.metric, c.query, c.T, pos, got, want);
}

template <int ENG, int CH, int NT>
static hipError_t launch(u32 n, u32 smem, const IndexDev &ix, const DevBuf &cases, const DevBuf &cl, const DevBuf &q, const DevBuf &qm, const DevBuf &spec, const DevBuf &single) {
    hipLaunchKernelGGL((probe_kernel<ENG, CH, NT>), dim3(n), dim3(NT), smem, 0, ix, (const Case *)cases.p, (const u64 *)cl.p, (const uint8_t *)q.p, (const float *)qm.p,
                       (u64 *)spec.p, (u32 *)single.p);
    return hipGetLastError();
}
template <int ENG>
static hipError_t launch_ch(u32 ch, u32 n, u32 smem, const IndexDev &ix, const DevBuf &cases, const DevBuf &cl, const DevBuf &q, const DevBuf &qm, const DevBuf &spec, const DevBuf &single) {
    switch (ch) {
    case 1: return launch<ENG, 1, 64>(n, smem, ix, cases, cl, q, qm, spec, single);
    case 2: return launch<ENG, 2, 64>(n, smem, ix, cases, cl, q, qm, spec, single);
    case 3: return launch<ENG, 3, 64>(n, smem, ix, cases, cl, q, qm, spec, single);
    case 4: return launch<ENG, 4, 64>(n, smem, ix, cases, cl, q, qm, spec, single);
    default: return hipErrorInvalidValue;
    }
}

// one (storage, dim): the table, the queries, every case in one launch per probe; words: the compared words of the storage
static int run_dim(int st, u32 dim, bool full_T, size_t &words) {
    using namespace ldm;
    const u32 stride = row_stride(st, dim);
    std::vector<std::vector<uint8_t>> ref_rows(TABLE_ROWS), ref_q(N_QUERIES);
    std::vector<uint8_t> codes((size_t)TABLE_ROWS * stride), qcodes((size_t)N_QUERIES * stride);
    std::vector<float> mags(TABLE_ROWS), qmags(N_QUERIES);
    for (u32 r = 0; r < TABLE_ROWS; r++) {
        ref_rows[r] = gen_row(st, dim, r, SEED_TABLE);
        to_device_layout(st, dim, ref_rows[r].data(), &codes[(size_t)r * stride]);
        mags[r] = row_mag(st, dim, ref_rows[r].data(), r == ZERO_ROWS[0] || r == ZERO_ROWS[1] || r == ZERO_ROWS[2]);
    }
    for (u32 q = 0; q < N_QUERIES; q++) {
        ref_q[q] = gen_row(st, dim, q, SEED_QUERY);
        to_device_layout(st, dim, ref_q[q].data(), &qcodes[(size_t)q * stride]);
        qmags[q] = row_mag(st, dim, ref_q[q].data(), q == ZERO_QUERY);
    }
    std::vector<float> dots((size_t)N_QUERIES * TABLE_ROWS); // the model, once per (query, row)
    for (u32 q = 0; q < N_QUERIES; q++)
        for (u32 r = 0; r < TABLE_ROWS; r++) dots[(size_t)q * TABLE_ROWS + r] = model_dot(st, dim, ref_q[q].data(), ref_rows[r].data());

    std::vector<u32> Ts;
    if (full_T) for (u32 t = 0; t <= SLOTS; t++) Ts.push_back(t);
    else Ts = {1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256};
    std::vector<u32> metrics = {0u, 3u};
    if (full_T) metrics.push_back(1u);
    std::vector<Case> cases;
    std::vector<u64> cl;
    Rng rng = rng_for(st, dim, 0xC1u, 7u);
    for (u32 metric : metrics)
        for (u32 q = 0; q < N_QUERIES; q++)
            for (u32 T : Ts) {
                u32 pos[SLOTS], row[SLOTS];
                for (u32 i = 0; i < SLOTS; i++) pos[i] = i;
                for (u32 i = 0; i < T; i++) { // a random injection of the T candidates into the slots
                    const u32 j = i + rng.below(SLOTS - i);
                    std::swap(pos[i], pos[j]);
                    row[i] = rng.below(TABLE_ROWS);
                }
                if (T >= 2) row[1] = row[0];                 // the same row twice in one block
                if (T >= 3) row[T / 2] = TABLE_ROWS - 1;     // the table's last row: its last 16 bytes end the allocation
                if (T >= 4 && (T & 1u)) row[2] = ZERO_ROWS[T % 3]; // one bad candidate among good ones
                if (T > 64) row[T - 1] = row[0];             // ... and in two blocks
                cases.push_back(Case{metric, q, T, T ? row[T - 1] : TABLE_ROWS - 1});
                // past T nothing may be read: those entries name row 0 and the slots nobody owns, so a block that did would break a sentinel
                for (u32 i = 0; i < SLOTS; i++) cl.push_back((u64)(i < T ? row[i] : 0u) | (u64)pos[i] << 32);
            }

    IndexDev ix{};
    DevBuf d_codes, d_mags, d_q, d_qm, d_cases, d_cl;
    TRY(upload(d_codes, codes));
    TRY(upload(d_mags, mags));
    TRY(upload(d_q, qcodes));
    TRY(upload(d_qm, qmags));
    TRY(upload(d_cases, cases));
    TRY(upload(d_cl, cl));
    ix.codes = (const uint8_t *)d_codes.p, ix.mags = (const float *)d_mags.p;
    ix.row_stride = stride, ix.n = TABLE_ROWS, ix.dim = dim, ix.nchunks = n_chunks(st, dim);
    const int eng = st == ST_F32 ? ENG_F32 : st == ST_F16 ? ENG_F16 : st == ST_BIN ? ENG_Q1 : ENG_Q3;
    const bool flt = st == ST_F32 || st == ST_F16;
    const u32 n = (u32)cases.size();
    for (int nt : {64, 256}) {
        if (nt == 256 && !flt) break; // the integer blocks are the same call in both kernels
        const u32 smem = nt == 64 ? walk_lat_lds_bytes(eng, dim, PROBE_EF, LAT_MMAX) : walk_lat4_lds_bytes(eng, dim, PROBE_EF, LAT4_CAP, LAT4_MMAX, 1);
        if (smem > 65536u) return fprintf(stderr, "storage %s dim %u: %u bytes of LDS\n", storage_name(st), dim, smem), 1;
        std::vector<u64> spec((size_t)n * SLOTS, 0ull);
        std::vector<u32> single(n, 0xDEADBEEFu);
        DevBuf d_spec, d_single;
        TRY(upload(d_spec, spec));
        TRY(upload(d_single, single));
        hipError_t e;
        if (eng == ENG_F32) e = nt == 64 ? launch<ENG_F32, 1, 64>(n, smem, ix, d_cases, d_cl, d_q, d_qm, d_spec, d_single) : launch<ENG_F32, 1, 256>(n, smem, ix, d_cases, d_cl, d_q, d_qm, d_spec, d_single);
        else if (eng == ENG_F16) e = nt == 64 ? launch<ENG_F16, 1, 64>(n, smem, ix, d_cases, d_cl, d_q, d_qm, d_spec, d_single) : launch<ENG_F16, 1, 256>(n, smem, ix, d_cases, d_cl, d_q, d_qm, d_spec, d_single);
        else if (eng == ENG_Q1) e = launch_ch<ENG_Q1>((ix.nchunks + 15u) / 16u, n, smem, ix, d_cases, d_cl, d_q, d_qm, d_spec, d_single);
        else e = launch_ch<ENG_Q3>((ix.nchunks + 15u) / 16u, n, smem, ix, d_cases, d_cl, d_q, d_qm, d_spec, d_single);
        CK(e);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(spec.data(), d_spec.p, spec.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(single.data(), d_single.p, single.size() * 4, hipMemcpyDeviceToHost));
        for (u32 c = 0; c < n; c++) {
            const Case &cs = cases[c];
            u64 want[SLOTS];
            for (u32 i = 0; i < SLOTS; i++) want[i] = SENTINEL;
            for (u32 i = 0; i < cs.T; i++) {
                const u64 e = cl[(size_t)c * SLOTS + i];
                want[(u32)(e >> 32)] = parked_word(cs.metric, dots[(size_t)cs.query * TABLE_ROWS + (u32)e], qmags[cs.query], mags[(u32)e]);
            }
            for (u32 i = 0; i < SLOTS; i++) {
                const u64 got = spec[(size_t)c * SLOTS + i];
                if (want[i] == SENTINEL ? got != SENTINEL : !same_word(cs.metric, got, want[i])) mismatch(want[i] == SENTINEL ? "slot not owned" : "parked word", st, dim, nt, cs, i, got, want[i]);
            }
            const float sd = dots[(size_t)cs.query * TABLE_ROWS + cs.single_row];
            const u32 sw = flt ? bits_of(sd) : (u32)sd; // the integer dot itself (below 2^24: exact in the f32 the model returns)
            if (flt ? !same_f32(single[c], sw) : single[c] != sw) mismatch("single row", st, dim, nt, cs, cs.single_row, single[c], sw);
            words += SLOTS + 1;
        }
    }
    return 0;
}

int main() {
    using namespace ldm;
    const u32 full_dim[4] = {100, 135, 2049, 1025}; // every T = 0 .. 256 here: a tail and a partial batch of steps; tiles with an n % 8 tail; CH 2; CH 3
    size_t words[4] = {0, 0, 0, 0};
    for (int st : {ST_F32, ST_F16, ST_BIN, ST_OCT})
        for (u32 dim : sweep_dims(st)) {
            const int r = run_dim(st, dim, dim == full_dim[st], words[st]);
            if (r) return r == 2 ? 2 : (printf("MISMATCH (see stderr)\n"), 1);
        }
    if (g_bad) {
        printf("MISMATCH %zu words (see stderr)\n", g_bad);
        return 1;
    }
    printf("OK words compared (256 slots + the single-row dot per case): f32 %zu, f16 %zu, binary %zu, octal %zu\n", words[0], words[1], words[2], words[3]);
    return 0;
}
