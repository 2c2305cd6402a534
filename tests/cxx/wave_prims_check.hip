// wave_prims_check.hip — device check of three wave primitives the walks rest on, against the models of topk_check_host.h:
//   group_reduce_add_u32(v, G), G = 1 .. 64 (device_common.h): wrapping u32 sums over aligned groups, in every lane of the group;
//   vis_alias_winners (walk_common.h): of the lanes in cmask that share a filter residue, the lowest wins;
//   div_rn_unscaled (device_common.h): the bits of the IEEE quotient, on (a) the operands the walk can form and (b) the range the
//   header states, about 2^24 pairs each in one launch.
// Test infrastructure: compiled and run by tests/test_gpu_wave_prims.py (hipcc --offload-arch=gfx950 -I cosdata_amd/csrc).
// Exit status: 0 every case matched (one OK line), 1 mismatch, 2 HIP error (returns at the first one and launches nothing further).
#include <hip/hip_runtime.h>

#include "topk_check_host.h"
#include "walk_common.h"

using cosdev::u32;
using cosdev::u64;
using namespace tkc;

__global__ __launch_bounds__(64) void group_reduce_kernel(const u32 *in, u32 *out, int G) { // [waves][64]
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    out[i] = cosdev::group_reduce_add_u32(in[i], G);
}
// per case: 64 residues, then cmask and lostmask; one wave per case
__global__ __launch_bounds__(64) void alias_kernel(const u32 *bit, const u64 *masks, u64 *out) {
    const u64 cmask = cosdev::readlane_u64(masks[(size_t)blockIdx.x * 2], 0), lostmask = cosdev::readlane_u64(masks[(size_t)blockIdx.x * 2 + 1], 0);
    const u64 w = cosdev::vis_alias_winners(cmask, bit[(size_t)blockIdx.x * 64 + threadIdx.x], lostmask);
    if (threadIdx.x == 0) out[blockIdx.x] = w;
}
__global__ __launch_bounds__(256) void div_kernel(const float *num, const float *den, float *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = cosdev::div_rn_unscaled(num[i], den[i]);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define TRY(x) do { if ((x) != 0) return 2; } while (0)

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

static Report g_rep;

static int run_group_reduce() {
    const std::vector<u32> in = group_inputs(GROUP_WAVES, 9);
    DevBuf d_in;
    TRY(upload(d_in, in));
    int rc = 0;
    for (u32 G : GROUP_SIZES) {
        std::vector<u32> got(in.size(), 0xDEADBEEFu);
        DevBuf d_out;
        TRY(upload(d_out, got));
        hipLaunchKernelGGL(group_reduce_kernel, dim3(GROUP_WAVES), dim3(64), 0, 0, (const u32 *)d_in.p, (u32 *)d_out.p, (int)G);
        CK(hipGetLastError());
        TRY(download(got, d_out));
        if (verify_group(G, in, got.data(), g_rep)) rc = 1;
    }
    return rc;
}

static int run_alias(size_t &n_cases) {
    const std::vector<AliasCase> cases = alias_cases(10);
    std::vector<u32> bit;
    std::vector<u64> masks, got(cases.size(), 0xDEADBEEFDEADBEEFull);
    for (const AliasCase &c : cases) {
        if (!alias_case_contract(c)) return fprintf(stderr, "vis_alias_winners case '%s': lostmask is not what the atomics can leave\n", c.name.c_str()), 1;
        bit.insert(bit.end(), c.bit, c.bit + 64);
        masks.push_back(c.cmask);
        masks.push_back(c.lostmask);
    }
    DevBuf d_bit, d_masks, d_out;
    TRY(upload(d_bit, bit));
    TRY(upload(d_masks, masks));
    TRY(upload(d_out, got));
    hipLaunchKernelGGL(alias_kernel, dim3((u32)cases.size()), dim3(64), 0, 0, (const u32 *)d_bit.p, (const u64 *)d_masks.p, (u64 *)d_out.p);
    CK(hipGetLastError());
    TRY(download(got, d_out));
    size_t bad = 0;
    for (size_t c = 0; c < cases.size(); c++) bad += verify_alias(cases[c], got[c], g_rep);
    n_cases = cases.size();
    return bad ? 1 : 0;
}

// both sets in one launch; bad_a / bad_b: the mismatch counts of (a) the walk's operands and (b) the stated range
static int run_div(size_t &na, size_t &nb, size_t &bad_a, size_t &bad_b) {
    DivPairs p;
    div_walk_pairs(p, (size_t)1 << 24, 11);
    na = p.size();
    div_range_pairs(p, (size_t)1 << 24, 12);
    nb = p.size() - na;
    const std::vector<float> want = div_model(p);
    std::vector<float> got(p.size(), -1.0f);
    DevBuf d_num, d_den, d_out;
    TRY(upload(d_num, p.num));
    TRY(upload(d_den, p.den));
    TRY(upload(d_out, got));
    hipLaunchKernelGGL(div_kernel, dim3((u32)((p.size() + 255) / 256)), dim3(256), 0, 0, (const float *)d_num.p, (const float *)d_den.p, (float *)d_out.p, p.size());
    CK(hipGetLastError());
    TRY(download(got, d_out));
    Report rep_a, rep_b; // eight lines each: a mismatch in (a) is a walk bug, one in (b) alone a comment to correct
    bad_a = verify_div("a:walk_operands", p, 0, na, got.data(), want.data(), rep_a);
    bad_b = verify_div("b:stated_range", p, na, p.size(), got.data(), want.data(), rep_b);
    if (bad_b) { // where: the range to state instead is read off this
        float nlo = 3e38f, nhi = 0, dlo = 3e38f, dhi = 0;
        for (size_t i = na; i < p.size(); i++)
            if (bits_of_f32(got[i]) != bits_of_f32(want[i])) {
                nlo = std::min(nlo, p.num[i]); nhi = std::max(nhi, p.num[i]);
                dlo = std::min(dlo, p.den[i]); dhi = std::max(dhi, p.den[i]);
            }
        fprintf(stderr, "div_rn_unscaled set b: %zu of %zu differ, num in [%.9g, %.9g], den in [%.9g, %.9g]\n", bad_b, nb, (double)nlo, (double)nhi, (double)dlo, (double)dhi);
    }
    return bad_a || bad_b ? 1 : 0;
}

int main() {
    int rc = 0, r;
    size_t n_alias = 0, na = 0, nb = 0, bad_a = 0, bad_b = 0;
    r = run_group_reduce();
    if (r == 2) return 2;
    rc |= r;
    r = run_alias(n_alias);
    if (r == 2) return 2;
    rc |= r;
    r = run_div(na, nb, bad_a, bad_b);
    if (r == 2) return 2;
    rc |= r;
    if (rc) {
        printf("MISMATCH (see stderr; div_rn_unscaled: %zu of %zu walk operands, %zu of %zu of the stated range)\n", bad_a, na, bad_b, nb);
        return 1;
    }
    printf("OK group_reduce_add_u32 at G = 1, 2, 4, 8, 16, 32, 64 (%u waves each); vis_alias_winners (%zu cases); div_rn_unscaled: the bits of num / den on %zu "
           "walk operands and %zu pairs of the stated range\n",
           GROUP_WAVES, n_alias, na, nb);
    return 0;
}
