// topk_check_selftest.cpp — proves on a CPU that the verifiers of topk_check_host.h can fail: for every primitive and width the
// model's own output passes, every damaged copy of it is rejected, and every generated case keeps the contract of topk_select.h
// (keys unique apart from 0, insert positions < 64 R, lostmask inside cmask), so that no case asks the device for undefined behaviour.
//   g++ -std=c++17 -O1 tests/cxx/topk_check_selftest.cpp -o topk_check_selftest && ./topk_check_selftest
#include "topk_check_host.h"

using namespace tkc;

enum Damage { SWAP_ADJACENT, DUP_NEIGHBOUR, LAST_ZERO, ZERO_AHEAD, EQUAL_SCORE_ORDER, FLIP_LOW, FLIP_HIGH, ULP_UP, ULP_DOWN, N_DAMAGE };
static const char *damage_name[N_DAMAGE] = {"two adjacent keys swapped", "a key replaced by a duplicate of its neighbour", "the last key replaced by 0",
                                            "a zero moved ahead of a nonzero key", "two equal-score keys ordered smaller id first",
                                            "a bit flipped in the low half", "a bit flipped in the high half", "quotient one ulp up", "quotient one ulp down"};
struct Tally {
    std::string what;
    size_t clean = 0, applied[N_DAMAGE] = {}, missed[N_DAMAGE] = {};
};
static int failures = 0;
static void fail(const std::string &msg) {
    failures++;
    fprintf(stderr, "SELFTEST FAIL: %s\n", msg.c_str());
}

// every damage that applies to `good` (an array the verifier accepts); verify(got) returns the mismatch count
template <typename T, typename V>
static void damage_all(const std::vector<T> &good, V verify, Tally &t, const std::string &cname) {
    if (verify(good.data()) != 0) return fail(t.what + " case '" + cname + "': the model's own output is rejected");
    t.clean++;
    const size_t n = good.size();
    const int half = (int)sizeof(T) * 4;
    auto attempt = [&](Damage d, const std::vector<T> &bad) {
        t.applied[d]++;
        if (verify(bad.data()) == 0) {
            t.missed[d]++;
            fail(t.what + " case '" + cname + "': accepted with " + damage_name[d]);
        }
    };
    for (size_t i = 0; i + 1 < n; i++)
        if (good[i] != good[i + 1] && good[i] != 0 && good[i + 1] != 0) {
            std::vector<T> b = good;
            std::swap(b[i], b[i + 1]);
            attempt(SWAP_ADJACENT, b);
            b = good;
            b[i + 1] = b[i];
            attempt(DUP_NEIGHBOUR, b);
            break;
        }
    if (n && good[n - 1] != 0) {
        std::vector<T> b = good;
        b[n - 1] = 0;
        attempt(LAST_ZERO, b);
    }
    for (size_t i = 0; i + 1 < n; i++)
        if (good[i] != 0 && good[i + 1] == 0) {
            std::vector<T> b = good;
            std::swap(b[i], b[i + 1]);
            attempt(ZERO_AHEAD, b);
            break;
        }
    if (sizeof(T) == 8)
        for (size_t i = 0; i + 1 < n; i++)
            if (good[i] != good[i + 1] && good[i] != 0 && good[i + 1] != 0 && ((u64)good[i] >> 32) == ((u64)good[i + 1] >> 32)) {
                std::vector<T> b = good;
                std::swap(b[i], b[i + 1]);
                attempt(EQUAL_SCORE_ORDER, b);
                break;
            }
    if (n) {
        std::vector<T> b = good;
        b[n / 2] ^= (T)1 << 3;
        attempt(FLIP_LOW, b);
        b = good;
        b[n / 3] ^= (T)1 << (half + 5);
        attempt(FLIP_HIGH, b);
    }
}
// the damages in `need` were each tried at least once for this primitive and width
static void require(const Tally &t, std::initializer_list<Damage> need) {
    if (!t.clean) fail(t.what + ": no case");
    for (Damage d : need)
        if (!t.applied[d]) fail(t.what + ": no case to which '" + damage_name[d] + "' applies");
}
static const std::initializer_list<Damage> KEY_DAMAGES = {SWAP_ADJACENT, DUP_NEIGHBOUR, LAST_ZERO, ZERO_AHEAD, EQUAL_SCORE_ORDER, FLIP_LOW, FLIP_HIGH};

static Report quiet() { // the verifiers print what they reject: not here
    Report r;
    r.quiet = true;
    return r;
}

static void seq_selftest(const char *prim, const char *wname, u32 width, const std::vector<SeqCase> &cases, size_t n_in, size_t n_out, int sorted_lists, bool bitonic,
                         size_t &total) {
    Tally t;
    t.what = std::string(prim) + " " + wname + "=" + std::to_string(width);
    for (const SeqCase &c : cases) {
        if (c.in.size() != n_in || c.want.size() != n_out) fail(t.what + " case '" + c.name + "': wrong size");
        if (!keys_unique(c.in)) fail(t.what + " case '" + c.name + "': duplicate key");
        const size_t per = sorted_lists ? n_in / sorted_lists : 0;
        for (int l = 0; l < sorted_lists; l++)
            if (!is_sorted_desc(c.in, l * per, (l + 1) * per)) fail(t.what + " case '" + c.name + "': input list not sorted");
        if (bitonic)
            for (size_t b = 0; b < n_in; b += width)
                if (!is_bitonic(c.in, b, b + width)) fail(t.what + " case '" + c.name + "': input not bitonic");
        damage_all(c.want, [&](const u64 *got) { Report r = quiet(); return verify_seq(prim, wname, width, c, got, r); }, t, c.name);
        total++;
    }
    require(t, KEY_DAMAGES);
    printf("  %-44s %4zu cases\n", t.what.c_str(), cases.size());
}

int main() {
    size_t total = 0;
    for (u32 R : REG_WIDTHS) {
        const u32 P = 64 * R;
        seq_selftest("bitonic_sort_desc", "R", R, sort_cases(P, 1), P, P, 0, false, total);
        std::vector<SeqCase> bc = bitonic_cases(P, R, 2);
        { // (the bitonic check wants the sequence length as width)
            Tally t;
            t.what = "bitonic_merge_desc R=" + std::to_string(R);
            for (const SeqCase &c : bc) {
                if (c.in.size() != P || !keys_unique(c.in) || !is_bitonic(c.in, 0, P)) fail(t.what + " case '" + c.name + "': not P unique keys in bitonic order");
                damage_all(c.want, [&](const u64 *got) { Report r = quiet(); return verify_seq("bitonic_merge_desc", "R", R, c, got, r); }, t, c.name);
                total++;
            }
            require(t, KEY_DAMAGES);
            printf("  %-44s %4zu cases\n", t.what.c_str(), bc.size());
        }
        seq_selftest("merge_sorted_desc", "R", R, merge_sorted_cases(P, 3), 2 * P, P, 2, false, total);
        {
            Tally t, ts;
            t.what = "Pool R=" + std::to_string(R);
            ts.what = t.what + " (results, thr)";
            std::vector<PoolCase> pc = pool_cases(R, 4);
            size_t ops = 0;
            for (const PoolCase &c : pc) {
                std::string why;
                if (!pool_case_contract(c, R, why)) fail(t.what + " case '" + c.name + "': " + why);
                if (c.want_pool.size() != c.ops.size() * P || c.want_scalar.size() != c.ops.size() * 2) fail(t.what + " case '" + c.name + "': wrong size");
                damage_all(c.want_pool, [&](const u64 *got) { Report r = quiet(); return verify_pool(R, c, got, c.want_scalar.data(), r); }, t, c.name);
                damage_all(c.want_scalar, [&](const u64 *got) { Report r = quiet(); return verify_pool(R, c, c.want_pool.data(), got, r); }, ts, c.name);
                ops += c.ops.size();
                total++;
            }
            require(t, KEY_DAMAGES);
            require(ts, {FLIP_LOW, FLIP_HIGH});
            printf("  %-44s %4zu cases, %zu operations\n", t.what.c_str(), pc.size(), ops);
        }
    }
    for (u32 R : STREAM_WIDTHS) {
        const u32 P = 64 * R;
        Tally t, tt;
        t.what = "fold_stream R=" + std::to_string(R);
        tt.what = t.what + " (thr)";
        std::vector<StreamCase> sc = stream_cases(P, 5);
        for (const StreamCase &c : sc) {
            if (!keys_unique(concat(c.s1, c.s2)) || c.want.size() != P) fail(t.what + " case '" + c.name + "': duplicate key or wrong size");
            damage_all(c.want, [&](const u64 *got) { Report r = quiet(); return verify_stream(R, c, got, c.want.back(), r); }, t, c.name);
            damage_all(std::vector<u64>(1, c.want.back()), [&](const u64 *got) { Report r = quiet(); return verify_stream(R, c, c.want.data(), got[0], r); }, tt, c.name);
            total++;
        }
        require(t, KEY_DAMAGES);
        require(tt, {FLIP_LOW, FLIP_HIGH});
        printf("  %-44s %4zu cases\n", t.what.c_str(), sc.size());
    }
    for (u32 N : LDS_SIZES) {
        seq_selftest("lds_bitonic_sort_desc", "N", N, sort_cases(N, 6), N, N, 0, false, total);
        seq_selftest("fold_reversed+lds_bitonic_merge_desc(1)", "N", N, merge_sorted_cases(N, 7), 2 * N, N, 2, false, total);
        seq_selftest("lds_bitonic_merge_desc(2)", "N", N, two_seq_cases(N, 8), 2 * N, 2 * N, 0, true, total);
    }
    for (u32 G : GROUP_SIZES) {
        Tally t;
        t.what = "group_reduce_add_u32 G=" + std::to_string(G);
        const std::vector<u32> in = group_inputs(GROUP_WAVES, 9);
        damage_all(group_model(in, G), [&](const u32 *got) { Report r = quiet(); return verify_group(G, in, got, r); }, t, "random_u32");
        if (G == 64) { // the model itself, once by hand: lanes 0..63 of the first wave
            u32 s = 0;
            for (int l = 0; l < 64; l++) s += in[l];
            if (group_model(in, 64)[63] != s || group_model(in, 1) != in) fail("group model");
        }
        require(t, G > 1 ? std::initializer_list<Damage>{SWAP_ADJACENT, DUP_NEIGHBOUR, FLIP_LOW, FLIP_HIGH} : std::initializer_list<Damage>{SWAP_ADJACENT, FLIP_LOW, FLIP_HIGH});
        total++;
        printf("  %-44s %4u waves\n", t.what.c_str(), GROUP_WAVES);
    }
    {
        Tally t;
        t.what = "vis_alias_winners";
        std::vector<AliasCase> ac = alias_cases(10);
        size_t collide = 0, lower_wins = 0;
        for (const AliasCase &c : ac) {
            if (!alias_case_contract(c)) fail(t.what + " case '" + c.name + "': lostmask is not what the atomics can leave");
            if (c.want & ~c.cmask) fail(t.what + " case '" + c.name + "': the model lets a lane lower_wins cmask win");
            collide += c.lostmask != 0;
            lower_wins += (c.want & c.lostmask) != 0; // a lower slot that lost the atomic wins: the rule under test
            damage_all(std::vector<u64>(1, c.want), [&](const u64 *got) { Report r = quiet(); return verify_alias(c, got[0], r); }, t, c.name);
            total++;
        }
        if (!collide || !lower_wins) fail("vis_alias_winners: no case where a lane that lost the atomic must win");
        require(t, {FLIP_LOW, FLIP_HIGH});
        printf("  %-44s %4zu cases (%zu with a collision, %zu where a lane that lost the atomic wins)\n", t.what.c_str(), ac.size(), collide, lower_wins);
    }
    {
        Tally t;
        t.what = "div_rn_unscaled";
        DivPairs p;
        div_walk_pairs(p, 1u << 16, 11);
        const size_t na = p.size();
        div_range_pairs(p, 1u << 16, 12);
        const std::vector<float> want = div_model(p);
        for (size_t i = 0; i < p.size(); i++) {
            const bool walk = i < na;
            const float hi = walk ? (float)DIV_MAX_SS : 134217728.0f;
            if (!(p.num[i] >= 0.0f && p.num[i] <= hi && p.num[i] == __builtin_truncf(p.num[i]))) fail(fmt("div pair %llu: num out of range", i));
            if (!(p.den[i] >= 1.0f && p.den[i] < 268435456.0f)) fail(fmt("div pair %llu: den out of range", i));
            if (walk && !((double)p.num[i] <= (double)p.den[i] * (1.0 + 1e-6) + 1.0)) fail(fmt("div pair %llu: num above Cauchy-Schwarz", i));
        }
        auto verify = [&](const float *got) { Report r = quiet(); return verify_div("a", p, 0, na, got, want.data(), r) + verify_div("b", p, na, p.size(), got, want.data(), r); };
        if (verify(want.data()) != 0) fail("div: the model's own output is rejected");
        t.clean++;
        size_t tried = 0;
        for (size_t i = 0; i < p.size(); i += 97) { // a quotient off by one ulp, either way, at any pair
            for (int dir = 0; dir < 2; dir++) {
                const u32 b = bits_of_f32(want[i]);
                if (dir == 1 && b == 0) continue;
                std::vector<float> bad = want;
                bad[i] = f32_of_bits(dir == 0 ? b + 1 : b - 1);
                t.applied[dir == 0 ? ULP_UP : ULP_DOWN]++;
                if (verify(bad.data()) != 1) {
                    t.missed[dir == 0 ? ULP_UP : ULP_DOWN]++;
                    fail(fmt("div pair %llu: a quotient one ulp off is accepted", i));
                }
                tried++;
            }
        }
        { // +0 against -0 differ in bits only
            std::vector<float> bad = want;
            size_t z = 0;
            while (z < want.size() && bits_of_f32(want[z]) != 0) z++;
            if (z == want.size()) fail("div: no pair with num 0");
            else {
                bad[z] = f32_of_bits(0x80000000u);
                t.applied[FLIP_HIGH]++;
                if (verify(bad.data()) != 1) fail("div: -0 accepted for +0");
            }
        }
        require(t, {ULP_UP, ULP_DOWN, FLIP_HIGH});
        total++;
        printf("  %-44s %4zu pairs here (2^24 per set on the device), %zu one-ulp damages\n", t.what.c_str(), p.size(), tried);
    }
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("OK topk_check_host.h: %zu cases pass clean, every damaged copy is rejected, every case keeps the contract\n", total);
    return 0;
}
