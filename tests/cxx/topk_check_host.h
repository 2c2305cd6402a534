// topk_check_host.h — the host side of the device checks of cosdata_amd/csrc/topk_select.h and of three wave primitives
// (div_rn_unscaled, group_reduce_add_u32: device_common.h; vis_alias_winners: walk_common.h).  Plain C++, no HIP: the case
// generators (deterministic, every case named), the models the device output is compared with, and the verifiers.
// Used by tests/cxx/topk_select_check.hip and tests/cxx/wave_prims_check.hip (on the GPU) and by tests/cxx/topk_check_selftest.cpp
// (on a CPU: proves that the verifiers reject damaged output and that every case keeps the header's contract).
// Everything compared is an integer or a bit pattern: there is no tolerance anywhere.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

namespace tkc {

typedef uint32_t u32;
typedef unsigned long long u64; // as cosdev::u64

// ---- deterministic randomness: the LCG of wave_reduce_check.hip ---------------------------------------------------------------
struct Rng {
    u64 s;
    explicit Rng(u64 seed) : s(seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull) {}
    u64 next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return s; }
    u32 bits() { return (u32)(next() >> 32); }
    u32 below(u32 n) { return (u32)(((u64)bits() * n) >> 32); } // [0, n)
};
template <typename T>
inline void shuffle(Rng &rng, std::vector<T> &v) {
    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rng.below((u32)i)]);
}
inline std::string fmt(const char *f, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
    char buf[160];
    snprintf(buf, sizeof(buf), f, a, b, c);
    return buf;
}

// ---- keys ------------------------------------------------------------------------------------------------------------------------
// n keys (score << 32 | id), unique and nonzero whatever the scores: the ids are distinct and nonzero (an odd multiplier is a
// bijection of u32, and start + i never wraps to 0), half of them with the top bit set.
enum Flavor { F_RANDOM, F_EQUAL, F_TWO, F_HIGH };
inline const char *flavor_name(Flavor f) { return f == F_RANDOM ? "random" : f == F_EQUAL ? "equal_scores" : f == F_TWO ? "two_scores" : "high_words"; }
inline std::vector<u64> keyset(Rng &rng, size_t n, Flavor f) {
    std::vector<u64> k(n);
    const u32 start = 1u + rng.below(1u << 30);
    static const u32 high[3] = {0xFFFFFFFFu, 0x80000000u, 0u};
    for (size_t i = 0; i < n; i++) {
        const u32 id = (start + (u32)i) * 0x9E3779B1u;
        u32 score = 0;
        switch (f) {
        case F_RANDOM: score = rng.bits(); break;
        case F_EQUAL: score = 0x3F800000u; break;
        case F_TWO: score = (rng.bits() & 1u) ? 0xBF800000u : 0x3F800000u; break; // differ in the top bit
        case F_HIGH: score = high[rng.below(3)]; break;
        }
        k[i] = ((u64)score << 32) | id;
    }
    return k;
}
inline void sort_desc(std::vector<u64> &v) { std::sort(v.begin(), v.end(), std::greater<u64>()); }
inline void sort_asc(std::vector<u64> &v) { std::sort(v.begin(), v.end()); }

// THE model of every sort, merge and fold: the best P of a multiset — the nonzero keys descending as u64, cut to P, padded with 0
inline std::vector<u64> best_of(std::vector<u64> all, size_t P) {
    all.erase(std::remove(all.begin(), all.end(), 0ull), all.end());
    sort_desc(all);
    all.resize(P, 0ull);
    return all;
}
inline std::vector<u64> concat(std::vector<u64> a, const std::vector<u64> &b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
// keys are unique, apart from 0
inline bool keys_unique(std::vector<u64> v) {
    v.erase(std::remove(v.begin(), v.end(), 0ull), v.end());
    std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) == v.end();
}
inline bool is_sorted_desc(const std::vector<u64> &v, size_t b, size_t e) { // [b, e), zeros last
    for (size_t i = b; i + 1 < e; i++)
        if (v[i] < v[i + 1] || (v[i] == v[i + 1] && v[i] != 0)) return false;
    return true;
}
inline bool is_bitonic(const std::vector<u64> &v, size_t b, size_t e) { // up then down, or down then up (non-strict)
    size_t i = b;
    while (i + 1 < e && v[i] <= v[i + 1]) i++;
    while (i + 1 < e && v[i] >= v[i + 1]) i++;
    if (i + 1 >= e) return true;
    i = b;
    while (i + 1 < e && v[i] >= v[i + 1]) i++;
    while (i + 1 < e && v[i] <= v[i + 1]) i++;
    return i + 1 >= e;
}

// ---- cases whose input and output are flat key arrays ------------------------------------------------------------------------------
struct SeqCase {
    std::string name;
    std::vector<u64> in;   // what the wrapper kernel loads
    std::vector<u64> want; // what it must store
};

// any N keys -> sorted (bitonic_sort_desc<N / 64>, lds_bitonic_sort_desc<N>)
inline std::vector<SeqCase> sort_cases(u32 N, u64 seed) {
    Rng rng(seed * 1000 + N);
    std::vector<SeqCase> c;
    auto add = [&](const std::string &name, const std::vector<u64> &in) { c.push_back({name, in, best_of(in, N)}); };
    std::vector<u64> k = keyset(rng, N, F_RANDOM);
    add("random", k);
    sort_desc(k);
    add("already_descending", k);
    sort_asc(k);
    add("already_ascending", k);
    add("equal_scores_distinct_ids", keyset(rng, N, F_EQUAL));
    add("two_scores", keyset(rng, N, F_TWO));
    add("high_words_ffffffff_80000000_0", keyset(rng, N, F_HIGH));
    {
        std::vector<u64> h = keyset(rng, N / 2, F_RANDOM);
        h.resize(N, 0ull);
        shuffle(rng, h);
        add("half_zero_scattered", h);
        std::vector<u64> t = keyset(rng, N / 2, F_TWO);
        t.resize(N, 0ull);
        shuffle(rng, t);
        add("half_zero_scattered_two_scores", t);
    }
    add("all_zero", std::vector<u64>(N, 0ull));
    const u32 at[4] = {0u, 1u, N / 2 + 1, N - 1};
    for (u32 p : at) {
        std::vector<u64> one(N, 0ull);
        one[p] = keyset(rng, 1, F_RANDOM)[0];
        add(fmt("one_nonzero_at_%llu", p), one);
    }
    {
        std::vector<u64> lone(N, 0ull);
        lone[N - 1] = 1ull;
        add("lone_smallest_key_1", lone);
        std::vector<u64> s = keyset(rng, N - 1, F_HIGH); // score 0 keys around it: the low half alone decides
        s.push_back(1ull);
        shuffle(rng, s);
        add("smallest_key_1_among_high_words", s);
    }
    return c;
}

// bitonic inputs (bitonic_merge_desc<R>, lds_bitonic_merge_desc<N>): the turn at every position where the network changes from
// cross-lane to in-lane steps or a sequence ends; zeros at the valley / the tail
inline std::vector<SeqCase> bitonic_cases(u32 N, u32 R, u64 seed) {
    Rng rng(seed * 1000 + N);
    std::vector<SeqCase> c;
    std::vector<u32> turns = {0u, 1u, R - 1, R, R + 1, N / 2, N - 2, N - 1};
    std::sort(turns.begin(), turns.end());
    turns.erase(std::unique(turns.begin(), turns.end()), turns.end());
    auto build = [&](bool up_first, u32 t, u32 zeros, Flavor f) {
        std::vector<u64> k = keyset(rng, N - zeros, f);
        shuffle(rng, k);
        // [0, t) is the first run, [t, N) the second; the zeros go to the second run as far as it holds them
        const u32 zb = std::min(zeros, N - t), za = zeros - zb;
        std::vector<u64> a(k.begin(), k.begin() + (t - za)), b(k.begin() + (t - za), k.end());
        a.resize(t, 0ull);
        b.resize(N - t, 0ull);
        if (up_first) { sort_asc(a); sort_desc(b); } else { sort_desc(a); sort_asc(b); }
        std::vector<u64> in = concat(a, b);
        c.push_back({fmt(up_first ? "ascending_then_descending/turn=%llu/zeros=%llu/" : "descending_then_ascending/turn=%llu/zeros=%llu/", t, zeros) + flavor_name(f), in,
                     best_of(in, N)});
    };
    for (int up = 0; up < 2; up++)
        for (u32 t : turns)
            for (u32 z : {0u, N / 4, N - 1}) build(up != 0, t, z, F_RANDOM);
    for (int up = 0; up < 2; up++)
        for (Flavor f : {F_EQUAL, F_TWO, F_HIGH}) {
            build(up != 0, N / 2, 0, f);
            build(up != 0, R + 1, N / 4, f);
        }
    c.push_back({"all_zero", std::vector<u64>(N, 0ull), std::vector<u64>(N, 0ull)});
    return c;
}

// two sorted lists of P keys, in = pool ++ other -> the best P of both (merge_sorted_desc<R>, fold_reversed<N> + lds_bitonic_merge_desc<N>)
inline std::vector<SeqCase> merge_sorted_cases(u32 P, u64 seed) {
    Rng rng(seed * 1000 + P);
    std::vector<SeqCase> c;
    auto add = [&](const std::string &name, std::vector<u64> a, std::vector<u64> b) {
        sort_desc(a);
        sort_desc(b);
        a.resize(P, 0ull);
        b.resize(P, 0ull);
        std::vector<u64> in = concat(a, b);
        c.push_back({name, in, best_of(in, P)});
    };
    auto split = [&](std::vector<u64> k, size_t na, std::vector<u64> &a, std::vector<u64> &b) {
        shuffle(rng, k);
        a.assign(k.begin(), k.begin() + na);
        b.assign(k.begin() + na, k.end());
    };
    const u32 fills[5] = {0u, 1u, P / 2, P - 1, P};
    for (u32 na : fills)
        for (u32 nb : fills) {
            std::vector<u64> a, b;
            split(keyset(rng, na + nb, F_RANDOM), na, a, b);
            add(fmt("fill=(%llu,%llu)/random", na, nb), a, b);
        }
    for (u32 n : {P, P / 2}) { // every key of `other` better, every key worse, perfectly interleaved
        std::vector<u64> k = keyset(rng, 2 * n, F_RANDOM);
        sort_desc(k);
        std::vector<u64> top(k.begin(), k.begin() + n), bottom(k.begin() + n, k.end()), even, odd;
        for (size_t i = 0; i < k.size(); i++) (i & 1 ? odd : even).push_back(k[i]);
        add(fmt("other_all_better/fill=%llu", n), bottom, top);
        add(fmt("other_all_worse/fill=%llu", n), top, bottom);
        add(fmt("interleaved_pool_first/fill=%llu", n), even, odd);
        add(fmt("interleaved_other_first/fill=%llu", n), odd, even);
    }
    for (Flavor f : {F_EQUAL, F_TWO, F_HIGH})
        for (u32 n : {P, P / 2 + 1}) {
            std::vector<u64> a, b;
            split(keyset(rng, 2 * n, f), n, a, b);
            add(fmt("equal_scores_across_lists/fill=%llu/", n) + flavor_name(f), a, b);
        }
    return c;
}

// two bitonic sequences side by side, as block_merge_pools stages them: lds_bitonic_merge_desc<N>(buf, 2, 2N); in = seq0 ++ seq1
inline std::vector<SeqCase> two_seq_cases(u32 N, u64 seed) {
    std::vector<SeqCase> one = bitonic_cases(N, N / 64, seed), c;
    for (size_t j = 0; j < one.size(); j++) {
        const SeqCase &a = one[j], &b = one[(j + 7) % one.size()];
        c.push_back({a.name + " | " + b.name, concat(a.in, b.in), concat(a.want, b.want)});
    }
    return c;
}

// ---- fold_stream<R> -------------------------------------------------------------------------------------------------------------------
struct StreamCase {
    std::string name;
    std::vector<u64> s1, s2; // the stream; s2 is a second call on the same pool with thr carried over
    bool twice;
    std::vector<u64> want; // the pool; thr must be want[P - 1] (0 while the pool is not full)
};
inline std::vector<StreamCase> stream_cases(u32 P, u64 seed) {
    Rng rng(seed * 1000 + P);
    std::vector<StreamCase> c;
    const u32 counts[10] = {0u, 1u, 63u, 64u, 65u, P - 1, P, P + 1, 2 * P + 63, 5 * P + 17};
    for (u32 n : counts) {
        auto add = [&](const char *order, const std::vector<u64> &s) { c.push_back({fmt("count=%llu/", n) + order, s, {}, false, best_of(s, P)}); };
        std::vector<u64> k = keyset(rng, n, F_RANDOM);
        add("random", k);
        sort_asc(k);
        add("ascending", k); // every key beats the bar: every batch flushes full
        sort_desc(k);
        add("descending", k); // nothing enters after the first P
        add("equal_scores", keyset(rng, n, F_EQUAL));
        std::vector<u64> z = keyset(rng, n - n / 3, F_RANDOM);
        z.resize(n, 0ull);
        shuffle(rng, z);
        add("zeros_scattered", z);
    }
    auto twice = [&](const std::string &name, const std::vector<u64> &s1, const std::vector<u64> &s2) {
        c.push_back({name, s1, s2, true, best_of(concat(s1, s2), P)});
    };
    {
        std::vector<u64> k = keyset(rng, 3 * P + 42, F_RANDOM), s1, s2;
        shuffle(rng, k);
        s1.assign(k.begin(), k.begin() + P + 37); // fills the pool: the bar is carried
        s2.assign(k.begin() + P + 37, k.end());   // random scores: above and below it
        twice("twice/seed_fills_pool/second_above_and_below_bar", s1, s2);
        s1.assign(k.begin(), k.begin() + P / 2); // pool not full: thr 0 carried
        s2.assign(k.begin() + P / 2, k.end());
        twice("twice/seed_half_fills_pool", s1, s2);
        sort_desc(k);
        s1.assign(k.begin(), k.begin() + P); // the best P already in: nothing of the second stream may enter
        s2.assign(k.begin() + P, k.end());
        shuffle(rng, s2);
        twice("twice/second_all_below_bar", s1, s2);
        s1.assign(k.end() - P, k.end()); // the worst P in: the second stream replaces all of them
        s2.assign(k.begin(), k.end() - P);
        sort_asc(s2);
        twice("twice/second_all_above_bar_ascending", s1, s2);
        std::vector<u64> e = keyset(rng, 2 * P + 64, F_EQUAL);
        s1.assign(e.begin(), e.begin() + P);
        s2.assign(e.begin() + P, e.end());
        twice("twice/equal_scores_ends_at_batch_boundary", s1, s2);
    }
    return c;
}

// ---- Pool<R>: scripts of operations replayed by one wave ----------------------------------------------------------------------------------
enum PoolOpKind : u32 { OP_INSERT_AT, OP_POP_HEAD, OP_RANK_OF, OP_HEAD, OP_PEEK_DYN, OP_PEEK, OP_PEEK_NODE, OP_FOLD_LANES, OP_FOLD_MASK };
inline const char *op_name(u32 op) {
    static const char *n[] = {"insert_at", "pop_head", "rank_of", "head", "peek_dyn", "peek<I>", "peek_node<I>", "pool_fold_lanes", "pool_fold_mask"};
    return op < 9 ? n[op] : "?";
}
struct PoolOp {
    u32 op;
    u32 arg; // insert_at: position; peek_dyn: position; peek / peek_node: which of I = {0, R - 1, R, P - 1}; folds: the wave of 64 keys
    u64 key; // insert_at, rank_of: the key; pool_fold_mask: the lane mask
};
inline u32 peek_index(u32 which, u32 R) { return which == 0 ? 0u : which == 1 ? R - 1 : which == 2 ? R : 64u * R - 1; }

// the model: a sorted array of P keys
struct PoolModel {
    std::vector<u64> e;
    u64 thr = 0; // what the fold operations carry
    explicit PoolModel(u32 P) : e(P, 0ull) {}
    void insert_at(u64 k, u32 p) { // positions >= p shift up by one, the last drops
        for (size_t i = e.size() - 1; i > p; i--) e[i] = e[i - 1];
        e[p] = k;
    }
    void pop_head() {
        for (size_t i = 0; i + 1 < e.size(); i++) e[i] = e[i + 1];
        e.back() = 0ull;
    }
    u32 rank_of(u64 k) const { // the number of entries > k
        u32 n = 0;
        for (u64 x : e) n += x > k;
        return n;
    }
    u64 head() const { return e[0]; }
    u64 peek(u32 pos) const { return e[pos]; }
    u64 vote(const u64 *keys) const { // the lanes whose key beats thr
        u64 m = 0;
        for (int l = 0; l < 64; l++) m |= (u64)(keys[l] > thr) << l;
        return m;
    }
    void fold_mask(const u64 *keys, u64 m) { // lowest lane first; a key that an earlier insert pushed below the bar is dropped
        for (int l = 0; l < 64; l++)
            if (((m >> l) & 1) && keys[l] > thr) {
                insert_at(keys[l], rank_of(keys[l]));
                thr = e.back();
            }
    }
    // one operation; returns its scalar result (0 where it has none)
    u64 apply(const PoolOp &o, const std::vector<u64> &waves, u32 R) {
        switch (o.op) {
        case OP_INSERT_AT: insert_at(o.key, o.arg); return 0;
        case OP_POP_HEAD: pop_head(); return 0;
        case OP_RANK_OF: return rank_of(o.key);
        case OP_HEAD: return head();
        case OP_PEEK_DYN: return peek(o.arg);
        case OP_PEEK: return peek(peek_index(o.arg, R));
        case OP_PEEK_NODE: return (u32)peek(peek_index(o.arg, R));
        case OP_FOLD_LANES: fold_mask(&waves[(size_t)o.arg * 64], vote(&waves[(size_t)o.arg * 64])); return 0;
        case OP_FOLD_MASK: fold_mask(&waves[(size_t)o.arg * 64], o.key); return 0;
        }
        return 0;
    }
};
struct PoolCase {
    std::string name;
    std::vector<PoolOp> ops;
    std::vector<u64> waves;       // [slots][64]: the keys of the fold operations
    std::vector<u64> want_pool;   // [ops][P]: the whole pool after every operation
    std::vector<u64> want_scalar; // [ops][2]: the operation's result, thr
};
struct PoolScript { // builds a case and its expected output side by side
    PoolCase c;
    PoolModel m;
    u32 R, P;
    PoolScript(const std::string &name, u32 R_) : m(64 * R_), R(R_), P(64 * R_) { c.name = name; }
    u64 op(u32 kind, u32 arg = 0, u64 key = 0) {
        const PoolOp o{kind, arg, key};
        c.ops.push_back(o);
        const u64 res = m.apply(o, c.waves, R);
        c.want_pool.insert(c.want_pool.end(), m.e.begin(), m.e.end());
        c.want_scalar.push_back(res);
        c.want_scalar.push_back(m.thr);
        return res;
    }
    u32 wave(const std::vector<u64> &keys64) {
        c.waves.insert(c.waves.end(), keys64.begin(), keys64.end());
        return (u32)(c.waves.size() / 64 - 1);
    }
    void fold_lanes(std::vector<u64> keys) { // any number of keys, 64 per operation
        keys.resize((keys.size() + 63) / 64 * 64, 0ull);
        for (size_t i = 0; i < keys.size(); i += 64) op(OP_FOLD_LANES, wave(std::vector<u64>(keys.begin() + i, keys.begin() + i + 64)));
    }
};
// keys with scores lo + step * i: room between any two of them and on both sides
inline std::vector<u64> spaced_keys(Rng &rng, u32 n, u32 lo, u32 step) {
    std::vector<u64> k = keyset(rng, n, F_EQUAL);
    for (u32 i = 0; i < n; i++) k[i] = ((u64)(lo + step * i) << 32) | (u32)k[i];
    return k;
}
inline std::vector<PoolCase> pool_cases(u32 R, u64 seed) {
    const u32 P = 64 * R;
    Rng rng(seed * 1000 + R);
    std::vector<PoolCase> out;
    // one pot of unique keys per width: a case draws what it inserts
    std::vector<u64> pot = keyset(rng, 64 * P + 4096, F_RANDOM);
    size_t pot_at = 0;
    auto draw = [&](size_t n) {
        std::vector<u64> k(pot.begin() + pot_at, pot.begin() + pot_at + n);
        pot_at += n;
        return k;
    };
    std::vector<u32> poss = {0u, 1u, R - 1, R, R + 1, P / 2, P - R, P - 2, P - 1};
    std::sort(poss.begin(), poss.end());
    poss.erase(std::unique(poss.begin(), poss.end()), poss.end());

    // insert_at: every position, into an empty, a half-full and a full pool (mechanical: the pool need not stay sorted)
    for (u32 fill : {0u, P / 2, P})
        for (u32 p : poss) {
            PoolScript s(fmt("insert_at/fill=%llu/pos=%llu", fill, p), R);
            s.fold_lanes(draw(fill));
            const std::vector<u64> k = draw(3);
            s.op(OP_INSERT_AT, p, k[0]);
            s.op(OP_HEAD);
            s.op(OP_PEEK_DYN, p);
            s.op(OP_INSERT_AT, p, k[1]);
            s.op(OP_INSERT_AT, (p + 1) % P, k[2]);
            s.op(OP_PEEK_DYN, P - 1);
            out.push_back(std::move(s.c));
        }
    // rank_of: above all, below all, between two equal-score entries, an entry itself
    for (Flavor f : {F_EQUAL, F_TWO, F_HIGH})
        for (u32 fill : {P, P / 2}) {
            PoolScript s(fmt("rank_of/fill=%llu/", fill) + flavor_name(f), R);
            std::vector<u64> k = keyset(rng, fill, f);
            s.fold_lanes(k);
            s.op(OP_RANK_OF, 0, ~0ull);
            s.op(OP_RANK_OF, 0, 0ull);
            s.op(OP_RANK_OF, 0, s.m.e[0] + 1);
            s.op(OP_RANK_OF, 0, s.m.e[fill - 1] - 1);
            for (u32 j : {0u, R - 1, R, fill / 2, fill - 2}) {
                if (j + 1 >= fill) continue;
                s.op(OP_RANK_OF, 0, s.m.e[j + 1] + 1); // between entries j and j + 1 (the ids are far apart)
                s.op(OP_RANK_OF, 0, s.m.e[j]);
            }
            out.push_back(std::move(s.c));
        }
    // the walk's pattern: pop the head, then insert only at pos < limit; down to nothing, then refilled
    for (Flavor f : {F_RANDOM, F_TWO}) {
        PoolScript s(std::string("walk_pop_insert/") + flavor_name(f), R);
        std::vector<u64> k = f == F_RANDOM ? draw(3 * P + 80) : keyset(rng, 3 * P + 80, f);
        size_t at = P;
        s.fold_lanes(std::vector<u64>(k.begin(), k.begin() + P));
        u32 popped = 0;
        while (s.m.head() != 0ull) {
            s.op(OP_HEAD);
            s.op(OP_POP_HEAD);
            popped++;
            const u32 limit = popped < P ? P - popped : 0u; // the walk's ef - popped
            for (int t = 0; t < 2 && popped < P / 4; t++) {
                const u64 key = k[at++];
                const u32 p = (u32)s.op(OP_RANK_OF, 0, key);
                if (p < limit) s.op(OP_INSERT_AT, p, key);
            }
        }
        s.op(OP_HEAD); // empty: 0
        for (int t = 0; t < 70; t++) { // refilled, past one lane's share of every width
            const u64 key = k[at++];
            s.op(OP_INSERT_AT, (u32)s.op(OP_RANK_OF, 0, key), key);
        }
        for (int t = 0; t < 5; t++) {
            s.op(OP_HEAD);
            s.op(OP_POP_HEAD);
        }
        s.op(OP_PEEK_DYN, std::min(64u, P - 1));
        out.push_back(std::move(s.c));
    }
    // peek_dyn: every position of a full pool; the positions of poss in a half-full one
    {
        PoolScript s("peek_dyn/full/every_position", R);
        s.fold_lanes(draw(P));
        for (u32 p = 0; p < P; p++) s.op(OP_PEEK_DYN, p);
        out.push_back(std::move(s.c));
        PoolScript h("peek_dyn/half_full", R);
        h.fold_lanes(draw(P / 2));
        for (u32 p : poss) h.op(OP_PEEK_DYN, p);
        out.push_back(std::move(h.c));
    }
    // peek<I>, peek_node<I>: I = 0, R - 1, R, P - 1
    for (Flavor f : {F_RANDOM, F_HIGH}) {
        PoolScript s(std::string("peek_static/") + flavor_name(f), R);
        s.fold_lanes(f == F_RANDOM ? draw(P) : keyset(rng, P, f));
        for (u32 w = 0; w < 4; w++) s.op(OP_PEEK, w);
        for (u32 w = 0; w < 4; w++) s.op(OP_PEEK_NODE, w);
        out.push_back(std::move(s.c));
    }
    // pool_fold_lanes / pool_fold_mask over a full pool of scores 1000, 1010, ...: waves in which 0, 1 or all 64 lanes beat thr, one
    // whose early lanes push thr above its later lanes' keys, random ones.  `subset`: pool_fold_mask with every second qualifying
    // lane — the unnamed lanes must stay out; otherwise the full vote.
    for (int mode = 0; mode < 3; mode++) { // 0: pool_fold_lanes, 1: pool_fold_mask(full vote), 2: pool_fold_mask(every second lane)
        for (u32 fill : {P, P / 2, 0u}) {
            PoolScript s(fmt(mode == 0 ? "pool_fold_lanes/fill=%llu" : mode == 1 ? "pool_fold_mask/full_vote/fill=%llu" : "pool_fold_mask/every_second_lane/fill=%llu", fill), R);
            s.fold_lanes(spaced_keys(rng, fill, 1000u, 10u));
            u32 uniq = 0; // distinct ids for the keys made here: scores off the pool's grid
            auto key = [&](u32 score) { return ((u64)score << 32) | (0x40000000u + 977u * uniq++); };
            auto fold = [&](const std::vector<u64> &w) {
                const u32 slot = s.wave(w);
                if (mode == 0) { s.op(OP_FOLD_LANES, slot); return; }
                u64 m = s.m.vote(&w[0]);
                if (mode == 2) {
                    u64 sub = 0;
                    bool take = true;
                    for (int l = 0; l < 64; l++)
                        if ((m >> l) & 1) { if (take) sub |= 1ull << l; take = !take; }
                    m = sub;
                }
                s.op(OP_FOLD_MASK, slot, m);
            };
            std::vector<u64> w(64);
            for (int l = 0; l < 64; l++) w[l] = (l % 3 == 0) ? 0ull : key(1u + (u32)l); // none beats a full pool's bar (all enter another)
            fold(w);
            for (int l = 0; l < 64; l++) w[l] = l == 17 ? key(1000u + 10u * (P / 2) + 5u) : (l & 1 ? 0ull : key(500u + (u32)l)); // lane 17 alone
            fold(w);
            // lanes 0..31 far above the pool: after them thr is the old entry 32 from the end; lanes 32..63 sit just above the OLD bar (1010)
            // and must be dropped — but lane 40, above the new bar, must enter
            for (int l = 0; l < 64; l++) w[l] = l < 32 ? key(100000u + 7u * (u32)((l * 37) % 32)) : key(1013u + (u32)(l & 3));
            w[40] = key(1000u + 10u * 40u + 5u);
            fold(w);
            for (int l = 0; l < 64; l++) w[l] = key(200000u + (u32)((l * 29) % 64)); // all 64 beat thr, out of order
            fold(w);
            for (int t = 0; t < 4; t++) { // random: scores around the pool's
                for (int l = 0; l < 64; l++) w[l] = rng.below(5) == 0 ? 0ull : key(900u + rng.below(12u * P + 400u));
                fold(w);
            }
            s.op(OP_HEAD);
            out.push_back(std::move(s.c));
        }
    }
    return out;
}
// the contract of a pool case: inserted keys unique and nonzero, positions < 64 R, a fold mask inside the vote, folds only into a sorted pool
inline bool pool_case_contract(const PoolCase &c, u32 R, std::string &why) {
    const u32 P = 64 * R;
    std::vector<u64> all;
    PoolModel m(P);
    for (const PoolOp &o : c.ops) {
        if (o.op == OP_INSERT_AT) {
            if (o.arg >= P) return why = "insert position >= 64 R", false;
            if (o.key == 0) return why = "inserts the empty key", false;
            all.push_back(o.key);
        }
        if ((o.op == OP_PEEK_DYN && o.arg >= P) || ((o.op == OP_PEEK || o.op == OP_PEEK_NODE) && o.arg >= 4)) return why = "peek position out of range", false;
        if (o.op == OP_FOLD_LANES || o.op == OP_FOLD_MASK) {
            if ((size_t)(o.arg + 1) * 64 > c.waves.size()) return why = "wave slot out of range", false;
            if (!is_sorted_desc(m.e, 0, P)) return why = "fold into an unsorted pool", false;
            if (m.thr != m.e.back()) return why = "thr is not the pool's last key", false;
            if (o.op == OP_FOLD_MASK && (o.key & ~m.vote(&c.waves[(size_t)o.arg * 64]))) return why = "mask names a lane that does not beat thr", false;
        }
        m.apply(o, c.waves, R);
    }
    all.insert(all.end(), c.waves.begin(), c.waves.end());
    if (!keys_unique(all)) return why = "duplicate key", false;
    return true;
}

// ---- group_reduce_add_u32(v, G): wrapping u32 sums over aligned groups of G lanes; every lane holds its group's sum -------------
inline std::vector<u32> group_inputs(u32 waves, u64 seed) {
    Rng rng(seed);
    std::vector<u32> v((size_t)waves * 64);
    for (u32 &x : v) x = rng.bits(); // the sums wrap
    return v;
}
inline std::vector<u32> group_model(const std::vector<u32> &in, u32 G) {
    std::vector<u32> out(in.size());
    for (size_t g = 0; g < in.size(); g += G) {
        u32 s = 0;
        for (u32 l = 0; l < G; l++) s += in[g + l];
        for (u32 l = 0; l < G; l++) out[g + l] = s;
    }
    return out;
}

// ---- vis_alias_winners(cmask, bit, lostmask) ----------------------------------------------------------------------------------------------
struct AliasCase {
    std::string name;
    u32 bit[64];
    u64 cmask, lostmask;
    u64 want;
};
// of the lanes in cmask that share a residue, the lowest one
inline u64 alias_model(const AliasCase &c) {
    u64 w = 0;
    for (int l = 0; l < 64; l++) {
        if (!((c.cmask >> l) & 1)) continue;
        bool lowest = true;
        for (int j = 0; j < l; j++) lowest &= !(((c.cmask >> j) & 1) && c.bit[j] == c.bit[l]);
        if (lowest) w |= 1ull << l;
    }
    return w;
}
// lostmask as the atomics leave it: of every residue group inside cmask one lane found the bit clear — pick(group) chooses which
inline std::vector<AliasCase> alias_cases(u64 seed) {
    Rng rng(seed);
    std::vector<AliasCase> c;
    enum Pick { LOWEST, HIGHEST, RANDOM };
    auto add = [&](const std::string &name, const u32 *bit, u64 cmask, Pick pick) {
        AliasCase a;
        a.name = name;
        memcpy(a.bit, bit, sizeof(a.bit));
        a.cmask = cmask;
        a.lostmask = 0;
        u64 seen = 0;
        for (int l = 0; l < 64; l++) {
            if (!((cmask >> l) & 1) || ((seen >> l) & 1)) continue;
            std::vector<int> grp;
            for (int j = l; j < 64; j++)
                if (((cmask >> j) & 1) && bit[j] == bit[l]) grp.push_back(j);
            const int win = pick == LOWEST ? grp.front() : pick == HIGHEST ? grp.back() : grp[rng.below((u32)grp.size())];
            for (int j : grp) {
                seen |= 1ull << j;
                if (j != win) a.lostmask |= 1ull << j;
            }
        }
        a.want = alias_model(a);
        c.push_back(a);
    };
    u32 bit[64];
    for (int l = 0; l < 64; l++) bit[l] = 1000u + 3u * (u32)l;
    add("no_collision", bit, ~0ull, RANDOM);
    add("no_collision/cmask_sparse", bit, 0x8000000000010401ull, RANDOM);
    add("cmask_empty", bit, 0ull, RANDOM);
    for (int l = 0; l < 64; l++) bit[l] = 77u;
    for (Pick p : {LOWEST, HIGHEST, RANDOM}) add(fmt("all_64_on_one_residue/atomic_winner=%llu", p), bit, ~0ull, p);
    add("all_on_one_residue/cmask_empty", bit, 0ull, RANDOM);
    add("all_on_one_residue/cmask_one_lane", bit, 1ull << 63, RANDOM);
    for (int l = 0; l < 64; l++) bit[l] = (u32)(l / 2);
    for (Pick p : {LOWEST, HIGHEST}) add(fmt("pairs_adjacent/atomic_winner=%llu", p), bit, ~0ull, p);
    for (int l = 0; l < 64; l++) bit[l] = (u32)(l % 32);
    for (Pick p : {LOWEST, HIGHEST}) add(fmt("pairs_32_apart/atomic_winner=%llu", p), bit, ~0ull, p);
    for (int l = 0; l < 64; l++) bit[l] = (u32)(l % 5) + 0xFFFFFFF0u;
    add("atomic_winner_is_highest_of_its_group/5_residues", bit, ~0ull, HIGHEST);
    // lanes 0..7 share residue 9 but are outside cmask: lower than every lane of the group, they must not win
    for (int l = 0; l < 64; l++) bit[l] = l < 8 || l % 4 == 0 ? 9u : 100u + (u32)l;
    for (Pick p : {LOWEST, HIGHEST, RANDOM}) add(fmt("lane_outside_cmask_shares_residue/atomic_winner=%llu", p), bit, ~0xFFull, p);
    for (int t = 0; t < 240; t++) {
        const u32 residues = 1u + rng.below(t % 3 == 0 ? 4u : 64u);
        for (int l = 0; l < 64; l++) bit[l] = rng.below(residues) * 0x01000193u;
        const u64 cm = t % 4 == 0 ? rng.next() & rng.next() : t % 4 == 1 ? rng.next() | rng.next() : rng.next();
        add(fmt("random_%llu/residues=%llu", (u64)t, residues), bit, cm, RANDOM);
    }
    return c;
}
inline bool alias_case_contract(const AliasCase &a) { // lostmask inside cmask, and exactly one lane of every group found its bit clear
    if (a.lostmask & ~a.cmask) return false;
    for (int l = 0; l < 64; l++) {
        if (!((a.cmask >> l) & 1)) continue;
        int clear = 0;
        for (int j = 0; j < 64; j++) clear += ((a.cmask >> j) & 1) && a.bit[j] == a.bit[l] && !((a.lostmask >> j) & 1);
        if (clear != 1) return false;
    }
    return true;
}

// ---- div_rn_unscaled(num, den) against the host's float quotient (round to nearest) ---------------------------------------------------
struct DivPairs {
    std::vector<float> num, den;
    void add(float n, float d) { num.push_back(n); den.push_back(d); }
    size_t size() const { return num.size(); }
};
inline float f32_of_bits(u32 b) { float f; memcpy(&f, &b, 4); return f; }
inline u32 bits_of_f32(float f) { u32 b; memcpy(&b, &f, 4); return b; }
inline u64 isqrt_ceil(u64 x) { // the least s with s * s >= x
    u64 s = (u64)__builtin_sqrt((double)x);
    while (s * s < x) s++;
    while (s > 0 && (s - 1) * (s - 1) >= x) s--;
    return s;
}
inline u64 log_uniform(Rng &rng, u64 lo, u64 hi) { // [lo, hi], every binade about equally often
    if (hi <= lo) return lo;
    const u64 span = hi - lo;
    const int top = 64 - __builtin_clzll(span);
    const int b = 1 + (int)rng.below((u32)top);
    const u64 v = rng.next() >> (64 - b);
    return lo + (v > span ? v % (span + 1) : v);
}
constexpr u32 DIV_MAX_DIM = 4096;
constexpr u64 DIV_MAX_SS = 255ull * 255ull * DIV_MAX_DIM; // 266342400 < 2^28
// (a) what the walk can form: den = fl(|q| * |v|) with the norms sqrtf(sum of squares as f32) of u8 rows of 1..4096 dimensions
// (kernels_walk.hip: `(sum::<u32>() as f32).sqrt()`; identical to fl(sqrt(a)) while a < 2^24), num an integer dot `as f32` inside
// Cauchy-Schwarz, 0 <= num <= ceil(sqrt(a b)).
inline void div_walk_pairs(DivPairs &out, size_t n, u64 seed) {
    Rng rng(seed);
    auto den_of = [](u64 a, u64 b) { return __builtin_sqrtf((float)a) * __builtin_sqrtf((float)b); };
    auto nums = [&](u64 a, u64 b, u64 which) -> u64 {
        const u64 top = isqrt_ceil(a * b);
        switch (which) {
        case 0: return 0;
        case 1: return 1;
        case 2: return top;
        case 3: return top - 1;
        case 4: return top > (1ull << 24) ? log_uniform(rng, (1ull << 24) + 1, top) : top / 2;
        case 5: return log_uniform(rng, 0, top);
        default: return rng.next() % (top + 1);
        }
    };
    const u64 corners[] = {1, 2, 3, 4, 255ull * 255, 255ull * 255 + 1, (1ull << 24) - 1, 1ull << 24, (1ull << 24) + 1, (1ull << 27) - 1, 1ull << 27, DIV_MAX_SS - 1, DIV_MAX_SS};
    for (u64 a : corners)
        for (u64 b : corners)
            for (u64 w = 0; w < 6; w++) out.add((float)nums(a, b, w), den_of(a, b));
    u64 t = 0;
    while (out.size() < n) {
        const u64 dim = log_uniform(rng, 1, DIV_MAX_DIM), hi = 255ull * 255ull * dim;
        const u64 a = t % 5 == 0 ? hi - rng.below(3) : log_uniform(rng, 1, hi), b = t % 7 == 0 ? a : log_uniform(rng, 1, hi);
        out.add((float)nums(a, b, 2 + t % 5), den_of(a, b));
        t++;
    }
}
// (b) the range device_common.h states: num an integer in [0, 2^27), den a float in [1, 2^28), independent, log-uniform + corners
inline void div_range_pairs(DivPairs &out, size_t n, u64 seed) {
    Rng rng(seed);
    const size_t end = out.size() + n;
    const u64 nc[] = {0, 1, 2, 3, (1ull << 23) + 1, (1ull << 24) - 1, 1ull << 24, (1ull << 24) + 1, (1ull << 24) + 3, (1ull << 26) + 4, (1ull << 27) - 9, (1ull << 27) - 1};
    const u32 dc[] = {0x3F800000u, 0x3F800001u, 0x3FFFFFFFu, 0x40000000u, 0x40400000u, 0x4B7FFFFFu, 0x4B800000u, 0x4D7FFFFFu, 0x4D800000u - 1u, 0x4D000001u};
    for (u64 nn : nc)
        for (u32 d : dc) out.add((float)nn, f32_of_bits(d));
    while (out.size() < end) {
        const u32 d = ((127u + rng.below(28)) << 23) | (rng.bits() >> 9); // [1, 2^28): every exponent, any mantissa
        out.add((float)log_uniform(rng, 0, (1ull << 27) - 1), f32_of_bits(d));
    }
}
inline std::vector<float> div_model(const DivPairs &p) {
    std::vector<float> q(p.size());
    for (size_t i = 0; i < p.size(); i++) q[i] = p.num[i] / p.den[i];
    return q;
}

// ---- the verifiers: (what was asked, device output, model output) -> mismatch count; up to 8 mismatches printed ----------------------------
struct Report {
    int printed = 0;
    bool quiet = false; // count only
    void line(const char *prim, const char *wname, u32 width, const std::string &cname, size_t pos, u64 got, u64 want) {
        if (!quiet && printed++ < 8) fprintf(stderr, "MISMATCH %s %s=%u case '%s' position %zu: got 0x%016llx want 0x%016llx\n", prim, wname, width, cname.c_str(), pos, got, want);
    }
};
template <typename T>
inline size_t verify_array(const char *prim, const char *wname, u32 width, const std::string &cname, const T *got, const T *want, size_t n, Report &rep) {
    size_t bad = 0;
    for (size_t i = 0; i < n; i++)
        if (got[i] != want[i]) {
            bad++;
            rep.line(prim, wname, width, cname, i, (u64)got[i], (u64)want[i]);
        }
    return bad;
}
inline size_t verify_seq(const char *prim, const char *wname, u32 width, const SeqCase &c, const u64 *got, Report &rep) {
    return verify_array(prim, wname, width, c.name, got, c.want.data(), c.want.size(), rep);
}
inline size_t verify_stream(u32 R, const StreamCase &c, const u64 *got_pool, u64 got_thr, Report &rep) {
    size_t bad = verify_array("fold_stream", "R", R, c.name, got_pool, c.want.data(), c.want.size(), rep);
    if (got_thr != c.want.back()) {
        bad++;
        rep.line("fold_stream", "R", R, c.name + " [thr]", c.want.size(), got_thr, c.want.back());
    }
    return bad;
}
inline size_t verify_pool(u32 R, const PoolCase &c, const u64 *got_pool, const u64 *got_scalar, Report &rep) {
    const size_t P = 64 * (size_t)R;
    size_t bad = 0;
    for (size_t o = 0; o < c.ops.size(); o++) {
        const std::string at = c.name + fmt(" op %llu ", o) + op_name(c.ops[o].op);
        bad += verify_array("Pool", "R", R, at, got_pool + o * P, c.want_pool.data() + o * P, P, rep);
        bad += verify_array("Pool", "R", R, at + " [result, thr]", got_scalar + o * 2, c.want_scalar.data() + o * 2, 2, rep);
    }
    return bad;
}
inline size_t verify_group(u32 G, const std::vector<u32> &in, const u32 *got, Report &rep) {
    const std::vector<u32> want = group_model(in, G);
    return verify_array("group_reduce_add_u32", "G", G, "random_u32", got, want.data(), want.size(), rep);
}
inline size_t verify_alias(const AliasCase &c, u64 got, Report &rep) { return verify_array("vis_alias_winners", "lanes", 64u, c.name, &got, &c.want, 1, rep); }
inline size_t verify_div(const char *set, const DivPairs &p, size_t begin, size_t end, const float *got, const float *want, Report &rep) {
    size_t bad = 0;
    for (size_t i = begin; i < end; i++)
        if (bits_of_f32(got[i]) != bits_of_f32(want[i])) {
            bad++;
            if (!rep.quiet && rep.printed++ < 8)
                fprintf(stderr, "MISMATCH div_rn_unscaled set %s pair %zu: num %.9g (0x%08x) den %.9g (0x%08x): got 0x%08x want 0x%08x\n", set, i, (double)p.num[i],
                        bits_of_f32(p.num[i]), (double)p.den[i], bits_of_f32(p.den[i]), bits_of_f32(got[i]), bits_of_f32(want[i]));
        }
    return bad;
}

// the widths the kernels instantiate
constexpr u32 REG_WIDTHS[5] = {1, 2, 4, 8, 16};           // bitonic_sort_desc, bitonic_merge_desc, merge_sorted_desc, Pool
constexpr u32 STREAM_WIDTHS[4] = {2, 4, 8, 16};           // fold_stream
constexpr u32 LDS_SIZES[4] = {128, 256, 512, 1024};       // lds_bitonic_sort_desc, lds_bitonic_merge_desc, fold_reversed
constexpr u32 LDS_THREADS[2] = {256, 192};                // what kernels_sparse.hip launches with; one that does not divide N / 2
constexpr u32 GROUP_SIZES[7] = {1, 2, 4, 8, 16, 32, 64};  // group_reduce_add_u32
constexpr u32 GROUP_WAVES = 257;

} // namespace tkc
