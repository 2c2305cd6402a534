// Stand-alone check of cosdata_amd/csrc/hybrid_plan.h (driven by tests/test_hybrid_plan.py, built with -fsanitize=address,undefined):
// the split of a mixed hybrid request's arm[] into the dense / sparse / BM25 sub-batches, and every refusal that is decided on the
// host.  The expected positions are written here by hand (tables, or the closed form of a cycling batch), never taken from the header.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hybrid_plan.h"

namespace hp = hybrid_plan;

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            failures++;                                                       \
        }                                                                     \
    } while (0)

struct Want {
    uint32_t arm, first, second;
};

// runs split() into a vector of exactly B slots (the sanitizer sees a write past it) and compares with the table
static void expect_split(const std::vector<uint8_t> &arms, const std::vector<Want> &want, uint32_t nd, uint32_t ns, uint32_t nb) {
    const uint32_t B = (uint32_t)arms.size();
    std::vector<hp::Slot> slots(B);
    hp::Split sp;
    uint32_t bad = 0xFFFFFFFFu;
    EXPECT(hp::split(arms.data(), B, slots.data(), sp, &bad) == 0);
    EXPECT(bad == 0xFFFFFFFFu);
    EXPECT(sp.n_dense == nd && sp.n_sparse == ns && sp.n_bm25 == nb);
    EXPECT(want.size() == B);
    for (uint32_t q = 0; q < B && q < want.size(); q++) {
        if (slots[q].arm != want[q].arm || slots[q].pos_first != want[q].first || slots[q].pos_second != want[q].second) {
            std::printf("FAIL query %u of %u: got (%u, %u, %u), want (%u, %u, %u)\n", q, B, slots[q].arm, slots[q].pos_first, slots[q].pos_second,
                        want[q].arm, want[q].first, want[q].second);
            failures++;
        }
    }
}

int main() {
    // ---- all-one-arm batches: both lists of query q are row q of their sub-batches; the third sub-batch is empty ----
    expect_split({0, 0, 0, 0, 0}, {{0, 0, 0}, {0, 1, 1}, {0, 2, 2}, {0, 3, 3}, {0, 4, 4}}, 5, 5, 0);
    expect_split({1, 1, 1, 1, 1}, {{1, 0, 0}, {1, 1, 1}, {1, 2, 2}, {1, 3, 3}, {1, 4, 4}}, 5, 0, 5);
    expect_split({2, 2, 2, 2, 2}, {{2, 0, 0}, {2, 1, 1}, {2, 2, 2}, {2, 3, 3}, {2, 4, 4}}, 0, 5, 5);
    // ---- every arm absent in turn (first list, second list): arm 0 = (dense, sparse), 1 = (dense, BM25), 2 = (sparse, BM25) ----
    // no DENSE_SPARSE: BM25 takes every query, dense and sparse every other one
    expect_split({1, 2, 1, 2}, {{1, 0, 0}, {2, 0, 1}, {1, 1, 2}, {2, 1, 3}}, 2, 2, 4);
    // no DENSE_BM25: sparse takes every query
    expect_split({0, 2, 2, 0}, {{0, 0, 0}, {2, 1, 0}, {2, 2, 1}, {0, 1, 3}}, 2, 4, 2);
    // no SPARSE_BM25: dense takes every query
    expect_split({0, 1, 1, 0, 1}, {{0, 0, 0}, {1, 1, 0}, {1, 2, 1}, {0, 3, 1}, {1, 4, 2}}, 5, 2, 3);
    // ---- B = 1 ----
    expect_split({0}, {{0, 0, 0}}, 1, 1, 0);
    expect_split({1}, {{1, 0, 0}}, 1, 0, 1);
    expect_split({2}, {{2, 0, 0}}, 0, 1, 1);
    // ---- 257 queries, arms cycling 0, 1, 2.  Cycle i (queries 3i, 3i + 1, 3i + 2) finds 2i rows in every sub-batch:
    //   3i     DENSE_SPARSE  dense 2i,     sparse 2i
    //   3i + 1 DENSE_BM25    dense 2i + 1, BM25   2i
    //   3i + 2 SPARSE_BM25   sparse 2i + 1, BM25  2i + 1
    // 257 = 85 cycles + queries 255 (arm 0) and 256 (arm 1): 86 + 86 dense, 86 + 85 sparse, 86 + 85 BM25 ----
    {
        std::vector<uint8_t> arms(257);
        std::vector<Want> want(257);
        for (uint32_t q = 0; q < 257; q++) {
            const uint32_t i = q / 3;
            arms[q] = (uint8_t)(q % 3);
            if (q % 3 == 0) want[q] = {0, 2 * i, 2 * i};
            else if (q % 3 == 1) want[q] = {1, 2 * i + 1, 2 * i};
            else want[q] = {2, 2 * i + 1, 2 * i + 1};
        }
        expect_split(arms, want, 172, 171, 171);
        EXPECT(want[256].arm == 1 && want[256].first == 171 && want[256].second == 170); // the last dense row, the last BM25 row
    }
    // ---- an arm value above 2: INVALID (3), the query named ----
    {
        const uint8_t arms[4] = {0, 1, 3, 2};
        hp::Slot slots[4];
        hp::Split sp;
        uint32_t bad = 99;
        EXPECT(hp::split(arms, 4, slots, sp, &bad) == 3);
        EXPECT(bad == 2);
        const uint8_t arms255[1] = {255};
        EXPECT(hp::split(arms255, 1, slots, sp, nullptr) == 3);
    }
    // ---- the request's own numbers ----
    EXPECT(hp::check_request(88, 88, 1, 1) == 0);
    EXPECT(hp::check_request(96, 88, 256, 170) == 0);             // a longer struct of a later version is accepted; 3 * 170 = 510 <= 512
    EXPECT(hp::check_request(87, 88, 1, 1) == 3);                 // small struct_size
    EXPECT(hp::check_request(0, 88, 1, 1) == 3);
    EXPECT(hp::check_request(88, 88, 0, 10) == 3);                // B == 0
    EXPECT(hp::check_request(88, 88, 4, 0) == 3);                 // top_k == 0
    EXPECT(hp::check_request(88, 88, 4, 171) == 4);               // 3 * 171 = 513 > 512: UNIMPLEMENTED
    EXPECT(hp::check_request(88, 88, 4, 0xFFFFFFFFu) == 4);
    EXPECT(hp::check_request(88, 88, 0, 171) == 3);               // an invalid request is invalid before it is too wide
    // ---- offsets ----
    {
        const uint32_t up[5] = {0, 3, 3, 7, 9}, down[5] = {0, 3, 2, 7, 9}, last[3] = {0, 5, 4};
        EXPECT(hp::offsets_ascend(up, 4));
        EXPECT(!hp::offsets_ascend(down, 4));
        EXPECT(hp::offsets_ascend(down, 1));                      // only the first n + 1 entries are looked at
        EXPECT(!hp::offsets_ascend(last, 2));
        EXPECT(hp::offsets_ascend(up, 0));
    }
    // ---- handles: one is needed exactly when its sub-batch is not empty ----
    {
        hp::Split ds, db, sb, all;
        ds.n_dense = ds.n_sparse = 3;
        db.n_dense = db.n_bm25 = 3;
        sb.n_sparse = sb.n_bm25 = 3;
        all.n_dense = all.n_sparse = all.n_bm25 = 2;
        EXPECT(hp::check_handles(ds, true, true, false) == 0);
        EXPECT(hp::check_handles(db, true, false, true) == 0);
        EXPECT(hp::check_handles(sb, false, true, true) == 0);
        EXPECT(hp::check_handles(ds, true, false, true) == 3);
        EXPECT(hp::check_handles(ds, false, true, true) == 3);
        EXPECT(hp::check_handles(db, true, true, false) == 3);
        EXPECT(hp::check_handles(sb, true, false, true) == 3);
        EXPECT(hp::check_handles(all, true, true, true) == 0);
        EXPECT(hp::check_handles(all, true, true, false) == 3);
    }
    // ---- the sparse half: 3 * top_k * max(reranking_factor, 1) against the handle's setting ----
    {
        const hp::SparseLimits narrow{64, true, 0x80000000u}, wide{1024, true, 0x80000000u}, no_raw{1024, false, 0x80000000u};
        EXPECT(hp::check_sparse(5, 21, 0, narrow) == 0);          // 63
        EXPECT(hp::check_sparse(5, 22, 0, narrow) == 4);          // 66 > 64
        EXPECT(hp::check_sparse(5, 10, 2, narrow) == 0);          // 60
        EXPECT(hp::check_sparse(5, 10, 3, narrow) == 4);          // 90
        EXPECT(hp::check_sparse(5, 170, 0, wide) == 0);           // 510
        EXPECT(hp::check_sparse(5, 170, 2, wide) == 0);           // 1020
        EXPECT(hp::check_sparse(5, 170, 3, wide) == 4);           // 1530 > 1024
        EXPECT(hp::check_sparse(5, 10, 5, wide) == 0);            // 150
        EXPECT(hp::check_sparse(5, 170, 0xFFFFFFFFu, wide) == 4); // no 32-bit wrap
        EXPECT(hp::check_sparse(5, 10, 0, no_raw) == 0);
        EXPECT(hp::check_sparse(5, 10, 2, no_raw) == 6);          // a rerank without raw vectors: NOT_READY
        EXPECT(hp::check_sparse(5, 170, 3, no_raw) == 6);         // ... decided before the width, like the sparse search
        EXPECT(hp::check_sparse(0x80000000u, 10, 0, wide) == 3);  // the sparse search's own batch bound
        EXPECT(hp::check_sparse(0x7FFFFFFFu, 10, 0, wide) == 0);
        EXPECT(hp::check_sparse(0, 170, 3, no_raw) == 0);         // no sparse query: nothing is asked of the handle
    }
    // ---- keys per lane of the fusion: 2 * 3 * top_k ids over 64 lanes ----
    EXPECT(hp::rrf_keys_per_lane(60) == 1);    // top_k 10
    EXPECT(hp::rrf_keys_per_lane(64) == 1);
    EXPECT(hp::rrf_keys_per_lane(66) == 2);    // top_k 11
    EXPECT(hp::rrf_keys_per_lane(180) == 4);   // top_k 30
    EXPECT(hp::rrf_keys_per_lane(512) == 8);
    EXPECT(hp::rrf_keys_per_lane(1020) == 16); // top_k 170
    EXPECT(hp::rrf_keys_per_lane(1024) == 16);
    EXPECT(hp::rrf_keys_per_lane(1026) == 0);
    // ---- the constants the header restates ----
    EXPECT(hp::MAX_TOP_K == 170 && hp::MAX_LIST == 512 && hp::LIST_FACTOR == 3);
    EXPECT(hp::arm_has_dense(0) && hp::arm_has_dense(1) && !hp::arm_has_dense(2));
    EXPECT(hp::arm_has_sparse(0) && !hp::arm_has_sparse(1) && hp::arm_has_sparse(2));
    EXPECT(!hp::arm_has_bm25(0) && hp::arm_has_bm25(1) && hp::arm_has_bm25(2));
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
