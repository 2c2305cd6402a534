// merge_plan_check — stand-alone check of cosdata_amd/csrc/merge_plan.h (tests/test_merge_plan.py builds it with the address and
// undefined-behaviour sanitizers): the kernel and width of every key count at and around every boundary, and the refusals.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "merge_plan.h"

using namespace merge_plan;

static int failures = 0;

static void expect(uint32_t S, uint32_t k, uint32_t max_keys, Kind kind, uint32_t width, int32_t status) {
    const Plan p = plan(S, k, max_keys);
    if (p.kind != kind || p.width != width || p.status != status || p.keys != (uint64_t)S * k) {
        printf("FAIL S=%u k=%u max=%u: kind %d width %u status %d keys %llu, expected kind %d width %u status %d\n", S, k, max_keys, (int)p.kind, p.width,
               p.status, (unsigned long long)p.keys, (int)kind, width, status);
        failures++;
    }
}

int main() {
    const uint32_t W = WAVE_MAX_KEYS, L = LDS_MAX_KEYS;
    if (W != 1024 || L != 8192 || LDS_THREADS == 0 || LDS_THREADS % 64 != 0 || (LDS_THREADS & (LDS_THREADS - 1)) != 0) { printf("FAIL constants\n"); return 1; }
    for (uint32_t max_keys : {W, L}) {
        // the wave kernel: R = 1, 2, 4, 8, 16 at 64, 128, 256, 512, 1024 keys
        expect(1, 1, max_keys, Kind::WAVE, 1, OK);
        expect(8, 8, max_keys, Kind::WAVE, 1, OK);
        expect(5, 13, max_keys, Kind::WAVE, 2, OK); // 65
        expect(2, 64, max_keys, Kind::WAVE, 2, OK);
        expect(3, 43, max_keys, Kind::WAVE, 4, OK); // 129
        expect(4, 64, max_keys, Kind::WAVE, 4, OK);
        expect(1, 257, max_keys, Kind::WAVE, 8, OK);
        expect(8, 64, max_keys, Kind::WAVE, 8, OK);
        expect(1, 513, max_keys, Kind::WAVE, 16, OK);
        expect(8, 128, max_keys, Kind::WAVE, 16, OK); // 1024
        expect(1024, 1, max_keys, Kind::WAVE, 16, OK);
        expect(1, 1024, max_keys, Kind::WAVE, 16, OK);
        // nothing to merge
        expect(0, 10, max_keys, Kind::REFUSED, 0, INVALID);
        expect(10, 0, max_keys, Kind::REFUSED, 0, INVALID);
        // products that do not fit 32 bits: 2^32 would wrap to 0, 65537 * 65535 to a small number
        expect(65536, 65536, max_keys, Kind::REFUSED, 0, UNIMPLEMENTED);
        expect(65537, 65535, max_keys, Kind::REFUSED, 0, UNIMPLEMENTED);
        expect(0xFFFFFFFFu, 0xFFFFFFFFu, max_keys, Kind::REFUSED, 0, UNIMPLEMENTED);
        expect(0x80000000u, 2, max_keys, Kind::REFUSED, 0, UNIMPLEMENTED);
        expect(3, 2731, max_keys, Kind::REFUSED, 0, UNIMPLEMENTED); // 8193
        expect(8193, 1, max_keys, Kind::REFUSED, 0, UNIMPLEMENTED);
        expect(1, 8193, max_keys, Kind::REFUSED, 0, UNIMPLEMENTED);
    }
    // 1025: the first count past the wave kernel
    expect(5, 205, W, Kind::REFUSED, 0, UNIMPLEMENTED);
    expect(1, 1025, W, Kind::REFUSED, 0, UNIMPLEMENTED);
    expect(8, 512, W, Kind::REFUSED, 0, UNIMPLEMENTED);
    expect(5, 205, L, Kind::LDS, 2048, OK);
    expect(1, 1025, L, Kind::LDS, 2048, OK);
    expect(1025, 1, L, Kind::LDS, 2048, OK);
    expect(8, 204, L, Kind::LDS, 2048, OK); // 1632: eight shards of the widest flat search
    expect(8, 256, L, Kind::LDS, 2048, OK); // 2048
    expect(1, 2048, L, Kind::LDS, 2048, OK);
    expect(1, 2049, L, Kind::LDS, 4096, OK);
    expect(3, 683, L, Kind::LDS, 4096, OK);  // 2049
    expect(8, 512, L, Kind::LDS, 4096, OK);  // 4096: eight shards of the widest brute force
    expect(4096, 1, L, Kind::LDS, 4096, OK);
    expect(1, 4097, L, Kind::LDS, 8192, OK);
    expect(17, 241, L, Kind::LDS, 8192, OK); // 4097
    expect(16, 512, L, Kind::LDS, 8192, OK); // 8192
    expect(8192, 1, L, Kind::LDS, 8192, OK);
    expect(1, 8192, L, Kind::LDS, 8192, OK);
    // every count up to one past the limit: the width is the smallest that holds the keys, and the LDS image is 8 bytes a key
    for (uint32_t keys = 1; keys <= L + 1; keys++) {
        const Plan p = plan(1, keys, L), t = plan(keys, 1, L);
        if (p.kind != t.kind || p.width != t.width || p.status != t.status) { printf("FAIL S/k symmetry at %u\n", keys); failures++; }
        if (keys > L) { if (p.kind != Kind::REFUSED || p.lds_bytes() != 0) { printf("FAIL %u not refused\n", keys); failures++; } continue; }
        const uint32_t cap = p.kind == Kind::WAVE ? 64 * p.width : p.width;
        const bool smallest = cap >= keys && (p.kind == Kind::WAVE ? (p.width == 1 || cap / 2 < keys) : (p.width == 2048 ? keys > W : cap / 2 < keys));
        if (p.status != OK || (p.kind == Kind::WAVE) != (keys <= W) || !smallest || p.lds_bytes() != (p.kind == Kind::LDS ? p.width * 8 : 0) || p.lds_bytes() > 65536) {
            printf("FAIL keys=%u kind %d width %u\n", keys, (int)p.kind, p.width);
            failures++;
        }
    }
    if (failures) return 1;
    printf("OK\n");
    return 0;
}
