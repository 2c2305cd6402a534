// lat_dots_selftest.cpp — the host models of lat_dots_host.h on their own inputs, on a CPU (tests/test_lat_dots_model.py builds and runs
// it and holds every printed number to the oracle).  Usage: lat_dots_selftest <inputs.bin>
//   stdout, one line per (storage, dim, query, row) of the first SELF_ROWS table rows:
//     D <storage> <dim> <query> <row> <dot> <qmag> <mag> <word cosine> <word dot product> <variant dots ...>      (hex bit patterns)
//   inputs.bin, per (storage, dim): int32 {storage, dim, queries, rows, bytes per row}, the queries, then the rows (reference layout).
// Exit status 1 if the fused f16 chain, which cannot differ (lat_dots_host.h), does.
#include <cstdio>

#include "lat_dots_host.h"

using namespace ldm;

constexpr uint32_t SELF_ROWS = 96; // holds the zero row 3 and every special f16 row

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s <inputs.bin>\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "wb");
    if (!f) return perror(argv[1]), 2;
    int rc = 0;
    for (int st : {ST_F32, ST_F16, ST_BIN, ST_OCT})
        for (uint32_t dim : sweep_dims(st)) {
            const int32_t head[5] = {st, (int32_t)dim, (int32_t)N_QUERIES, (int32_t)SELF_ROWS, (int32_t)ref_bytes(st, dim)};
            fwrite(head, 4, 5, f);
            std::vector<std::vector<uint8_t>> q, rows;
            for (uint32_t i = 0; i < N_QUERIES; i++) { q.push_back(gen_row(st, dim, i, SEED_QUERY)); fwrite(q.back().data(), 1, q.back().size(), f); }
            for (uint32_t i = 0; i < SELF_ROWS; i++) { rows.push_back(gen_row(st, dim, i, SEED_TABLE)); fwrite(rows.back().data(), 1, rows.back().size(), f); }
            for (uint32_t qi = 0; qi < N_QUERIES; qi++) {
                const float qmag = row_mag(st, dim, q[qi].data(), qi == ZERO_QUERY);
                for (uint32_t r = 0; r < SELF_ROWS; r++) {
                    const bool zero = r == ZERO_ROWS[0] || r == ZERO_ROWS[1] || r == ZERO_ROWS[2];
                    const float mag = row_mag(st, dim, rows[r].data(), zero), dot = model_dot(st, dim, q[qi].data(), rows[r].data());
                    printf("D %d %u %u %u %08x %08x %08x %09llx %09llx", st, dim, qi, r, bits_of(dot), bits_of(qmag), bits_of(mag),
                           (unsigned long long)parked_word(0, dot, qmag, mag), (unsigned long long)parked_word(3, dot, qmag, mag));
                    if (st == ST_F32)
                        for (int v = 0; v < F32_VARIANTS; v++) printf(" %08x", bits_of(dot_f32_variant(v, (const float *)q[qi].data(), (const float *)rows[r].data(), dim)));
                    if (st == ST_F16)
                        for (int v = 0; v < F16_VARIANTS; v++) {
                            const float w = dot_f16_variant(v, (const uint16_t *)q[qi].data(), (const uint16_t *)rows[r].data(), dim);
                            printf(" %08x", bits_of(w));
                            if (v == F16_FUSED && !same_f32(bits_of(w), bits_of(dot))) { fprintf(stderr, "f16 dim %u query %u row %u: the fused chain differs\n", dim, qi, r); rc = 1; }
                        }
                    printf("\n");
                }
            }
        }
    fclose(f);
    return rc;
}
