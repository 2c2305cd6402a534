// gen_walk_plan_cases.cpp — writes tests/golden/walk_plan_cases.txt: the launch decisions of a dense search for a grid of inputs, AS THE
// COMMIT BEFORE walk_plan.h MADE THEM (157c5dc).  It only builds against that commit: it calls that build's own
// cosdev::walk_general_needed and cosdev::walk_kernel_kind, and applies the conditions that lived inside the static get_workspace /
// run_search of its engine.hip, copied verbatim with their line numbers.  Host code only, no GPU.  At that commit:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I cosdata_amd/csrc -I include gen_walk_plan_cases.cpp -L cosdata_amd -lcosdata_hip \
//         -Wl,-rpath,$PWD/cosdata_amd -o gen_walk_plan_cases && ./gen_walk_plan_cases > walk_plan_cases.txt
//
// tests/cxx/walk_plan_check.cpp replays every line through walk_plan.h.  One case per line, unsigned integers:
//   in:   eng storage nchunks G num_layers M_upper M0 shortlist visited_mode mdim B ef chain no_self_seed lat_max_B lat4_max_B
//         small_table_tk adj_mag_mode table_min_B order_min_B chain_min_B side_min_B table_after_sort table_supported adj_mag_valid
//   have: table_level_min table_cols table_buffer n_order_keys order_level0 order_buffers
//   out:  kernel(0 general | 1 throughput | 2 one-wave | 3 four-wave) ordered use_table table_waits_for_sort use_adj_mag refill_adj_mag
//         chained side_stream table_level_min table_cols cut_after_level | prepared_order prepared_table (what that commit prepared)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "cosdata_hip.h"
#include "engine_types.h"

namespace cosdev {
bool walk_general_needed(const IndexDev &ix, u32 ef);
int walk_kernel_kind(int eng, const IndexDev &ix, const WalkArgs &wa, u32 lat_max_B, u32 lat4_max_B, bool table_available);
} // namespace cosdev
using cosdev::u32;
using cosdev::u64;

struct Case {
    u32 eng, storage, nchunks, G, num_layers, Mup, M0, shortlist, visited, mdim, B, ef, chain, noseed, lat, lat4, tk, adjmode, tmin, omin, cmin,
        smin, gate, tsupp, adjvalid, tlmin, tcols, tbuf, nkeys, klevel0, obuf;
};

static u32 g_tk = 1;
static void emit(const Case &c) {
    if (c.tk != g_tk) { // the one knob walk_kernel_kind reads from the registry itself
        cos_tuning_set("walk_small_table_tk", c.tk);
        g_tk = c.tk;
    }
    static const float dummy[1] = {0};
    cosdev::IndexDev dev;
    memset(&dev, 0, sizeof(dev));
    dev.storage = c.storage;
    dev.num_layers = c.num_layers;
    dev.shortlist = c.shortlist;
    dev.visited_mode = c.visited;
    dev.nchunks = c.nchunks;
    dev.G = c.G;
    dev.mdim = c.mdim;
    for (u32 l = 0; l <= c.num_layers; l++) {
        dev.lv[l].M = l == 0 ? c.M0 : c.Mup;
        dev.lv[l].adj_mag = (c.adjvalid && c.adjmode != 0) ? dummy : nullptr; // engine.hip:94
    }
    const u32 B = c.B, ef = c.ef;
    // ---- get_workspace (engine.hip:956-965): what was prepared
    const bool refill = !c.adjvalid && B >= 1024u;                                         // :956 (ADJ_MAG_REFILL_MIN_B, :925)
    const bool prep_order = c.omin && B >= c.omin && ef <= 256u;                           // :958
    const bool prep_table = c.tmin && (B >= c.tmin || B <= c.lat4);                        // :965
    // ---- run_search's snapshot (engine.hip:1020-1035)
    const u32 order_min_B = c.nkeys ? c.omin : 0u;                                         // :1020 (order_rank_valid && !order_levels.empty())
    const u32 n_keys = c.nkeys;
    const u32 tab_min_B = c.tmin;                                                          // :1026
    u32 tab_level_min = 0, tab_cols = 0;
    if (tab_min_B && c.tlmin && c.tbuf) {                                                  // :1027 (level_table_valid && table_level_min && w->tab && B * stride <= cap)
        tab_level_min = c.tlmin;
        tab_cols = c.tcols;
    }
    if (c.adjmode != 2)                                                                    // :1048
        for (u32 l = 0; l <= dev.num_layers; l++)
            if (ef > 2u * dev.lv[l].M || B < 4096u) dev.lv[l].adj_mag = nullptr;           // :1050 (ADJ_MAG_USE_MIN_B, :925)
    u32 adjmask = 0;
    for (u32 l = 0; l <= dev.num_layers; l++)
        if (dev.lv[l].adj_mag) adjmask |= 1u << l;
    const bool general = cosdev::walk_general_needed(dev, ef);                             // :1060
    const bool ordered = !general && order_min_B && B >= order_min_B && n_keys > 0 && c.obuf && ef <= 256u; // :1061 (w->order.cap >= B)
    if (general) tab_level_min = 0;                                                        // :1062
    if (tab_level_min) {                                                                   // :1063-1071
        cosdev::WalkArgs probe;
        memset(&probe, 0, sizeof(probe));
        probe.B = B;
        probe.ef = ef;
        const int kind = ordered ? 0 : cosdev::walk_kernel_kind((int)c.eng, dev, probe, c.lat, c.lat4, true);
        if (!((kind == 4 && c.eng == cosdev::ENG_U8) || (kind == 0 && (B >= tab_min_B || B <= c.lat4)))) tab_level_min = 0;
    }
    const bool chained = c.chain && B >= c.cmin;                                           // :1079
    const long long gate = c.gate;
    const bool waits = tab_level_min && chained && (gate == 2 || (gate == 1 && (u64)tab_cols * B >= (1ull << 30))); // :1080-1085
    const bool side = c.smin && B >= c.smin;                                               // :1119
    // ---- launch_walk (kernels_walk.hip:658-664), as run_search's walk lambda calls it (engine.hip:1140 unsplit, :1155 every range of a split walk)
    cosdev::WalkArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.B = B;
    wa.ef = ef;
    wa.no_self_seed = c.noseed;
    if (tab_level_min) wa.tab = dummy;                                                     // engine.hip:1107-1108
    int kernel;
    if (ordered) wa.phase = 1;                                                             // :1143
    if (cosdev::walk_general_needed(dev, wa.ef)) kernel = 0;                               // kernels_walk.hip:660
    else {
        const int kind = wa.no_self_seed ? 0                                               // kernels_walk.hip:662
                                         : cosdev::walk_kernel_kind((int)c.eng, dev, wa, ordered ? 0u : c.lat, ordered ? 0u : c.lat4, wa.tab != nullptr);
        kernel = kind == 4 ? 3 : kind == 1 ? 2 : 1;                                        // :663-664
    }
    if (!tab_level_min) tab_cols = 0;                                                      // cos_index_last_walk_split, engine.hip:1694-1696
    const u32 cut = ordered ? c.klevel0 : 0u;                                              // :1195
    printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d %d %d %d %u %d %d %d %u %u %u %d %d\n", c.eng,
           c.storage, c.nchunks, c.G, c.num_layers, c.Mup, c.M0, c.shortlist, c.visited, c.mdim, c.B, c.ef, c.chain, c.noseed, c.lat, c.lat4, c.tk,
           c.adjmode, c.tmin, c.omin, c.cmin, c.smin, c.gate, c.tsupp, c.adjvalid, c.tlmin, c.tcols, c.tbuf, c.nkeys, c.klevel0, c.obuf, kernel,
           (int)ordered, (int)(tab_level_min != 0), (int)waits, adjmask, (int)refill, (int)chained, (int)side, tab_level_min, tab_cols, cut,
           (int)prep_order, (int)prep_table);
}

struct Shape { u32 eng, storage, nchunks, G, tsupp; };
static const Shape SHAPES[] = {
    {cosdev::ENG_U8, COS_STORAGE_U8, 48, 64, 1},      // u8 x 768: one chunk pass
    {cosdev::ENG_U8, COS_STORAGE_U8, 6, 8, 1},        // u8 x 96: rows narrower than a wave
    {cosdev::ENG_U8, COS_STORAGE_U8, 256, 64, 1},     // u8 x 4096: four passes
    {cosdev::ENG_U8, COS_STORAGE_U8, 320, 64, 1},     // u8 x 5120: five passes (walk_general_kernel)
    {cosdev::ENG_Q2, COS_STORAGE_SUBBYTE, 12, 16, 1}, // quaternary x 768
    {cosdev::ENG_Q2, COS_STORAGE_SUBBYTE, 65, 64, 0}, // quaternary x 4160: more than 64 chunks (walk_general_kernel)
    {cosdev::ENG_Q1, COS_STORAGE_SUBBYTE, 6, 8, 0},   // binary x 768
    {cosdev::ENG_F32, COS_STORAGE_F32, 0, 2, 0},      // f32
};
struct Graph { u32 Mup, M0, shortlist; };
static const Graph GRAPHS[] = {{16, 32, 64}, {64, 64, 64}, {64, 256, 64}, {64, 256, 256}, {64, 128, 128}};
// both sides of every threshold: 1 | lat4 512 | lat 2048 | table min 3000 | order min 8192 | norms 1024, 4096 (= side min) | chain min 16384
static const u32 BS[] = {1, 512, 513, 1023, 1024, 2048, 2049, 2999, 3000, 4095, 4096, 8191, 8192, 16383, 16384};
static const u32 EFS[] = {1, 48, 64, 65, 128, 129, 256, 257, 1024, 1025};
static const u32 TMINS[] = {0, 1, 3000}, CMINS[] = {16384, 16384, 0, 0xFFFFFFFFu};

static Case base(const Shape &s, const Graph &g, u32 B, u32 ef) {
    Case c{};
    c.eng = s.eng; c.storage = s.storage; c.nchunks = s.nchunks; c.G = s.G; c.tsupp = s.tsupp;
    c.num_layers = 3; c.Mup = g.Mup; c.M0 = g.M0; c.shortlist = g.shortlist;
    c.B = B; c.ef = ef; c.chain = 1;
    c.lat = 2048; c.lat4 = 512; c.tk = 1; c.adjmode = 1; c.tmin = 1; c.omin = 8192; c.cmin = 16384; c.smin = 4096; c.gate = 1; c.adjvalid = 1;
    if (s.tsupp) { c.tlmin = 2; c.tcols = 700; c.tbuf = 1; }
    c.nkeys = 1; c.klevel0 = 1; c.obuf = 1;
    return c;
}

static u64 mix(u64 x) { // splitmix64: the thinned cross product's factor choices, reproducible
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

int main() {
    printf("# walk plan cases: the decisions of commit 157c5dc (scripts/gen_walk_plan_cases.cpp describes the columns)\n");
    // The cross product of every factor is thinned: the (B, ef) grid in full for the handle's defaults, and every other factor against
    // every B and every ef at least once (pairwise), not against every (B, ef) pair.
    // 1. the handle's defaults: every B at the ef edges of the order and the norms, every ef at the B edges of the kernel choice;
    //    small_table_tk off, a late table and a wide level 0 at the edges they move
    for (u32 B : BS)
        for (u32 ef : EFS)
            if (ef == 48u || ef == 64u || ef == 65u || ef == 256u || ef == 257u || B == 1u || B == 512u || B == 513u || B == 2048u || B == 2049u)
                emit(base(SHAPES[0], GRAPHS[0], B, ef));
    for (u32 v = 1; v < 4; v++)
        for (u32 B : {1u, 512u, 513u, 2048u, 2999u, 3000u, 8192u})
            for (u32 ef : {48u, 129u, 257u}) {
                Case c = base(SHAPES[0], GRAPHS[v == 3 ? 2 : 0], B, ef);
                c.tk = v != 1;
                c.tmin = v == 2 ? 3000 : 1;
                emit(c);
            }
    // 2. every engine and row shape against every B and every ef, the other factors drawn per case
    u64 n = 0;
    for (const Shape &s : SHAPES)
        for (u32 i = 0; i < 15; i++) {
            const u64 h = mix(++n), h2 = mix(h);
            Case c = base(s, GRAPHS[h % 4], BS[i], EFS[(i + n) % 10]);
            c.visited = (h >> 2) % 2;
            c.tk = (h >> 3) % 2;
            c.adjmode = (h >> 4) % 3;
            c.adjvalid = (h >> 6) % 2;
            c.tmin = TMINS[(h >> 7) % 3];
            if ((h >> 9) % 2) c.tlmin = c.tcols = c.tbuf = 0;
            if ((h >> 10) % 2) c.nkeys = c.klevel0 = 0;
            c.chain = (h >> 11) % 2;
            c.gate = (h >> 12) % 3;
            c.lat = (h >> 14) % 2 ? 2048 : 0;
            c.lat4 = (h >> 15) % 2 ? 512 : 0;
            c.omin = (h >> 16) % 4 ? 8192 : 0;
            c.smin = (h >> 18) % 4 ? 4096 : 0;
            c.cmin = CMINS[(h >> 20) % 4];
            c.mdim = (h2 % 8) == 0 ? 4 : 0;
            c.num_layers = 1 + (h2 >> 3) % 5;
            if (c.tlmin > c.num_layers) c.tlmin = c.num_layers;
            emit(c);
        }
    // 3. what preparation can leave short: no room for the workspace's table, no operand, short order buffers, no key level
    for (u32 miss = 0; miss < 4; miss++)
        for (u32 si : {0u, 4u})
            for (u32 B : {1u, 513u, 3000u, 8192u, 16384u})
                for (u32 ef : {48u, 257u}) {
                    if (si == 4u && (miss >= 2 || ef == 257u || B > 3000u)) continue;
                    Case c = base(SHAPES[si], GRAPHS[miss % 2], B, ef);
                    if (miss == 0) c.tbuf = 0;
                    if (miss == 1) c.tlmin = c.tcols = 0;
                    if (miss == 2) c.obuf = 0;
                    if (miss == 3) c.nkeys = c.klevel0 = 0;
                    emit(c);
                }
    // 4. the latency knobs at 0, one at a time and both
    for (u32 k = 0; k < 3; k++)
        for (u32 si : {0u, 4u})
            for (u32 B : {1u, 512u, 513u, 2048u, 2049u})
                for (u32 ef : {128u, 129u, 256u, 257u}) {
                    if (si == 4u && (ef == 129u || ef == 256u || B == 512u || B == 2048u)) continue;
                    Case c = base(SHAPES[si], GRAPHS[0], B, ef);
                    if (k != 1) c.lat = 0;
                    if (k != 0) c.lat4 = 0;
                    emit(c);
                }
    // 5. the builder's walks: no table, no order; insertion with the handle's latency knobs, delete_embedding's unseeded walk
    for (u32 si = 0; si < 8; si++)
        for (u32 gi : {0u, 3u})
            for (u32 B : {1u, 512u, 513u, 2048u, 2049u})
                for (u32 ef : {256u, 257u, 1025u})
                    for (u32 noseed = 0; noseed < 2; noseed++) {
                        if ((noseed && (B != 1 || ef != 256u)) || (gi == 3u && (si != 0 || ef != 256u)) || (ef != 256u && B != 1)) continue;
                        Case c = base(SHAPES[si], GRAPHS[gi], B, ef);
                        c.tmin = c.omin = 0;
                        c.tlmin = c.tcols = c.tbuf = c.nkeys = c.klevel0 = c.obuf = 0;
                        c.noseed = noseed;
                        emit(c);
                    }
    for (u32 B : {1u, 4096u, 8192u}) emit(base(SHAPES[0], GRAPHS[4], B, 48)); // 128 scanned slots on level 0: walk_general_kernel
    // 6. the after-sort gate: table_cols x B just under and at 2^30, every gate value, chained or not
    for (u32 gate = 0; gate < 3; gate++)
        for (u32 chain = 0; chain < 2; chain++)
            for (u32 B : {16383u, 16384u, 32768u})
                for (u32 cols : {32767u, 32768u, 65535u, 65536u}) {
                    if ((B == 32768u) != (cols < 65535u) || (B == 16383u && cols == 65535u)) continue;
                    Case c = base(SHAPES[0], GRAPHS[0], B, 64);
                    c.gate = gate;
                    c.chain = chain;
                    c.tcols = cols;
                    emit(c);
                }
    // 7. thresholds pulled down (tests/test_gpu_walk_plan.py): four waves up to 4 queries, one wave up to 16, table from 64, order from 128,
    //    chain and side stream from 256; the norms invalid at their two thresholds
    for (u32 B : {1u, 4u, 5u, 16u, 17u, 63u, 64u, 127u, 128u, 255u, 256u, 300u, 1023u, 1024u, 4095u, 4096u})
        for (u32 ef : {32u, 257u})
            for (u32 valid = 0; valid < 2; valid++) {
                if (!valid && (B < 1023u || ef != 32u)) continue;
                Case c = base(SHAPES[1], GRAPHS[0], B, ef);
                c.lat = 16; c.lat4 = 4; c.tmin = 64; c.omin = 128; c.cmin = 256; c.smin = 256;
                c.tlmin = 1; c.tcols = 190; c.adjvalid = valid;
                emit(c);
            }
    return 0;
}
