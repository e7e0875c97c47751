// check_confidence_plan.cpp -- a stand-alone host program over mad_confidence_plan.h, the host side of mad_map_sort, mad_map_kth and
// mad_map_confidence, meant to be built with a host sanitizer (make -C mad_amd/csrc check-confidence-plan builds and runs it with
// AddressSanitizer and UBSan).  No device, no launch: the tile and table arithmetic at its edges, the refusals, the key of a value
// and its inverse, the noise boxes and the voxel of a sample, the two searches the device shares, and the passes of the sort replayed
// one lane after the other against heap buffers of exactly the keys, exactly a pass's table and exactly a tile's LDS, with the
// kernels' own index expressions (cf_key_index, cf_table_index, cf_digit), so that an index a kernel would form outside its memory
// is an out-of-bounds access here; the replayed sort is compared with std::sort.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "mad_confidence_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float value(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// k_cf_count, mad_scan_i32 and k_cf_scatter for every pass: float bits in, float bits out, descending
static std::vector<uint32_t> replay(const CfPlan &P, const std::vector<uint32_t> &grid) {
    std::vector<uint32_t> a(grid), b(P.n);      // exactly the keys
    for (int pass = 0; pass < CF_PASSES; pass++) {
        const bool first = pass == 0, last = pass == CF_PASSES - 1;
        std::vector<int32_t> tab(P.table), off((size_t)P.table + 1);      // exactly a pass's table, and its scan
        for (uint32_t tile = 0; tile < P.tiles; tile++) {
            std::vector<uint32_t> s_h(CF_RADIX, 0u);
            for (uint32_t w = 0; w < CF_WAVES; w++)
                for (uint32_t r = 0; r < CF_ROUNDS; r++)
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        const uint32_t i = cf_key_index(tile, w, r, lane);
                        if (i >= P.n) continue;
                        const uint32_t u = first ? cf_key(a.data()[i]) : a.data()[i];
                        s_h.data()[cf_digit(u, pass)]++;
                    }
            for (uint32_t t = 0; t < CF_THREADS; t++) tab.data()[cf_table_index(t, tile, P.tiles)] = (int32_t)s_h.data()[t];
        }
        long long run = 0;
        for (uint32_t e = 0; e < P.table; e++) {
            off.data()[e] = (int32_t)run;
            run += tab.data()[e];
        }
        off.data()[P.table] = (int32_t)run;
        CHECK(run == (long long)P.n);
        for (uint32_t tile = 0; tile < P.tiles; tile++) {
            std::vector<uint32_t> s_keys(CF_TILE), s_cnt((size_t)CF_WAVES * CF_RADIX, 0u), s_start(CF_RADIX), s_gbase(CF_RADIX);      // exactly the LDS
            std::vector<uint32_t> key((size_t)CF_TILE), rank((size_t)CF_TILE);      // the lanes' registers, [w][r][lane]
            for (uint32_t w = 0; w < CF_WAVES; w++)
                for (uint32_t r = 0; r < CF_ROUNDS; r++) {
                    uint32_t d[64];
                    bool valid[64];
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        const uint32_t i = cf_key_index(tile, w, r, lane), at = (w * CF_ROUNDS + r) * 64 + lane;
                        valid[lane] = i < P.n;
                        const uint32_t u = valid[lane] ? a.data()[i] : 0u;
                        key.data()[at] = first ? cf_key(u) : u;
                        d[lane] = cf_digit(key.data()[at], pass);
                    }
                    uint32_t pre[64];      // the counters as the round finds them: every group's first lane reads before any writes matter
                    for (uint32_t lane = 0; lane < 64; lane++) pre[lane] = s_cnt.data()[w * CF_RADIX + d[lane]];
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        if (!valid[lane]) continue;
                        uint32_t below = 0, all = 0;
                        for (uint32_t o = 0; o < 64; o++)
                            if (valid[o] && d[o] == d[lane]) { all++; below += o < lane; }
                        rank.data()[(w * CF_ROUNDS + r) * 64 + lane] = pre[lane] + below;
                        if (below == 0) s_cnt.data()[w * CF_RADIX + d[lane]] = pre[lane] + all;
                    }
                }
            uint32_t start = 0;
            for (uint32_t t = 0; t < CF_THREADS; t++) {
                uint32_t before = 0;
                for (uint32_t w = 0; w < CF_WAVES; w++) {
                    const uint32_t c = s_cnt.data()[w * CF_RADIX + t];
                    s_cnt.data()[w * CF_RADIX + t] = before;
                    before += c;
                }
                s_start.data()[t] = start;
                s_gbase.data()[t] = (uint32_t)off.data()[cf_table_index(t, tile, P.tiles)] - start;
                start += before;
            }
            const uint32_t n_valid = std::min((uint32_t)CF_TILE, P.n - tile * (uint32_t)CF_TILE);
            CHECK(start == n_valid);
            for (uint32_t w = 0; w < CF_WAVES; w++)
                for (uint32_t r = 0; r < CF_ROUNDS; r++)
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        if (cf_key_index(tile, w, r, lane) >= P.n) continue;
                        const uint32_t at = (w * CF_ROUNDS + r) * 64 + lane, dd = cf_digit(key.data()[at], pass);
                        s_keys.data()[s_start.data()[dd] + s_cnt.data()[w * CF_RADIX + dd] + rank.data()[at]] = key.data()[at];
                    }
            for (uint32_t r = 0; r < CF_ROUNDS; r++)
                for (uint32_t t = 0; t < CF_THREADS; t++) {
                    const uint32_t pos = r * CF_THREADS + t;
                    if (pos >= n_valid) continue;
                    const uint32_t k = s_keys.data()[pos];
                    const uint32_t dst = s_gbase.data()[cf_digit(k, pass)] + pos;
                    CHECK(dst < P.n);
                    if (dst < P.n) b.data()[dst] = last ? cf_unkey(k) : k;
                }
        }
        a.swap(b);
    }
    return a;
}

int main() {
    char msg[320];
    CfPlan P;
    const char *who = "mad_map_sort";
    {   // the tile and table arithmetic at its edges, and the refusals
        CHECK(cf_plan(who, 1, P, msg, sizeof msg) == CF_OK && P.n == 1 && P.tiles == 1 && P.table == CF_RADIX && P.q_blocks == 1 && P.key_bytes == 4);
        CHECK(cf_plan(who, CF_TILE, P, msg, sizeof msg) == CF_OK && P.tiles == 1 && P.table == CF_RADIX);
        CHECK(cf_plan(who, CF_TILE + 1, P, msg, sizeof msg) == CF_OK && P.tiles == 2 && P.table == 2 * CF_RADIX && P.table_bytes >= (2 * CF_RADIX + 1) * 4);
        CHECK(cf_plan(who, CF_QBLOCK + 1, P, msg, sizeof msg) == CF_OK && P.q_blocks == 2);
        CHECK(cf_plan(who, (1ll << 31) - 1, P, msg, sizeof msg) == CF_OK && P.n == 2147483647u && P.tiles == (1u << 19) && P.table == (1u << 27));
        CHECK(P.table_bytes % 256 == 0 && P.table_bytes >= ((size_t)P.table + 1) * 4 && P.key_bytes == (size_t)P.n * 4 && P.q_blocks == (1u << 20));
        // the largest index a lane of the last tile forms, and the largest table entry, in 32 bits
        CHECK((unsigned long long)(P.tiles - 1) * CF_TILE + CF_TILE - 1 < (1ull << 32) && cf_key_index(P.tiles - 1, CF_WAVES - 1, CF_ROUNDS - 1, 63) == (1u << 31) - 1u);
        CHECK(cf_table_index(CF_RADIX - 1, P.tiles - 1, P.tiles) == P.table - 1);
        CHECK(cf_plan(who, 0, P, msg, sizeof msg) == CF_EINVAL && strstr(msg, "0 voxels"));
        CHECK(cf_plan(who, -5, P, msg, sizeof msg) == CF_EINVAL);
        CHECK(cf_plan(who, 1ll << 31, P, msg, sizeof msg) == CF_EINVAL && strstr(msg, "2^31"));
        const int32_t d[3] = {20, 24, 70}, d0[3] = {20, 0, 70}, big[3] = {2048, 1024, 1024}, edge[3] = {1, 1, 2147483647};
        CHECK(cf_plan_dims(who, d, P, msg, sizeof msg) == CF_OK && P.n == 20u * 24 * 70 && P.tiles == 9);
        CHECK(cf_plan_dims(who, d0, P, msg, sizeof msg) == CF_EINVAL && strstr(msg, "grid of 20 x 0 x 70"));
        CHECK(cf_plan_dims(who, big, P, msg, sizeof msg) == CF_EINVAL && strstr(msg, "2^31"));
        CHECK(cf_plan_dims(who, edge, P, msg, sizeof msg) == CF_OK && P.n == 2147483647u);
        const int64_t k_ok[3] = {1, 33600, 7}, k_lo[2] = {1, 0}, k_hi[1] = {33601};
        CHECK(cf_kth_args(who, 33600, 3, k_ok, msg, sizeof msg) == CF_OK);
        CHECK(cf_kth_args(who, 33600, 2, k_lo, msg, sizeof msg) == CF_EINVAL && strstr(msg, "rank 0"));
        CHECK(cf_kth_args(who, 33600, 1, k_hi, msg, sizeof msg) == CF_EINVAL && strstr(msg, "rank 33601"));
        CHECK(cf_kth_args(who, 33600, 0, k_ok, msg, sizeof msg) == CF_EINVAL && cf_kth_args(who, 33600, CF_MAX_K + 1, k_ok, msg, sizeof msg) == CF_EINVAL);
    }
    {   // the key: descending values have ascending keys; -0.0 is +0.0; the inverse; what is not finite
        const float v[] = {3.0e38f, 1.0f, 1.0e-38f, 1.4e-45f, 0.0f, -1.4e-45f, -1.0e-38f, -1.0f, -3.0e38f};
        for (size_t i = 0; i + 1 < sizeof v / sizeof v[0]; i++) CHECK(cf_key(bits(v[i])) < cf_key(bits(v[i + 1])));
        for (float f : v) CHECK(cf_unkey(cf_key(bits(f))) == bits(f) && cf_bits_finite(bits(f)));
        CHECK(cf_key(bits(-0.0f)) == cf_key(bits(0.0f)) && cf_unkey(cf_key(bits(-0.0f))) == 0u);
        CHECK(cf_key(0x7f7fffffu) == 0x00800000u && cf_key(0xff7fffffu) == 0xff7fffffu);      // the largest and the smallest finite value
        CHECK(!cf_bits_finite(bits(INFINITY)) && !cf_bits_finite(bits(-INFINITY)) && !cf_bits_finite(bits(NAN)) && !cf_bits_finite(0xffc00001u));
        CHECK(cf_digit(0xa1b2c3d4u, 0) == 0xd4 && cf_digit(0xa1b2c3d4u, 1) == 0xc3 && cf_digit(0xa1b2c3d4u, 3) == 0xa1);
    }
    {   // the passes replayed: one key, around a tile, several tiles with a partial one; bits of every kind
        unsigned long long rng = 0x9e3779b97f4a7c15ull;
        auto next = [&]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 32); };
        for (long long n : {1ll, 2ll, 63ll, 64ll, 65ll, 257ll, (long long)CF_TILE - 1, (long long)CF_TILE, (long long)CF_TILE + 1, 3ll * CF_TILE + 77})
            for (int kind = 0; kind < 5; kind++) {
                CHECK(cf_plan(who, n, P, msg, sizeof msg) == CF_OK);
                std::vector<uint32_t> g((size_t)n);
                for (auto &u : g) {
                    uint32_t x = next();
                    if (kind == 0) { while (!cf_bits_finite(x)) x = next(); }                       // any finite bits
                    else if (kind == 1) x = bits(1.5f);                                             // all equal
                    else if (kind == 2) x = (x % 10 < 7) ? ((x & 1u) << 31) : bits(1.0f + (float)(x % 5));      // zeros of both signs, a few values
                    else if (kind == 3) x = 0x3f800000u | (x & 0xffu);                              // the lowest byte only
                    else x = (x & 0x7f000000u) == 0x7f000000u ? 0x12345u : ((x & 0xff000000u) | 0x12345u);      // the highest byte only
                    u = x;
                }
                std::vector<uint32_t> want(g);
                for (auto &u : want) u = cf_unkey(cf_key(u));
                std::sort(want.begin(), want.end(), [](uint32_t x, uint32_t y) { return cf_key(x) < cf_key(y); });
                for (size_t i = 0; i + 1 < want.size(); i++) CHECK(value(want[i]) >= value(want[i + 1]));
                const std::vector<uint32_t> got = replay(P, g);
                CHECK(got == want);
                for (size_t i = 0; i < want.size(); i += 97) CHECK(cf_find_key(want.data(), n, cf_key(want[i])) >= 0 && want[(size_t)cf_find_key(want.data(), n, cf_key(want[i]))] == want[i]);
                CHECK(cf_find_key(want.data(), n, cf_key(bits(-7.25f))) == -1);
            }
    }
    {   // the noise boxes
        const char *w = "mad_map_confidence";
        const int32_t d[3] = {20, 24, 70};
        int64_t first[8], n = 0;
        const int32_t ok[3][4] = {{0, 0, 0, 2}, {17, 21, 67, 3}, {5, 5, 5, 1}};
        CHECK(cf_boxes(w, d, 3, &ok[0][0], first, &n, msg, sizeof msg) == CF_OK && n == 36 && first[0] == 0 && first[1] == 8 && first[2] == 35 && first[3] == 36);
        CHECK(cf_sample_voxel(0, 3, &ok[0][0], first, 24, 70) == 0 && cf_sample_voxel(7, 3, &ok[0][0], first, 24, 70) == (1 * 24 + 1) * 70 + 1);
        CHECK(cf_sample_voxel(8, 3, &ok[0][0], first, 24, 70) == (17 * 24 + 21) * 70 + 67 && cf_sample_voxel(34, 3, &ok[0][0], first, 24, 70) == 20 * 24 * 70 - 1);
        CHECK(cf_sample_voxel(35, 3, &ok[0][0], first, 24, 70) == (5 * 24 + 5) * 70 + 5);
        CHECK(cf_sample_voxel(8 + 5, 3, &ok[0][0], first, 24, 70) == ((17 + 0) * 24 + 21 + 1) * 70 + 67 + 2);      // file order: z fastest
        const int32_t out_hi[1][4] = {{18, 0, 0, 3}}, out_lo[1][4] = {{0, -1, 0, 3}}, zero[1][4] = {{0, 0, 0, 0}}, neg[1][4] = {{0, 0, 0, -2}}, one[1][4] = {{3, 3, 3, 1}};
        const int32_t huge[1][4] = {{0, 0, 0, 2147483647}}, whole[1][4] = {{0, 0, 0, 20}};
        CHECK(cf_boxes(w, d, 1, &out_hi[0][0], first, &n, msg, sizeof msg) == CF_EINVAL && strstr(msg, "not inside the grid"));
        CHECK(cf_boxes(w, d, 1, &out_lo[0][0], first, &n, msg, sizeof msg) == CF_EINVAL);
        CHECK(cf_boxes(w, d, 1, &zero[0][0], first, &n, msg, sizeof msg) == CF_EINVAL && strstr(msg, "edge 0"));
        CHECK(cf_boxes(w, d, 1, &neg[0][0], first, &n, msg, sizeof msg) == CF_EINVAL && cf_boxes(w, d, 1, &huge[0][0], first, &n, msg, sizeof msg) == CF_EINVAL);
        CHECK(cf_boxes(w, d, 1, &one[0][0], first, &n, msg, sizeof msg) == CF_EINVAL && strstr(msg, "2 or more"));
        CHECK(cf_boxes(w, d, 1, &whole[0][0], first, &n, msg, sizeof msg) == CF_OK && n == 8000);
        CHECK(cf_boxes(w, d, 0, &ok[0][0], first, &n, msg, sizeof msg) == CF_EINVAL && cf_boxes(w, d, CF_MAX_BOXES + 1, &ok[0][0], first, &n, msg, sizeof msg) == CF_EINVAL);
        const double lv[3] = {0.01, 0.0, 1.0}, bad1[1] = {-0.01}, bad2[1] = {1.5}, bad3[1] = {NAN};
        CHECK(cf_levels(w, 1.0, 3, lv, msg, sizeof msg) == CF_OK && cf_levels(w, 17.2, 0, nullptr, msg, sizeof msg) == CF_OK);
        CHECK(cf_levels(w, 0.5, 3, lv, msg, sizeof msg) == CF_EINVAL && cf_levels(w, NAN, 3, lv, msg, sizeof msg) == CF_EINVAL && cf_levels(w, INFINITY, 3, lv, msg, sizeof msg) == CF_EINVAL);
        CHECK(cf_levels(w, 1.0, 1, bad1, msg, sizeof msg) == CF_EINVAL && cf_levels(w, 1.0, 1, bad2, msg, sizeof msg) == CF_EINVAL && cf_levels(w, 1.0, 1, bad3, msg, sizeof msg) == CF_EINVAL);
        CHECK(cf_levels(w, 1.0, -1, lv, msg, sizeof msg) == CF_EINVAL && cf_levels(w, 1.0, CF_MAX_LEVELS + 1, lv, msg, sizeof msg) == CF_EINVAL);
    }
    {   // the level search on monotone arrays made by hand
        const double q[8] = {0.0, 1e-300, 0.004, 0.01, 0.01, 0.01, 0.5, 1.0};
        std::vector<double> h(q, q + 8);      // on the heap: a read past either end is seen
        CHECK(cf_level_count(h.data(), 8, 0.01) == 6 && cf_level_count(h.data(), 8, 0.0099999) == 3 && cf_level_count(h.data(), 8, 0.0) == 1);
        CHECK(cf_level_count(h.data(), 8, 1.0) == 8 && cf_level_count(h.data(), 8, 0.75) == 7 && cf_level_count(h.data() + 2, 6, 0.001) == 0);
        CHECK(cf_level_count(h.data(), 1, 0.0) == 1 && cf_level_count(h.data() + 7, 1, 0.99) == 0 && cf_level_count(h.data(), 0, 0.5) == 0);
        std::vector<double> ones(1000, 1.0), ramp(1000);
        for (int i = 0; i < 1000; i++) ramp[(size_t)i] = i / 1000.0;
        CHECK(cf_level_count(ones.data(), 1000, 0.05) == 0 && cf_level_count(ones.data(), 1000, 1.0) == 1000);
        for (int i = 0; i < 1000; i += 37) CHECK(cf_level_count(ramp.data(), 1000, i / 1000.0) == i + 1);
    }
    if (failures) {
        fprintf(stderr, "check_confidence_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("check_confidence_plan: ok\n");
    return 0;
}
