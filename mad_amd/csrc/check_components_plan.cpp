// check_components_plan.cpp -- a stand-alone host program over mad_components_plan.h, the host side of mad_map_components and
// mad_map_dust, meant to be built with a host sanitizer (make -C mad_amd/csrc check-components-plan builds and runs it with
// AddressSanitizer and UBSan).  No device, no launch: the argument checks, the tile counts, the halves of the neighbourhoods, the
// selection rule, and the two kernels replayed one lane after the other against heap buffers of exactly a tile's LDS and exactly
// the grid, with the kernels' own index expressions (cc_local, cc_in_tile, cc_on_face, cc_is_forward and the skipping rules of
// both), so that an index a kernel would form outside its memory is an out-of-bounds access here; the replayed forest is compared
// with a flood fill.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_components_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static int find(const int *p, int x) {
    while (p[x] != x) {
        CHECK(p[x] >= 0 && p[x] < x);
        x = p[x];
    }
    return x;
}

// the union of both kernels, one lane at a time: the atomic is a plain minimum here
static void unite(int *p, int a, int b) {
    a = find(p, a);
    b = find(p, b);
    while (a != b) {
        if (a < b) std::swap(a, b);
        const int old = p[a];
        p[a] = old < b ? old : b;
        if (old == a) break;
        a = find(p, old);
        b = find(p, b);
    }
}

// k_cc_tile and k_cc_border on a grid of foreground flags -> the root of every voxel (-1: background)
static void replay(const CcPlan &P, const std::vector<char> &fg, std::vector<int> &root) {
    const int nx = P.n[0], ny = P.n[1], nz = P.n[2];
    std::vector<int> p(P.n_vox);      // exactly the grid
    for (uint32_t b = 0; b < P.tiles; b++) {
        const uint32_t tz = b % P.bz, bt = b / P.bz, ty = bt % P.by, tx = bt / P.by;
        CHECK(tx < P.bx);
        const int x0 = (int)tx * CC_TX, y0 = (int)ty * CC_TY, z0 = (int)tz * CC_TZ;
        std::vector<int> s(CC_TILE);      // exactly the tile's LDS
        for (int row = 0; row < CC_ROWS; row++) {
            const int cx = row / CC_TY, cy = row % CC_TY, x = x0 + cx, y = y0 + cy;
            unsigned long long m = 0;
            for (int lane = 0; lane < CC_TZ; lane++)
                if (x < nx && y < ny && z0 + lane < nz && fg[((size_t)x * ny + y) * nz + z0 + lane]) m |= 1ull << lane;
            for (int lane = 0; lane < CC_TZ; lane++) {
                const unsigned long long gaps = ~m & ((1ull << lane) - 1ull);
                const int start = gaps ? 64 - __builtin_clzll(gaps) : 0;
                s.data()[cc_local(cx, cy, lane)] = (m >> lane & 1) ? cc_local(cx, cy, start) : -1;
            }
        }
        for (int row = 0; row < CC_ROWS; row++)
            for (int lane = 0; lane < CC_TZ; lane++) {
                const int cx = row / CC_TY, cy = row % CC_TY, l = cc_local(cx, cy, lane);
                if (s.data()[l] < 0) continue;
                const bool prev = lane > 0 && s.data()[l - 1] >= 0;
                for (int dx = 0; dx <= 1; dx++)
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dz = -1; dz <= 1; dz++) {
                            if (!cc_is_forward(dx, dy, dz, P.conn) || (dx == 0 && dy == 0)) continue;
                            const int ncx = cx + dx, ncy = cy + dy, ncz = lane + dz;
                            if (!cc_in_tile(ncx, ncy, ncz)) continue;
                            const int mm = cc_local(ncx, ncy, ncz);
                            if (s.data()[mm] < 0) continue;
                            if (prev && ncz > 0 && s.data()[mm - 1] >= 0) continue;
                            unite(s.data(), l, mm);
                        }
            }
        for (int row = 0; row < CC_ROWS; row++)
            for (int lane = 0; lane < CC_TZ; lane++) {
                const int cx = row / CC_TY, cy = row % CC_TY, x = x0 + cx, y = y0 + cy, z = z0 + lane;
                if (x >= nx || y >= ny || z >= nz) continue;
                const int l = cc_local(cx, cy, lane);
                int out = -1;
                if (s.data()[l] >= 0) {
                    const int r = find(s.data(), l);
                    const int rx = r / (CC_TY * CC_TZ), ry = r / CC_TZ % CC_TY, rz = r % CC_TZ;
                    out = (int)(((long long)(x0 + rx) * ny + (y0 + ry)) * nz + (z0 + rz));
                }
                p.data()[((size_t)x * ny + y) * nz + z] = out;
            }
    }
    const int sx = ny * nz, sy = nz;
    for (uint32_t b = 0; b < P.tiles; b++) {
        const uint32_t tz = b % P.bz, bt = b / P.bz, ty = bt % P.by, tx = bt / P.by;
        const int x0 = (int)tx * CC_TX, y0 = (int)ty * CC_TY, z0 = (int)tz * CC_TZ;
        for (int row = 0; row < CC_ROWS; row++)
            for (int lane = 0; lane < CC_TZ; lane++) {
                const int cx = row / CC_TY, cy = row % CC_TY, x = x0 + cx, y = y0 + cy, z = z0 + lane;
                if (x >= nx || y >= ny || z >= nz) continue;
                const int L = (int)(((long long)x * ny + y) * nz + z);
                const bool prev = cc_row_on_face(cx, cy) && lane > 0 && p.data()[L - 1] >= 0;
                for (int dx = 0; dx <= 1; dx++)
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dz = -1; dz <= 1; dz++) {
                            if (!cc_is_forward(dx, dy, dz, P.conn) || cc_in_tile(cx + dx, cy + dy, lane + dz)) continue;
                            CHECK(cc_on_face(cx, cy, lane));      // no voxel off the faces has a neighbour in another tile
                            if (!cc_on_face(cx, cy, lane) || p.data()[L] < 0) continue;
                            const int X = x + dx, Y = y + dy, Z = z + dz;
                            if (X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                            const int M = L + dx * sx + dy * sy + dz;
                            if (p.data()[M] < 0) continue;
                            if (prev && Z % CC_TZ != 0 && p.data()[M - 1] >= 0) continue;
                            unite(p.data(), L, M);
                        }
            }
    }
    root.assign(P.n_vox, -1);
    for (uint32_t i = 0; i < P.n_vox; i++)
        if (p[i] >= 0) root[i] = find(p.data(), (int)i);
}

// the definition: a flood fill from every voxel not yet reached, in ascending L, so that the seed is the component's smallest L
static void define(const CcPlan &P, const std::vector<char> &fg, std::vector<int> &root) {
    const int nx = P.n[0], ny = P.n[1], nz = P.n[2];
    root.assign(P.n_vox, -1);
    std::vector<int> stack;
    for (uint32_t i = 0; i < P.n_vox; i++) {
        if (!fg[i] || root[i] >= 0) continue;
        root[i] = (int)i;
        stack.push_back((int)i);
        while (!stack.empty()) {
            const int L = stack.back();
            stack.pop_back();
            const int x = L / (ny * nz), y = L / nz % ny, z = L % nz;
            for (int dx = -1; dx <= 1; dx++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dz = -1; dz <= 1; dz++) {
                        if (!cc_is_neighbour(dx, dy, dz, P.conn)) continue;
                        const int X = x + dx, Y = y + dy, Z = z + dz;
                        if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                        const int M = (X * ny + Y) * nz + Z;
                        if (fg[M] && root[M] < 0) { root[M] = (int)i; stack.push_back(M); }
                    }
        }
    }
}

int main() {
    char msg[320];
    CcPlan P;
    const char *who = "mad_map_components";
    {   // a good call, and the refusals
        const int32_t d[3] = {20, 24, 70};
        CHECK(cc_plan(who, d, 0.5, 26, P, msg, sizeof msg) == CC_OK);
        CHECK(P.n_vox == 20u * 24 * 70 && P.bx == 3 && P.by == 3 && P.bz == 2 && P.tiles == 18 && P.conn == 26);
        CHECK(cc_plan(who, d, -INFINITY, 6, P, msg, sizeof msg) == CC_OK && cc_plan(who, d, INFINITY, 18, P, msg, sizeof msg) == CC_OK);
        const int32_t d0[3] = {20, 0, 70}, dn[3] = {-1, 4, 4}, big[3] = {2048, 1024, 1024}, edge[3] = {1, 1, 2147483647}, one[3] = {1, 1, 1};
        CHECK(cc_plan(who, d0, 0.5, 26, P, msg, sizeof msg) == CC_EINVAL && strstr(msg, "grid of 20 x 0 x 70"));
        CHECK(cc_plan(who, dn, 0.5, 26, P, msg, sizeof msg) == CC_EINVAL);
        CHECK(cc_plan(who, big, 0.5, 26, P, msg, sizeof msg) == CC_EINVAL && strstr(msg, "2^31"));
        CHECK(cc_plan(who, edge, 0.5, 26, P, msg, sizeof msg) == CC_OK && P.bx == 1 && P.by == 1 && P.bz == (1u << 25) && P.tiles == (1u << 25));
        CHECK(cc_plan(who, one, 0.5, 26, P, msg, sizeof msg) == CC_OK && P.tiles == 1 && P.n_vox == 1);
        CHECK(cc_plan(who, d, NAN, 26, P, msg, sizeof msg) == CC_EINVAL && strstr(msg, "threshold"));
        for (int conn = -1; conn <= 30; conn++)
            CHECK((cc_plan(who, d, 0.5, conn, P, msg, sizeof msg) == CC_OK) == (conn == 6 || conn == 18 || conn == 26));
        CHECK(strstr(msg, "connectivity 30"));
        CHECK(cc_dust_args(who, 0.5, 1, 0, 0.0f, msg, sizeof msg) == CC_OK && cc_dust_args(who, 0.5, 7, 3, 0.5f, msg, sizeof msg) == CC_OK);
        CHECK(cc_dust_args(who, 0.5, 0, 0, 0.0f, msg, sizeof msg) == CC_EINVAL && strstr(msg, "min_size 0"));
        CHECK(cc_dust_args(who, 0.5, 1, -1, 0.0f, msg, sizeof msg) == CC_EINVAL);
        CHECK(cc_dust_args(who, 0.5, 1, 0, 0.75f, msg, sizeof msg) == CC_EINVAL && strstr(msg, "fill"));
        CHECK(cc_dust_args(who, 0.5, 1, 0, NAN, msg, sizeof msg) == CC_EINVAL && cc_dust_args(who, 0.5, 1, 0, -INFINITY, msg, sizeof msg) == CC_EINVAL);
        CHECK(cc_dust_args(who, INFINITY, 1, 0, INFINITY, msg, sizeof msg) == CC_EINVAL);
        CHECK(cc_dust_args(who, -INFINITY, 1, 0, -3.0e38f, msg, sizeof msg) == CC_EINVAL);      // nothing is at or below -inf and finite
        CHECK(cc_dust_args(who, -1.0, 1, 0, -1.0f, msg, sizeof msg) == CC_OK && cc_dust_args(who, -1.0, 1, 0, 0.0f, msg, sizeof msg) == CC_EINVAL);
    }
    // the halves: 3, 9, 13 forward offsets; a half and its mirror image make the neighbourhood, and share nothing
    for (int conn : {6, 18, 26}) {
        int fwd = 0, all = 0;
        for (int dx = -1; dx <= 1; dx++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dz = -1; dz <= 1; dz++) {
                    const bool f = cc_is_forward(dx, dy, dz, conn), bk = cc_is_forward(-dx, -dy, -dz, conn), nb = cc_is_neighbour(dx, dy, dz, conn);
                    fwd += f;
                    all += nb;
                    CHECK(!(f && bk) && (f || bk) == nb);
                    if (f) CHECK(dx >= 0 && (dx * 512 + dy * 64 + dz) > 0);
                }
        CHECK(all == conn && fwd == conn / 2);
    }
    CHECK(cc_local(0, 0, 0) == 0 && cc_local(CC_TX - 1, CC_TY - 1, CC_TZ - 1) == CC_TILE - 1 && cc_local(1, 2, 3) == (1 * 8 + 2) * 64 + 3);
    // both kernels replayed: grids that are no multiple of the tile, one voxel thin, and of several tiles along every axis
    const int32_t shapes[][3] = {{1, 1, 1}, {1, 1, 70}, {70, 1, 1}, {5, 66, 3}, {9, 9, 130}, {17, 18, 65}, {16, 16, 128}};
    unsigned long long rng = 0x9e3779b97f4a7c15ull;
    std::vector<int> got, want;
    for (const auto &sh : shapes)
        for (int conn : {6, 18, 26})
            for (int dens : {5, 20, 32, 60, 100}) {
                CHECK(cc_plan(who, sh, 0.5, conn, P, msg, sizeof msg) == CC_OK);
                std::vector<char> fg(P.n_vox);
                for (auto &f : fg) {
                    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                    f = (int)((rng >> 33) % 100) < dens;
                }
                replay(P, fg, got);
                define(P, fg, want);
                CHECK(got == want);
            }
    {   // the selection: size descending, root ascending; min_size and keep together
        const int64_t root[6] = {0, 5, 9, 20, 31, 40}, size[6] = {2, 7, 2, 7, 1, 3};
        std::vector<int32_t> flag;
        int64_t c[4];
        cc_select(6, root, size, 1, 0, flag, c);
        CHECK(flag == std::vector<int32_t>({1, 1, 1, 1, 1, 1}) && c[0] == 6 && c[1] == 6 && c[2] == 22 && c[3] == 22);
        cc_select(6, root, size, 1, 1, flag, c);      // of the two of size 7 the smaller root
        CHECK(flag == std::vector<int32_t>({0, 1, 0, 0, 0, 0}) && c[1] == 1 && c[3] == 7);
        cc_select(6, root, size, 1, 4, flag, c);      // ranks: 1, 3, 5, 0, 2, 4 -> the fourth is the component of size 2 at root 0
        CHECK(flag == std::vector<int32_t>({1, 1, 0, 1, 0, 1}) && c[1] == 4 && c[3] == 19);
        cc_select(6, root, size, 3, 0, flag, c);
        CHECK(flag == std::vector<int32_t>({0, 1, 0, 1, 0, 1}) && c[1] == 3 && c[3] == 17);
        cc_select(6, root, size, 3, 5, flag, c);      // the rank admits five, the size three of them
        CHECK(flag == std::vector<int32_t>({0, 1, 0, 1, 0, 1}) && c[1] == 3);
        cc_select(6, root, size, 8, 2, flag, c);
        CHECK(flag == std::vector<int32_t>({0, 0, 0, 0, 0, 0}) && c[0] == 6 && c[1] == 0 && c[2] == 22 && c[3] == 0);
        cc_select(0, root, size, 1, 0, flag, c);
        CHECK(flag.empty() && c[0] == 0 && c[1] == 0 && c[2] == 0 && c[3] == 0);
    }
    if (failures) {
        fprintf(stderr, "check_components_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("check_components_plan: ok\n");
    return 0;
}
