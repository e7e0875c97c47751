// check_localfilter_plan.cpp -- a stand-alone host program over mad_localfilter_plan.h, the host side of mad_map_local_filter, meant
// to be built with a host sanitizer (make -C mad_amd/csrc check-localfilter-plan builds and runs it with AddressSanitizer and
// UBSan).  No device, no launch: the argument checks, the scan of the samples, and the arithmetic of tiles, halos and slabs, which
// is replayed against a heap buffer of exactly the launch's LDS size with the kernel's own index expressions, so that an index the
// kernel would form outside its LDS is an out-of-bounds access here.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_localfilter_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static const double K = M_PI * sqrt(2.0);

static int plan(const int32_t d[3], double voxsp, const std::vector<double> &res, const int32_t rd[3], int step, LfPlan &P, char *msg) {
    return lf_plan(d, voxsp, res.data(), rd, step, K, P, msg, 320);
}

// every LDS index k_lf_tile forms for a tile whose largest radius is H, in a launch with `lds` bytes of dynamic LDS
static void replay_tile(int H, unsigned lds) {
    std::vector<unsigned char> mem(lds);      // exactly the launch's size: one byte past it is the sanitizer's
    double *S = (double *)mem.data();
    int *ctl = (int *)(mem.data() + LF_LDS_SUMS);
    float *img = (float *)(mem.data() + LF_LDS_HEAD);
    for (int i = 0; i < LF_PER_THREAD; i++)
        for (int t = 0; t < LF_THREADS; t++) S[i * LF_THREADS + t] = 0.0;
    ctl[0] = H;
    const LfSlab sl = lf_slab(H, lds);
    CHECK(sl.planes >= 1 && sl.n_slabs >= 1 && sl.n_slabs * sl.planes >= LF_TX + 2 * H && (sl.n_slabs - 1) * sl.planes < LF_TX + 2 * H);
    CHECK((size_t)LF_LDS_HEAD + (size_t)sl.planes * sl.py * sl.pz * 4 <= lds);
    const int x0 = 0, x_end = x0 + LF_TX + H;
    long long covered = 0;
    for (int s = 0; s < sl.n_slabs; s++) {
        const int xs = x0 - H + s * sl.planes, np = sl.planes < x_end - xs ? sl.planes : x_end - xs;
        CHECK(np >= 1);
        for (int r = 0; r < np * sl.py; r++)
            for (int rz = 0; rz < sl.pz; rz++) img[r * sl.pz + rz] = 1.f;
        // the reads of the corner threads and a middle one at the largest radius: dx, dy and k at their extremes
        const int ls[3] = {0, 3, 7}, zs[3] = {0, 17, LF_TZ - 1};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++)
                for (int ox = 0; ox < LF_TX; ox++) {
                    const int ly = ls[a], lz = zs[b], x = x0 + ox;
                    const int d_lo = -H > xs - x ? -H : xs - x, d_hi = H < xs + np - 1 - x ? H : xs + np - 1 - x;
                    const float *centre = img + ((ly + H) * sl.pz + lz + H);
                    float sum = 0.f;
                    for (int dx = d_lo; dx <= d_hi; dx++) {
                        const float *plane = centre + (x + dx - xs) * sl.py * sl.pz;
                        for (int dy = -H; dy <= H; dy += H) sum += (plane + dy * sl.pz)[-H] + (plane + dy * sl.pz)[H];
                        if (a == 0 && b == 0) covered++;
                    }
                    CHECK(sum == 6.f * (float)(d_hi >= d_lo ? d_hi - d_lo + 1 : 0));
                }
    }
    CHECK(covered == (long long)LF_TX * (2 * H + 1));      // every (output, dx) met in exactly one slab
}

int main() {
    char msg[320];
    LfPlan P;
    {   // a good call: lattice, tiles, the halo from the largest sample
        const int32_t d[3] = {20, 24, 70}, rd[3] = {7, 8, 24};
        std::vector<double> res((size_t)7 * 8 * 24, 8.0);
        res[5] = 20.0;
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_OK);
        CHECK(P.m[0] == 7 && P.m[1] == 8 && P.m[2] == 24 && P.n_vox == (size_t)20 * 24 * 70 && P.n_res == res.size());
        CHECK(P.tiles[0] == 3 && P.tiles[1] == 3 && P.tiles[2] == 3 && P.n_tiles == 27);
        CHECK(P.H == lf_radius(20.0 / (1.5 * K)) && P.H == 12 && P.lds == LF_LDS_BYTES);
        res[5] = 8.0;
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_OK && P.H == 5 && P.lds == lf_lds_bytes(5) && P.lds < LF_LDS_BYTES);
        // the refusals
        res[17] = 0.0;
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_EINVAL && strstr(msg, "sample (0, 0, 17)"));
        res[17] = -1.0;
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_EINVAL);
        res[17] = NAN;
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_EINVAL);
        res[17] = INFINITY;
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_EINVAL);
        res[17] = LF_MAX_SIGMA * K * 1.5 * 1.001;
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_EDOM && strstr(msg, "voxels wide") && strstr(msg, "sample (0, 0, 17)"));
        res[17] = LF_MAX_SIGMA * K * 1.5 * (1.0 - 1e-12);
        CHECK(plan(d, 1.5, res, rd, 3, P, msg) == LF_OK && P.H == LF_MAX_R);
        res[17] = 8.0;
        CHECK(plan(d, 1.5, res, rd, 0, P, msg) == LF_EINVAL && strstr(msg, "step 0"));
        CHECK(plan(d, 1.5, res, rd, -3, P, msg) == LF_EINVAL);
        CHECK(plan(d, 1.5, res, rd, 2, P, msg) == LF_EINVAL && strstr(msg, "rdims"));
        CHECK(plan(d, 0.0, res, rd, 3, P, msg) == LF_EINVAL && strstr(msg, "voxsp"));
        CHECK(plan(d, -1.0, res, rd, 3, P, msg) == LF_EINVAL);
        CHECK(plan(d, NAN, res, rd, 3, P, msg) == LF_EINVAL);
        CHECK(plan(d, INFINITY, res, rd, 3, P, msg) == LF_EINVAL);
        CHECK(plan(d, 1e308, res, rd, 3, P, msg) == LF_EINVAL);      // voxsp K overflows
        const int32_t d0[3] = {20, 0, 70}, big[3] = {2048, 1024, 1024}, edge[3] = {1, 1, 2147483647};
        CHECK(plan(d0, 1.5, res, rd, 3, P, msg) == LF_EINVAL && strstr(msg, "grid of 20 x 0 x 70"));
        CHECK(plan(big, 1.5, res, rd, 3, P, msg) == LF_EINVAL && strstr(msg, "2^31"));
        // the largest lattice along one axis: the tile count and the rounds stay in range (rdims refuses before the samples are read)
        CHECK(plan(edge, 1.5, res, rd, 3, P, msg) == LF_EINVAL && strstr(msg, "rdims"));
    }
    {   // step 1 on a one-voxel grid; a step beyond the grid
        const int32_t d[3] = {1, 1, 1}, rd[3] = {1, 1, 1};
        std::vector<double> res(1, 3.0);
        CHECK(plan(d, 1.5, res, rd, 1, P, msg) == LF_OK && P.n_tiles == 1 && P.H == 2);
        CHECK(plan(d, 1.5, res, rd, 1000, P, msg) == LF_OK);
        const int32_t d2[3] = {5, 7, 6}, rd2[3] = {1, 1, 1};
        CHECK(plan(d2, 1.5, res, rd2, 2147483647, P, msg) == LF_OK && P.m[0] == 1);
    }
    // radii at the knife edges of (int)(4 sigma + 0.5)
    CHECK(lf_radius(1e-9) == 1 && lf_radius(0.374) == 1 && lf_radius(0.376) == 2 && lf_radius(1.5) == 6 && lf_radius(1.50055) == 6);
    CHECK(lf_radius(LF_MAX_SIGMA) == LF_MAX_R && lf_radius(5.874) == 23 && lf_radius(5.876) == 24);
    // every halo, in the launch sized for it and in the launch sized for the widest
    for (int H = 1; H <= LF_MAX_R; H++) {
        replay_tile(H, lf_lds_bytes(H));
        replay_tile(H, LF_LDS_BYTES);
        for (int top = H; top <= LF_MAX_R; top += 5) replay_tile(H, lf_lds_bytes(top));
        CHECK(lf_lds_bytes(H) <= LF_LDS_BYTES && lf_lds_bytes(H) % 16 == 0);
    }
    CHECK(lf_slab(8, lf_lds_bytes(8)).n_slabs == 1 && lf_slab(9, lf_lds_bytes(9)).n_slabs == 1 && lf_slab(10, lf_lds_bytes(10)).n_slabs == 2);
    CHECK(lf_slab(24, LF_LDS_BYTES).planes == 8 && lf_slab(24, LF_LDS_BYTES).n_slabs == 7);
    if (failures) {
        fprintf(stderr, "check_localfilter_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("check_localfilter_plan: ok\n");
    return 0;
}
