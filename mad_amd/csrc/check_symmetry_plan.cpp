// check_symmetry_plan.cpp -- a stand-alone host program over mad_symmetry_plan.h, the host side of mad_map_symmetry_score, meant to be
// built with a host sanitizer (make -C mad_amd/csrc check-symmetry-plan builds and runs it with AddressSanitizer and UBSan).  No
// device, no launch: the refusals; the box against a walk over every multiple of the stride; every point of every run inside the grid;
// the levels of the sums; and the kernels' record indices replayed on heap buffers of exactly the sizes the plan names, chunk by
// chunk, at budgets from one record to plenty.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_symmetry_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * 0x1p-53;
}

static char msg[256];

static bool plan(const int32_t *dims, const double *origin, double voxsp, const double *centre, double radius, int stride, int n_ops, int64_t budget,
                 SymPlan &P) {
    memset(&P, 0, sizeof(P));
    return sym_plan(dims, origin, voxsp, centre, radius, stride, n_ops, budget, P, msg, sizeof(msg));
}

static void refusals() {
    const int32_t d[3] = {8, 9, 10};
    const double o[3] = {1.0, 2.0, 3.0}, c[3] = {4.0, 5.0, 6.0};
    SymPlan P;
    CHECK(plan(d, o, 1.5, c, 3.0, 1, 1, 1 << 20, P));
    CHECK(!plan(nullptr, o, 1.5, c, 3.0, 1, 1, 1 << 20, P));
    CHECK(!plan(d, nullptr, 1.5, c, 3.0, 1, 1, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, nullptr, 3.0, 1, 1, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, c, 3.0, 1, 0, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, c, 3.0, 1, -3, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, c, 3.0, 0, 1, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, c, 3.0, -1, 1, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, c, -0.5, 1, 1, 1 << 20, P));
    CHECK(!plan(d, o, 0.0, c, 3.0, 1, 1, 1 << 20, P));
    CHECK(!plan(d, o, -1.0, c, 3.0, 1, 1, 1 << 20, P));
    CHECK(!plan(d, o, NAN, c, 3.0, 1, 1, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, c, INFINITY, 1, 1, 1 << 20, P));
    CHECK(!plan(d, o, 1.5, c, NAN, 1, 1, 1 << 20, P));
    for (int a = 0; a < 3; a++) {
        double bad[3] = {1.0, 2.0, 3.0};
        bad[a] = a == 1 ? NAN : INFINITY;
        CHECK(!plan(d, bad, 1.5, c, 3.0, 1, 1, 1 << 20, P));
        CHECK(!plan(d, o, 1.5, bad, 3.0, 1, 1, 1 << 20, P));
        int32_t thin[3] = {8, 9, 10};
        thin[a] = 1;
        CHECK(!plan(thin, o, 1.5, c, 3.0, 1, 1, 1 << 20, P));
        thin[a] = -4;
        CHECK(!plan(thin, o, 1.5, c, 3.0, 1, 1, 1 << 20, P));
    }
    const int32_t big[3] = {2048, 2048, 1024};      // 2^32 voxels
    CHECK(!plan(big, o, 1.5, c, 3.0, 1, 1, 1 << 20, P));
    const int32_t wide[3] = {65536, 65536, 2};      // the product of two axes alone is 2^32
    CHECK(!plan(wide, o, 1.5, c, 3.0, 1, 1, 1 << 20, P));
    const double far[3] = {1e308, -1e308, 0.0};     // finite, but the ball in voxels is not
    CHECK(!plan(d, o, 1e-3, far, 3.0, 1, 1, 1 << 20, P));
    const double away[3] = {1e200, 0.0, 0.0};       // finite in voxels: an empty box, no refusal
    CHECK(plan(d, o, 1.5, away, 3.0, 1, 4, 1 << 20, P) && P.box.n_box == 0 && P.n_chunks == 0 && P.box.n_runs == 0 && P.n_levels == 0);
}

// the box against a walk over every multiple of the stride, and every point of every run
static void boxes() {
    for (int trial = 0; trial < 400; trial++) {
        int32_t d[3];
        double o[3], c[3];
        for (int a = 0; a < 3; a++) {
            d[a] = 2 + (int)(uniform() * 20);
            o[a] = (uniform() - 0.5) * 40.0;
        }
        double vs = 0.5 + uniform() * 2.0;
        const int stride = 1 + (int)(uniform() * 4);
        for (int a = 0; a < 3; a++) c[a] = o[a] + vs * ((uniform() * 1.6 - 0.3) * d[a]);      // inside, on a face, outside
        double radius = trial % 7 == 0 ? 0.0 : uniform() * 14.0 * vs;
        if (trial % 11 == 0) {      // a centre on a lattice point (origin and spacing exact in binary), with radius 0 every 77th: one point
            vs = 1.5;
            for (int a = 0; a < 3; a++) {
                o[a] = floor(o[a]);
                c[a] = o[a] + vs * (double)(stride * ((d[a] - 1) / stride));
            }
        }
        SymPlan P;
        CHECK(plan(d, o, vs, c, radius, stride, 3, 1 << 20, P));
        const SymBox &B = P.box;
        long long in_box[3] = {0, 0, 0}, first[3] = {-1, -1, -1};
        for (int a = 0; a < 3; a++)
            for (long long k = 0; k * stride <= d[a] - 1; k++)
                if (fabs((double)(k * stride) - B.c[a]) <= P.r) {
                    if (first[a] < 0) first[a] = k;
                    in_box[a]++;
                }
        const bool empty = in_box[0] == 0 || in_box[1] == 0 || in_box[2] == 0;
        for (int a = 0; a < 3; a++) {
            CHECK(B.nb[a] == (empty ? 0 : in_box[a]));
            CHECK(empty || B.lo[a] == first[a]);
        }
        CHECK(B.n_box == (uint64_t)B.nb[0] * B.nb[1] * B.nb[2] && B.n_runs == (B.n_box + SYM_RUN - 1) / SYM_RUN);
        long long counted = 0, expect = 0;
        for (uint64_t i = 0; i < B.n_box; i++) {
            int32_t j[3];
            const bool in = sym_point(B, i, j);
            for (int a = 0; a < 3; a++) CHECK(j[a] >= 0 && j[a] < d[a] && j[a] % stride == 0);
            counted += in;
        }
        if (!empty)
            for (long long x = first[0]; x < first[0] + in_box[0]; x++)
                for (long long y = first[1]; y < first[1] + in_box[1]; y++)
                    for (long long z = first[2]; z < first[2] + in_box[2]; z++) {
                        const double dx = (double)(x * stride) - B.c[0], dy = (double)(y * stride) - B.c[1], dz = (double)(z * stride) - B.c[2];
                        expect += ((dx * dx + dy * dy) + dz * dz) <= P.r * P.r;
                    }
        CHECK(counted == expect);
        if (trial % 11 == 0) CHECK(radius > 0.0 || B.n_box == 1);
    }
}

// the kernels' record indices of every chunk on buffers of the plan's sizes
static void replay(const int32_t d[3], double radius, int stride, int n_ops, int64_t budget, bool walk) {
    const double o[3] = {0.0, 0.0, 0.0}, c[3] = {(d[0] - 1) / 2.0, (d[1] - 1) / 2.0, (d[2] - 1) / 2.0};
    SymPlan P;
    CHECK(plan(d, o, 1.0, c, radius, stride, n_ops, budget, P));
    const SymBox &B = P.box;
    if (B.n_box == 0) {      // nothing to launch
        CHECK(P.n_chunks == 0 && P.n_levels == 0 && B.n_runs == 0);
        return;
    }
    CHECK(P.ops_chunk >= 1 && P.ops_chunk <= n_ops);
    CHECK((long long)P.n_chunks * P.ops_chunk >= n_ops && (long long)(P.n_chunks - 1) * P.ops_chunk < n_ops);
    CHECK((P.ops_chunk + SYM_OPS_WG - 1) / SYM_OPS_WG <= SYM_MAX_BATCHES);
    CHECK(P.level_n[0] == B.n_runs && P.level_n[P.n_levels] == 1 && P.n_levels <= SYM_MAX_LEVELS);
    for (int l = 0; l < P.n_levels; l++) CHECK(P.level_n[l + 1] == (P.level_n[l] + SYM_RUN - 1) / SYM_RUN && P.level_n[l] > 1);
    const uint64_t per_slot = (P.rec_a + P.rec_b) * SYM_REC * sizeof(double);
    CHECK(P.scratch_bytes == (uint64_t)(P.ops_chunk + 1) * per_slot);
    CHECK(P.scratch_bytes <= (uint64_t)budget || P.ops_chunk == 1);      // one operator's records are the floor
    if (P.ops_chunk < n_ops && P.ops_chunk > SYM_OPS_WG) CHECK(P.ops_chunk % SYM_OPS_WG == 0);
    if (!walk) return;
    const size_t slots = (size_t)P.ops_chunk + 1;
    std::vector<double> A(slots * P.rec_a * SYM_REC), Bv(slots * P.rec_b * SYM_REC);
    double *buf[2] = {A.data(), Bv.data()};
    const size_t cap[2] = {A.size(), Bv.size()};
    for (int ch = 0; ch < P.n_chunks; ch++) {
        const int g0 = ch * P.ops_chunk, n = P.ops_chunk < n_ops - g0 ? P.ops_chunk : n_ops - g0;
        CHECK(n >= 1);
        const int batches = (n + SYM_OPS_WG - 1) / SYM_OPS_WG;
        for (uint32_t run = 0; run < B.n_runs; run++) {
            for (int by = 0; by < batches; by++)
                for (int k = 0; k < SYM_OPS_WG && by * SYM_OPS_WG + k < n; k++) {
                    const size_t at = ((size_t)(by * SYM_OPS_WG + k) * B.n_runs + run) * SYM_REC;
                    CHECK(at + SYM_REC <= cap[0]);
                    buf[0][at] = buf[0][at + 1] = buf[0][at + 2] = 1.0;
                }
            const size_t at = ((size_t)n * B.n_runs + run) * SYM_REC;      // the points' own slot
            CHECK(at + SYM_REC <= cap[0]);
            buf[0][at] = buf[0][at + 1] = buf[0][at + 2] = 1.0;
        }
        int cur = 0;
        for (int l = 0; l < P.n_levels; l++, cur ^= 1) {
            const uint32_t n_in = P.level_n[l], m = P.level_n[l + 1];
            for (int slot = 0; slot <= n; slot++)
                for (uint32_t b = 0; b < m; b++) {
                    double s = 0.0;
                    for (uint32_t t = 0; t < SYM_RUN; t++) {
                        const size_t i = (size_t)b * SYM_RUN + t;
                        if (i < n_in) {
                            const size_t at = ((size_t)slot * n_in + i) * SYM_REC;
                            CHECK(at + SYM_REC <= cap[cur]);
                            s += buf[cur][at];
                        }
                    }
                    const size_t at = ((size_t)slot * m + b) * SYM_REC;
                    CHECK(at + SYM_REC <= cap[cur ^ 1]);
                    buf[cur ^ 1][at] = buf[cur ^ 1][at + 1] = buf[cur ^ 1][at + 2] = s;
                }
        }
        for (int slot = 0; slot <= n; slot++) CHECK(buf[cur][(size_t)slot * SYM_REC] == (double)B.n_runs);      // every run was counted once
    }
}

int main() {
    refusals();
    boxes();
    const int32_t small[3] = {13, 10, 7}, odd[3] = {13, 11, 7}, mid[3] = {70, 66, 61}, large[3] = {2048, 2048, 1023};
    for (int64_t budget : {(int64_t)1, (int64_t)24, (int64_t)1000, (int64_t)100000, (int64_t)1 << 26})
        for (int n_ops : {1, 2, SYM_OPS_WG, SYM_OPS_WG + 1, 61, 700}) {
            replay(small, 6.0, 1, n_ops, budget, true);
            replay(small, 6.0, 3, n_ops, budget, true);
            replay(small, 0.0, 1, n_ops, budget, true);      // the centre (6, 4.5, 3) is off the lattice: empty
            replay(odd, 0.0, 1, n_ops, budget, true);        // (6, 5, 3): one point
            replay(mid, 40.0, 1, n_ops, budget, n_ops <= 61);      // 1101 runs: two levels
        }
    replay(large, 4000.0, 1, 1 << 24, (int64_t)1 << 26, false);      // every voxel of the largest grid: three levels, sizes only
    replay(large, 4000.0, 1, 2000000, (int64_t)1 << 40, false);      // more operators than gridDim.y takes in one chunk
    SymPlan P;
    const double o[3] = {0, 0, 0}, c[3] = {1000, 1000, 500};
    CHECK(plan(large, o, 1.0, c, 4000.0, 1, 1, 1, P) && P.box.n_box == 2048ull * 2048ull * 1023ull && P.n_levels == 3 && P.ops_chunk == 1);
    if (failures) {
        fprintf(stderr, "check_symmetry_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("check_symmetry_plan: ok\n");
    return 0;
}
