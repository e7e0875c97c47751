// check_jointfit_plan.cpp -- a stand-alone host program over mad_jointfit_plan.h, the host side of mad_assembly_density and
// mad_assembly_refine, meant to be built with a host sanitizer (make -C mad_amd/csrc check-jointfit-plan builds and runs it with
// AddressSanitizer and UBSan).  No device, no launch: the argument checks on heap buffers of exactly the sizes the contract names,
// the taps, the round count, the workgroups per body, and the property the kernels rest on: wherever a body stands and however it
// moves within a round, every lattice voxel its model reaches and every cell its atoms gather from lies inside its box, or
// outside the map.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_jointfit_plan.h"

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

struct Call {
    int32_t dims[3] = {24, 20, 28};
    double origin[3] = {4.0, -9.0, 2.5}, vs = 1.5;
    std::vector<double> atoms, mass;
    std::vector<int64_t> first = {0};
    double resolution = 6.0;
    int32_t n_steps = 500;
    double max_step = 0.5, min_step = 0.01;
    void body(int n, double cx, double cy, double cz, double radius) {
        for (int i = 0; i < n; i++) {
            atoms.push_back(cx + radius * (2 * uniform() - 1)); atoms.push_back(cy + radius * (2 * uniform() - 1));
            atoms.push_back(cz + radius * (2 * uniform() - 1)); mass.push_back(12.0 + 20.0 * uniform());
        }
        first.push_back((int64_t)mass.size());
    }
    bool plan(JfPlan &P, char *msg, size_t len, bool refine = true, bool with_map = true) const {
        // heap copies of exactly the contract's sizes, so that a read past one is seen
        std::vector<double> a(atoms), m(mass);
        std::vector<int64_t> f(first);
        return jf_plan("check", with_map ? dims : nullptr, origin, vs, (int32_t)f.size() - 1, a.empty() ? nullptr : a.data(), m.empty() ? nullptr : m.data(),
                       f.data(), resolution, refine, n_steps, max_step, min_step, P, msg, len);
    }
};

static Call base_call() {
    Call c;
    c.body(1, 22.0, 6.0, 23.5, 0.0);
    c.body(63, 6.5, 5.0, 14.0, 3.0);
    c.body(130, 20.0, 4.0, 25.0, 5.0);
    return c;
}

static bool refused(const Call &c, const char *word, bool refine = true, bool with_map = true) {
    static JfPlan P;
    char msg[256] = "";
    const bool ok = c.plan(P, msg, sizeof msg, refine, with_map);
    if (ok || !strstr(msg, word)) fprintf(stderr, "  wanted a refusal naming '%s', got %s '%s'\n", word, ok ? "a plan," : "", msg);
    return !ok && strstr(msg, word) != nullptr;
}

int main() {
    static JfPlan P;
    char msg[256];

    // rounds and their steps
    CHECK(jf_rounds(1) == 1 && jf_rounds(4) == 1 && jf_rounds(5) == 2 && jf_rounds(500) == 125 && jf_rounds(2147483647) == 536870912);
    for (int n = 1; n <= 13; n++) {
        int total = 0;
        for (int r = 0; r < jf_rounds(n); r++) { const int s = jf_round_steps(n, r); CHECK(s >= 1 && s <= JF_BATCH); total += s; }
        CHECK(total == n && jf_round_steps(n, jf_rounds(n)) == 0);
    }

    // taps: 6 A at 1.5 A is r = 3; they add up to 1, are symmetric and fall from the centre; the bounds of r
    {
        double taps[2 * JF_MAX_R + 1], sig;
        int32_t r;
        CHECK(jf_taps(6.0, 1.5, &r, &sig, taps) && r == 3);
        double sum = 0;
        for (int t = 0; t <= 2 * r; t++) { sum += taps[t]; CHECK(taps[t] == taps[2 * r - t]); if (t < r) CHECK(taps[t] < taps[t + 1]); }
        CHECK(fabs(sum - 1.0) < 1e-15);
        CHECK(jf_taps(1e-9, 1.5, &r, &sig, taps) && r == 1 && taps[1] == 1.0 && taps[0] == 0.0);
        CHECK(jf_taps(64.0 * M_PI * sqrt(2.0) / 3.0 * 0.999, 1.0, &r, &sig, taps) && r == 64);
        CHECK(!jf_taps(64.0 * M_PI * sqrt(2.0) / 3.0 * 1.02, 1.0, &r, &sig, taps));
        CHECK(!jf_taps(NAN, 1.0, &r, &sig, taps) && !jf_taps(INFINITY, 1.0, &r, &sig, taps));
    }

    // workgroups per body: mad_refine's rule
    CHECK(jf_groups(256, 1, 4097, 8) == 2 && jf_groups(256, 1, 4095, 8) == 1 && jf_groups(256, 1, 26000, 8) == 8 && jf_groups(256, 64, 26000, 8) == 4);
    CHECK(jf_groups(256, 4, 26000, 8) == 8 && jf_groups(256, 1, 4097, 1) == 1 && jf_groups(8, 64, 100000, 8) == 1);
    CHECK(jf_fits_registers(4096, 1) && !jf_fits_registers(4097, 1) && jf_fits_registers(4097, 2) && jf_fits_registers(26000, 8));
    for (int B = 1; B <= JF_MAX_BODIES; B++) CHECK(B * jf_groups(256, B, 1 << 20, 8) <= 256);      // all workgroups resident at one per compute unit
    // ... and with bodies of mixed sizes, as jf_setup adds them up: every B, every cap, sizes of 30, 4097 and 2^20 atoms in turn from
    // every starting size, in runs of 1 to 3 bodies, and drawn at random.  A body's G never exceeds that of the largest size.
    {
        const int64_t sizes[3] = {30, 4097, 1 << 20};
        for (int B = 1; B <= JF_MAX_BODIES; B++)
            for (int cap = 1; cap <= 8; cap++) {
                const int32_t g_max = jf_groups(256, B, sizes[2], cap);
                CHECK(jf_groups(256, B, sizes[0], cap) == 1 && jf_groups(256, B, sizes[1], cap) == (cap >= 2 ? 2 : 1) && g_max <= cap);
                for (int pattern = 0; pattern < 12; pattern++) {
                    int total = 0;
                    bool mixed[3] = {false, false, false};
                    for (int b = 0; b < B; b++) {
                        const int pick = pattern < 9 ? (b / (1 + pattern / 3) + pattern % 3) % 3 : (int)(uniform() * 3.0);
                        const int32_t G = jf_groups(256, B, sizes[pick], cap);
                        CHECK(G >= 1 && G <= g_max && G <= JF_MAX_G);
                        total += G;
                        mixed[pick] = true;
                    }
                    CHECK(total <= 256 && total >= B);
                    if (B >= 9 && pattern < 9) CHECK(mixed[0] && mixed[1] && mixed[2]);
                }
            }
    }

    // the plan of three bodies
    {
        Call c = base_call();
        CHECK(c.plan(P, msg, sizeof msg));
        CHECK(P.n_bodies == 3 && P.n_atoms == 194 && P.r == 3 && P.max_atoms == 130 && P.max_dist[0] == 0.0);
        CHECK(P.edge[0] == 13);      // ceil(2 (0 + 3 x 1.5 + 4 x 0.5) / 1.5 + 4)
        CHECK(c.plan(P, msg, sizeof msg, false) && P.edge[0] == 10);      // mad_assembly_density: the bodies do not move
        int64_t sum = 0;
        for (int b = 0; b < 3; b++) {
            CHECK(P.vox0[b] == sum);
            int64_t v = 1;
            for (int d = 0; d < 3; d++) { v *= P.e[b][d]; CHECK(P.lo[b][d] >= 0 && P.lo[b][d] + P.e[b][d] <= c.dims[d] && P.e[b][d] <= P.edge[b]); }
            sum += v;
            CHECK(v <= P.max_box);
        }
        CHECK(P.vox0[3] == sum);
    }

    // refusals, each naming its argument
    {
        Call c = base_call();
        CHECK(refused(c, "mad_upload_density", true, false));
        c = base_call(); c.first = {0}; CHECK(refused(c, "n_bodies"));
        c = base_call(); for (int b = 0; b < 64; b++) c.body(1, 10, 0, 10, 0); CHECK(refused(c, "n_bodies"));
        c = base_call(); c.first.push_back(c.first.back()); CHECK(refused(c, "empty"));
        c = base_call(); c.first[0] = 1; CHECK(refused(c, "first_atom"));
        c = base_call(); c.atoms[7] = NAN; CHECK(refused(c, "atoms"));
        c = base_call(); c.atoms[7] = INFINITY; CHECK(refused(c, "atoms"));
        c = base_call(); c.atoms[7] = 1e13; CHECK(refused(c, "atoms"));
        c = base_call(); c.mass[5] = NAN; CHECK(refused(c, "mass"));
        c = base_call(); c.resolution = 0; CHECK(refused(c, "resolution"));
        c = base_call(); c.resolution = -1; CHECK(refused(c, "resolution"));
        c = base_call(); c.resolution = NAN; CHECK(refused(c, "resolution"));
        c = base_call(); c.resolution = 1e4; CHECK(refused(c, "resolution"));
        c = base_call(); c.n_steps = 0; CHECK(refused(c, "n_steps"));
        c = base_call(); c.min_step = 0; CHECK(refused(c, "min_step"));
        c = base_call(); c.min_step = 0.6; CHECK(refused(c, "min_step"));
        c = base_call(); c.max_step = NAN; CHECK(refused(c, "max_step"));
        c = base_call(); c.min_step = NAN; CHECK(refused(c, "min_step"));
        c = base_call(); c.n_steps = 0; c.min_step = 7; CHECK(c.plan(P, msg, sizeof msg, false));      // the step arguments are the refinement's
        c = base_call(); c.atoms.clear(); c.mass.clear(); CHECK(refused(c, "atoms"));
        c = base_call(); c.body(3, 1e9, 0, 0, 1e8); CHECK(refused(c, "atoms"));      // a body no box holds
    }

    // placement: inside the map, centred when the map has room, a face of the map for centres far away and for NaN
    {
        CHECK(jf_box_extent(13, 24) == 13 && jf_box_extent(40, 24) == 24);
        CHECK(jf_box_lo(4.0 + 1.5 * 12, 4.0, 1.5, 13, 24) == 6 && jf_box_lo(4.0 + 1.5 * 12.49, 4.0, 1.5, 13, 24) == 6 && jf_box_lo(4.0 + 1.5 * 12.5, 4.0, 1.5, 13, 24) == 7);
        CHECK(jf_box_lo(-1e300, 4.0, 1.5, 13, 24) == 0 && jf_box_lo(1e300, 4.0, 1.5, 13, 24) == 11 && jf_box_lo(NAN, 4.0, 1.5, 13, 24) == 0);
        CHECK(jf_box_lo(INFINITY, 4.0, 1.5, 13, 24) == 11 && jf_box_lo(-INFINITY, 4.0, 1.5, 13, 24) == 0 && jf_box_lo(20.0, 4.0, 1.5, 40, 24) == 0);
    }

    // The property: a body of farthest atom max_dist around a centre c0; its box is placed from c0.  Within a round the centre moves
    // by at most 2 max_step and an atom by at most 4 max_step.  Every atom position p within max_dist of a centre within 2 max_step
    // of c0 whose cell is a cell of the map (0 .. n - 2) has that cell and the next voxel inside the box, with r more voxels on
    // either side for the blur unless the map ends there.
    for (int trial = 0; trial < 20000; trial++) {
        const int32_t n = 8 + (int32_t)(uniform() * 120);
        const double vs = 0.5 + 3.0 * uniform(), o = -50.0 + 100.0 * uniform(), max_step = 0.01 + 2.0 * uniform();
        const double max_dist = uniform() < 0.1 ? 0.0 : 40.0 * uniform();
        const int32_t r = (int32_t)(uniform() * 9);
        const int32_t edge = jf_box_edge(max_dist, r, vs, max_step);
        CHECK(edge >= 4);
        const double c0 = o + vs * n * (-0.5 + 2.0 * uniform());
        const int32_t lo = jf_box_lo(c0, o, vs, edge, n), e = jf_box_extent(edge, n);
        CHECK(lo >= 0 && lo + e <= n);
        for (int k = 0; k < 8; k++) {
            const double c = c0 + 2.0 * max_step * (2 * uniform() - 1);
            const double p = c + (max_dist + 2.0 * max_step) * (k == 0 ? 1.0 : k == 1 ? -1.0 : 2 * uniform() - 1);
            const double g = (p - o) / vs;
            if (!(g >= 0.0) || !(g < (double)(n - 1))) continue;
            const int32_t i0 = (int32_t)floor(g);
            CHECK(i0 - lo >= 0 && i0 + 1 - lo < e);
            CHECK(i0 - r >= lo || lo == 0);
            CHECK(i0 + 1 + r < lo + e || lo + e == n);
        }
    }
    CHECK(jf_box_edge(1e9, 3, 1.0, 0.5) == -1 && jf_box_edge(NAN, 3, 1.0, 0.5) == -1 && jf_box_edge(0.0, 0, 1.0, 0.0) == 4);

    // ---- units under operators (mad_assembly_refine_symmetric) ----
    // the operators: the quarter turn about z through (10, 2, 0) and its powers, on heap buffers of exactly n_ops x 9 and n_ops x 3
    {
        const double c[3] = {10.0, 2.0, 0.0};
        std::vector<double> rot, tr;
        for (int g = 0; g < 4; g++) {
            const double co[4] = {1, 0, -1, 0}, si[4] = {0, 1, 0, -1};
            const double R[9] = {co[g], si[g], 0, -si[g], co[g], 0, 0, 0, 1};      // row vectors: x -> x R
            rot.insert(rot.end(), R, R + 9);
            for (int j = 0; j < 3; j++) tr.push_back(g == 0 ? 0.0 : c[j] - ((c[0] * R[j] + c[1] * R[3 + j]) + c[2] * R[6 + j]));
        }
        auto ops_refused = [&](int32_t U, int32_t K, const std::vector<double> &r, const std::vector<double> &t, const char *word) {
            std::vector<double> rr(r), tt(t);      // exact sizes
            char m[256] = "";
            const bool ok = jf_ops_check("check", U, K, rr.empty() ? nullptr : rr.data(), tt.empty() ? nullptr : tt.data(), m, sizeof m);
            if (ok || !strstr(m, word)) fprintf(stderr, "  wanted a refusal naming '%s', got %s '%s'\n", word, ok ? "a pass," : "", m);
            return !ok && strstr(m, word) != nullptr;
        };
        CHECK(jf_ops_check("check", 16, 4, rot.data(), tr.data(), msg, sizeof msg));
        CHECK(jf_ops_check("check", 64, 1, rot.data(), tr.data(), msg, sizeof msg));
        CHECK(ops_refused(17, 4, rot, tr, "n_units x n_ops = 68"));
        CHECK(ops_refused(0, 4, rot, tr, "n_units") && ops_refused(65, 1, rot, tr, "n_units"));
        CHECK(ops_refused(1, 0, rot, tr, "n_ops") && ops_refused(1, 65, rot, tr, "n_ops") && ops_refused(1, -1, rot, tr, "n_ops"));
        CHECK(ops_refused(1, 4, {}, tr, "op_rot") && ops_refused(1, 4, rot, {}, "op_trans"));
        std::vector<double> r2(rot), t2(tr);
        r2[0] = 1.0 + 1e-15; CHECK(ops_refused(1, 4, r2, tr, "identity"));
        r2 = rot; r2[1] = 1e-300; CHECK(ops_refused(1, 4, r2, tr, "identity"));
        t2[2] = -1e-300; CHECK(ops_refused(1, 4, rot, t2, "identity"));
        r2 = rot; std::swap_ranges(r2.begin(), r2.begin() + 9, r2.begin() + 9); CHECK(ops_refused(1, 4, r2, tr, "identity"));
        r2 = rot; for (int i = 0; i < 9; i++) r2[9 + i] *= 1.0 + 1e-6; CHECK(ops_refused(1, 4, r2, tr, "orthonormal"));      // R R^T - I = 2e-6
        r2 = rot; for (int i = 0; i < 9; i++) r2[9 + i] *= 1.0 + 1e-7; CHECK(jf_ops_check("check", 1, 4, r2.data(), tr.data(), msg, sizeof msg));
        r2 = rot; r2[18 + 5] = 2e-6; CHECK(ops_refused(1, 4, r2, tr, "operator 2 is not orthonormal"));      // a shear
        r2 = rot; r2[27 + 8] = -1.0; CHECK(ops_refused(1, 4, r2, tr, "operator 3 is a reflection"));
        r2 = rot; r2[9 + 4] = NAN; CHECK(ops_refused(1, 4, r2, tr, "op_rot"));
        t2 = tr; t2[4] = INFINITY; CHECK(ops_refused(1, 4, rot, t2, "op_trans"));
        t2 = tr; t2[4] = 1e13; CHECK(ops_refused(1, 4, rot, t2, "op_trans"));
        // image and pull-back: a point and its images keep their distance to the centre; h = g R^T undoes x R on a vector
        const double p[3] = {13.0, 3.0, 5.0};
        for (int g = 1; g < 4; g++) {
            double q[3], h[3], back[3];
            jf_image(&rot[9 * g], &tr[3 * g], p, q);
            CHECK(fabs(hypot(q[0] - c[0], q[1] - c[1]) - hypot(3.0, 1.0)) < 1e-12 && q[2] == 5.0);
            const double zero[3] = {0, 0, 0}, v[3] = {0.3, -1.1, 2.0};
            jf_image(&rot[9 * g], zero, v, h);
            jf_pull_back(&rot[9 * g], h, back);
            CHECK(fabs(back[0] - v[0]) < 1e-15 && fabs(back[1] - v[1]) < 1e-15 && back[2] == v[2]);
        }
        double q4[3];
        jf_image(&rot[9], &tr[3], p, q4);
        CHECK(q4[0] == 10.0 - 1.0 && q4[1] == 2.0 + 3.0);      // (3, 1) about the centre turns to (-1, 3)

        // the plan of the images: two units under the four operators in the map of base_call
        Call cl;
        cl.body(40, 24.0, 6.0, 20.0, 3.0);
        cl.body(7, 18.0, -2.0, 30.0, 2.0);
        std::vector<double> a(cl.atoms), ms(cl.mass);
        std::vector<int64_t> f(cl.first);
        static JfPlan U;
        CHECK(jf_plan("check", cl.dims, cl.origin, cl.vs, 2, a.data(), ms.data(), f.data(), 6.0, true, 500, 0.5, 0.01, U, msg, sizeof msg));
        CHECK(jf_plan_sym("check", cl.dims, cl.origin, cl.vs, 2, a.data(), ms.data(), f.data(), 4, rot.data(), tr.data(), 6.0, 500, 0.5, 0.01, P, msg, sizeof msg));
        CHECK(P.n_bodies == 8 && P.n_atoms == 4 * 47 && P.max_atoms == 40 && P.r == U.r && P.max_box == U.max_box);
        int64_t sum = 0;
        for (int b = 0; b < 8; b++) {
            const int u = b / 4, g = b % 4;
            CHECK(P.edge[b] == U.edge[u] && P.max_dist[b] == U.max_dist[u] && P.vox0[b] == sum);
            double q[3];
            jf_image(&rot[9 * g], &tr[3 * g], U.cen[u], q);
            int64_t v = 1;
            for (int d = 0; d < 3; d++) {
                CHECK(g == 0 ? P.cen[b][d] == U.cen[u][d] : P.cen[b][d] == q[d]);
                CHECK(P.e[b][d] == U.e[u][d] && P.lo[b][d] == jf_box_lo(P.cen[b][d], cl.origin[d], cl.vs, P.edge[b], cl.dims[d]));
                CHECK(P.lo[b][d] >= 0 && P.lo[b][d] + P.e[b][d] <= cl.dims[d]);
                if (g == 0) CHECK(P.lo[b][d] == U.lo[u][d]);
                v *= P.e[b][d];
            }
            sum += v;
        }
        CHECK(P.vox0[8] == sum);
        // the refusals of the units are jf_plan's, those of the operators come first, no map before either
        char m2[256];
        CHECK(!jf_plan_sym("check", nullptr, cl.origin, cl.vs, 2, a.data(), ms.data(), f.data(), 0, nullptr, nullptr, 6.0, 500, 0.5, 0.01, P, m2, sizeof m2) && strstr(m2, "mad_upload_density"));
        CHECK(!jf_plan_sym("check", cl.dims, cl.origin, cl.vs, 2, nullptr, ms.data(), f.data(), 0, rot.data(), tr.data(), 6.0, 500, 0.5, 0.01, P, m2, sizeof m2) && strstr(m2, "n_ops"));
        CHECK(!jf_plan_sym("check", cl.dims, cl.origin, cl.vs, 2, nullptr, ms.data(), f.data(), 4, rot.data(), tr.data(), 6.0, 500, 0.5, 0.01, P, m2, sizeof m2) && strstr(m2, "atoms"));
        CHECK(!jf_plan_sym("check", cl.dims, cl.origin, cl.vs, 2, a.data(), ms.data(), f.data(), 4, rot.data(), tr.data(), 6.0, 0, 0.5, 0.01, P, m2, sizeof m2) && strstr(m2, "n_steps"));
        a[5] = NAN;
        CHECK(!jf_plan_sym("check", cl.dims, cl.origin, cl.vs, 2, a.data(), ms.data(), f.data(), 4, rot.data(), tr.data(), 6.0, 500, 0.5, 0.01, P, m2, sizeof m2) && strstr(m2, "atoms"));
        // 64 images: the last body's entries are the arrays' last
        Call one;
        one.body(5, 20.0, 4.0, 25.0, 1.0);
        std::vector<double> r64, t64;
        for (int g = 0; g < 64; g++) { r64.insert(r64.end(), rot.begin() + 9 * (g % 4), rot.begin() + 9 * (g % 4) + 9); t64.insert(t64.end(), tr.begin() + 3 * (g % 4), tr.begin() + 3 * (g % 4) + 3); }
        CHECK(jf_plan_sym("check", one.dims, one.origin, one.vs, 1, one.atoms.data(), one.mass.data(), one.first.data(), 64, r64.data(), t64.data(), 6.0, 500, 0.5, 0.01, P, m2, sizeof m2));
        CHECK(P.n_bodies == 64 && P.n_atoms == 320 && P.vox0[64] == 64 * P.vox0[1] && P.edge[63] == P.edge[0]);
    }
    // residency: the image count in the place of the body count.  Every U x K <= 64, every cap, units of 30, 4097 and 2^20 atoms: all
    // images' workgroups are at most the compute units, and a unit's reduction group is at most JF_SYM_MAX_MEMBERS
    for (int U = 1; U <= JF_MAX_BODIES; U++)
        for (int K = 1; U * K <= JF_MAX_BODIES; K++)
            for (int cap = 1; cap <= 8; cap++) {
                const int64_t sizes[3] = {30, 4097, 1 << 20};
                int total = 0;
                for (int u = 0; u < U; u++) {
                    const int32_t G = jf_groups(256, U * K, sizes[(u + cap) % 3], cap);
                    CHECK(G >= 1 && K * G <= JF_SYM_MAX_MEMBERS && K * G <= 256 / U);
                    total += K * G;
                }
                CHECK(total <= 256 && total >= U * K);
            }
    CHECK(jf_groups(256, 2, 4100, 8) == 2 && jf_groups(256, 60, 30, 8) == 1 && jf_groups(256, 4, 26000, 8) == 8 && jf_groups(256, 60, 1 << 20, 8) == 4);

    if (failures) {
        fprintf(stderr, "check_jointfit_plan: %d check(s) failed\n", failures);
        return 1;
    }
    printf("check_jointfit_plan: ok\n");
    return 0;
}
