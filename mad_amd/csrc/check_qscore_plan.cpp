// check_qscore_plan.cpp -- a stand-alone host program over mad_qscore_plan.h, the host side of mad_map_qscore, meant to be built with
// a host sanitizer (make -C mad_amd/csrc check-qscore-plan builds and runs it with AddressSanitizer and UBSan).  No device, no
// launch: the argument checks on heap buffers of exactly the sizes the contract names, the cell grid (atoms 10^6 A from the origin,
// an extent that hits the cell cap, every atom on one point), and the two culls replayed: for every atom, shell and candidate the
// decision taken from the atoms of the 27 cells that pass the shell's cut must be the decision taken from all atoms.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_qscore_plan.h"

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

// the sets 1 .. n_tries of a spiral over the sphere, normalised: exactly 4 n_tries (n_tries + 1) rows
static std::vector<double> make_dirs(int n_tries) {
    std::vector<double> d;
    for (int t = 1; t <= n_tries; t++) {
        const int n = QS_POINTS * t;
        double phi = 0.0;
        for (int k = 0; k < n; k++) {
            const double h = -1.0 + 2.0 * k / (n - 1.0), s = sqrt(fmax(1.0 - h * h, 0.0));
            phi = (k == 0 || k == n - 1) ? 0.0 : fmod(phi + 3.6 / sqrt(n * (1.0 - h * h)), 2.0 * M_PI);
            double v[3] = {s * cos(phi), s * sin(phi), h};
            const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int a = 0; a < 3; a++) d.push_back(v[a] / l);
        }
    }
    return d;
}

struct Call {
    int32_t dims[3] = {16, 16, 16};
    double origin[3] = {0.0, 0.0, 0.0}, voxsp = 1.0;
    std::vector<double> atoms, radii, ref, dirs;
    std::vector<int64_t> index;
    bool use_index = false;
    int n_tries = 4;
    bool plan(QsPlan &P, char *msg, size_t len) const {
        return qs_plan(dims, origin, voxsp, atoms.empty() ? nullptr : atoms.data(), (int64_t)(atoms.size() / 3), use_index ? index.data() : nullptr,
                       (int64_t)index.size(), radii.data(), ref.data(), (int32_t)radii.size(), dirs.data(), n_tries, P, msg, len);
    }
};

static Call base_call(int n_atoms, double box, double centre, int n_r = 21, int n_tries = 4) {
    Call c;
    c.n_tries = n_tries;
    for (int k = 0; k < n_r; k++) { c.radii.push_back(0.1 * k); c.ref.push_back(exp(-0.5 * (0.1 * k / 0.6) * (0.1 * k / 0.6))); }
    c.dirs = make_dirs(n_tries);
    for (int i = 0; i < 3 * n_atoms; i++) c.atoms.push_back(centre + box * uniform());
    return c;
}

static int cell_of(const QsPlan &P, const double *x, int c3[3]) {
    for (int a = 0; a < 3; a++) {
        c3[a] = qs_cell(x[a], P.glo[a], P.h, P.nc[a]);
        CHECK(c3[a] >= 0 && c3[a] < P.nc[a]);
    }
    return (c3[0] * P.nc[1] + c3[1]) * P.nc[2] + c3[2];
}

// the culls replayed -> candidates decided; every decision from the culled neighbours must equal the one from all atoms
static long replay(const Call &c, const QsPlan &P) {
    const int n = (int)(c.atoms.size() / 3);
    std::vector<int> cells(3 * (size_t)n);
    for (int i = 0; i < n; i++) CHECK(cell_of(P, &c.atoms[3 * (size_t)i], &cells[3 * (size_t)i]) < P.n_cells);
    long decided = 0;
    for (int i = 0; i < n; i++) {
        const double *x = &c.atoms[3 * (size_t)i];
        for (int k = 0; k < P.n_r; k++) {
            const double R = c.radii[k];
            if (R == 0.0) continue;
            std::vector<int> near;      // what the kernel tests: the 27 cells, the shell's cut
            for (int b = 0; b < n; b++) {
                if (b == i) continue;
                bool in27 = true;
                for (int a = 0; a < 3; a++) in27 = in27 && abs(cells[3 * (size_t)b + a] - cells[3 * (size_t)i + a]) <= 1;
                if (in27 && qs_d2(&c.atoms[3 * (size_t)b], x) <= P.cut[k]) near.push_back(b);
            }
            for (long long d = 0; d < P.n_dirs; d++) {
                const double p[3] = {x[0] + R * c.dirs[3 * d], x[1] + R * c.dirs[3 * d + 1], x[2] + R * c.dirs[3 * d + 2]};
                bool all = true, culled = true;
                for (int b = 0; b < n && all; b++)
                    if (b != i) all = qs_d2(p, &c.atoms[3 * (size_t)b]) > P.r2[k];
                for (size_t q = 0; q < near.size() && culled; q++) culled = qs_d2(p, &c.atoms[3 * (size_t)near[q]]) > P.r2[k];
                CHECK(all == culled);
                decided++;
            }
        }
    }
    return decided;
}

int main() {
    char msg[320];
    QsPlan P;
    {   // a good call
        Call c = base_call(50, 12.0, 2.0);
        CHECK(c.plan(P, msg, sizeof msg));
        CHECK(P.n_atoms == 50 && P.n_scored == 50 && P.n_r == 21 && P.n_tries == 4 && P.n_dirs == 80 && (long long)c.dirs.size() == 3 * P.n_dirs);
        CHECK(P.h >= 4.0 && P.h < 4.0001 && P.n_cells == P.nc[0] * P.nc[1] * P.nc[2] && P.nc[0] <= 4);
        CHECK(P.r2[20] == c.radii[20] * c.radii[20] && P.cut[20] > 16.0 && P.cut[20] < 16.0001 && P.cut[0] < 1e-18);
        c.use_index = true;
        c.index = {3, 3, 49, 0};
        CHECK(c.plan(P, msg, sizeof msg) && P.n_scored == 4);
        c.index.clear();
        CHECK(c.plan(P, msg, sizeof msg) && P.n_scored == 0);      // nothing to score: no refusal
        CHECK(qs_set_offset(1) == 0 && qs_set_offset(2) == 8 && qs_set_offset(50) == 9800 && qs_dirs_total(50) == 10200 && qs_dirs_total(64) == 16640);
    }
    {   // the refusals
        const Call good = base_call(20, 10.0, 0.0);
        Call c = good;
        CHECK(!qs_plan(nullptr, c.origin, 1.0, c.atoms.data(), 20, nullptr, 0, c.radii.data(), c.ref.data(), 21, c.dirs.data(), 4, P, msg, sizeof msg) && strstr(msg, "NULL"));
        CHECK(!qs_plan(c.dims, c.origin, 1.0, c.atoms.data(), 20, nullptr, 0, c.radii.data(), c.ref.data(), 21, nullptr, 4, P, msg, sizeof msg) && strstr(msg, "NULL"));
        CHECK(!qs_plan(c.dims, c.origin, 1.0, nullptr, 20, nullptr, 0, c.radii.data(), c.ref.data(), 21, c.dirs.data(), 4, P, msg, sizeof msg) && strstr(msg, "NULL atoms"));
        CHECK(qs_plan(c.dims, c.origin, 1.0, nullptr, 0, nullptr, 0, c.radii.data(), c.ref.data(), 21, c.dirs.data(), 4, P, msg, sizeof msg) && P.n_atoms == 0 && P.n_cells == 1);
        c.dims[1] = 0; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "16 x 0 x 16")); c = good;
        c.dims[0] = 2048; c.dims[1] = 2048; c.dims[2] = 1024; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "2^32")); c = good;
        c.dims[0] = 1; c.dims[1] = 1; c.dims[2] = 2147483647; CHECK(c.plan(P, msg, sizeof msg)); c = good;
        c.origin[2] = INFINITY; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "not finite")); c = good;
        c.voxsp = NAN; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "not finite")); c = good;
        c.voxsp = 0.0; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "voxsp")); c = good;
        c.voxsp = -1.0; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "voxsp")); c = good;
        c.atoms[31] = NAN; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "atom 10")); c = good;
        c.atoms[59] = -INFINITY; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "atom 19")); c = good;
        c.radii[5] = NAN; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "shell 5")); c = good;
        c.ref[20] = INFINITY; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "shell 20")); c = good;
        c.radii[0] = -0.05; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "negative")); c = good;
        c.radii[7] = c.radii[6]; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "ascend at shell 7")); c = good;
        c.radii[7] = 0.3; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "ascend")); c = good;
        c.dirs[3 * 17 + 1] = NAN; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "direction 17")); c = good;
        c.dirs[3 * 79] = 1.5; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "direction 79")); c = good;
        c.use_index = true;
        c.index = {0, 19, 20}; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "index[2] = 20"));
        c.index = {-1}; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "index[0] = -1"));
        c = good;
        for (int n_r : {0, -3, QS_MAX_R + 1})
            CHECK(!qs_plan(c.dims, c.origin, 1.0, c.atoms.data(), 20, nullptr, 0, c.radii.data(), c.ref.data(), n_r, c.dirs.data(), 4, P, msg, sizeof msg) && strstr(msg, "shells"));
        for (int n_t : {0, -1, QS_MAX_TRIES + 1})
            CHECK(!qs_plan(c.dims, c.origin, 1.0, c.atoms.data(), 20, nullptr, 0, c.radii.data(), c.ref.data(), 21, c.dirs.data(), n_t, P, msg, sizeof msg) && strstr(msg, "point sets"));
        CHECK(!qs_plan(c.dims, c.origin, 1.0, c.atoms.data(), 1ll << 31, nullptr, 0, c.radii.data(), c.ref.data(), 21, c.dirs.data(), 4, P, msg, sizeof msg) && strstr(msg, "2^31"));
        CHECK(!qs_plan(c.dims, c.origin, 1.0, c.atoms.data(), -1, nullptr, 0, c.radii.data(), c.ref.data(), 21, c.dirs.data(), 4, P, msg, sizeof msg));
        c.atoms[0] = 1.7e308; c.atoms[3] = -1.7e308; CHECK(!c.plan(P, msg, sizeof msg) && strstr(msg, "too large"));
    }
    {   // the limits of both table sizes, with buffers of exactly their lengths
        Call c = base_call(5, 6.0, 0.0, QS_MAX_R, QS_MAX_TRIES);
        for (int k = 0; k < QS_MAX_R; k++) c.radii[k] = 0.05 * k;
        CHECK(c.plan(P, msg, sizeof msg) && P.n_dirs == 16640 && P.n_r == 64);
        Call one = base_call(5, 6.0, 0.0, 1, 1);
        CHECK(one.plan(P, msg, sizeof msg) && P.n_dirs == 8 && P.cut[0] > 0.0 && P.h > 0.0);
    }
    {   // every atom on one point, and on the origin with no shell but R = 0
        Call c = base_call(6, 0.0, 3.25);
        CHECK(c.plan(P, msg, sizeof msg) && P.n_cells == 1 && P.h > 4.0);
        CHECK(replay(c, P) > 0);
        Call z = base_call(3, 0.0, 0.0, 1, 2);
        CHECK(z.plan(P, msg, sizeof msg) && P.n_cells == 1 && P.h == 1.0);
        int c3[3];
        CHECK(cell_of(P, z.atoms.data(), c3) == 0);
    }
    // the culls replayed: a crowded cloud in several cells; atoms 10^6 A from the origin; an extent that hits the cell cap (two crowded
    // clusters 2 000 A apart: h = extent / 64); a flat cloud (one cell along z)
    {
        Call c = base_call(150, 11.0, -3.0);
        CHECK(c.plan(P, msg, sizeof msg) && P.nc[0] >= 3 && P.nc[0] <= QS_MAXC);
        CHECK(replay(c, P) == 150l * 20 * 80);
        Call far = base_call(120, 10.0, 1.0e6);
        CHECK(far.plan(P, msg, sizeof msg) && P.h > 4.0009 && P.h < 4.002 && P.nc[0] >= 3 && P.glo[0] >= 1.0e6);
        CHECK(replay(far, P) > 0);
        Call wide = base_call(120, 7.0, 0.0);
        for (size_t i = 0; i < wide.atoms.size() / 2; i++) wide.atoms[i] += 2000.0;
        CHECK(wide.plan(P, msg, sizeof msg) && P.nc[0] == QS_MAXC && P.nc[1] == QS_MAXC && P.nc[2] == QS_MAXC && P.h > 31.0 && P.n_cells == QS_MAXC * QS_MAXC * QS_MAXC);
        CHECK(replay(wide, P) > 0);
        Call flat = base_call(100, 12.0, 5.0);
        for (size_t i = 2; i < flat.atoms.size(); i += 3) flat.atoms[i] = 7.0 + 0.3 * uniform();
        CHECK(flat.plan(P, msg, sizeof msg) && P.nc[2] == 1 && P.nc[0] >= 3);
        CHECK(replay(flat, P) > 0);
        // atoms exactly on cell borders, 2 R_max apart along x: the pair is within the cut and must share a neighbourhood
        Call edge = base_call(0, 0.0, 0.0);
        for (int i = 0; i < 12; i++) { edge.atoms.push_back(4.0 * i); edge.atoms.push_back(0.0); edge.atoms.push_back(0.0); }
        CHECK(edge.plan(P, msg, sizeof msg) && P.nc[0] >= 11);
        CHECK(replay(edge, P) > 0);
    }
    if (failures) {
        fprintf(stderr, "check_qscore_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("check_qscore_plan: ok\n");
    return 0;
}
