// check_flexfit_plan.cpp -- a stand-alone host program over mad_flexfit_plan.h, the host side of mad_flex_network and mad_flex_fit,
// meant to be built with a host sanitizer (make -C mad_amd/csrc check-flexfit-plan builds and runs it with AddressSanitizer and
// UBSan).  No device, no launch: the argument checks on heap buffers of exactly the sizes the contract names, the cell grid over
// degenerate boxes, the property the network kernels rest on (every pair within the cutoff lies in the same or in touching cells),
// the check of a caller's network, and the workgroups of the persistent launch, never more than the compute units.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_flexfit_plan.h"

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

static bool net_args(const std::vector<double> &x, double cutoff, FxGrid &g, const char *word = nullptr) {
    std::vector<double> copy(x);      // a heap copy of exactly n x 3 doubles, so that a read past it is seen
    const bool ok = fx_check_network_args("check", (int64_t)(copy.size() / 3), copy.empty() ? nullptr : copy.data(), cutoff, g, msg, sizeof msg);
    if (!ok && word && !strstr(msg, word)) { fprintf(stderr, "message '%s' lacks '%s'\n", msg, word); failures++; }
    return ok;
}

// every pair within the cutoff in the same or in touching cells; every cell index inside the grid
static void check_pairs(const std::vector<double> &x, double cutoff) {
    FxGrid g;
    CHECK(net_args(x, cutoff, g));
    const int64_t n = (int64_t)(x.size() / 3);
    CHECK(g.cells == (int64_t)g.dim[0] * g.dim[1] * g.dim[2] && g.cells >= 1 && (double)g.cells <= 4.0 * (double)n + 64.0);
    CHECK(g.edge > cutoff);
    std::vector<int32_t> c(x.size());
    for (int64_t i = 0; i < n; i++)
        for (int d = 0; d < 3; d++) {
            c[3 * i + d] = fx_cell_of(x[3 * i + d], g.lo[d], g.edge, g.dim[d]);
            CHECK(c[3 * i + d] >= 0 && c[3 * i + d] < g.dim[d]);
        }
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = i + 1; j < n; j++) {
            const double dx = x[3 * j] - x[3 * i], dy = x[3 * j + 1] - x[3 * i + 1], dz = x[3 * j + 2] - x[3 * i + 2];
            if ((dx * dx + dy * dy) + dz * dz <= cutoff * cutoff)
                for (int d = 0; d < 3; d++) CHECK(abs(c[3 * i + d] - c[3 * j + d]) <= 1);
        }
}

struct Net {
    std::vector<int32_t> first, nbr;
    std::vector<double> rest;
    bool ok(int64_t n, const char *word = nullptr) const {
        std::vector<int32_t> f(first), b(nbr);
        std::vector<double> r(rest);
        const bool good = fx_check_network("check", n, f.data(), b.empty() ? nullptr : b.data(), r.empty() ? nullptr : r.data(), msg, sizeof msg);
        if (!good && word && !strstr(msg, word)) { fprintf(stderr, "message '%s' lacks '%s'\n", msg, word); failures++; }
        return good;
    }
};

int main() {
    FxGrid g;
    // -- arguments of the network
    std::vector<double> one = {1.5, -2.0, 3.0};
    CHECK(net_args(one, 6.0, g) && g.dim[0] == 1 && g.dim[1] == 1 && g.dim[2] == 1 && g.cells == 1);
    CHECK(fx_cell_of(1.5, g.lo[0], g.edge, 1) == 0);
    CHECK(!net_args({}, 6.0, g, "n_atoms"));
    CHECK(!fx_check_network_args("check", 4, nullptr, 6.0, g, msg, sizeof msg) && strstr(msg, "NULL coords"));
    CHECK(!fx_check_network_args("check", (int64_t)FX_MAX_ATOMS + 1, one.data(), 6.0, g, msg, sizeof msg) && strstr(msg, "n_atoms"));
    CHECK(!net_args(one, 0.0, g, "cutoff") && !net_args(one, -1.0, g, "cutoff") && !net_args(one, NAN, g, "cutoff") && !net_args(one, INFINITY, g, "cutoff"));
    CHECK(!net_args({0.0, NAN, 0.0}, 6.0, g, "atom 0") && !net_args({0.0, 0.0, 0.0, INFINITY, 0.0, 0.0}, 6.0, g, "atom 1") && !net_args({1e13, 0.0, 0.0}, 6.0, g, "coords"));

    // -- the grid over degenerate boxes
    std::vector<double> plane, line, same;
    for (int i = 0; i < 200; i++) { plane.push_back(40.0 * uniform() - 20.0); plane.push_back(40.0 * uniform() - 20.0); plane.push_back(4.25); }
    for (int i = 0; i < 100; i++) { line.push_back(-7.0); line.push_back(0.5 * i); line.push_back(1e3); }
    for (int i = 0; i < 10; i++) { same.push_back(3.0); same.push_back(3.0); same.push_back(3.0); }
    CHECK(net_args(plane, 5.0, g) && g.dim[2] == 1 && g.dim[0] >= 7 && g.dim[1] >= 7);
    CHECK(net_args(line, 6.0, g) && g.dim[0] == 1 && g.dim[2] == 1 && g.dim[1] == 9);
    CHECK(net_args(same, 6.0, g) && g.cells == 1);
    check_pairs(plane, 5.0);
    check_pairs(line, 6.0);
    check_pairs(same, 6.0);
    // atoms exactly on the faces of cells of edge `cutoff`, pairs at exactly the cutoff
    std::vector<double> faces;
    for (int a = 0; a < 5; a++) for (int b = 0; b < 5; b++) for (int c = 0; c < 5; c++) { faces.push_back(-12.0 + 3.0 * a); faces.push_back(-12.0 + 3.0 * b); faces.push_back(-12.0 + 3.0 * c); }
    check_pairs(faces, 6.0);
    CHECK(net_args(faces, 6.0, g) && g.dim[0] == 2 && g.dim[1] == 2 && g.dim[2] == 2);
    // random clouds, negative coordinates, cutoffs that do not divide the box
    for (int t = 0; t < 20; t++) {
        std::vector<double> cloud;
        const int n = 1 + (int)(300 * uniform());
        const double span = 1.0 + 60.0 * uniform(), cutoff = 0.5 + 9.0 * uniform();
        for (int i = 0; i < 3 * n; i++) cloud.push_back(span * (uniform() - 0.7));
        check_pairs(cloud, cutoff);
    }
    // two atoms a long way apart: the edge doubles until the cells fit 4 n + 64 and 2^20 per axis
    std::vector<double> far = {0.0, 0.0, 0.0, 9e11, -9e11, 5e5};
    CHECK(net_args(far, 1.0, g) && g.cells <= 72 && g.dim[0] <= FX_MAX_DIM && g.edge > 1.0);
    check_pairs(far, 1.0);
    std::vector<double> near_far = {0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 1e6, 0.0, 0.0};
    check_pairs(near_far, 1.0);

    // -- a caller's network
    Net ok4;      // 4 atoms: rows {1, 3}, {0}, {}, {0}
    ok4.first = {0, 2, 3, 3, 4}; ok4.nbr = {1, 3, 0, 0}; ok4.rest = {1.5, 2.0, 1.5, 2.0};
    CHECK(ok4.ok(4));
    Net none;
    none.first = {0, 0, 0};
    CHECK(none.ok(2));      // no spring at all, nbr and rest NULL
    Net b = ok4; b.first[0] = 1; CHECK(!b.ok(4, "first[0]"));
    b = ok4; b.first[2] = 1; CHECK(!b.ok(4, "first descends"));
    b = ok4; b.nbr[0] = 4; CHECK(!b.ok(4, "neighbour 4"));
    b = ok4; b.nbr[1] = -1; CHECK(!b.ok(4, "neighbour -1"));
    b = ok4; b.nbr[2] = 1; CHECK(!b.ok(4, "own neighbour"));
    b = ok4; b.nbr[0] = 3; CHECK(!b.ok(4, "does not ascend"));
    b = ok4; b.nbr[1] = 1; b.nbr[0] = 1; CHECK(!b.ok(4, "does not ascend"));
    b = ok4; b.rest[3] = 0.0; CHECK(!b.ok(4, "rest length"));
    b = ok4; b.rest[1] = -2.0; CHECK(!b.ok(4, "rest length"));
    b = ok4; b.rest[0] = NAN; CHECK(!b.ok(4, "rest length"));
    b = ok4; b.rest[0] = INFINITY; CHECK(!b.ok(4, "rest length"));
    CHECK(!fx_check_network("check", 4, nullptr, ok4.nbr.data(), ok4.rest.data(), msg, sizeof msg) && strstr(msg, "NULL first"));
    CHECK(!fx_check_network("check", 4, ok4.first.data(), nullptr, ok4.rest.data(), msg, sizeof msg) && strstr(msg, "NULL nbr"));
    CHECK(!fx_check_network("check", 4, ok4.first.data(), ok4.nbr.data(), nullptr, msg, sizeof msg) && strstr(msg, "NULL rest"));

    // -- arguments of the fit
    std::vector<double> x4 = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, w4 = {1.0, 0.0, -2.0, 3.5};
    auto fit = [&](bool map, int64_t n, const double *x, const double *w, double k, int steps, double mx, double mn) {
        return fx_check_fit_args("check", map, n, x, w, k, steps, mx, mn, msg, sizeof msg);
    };
    CHECK(fit(true, 4, x4.data(), w4.data(), 1.0, 2000, 0.5, 0.01) && fit(true, 4, x4.data(), nullptr, 0.0, 1, 0.5, 0.5));
    CHECK(!fit(false, 4, x4.data(), nullptr, 1.0, 1, 0.5, 0.01) && strstr(msg, "no map"));
    CHECK(!fit(true, 0, x4.data(), nullptr, 1.0, 1, 0.5, 0.01) && strstr(msg, "n_atoms"));
    CHECK(!fit(true, 4, nullptr, nullptr, 1.0, 1, 0.5, 0.01) && strstr(msg, "NULL coords"));
    CHECK(!fit(true, 4, x4.data(), w4.data(), -0.1, 1, 0.5, 0.01) && strstr(msg, "stiffness"));
    CHECK(!fit(true, 4, x4.data(), w4.data(), NAN, 1, 0.5, 0.01) && strstr(msg, "stiffness"));
    CHECK(!fit(true, 4, x4.data(), w4.data(), 1.0, 0, 0.5, 0.01) && strstr(msg, "n_steps"));
    CHECK(!fit(true, 4, x4.data(), w4.data(), 1.0, 1, 0.5, 0.0) && strstr(msg, "min_step"));
    CHECK(!fit(true, 4, x4.data(), w4.data(), 1.0, 1, 0.5, 0.6) && strstr(msg, "min_step"));
    CHECK(!fit(true, 4, x4.data(), w4.data(), 1.0, 1, INFINITY, 0.01) && strstr(msg, "max_step"));
    CHECK(!fit(true, 4, x4.data(), w4.data(), 1.0, 1, NAN, 0.01) && strstr(msg, "max_step"));
    w4[2] = NAN;
    CHECK(!fit(true, 4, x4.data(), w4.data(), 1.0, 1, 0.5, 0.01) && strstr(msg, "weight of atom 2"));
    x4[7] = -INFINITY;
    CHECK(!fit(true, 4, x4.data(), nullptr, 1.0, 1, 0.5, 0.01) && strstr(msg, "atom 2"));

    // -- the launch: never more workgroups than compute units, every atom owned, no thread count but a multiple of 64
    for (int n_cu : {1, 8, 256, 304})
        for (int64_t n = 1; n <= (1 << 20); n = n < 1100 ? n + 1 : n * 2 + 1)
            for (int fg : {0, 1, 2, 5, 1000})
                for (int ft : {0, 64, 256, 1024}) {
                    const FxPlan p = fx_plan(n_cu, n, fg, ft);
                    CHECK(p.groups >= 1 && p.groups <= n_cu);
                    CHECK(p.threads == (ft ? ft : FX_THREADS) && p.threads % 64 == 0 && p.threads <= FX_MAX_THREADS);
                    CHECK((int64_t)p.groups * p.threads * p.atoms_per_thread >= n);
                    CHECK((int64_t)p.groups * p.threads * (p.atoms_per_thread - 1) < n);
                    if (fg && fg <= n_cu) CHECK(p.groups == fg);
                }
    {
        const FxPlan a = fx_plan(256, 700, 0, 0), c = fx_plan(256, 26000, 0, 0), d = fx_plan(256, 1 << 20, 0, 0), e = fx_plan(256, 88, 2, 64);
        CHECK(a.groups == 3 && a.atoms_per_thread == 1 && c.groups == 102 && c.atoms_per_thread == 1);
        CHECK(d.groups == 256 && d.atoms_per_thread == 16 && e.groups == 2 && e.threads == 64 && e.atoms_per_thread == 1);
    }

    if (failures) { fprintf(stderr, "check_flexfit_plan: %d failure(s)\n", failures); return 1; }
    printf("check_flexfit_plan: ok\n");
    return 0;
}
