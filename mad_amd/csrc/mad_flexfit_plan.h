// mad_flexfit_plan.h -- the host side of mad_flex_network and mad_flex_fit: the argument checks, the cell grid
// over the atoms' bounding box, the check of a caller's network, and the workgroups and threads of the persistent launch.
// Plain C++ without a HIP type, so that it also compiles into a stand-alone host program (check_flexfit_plan.cpp); the functions
// the kernels share with that program carry FX_HD.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define FX_HD __host__ __device__
#else
#define FX_HD
#endif

#define FX_MAX_DEGREE 128            // MAD_FLEX_MAX_DEGREE of include/mad_amd.h: springs of one atom that mad_flex_network builds at most
#define FX_MAX_ATOMS ((1 << 24) - 1) // N at most: N x FX_MAX_DEGREE springs stay below 2^31
#define FX_MAX_DIM (1 << 20)         // cells per axis at most
#define FX_BATCH 4                   // steps between two looks at the displacement, as refine_pdb
#define FX_RUN 256                   // elements of one run of fourier.tree_sum's pairing
#define FX_THREADS 256               // threads of a workgroup unless "flex_threads" says otherwise
#define FX_MAX_THREADS 1024

// ---------------------------------------------------------------------------
// arguments
// ---------------------------------------------------------------------------

// n, the pointer and every coordinate (finite, |v| < 1e12); lo / hi (nullable) receive the bounding box
static inline bool fx_check_coords(const char *who, int64_t n, const double *coords, double *lo, double *hi, char *msg, size_t msg_len) {
    if (n < 1 || n > FX_MAX_ATOMS) { snprintf(msg, msg_len, "%s: n_atoms = %lld (1 .. %d)", who, (long long)n, FX_MAX_ATOMS); return false; }
    if (!coords) { snprintf(msg, msg_len, "%s: NULL coords", who); return false; }
    for (int64_t i = 0; i < n; i++)
        for (int d = 0; d < 3; d++) {
            const double v = coords[3 * i + d];
            if (!std::isfinite(v) || !(fabs(v) < 1e12)) { snprintf(msg, msg_len, "%s: coords: coordinate of atom %lld is not finite", who, (long long)i); return false; }
            if (lo && (i == 0 || v < lo[d])) lo[d] = v;
            if (hi && (i == 0 || v > hi[d])) hi[d] = v;
        }
    return true;
}

// The cell grid of mad_flex_network.  A pair within `cutoff` must lie in the same or in touching cells, whatever the rounding of the
// two cell indices: the edge is cutoff (1 + 2^-20), not cutoff.  (An index is floor of a quotient with two roundings, 2^-52 of
// its value together; two atoms whose true quotients differ by at most 1 / (1 + 2^-20) cannot get indices two apart below index
// 2^30, and FX_MAX_DIM is 2^20.)  The edge doubles until the grid has at most 4 n + 64 cells and FX_MAX_DIM per axis: wider cells
// hold every pair as well, and atoms strewn over a huge box cost no memory.  A box without extent on an axis has one cell there.
struct FxGrid {
    double lo[3], edge;
    int32_t dim[3];
    int64_t cells;
};
FX_HD static inline int32_t fx_cell_of(double v, double lo, double edge, int32_t dim) {
    const double q = floor((v - lo) / edge);
    const int32_t c = q > 0.0 ? (q < (double)(dim - 1) ? (int32_t)q : dim - 1) : 0;      // (a NaN lands in cell 0)
    return c;
}
static inline void fx_grid(int64_t n, const double lo[3], const double hi[3], double cutoff, FxGrid &g) {
    g.edge = cutoff * (1.0 + 0x1p-20);
    for (;;) {
        double cells = 1.0;
        bool fits = true;
        for (int d = 0; d < 3; d++) {
            const double q = floor((hi[d] - lo[d]) / g.edge) + 1.0;
            if (!(q <= (double)FX_MAX_DIM)) { fits = false; break; }
            g.dim[d] = (int32_t)q;
            cells *= q;
        }
        if (fits && cells <= 4.0 * (double)n + 64.0) { g.cells = (int64_t)cells; break; }
        g.edge *= 2.0;
    }
    for (int d = 0; d < 3; d++) g.lo[d] = lo[d];
}

static inline bool fx_check_network_args(const char *who, int64_t n, const double *coords, double cutoff, FxGrid &g, char *msg, size_t msg_len) {
    double lo[3], hi[3];
    if (!fx_check_coords(who, n, coords, lo, hi, msg, msg_len)) return false;
    if (!(cutoff > 0.0) || !(cutoff < 1e12)) { snprintf(msg, msg_len, "%s: cutoff = %g", who, cutoff); return false; }
    fx_grid(n, lo, hi, cutoff, g);
    return true;
}

// A network as mad_flex_fit takes it: first[n + 1] ascending from 0, rows that may be empty, neighbours in range, no atom its own
// neighbour, every row strictly ascending, rest lengths finite and positive.
static inline bool fx_check_network(const char *who, int64_t n, const int32_t *first, const int32_t *nbr, const double *rest, char *msg, size_t msg_len) {
    if (!first) { snprintf(msg, msg_len, "%s: NULL first", who); return false; }
    if (first[0] != 0) { snprintf(msg, msg_len, "%s: network: first[0] = %d", who, first[0]); return false; }
    for (int64_t i = 0; i < n; i++)
        if (first[i + 1] < first[i]) { snprintf(msg, msg_len, "%s: network: first descends at atom %lld", who, (long long)i); return false; }
    if (first[n] > 0 && !nbr) { snprintf(msg, msg_len, "%s: NULL nbr", who); return false; }
    if (first[n] > 0 && !rest) { snprintf(msg, msg_len, "%s: NULL rest", who); return false; }
    for (int64_t i = 0; i < n; i++)
        for (int32_t e = first[i]; e < first[i + 1]; e++) {
            const int32_t j = nbr[e];
            if (j < 0 || j >= n) { snprintf(msg, msg_len, "%s: network: atom %lld has neighbour %d of %lld atoms", who, (long long)i, j, (long long)n); return false; }
            if (j == i) { snprintf(msg, msg_len, "%s: network: atom %lld is its own neighbour", who, (long long)i); return false; }
            if (e > first[i] && j <= nbr[e - 1]) { snprintf(msg, msg_len, "%s: network: the row of atom %lld does not ascend", who, (long long)i); return false; }
            if (!std::isfinite(rest[e]) || !(rest[e] > 0.0)) { snprintf(msg, msg_len, "%s: network: rest length %g of spring %lld - %d", who, rest[e], (long long)i, j); return false; }
        }
    return true;
}

// everything of mad_flex_fit but the map and the network
static inline bool fx_check_fit_args(const char *who, bool have_map, int64_t n, const double *coords, const double *weights, double stiffness,
                                     int32_t n_steps, double max_step, double min_step, char *msg, size_t msg_len) {
    if (!have_map) { snprintf(msg, msg_len, "%s: no map: call mad_upload_density first", who); return false; }
    if (!fx_check_coords(who, n, coords, nullptr, nullptr, msg, msg_len)) return false;
    if (weights)
        for (int64_t i = 0; i < n; i++)
            if (!std::isfinite(weights[i])) { snprintf(msg, msg_len, "%s: weights: weight of atom %lld is not finite", who, (long long)i); return false; }
    if (!(stiffness >= 0.0) || !(stiffness < 1e12)) { snprintf(msg, msg_len, "%s: stiffness = %g", who, stiffness); return false; }
    if (n_steps < 1) { snprintf(msg, msg_len, "%s: n_steps = %d", who, n_steps); return false; }
    if (!(min_step > 0.0) || !(max_step < 1e12)) { snprintf(msg, msg_len, "%s: min_step = %g, max_step = %g", who, min_step, max_step); return false; }
    if (!(min_step <= max_step)) { snprintf(msg, msg_len, "%s: min_step = %g above max_step = %g", who, min_step, max_step); return false; }
    return true;
}

// ---------------------------------------------------------------------------
// the persistent launch: thread t of all T = groups x threads owns atoms t, t + T, ...
// ---------------------------------------------------------------------------
struct FxPlan {
    int32_t groups, threads, atoms_per_thread;
};
// forced_threads: 0, or a multiple of 64 up to FX_MAX_THREADS; forced_groups: 0, or 1 .. (it is cut to n_cu: every workgroup has to
// be resident, the grid barrier waits for all of them).  By default a thread owns one atom until the compute units run out.
static inline FxPlan fx_plan(int32_t n_cu, int64_t n, int32_t forced_groups, int32_t forced_threads) {
    FxPlan p;
    p.threads = forced_threads > 0 ? forced_threads : FX_THREADS;
    int64_t g = forced_groups > 0 ? forced_groups : (n + p.threads - 1) / p.threads;
    if (g > n_cu) g = n_cu;
    if (g < 1) g = 1;
    p.groups = (int32_t)g;
    const int64_t T = (int64_t)p.groups * p.threads;
    p.atoms_per_thread = (int32_t)((n + T - 1) / T);
    return p;
}
