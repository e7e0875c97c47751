// mad_bfactor_plan.h -- the host side of mad_model_density_b and mad_bfactor_refine: the argument checks, the
// box of voxels the atoms can reach at b_max and its clipping, the cell grid over the atoms that reach the lattice (a stable counting
// sort: cells ascending, atoms ascending within a cell), the group table, and the bricks, chunks and sum levels of a call.
// Plain C++ without a HIP type, so that it also compiles into a stand-alone host program (check_bfactor_plan.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mad_flexfit_plan.h"      // FxGrid, fx_grid, fx_cell_of: the cell grid over a bounding box

#define BF_BRICK 8                   // a gather workgroup's brick is 8 x 8 x 8 voxels of the box
#define BF_BRICK_VOXELS (BF_BRICK * BF_BRICK * BF_BRICK)
#define BF_RUN 256                   // elements of one run of fourier.tree_sum's pairing, and the workgroup of the sum kernels
#define BF_BATCH 4                   // cycles between two looks at how far B moved, as refine_pdb
#define BF_CHUNK 512                 // atoms of one LDS chunk unless "bf_chunk" says otherwise
#define BF_MIN_CHUNK 64
#define BF_MAX_CHUNK 1024
#define BF_STAGE 6                   // doubles staged per atom: x, y, z, 9 v, 2 v, m / ((2 pi v) sqrt(2 pi v))
#define BF_THREADS 256               // threads of a gather workgroup unless "bf_threads" says otherwise
#define BF_MAX_THREADS 512           // (a thread has a voxel of the brick at least)
#define BF_MAX_ATOMS ((1 << 24) - 1)
#define BF_MAX_DIM 2048              // voxels per axis of the lattice at most
#define BF_MAX_LEVELS 8

static inline double bf_K() { return 8.0 * M_PI * M_PI; }
static inline double bf_v0(double resolution) {
    const double s0 = resolution / (M_PI * sqrt(2.0));
    return s0 * s0;
}

// ---------------------------------------------------------------------------
// arguments
// ---------------------------------------------------------------------------
static inline bool bf_check_lattice(const char *who, const int32_t dims[3], const double origin[3], double voxsp, char *msg, size_t msg_len) {
    if (!dims || !origin) { snprintf(msg, msg_len, "%s: NULL %s", who, !dims ? "dims" : "origin"); return false; }
    for (int d = 0; d < 3; d++) {
        if (dims[d] < 1 || dims[d] > BF_MAX_DIM) { snprintf(msg, msg_len, "%s: dims[%d] = %d (1 .. %d)", who, d, dims[d], BF_MAX_DIM); return false; }
        if (!std::isfinite(origin[d]) || !(fabs(origin[d]) < 1e12)) { snprintf(msg, msg_len, "%s: origin[%d] is not finite", who, d); return false; }
    }
    if (!(voxsp > 0.0) || !(voxsp < 1e6)) { snprintf(msg, msg_len, "%s: voxsp = %g", who, voxsp); return false; }
    return true;
}

static inline bool bf_check_atoms(const char *who, int64_t n, const double *coords, const double *masses, double resolution, char *msg, size_t msg_len) {
    if (!(resolution > 0.0) || !(resolution < 1e6)) { snprintf(msg, msg_len, "%s: resolution = %g", who, resolution); return false; }
    if (!fx_check_coords(who, n, coords, nullptr, nullptr, msg, msg_len)) return false;
    if (!masses) { snprintf(msg, msg_len, "%s: NULL masses", who); return false; }
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(masses[i])) { snprintf(msg, msg_len, "%s: masses: mass of atom %lld is not finite", who, (long long)i); return false; }
    return true;
}

static inline bool bf_check_limits(const char *who, double b_min, double b_max, char *msg, size_t msg_len) {
    if (!(b_min >= 0.0) || !(b_max < 1e9) || !(b_min <= b_max)) { snprintf(msg, msg_len, "%s: b_min = %g, b_max = %g (0 <= b_min <= b_max)", who, b_min, b_max); return false; }
    return true;
}

// every value of b (n of them, `what` names the argument) within [b_min, b_max]
static inline bool bf_check_b(const char *who, const char *what, int64_t n, const double *b, double b_min, double b_max, char *msg, size_t msg_len) {
    if (!b) { snprintf(msg, msg_len, "%s: NULL %s", who, what); return false; }
    for (int64_t i = 0; i < n; i++)
        if (!(b[i] >= b_min) || !(b[i] <= b_max)) { snprintf(msg, msg_len, "%s: %s[%lld] = %g outside [b_min, b_max] = [%g, %g]", who, what, (long long)i, b[i], b_min, b_max); return false; }
    return true;
}

// The group table: first_atom[n_groups + 1] ascends from 0 to n_atoms (a group may be empty); the atoms come sorted by group.
static inline bool bf_check_groups(const char *who, int64_t n_atoms, int64_t n_groups, const int64_t *first_atom, char *msg, size_t msg_len) {
    if (n_groups < 1 || n_groups > BF_MAX_ATOMS) { snprintf(msg, msg_len, "%s: n_groups = %lld (1 .. %d)", who, (long long)n_groups, BF_MAX_ATOMS); return false; }
    if (!first_atom) { snprintf(msg, msg_len, "%s: NULL first_atom", who); return false; }
    if (first_atom[0] != 0) { snprintf(msg, msg_len, "%s: first_atom[0] = %lld: the groups do not cover the atoms", who, (long long)first_atom[0]); return false; }
    for (int64_t g = 0; g < n_groups; g++)
        if (first_atom[g + 1] < first_atom[g]) { snprintf(msg, msg_len, "%s: first_atom descends at group %lld", who, (long long)g); return false; }
    if (first_atom[n_groups] != n_atoms) { snprintf(msg, msg_len, "%s: first_atom ends at %lld of %lld atoms: the groups do not cover the atoms", who, (long long)first_atom[n_groups], (long long)n_atoms); return false; }
    return true;
}

static inline bool bf_check_cycles(const char *who, int32_t n_cycles, double max_step, double min_step, char *msg, size_t msg_len) {
    if (n_cycles < 1 || n_cycles > 100000) { snprintf(msg, msg_len, "%s: n_cycles = %d (1 .. 100000)", who, n_cycles); return false; }
    if (!(min_step > 0.0) || !(max_step < 1e9) || !(min_step <= max_step)) { snprintf(msg, msg_len, "%s: min_step = %g, max_step = %g (0 < min_step <= max_step)", who, min_step, max_step); return false; }
    return true;
}

// ---------------------------------------------------------------------------
// the box: the voxels any atom can reach at b_max, clipped to the lattice
// ---------------------------------------------------------------------------
// An atom reaches no farther than rmax = 3 sqrt(v0 + b_max / K) along an axis.  Its voxels on an axis lie within floor((x - rmax - o) / vs)
// .. ceil((x + rmax - o) / vs): a voxel more on either side than the true range, which covers the roundings of the quotient.  An atom
// whose range misses the lattice on an axis reaches no voxel of it and is left out of the cell grid (keep = 0); the box is the union of
// the kept atoms' clipped ranges.
struct BfBox {
    int32_t lo[3], dim[3];      // the first voxel and the extent per axis (dim 0: no atom reaches the lattice)
    int64_t voxels, kept;
    double rmax;
};
static inline int32_t bf_clamp_index(double q, int32_t lo, int32_t hi) { return q < (double)lo ? lo : (q > (double)hi ? hi : (int32_t)q); }
// the clipped range of one coordinate reaching r on an axis of n voxels: false when it misses the lattice
static inline bool bf_axis_range(double x, double r, double o, double vs, int32_t n, int32_t &lo, int32_t &hi) {
    const double ql = floor((x - r - o) / vs), qh = ceil((x + r - o) / vs);
    if (!(qh >= 0.0) || !(ql <= (double)(n - 1))) return false;
    lo = bf_clamp_index(ql, 0, n - 1);
    hi = bf_clamp_index(qh, 0, n - 1);
    return true;
}
static inline void bf_box(const int32_t dims[3], const double origin[3], double vs, int64_t n, const double *coords, double resolution, double b_max,
                          BfBox &box, std::vector<uint8_t> &keep) {
    box.rmax = 3.0 * sqrt(bf_v0(resolution) + b_max / bf_K());
    keep.assign((size_t)n, 0);
    int32_t blo[3] = {0, 0, 0}, bhi[3] = {-1, -1, -1};
    box.kept = 0;
    for (int64_t i = 0; i < n; i++) {
        int32_t lo[3], hi[3];
        bool in = true;
        for (int d = 0; d < 3 && in; d++) in = bf_axis_range(coords[3 * i + d], box.rmax, origin[d], vs, dims[d], lo[d], hi[d]);
        if (!in) continue;
        for (int d = 0; d < 3; d++) {
            if (box.kept == 0 || lo[d] < blo[d]) blo[d] = lo[d];
            if (box.kept == 0 || hi[d] > bhi[d]) bhi[d] = hi[d];
        }
        keep[(size_t)i] = 1;
        box.kept++;
    }
    box.voxels = box.kept ? 1 : 0;
    for (int d = 0; d < 3; d++) {
        box.lo[d] = blo[d];
        box.dim[d] = box.kept ? bhi[d] - blo[d] + 1 : 0;
        box.voxels *= box.dim[d];
    }
}

// ---------------------------------------------------------------------------
// the cell grid over the kept atoms: fx_grid with the reach as the cutoff; order[] lists them cell by cell, ascending within a cell
// ---------------------------------------------------------------------------
struct BfCells {
    FxGrid g;
    std::vector<int32_t> start;      // cells + 1
    std::vector<int32_t> order;      // kept atoms
};
static inline void bf_cells(int64_t n, const double *coords, const std::vector<uint8_t> &keep, int64_t kept, double rmax, BfCells &c) {
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool first = true;
    for (int64_t i = 0; i < n; i++) {
        if (!keep[(size_t)i]) continue;
        for (int d = 0; d < 3; d++) {
            const double v = coords[3 * i + d];
            if (first || v < lo[d]) lo[d] = v;
            if (first || v > hi[d]) hi[d] = v;
        }
        first = false;
    }
    fx_grid(kept > 0 ? kept : 1, lo, hi, rmax, c.g);
    c.start.assign((size_t)c.g.cells + 1, 0);
    c.order.assign((size_t)kept, 0);
    std::vector<int32_t> cell((size_t)n, -1);
    for (int64_t i = 0; i < n; i++) {
        if (!keep[(size_t)i]) continue;
        const int32_t cx = fx_cell_of(coords[3 * i], c.g.lo[0], c.g.edge, c.g.dim[0]), cy = fx_cell_of(coords[3 * i + 1], c.g.lo[1], c.g.edge, c.g.dim[1]),
                      cz = fx_cell_of(coords[3 * i + 2], c.g.lo[2], c.g.edge, c.g.dim[2]);
        cell[(size_t)i] = (cx * c.g.dim[1] + cy) * c.g.dim[2] + cz;
        c.start[(size_t)cell[(size_t)i] + 1]++;
    }
    for (int64_t k = 0; k < c.g.cells; k++) c.start[(size_t)k + 1] += c.start[(size_t)k];
    std::vector<int32_t> cursor(c.start.begin(), c.start.end() - 1);
    for (int64_t i = 0; i < n; i++)      // ascending i: ascending within a cell
        if (cell[(size_t)i] >= 0) c.order[(size_t)cursor[(size_t)cell[(size_t)i]]++] = (int32_t)i;
}

// The cells that can hold an atom within rmax of the voxels j0 .. j1 of an axis: from the cell of the first voxel less rmax to the
// cell of the last plus rmax, one spare cell on either side for the roundings, clamped (the cell function is monotone).
FX_HD static inline void bf_cell_range(double o, double vs, int32_t j0, int32_t j1, double rmax, double glo, double edge, int32_t dim, int32_t &c0, int32_t &c1) {
    c0 = fx_cell_of(o + vs * (double)j0 - rmax, glo, edge, dim) - 1;
    c1 = fx_cell_of(o + vs * (double)j1 + rmax, glo, edge, dim) + 1;
    if (c0 < 0) c0 = 0;
    if (c1 > dim - 1) c1 = dim - 1;
}

// ---------------------------------------------------------------------------
// the launches
// ---------------------------------------------------------------------------
struct BfPlan {
    int32_t bricks[3], chunk, threads, levels;
    int64_t n_bricks, runs[BF_MAX_LEVELS];      // runs[l]: the sums level l writes (runs[levels - 1] == 1)
};
// forced_chunk: 0, or BF_MIN_CHUNK .. BF_MAX_CHUNK; forced_threads: 0, or a multiple of 64 up to BF_MAX_THREADS
static inline BfPlan bf_plan(const BfBox &box, int32_t forced_chunk, int32_t forced_threads) {
    BfPlan p;
    p.chunk = forced_chunk > 0 ? forced_chunk : BF_CHUNK;
    p.threads = forced_threads > 0 ? forced_threads : BF_THREADS;
    p.n_bricks = 1;
    for (int d = 0; d < 3; d++) {
        p.bricks[d] = (box.dim[d] + BF_BRICK - 1) / BF_BRICK;
        p.n_bricks *= p.bricks[d];
    }
    p.levels = 0;
    int64_t terms = box.voxels;
    do {
        terms = (terms + BF_RUN - 1) / BF_RUN;
        p.runs[p.levels++] = terms;
    } while (terms > 1 && p.levels < BF_MAX_LEVELS);
    return p;
}
