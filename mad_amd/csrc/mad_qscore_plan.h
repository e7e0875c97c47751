// mad_qscore_plan.h -- the host side of mad_map_qscore: the argument checks, the per-shell tables and the
// cell grid over the atoms' bounding box.  Plain C++ without a HIP type, so that it also compiles into a stand-alone host program
// (check_qscore_plan.cpp); the two functions the kernels share with that program carry QS_HD.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define QS_HD __host__ __device__
#else
#define QS_HD
#endif

#define QS_POINTS 8             // points of a shell
#define QS_MAX_R 64             // shells at most
#define QS_MAX_TRIES 64         // point sets at most: set t has QS_POINTS * t directions, 512 in the largest
#define QS_CHUNK 256            // neighbours of one LDS chunk of a wave (8 KiB)
#define QS_MAXC 64              // cells per axis at most, as mad_zone.hip
#define QS_WAVES 4              // waves (= scored atoms) per workgroup

// directions before set t (1-based) and in all sets up to t
static inline long long qs_set_offset(int t) { return 4ll * t * (t - 1); }
static inline long long qs_dirs_total(int n_tries) { return 4ll * n_tries * (n_tries + 1); }

struct QsPlan {
    int32_t n[3] = {0, 0, 0};              // voxels
    double o[3] = {0, 0, 0}, voxsp = 0;
    int32_t nc[3] = {1, 1, 1};             // cells
    double glo[3] = {0, 0, 0}, h = 1;      // cell c of axis a begins at glo[a] + h * c
    int32_t n_r = 0, n_tries = 0, n_cells = 1;
    int64_t n_atoms = 0, n_scored = 0, n_dirs = 0;
    double r2[QS_MAX_R];                   // R * R: what a candidate's D2 is compared with
    double cut[QS_MAX_R];                  // a neighbour whose d2 to the scored atom is above this decides nothing in the shell
};

// cell of coordinate v on one axis: monotone in v, clamped into the grid
QS_HD static inline int qs_cell(double v, double glo, double h, int nc) {
    const double c = floor((v - glo) / h);
    return c < 0.0 ? 0 : (c > (double)(nc - 1) ? nc - 1 : (int)c);
}
// squared distance between two atoms: the contract's expression
QS_HD static inline double qs_d2(const double a[3], const double b[3]) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// false with a message in msg: the call is refused.  Everything the contract refuses is refused here except a NULL ctx, grid or
// output (the caller's).
//
// The margins.  Atom b changes a decision of atom x in the shell of radius R only if some candidate p = fl(x + fl(R dir)) has a
// computed D2(p, b) <= fl(R R).  Write u = 2^-53 and S = `scale`, a bound on every coordinate that occurs (|atom| + R_max).
//   * dir is no longer than 1 + 2^-21 (checked below: |dir|^2 <= 1 + 2^-20), a product and a sum round by at most u S each per
//     axis, so the real |p - x| <= R (1 + 2^-21) + 2 sqrt(3) u S.
//   * dx = fl(p - b) is off by at most u S per axis and the three squares and two sums of D2 by 3 u relative, so a computed
//     D2 <= fl(R R) means a real |p - b| <= R (1 + 3 u) + sqrt(3) u S.
//   * hence the real |x - b| <= 2 R (1 + 2^-21 + 3 u) + 3 sqrt(3) u S, and the computed d2(x, b) is at most the square of that
//     times (1 + 3 u) plus 2 sqrt(3) u S |x - b|.
// cut(R) = (2 R (1 + 2^-20) + 2^-40 S)^2 is the square of a length that exceeds that bound twice over: its relative term 2^-20
// is twice 2^-21 + 3 u, and its absolute term 2^-40 S = 2^13 u S is a thousand times the (3 + 2) sqrt(3) u S of the roundings.  A
// neighbour with d2 > cut(R) cannot change a decision, and one kept needlessly costs time only, never a decision: the kernel
// decides every candidate by the contract's own expression.
// The cell edge is h >= 2 R_max (1 + 2^-20) + 2^-30 S (or the atoms' extent / QS_MAXC where that is more).  Two atoms within
// sqrt(cut(R_max)) = 2 R_max (1 + 2^-20) + 2^-40 S of each other differ by at most h - (2^-30 - 2^-40) S per axis, so their real
// quotients (v - glo) / h differ by at most 1 - 2^-31 S / h.  A computed quotient carries two roundings: the difference, u S / h in the
// quotient, 2^22 times smaller than the spare; and the division, u times a quotient below QS_MAXC + 1, under 2^-46, where the spare
// is at least 2^-33 (S >= R_max by construction and h < 2.1 R_max + 2^-30 S, or h = extent / QS_MAXC <= S / 32: S / h > 1 / 4).
// floor and the clamp are monotone: the cells differ by at most 1 per axis, and the 27 cells around the cell of x hold b.  (With
// R_max = 0 no neighbour is ever asked for.)
static inline bool qs_plan(const int32_t dims[3], const double origin[3], double voxsp, const double *atoms, int64_t n_atoms,
                           const int64_t *index, int64_t n_index, const double *radii, const double *ref, int32_t n_r,
                           const double *dirs, int32_t n_tries, QsPlan &P, char *msg, size_t msg_len) {
    const char *who = "mad_map_qscore";
    if (!dims || !origin || !radii || !ref || !dirs) { snprintf(msg, msg_len, "%s: NULL argument", who); return false; }
    if (n_atoms < 0 || n_index < 0) { snprintf(msg, msg_len, "%s: %lld atoms, %lld indices", who, (long long)n_atoms, (long long)n_index); return false; }
    if (n_atoms > 0 && !atoms) { snprintf(msg, msg_len, "%s: NULL atoms", who); return false; }
    if (n_atoms >= (1ll << 31) || n_index >= (1ll << 31)) {
        snprintf(msg, msg_len, "%s: %lld atoms, %lld indices: 2^31 or more are not supported", who, (long long)n_atoms, (long long)n_index);
        return false;
    }
    for (int k = 0; k < 3; k++)
        if (dims[k] < 1) { snprintf(msg, msg_len, "%s: grid of %d x %d x %d voxels", who, dims[0], dims[1], dims[2]); return false; }
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 32) || vxy * (unsigned long long)dims[2] >= (1ull << 32)) {
        snprintf(msg, msg_len, "%s: %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
        return false;
    }
    if (!std::isfinite(voxsp) || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) {
        snprintf(msg, msg_len, "%s: an origin or a spacing that is not finite", who);
        return false;
    }
    if (!(voxsp > 0)) { snprintf(msg, msg_len, "%s: voxsp %g", who, voxsp); return false; }
    if (n_r < 1 || n_r > QS_MAX_R) { snprintf(msg, msg_len, "%s: %d shells (1 .. %d)", who, n_r, QS_MAX_R); return false; }
    if (n_tries < 1 || n_tries > QS_MAX_TRIES) { snprintf(msg, msg_len, "%s: %d point sets (1 .. %d)", who, n_tries, QS_MAX_TRIES); return false; }
    for (int k = 0; k < n_r; k++) {
        if (!std::isfinite(radii[k]) || !std::isfinite(ref[k])) { snprintf(msg, msg_len, "%s: shell %d has a radius or a ref value that is not finite", who, k); return false; }
        if (radii[k] < 0) { snprintf(msg, msg_len, "%s: radius %g of shell %d is negative", who, radii[k], k); return false; }
        if (k > 0 && !(radii[k] > radii[k - 1])) { snprintf(msg, msg_len, "%s: the radii do not ascend at shell %d", who, k); return false; }
    }
    P.n_dirs = qs_dirs_total(n_tries);
    for (int64_t i = 0; i < P.n_dirs; i++) {
        const double *d = dirs + 3 * i;
        const double l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        if (!(l2 <= 1.0 + 0x1p-20)) { snprintf(msg, msg_len, "%s: direction %lld is not a unit vector (or not finite)", who, (long long)i); return false; }
    }
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n_atoms; i++)
        for (int a = 0; a < 3; a++) {
            const double v = atoms[3 * i + a];
            if (!std::isfinite(v)) { snprintf(msg, msg_len, "%s: atom %lld has a coordinate that is not finite", who, (long long)i); return false; }
            mn[a] = v < mn[a] ? v : mn[a];
            mx[a] = v > mx[a] ? v : mx[a];
        }
    if (index)
        for (int64_t j = 0; j < n_index; j++)
            if (index[j] < 0 || index[j] >= n_atoms) {
                snprintf(msg, msg_len, "%s: index[%lld] = %lld, there are %lld atoms", who, (long long)j, (long long)index[j], (long long)n_atoms);
                return false;
            }
    P.n_atoms = n_atoms;
    P.n_scored = index ? n_index : n_atoms;
    P.n_r = n_r;
    P.n_tries = n_tries;
    P.voxsp = voxsp;
    for (int a = 0; a < 3; a++) { P.n[a] = dims[a]; P.o[a] = origin[a]; P.nc[a] = 1; P.glo[a] = 0.0; }
    P.h = 1.0;
    P.n_cells = 1;
    const double r_max = radii[n_r - 1];
    double scale = 0.0, ext = 0.0;
    if (n_atoms > 0)
        for (int a = 0; a < 3; a++) {
            scale = fmax(scale, fmax(fabs(mn[a]), fabs(mx[a])));
            ext = fmax(ext, mx[a] - mn[a]);
        }
    scale += r_max;
    if (!std::isfinite(scale) || !std::isfinite(ext) || !std::isfinite(2.0 * r_max * (1.0 + 0x1p-20) + 0x1p-30 * scale)) {
        snprintf(msg, msg_len, "%s: the atoms' box grown by the largest radius is too large for float64", who);
        return false;
    }
    for (int k = 0; k < QS_MAX_R; k++) {
        const double R = k < n_r ? radii[k] : 0.0, c = 2.0 * R * (1.0 + 0x1p-20) + 0x1p-40 * scale;
        P.r2[k] = R * R;
        P.cut[k] = c * c;
    }
    if (n_atoms > 0) {
        P.h = fmax(2.0 * r_max * (1.0 + 0x1p-20) + 0x1p-30 * scale, ext / (double)QS_MAXC);
        if (!(P.h > 0.0)) P.h = 1.0;      // every atom at the origin and no shell but R = 0: one cell
        for (int a = 0; a < 3; a++) {
            P.glo[a] = mn[a];
            const double c = floor((mx[a] - mn[a]) / P.h) + 1.0;
            P.nc[a] = c < 1.0 ? 1 : (c > (double)QS_MAXC ? QS_MAXC : (int)c);
            P.n_cells *= P.nc[a];
        }
    }
    return true;
}
