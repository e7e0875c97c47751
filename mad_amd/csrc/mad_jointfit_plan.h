// mad_jointfit_plan.h -- the host side of mad_assembly_density and mad_assembly_refine: the argument checks,
// the blur taps, a body's box (edge and clipped placement), the round count and the workgroups per body; and of
// mad_assembly_refine_symmetric (section 4z): the operator checks, an image and a pulled-back gradient, the plan of the images.
// Plain C++ without a HIP type, so that it also compiles into a stand-alone host program (check_jointfit_plan.cpp); the functions
// the kernels share with that program carry JF_HD.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define JF_HD __host__ __device__
#else
#define JF_HD
#endif

#define JF_MAX_BODIES 64
#define JF_MAX_R 64             // blur radius in voxels at most (as mad_structure_to_density)
#define JF_BATCH 4              // steps of a round = a batch of refine_pdb (structure_utils.py:83)
#define JF_THREADS 1024         // workgroup of the global-memory form of k_jf_steps, as k_refine<0>
#define JF_THREADS_REG 512      // ... and of the register-resident form, as k_refine<8>
#define JF_MAXA 8               // atoms a thread of the register-resident form holds at most
#define JF_MAX_G 8              // workgroups per body at most
#define JF_FIX_BITS 36          // the splat accumulates in 2^-36 fixed point, as k_splat_b

// rounds of a run of n_steps steps: complete batches, and an incomplete one when n_steps is no multiple of JF_BATCH
static inline int32_t jf_rounds(int32_t n_steps) { return n_steps / JF_BATCH + (n_steps % JF_BATCH != 0); }
// steps of round `round`
JF_HD static inline int32_t jf_round_steps(int32_t n_steps, int32_t round) {
    const int32_t left = n_steps - JF_BATCH * round;
    return left < 0 ? 0 : (left < JF_BATCH ? left : JF_BATCH);
}

// sig = resolution / (pi sqrt 2) / vs, r = ceil(3 sig), taps[t] = exp(-(t - r)^2 / (2 sig^2)) / their sum, t = 0 .. 2 r: the 1-D factor of
// structure_to_density's Gaussian.  false: r is outside 0 .. JF_MAX_R (taps must hold 2 JF_MAX_R + 1 values).
static inline bool jf_taps(double resolution, double vs, int32_t *r_out, double *sig_out, double *taps) {
    const double sig = resolution / (M_PI * sqrt(2.0)) / vs;
    const double r3 = ceil(3.0 * sig);
    if (!(r3 >= 0.0) || !(r3 <= (double)JF_MAX_R)) return false;
    const int r = (int)r3;
    double ts = 0;
    for (int t = -r; t <= r; t++) { taps[t + r] = exp(-(double)(t * t) / (2.0 * sig * sig)); ts += taps[t + r]; }
    for (int t = 0; t <= 2 * r; t++) taps[t] /= ts;
    *r_out = r; *sig_out = sig;
    return true;
}

// Edge of a body's cube in voxels, fixed for the run: 2 (max_dist + r vs + 4 max_step) / vs + 4, rounded up.  Half of it holds the
// farthest atom, the blur's reach and the most a body moves in a round (two translations and two rotations of at most max_step
// each); the 4 spare voxels hold the splat's far corner (1), the rounding of the centre to the lattice (1/2) and roundings of
// max_dist and the centre.  -1: more than 2^20 voxels, which no map has.
static inline int32_t jf_box_edge(double max_dist, int32_t r, double vs, double max_step) {
    const double e = ceil(2.0 * (max_dist + r * vs + 4.0 * max_step) / vs + 4.0);
    if (!(e >= 4.0) || !(e <= 1048576.0)) return -1;
    return (int32_t)e;
}

// Where the cube of edge `edge` around the coordinate c starts on an axis of n voxels (origin o, spacing vs): centred on c rounded
// to the lattice, then shifted into 0 .. n - e, e = min(edge, n) being the cube's extent on this axis.  A shift loses nothing of
// the body that lies inside the map: the part of the axis it gives up lies beyond the map's face.  A c that is not finite, or
// far outside, gives a face of the map.
JF_HD static inline int32_t jf_box_extent(int32_t edge, int32_t n) { return edge < n ? edge : n; }
JF_HD static inline int32_t jf_box_lo(double c, double o, double vs, int32_t edge, int32_t n) {
    const int32_t e = jf_box_extent(edge, n);
    double t = floor((c - o) / vs + 0.5);
    if (!(t > -4194304.0)) t = -4194304.0;      // (NaN lands here too)
    if (t > 4194304.0) t = 4194304.0;
    const int32_t lo = (int32_t)t - edge / 2;
    return lo < 0 ? 0 : (lo > n - e ? n - e : lo);
}

// Workgroups per body and kernel form, by mad_refine's rule for a batch of n_bodies candidates, so that a run of one body is
// k_refine's: G <= n_cu / n_bodies (all workgroups resident at one per compute unit: the wait of the group reduction relies on it),
// G <= cap, and a workgroup of the global-memory form keeps at least 2 atoms per thread.
static inline int32_t jf_groups(int32_t n_cu, int32_t n_bodies, int64_t n_atoms, int32_t cap) {
    int32_t G = n_cu / n_bodies;
    if (G > cap) G = cap;
    if (G > JF_MAX_G) G = JF_MAX_G;
    if (G < 1) G = 1;
    while (G > 1 && n_atoms < (int64_t)G * JF_THREADS * 2) G--;
    return G;
}
static inline bool jf_fits_registers(int64_t n_atoms, int32_t G) {
    return (n_atoms + (int64_t)G * JF_THREADS_REG - 1) / ((int64_t)G * JF_THREADS_REG) <= JF_MAXA;
}

struct JfPlan {
    int32_t n_bodies = 0;
    int64_t n_atoms = 0;                       // of all bodies
    int32_t r = 0;
    double sig = 0;
    double taps[2 * JF_MAX_R + 1];
    double cen[JF_MAX_BODIES][3];              // the bodies' centres and farthest atoms as the HOST sums them: they size and place
    double max_dist[JF_MAX_BODIES];            // the boxes only (the refinement's own are the device's)
    int32_t edge[JF_MAX_BODIES];
    int32_t lo[JF_MAX_BODIES][3], e[JF_MAX_BODIES][3];
    int64_t vox0[JF_MAX_BODIES + 1];           // body b's box begins at voxel vox0[b] of the box buffers
    int64_t max_box = 0, max_atoms = 0;
};

// false with a message in msg: the call is refused.  `who` is the entry point's name; refine: the step arguments are checked too.
// dims == nullptr: no map has been uploaded.
static inline bool jf_plan(const char *who, const int32_t *dims, const double *origin, double vs, int32_t n_bodies, const double *atoms,
                           const double *mass, const int64_t *first_atom, double resolution, bool refine, int32_t n_steps, double max_step,
                           double min_step, JfPlan &P, char *msg, size_t msg_len) {
    if (!dims) { snprintf(msg, msg_len, "%s: no map: call mad_upload_density first", who); return false; }
    if (n_bodies < 1 || n_bodies > JF_MAX_BODIES) { snprintf(msg, msg_len, "%s: n_bodies = %d (1 .. %d)", who, n_bodies, JF_MAX_BODIES); return false; }
    if (!atoms) { snprintf(msg, msg_len, "%s: NULL atoms", who); return false; }
    if (!mass) { snprintf(msg, msg_len, "%s: NULL mass", who); return false; }
    if (!first_atom) { snprintf(msg, msg_len, "%s: NULL first_atom", who); return false; }
    if (!(resolution > 0.0) || !(resolution < 1e12)) { snprintf(msg, msg_len, "%s: resolution = %g", who, resolution); return false; }
    if (refine) {
        if (n_steps < 1) { snprintf(msg, msg_len, "%s: n_steps = %d", who, n_steps); return false; }
        if (!(min_step > 0.0) || !(max_step < 1e12)) { snprintf(msg, msg_len, "%s: min_step = %g, max_step = %g", who, min_step, max_step); return false; }
        if (!(min_step <= max_step)) { snprintf(msg, msg_len, "%s: min_step = %g above max_step = %g", who, min_step, max_step); return false; }
    } else {
        max_step = 0.0;
    }
    if (first_atom[0] != 0) { snprintf(msg, msg_len, "%s: first_atom[0] = %lld", who, (long long)first_atom[0]); return false; }
    for (int b = 0; b < n_bodies; b++) {
        if (first_atom[b + 1] <= first_atom[b]) { snprintf(msg, msg_len, "%s: body %d is empty (first_atom)", who, b); return false; }
        if (first_atom[b + 1] >= (1ll << 31)) { snprintf(msg, msg_len, "%s: first_atom: 2^31 atoms or more", who); return false; }
    }
    P.n_bodies = n_bodies;
    P.n_atoms = first_atom[n_bodies];
    if (!jf_taps(resolution, vs, &P.r, &P.sig, P.taps)) {
        snprintf(msg, msg_len, "%s: resolution = %g at spacing %g: a blur of more than %d voxels", who, resolution, vs, JF_MAX_R);
        return false;
    }
    P.vox0[0] = 0; P.max_box = 0; P.max_atoms = 0;
    for (int b = 0; b < n_bodies; b++) {
        const int64_t a0 = first_atom[b], n = first_atom[b + 1] - a0;
        double c[3] = {0, 0, 0};
        for (int64_t i = a0; i < a0 + n; i++) {
            if (!std::isfinite(mass[i])) { snprintf(msg, msg_len, "%s: mass of atom %lld is not finite", who, (long long)i); return false; }
            for (int d = 0; d < 3; d++) {
                const double v = atoms[3 * i + d];
                if (!std::isfinite(v) || !(fabs(v) < 1e12)) { snprintf(msg, msg_len, "%s: atoms: coordinate of atom %lld is not finite", who, (long long)i); return false; }
                c[d] += v;
            }
        }
        double md = 0;
        for (int d = 0; d < 3; d++) c[d] /= (double)n;
        for (int64_t i = a0; i < a0 + n; i++) {
            const double x = atoms[3 * i] - c[0], y = atoms[3 * i + 1] - c[1], z = atoms[3 * i + 2] - c[2];
            md = fmax(md, sqrt(x * x + y * y + z * z));
        }
        P.max_dist[b] = md;
        P.edge[b] = jf_box_edge(md, P.r, vs, max_step);
        if (P.edge[b] < 0) { snprintf(msg, msg_len, "%s: atoms: body %d spans %g A around its centre", who, b, md); return false; }
        int64_t vox = 1;
        for (int d = 0; d < 3; d++) {
            P.cen[b][d] = c[d];
            P.e[b][d] = jf_box_extent(P.edge[b], dims[d]);
            P.lo[b][d] = jf_box_lo(c[d], origin[d], vs, P.edge[b], dims[d]);
            vox *= P.e[b][d];
        }
        P.vox0[b + 1] = P.vox0[b] + vox;
        if (vox > P.max_box) P.max_box = vox;
        if (n > P.max_atoms) P.max_atoms = n;
    }
    return true;
}

// ---------------------------------------------------------------------------
// mad_assembly_refine_symmetric: units under the operators of a point group
// ---------------------------------------------------------------------------
#define JF_SYM_MAX_MEMBERS (JF_MAX_BODIES * JF_MAX_G)      // workgroups of a unit's reduction group at most (K G; a launch has n_cu at most)
#define JF_SYM_ORTHO_TOL 1e-6                              // |R R^T - I| in every entry

// q = p R + T for row vectors, R row-major: ((x R[0][j] + y R[1][j]) + z R[2][j]) + T[j]
JF_HD static inline void jf_image(const double *R, const double *T, const double p[3], double q[3]) {
    for (int j = 0; j < 3; j++) q[j] = ((p[0] * R[j] + p[1] * R[3 + j]) + p[2] * R[6 + j]) + T[j];
}
// h = g R^T: a gradient gathered at the image, in the unit's frame
JF_HD static inline void jf_pull_back(const double *R, const double g[3], double h[3]) {
    for (int i = 0; i < 3; i++) h[i] = (g[0] * R[3 * i] + g[1] * R[3 * i + 1]) + g[2] * R[3 * i + 2];
}

// false with a message: n_units, n_ops, their product, or an operator is refused
static inline bool jf_ops_check(const char *who, int32_t n_units, int32_t n_ops, const double *op_rot, const double *op_trans, char *msg,
                                size_t msg_len) {
    if (n_units < 1 || n_units > JF_MAX_BODIES) { snprintf(msg, msg_len, "%s: n_units = %d (1 .. %d)", who, n_units, JF_MAX_BODIES); return false; }
    if (n_ops < 1 || n_ops > JF_MAX_BODIES) { snprintf(msg, msg_len, "%s: n_ops = %d (1 .. %d)", who, n_ops, JF_MAX_BODIES); return false; }
    if (n_units * n_ops > JF_MAX_BODIES) {
        snprintf(msg, msg_len, "%s: n_units x n_ops = %d images (%d at most)", who, n_units * n_ops, JF_MAX_BODIES);
        return false;
    }
    if (!op_rot) { snprintf(msg, msg_len, "%s: NULL op_rot", who); return false; }
    if (!op_trans) { snprintf(msg, msg_len, "%s: NULL op_trans", who); return false; }
    for (int i = 0; i < 9; i++)
        if (op_rot[i] != ((i % 4 == 0) ? 1.0 : 0.0)) { snprintf(msg, msg_len, "%s: op_rot: operator 0 is not the identity", who); return false; }
    for (int i = 0; i < 3; i++)
        if (op_trans[i] != 0.0) { snprintf(msg, msg_len, "%s: op_trans: operator 0 is not the identity", who); return false; }
    for (int g = 0; g < n_ops; g++) {
        const double *R = op_rot + 9 * g, *T = op_trans + 3 * g;
        for (int i = 0; i < 9; i++)
            if (!std::isfinite(R[i])) { snprintf(msg, msg_len, "%s: op_rot: operator %d is not finite", who, g); return false; }
        for (int i = 0; i < 3; i++)
            if (!std::isfinite(T[i]) || !(fabs(T[i]) < 1e12)) { snprintf(msg, msg_len, "%s: op_trans: operator %d is not finite", who, g); return false; }
        for (int i = 0; i < 3; i++)
            for (int k = 0; k < 3; k++) {
                const double d = (R[3 * i] * R[3 * k] + R[3 * i + 1] * R[3 * k + 1]) + R[3 * i + 2] * R[3 * k + 2];
                if (!(fabs(d - (i == k ? 1.0 : 0.0)) <= JF_SYM_ORTHO_TOL)) {
                    snprintf(msg, msg_len, "%s: op_rot: operator %d is not orthonormal (|R R^T - I| above %g)", who, g, JF_SYM_ORTHO_TOL);
                    return false;
                }
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(det > 0.0)) { snprintf(msg, msg_len, "%s: op_rot: operator %d is a reflection (determinant %g)", who, g, det); return false; }
    }
    return true;
}

// The plan of the n_units x n_ops images as bodies: image (u, g) is body u n_ops + g.  The units are checked as jf_plan checks
// bodies; an image's box has its unit's edge and is placed around the image of the unit's centre.  P.n_atoms counts the atoms of
// all images, P.max_atoms those of the largest unit.
static inline bool jf_plan_sym(const char *who, const int32_t *dims, const double *origin, double vs, int32_t n_units, const double *atoms,
                               const double *mass, const int64_t *first_atom, int32_t n_ops, const double *op_rot, const double *op_trans,
                               double resolution, int32_t n_steps, double max_step, double min_step, JfPlan &P, char *msg, size_t msg_len) {
    if (!dims) { snprintf(msg, msg_len, "%s: no map: call mad_upload_density first", who); return false; }
    if (!jf_ops_check(who, n_units, n_ops, op_rot, op_trans, msg, msg_len)) return false;
    if (!jf_plan(who, dims, origin, vs, n_units, atoms, mass, first_atom, resolution, true, n_steps, max_step, min_step, P, msg, msg_len)) return false;
    const int32_t K = n_ops;
    for (int u = n_units - 1; u >= 0; u--)      // descending: body u K + g >= u is written after unit u was read
        for (int g = K - 1; g >= 0; g--) {
            const int b = u * K + g;
            const double c[3] = {P.cen[u][0], P.cen[u][1], P.cen[u][2]};
            const double md = P.max_dist[u];
            const int32_t edge = P.edge[u];
            double q[3] = {c[0], c[1], c[2]};
            if (g > 0) jf_image(op_rot + 9 * g, op_trans + 3 * g, c, q);
            P.max_dist[b] = md; P.edge[b] = edge;
            for (int d = 0; d < 3; d++) {
                P.cen[b][d] = q[d];
                P.e[b][d] = jf_box_extent(edge, dims[d]);
                P.lo[b][d] = jf_box_lo(q[d], origin[d], vs, edge, dims[d]);
            }
        }
    P.n_bodies = n_units * K;
    P.n_atoms *= K;
    P.vox0[0] = 0;
    for (int b = 0; b < P.n_bodies; b++) P.vox0[b + 1] = P.vox0[b] + (int64_t)P.e[b][0] * P.e[b][1] * P.e[b][2];
    return true;
}
