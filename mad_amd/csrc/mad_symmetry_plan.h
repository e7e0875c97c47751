// mad_symmetry_plan.h -- the host side of mad_map_symmetry_score: the argument checks, the box of sample points
// around the ball, its runs of 256, the levels of the sums, the operators per workgroup and the chunks of operators under a scratch
// budget.  Plain C++ without a HIP type, so that it also compiles into a stand-alone host program (check_symmetry_plan.cpp); the
// function the kernel shares with that program carries SYM_HD.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define SYM_HD __host__ __device__
#else
#define SYM_HD
#endif

#define SYM_RUN 256             // points of a run of tree_sum (fourier.py), and the workgroup of the kernels
#define SYM_OPS_WG 8            // operators a workgroup of k_sym_score takes over its run
#define SYM_MAX_LEVELS 4        // levels of 256 that reduce the runs of a box of fewer than 2^32 points to one record
#define SYM_REC 3               // doubles of a partial record: (sum b, sum b^2, sum a b) of an operator, (n, sum a, sum a^2) of the points
#define SYM_MAX_BATCHES 65535   // gridDim.y

// The sample points: candidate (kx, ky, kz) of the box is lattice index j_a = stride (lo_a + k_a), point i = (kx nb_1 + ky) nb_2 + kz.
struct SymBox {
    int32_t n[3];               // voxels of the grid
    int32_t stride;
    int32_t lo[3], nb[3];       // first multiple and count per axis (nb = 0 on every axis: the box is empty)
    double c[3], r2;            // the ball's centre in voxels and its squared radius in voxels
    uint64_t n_box;             // nb_0 nb_1 nb_2 < 2^32
    uint32_t n_runs;            // ceil(n_box / 256)
};

struct SymPlan {
    SymBox box;
    double r;                                   // the radius in voxels
    int32_t n_levels;                           // reduction launches behind k_sym_score: level l turns level_n[l] records into level_n[l + 1]
    uint32_t level_n[SYM_MAX_LEVELS + 2];       // level_n[0] = n_runs ... level_n[n_levels] = 1
    int32_t n_ops, ops_chunk, n_chunks;         // operators of a chunk (the last may hold fewer), chunks
    uint64_t rec_a, rec_b;                      // records per slot of the two buffers; a chunk has ops_chunk + 1 slots (the last: the points' own sums)
    uint64_t scratch_bytes;                     // both buffers of a chunk
};

// point i < n_box of the box -> its lattice index j (always inside the grid); true: it lies in the ball and counts
SYM_HD static inline bool sym_point(const SymBox &B, uint64_t i, int32_t j[3]) {
    const uint32_t q = (uint32_t)i, kz = q % (uint32_t)B.nb[2], t = q / (uint32_t)B.nb[2], ky = t % (uint32_t)B.nb[1], kx = t / (uint32_t)B.nb[1];
    j[0] = B.stride * (B.lo[0] + (int32_t)kx);
    j[1] = B.stride * (B.lo[1] + (int32_t)ky);
    j[2] = B.stride * (B.lo[2] + (int32_t)kz);
    const double dx = (double)j[0] - B.c[0], dy = (double)j[1] - B.c[1], dz = (double)j[2] - B.c[2];
    return ((dx * dx + dy * dy) + dz * dz) <= B.r2;
}

// candidate k of an axis belongs to the box: |stride k - c| <= r
static inline bool sym_in_box(int64_t k, int32_t stride, double c, double r) { return fabs((double)(stride * k) - c) <= r; }

static inline int64_t sym_clamp(double v, int64_t lo, int64_t hi) { return v < (double)lo ? lo : (v > (double)hi ? hi : (int64_t)v); }

// The k of one axis with |stride k - c| <= r and 0 <= stride k <= n - 1: first and count.  The exact first and last lie within two
// of the real-number bounds (c -+ r) / stride (every quantity is below 2^32 where it matters, the roundings are of relative size
// 2^-53), so five candidates around each bound decide; a bound outside 0 .. kmax is clamped onto it first.
static inline void sym_axis(int32_t n, int32_t stride, double c, double r, int32_t *first, int32_t *count) {
    const int64_t kmax = (int64_t)(n - 1) / stride;
    const double s = (double)stride;
    const double el = floor((c - r) / s), eh = ceil((c + r) / s);
    int64_t lo = -1, hi = -1;
    for (int64_t k = sym_clamp(el - 2.0, 0, kmax); k <= sym_clamp(el + 2.0, 0, kmax); k++)
        if (sym_in_box(k, stride, c, r)) { lo = k; break; }
    for (int64_t k = sym_clamp(eh + 2.0, 0, kmax); k >= sym_clamp(eh - 2.0, 0, kmax); k--)
        if (sym_in_box(k, stride, c, r)) { hi = k; break; }
    if (lo < 0 || hi < lo) { *first = 0; *count = 0; return; }
    *first = (int32_t)lo;
    *count = (int32_t)(hi - lo + 1);
}

// false with a message in msg: the call is refused.  Everything the contract refuses is refused here except a NULL ctx, grid, operator
// table or output and an R that is no rotation (the caller's: mad_resample_taps.h).  budget: bytes of partial records a chunk of
// operators may take; a chunk holds at least one operator, so one operator's records are the floor of what a call needs.
static inline bool sym_plan(const int32_t dims[3], const double origin[3], double voxsp, const double centre[3], double radius, int32_t stride,
                            int32_t n_ops, int64_t budget, SymPlan &P, char *msg, size_t msg_len) {
    const char *who = "mad_map_symmetry_score";
    if (!dims || !origin || !centre) { snprintf(msg, msg_len, "%s: NULL argument", who); return false; }
    if (n_ops < 1) { snprintf(msg, msg_len, "%s: %d operators (1 or more)", who, n_ops); return false; }
    if (stride < 1) { snprintf(msg, msg_len, "%s: stride %d (1 or more)", who, stride); return false; }
    for (int k = 0; k < 3; k++)
        if (dims[k] < 2) { snprintf(msg, msg_len, "%s: grid of %d x %d x %d voxels: every axis needs 2", who, dims[0], dims[1], dims[2]); return false; }
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 32) || vxy * (unsigned long long)dims[2] >= (1ull << 32)) {
        snprintf(msg, msg_len, "%s: %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
        return false;
    }
    if (!std::isfinite(voxsp) || !std::isfinite(radius) || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]) ||
        !std::isfinite(centre[0]) || !std::isfinite(centre[1]) || !std::isfinite(centre[2])) {
        snprintf(msg, msg_len, "%s: a number that is not finite", who);
        return false;
    }
    if (!(voxsp > 0)) { snprintf(msg, msg_len, "%s: voxsp %g", who, voxsp); return false; }
    if (radius < 0) { snprintf(msg, msg_len, "%s: radius %g is negative", who, radius); return false; }
    if (budget < 1) budget = 1;
    SymBox &B = P.box;
    P.r = radius / voxsp;
    B.r2 = P.r * P.r;
    B.stride = stride;
    for (int a = 0; a < 3; a++) {
        B.n[a] = dims[a];
        B.c[a] = (centre[a] - origin[a]) / voxsp;
    }
    if (!std::isfinite(P.r) || !std::isfinite(B.r2) || !std::isfinite(B.c[0]) || !std::isfinite(B.c[1]) || !std::isfinite(B.c[2])) {
        snprintf(msg, msg_len, "%s: the ball in voxels is too large for float64", who);
        return false;
    }
    bool empty = false;
    for (int a = 0; a < 3; a++) {
        sym_axis(dims[a], stride, B.c[a], P.r, &B.lo[a], &B.nb[a]);
        empty = empty || B.nb[a] == 0;
    }
    if (empty)
        for (int a = 0; a < 3; a++) B.lo[a] = B.nb[a] = 0;
    B.n_box = (uint64_t)B.nb[0] * (uint64_t)B.nb[1] * (uint64_t)B.nb[2];      // at most the grid's voxels: < 2^32
    B.n_runs = (uint32_t)((B.n_box + SYM_RUN - 1) / SYM_RUN);
    P.n_levels = 0;
    for (int l = 0; l < SYM_MAX_LEVELS + 2; l++) P.level_n[l] = 0;
    P.level_n[0] = B.n_runs;
    while (P.level_n[P.n_levels] > 1) {
        P.level_n[P.n_levels + 1] = (P.level_n[P.n_levels] + SYM_RUN - 1) / SYM_RUN;
        P.n_levels++;
    }
    P.rec_a = B.n_runs;
    P.rec_b = P.n_levels > 0 ? P.level_n[1] : 0;
    const uint64_t per_slot = (P.rec_a + P.rec_b) * SYM_REC * sizeof(double);
    P.n_ops = n_ops;
    int64_t chunk = per_slot ? (int64_t)((uint64_t)budget / per_slot) - 1 : n_ops;      // one slot is the points' own
    if (chunk > (int64_t)SYM_MAX_BATCHES * SYM_OPS_WG) chunk = (int64_t)SYM_MAX_BATCHES * SYM_OPS_WG;
    if (chunk > n_ops) chunk = n_ops;
    if (chunk > SYM_OPS_WG && chunk < n_ops) chunk -= chunk % SYM_OPS_WG;      // whole workgroups in every chunk but the last
    if (chunk < 1) chunk = 1;
    P.ops_chunk = (int32_t)chunk;
    P.n_chunks = B.n_box ? (n_ops + P.ops_chunk - 1) / P.ops_chunk : 0;
    P.scratch_bytes = (uint64_t)(P.ops_chunk + 1) * per_slot;
    return true;
}
