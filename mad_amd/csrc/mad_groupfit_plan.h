// mad_groupfit_plan.h -- the host side of mad_map_group_fit: the argument checks and the work list.  Plain
// C++ without a HIP type, so that it also compiles into a stand-alone host program.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define GF_BX 8                 // a workgroup's brick is 8 x 8 x 16 voxels, a lane's share 1 x 1 x 4
#define GF_BY 8
#define GF_BZ 16

struct GfPlan {
    long long s[3] = {0, 0, 0};            // voxel j of grid 1 is voxel j - s of grid 2
    std::vector<int32_t> items;            // per item {group, x0, y0, z0}: the first voxel of its brick
    std::vector<uint32_t> first_item;      // [n_groups + 1]: group g owns the items first_item[g] .. first_item[g + 1] - 1
};

// false with a message in msg: the call is refused.  Everything the contract refuses is refused here except NULL ctx, grids and
// outputs (the caller's).  With true, P holds the shift and the work list, group-major, a group's bricks z fastest.
static inline bool gf_plan(const int32_t dims1[3], const double origin1[3], const int32_t dims2[3], const double origin2[3], double voxsp,
                           const double *atoms, const int64_t *first_atom, int32_t n_groups, double radius, double isovalue, GfPlan &P,
                           char *msg, size_t msg_len) {
    const char *who = "mad_map_group_fit";
    if (!dims1 || !origin1 || !dims2 || !origin2 || !first_atom) { snprintf(msg, msg_len, "%s: NULL argument", who); return false; }
    if (n_groups < 0) { snprintf(msg, msg_len, "%s: %d groups", who, n_groups); return false; }
    for (int t = 0; t < 2; t++) {
        const int32_t *d = t ? dims2 : dims1;
        for (int k = 0; k < 3; k++)
            if (d[k] < 1) { snprintf(msg, msg_len, "%s: grid %d of %d x %d x %d voxels", who, t + 1, d[0], d[1], d[2]); return false; }
        const unsigned long long vxy = (unsigned long long)d[0] * (unsigned long long)d[1];
        if (vxy >= (1ull << 32) || vxy * (unsigned long long)d[2] >= (1ull << 32)) {
            snprintf(msg, msg_len, "%s: grid %d of %d x %d x %d voxels: 2^32 voxels or more are not supported", who, t + 1, d[0], d[1], d[2]);
            return false;
        }
    }
    bool finite = std::isfinite(voxsp) && std::isfinite(radius) && std::isfinite(isovalue);
    for (int a = 0; a < 3; a++) finite = finite && std::isfinite(origin1[a]) && std::isfinite(origin2[a]);
    if (!finite) { snprintf(msg, msg_len, "%s: a number that is not finite", who); return false; }
    if (!(voxsp > 0)) { snprintf(msg, msg_len, "%s: voxsp %g", who, voxsp); return false; }
    if (radius < 0 || isovalue < 0) { snprintf(msg, msg_len, "%s: radius %g, isovalue %g (neither may be negative)", who, radius, isovalue); return false; }
    if (first_atom[0] != 0) { snprintf(msg, msg_len, "%s: first_atom[0] = %lld, not 0", who, (long long)first_atom[0]); return false; }
    for (int32_t g = 0; g < n_groups; g++)
        if (first_atom[g + 1] < first_atom[g]) { snprintf(msg, msg_len, "%s: first_atom decreases at group %d", who, g); return false; }
    const int64_t n_atoms = first_atom[n_groups];
    if (n_atoms >= (1ll << 31)) { snprintf(msg, msg_len, "%s: %lld atoms: 2^31 or more are not supported", who, (long long)n_atoms); return false; }
    if (n_atoms > 0 && !atoms) { snprintf(msg, msg_len, "%s: NULL atoms", who); return false; }
    for (int a = 0; a < 3; a++) {
        const double d = origin2[a] / voxsp - origin1[a] / voxsp;
        if (!std::isfinite(d)) { snprintf(msg, msg_len, "%s: the offset between the grids in voxels is not finite", who); return false; }
        const double r = nearbyint(d);      // half to even, python's round()
        P.s[a] = r > 0x1p40 ? (1ll << 40) : (r < -0x1p40 ? -(1ll << 40) : (long long)r);      // beyond 2^32 either way: no common voxel
    }

    P.items.clear();
    P.first_item.assign((size_t)n_groups + 1, 0u);
    unsigned long long n_items = 0;
    for (int32_t g = 0; g < n_groups; g++) {
        P.first_item[g] = (uint32_t)n_items;
        const int64_t a0 = first_atom[g], a1 = first_atom[g + 1];
        if (a0 == a1) continue;
        double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int64_t i = a0; i < a1; i++)
            for (int a = 0; a < 3; a++) {
                const double v = atoms[3 * i + a];
                if (!std::isfinite(v)) { snprintf(msg, msg_len, "%s: atom %lld has a coordinate that is not finite", who, (long long)i); return false; }
                mn[a] = v < mn[a] ? v : mn[a];
                mx[a] = v > mx[a] ? v : mx[a];
            }
        // The index box: every voxel that can be within `radius` of the atoms' box.  A member has |p_a - x_a| <= radius up to a few
        // roundings of numbers no larger than `scale`, about 2^-50 scale / voxsp voxels: one spare voxel on every side covers that
        // for any scale below 2^48 voxsp, and beyond the spare grows with it.  A wider box costs time, never a voxel: the kernel
        // decides every voxel of a brick by the contract's own expression.
        long lo[3], hi[3];
        bool empty = false;
        for (int a = 0; a < 3; a++) {
            const double last = origin1[a] + voxsp * (double)(dims1[a] - 1);
            const double scale = fmax(fmax(fabs(origin1[a]), fabs(last)), fmax(fabs(mn[a]), fabs(mx[a])) + radius);
            const double spare = 1.0 + fmin(floor(scale * 0x1p-48 / voxsp), 0x1p31);
            const double flo = floor((mn[a] - radius - origin1[a]) / voxsp) - spare, fhi = ceil((mx[a] + radius - origin1[a]) / voxsp) + spare;
            const double top = (double)(dims1[a] - 1);
            if (!(flo <= top) || !(fhi >= 0.0)) { empty = true; break; }
            lo[a] = flo < 0.0 ? 0 : (long)flo;
            hi[a] = fhi > top ? (long)top : (long)fhi;
        }
        if (empty) continue;
        lo[2] &= ~3l;      // bricks begin at a multiple of 4 along z, so that a lane's four voxels can be one 16-byte load
        const unsigned long long nb[3] = {(unsigned long long)((hi[0] - lo[0]) / GF_BX + 1), (unsigned long long)((hi[1] - lo[1]) / GF_BY + 1),
                                          (unsigned long long)((hi[2] - lo[2]) / GF_BZ + 1)};      // each below 2^31, the product below 2^32
        n_items += nb[0] * nb[1] * nb[2];
        if (n_items >= (1ull << 31)) { snprintf(msg, msg_len, "%s: a work list of 2^31 bricks or more", who); return false; }
        for (unsigned long long bx = 0; bx < nb[0]; bx++)
            for (unsigned long long by = 0; by < nb[1]; by++)
                for (unsigned long long bz = 0; bz < nb[2]; bz++) {
                    P.items.push_back(g);
                    P.items.push_back((int32_t)(lo[0] + (long)bx * GF_BX));
                    P.items.push_back((int32_t)(lo[1] + (long)by * GF_BY));
                    P.items.push_back((int32_t)(lo[2] + (long)bz * GF_BZ));
                }
    }
    P.first_item[n_groups] = (uint32_t)n_items;
    return true;
}
