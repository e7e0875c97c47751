// mad_components_plan.h -- the host side of mad_map_components and mad_map_dust: the argument checks, the
// tiles, the forward half of a neighbourhood with the index expressions the two kernels form from it, and the selection rule of
// mad_map_dust (rank and ties).  Plain C++ without a HIP type, so that it also compiles into a stand-alone host program
// (check_components_plan.cpp) for a host sanitizer.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#if defined(__HIPCC__)
#define CC_HD __host__ __device__
#else
#define CC_HD
#endif

#define CC_THREADS 256
#define CC_TX 8                  // a workgroup's tile: 8 x 8 x 64 voxels, the tile of k_seg_parent (lanes along z)
#define CC_TY 8
#define CC_TZ 64
#define CC_TILE (CC_TX * CC_TY * CC_TZ)
#define CC_ROWS (CC_TX * CC_TY)

#define CC_BORDER_Y (CC_ROWS / (CC_THREADS / CC_TZ))      // workgroups of k_cc_border per tile: a z row per wavefront
#define CC_LABEL_PER 4096        // voxels of one workgroup of k_cc_label (16 rounds of CC_THREADS)
#define CC_LABEL_SLOTS 512       // (id, count) pairs it keeps in LDS: id & (CC_LABEL_SLOTS - 1) is an id's slot

static_assert(CC_TILE <= 65536, "a local index fits 16 bits");
static_assert(CC_ROWS % (CC_THREADS / CC_TZ) == 0 && CC_BORDER_Y <= 65535, "whole workgroups, and a legal grid");
static_assert(CC_LABEL_PER % CC_THREADS == 0, "whole rounds");
static_assert((CC_LABEL_SLOTS & (CC_LABEL_SLOTS - 1)) == 0, "a power of two: the slot is a mask");

// Offset (dx, dy, dz) in {-1, 0, 1}^3 belongs to the neighbourhood `conn` (6, 18, 26: 1, at most 2, at most 3 components that are not 0) ...
CC_HD static inline bool cc_is_neighbour(int dx, int dy, int dz, int conn) {
    const int nz = (dx != 0) + (dy != 0) + (dz != 0);
    return nz >= 1 && nz <= (conn == 6 ? 1 : (conn == 18 ? 2 : 3));
}
// ... and to its forward half: the neighbour's L is the larger one (lexicographic (dx, dy, dz) > 0).  3, 9 or 13 offsets; the other half
// is their mirror image, so every pair of neighbours is met once, from its member with the smaller L.
CC_HD static inline bool cc_is_forward(int dx, int dy, int dz, int conn) {
    return cc_is_neighbour(dx, dy, dz, conn) && (dx > 0 || (dx == 0 && (dy > 0 || (dy == 0 && dz > 0))));
}
// the local index of voxel (cx, cy, cz) of a tile: lexicographic, which is the order of L inside the tile
CC_HD static inline int cc_local(int cx, int cy, int cz) { return (cx * CC_TY + cy) * CC_TZ + cz; }
CC_HD static inline bool cc_in_tile(int cx, int cy, int cz) { return cx >= 0 && cx < CC_TX && cy >= 0 && cy < CC_TY && cz >= 0 && cz < CC_TZ; }
// A voxel at (cx, cy, cz) of its tile can have a forward neighbour in another tile (dx >= 0; dy = -1 only with dx = 1; dz any).
CC_HD static inline bool cc_row_on_face(int cx, int cy) { return cx == CC_TX - 1 || cy == 0 || cy == CC_TY - 1; }
CC_HD static inline bool cc_on_face(int cx, int cy, int cz) { return cc_row_on_face(cx, cy) || cz == 0 || cz == CC_TZ - 1; }

struct CcPlan {
    int32_t n[3] = {0, 0, 0};
    int32_t conn = 0;
    uint32_t n_vox = 0, bx = 0, by = 0, bz = 0, tiles = 0;
};

enum { CC_OK = 0, CC_EINVAL = 1 };

// CC_OK, or what the contract of both entries refuses with a message in msg (NULL pointers are the caller's).
static inline int cc_plan(const char *who, const int32_t dims[3], double threshold, int32_t connectivity, CcPlan &P, char *msg, size_t msg_len) {
    for (int a = 0; a < 3; a++)
        if (dims[a] < 1) { snprintf(msg, msg_len, "%s: grid of %d x %d x %d voxels", who, dims[0], dims[1], dims[2]); return CC_EINVAL; }
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 31) || vxy * (unsigned long long)dims[2] >= (1ull << 31)) {
        snprintf(msg, msg_len, "%s: %d x %d x %d voxels: grids of 2^31 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
        return CC_EINVAL;
    }
    if (threshold != threshold) { snprintf(msg, msg_len, "%s: the threshold is not a number", who); return CC_EINVAL; }
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) {
        snprintf(msg, msg_len, "%s: connectivity %d (6, 18 or 26)", who, connectivity);
        return CC_EINVAL;
    }
    for (int a = 0; a < 3; a++) P.n[a] = dims[a];
    P.conn = connectivity;
    P.n_vox = (uint32_t)(vxy * (unsigned long long)dims[2]);
    P.bx = ((uint32_t)dims[0] + CC_TX - 1u) / CC_TX;
    P.by = ((uint32_t)dims[1] + CC_TY - 1u) / CC_TY;
    P.bz = ((uint32_t)dims[2] + CC_TZ - 1u) / CC_TZ;
    P.tiles = P.bx * P.by * P.bz;      // a tile holds a voxel: fewer than 2^31
    return CC_OK;
}

// what mad_map_dust refuses beyond that
static inline int cc_dust_args(const char *who, double threshold, int64_t min_size, int64_t keep, float fill, char *msg, size_t msg_len) {
    if (min_size < 1 || keep < 0) {
        snprintf(msg, msg_len, "%s: min_size %lld, keep %lld (1 or more; 0 or more)", who, (long long)min_size, (long long)keep);
        return CC_EINVAL;
    }
    if (!std::isfinite(fill) || (double)fill > threshold) {
        snprintf(msg, msg_len, "%s: fill %g (finite and not above the threshold %g: it would be foreground again)", who, (double)fill, threshold);
        return CC_EINVAL;
    }
    return CC_OK;
}

// The selection of mad_map_dust: the n components ranked by size descending, root ascending (roots are distinct: a strict order);
// component c is kept iff size[c] >= min_size and (keep == 0 or its rank < keep).  flag[c] = 1 for a kept one, else 0;
// counts = {components, kept components, foreground voxels, kept voxels}.
static inline void cc_select(int64_t n, const int64_t *root, const int64_t *size, int64_t min_size, int64_t keep, std::vector<int32_t> &flag,
                             int64_t counts[4]) {
    flag.assign((size_t)n, 0);
    std::vector<int64_t> order((size_t)n);
    for (int64_t c = 0; c < n; c++) order[(size_t)c] = c;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return size[a] != size[b] ? size[a] > size[b] : root[a] < root[b]; });
    counts[0] = n; counts[1] = 0; counts[2] = 0; counts[3] = 0;
    for (int64_t rank = 0; rank < n; rank++) {
        const int64_t c = order[(size_t)rank];
        counts[2] += size[c];
        if (size[c] >= min_size && (keep == 0 || rank < keep)) {
            flag[(size_t)c] = 1;
            counts[1]++;
            counts[3] += size[c];
        }
    }
}
