// mad_localfilter_plan.h -- the host side of mad_map_local_filter: the argument checks, the scan of the
// resolution samples, and the arithmetic of tiles, halos and slabs that the kernel shares.  Plain C++ without a HIP type, so that it
// also compiles into a stand-alone host program (check_localfilter_plan.cpp) for a host sanitizer.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define LF_HD __host__ __device__
#else
#define LF_HD
#endif

#define LF_TX 8                      // a workgroup's tile of outputs: 8 x 8 x 32 voxels
#define LF_TY 8
#define LF_TZ 32
#define LF_THREADS 512               // thread t: z = t % 32, y = t / 32 % 8, x = t / 256 * 4 + (0 .. 3): four outputs each
#define LF_PER_THREAD (LF_TX * LF_TY * LF_TZ / LF_THREADS)
#define LF_MAX_SIGMA 6.0             // voxels: fourier.LOCAL_FILTER_MAX_SIGMA
#define LF_MAX_R 24                  // = lf_radius(LF_MAX_SIGMA)
#define LF_LDS_BYTES (160 * 1024)    // what a workgroup may ask for on gfx950
// dynamic LDS, in this order: the partial sums S [LF_PER_THREAD][LF_THREADS] float64, 16 bytes of control words, the staged planes
#define LF_LDS_SUMS (LF_PER_THREAD * LF_THREADS * 8)
#define LF_LDS_HEAD (LF_LDS_SUMS + 16)
#define LF_ROUND (1u << 21)          // workgroups of one launch: LF_ROUND * LF_THREADS = 2^30 threads (a grid may not have 2^32)

static_assert(LF_TX * LF_TY * LF_TZ % LF_THREADS == 0 && LF_THREADS % (LF_TY * LF_TZ) == 0, "whole outputs per thread, whole x planes per pass");
static_assert(LF_TZ == 32, "a wavefront is two z rows of the tile: its LDS reads of a tap are two runs of 32 consecutive floats");

// The taps of the contract reach R = max(1, (int)(4 sigma + 0.5)) voxels to either side: mad_map_smooth's truncation (seg_taps in
// mad_segment.hip), with a floor of one voxel.  sigma <= LF_MAX_SIGMA on every call that is not refused.
LF_HD static inline int lf_radius(double sigma) {
    const int r = (int)(4.0 * sigma + 0.5);
    return r < 1 ? 1 : (r > LF_MAX_R ? LF_MAX_R : r);
}

// A tile whose largest radius is H is staged with a halo of H voxels: planes of (LF_TY + 2 H) rows of (LF_TZ + 2 H) floats, of which
// the tile needs LF_TX + 2 H along x.  As many of them as `lds_bytes` holds behind the head are staged at a time (a slab).
struct LfSlab {
    int py, pz;        // rows of a plane, floats of a row
    int planes;        // planes of one slab (>= 1)
    int n_slabs;       // slabs that cover LF_TX + 2 H planes
};
LF_HD static inline LfSlab lf_slab(int H, unsigned lds_bytes) {
    LfSlab s;
    s.py = LF_TY + 2 * H;
    s.pz = LF_TZ + 2 * H;
    const int need = LF_TX + 2 * H, fit = (int)((lds_bytes - LF_LDS_HEAD) / ((unsigned)(s.py * s.pz) * 4u));
    s.planes = fit < need ? fit : need;
    s.n_slabs = s.planes > 0 ? (need + s.planes - 1) / s.planes : 0;
    return s;
}
// dynamic LDS a launch needs when no tile's radius exceeds H: everything at once where that fits, else all there is
static inline unsigned lf_lds_bytes(int H) {
    const unsigned long long all = (unsigned long long)LF_LDS_HEAD + (unsigned long long)(LF_TX + 2 * H) * (LF_TY + 2 * H) * (LF_TZ + 2 * H) * 4ull;
    return all < LF_LDS_BYTES ? (unsigned)((all + 15) & ~15ull) : (unsigned)LF_LDS_BYTES;
}
static_assert((LF_LDS_BYTES - LF_LDS_HEAD) / ((LF_TY + 2 * LF_MAX_R) * (LF_TZ + 2 * LF_MAX_R) * 4) >= 1, "a plane of the widest halo fits");

struct LfPlan {
    int32_t n[3] = {0, 0, 0};          // the grid
    int32_t m[3] = {0, 0, 0};          // the sample lattice
    int32_t step = 1;
    double inv = 0.0;                  // voxsp * K: sigma = d / inv
    size_t n_vox = 0, n_res = 0;
    double sigma_max = 0.0;            // of the samples, hence of every voxel (trilinear interpolation is convex)
    int H = 1;                         // lf_radius(sigma_max)
    unsigned lds = 0;                  // lf_lds_bytes(H)
    unsigned tiles[3] = {0, 0, 0};
    unsigned long long n_tiles = 0;
};

enum { LF_OK = 0, LF_EINVAL = 1, LF_EDOM = 2 };

// LF_OK, or what the contract refuses with a message in msg (NULL pointers are the caller's).  K = pi sqrt(2) from the caller.
static inline int lf_plan(const int32_t dims[3], double voxsp, const double *res, const int32_t rdims[3], int32_t step, double K, LfPlan &P,
                          char *msg, size_t msg_len) {
    const char *who = "mad_map_local_filter";
    for (int a = 0; a < 3; a++)
        if (dims[a] < 1) { snprintf(msg, msg_len, "%s: grid of %d x %d x %d voxels", who, dims[0], dims[1], dims[2]); return LF_EINVAL; }
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 31) || vxy * (unsigned long long)dims[2] >= (1ull << 31)) {
        snprintf(msg, msg_len, "%s: %d x %d x %d voxels: grids of 2^31 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
        return LF_EINVAL;
    }
    if (step < 1) { snprintf(msg, msg_len, "%s: step %d (1 or more)", who, step); return LF_EINVAL; }
    if (!(voxsp > 0) || !std::isfinite(voxsp) || !std::isfinite(voxsp * K)) {
        snprintf(msg, msg_len, "%s: voxsp %g (positive and finite)", who, voxsp);
        return LF_EINVAL;
    }
    for (int a = 0; a < 3; a++) {
        P.n[a] = dims[a];
        P.m[a] = (dims[a] - 1) / step + 1;
    }
    if (rdims[0] != P.m[0] || rdims[1] != P.m[1] || rdims[2] != P.m[2]) {
        snprintf(msg, msg_len, "%s: rdims %d x %d x %d, the samples at every %d-th voxel of %d x %d x %d are %d x %d x %d", who, rdims[0], rdims[1],
                 rdims[2], step, dims[0], dims[1], dims[2], P.m[0], P.m[1], P.m[2]);
        return LF_EINVAL;
    }
    P.step = step;
    P.inv = voxsp * K;
    P.n_vox = (size_t)(vxy * (unsigned long long)dims[2]);
    P.n_res = (size_t)P.m[0] * (size_t)P.m[1] * (size_t)P.m[2];
    double top = 0.0;
    for (size_t i = 0; i < P.n_res; i++) {
        const double d = res[i];
        const int k = (int)(i % (size_t)P.m[2]), j = (int)(i / (size_t)P.m[2] % (size_t)P.m[1]), ii = (int)(i / (size_t)P.m[2] / (size_t)P.m[1]);
        if (!std::isfinite(d) || !(d > 0)) {
            snprintf(msg, msg_len, "%s: sample (%d, %d, %d) is %g A (positive and finite)", who, ii, j, k, d);
            return LF_EINVAL;
        }
        const double sigma = d / P.inv;
        if (!(sigma <= LF_MAX_SIGMA)) {
            snprintf(msg, msg_len, "%s: sample (%d, %d, %d) is %g A, a Gaussian of sigma %g voxels wide (at most %g)", who, ii, j, k, d, sigma,
                     (double)LF_MAX_SIGMA);
            return LF_EDOM;
        }
        top = sigma > top ? sigma : top;
    }
    P.sigma_max = top;
    P.H = lf_radius(top);
    P.lds = lf_lds_bytes(P.H);
    P.tiles[0] = (unsigned)((dims[0] + LF_TX - 1) / LF_TX);
    P.tiles[1] = (unsigned)((dims[1] + LF_TY - 1) / LF_TY);
    P.tiles[2] = (unsigned)((dims[2] + LF_TZ - 1) / LF_TZ);
    P.n_tiles = (unsigned long long)P.tiles[0] * P.tiles[1] * P.tiles[2];      // below 2^31: a tile holds a voxel
    return LF_OK;
}
