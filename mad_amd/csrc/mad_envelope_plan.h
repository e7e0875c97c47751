// mad_envelope_plan.h -- the host side of mad_map_envelope: the argument checks, the window Rv, the units of
// the pass along z with the indices of its LDS window, and the saturating step of the min-plus that every pass shares.  Plain C++
// without a HIP type, so that it also compiles into a stand-alone host program (check_envelope_plan.cpp) for a host sanitizer.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define ENV_HD __host__ __device__
#else
#define ENV_HD
#endif

#define ENV_SENT 0x7fffffffu         // INT32_MAX: "no seed within the window"
#define ENV_MAX_RV 255               // 3 * 255^2 is far inside int32, and the window stays a sane size
#define ENV_THREADS 256
#define ENV_SEG 64                   // pass along z: a wavefront takes 64 consecutive outputs of one line
#define ENV_WAVES (ENV_THREADS / ENV_SEG)
#define ENV_ZW (ENV_SEG + 2 * ENV_MAX_RV + 2)      // int32 of one wavefront's window, the widest halo on either side (576: 2 304 bytes)
#define ENV_WGS 512                  // workgroups of the weight kernel = partial tallies, whatever the grid

static_assert(ENV_SEG + 2 * ENV_MAX_RV <= ENV_ZW, "the widest window fits its LDS row");
static_assert(3ll * ENV_MAX_RV * ENV_MAX_RV < 0x7fffffffll, "a squared distance inside the window is an int32");
static_assert((unsigned long long)ENV_SENT + (unsigned long long)ENV_MAX_RV * ENV_MAX_RV < (1ull << 32), "sentinel + tap stays a uint32");

// One step of the min-plus: the running minimum m against v + t, v an entry (a squared distance or the sentinel), t = j * j <=
// ENV_MAX_RV^2.  Unsigned, so that the sentinel plus a tap does not wrap (static_assert above); the result is cut back to the
// sentinel, which is how the sum saturates.
ENV_HD static inline unsigned env_step(unsigned m, unsigned v, unsigned t) {
    const unsigned c = v + t;
    const unsigned s = c < ENV_SENT ? c : ENV_SENT;
    return s < m ? s : m;
}

// out = min over |j| <= Rv of win[c + j] + j * j, walked outward from j = 0 and left once j * j is no smaller than the running
// minimum: no later tap can lower it.  win[c - Rv .. c + Rv] must exist; entries beyond the line's ends hold the sentinel.
ENV_HD static inline unsigned env_walk(const unsigned *win, int c, int Rv) {
    unsigned m = env_step(ENV_SENT, win[c], 0u);
    for (int j = 1; j <= Rv; j++) {
        const unsigned t = (unsigned)(j * j);
        if (t >= m) break;
        m = env_step(m, win[c - j], t);
        m = env_step(m, win[c + j], t);
    }
    return m;
}

// The pass along z: unit u = line * segs + seg is the outputs z0 .. z0 + ENV_SEG - 1 of one line, z0 = seg * ENV_SEG; its window
// holds z0 - Rv .. z0 + ENV_SEG - 1 + Rv at the indices 0 .. env_win_len(Rv) - 1, output lane l at index l + Rv.
ENV_HD static inline int env_win_len(int Rv) { return ENV_SEG + 2 * Rv; }
ENV_HD static inline int env_win_centre(int lane, int Rv) { return lane + Rv; }
ENV_HD static inline unsigned env_segs(int nz) { return ((unsigned)nz + ENV_SEG - 1u) / ENV_SEG; }

struct EnvPlan {
    int32_t n[3] = {0, 0, 0};
    int32_t Rv = 0;
    uint32_t n_vox = 0, n_lines = 0, segs = 0;
    unsigned long long units = 0;      // of the pass along z: n_lines * segs
    uint32_t wgs_z = 0, wgs_flat = 0;  // workgroups of the pass along z; of the passes along y and x
    double voxsp = 0, extend = 0, soft = 0, vv = 0, r2 = 0, R = 0, R2 = 0;
    uint32_t Rv2 = 0;
};

enum { ENV_OK = 0, ENV_EINVAL = 1, ENV_EDOM = 2 };

// ENV_OK, or what the contract refuses with a message in msg (NULL pointers are the caller's).
static inline int env_plan(const int32_t dims[3], double voxsp, double threshold, double extend, double soft, EnvPlan &P, char *msg,
                           size_t msg_len) {
    const char *who = "mad_map_envelope";
    int top = 0;
    for (int a = 0; a < 3; a++) {
        if (dims[a] < 1) { snprintf(msg, msg_len, "%s: grid of %d x %d x %d voxels", who, dims[0], dims[1], dims[2]); return ENV_EINVAL; }
        top = dims[a] > top ? dims[a] : top;
    }
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 31) || vxy * (unsigned long long)dims[2] >= (1ull << 31)) {
        snprintf(msg, msg_len, "%s: %d x %d x %d voxels: grids of 2^31 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
        return ENV_EINVAL;
    }
    if (!(voxsp > 0) || !std::isfinite(voxsp) || !std::isfinite(voxsp * voxsp) || !(voxsp * voxsp > 0)) {
        snprintf(msg, msg_len, "%s: voxsp %g (positive and finite, its square too)", who, voxsp);
        return ENV_EINVAL;
    }
    if (threshold != threshold) { snprintf(msg, msg_len, "%s: the threshold is not a number", who); return ENV_EINVAL; }
    if (!std::isfinite(extend) || !std::isfinite(soft) || extend < 0 || soft < 0 || !std::isfinite(extend + soft) ||
        !std::isfinite((extend + soft) * (extend + soft))) {
        snprintf(msg, msg_len, "%s: extend %g, soft %g (finite, neither negative)", who, extend, soft);
        return ENV_EINVAL;
    }
    // Rv = min(floor((extend + soft) / voxsp) + 1, max(dims) - 1), judged in float64 before anything becomes an int
    const double reach = floor((extend + soft) / voxsp) + 1.0;
    const int Rv = reach < (double)(top - 1) ? (int)reach : top - 1;
    if (Rv > ENV_MAX_RV) {
        snprintf(msg, msg_len, "%s: extend %g + soft %g at voxsp %g is a window of %d voxels to either side (at most %d)", who, extend, soft,
                 voxsp, Rv, ENV_MAX_RV);
        return ENV_EDOM;
    }
    for (int a = 0; a < 3; a++) P.n[a] = dims[a];
    P.Rv = Rv;
    P.Rv2 = (uint32_t)(Rv * Rv);
    P.n_vox = (uint32_t)(vxy * (unsigned long long)dims[2]);
    P.n_lines = (uint32_t)vxy;
    P.segs = env_segs(dims[2]);
    P.units = (unsigned long long)P.n_lines * P.segs;      // a unit holds a voxel: fewer than 2^31
    P.wgs_z = (uint32_t)((P.units + ENV_WAVES - 1) / ENV_WAVES);
    P.wgs_flat = (uint32_t)(((unsigned long long)P.n_vox + ENV_THREADS - 1) / ENV_THREADS);
    P.voxsp = voxsp; P.extend = extend; P.soft = soft;
    P.vv = voxsp * voxsp;
    P.r2 = extend * extend;
    P.R = extend + soft;
    P.R2 = P.R * P.R;
    return ENV_OK;
}
