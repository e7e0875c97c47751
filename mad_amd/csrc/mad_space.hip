// mad_space.hip -- scale-space preparation and peak search on the device.
//
// Replaces the numerical body of MapSpace.build_space (mad/MapSpace.py:116-189): zero padding, the 2x
// upsampling by successive 1-D not-a-knot cubic splines (scipy interp1d(kind="cubic"), :206-214), the light
// pre-smoothing (:144), the scale-normalised LoG volumes (:169-173), the Gaussian-smoothed volumes and
// their gradients (:178-189) -- and the dense part of Detector.find_anchors (mad/Detector.py:28-29): the
// 3x3x3 local-maximum mask -- and its sub-voxel fit (check_localize, mad/Detector.py:53-123; k_localize, tiered).  The gradients are written straight into a field slot as the 16-byte texels the
// orientation / descriptor kernels sample, so a structure never leaves the device between its density grid
// and its descriptors.
//
// Arithmetic contract (what makes the volumes reproduce scipy's):
//  * every 1-D filter pass converts its input line to double, accumulates in double in the order of
//    scipy.ndimage's correlate1d for symmetric kernels -- centre tap first, then (left + right) * w from the
//    outermost tap inwards -- and rounds ONCE to the storage type of the volume (float32 or float64), pass
//    by pass in axis order 0, 1, 2, exactly like gaussian_filter does with its intermediate arrays;
//  * the boundary is scipy's "reflect" (d c b a | a b c d | d c b a);
//  * the kernel weights are inputs (computed by numpy on the host exactly as scipy computes them);
//  * the Laplacian is the storage-type sum of the three second-derivative filters in axis order
//    (generic_laplace), then * -1, * sigma^2, negatives clamped to 0;
//  * np.gradient: central differences / 2 inside, one-sided at the faces, in the storage type;
//  * the spline pass solves the banded collocation system per line (LU factors from the host, no pivoting)
//    and evaluates 4 basis weights per output sample, in double.  This is NOT bit-identical to LAPACK's
//    pivoted banded solve + de Boor, it agrees to ~4e-16 relative; after the float32 rounding of the
//    upsampled volume the difference survives in roughly one voxel per 1e7 as a single float32 ulp.
#include <algorithm>
#include <cstring>
#include <vector>

#include "mad_common.h"

namespace {

struct Dims {
    int n[3];
    __host__ __device__ size_t count() const { return (size_t)n[0] * n[1] * n[2]; }
};

// scipy.ndimage "reflect" (half-sample symmetric) extension of index i into [0, n)
__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

template <typename T>
__global__ __launch_bounds__(256) void k_pad(const T *__restrict__ src, Dims s, int pad, T *__restrict__ dst, Dims d) {
    const size_t total = d.count();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % d.n[2]), y = (int)((i / d.n[2]) % d.n[1]), x = (int)(i / ((size_t)d.n[2] * d.n[1]));
        const int sx = x - pad, sy = y - pad, sz = z - pad;
        T v = (T)0;
        if (sx >= 0 && sx < s.n[0] && sy >= 0 && sy < s.n[1] && sz >= 0 && sz < s.n[2]) v = src[((size_t)sx * s.n[1] + sy) * s.n[2] + sz];
        dst[i] = v;
    }
}

// start offset and element stride of line L along `axis` of a volume with dims d (z fastest)
__device__ __forceinline__ void line_of(size_t L, Dims d, int axis, size_t &off, size_t &stride) {
    if (axis == 0) { off = L; stride = (size_t)d.n[1] * d.n[2]; }
    else if (axis == 1) { off = (L / d.n[2]) * (size_t)d.n[1] * d.n[2] + (L % d.n[2]); stride = (size_t)d.n[2]; }
    else { off = L * (size_t)d.n[2]; stride = 1; }
}

// B-spline coefficients of every line along `axis`: forward / backward substitution with the banded LU
// factors lu = [l2 | l1 | d | u1 | u2] (5 x n) of the not-a-knot collocation matrix.  One thread per line.
template <typename T>
__global__ __launch_bounds__(256) void k_spline_solve(const T *__restrict__ in, Dims d, int axis, const double *__restrict__ lu,
                                                      double *__restrict__ c) {
    const int n = d.n[axis];
    const size_t n_lines = d.count() / n;
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= n_lines) return;
    size_t off, st;
    line_of(L, d, axis, off, st);
    const double *l2 = lu, *l1 = lu + n, *dg = lu + 2 * (size_t)n, *u1 = lu + 3 * (size_t)n, *u2 = lu + 4 * (size_t)n;
    double z1 = 0.0, z2 = 0.0;      // z[i-1], z[i-2]
    for (int i = 0; i < n; i++) {
        const double z = ((double)in[off + i * st] - l1[i] * z1) - l2[i] * z2;
        c[off + i * st] = z;
        z2 = z1; z1 = z;
    }
    double c1 = 0.0, c2 = 0.0;      // c[i+1], c[i+2]
    for (int i = n - 1; i >= 0; i--) {
        const double v = ((c[off + i * st] - u1[i] * c1) - u2[i] * c2) / dg[i];
        c[off + i * st] = v;
        c2 = c1; c1 = v;
    }
}

// value of the spline at the 2n-1 half-integer sites of every line: 4 basis weights per site
__global__ __launch_bounds__(256) void k_spline_eval(const double *__restrict__ c, Dims d, int axis, const double *__restrict__ ev_w,
                                                     const int32_t *__restrict__ ev_i, double *__restrict__ out, Dims o) {
    const size_t total = o.count();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int q[3];
        q[2] = (int)(i % o.n[2]); q[1] = (int)((i / o.n[2]) % o.n[1]); q[0] = (int)(i / ((size_t)o.n[2] * o.n[1]));
        const int m = q[axis];
        const int i0 = ev_i[m];
        q[axis] = i0;
        const size_t base = ((size_t)q[0] * d.n[1] + q[1]) * d.n[2] + q[2];
        const size_t st = axis == 0 ? (size_t)d.n[1] * d.n[2] : (axis == 1 ? (size_t)d.n[2] : 1);
        const double *w = ev_w + 4 * (size_t)m;
        out[i] = ((w[0] * c[base] + w[1] * c[base + st]) + w[2] * c[base + 2 * st]) + w[3] * c[base + 3 * st];
    }
}

// One pass of scipy.ndimage.correlate1d with a symmetric kernel of radius R along `axis`, "reflect" boundary;
// up to two kernels (w0, w1) applied to the same input.  One thread per voxel.
template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void k_filter_axis(const Tin *__restrict__ in, Dims d, int axis, int R, const double *__restrict__ w0,
                                                     const double *__restrict__ w1, Tout *__restrict__ out0, Tout *__restrict__ out1) {
    const size_t total = d.count();
    const size_t st = axis == 0 ? (size_t)d.n[1] * d.n[2] : (axis == 1 ? (size_t)d.n[2] : 1);
    const int n = d.n[axis];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pos = (int)((i / st) % n);
        const size_t base = i - (size_t)pos * st;
        const double centre = (double)in[i];
        double a0 = centre * w0[R], a1 = w1 ? centre * w1[R] : 0.0;
        if (pos >= R && pos + R < n) {
            for (int jj = -R; jj < 0; jj++) {
                const double pr = (double)in[i + (ptrdiff_t)jj * (ptrdiff_t)st] + (double)in[i - (ptrdiff_t)jj * (ptrdiff_t)st];
                a0 += pr * w0[R + jj];
                if (w1) a1 += pr * w1[R + jj];
            }
        } else {
            for (int jj = -R; jj < 0; jj++) {
                const double pr = (double)in[base + (size_t)reflect_idx(pos + jj, n) * st] + (double)in[base + (size_t)reflect_idx(pos - jj, n) * st];
                a0 += pr * w0[R + jj];
                if (w1) a1 += pr * w1[R + jj];
            }
        }
        out0[i] = (Tout)a0;
        if (w1) out1[i] = (Tout)a1;
    }
}

// Last (axis 2) pass of the three second-derivative filters and of the Gaussian, fused with the Laplacian sum:
//   term0 = G0_z(s01), term1 = G0_z(u01), term2 = G2_z(t01), gauss = G0_z(t01)      (each rounded to T)
//   log   = clamp0( (-1 * ((term0 + term1) + term2)) * sig2 )                          (T arithmetic, MapSpace.py:171-172)
template <typename T>
__global__ __launch_bounds__(256) void k_log_gauss(const T *__restrict__ s01, const T *__restrict__ u01, const T *__restrict__ t01, Dims d,
                                                   int R, const double *__restrict__ g0, const double *__restrict__ g2, double sig2,
                                                   T *__restrict__ gauss, T *__restrict__ logv) {
    const size_t total = d.count();
    const int n = d.n[2];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pos = (int)(i % n);
        const size_t base = i - pos;
        const double cs = (double)s01[i], cu = (double)u01[i], ct = (double)t01[i];
        double a0 = cs * g0[R], a1 = cu * g0[R], a2 = ct * g2[R], ag = ct * g0[R];
        for (int jj = -R; jj < 0; jj++) {
            const size_t il = base + reflect_idx(pos + jj, n), ir = base + reflect_idx(pos - jj, n);
            const double ps = (double)s01[il] + (double)s01[ir], pu = (double)u01[il] + (double)u01[ir], pt = (double)t01[il] + (double)t01[ir];
            a0 += ps * g0[R + jj];
            a1 += pu * g0[R + jj];
            a2 += pt * g2[R + jj];
            ag += pt * g0[R + jj];
        }
        gauss[i] = (T)ag;
        T l = (T)a0;
        l = l + (T)a1;
        l = l + (T)a2;
        l = (-l) * (T)sig2;
        logv[i] = (l < (T)0) ? (T)0 : l;
    }
}

// np.gradient of the smoothed volume (unit spacing, edge_order 1) -> texel {gx, gy, gz, |g|} in float32
template <typename T>
__global__ __launch_bounds__(256) void k_grad_tex(const T *__restrict__ g, Dims d, FieldDev F) {
    float4 *const tex = (float4 *)F.tex;
    unsigned *const tex4 = (unsigned *)F.tex4;
    const size_t total = d.count();
    const size_t sx = (size_t)d.n[1] * d.n[2], sy = (size_t)d.n[2];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % d.n[2]), y = (int)((i / d.n[2]) % d.n[1]), x = (int)(i / sx);
        T gx, gy, gz;
        if (x == 0) gx = g[i + sx] - g[i]; else if (x == d.n[0] - 1) gx = g[i] - g[i - sx]; else gx = (g[i + sx] - g[i - sx]) / (T)2;
        if (y == 0) gy = g[i + sy] - g[i]; else if (y == d.n[1] - 1) gy = g[i] - g[i - sy]; else gy = (g[i + sy] - g[i - sy]) / (T)2;
        if (z == 0) gz = g[i + 1] - g[i]; else if (z == d.n[2] - 1) gz = g[i] - g[i - 1]; else gz = (g[i + 1] - g[i - 1]) / (T)2;
        const float fx = (float)gx, fy = (float)gy, fz = (float)gz;
        const float s = __fadd_rn(__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy)), __fmul_rn(fz, fz));
        const float w = sqrtf(s);      // correctly rounded (see k_pack_field)
        tex[i] = make_float4(fx, fy, fz, w);
        tex4[mad_tex4_index(F, (unsigned)x, (unsigned)y, (unsigned)z)] = mad_tex4_encode(fx, fy, fz, w);      // in its brick
    }
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void k_convert(const Tin *__restrict__ in, Tout *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = (Tout)in[i];
}

// 3x3x3 local maxima (value == maximum of the zero-extended neighbourhood), strictly above the threshold,
// at least `border` voxels from every face (skimage.feature.peak_local_max, min_distance 1).  The threshold is
// compared in the storage type, as numpy compares an array with a Python float: a float32 volume against
// float32(thr), rounded to nearest, so a voxel holding exactly that float32 is no peak even where the double
// lies just below it; a float64 volume against thr itself.
template <typename T>
__global__ __launch_bounds__(256) void k_peaks(const T *__restrict__ v, Dims d, double thr, int border, int64_t *__restrict__ out_idx,
                                               double *__restrict__ out_val, int32_t *__restrict__ count, int cap) {
    const size_t total = d.count();
    const size_t sx = (size_t)d.n[1] * d.n[2], sy = (size_t)d.n[2];
    const T thr_t = (T)thr;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % d.n[2]), y = (int)((i / d.n[2]) % d.n[1]), x = (int)(i / sx);
        if (x < border || y < border || z < border || x >= d.n[0] - border || y >= d.n[1] - border || z >= d.n[2] - border) continue;
        const T c = v[i];
        if (!(c > thr_t)) continue;
        bool is_max = !(c < (T)0);      // the zero extension takes part in the maximum
        for (int dx = -1; dx <= 1 && is_max; dx++) {
            for (int dy = -1; dy <= 1 && is_max; dy++) {
                for (int dz = -1; dz <= 1; dz++) {
                    const int xx = x + dx, yy = y + dy, zz = z + dz;
                    T o = (T)0;
                    if (xx >= 0 && xx < d.n[0] && yy >= 0 && yy < d.n[1] && zz >= 0 && zz < d.n[2]) o = v[(size_t)xx * sx + (size_t)yy * sy + zz];
                    if (o > c) { is_max = false; break; }
                }
            }
        }
        if (!is_max) continue;
        const int slot = atomicAdd(count, 1);
        if (slot < cap) { out_idx[slot] = (int64_t)i; out_val[slot] = (double)c; }
    }
}

// (2r+1)^3 neighbourhoods of n voxels (zero outside the volume), for the host's sub-voxel fit
template <typename T>
__global__ __launch_bounds__(256) void k_patches(const T *__restrict__ v, Dims d, const int32_t *__restrict__ coords, int n, int r,
                                                 T *__restrict__ out) {
    const int side = 2 * r + 1;
    const size_t per = (size_t)side * side * side, total = per * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(i / per);
        const int q = (int)(i % per);
        const int x = coords[3 * p] + q / (side * side) - r, y = coords[3 * p + 1] + (q / side) % side - r, z = coords[3 * p + 2] + q % side - r;
        T o = (T)0;
        if (x >= 0 && x < d.n[0] && y >= 0 && y < d.n[1] && z >= 0 && z < d.n[2]) o = v[((size_t)x * d.n[1] + y) * d.n[2] + z];
        out[i] = o;
    }
}

// ---------------------------------------------------------------------------
// k_localize: Detector.check_localize (mad/Detector.py:53-123) on the device, tiered
// ---------------------------------------------------------------------------
// H and G are built from the same voxel reads, in the same operation order and in the storage type T, as the
// reference's numpy scalars.  Every decision numpy takes on them -- stop / move per axis of each iteration
// (float32 or float64 offset against float32(0.6) or 0.6) and "no positive eigenvalue" at the end -- is taken
// from an exact-input float64 solve (adjugate) only when it lies outside a band that covers the rounding of the
// float64 solve here and of numpy's expression -(float32(inv64(H)) . G); otherwise the candidate is undecided
// (status 2) and the host runs check_localize on it.  The band constants are mirrored by
// tools/check_localize_tier.py (a CPU test checks both against numpy).
#define MAD_LOC_U64 1.1102230246251565e-16      // 2^-53
#define MAD_LOC_U32 5.9604644775390625e-08      // 2^-24
#define MAD_LOC_KAPPA_MAX 16777216.0            // 2^24: ||H||inf ||H^-1||inf beyond this counts as near-singular
#define MAD_LOC_INV_C 64.0                      // LAPACK inverse: |X - H^-1|_ij <= C u64 kappa ||H^-1||inf
#define MAD_LOC_DOT_C32 5.0                     // float32 path: X rounded to float32 (1 u32) + 3-term float32 dot (gamma_3)
#define MAD_LOC_DOT_C64 4.0                     // float64 path: 3-term float64 dot
#define MAD_LOC_SAFETY 4.0                      // the band is SAFETY x (bound of this solve + bound of numpy's)
#define MAD_LOC_EIG_SHIFT 1.4551915228366852e-11      // 2^-36: eigenvalue margin delta = shift x 3 max|h_ij| (>> geev's error)
#define MAD_LOC_HMIN 1e-20                      // max|h_ij| below this: no eigenvalue decision
#define MAD_LOC_ITERS 5
#define MAD_LOC_BLOCK 64

// float64 adjugate solve of the stop / move decision.  cls[i] = -1 (o_i < -t), 0 (|o_i| < t), 1 (o_i > t) as numpy will
// find them; false = some component inside the band, or H near-singular.
__device__ __forceinline__ bool loc_decide_offset(const double h[6], const double g[3], double t, bool f32, int cls[3]) {
#pragma clang fp contract(off)
    const double u = MAD_LOC_U64;
    const double h00 = h[0], h01 = h[1], h02 = h[2], h11 = h[3], h12 = h[4], h22 = h[5];
    double A[3][3], E[3][3];
    A[0][0] = h11 * h22 - h12 * h12; E[0][0] = 2 * u * (fabs(h11 * h22) + h12 * h12);
    A[0][1] = h02 * h12 - h01 * h22; E[0][1] = 2 * u * (fabs(h02 * h12) + fabs(h01 * h22));
    A[0][2] = h01 * h12 - h02 * h11; E[0][2] = 2 * u * (fabs(h01 * h12) + fabs(h02 * h11));
    A[1][1] = h00 * h22 - h02 * h02; E[1][1] = 2 * u * (fabs(h00 * h22) + h02 * h02);
    A[1][2] = h01 * h02 - h00 * h12; E[1][2] = 2 * u * (fabs(h01 * h02) + fabs(h00 * h12));
    A[2][2] = h00 * h11 - h01 * h01; E[2][2] = 2 * u * (fabs(h00 * h11) + h01 * h01);
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    E[1][0] = E[0][1]; E[2][0] = E[0][2]; E[2][1] = E[1][2];
    const double det = (h00 * A[0][0] + h01 * A[0][1]) + h02 * A[0][2];
    const double det_err = (fabs(h00) * E[0][0] + fabs(h01) * E[0][1] + fabs(h02) * E[0][2]) +
                           3 * u * (fabs(h00 * A[0][0]) + fabs(h01 * A[0][1]) + fabs(h02 * A[0][2]));
    const double ad = fabs(det);
    if (!(ad > 4 * det_err) || !isfinite(ad)) return false;
    const double norm_h = fmax(fabs(h00) + fabs(h01) + fabs(h02), fmax(fabs(h01) + fabs(h11) + fabs(h12), fabs(h02) + fabs(h12) + fabs(h22)));
    double norm_inv = 0.0;
    for (int i = 0; i < 3; i++) norm_inv = fmax(norm_inv, (fabs(A[i][0]) + fabs(A[i][1]) + fabs(A[i][2])) / ad);
    const double kappa = norm_h * norm_inv;
    if (!(kappa <= MAD_LOC_KAPPA_MAX)) return false;
    const double g1 = fabs(g[0]) + fabs(g[1]) + fabs(g[2]);
    const double inv_term = MAD_LOC_INV_C * u * kappa * norm_inv * g1;
    const double dot_c = f32 ? MAD_LOC_DOT_C32 * MAD_LOC_U32 : MAD_LOC_DOT_C64 * u;
    for (int i = 0; i < 3; i++) {
        const double N = (A[i][0] * g[0] + A[i][1] * g[1]) + A[i][2] * g[2];
        const double sabs = fabs(A[i][0] * g[0]) + fabs(A[i][1] * g[1]) + fabs(A[i][2] * g[2]);
        const double n_err = (E[i][0] * fabs(g[0]) + E[i][1] * fabs(g[1]) + E[i][2] * fabs(g[2])) + 3 * u * sabs;
        const double o = -N / det;
        const double dev_err = (n_err + fabs(o) * det_err) / (ad - det_err) + 2 * u * fabs(o);
        const double band = MAD_LOC_SAFETY * (dev_err + inv_term + dot_c * (sabs / ad));
        if (!isfinite(o) || !isfinite(band)) return false;
        if (o - band > t) cls[i] = 1;
        else if (o + band < -t) cls[i] = -1;
        else if (o + band < t && o - band > -t) cls[i] = 0;
        else return false;
    }
    return true;
}

// "no eigenvalue of H is > 0" (np.linalg.eigvals, Detector.py:104-108), by Sylvester's criterion with a margin delta:
// 1 = every eigenvalue < -delta (leading minors of -H - delta I positive beyond their rounding), 0 = some eigenvalue > delta
// (a principal minor of delta I - H negative beyond its rounding), 2 = neither.
__device__ __forceinline__ int loc_decide_eigen(const double h[6]) {
#pragma clang fp contract(off)
    const double u = MAD_LOC_U64;
    double hmax = 0.0;
    for (int k = 0; k < 6; k++) hmax = fmax(hmax, fabs(h[k]));
    if (!(hmax >= MAD_LOC_HMIN) || !isfinite(hmax)) return 2;
    const double delta = MAD_LOC_EIG_SHIFT * 3.0 * hmax;
    for (int pass = 0; pass < 2; pass++) {
        // pass 0: B = -H - delta I (accept if B is positive definite); pass 1: B = delta I - H (reject if B is not PSD)
        const double s = pass == 0 ? -delta : delta;
        const double b00 = s - h[0], b11 = s - h[3], b22 = s - h[5], b01 = -h[1], b02 = -h[2], b12 = -h[4];
        const double m01 = b00 * b11 - b01 * b01, e01 = 4 * u * (fabs(b00 * b11) + b01 * b01);
        const double m02 = b00 * b22 - b02 * b02, e02 = 4 * u * (fabs(b00 * b22) + b02 * b02);
        const double m12 = b11 * b22 - b12 * b12, e12 = 4 * u * (fabs(b11 * b22) + b12 * b12);
        const double c0 = b11 * b22 - b12 * b12, c1 = b01 * b22 - b12 * b02, c2 = b01 * b12 - b11 * b02;
        const double m3 = (b00 * c0 - b01 * c1) + b02 * c2;
        const double p3 = fabs(b00) * (fabs(b11 * b22) + b12 * b12) + fabs(b01) * (fabs(b01 * b22) + fabs(b12 * b02)) +
                          fabs(b02) * (fabs(b01 * b12) + fabs(b11 * b02));
        const double e3 = 16 * u * p3;
        if (pass == 0) {
            if (b00 > 0 && m01 > e01 && m3 > e3) return 1;
        } else {
            if (b00 < 0 || b11 < 0 || b22 < 0 || m01 < -e01 || m02 < -e02 || m12 < -e12 || m3 < -e3) return 0;
        }
    }
    return 2;
}

// One lane per candidate: the walk of up to five steps of check_localize, in place on the LoG volume.  A latency kernel
// (<= 5 x 19 gathers per lane, a few thousand lanes): one wavefront per block so that the lanes spread over the CUs.
// Output per candidate: status (0 rejected, 1 accepted, 2 undecided), the voxel it ended on, H (9) and G (3) of the last
// iteration in T.  cand holds starting voxels inside [1, n-2] on every axis (the host checks), and the moves keep them there.
template <typename T>
__global__ __launch_bounds__(MAD_LOC_BLOCK) void k_localize(const T *__restrict__ v, Dims d, const int32_t *__restrict__ cand, int n, double t,
                                                            int32_t *__restrict__ status, int32_t *__restrict__ coord, T *__restrict__ Hout,
                                                            T *__restrict__ Gout) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * MAD_LOC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t sx = (size_t)d.n[1] * d.n[2], sy = (size_t)d.n[2];
    int x = cand[3 * i], y = cand[3 * i + 1], z = cand[3 * i + 2];
    int st = 0;
    T xx = 0, yy = 0, zz = 0, xy = 0, xz = 0, yz = 0, gx = 0, gy = 0, gz = 0;
    for (int it = 0; it < MAD_LOC_ITERS; it++) {
        const T *p = v + (size_t)x * sx + (size_t)y * sy + z;
        const T c = p[0];
        const T xm = p[-(ptrdiff_t)sx], xp = p[sx], ym = p[-(ptrdiff_t)sy], yp = p[sy], zm = p[-1], zp = p[1];
        // Detector.py:66-80, term by term as numpy evaluates them in T
        xx = (xm + xp) - (T)2 * c;
        yy = (ym + yp) - (T)2 * c;
        zz = (zm + zp) - (T)2 * c;
        xy = (T)0.25 * ((p[sx + sy] - p[sx - sy]) - (p[-(ptrdiff_t)sx + (ptrdiff_t)sy] - p[-(ptrdiff_t)sx - (ptrdiff_t)sy]));
        xz = (T)0.25 * ((p[sx + 1] - p[sx - 1]) - (p[-(ptrdiff_t)sx + 1] - p[-(ptrdiff_t)sx - 1]));
        yz = (T)0.25 * ((p[sy + 1] - p[sy - 1]) - (p[-(ptrdiff_t)sy + 1] - p[-(ptrdiff_t)sy - 1]));
        gx = (T)0.5 * (xp - xm);
        gy = (T)0.5 * (yp - ym);
        gz = (T)0.5 * (zp - zm);
        const double h[6] = {(double)xx, (double)xy, (double)xz, (double)yy, (double)yz, (double)zz};
        const double g[3] = {(double)gx, (double)gy, (double)gz};
        int cls[3];
        if (!loc_decide_offset(h, g, t, sizeof(T) == 4, cls)) { st = 2; break; }
        if (cls[0] == 0 && cls[1] == 0 && cls[2] == 0) {
            st = loc_decide_eigen(h);
            break;
        }
        if (cls[0] < 0 && x - 1 > 0) x -= 1;
        else if (cls[0] > 0 && x + 1 < d.n[0] - 1) x += 1;
        if (cls[1] < 0 && y - 1 > 0) y -= 1;
        else if (cls[1] > 0 && y + 1 < d.n[1] - 1) y += 1;
        if (cls[2] < 0 && z - 1 > 0) z -= 1;
        else if (cls[2] > 0 && z + 1 < d.n[2] - 1) z += 1;
    }
    status[i] = st;
    coord[3 * i] = x; coord[3 * i + 1] = y; coord[3 * i + 2] = z;
    T *H = Hout + 9 * (size_t)i;
    H[0] = xx; H[1] = xy; H[2] = xz; H[3] = xy; H[4] = yy; H[5] = yz; H[6] = xz; H[7] = yz; H[8] = zz;
    Gout[3 * i] = gx; Gout[3 * i + 1] = gy; Gout[3 * i + 2] = gz;
}

struct Octave {
    Dims d;
    bool f64 = false;
    int kind = 1;          // 0 = upsampled, 1 = base (DensityFeature.oct_scale)
    void *grid = nullptr, *gauss = nullptr, *logv = nullptr;
};

// temporaries of one build, freed together
struct Arena {
    std::vector<void *> ptrs;
    void *get(size_t bytes) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
    ~Arena() { for (void *p : ptrs) (void)hipFree(p); }
};

unsigned blocks_for(const mad_ctx *ctx, size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)ctx->n_cu * 32); }

}  // namespace

struct mad_space {
    int n_oct = 0;
    Octave oct[2];
};

static void space_release(mad_space *s) {
    for (int o = 0; o < 2; o++) {
        for (void **p : {&s->oct[o].grid, &s->oct[o].gauss, &s->oct[o].logv}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
    }
    s->n_oct = 0;
}

extern "C" int mad_space_create(mad_ctx *ctx, mad_space **out) {
    if (!ctx || !out) return MAD_EINVAL;
    *out = new mad_space();
    return MAD_OK;
}

extern "C" void mad_space_destroy(mad_ctx *ctx, mad_space *s) {
    if (!s) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    space_release(s);
    delete s;
}

template <typename T>
static int build_octave(mad_ctx *ctx, Octave &O, int R, const double *d_g0, const double *d_g2, double sig2, int slot) {
    Arena A;
    const size_t n = O.d.count(), bytes = n * sizeof(T);
    const unsigned nb = blocks_for(ctx, n);
    T *grid = (T *)O.grid;
    T *t0 = (T *)A.get(bytes), *s0 = (T *)A.get(bytes), *t01 = (T *)A.get(bytes), *s01 = (T *)A.get(bytes), *u01 = (T *)A.get(bytes);
    if (!t0 || !s0 || !t01 || !s01 || !u01) return mad_fail(ctx, MAD_ENOMEM, "mad_space_build: %zu bytes of filter temporaries", 5 * bytes);
    if (hipMalloc(&O.gauss, bytes) != hipSuccess || hipMalloc(&O.logv, bytes) != hipSuccess)
        return mad_fail(ctx, MAD_ENOMEM, "mad_space_build: %zu bytes of volumes", 2 * bytes);
    // axis 0: order 0 and order 2 of the same input
    hipLaunchKernelGGL((k_filter_axis<T, T>), dim3(nb), dim3(256), 0, ctx->stream, grid, O.d, 0, R, d_g0, d_g2, t0, s0);
    // axis 1: G0(t0) -> t01 and G2(t0) -> u01 in one pass, G0(s0) -> s01
    hipLaunchKernelGGL((k_filter_axis<T, T>), dim3(nb), dim3(256), 0, ctx->stream, t0, O.d, 1, R, d_g0, d_g2, t01, u01);
    hipLaunchKernelGGL((k_filter_axis<T, T>), dim3(nb), dim3(256), 0, ctx->stream, s0, O.d, 1, R, d_g0, (const double *)nullptr, s01, (T *)nullptr);
    // axis 2 + Laplacian
    hipLaunchKernelGGL((k_log_gauss<T>), dim3(nb), dim3(256), 0, ctx->stream, s01, u01, t01, O.d, R, d_g0, d_g2, sig2, (T *)O.gauss, (T *)O.logv);
    MAD_HIP(hipGetLastError());
    if (slot >= 0) {
        size_t cnt = 0;
        MAD_TRY(mad_field_alloc(ctx, slot, O.d.n[0], O.d.n[1], O.d.n[2], &cnt));
        hipLaunchKernelGGL((k_grad_tex<T>), dim3(nb), dim3(256), 0, ctx->stream, (const T *)O.gauss, O.d, ctx->fields[slot]);
        MAD_HIP(hipGetLastError());
    }
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // the arena goes away
    return MAD_OK;
}

template <typename T>
static int build_all(mad_ctx *ctx, mad_space *s, const T *h_grid, int nx, int ny, int nz, int pad, int oct_mode, const double *g0,
                     const double *g2, int R, double sig2, const double *pre, int pre_R, const double *const *lu,
                     const double *const *ev_w, const int32_t *const *ev_i, int slot_up, int slot_base) {
    Arena A;
    const Dims src{{nx, ny, nz}};
    const Dims b{{nx + 2 * pad, ny + 2 * pad, nz + 2 * pad}};
    // weights and tables
    double *d_g0 = (double *)A.get((2 * R + 1) * 8), *d_g2 = (double *)A.get((2 * R + 1) * 8), *d_pre = (double *)A.get((2 * pre_R + 1) * 8);
    T *d_src = (T *)A.get(src.count() * sizeof(T));
    if (!d_g0 || !d_g2 || !d_pre || !d_src) return mad_fail(ctx, MAD_ENOMEM, "mad_space_build: staging");
    MAD_HIP(hipMemcpyAsync(d_g0, g0, (2 * R + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_g2, g2, (2 * R + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (pre_R > 0) MAD_HIP(hipMemcpyAsync(d_pre, pre, (2 * pre_R + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_src, h_grid, src.count() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    T *base = nullptr;
    if (hipMalloc((void **)&base, b.count() * sizeof(T)) != hipSuccess) return mad_fail(ctx, MAD_ENOMEM, "mad_space_build: base volume");
    hipLaunchKernelGGL((k_pad<T>), dim3(blocks_for(ctx, b.count())), dim3(256), 0, ctx->stream, (const T *)d_src, src, pad, base, b);
    MAD_HIP(hipGetLastError());

    int n_oct = 0;
    if (oct_mode & 2) {
        // successive 1-D splines along axes 0, 1, 2 (MapSpace.interpn_so, :191-214), all in double
        Dims cur = b;
        const void *in = base;
        bool in_is_T = true;
        double *vol = nullptr;
        for (int a = 0; a < 3; a++) {
            const int n = cur.n[a];
            Dims o = cur;
            o.n[a] = 2 * n - 1;
            double *d_lu = (double *)A.get((size_t)5 * n * 8), *d_w = (double *)A.get((size_t)(2 * n - 1) * 32);
            int32_t *d_i = (int32_t *)A.get((size_t)(2 * n - 1) * 4);
            double *c = (double *)A.get(cur.count() * 8);
            double *outv = (double *)A.get(o.count() * 8);
            if (!d_lu || !d_w || !d_i || !c || !outv) return mad_fail(ctx, MAD_ENOMEM, "mad_space_build: spline volumes of %zu voxels", o.count());
            MAD_HIP(hipMemcpyAsync(d_lu, lu[a], (size_t)5 * n * 8, hipMemcpyHostToDevice, ctx->stream));
            MAD_HIP(hipMemcpyAsync(d_w, ev_w[a], (size_t)(2 * n - 1) * 32, hipMemcpyHostToDevice, ctx->stream));
            MAD_HIP(hipMemcpyAsync(d_i, ev_i[a], (size_t)(2 * n - 1) * 4, hipMemcpyHostToDevice, ctx->stream));
            const size_t n_lines = cur.count() / n;
            const unsigned lb = (unsigned)((n_lines + 255) / 256);
            if (in_is_T) hipLaunchKernelGGL((k_spline_solve<T>), dim3(lb), dim3(256), 0, ctx->stream, (const T *)in, cur, a, d_lu, c);
            else hipLaunchKernelGGL((k_spline_solve<double>), dim3(lb), dim3(256), 0, ctx->stream, (const double *)in, cur, a, d_lu, c);
            hipLaunchKernelGGL(k_spline_eval, dim3(blocks_for(ctx, o.count())), dim3(256), 0, ctx->stream, (const double *)c, cur, a, d_w, d_i, outv, o);
            MAD_HIP(hipGetLastError());
            in = outv; in_is_T = false; cur = o; vol = outv;
        }
        Octave &U = s->oct[n_oct];
        U.d = cur; U.f64 = false; U.kind = 0;
        if (hipMalloc(&U.grid, cur.count() * 4) != hipSuccess) return mad_fail(ctx, MAD_ENOMEM, "mad_space_build: upsampled volume");
        const unsigned nb = blocks_for(ctx, cur.count());
        if (pre_R > 0) {      // gaussian_filter(up, sigma=presmooth) in double, then .astype(float32) (MapSpace.py:144)
            double *p1 = (double *)A.get(cur.count() * 8);
            if (!p1) return mad_fail(ctx, MAD_ENOMEM, "mad_space_build: pre-smoothing volume");
            hipLaunchKernelGGL((k_filter_axis<double, double>), dim3(nb), dim3(256), 0, ctx->stream, (const double *)vol, cur, 0, pre_R, d_pre, (const double *)nullptr, p1, (double *)nullptr);
            hipLaunchKernelGGL((k_filter_axis<double, double>), dim3(nb), dim3(256), 0, ctx->stream, (const double *)p1, cur, 1, pre_R, d_pre, (const double *)nullptr, vol, (double *)nullptr);
            hipLaunchKernelGGL((k_filter_axis<double, float>), dim3(nb), dim3(256), 0, ctx->stream, (const double *)vol, cur, 2, pre_R, d_pre, (const double *)nullptr, (float *)U.grid, (float *)nullptr);
        } else {
            hipLaunchKernelGGL((k_convert<double, float>), dim3(nb), dim3(256), 0, ctx->stream, (const double *)vol, (float *)U.grid, cur.count());
        }
        MAD_HIP(hipGetLastError());
        n_oct++;
    }
    if (oct_mode & 1) {
        Octave &B = s->oct[n_oct];
        B.d = b; B.f64 = sizeof(T) == 8; B.kind = 1; B.grid = base;
        n_oct++;
    }
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (!(oct_mode & 1)) (void)hipFree(base);
    s->n_oct = n_oct;
    for (int o = 0; o < n_oct; o++) {
        Octave &O = s->oct[o];
        const int slot = O.kind == 0 ? slot_up : slot_base;
        if (O.f64) MAD_TRY(build_octave<double>(ctx, O, R, d_g0, d_g2, sig2, slot));
        else MAD_TRY(build_octave<float>(ctx, O, R, d_g0, d_g2, sig2, slot));
    }
    return MAD_OK;
}

extern "C" int mad_space_build(mad_ctx *ctx, mad_space *s, const void *grid, int is_f64, int nx, int ny, int nz, int pad,
                               int oct_mode, const double *g0, const double *g2, int radius, double sig2,
                               const double *pre, int pre_radius, const double *const *lu, const double *const *ev_w,
                               const int32_t *const *ev_i, int slot_up, int slot_base) {
    if (!ctx || !s || !grid || !g0 || !g2) return MAD_EINVAL;
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    space_release(s);      // a build that fails, for whatever reason, leaves the space empty
    if (nx < 2 || ny < 2 || nz < 2 || pad < 0 || radius < 1 || radius > 64 || pre_radius < 0 || pre_radius > 64)
        return mad_fail(ctx, MAD_EINVAL, "mad_space_build: dims %dx%dx%d pad %d radius %d/%d", nx, ny, nz, pad, radius, pre_radius);
    if (oct_mode < 1 || oct_mode > 3) return mad_fail(ctx, MAD_EINVAL, "mad_space_build: oct_mode %d", oct_mode);
    if ((oct_mode & 2) && std::min(nx, std::min(ny, nz)) + 2 * pad < 4) return mad_fail(ctx, MAD_EINVAL, "mad_space_build: a cubic spline needs 4 samples per axis");
    if ((oct_mode & 2) && (!lu || !ev_w || !ev_i || (pre_radius > 0 && !pre))) return mad_fail(ctx, MAD_EINVAL, "mad_space_build: spline tables missing");
    const size_t up = (size_t)(2 * (nx + 2 * pad) - 1) * (2 * (ny + 2 * pad) - 1) * (2 * (nz + 2 * pad) - 1);
    if ((oct_mode & 2) && up >= ((size_t)1 << 32)) return mad_fail(ctx, MAD_EINVAL, "mad_space_build: upsampled volume of %zu voxels exceeds 2^32", up);
    int rc;
    if (is_f64) rc = build_all<double>(ctx, s, (const double *)grid, nx, ny, nz, pad, oct_mode, g0, g2, radius, sig2, pre, pre_radius, lu, ev_w, ev_i, slot_up, slot_base);
    else rc = build_all<float>(ctx, s, (const float *)grid, nx, ny, nz, pad, oct_mode, g0, g2, radius, sig2, pre, pre_radius, lu, ev_w, ev_i, slot_up, slot_base);
    (void)hipStreamSynchronize(ctx->stream);
    if (rc != MAD_OK) space_release(s);
    return rc;
}

extern "C" int mad_space_info(mad_ctx *ctx, const mad_space *s, int *n_octaves, int32_t *dims6, int32_t *kind2, int32_t *is_f64_2) {
    if (!ctx || !s) return MAD_EINVAL;
    if (n_octaves) *n_octaves = s->n_oct;
    for (int o = 0; o < s->n_oct; o++) {
        if (dims6) { dims6[3 * o] = s->oct[o].d.n[0]; dims6[3 * o + 1] = s->oct[o].d.n[1]; dims6[3 * o + 2] = s->oct[o].d.n[2]; }
        if (kind2) kind2[o] = s->oct[o].kind;
        if (is_f64_2) is_f64_2[o] = s->oct[o].f64 ? 1 : 0;
    }
    return MAD_OK;
}

extern "C" int mad_space_download(mad_ctx *ctx, const mad_space *s, int entry, int what, void *out) {
    if (!ctx || !s || !out) return MAD_EINVAL;
    if (entry < 0 || entry >= s->n_oct) return mad_fail(ctx, MAD_EINVAL, "mad_space_download: entry %d of %d", entry, s->n_oct);
    const Octave &O = s->oct[entry];
    const void *src = what == 0 ? O.grid : (what == 1 ? O.logv : (what == 2 ? O.gauss : nullptr));
    if (!src) return mad_fail(ctx, MAD_EINVAL, "mad_space_download: volume %d", what);
    MAD_HIP(hipMemcpyAsync(out, src, O.d.count() * (O.f64 ? 8 : 4), hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

extern "C" int mad_space_peaks(mad_ctx *ctx, const mad_space *s, int entry, double threshold, int border, int64_t *lin_index,
                               double *value, int64_t cap, int64_t *n_out) {
    if (!ctx || !s || !n_out) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    if (entry < 0 || entry >= s->n_oct) return mad_fail(ctx, MAD_EINVAL, "mad_space_peaks: entry %d of %d", entry, s->n_oct);
    if (border < 0 || cap < 0 || cap >= ((int64_t)1 << 31)) return mad_fail(ctx, MAD_EINVAL, "mad_space_peaks: border %d cap %lld", border, (long long)cap);
    const Octave &O = s->oct[entry];
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (size_t)(cap + 1) * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), (size_t)(cap + 1) * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_MISC), 256));
    int32_t *d_cnt = scratch<int32_t>(ctx, S_MISC);
    MAD_HIP(hipMemsetAsync(d_cnt, 0, 4, ctx->stream));
    const unsigned nb = blocks_for(ctx, O.d.count());
    if (O.f64) hipLaunchKernelGGL((k_peaks<double>), dim3(nb), dim3(256), 0, ctx->stream, (const double *)O.logv, O.d, threshold, border, scratch<int64_t>(ctx, S_TMP_A), scratch<double>(ctx, S_TMP_B), d_cnt, (int)cap);
    else hipLaunchKernelGGL((k_peaks<float>), dim3(nb), dim3(256), 0, ctx->stream, (const float *)O.logv, O.d, threshold, border, scratch<int64_t>(ctx, S_TMP_A), scratch<double>(ctx, S_TMP_B), d_cnt, (int)cap);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(&ctx->pinned[0], d_cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t n = *(const int32_t *)&ctx->pinned[0];
    *n_out = n;
    if (n > cap) return mad_fail(ctx, MAD_ENOSPC, "mad_space_peaks: %lld peaks, capacity %lld", (long long)n, (long long)cap);
    if (n > 0 && lin_index) MAD_HIP(hipMemcpyAsync(lin_index, mad_sb(ctx, S_TMP_A).p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n > 0 && value) MAD_HIP(hipMemcpyAsync(value, mad_sb(ctx, S_TMP_B).p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

extern "C" int mad_space_patches(mad_ctx *ctx, const mad_space *s, int entry, const int32_t *coords, int n, int r, void *out) {
    if (!ctx || !s || (n > 0 && (!coords || !out))) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    if (entry < 0 || entry >= s->n_oct) return mad_fail(ctx, MAD_EINVAL, "mad_space_patches: entry %d of %d", entry, s->n_oct);
    if (n <= 0) return MAD_OK;
    if (r < 1 || r > 16) return mad_fail(ctx, MAD_EINVAL, "mad_space_patches: radius %d", r);
    const Octave &O = s->oct[entry];
    const int side = 2 * r + 1;
    const size_t total = (size_t)side * side * side * n, esz = O.f64 ? 8 : 4;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (size_t)n * 12));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), total * esz));
    MAD_HIP(hipMemcpyAsync(mad_sb(ctx, S_TMP_A).p, coords, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    const unsigned nb = blocks_for(ctx, total);
    if (O.f64) hipLaunchKernelGGL((k_patches<double>), dim3(nb), dim3(256), 0, ctx->stream, (const double *)O.logv, O.d, scratch<int32_t>(ctx, S_TMP_A), n, r, scratch<double>(ctx, S_TMP_B));
    else hipLaunchKernelGGL((k_patches<float>), dim3(nb), dim3(256), 0, ctx->stream, (const float *)O.logv, O.d, scratch<int32_t>(ctx, S_TMP_A), n, r, scratch<float>(ctx, S_TMP_B));
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out, mad_sb(ctx, S_TMP_B).p, total * esz, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// Runs k_localize on a device volume and brings status, voxel, H and G back in one copy.
static int localize_run(mad_ctx *ctx, const void *vol, bool f64, Dims d, const int32_t *cand, int n, int32_t *status,
                        int32_t *coord, void *H, void *G, int64_t *n_undecided) {
    const size_t esz = f64 ? 8 : 4;
    const size_t b_status = (size_t)n * 4, b_coord = (size_t)n * 12, b_H = (size_t)n * 9 * esz, b_G = (size_t)n * 3 * esz;
    const size_t total = b_status + b_coord + b_H + b_G;      // status + coord = 16 n bytes: H stays 8-byte aligned
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), b_coord));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), total));
    MAD_HIP(hipMemcpyAsync(mad_sb(ctx, S_TMP_A).p, cand, b_coord, hipMemcpyHostToDevice, ctx->stream));
    char *out = scratch<char>(ctx, S_TMP_B);
    int32_t *d_status = (int32_t *)out, *d_coord = (int32_t *)(out + b_status);
    void *d_H = out + b_status + b_coord, *d_G = out + b_status + b_coord + b_H;
    const unsigned nb = (unsigned)((n + MAD_LOC_BLOCK - 1) / MAD_LOC_BLOCK);
    if (f64) hipLaunchKernelGGL((k_localize<double>), dim3(nb), dim3(MAD_LOC_BLOCK), 0, ctx->stream, (const double *)vol, d,
                                scratch<int32_t>(ctx, S_TMP_A), n, 0.6, d_status, d_coord, (double *)d_H, (double *)d_G);
    else hipLaunchKernelGGL((k_localize<float>), dim3(nb), dim3(MAD_LOC_BLOCK), 0, ctx->stream, (const float *)vol, d,
                            scratch<int32_t>(ctx, S_TMP_A), n, (double)0.6f, d_status, d_coord, (float *)d_H, (float *)d_G);
    MAD_HIP(hipGetLastError());
    std::vector<char> host(total);
    MAD_HIP(hipMemcpyAsync(host.data(), out, total, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(status, host.data(), b_status);
    std::memcpy(coord, host.data() + b_status, b_coord);
    std::memcpy(H, host.data() + b_status + b_coord, b_H);
    std::memcpy(G, host.data() + b_status + b_coord + b_H, b_G);
    int64_t und = 0;
    for (int i = 0; i < n; i++) und += status[i] == 2;
    if (n_undecided) *n_undecided = und;
    return MAD_OK;
}

// every starting voxel inside [1, n-2] on every axis: the walk then never reads outside the volume
static int localize_check(mad_ctx *ctx, const char *who, Dims d, const int32_t *cand, int n) {
    if (d.n[0] < 3 || d.n[1] < 3 || d.n[2] < 3) return mad_fail(ctx, MAD_EINVAL, "%s: volume %dx%dx%d", who, d.n[0], d.n[1], d.n[2]);
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (cand[3 * i + a] < 1 || cand[3 * i + a] > d.n[a] - 2)
                return mad_fail(ctx, MAD_EDOM, "%s: candidate %d at (%d, %d, %d) is not inside [1, n-2] of %dx%dx%d", who, i, cand[3 * i],
                                cand[3 * i + 1], cand[3 * i + 2], d.n[0], d.n[1], d.n[2]);
    return MAD_OK;
}

extern "C" int mad_space_localize(mad_ctx *ctx, const mad_space *s, int entry, const int32_t *cand, int n, int32_t *status, int32_t *coord,
                                  void *H, void *G, int64_t *n_undecided) {
    if (!ctx || !s) return MAD_EINVAL;
    if (n_undecided) *n_undecided = 0;
    if (n < 0) return mad_fail(ctx, MAD_EINVAL, "mad_space_localize: n = %d", n);
    if (entry < 0 || entry >= s->n_oct) return mad_fail(ctx, MAD_EINVAL, "mad_space_localize: entry %d of %d", entry, s->n_oct);
    if (n == 0) return MAD_OK;
    if (!cand || !status || !coord || !H || !G) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    const Octave &O = s->oct[entry];
    MAD_TRY(localize_check(ctx, "mad_space_localize", O.d, cand, n));
    return localize_run(ctx, O.logv, O.f64, O.d, cand, n, status, coord, H, G, n_undecided);
}

extern "C" int mad_localize_volume(mad_ctx *ctx, const void *vol, int is_f64, int nx, int ny, int nz, const int32_t *cand, int n,
                                   int32_t *status, int32_t *coord, void *H, void *G, int64_t *n_undecided) {
    if (!ctx) return MAD_EINVAL;
    if (n_undecided) *n_undecided = 0;
    if (n < 0) return mad_fail(ctx, MAD_EINVAL, "mad_localize_volume: n = %d", n);
    if (is_f64 != 0 && is_f64 != 1) return mad_fail(ctx, MAD_EINVAL, "mad_localize_volume: is_f64 = %d", is_f64);
    if (n == 0) return MAD_OK;
    if (!vol || !cand || !status || !coord || !H || !G) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    const Dims d{{nx, ny, nz}};
    MAD_TRY(localize_check(ctx, "mad_localize_volume", d, cand, n));
    const size_t bytes = d.count() * (is_f64 ? 8 : 4);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), bytes));
    MAD_HIP(hipMemcpyAsync(mad_sb(ctx, S_TMP_C).p, vol, bytes, hipMemcpyHostToDevice, ctx->stream));
    return localize_run(ctx, mad_sb(ctx, S_TMP_C).p, is_f64 == 1, d, cand, n, status, coord, H, G, n_undecided);
}
