// mad_resample_taps.h -- what mad_resample.hip and mad_symmetry.hip share (DESIGN.md sections 4h and 4y): the checks of a grid and
// of a motion (R, T), the fold of a motion into u = b + A j, and the interpolated value at an output voxel.  One statement of each,
// so that a value mad_map_symmetry_score or mad_map_symmetrize forms is the value mad_map_resample forms, bit for bit.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

// index i in [-1, n + 1] of an axis of n >= 2 samples, mirrored about sample 0 and sample n - 1 (period 2 (n - 1))
__host__ __device__ static inline int rs_mirror(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return i < 0 ? -i : i;
}

// weights of the taps f - 1 .. f + 2 (ORDER 3) or f, f + 1 (ORDER 1) at t = u - f
template <int ORDER> __host__ __device__ static inline void rs_weights(double t, double *w) {
    if (ORDER == 1) { w[0] = 1.0 - t; w[1] = t; return; }
    const double r = 1.0 - t, t2 = t * t, t3 = t2 * t;
    w[0] = r * r * r / 6.0;
    w[1] = (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0;
    w[2] = (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0;
    w[3] = t3 / 6.0;
}

struct RsGeo {
    int n[3], m[3];             // source and output dims
    double A[9], b[3];          // u = b + A j
};

// the float64 value at output voxel (jx, jy, jz) before it is rounded: +0.0 outside the source, never -0.0 (every sum begins at +0.0)
template <int ORDER, typename SRC>
__device__ __forceinline__ double rs_value(const SRC *__restrict__ src, const RsGeo &G, int jx, int jy, int jz) {
    constexpr int NT = ORDER == 1 ? 2 : 4, LO = ORDER == 1 ? 0 : -1;
    double w[3][NT];
    int idx[3][NT];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double u = ((G.b[a] + G.A[3 * a] * (double)jx) + G.A[3 * a + 1] * (double)jy) + G.A[3 * a + 2] * (double)jz;
        if (!(u >= 0.0 && u <= (double)(G.n[a] - 1))) return 0.0;
        const double f = floor(u);
        rs_weights<ORDER>(u - f, w[a]);
#pragma unroll
        for (int k = 0; k < NT; k++) idx[a][k] = rs_mirror((int)f + LO + k, G.n[a]);
    }
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < NT; a++) {
        double sy = 0.0;
#pragma unroll
        for (int b = 0; b < NT; b++) {
            const SRC *row = src + ((size_t)idx[0][a] * G.n[1] + idx[1][b]) * (size_t)G.n[2];
            double sz = 0.0;
#pragma unroll
            for (int k = 0; k < NT; k++) sz += w[2][k] * (double)row[idx[2][k]];
            sy += w[1][b] * sz;
        }
        acc += w[0][a] * sy;
    }
    return acc;
}

template <int ORDER, typename SRC>
__device__ __forceinline__ float rs_sample(const SRC *__restrict__ src, const RsGeo &G, int jx, int jy, int jz) {
    return (float)rs_value<ORDER, SRC>(src, G, jx, jy, jz);
}

static inline bool rs_finite(const double *v, int n) {
    for (int k = 0; k < n; k++)
        if (!std::isfinite(v[k])) return false;
    return true;
}

static inline bool rs_voxels(const int32_t d[3], size_t *n) {
    const unsigned long long v = (unsigned long long)d[0] * (unsigned long long)d[1];
    if (v >= (1ull << 32) || v * (unsigned long long)d[2] >= (1ull << 32)) return false;
    *n = (size_t)(v * (unsigned long long)d[2]);
    return true;
}

// what mad_map_resample accepts as a rotation: max|R R^T - I| <= 1e-9 and det R >= 0 (R finite); *dev and *det for the message
static inline bool rs_rotation_ok(const double *R, double *dev_out, double *det_out) {
    double dev = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double d = (R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
            dev = std::max(dev, fabs(d));
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (dev_out) *dev_out = dev;
    if (det_out) *det_out = det;
    return !(dev > 1e-9 || det < 0);
}

// u = ((p + w j - T) @ R^T - o) / v as u = b + A j (mad_amd/resample.py::affine, the same expressions)
static inline void rs_fold(const double *R, const double *T, const double origin[3], double voxsp, const double out_origin[3], double out_voxsp,
                           double A[9], double b[3]) {
    for (int a = 0; a < 3; a++) {
        for (int k = 0; k < 3; k++) A[3 * a + k] = (R[3 * a + k] * out_voxsp) / voxsp;
        b[a] = ((((out_origin[0] - T[0]) * R[3 * a] + (out_origin[1] - T[1]) * R[3 * a + 1]) + (out_origin[2] - T[2]) * R[3 * a + 2]) - origin[a]) / voxsp;
    }
}
