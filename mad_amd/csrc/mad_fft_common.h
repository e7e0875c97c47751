// mad_fft_common.h -- what the transforms of mad_fourier.hip and mad_localres.hip share: complex128 arithmetic on double2 (no fused
// multiply-adds: the Makefile's -ffp-contract=off) and the exactly reduced roots of unity of the host tables.
#pragma once

#include "mad_common.h"

__device__ __forceinline__ double2 c_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 c_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 c_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 c_muli(double2 a) { return make_double2(-a.y, a.x); }      // i a

// cos and sin of 2 pi k / N, the angle reduced exactly (in integers) to [0, pi / 4] first; N a power of two >= 8
static inline void unit_root(int k, int N, double *c, double *s) {
    const int quad = N / 4, q = (k / quad) & 3, m = k % quad;
    double cm, sm;
    if (m <= N / 8) { cm = cos(2.0 * M_PI * (double)m / (double)N); sm = sin(2.0 * M_PI * (double)m / (double)N); }
    else { cm = sin(2.0 * M_PI * (double)(quad - m) / (double)N); sm = cos(2.0 * M_PI * (double)(quad - m) / (double)N); }
    if (m == 0) { cm = 1.0; sm = 0.0; }
    switch (q) {
    case 0: *c = cm; *s = sm; break;
    case 1: *c = -sm; *s = cm; break;
    case 2: *c = -cm; *s = -sm; break;
    default: *c = sm; *s = -cm; break;
    }
}
