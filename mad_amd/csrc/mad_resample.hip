// mad_resample.hip -- a map sampled on another lattice: trilinear (order 1) or cubic B-spline (order 3) interpolation of a grid of
// float32 [x][y][z] (z fastest) at the points of a second lattice, with an optional rigid motion of the source.  The contract is
// output voxel j takes the source value at index u = b + A j (float64, evaluated as
// ((b_a + A_a0 jx) + A_a1 jy) + A_a2 jz), the interpolated value where 0 <= u_a <= n_a - 1 on every axis and exactly 0.0f elsewhere;
// taps outside the grid are mirrored about the first and last sample; every sum is float64 and is rounded to float32 once.  This is
// scipy.ndimage.map_coordinates(order, mode="constant", cval=0, prefilter=True) on the float64 copy of the grid.
//
//   k_bspline_axis / k_bspline_axis_z   one pass of the recursive prefilter (pole sqrt(3) - 2) along x or y / along z
//   k_resample<ORDER>                   the general form: 8 or 64 taps per output voxel, output in compact bricks
//   k_resample_axis / k_resample_z      the axis-aligned form: three 1-D passes of 2 or 4 taps from per-axis tables
//   k_symmetrize<ORDER>                 mad_map_symmetrize (section 4y): the general form's value under up to 64 motions, averaged
//
// The taps, the fold of a motion and the checks of a grid are in mad_resample_taps.h, which mad_symmetry.hip shares.
//
// Determinism: no atomics, and no sum depends on the launch geometry.
#include <algorithm>
#include <vector>

#include "mad_common.h"
#include "mad_resample_taps.h"

#define RS_THREADS 256
#define RS_K 40                 // terms of the causal start value: |pole|^40 = 1.3e-23
#define RS_ZB 256               // k_bspline_axis_z: lines of a workgroup's bundle (one per thread)
#define RS_ZC 16                // ... z samples of a chunk
#define RS_ZP (RS_ZC + 1)       // ... padded LDS row: an odd count of doubles, so the threads' 8-byte accesses fall on distinct banks
#define RS_BX 4                 // k_resample: a workgroup's brick of the output is 4 x 8 x 32 voxels, a lane's share 1 x 1 x 4
#define RS_BY 8
#define RS_BZ 32
static_assert(RS_BX * RS_BY * (RS_BZ / 4) == RS_THREADS, "one lane per four z outputs of the brick");

// ---------------------------------------------------------------------------
// prefilter
// ---------------------------------------------------------------------------

// With x_i = gain g_i, a line's coefficients are: c+_0 = sum over the mirrored line of pole^i x_i, c+_i = x_i + pole c+_(i-1);
// c_(n-1) = zfac (c+_(n-1) + pole c+_(n-2)), c_i = pole (c_(i+1) - c+_i).  The start value in closed form is
// (sum_i w_i x_i) / den with w_0 = 1, w_(n-1) = pole^(n-1), w_i = pole^i + pole^(2n-2-i) otherwise and den = 1 - pole^(2n-2);
// terms from i = RS_K on are dropped.  tab = [w_0 .. w_(RS_K-1) | pole^0 .. pole^(RS_K-1)] in global memory.
struct PrefArgs {
    double z, gain, zfac, den;
    const double *tab;
};

// Along x or y: one thread per line, neighbouring threads take neighbouring z (line L begins at (L / inner) * outer_stride +
// L % inner, its samples are `stride` apart), so every access of a wave is contiguous.  SRC = float: the pass that also widens the
// source; SRC = double: in place (in == c).
template <typename SRC>
__global__ __launch_bounds__(RS_THREADS) void k_bspline_axis(const SRC *in, double *c, size_t n_lines, size_t inner, size_t outer_stride,
                                                             size_t stride, int n, const PrefArgs P) {
    const size_t L = (size_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (L >= n_lines) return;
    const size_t off = (L / inner) * outer_stride + L % inner;
    const int k0 = n < RS_K ? n : RS_K;
    double s = 0.0;
    for (int i = 0; i < k0; i++) s += P.tab[i] * (P.gain * (double)in[off + (size_t)i * stride]);
    double cp = s / P.den, pm = 0.0;
    c[off] = cp;
    int i = 1;
    for (; i + 4 <= n; i += 4) {      // four loads in flight per trip: the recurrence itself is serial
        const size_t o = off + (size_t)i * stride;
        const double x0 = P.gain * (double)in[o], x1 = P.gain * (double)in[o + stride], x2 = P.gain * (double)in[o + 2 * stride],
                     x3 = P.gain * (double)in[o + 3 * stride];
        const double c0 = x0 + P.z * cp, c1 = x1 + P.z * c0, c2 = x2 + P.z * c1, c3 = x3 + P.z * c2;
        c[o] = c0; c[o + stride] = c1; c[o + 2 * stride] = c2; c[o + 3 * stride] = c3;
        pm = c2; cp = c3;
    }
    for (; i < n; i++) {
        const size_t o = off + (size_t)i * stride;
        pm = cp;
        cp = P.gain * (double)in[o] + P.z * cp;
        c[o] = cp;
    }
    double cl = P.zfac * (cp + P.z * pm);
    c[off + (size_t)(n - 1) * stride] = cl;
    i = n - 2;
    for (; i >= 3; i -= 4) {
        const size_t o = off + (size_t)i * stride;
        const double v0 = c[o], v1 = c[o - stride], v2 = c[o - 2 * stride], v3 = c[o - 3 * stride];
        const double c0 = P.z * (cl - v0), c1 = P.z * (c0 - v1), c2 = P.z * (c1 - v2), c3 = P.z * (c2 - v3);
        c[o] = c0; c[o - stride] = c1; c[o - 2 * stride] = c2; c[o - 3 * stride] = c3;
        cl = c3;
    }
    for (; i >= 0; i--) {
        const size_t o = off + (size_t)i * stride;
        cl = P.z * (cl - c[o]);
        c[o] = cl;
    }
}

// The [nl lines] x [len samples from z0] piece of the bundle that begins at line L0, between global memory and LDS.  A lane moves an
// even-aligned pair of doubles (16 bytes) wherever both belong to the piece, and the odd sample at either end of a line alone.
template <bool TO_LDS>
__device__ __forceinline__ void bspline_z_move(double *c, double *lds, size_t L0, int nl, int n, int z0, int len) {
    const int slots = RS_ZC / 2 + 1;      // pairs that can touch RS_ZC samples beginning at an odd element
    for (int s = threadIdx.x; s < nl * slots; s += RS_THREADS) {
        const int l = s / slots, q = s - l * slots;
        const size_t first = (L0 + l) * (size_t)n + z0, e = (first & ~(size_t)1) + 2 * (size_t)q;
        const bool v0 = e >= first && e < first + len, v1 = e + 1 >= first && e + 1 < first + len;
        double *row = lds + l * RS_ZP;
        if (v0 && v1) {
            if (TO_LDS) { const double2 v = *(const double2 *)(c + e); row[e - first] = v.x; row[e + 1 - first] = v.y; }
            else *(double2 *)(c + e) = make_double2(row[e - first], row[e + 1 - first]);
        } else if (v0) {
            if (TO_LDS) row[e - first] = c[e]; else c[e] = row[e - first];
        } else if (v1) {
            if (TO_LDS) row[e + 1 - first] = c[e + 1]; else c[e + 1] = row[e + 1 - first];
        }
    }
}

// Along z, in place: the line is the contiguous direction.  A workgroup takes RS_ZB consecutive lines and carries them through LDS
// RS_ZC samples at a time, forwards and then backwards; thread l runs line l's recurrence on its LDS row.  The forward sweep starts
// from x_0 instead of the start value and gathers that value's sum on the way; since the recurrence is linear, the true c+_i is the
// stored one + pole^i delta with delta = start - x_0, which the backward sweep adds to the first RS_K samples as it reads them.
__global__ __launch_bounds__(RS_THREADS) void k_bspline_axis_z(double *c, size_t n_lines, int n, const PrefArgs P) {
    __shared__ double lds[RS_ZB * RS_ZP];
    const size_t L0 = (size_t)blockIdx.x * RS_ZB;
    const int nl = (int)(n_lines - L0 < (size_t)RS_ZB ? n_lines - L0 : (size_t)RS_ZB);
    const bool active = (int)threadIdx.x < nl;
    double *row = lds + threadIdx.x * RS_ZP;
    const int n_chunks = (n + RS_ZC - 1) / RS_ZC;
    double s = 0.0, x0 = 0.0, cp = 0.0, pm = 0.0;
    for (int ch = 0; ch < n_chunks; ch++) {
        const int z0 = ch * RS_ZC, len = n - z0 < RS_ZC ? n - z0 : RS_ZC;
        bspline_z_move<true>(c, lds, L0, nl, n, z0, len);
        __syncthreads();
        if (active)
            for (int k = 0; k < len; k++) {
                const int i = z0 + k;
                const double x = P.gain * row[k];
                if (i < RS_K) s += P.tab[i] * x;
                if (i == 0) { x0 = x; cp = x; }
                else { pm = cp; cp = x + P.z * cp; }
                row[k] = cp;
            }
        __syncthreads();
        bspline_z_move<false>(c, lds, L0, nl, n, z0, len);
        __syncthreads();
    }
    const double delta = s / P.den - x0;
    const double *zp = P.tab + RS_K;
    if (n - 1 < RS_K) cp += zp[n - 1] * delta;
    if (n - 2 < RS_K) pm += zp[n - 2] * delta;
    double cl = P.zfac * (cp + P.z * pm);
    for (int ch = n_chunks - 1; ch >= 0; ch--) {
        const int z0 = ch * RS_ZC, len = n - z0 < RS_ZC ? n - z0 : RS_ZC;
        bspline_z_move<true>(c, lds, L0, nl, n, z0, len);
        __syncthreads();
        if (active)
            for (int k = len - 1; k >= 0; k--) {
                const int i = z0 + k;
                if (i < n - 1) {
                    double v = row[k];
                    if (i < RS_K) v += zp[i] * delta;
                    cl = P.z * (cl - v);
                }
                row[k] = cl;
            }
        __syncthreads();
        bspline_z_move<false>(c, lds, L0, nl, n, z0, len);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// interpolation
// ---------------------------------------------------------------------------

// rs_mirror, rs_weights, RsGeo, rs_value / rs_sample: mad_resample_taps.h (shared with mad_symmetry.hip)

// The general form.  ORDER 1 reads the float32 source, ORDER 3 the float64 coefficients.  Workgroup blockIdx.x takes brick
// (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3) of the bricks counted z fastest: workgroups b and b + 8 share an XCD, so every XCD
// works through one contiguous run of bricks, neighbours in z first, and the taps they share meet in that XCD's L2.
template <int ORDER, typename SRC>
__global__ __launch_bounds__(RS_THREADS) void k_resample(const SRC *__restrict__ src, float *__restrict__ out, const RsGeo G, unsigned bricks_y,
                                                         unsigned bricks_z, unsigned n_bricks, unsigned per_xcd) {
    const unsigned brick = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (brick >= n_bricks) return;
    const unsigned bz = brick % bricks_z, t = brick / bricks_z, by = t % bricks_y, bx = t / bricks_y;
    const int jx = (int)(bx * RS_BX + (threadIdx.x >> 6)), jy = (int)(by * RS_BY + ((threadIdx.x >> 3) & 7)),
              jz = (int)(bz * RS_BZ + (threadIdx.x & 7) * 4);
    if (jx >= G.m[0] || jy >= G.m[1] || jz >= G.m[2]) return;
    const int nv = G.m[2] - jz < 4 ? G.m[2] - jz : 4;
    const size_t o = ((size_t)jx * G.m[1] + jy) * (size_t)G.m[2] + jz;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < nv) v[k] = rs_sample<ORDER, SRC>(src, G, jx, jy, jz + k);
    if (nv == 4 && (o & 3) == 0) *(float4 *)(out + o) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < nv) out[o + k] = v[k];
    }
}

// One output index of one axis in the axis-aligned form: the mirrored tap indices and their weights; idx[0] < 0: outside the source.
struct AxisTap {
    double w[4];
    int idx[4];
};

// four consecutive elements from i: one or two 16-byte accesses where i is a multiple of 4 and all four exist, else one by one
__device__ __forceinline__ void rs_load4(const float *p, size_t i, int nv, double *v) {
    if (nv == 4 && (i & 3) == 0) { const float4 q = *(const float4 *)(p + i); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else
        for (int k = 0; k < 4; k++) v[k] = k < nv ? (double)p[i + k] : 0.0;
}
__device__ __forceinline__ void rs_load4(const double *p, size_t i, int nv, double *v) {
    if (nv == 4 && (i & 3) == 0) {
        const double2 q = *(const double2 *)(p + i), r = *(const double2 *)(p + i + 2);
        v[0] = q.x; v[1] = q.y; v[2] = r.x; v[3] = r.y;
    } else
        for (int k = 0; k < 4; k++) v[k] = k < nv ? p[i + k] : 0.0;
}
__device__ __forceinline__ void rs_store4(float *p, size_t i, int nv, const double *v) {
    if (nv == 4 && (i & 3) == 0) *(float4 *)(p + i) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    else
        for (int k = 0; k < 4; k++)
            if (k < nv) p[i + k] = (float)v[k];
}
__device__ __forceinline__ void rs_store4(double *p, size_t i, int nv, const double *v) {
    if (nv == 4 && (i & 3) == 0) { *(double2 *)(p + i) = make_double2(v[0], v[1]); *(double2 *)(p + i + 2) = make_double2(v[2], v[3]); }
    else
        for (int k = 0; k < 4; k++)
            if (k < nv) p[i + k] = v[k];
}

// One pass of the axis-aligned form along x or y: in [outer][n_in][inner] -> out [outer][n_out][inner], out[o][j][r] = sum_k
// w_k(j) in[o][idx_k(j)][r], or 0 where j is outside.  A lane owns four consecutive r.
template <int ORDER, typename SRC, typename DST>
__global__ __launch_bounds__(RS_THREADS) void k_resample_axis(const SRC *__restrict__ in, DST *__restrict__ out, const AxisTap *__restrict__ tab,
                                                              size_t outer, int n_in, int n_out, size_t inner) {
    constexpr int NT = ORDER == 1 ? 2 : 4;
    const size_t nq = (inner + 3) >> 2, total = outer * (size_t)n_out * nq;
    for (size_t it = (size_t)blockIdx.x * RS_THREADS + threadIdx.x; it < total; it += (size_t)gridDim.x * RS_THREADS) {
        const size_t rq = it % nq, t = it / nq, j = t % (size_t)n_out, o = t / (size_t)n_out;
        const size_t r0 = rq << 2;
        const int nv = inner - r0 < 4 ? (int)(inner - r0) : 4;
        const AxisTap T = tab[j];
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (T.idx[0] >= 0) {
#pragma unroll
            for (int k = 0; k < NT; k++) {
                double v[4];
                rs_load4(in, (o * (size_t)n_in + (size_t)T.idx[k]) * inner + r0, nv, v);
#pragma unroll
                for (int e = 0; e < 4; e++) acc[e] += T.w[k] * v[e];
            }
        }
        rs_store4(out, (o * (size_t)n_out + j) * inner + r0, nv, acc);
    }
}

// The pass along z: in [rows][n_in] -> out [rows][n_out].  A lane owns four consecutive z outputs, each with its own taps.
template <int ORDER, typename SRC, typename DST>
__global__ __launch_bounds__(RS_THREADS) void k_resample_z(const SRC *__restrict__ in, DST *__restrict__ out, const AxisTap *__restrict__ tab,
                                                           size_t rows, int n_in, int n_out) {
    constexpr int NT = ORDER == 1 ? 2 : 4;
    const size_t nq = ((size_t)n_out + 3) >> 2, total = rows * nq;
    for (size_t it = (size_t)blockIdx.x * RS_THREADS + threadIdx.x; it < total; it += (size_t)gridDim.x * RS_THREADS) {
        const size_t row = it / nq, j0 = (it - row * nq) << 2;
        const int nv = (size_t)n_out - j0 < 4 ? (int)((size_t)n_out - j0) : 4;
        const SRC *line = in + row * (size_t)n_in;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e >= nv) continue;
            const AxisTap T = tab[j0 + e];
            if (T.idx[0] < 0) continue;
#pragma unroll
            for (int k = 0; k < NT; k++) acc[e] += T.w[k] * (double)line[T.idx[k]];
        }
        rs_store4(out, row * (size_t)n_out + j0, nv, acc);
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

static int rs_blocks(mad_ctx *ctx, size_t items) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(mad_ceil_div((int64_t)items, RS_THREADS), (int64_t)ctx->n_cu * 16));
}

template <int ORDER, typename SRC, typename DST>
static void rs_launch_pass(mad_ctx *ctx, int axis, const SRC *in, DST *out, const AxisTap *tab, const size_t cur[3], int n_out) {
    if (axis == 2) {
        const size_t rows = cur[0] * cur[1];
        hipLaunchKernelGGL((k_resample_z<ORDER, SRC, DST>), dim3(rs_blocks(ctx, rows * (((size_t)n_out + 3) >> 2))), dim3(RS_THREADS), 0,
                           ctx->stream, in, out, tab, rows, (int)cur[2], n_out);
    } else {
        const size_t outer = axis == 0 ? 1 : cur[0], inner = axis == 0 ? cur[1] * cur[2] : cur[2];
        hipLaunchKernelGGL((k_resample_axis<ORDER, SRC, DST>), dim3(rs_blocks(ctx, outer * (size_t)n_out * ((inner + 3) >> 2))),
                           dim3(RS_THREADS), 0, ctx->stream, in, out, tab, outer, (int)cur[axis], n_out, inner);
    }
}

// the three passes of the axis-aligned form, the pass that shrinks the volume most first; first: float32 source (ORDER 1) or
// float64 coefficients (ORDER 3)
template <int ORDER, typename SRC>
static void rs_separable(mad_ctx *ctx, const SRC *first, const int32_t n[3], const int32_t m[3], const AxisTap *tab, double *t1, double *t2,
                         float *out, const int order_of_axes[3]) {
    size_t cur[3] = {(size_t)n[0], (size_t)n[1], (size_t)n[2]};
    const AxisTap *tabs[3] = {tab, tab + m[0], tab + m[0] + m[1]};
    int a = order_of_axes[0];
    rs_launch_pass<ORDER, SRC, double>(ctx, a, first, t1, tabs[a], cur, m[a]);
    cur[a] = (size_t)m[a];
    a = order_of_axes[1];
    rs_launch_pass<ORDER, double, double>(ctx, a, (const double *)t1, t2, tabs[a], cur, m[a]);
    cur[a] = (size_t)m[a];
    a = order_of_axes[2];
    rs_launch_pass<ORDER, double, float>(ctx, a, (const double *)t2, out, tabs[a], cur, m[a]);
}

template <int ORDER, typename SRC> static void rs_general(mad_ctx *ctx, const SRC *src, float *out, const RsGeo &G) {
    const unsigned bx = (unsigned)mad_ceil_div(G.m[0], RS_BX), by = (unsigned)mad_ceil_div(G.m[1], RS_BY), bz = (unsigned)mad_ceil_div(G.m[2], RS_BZ);
    const unsigned n_bricks = bx * by * bz, per_xcd = (n_bricks + 7) / 8;
    hipLaunchKernelGGL((k_resample<ORDER, SRC>), dim3(per_xcd * 8), dim3(RS_THREADS), 0, ctx->stream, src, out, G, by, bz, n_bricks, per_xcd);
}

// The prefilter of the float32 source d_src into the float64 coefficients d_coef, three passes; d_small takes the three axes' tables
// (3 * 2 * RS_K doubles), staged in the caller's h_pref, which lives until the caller has synchronised.
static int rs_prefilter(mad_ctx *ctx, const int32_t dims[3], const float *d_src, double *d_coef, char *d_small, double (*h_pref)[2 * RS_K]) {
    const size_t bytes_pref = 2 * RS_K * sizeof(double);
    const double z = sqrt(3.0) - 2.0;
    PrefArgs P[3];
    for (int a = 0; a < 3; a++) {
        const int n = dims[a];
        for (int i = 0; i < RS_K; i++) {
            h_pref[a][i] = i == 0 ? 1.0 : (i == n - 1 ? pow(z, (double)i) : (i < n ? pow(z, (double)i) + pow(z, (double)(2 * n - 2 - i)) : 0.0));
            h_pref[a][RS_K + i] = pow(z, (double)i);
        }
        P[a].z = z; P[a].gain = (1.0 - z) * (1.0 - 1.0 / z); P[a].zfac = z / (z * z - 1.0);
        P[a].den = 1.0 - pow(z, (double)(2 * n - 2));
        P[a].tab = (const double *)(d_small + a * bytes_pref);
    }
    MAD_HIP(hipMemcpyAsync(d_small, h_pref, 3 * bytes_pref, hipMemcpyHostToDevice, ctx->stream));
    const size_t nyz = (size_t)dims[1] * dims[2], nxz = (size_t)dims[0] * dims[2], nxy = (size_t)dims[0] * dims[1];
    hipLaunchKernelGGL((k_bspline_axis<float>), dim3((unsigned)mad_ceil_div((int64_t)nyz, RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream,
                       (const float *)d_src, d_coef, nyz, nyz, (size_t)0, nyz, dims[0], P[0]);
    hipLaunchKernelGGL((k_bspline_axis<double>), dim3((unsigned)mad_ceil_div((int64_t)nxz, RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream,
                       (const double *)d_coef, d_coef, nxz, (size_t)dims[2], nyz, (size_t)dims[2], dims[1], P[1]);
    hipLaunchKernelGGL(k_bspline_axis_z, dim3((unsigned)mad_ceil_div((int64_t)nxy, RS_ZB)), dim3(RS_THREADS), 0, ctx->stream, d_coef, nxy,
                       dims[2], P[2]);
    return MAD_OK;
}

extern "C" int mad_map_resample(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp,
                                const double *R9, const double *T3, int order, const int32_t out_dims[3], const double out_origin[3],
                                double out_voxsp, float *out) {
    const char *who = "mad_map_resample";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !origin || !out_dims || !out_origin || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (order != 1 && order != 3) return mad_fail(ctx, MAD_EINVAL, "%s: order %d (1 or 3)", who, order);
    if ((R9 == nullptr) != (T3 == nullptr)) return mad_fail(ctx, MAD_EINVAL, "%s: R and T come together or not at all", who);
    for (int k = 0; k < 3; k++) {
        if (dims[k] < 2) return mad_fail(ctx, MAD_EINVAL, "%s: source of %d x %d x %d voxels: every axis needs 2", who, dims[0], dims[1], dims[2]);
        if (out_dims[k] <= 0) return mad_fail(ctx, MAD_EINVAL, "%s: output of %d x %d x %d voxels", who, out_dims[0], out_dims[1], out_dims[2]);
    }
    if (!rs_finite(origin, 3) || !rs_finite(out_origin, 3) || !std::isfinite(voxsp) || !std::isfinite(out_voxsp) || (R9 && !rs_finite(R9, 9)) ||
        (T3 && !rs_finite(T3, 3)))
        return mad_fail(ctx, MAD_EINVAL, "%s: a number that is not finite", who);
    if (!(voxsp > 0) || !(out_voxsp > 0)) return mad_fail(ctx, MAD_EINVAL, "%s: voxsp %g -> %g", who, voxsp, out_voxsp);
    size_t n_src = 0, n_out = 0;
    if (!rs_voxels(dims, &n_src) || !rs_voxels(out_dims, &n_out))
        return mad_fail(ctx, MAD_EINVAL, "%s: %d x %d x %d -> %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, dims[0], dims[1],
                        dims[2], out_dims[0], out_dims[1], out_dims[2]);
    static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero3[3] = {0, 0, 0};
    const double *R = R9 ? R9 : eye, *T = T3 ? T3 : zero3;
    if (R9) {
        double dev = 0.0, det = 0.0;
        if (!rs_rotation_ok(R, &dev, &det)) return mad_fail(ctx, MAD_EINVAL, "%s: R is no rotation (max|R R^T - I| = %g, det %g)", who, dev, det);
    }
    RsGeo G;
    for (int a = 0; a < 3; a++) { G.n[a] = dims[a]; G.m[a] = out_dims[a]; }
    rs_fold(R, T, origin, voxsp, out_origin, out_voxsp, G.A, G.b);
    if (!rs_finite(G.A, 9) || !rs_finite(G.b, 3)) return mad_fail(ctx, MAD_EINVAL, "%s: the lattices are too far apart for float64", who);
    const char *env = getenv("MAD_RESAMPLE_GENERAL");      // read per call: both forms can run in one process
    const bool general = memcmp(R, eye, sizeof(eye)) != 0 || (env && env[0] && strcmp(env, "0") != 0);

    // the axis-aligned form's plan: pass order (the smallest m / n first) and the sizes of its two intermediates
    int ax[3] = {0, 1, 2};
    std::stable_sort(ax, ax + 3, [&](int p, int q) { return (double)out_dims[p] / dims[p] < (double)out_dims[q] / dims[q]; });
    size_t n_t1 = 0, n_t2 = 0;
    if (!general) {
        size_t cur[3] = {(size_t)dims[0], (size_t)dims[1], (size_t)dims[2]};
        cur[ax[0]] = (size_t)out_dims[ax[0]];
        n_t1 = cur[0] * cur[1] * cur[2];
        cur[ax[1]] = (size_t)out_dims[ax[1]];
        n_t2 = cur[0] * cur[1] * cur[2];
        if (n_t1 >= (1ull << 34) || n_t2 >= (1ull << 34)) return mad_fail(ctx, MAD_EINVAL, "%s: an intermediate of the separable passes has 2^34 voxels or more", who);
    }
    const size_t n_tab = (size_t)out_dims[0] + out_dims[1] + out_dims[2];
    std::vector<AxisTap> tab;
    if (!general) {
        tab.resize(n_tab);
        size_t e = 0;
        for (int a = 0; a < 3; a++)
            for (int j = 0; j < out_dims[a]; j++, e++) {
                AxisTap &t = tab[e];
                memset(&t, 0, sizeof(t));
                const double u = G.b[a] + G.A[4 * a] * (double)j;      // the off-diagonal terms of the general expression are + 0.0
                if (!(u >= 0.0 && u <= (double)(dims[a] - 1))) { t.idx[0] = -1; continue; }
                const double f = floor(u);
                if (order == 1) rs_weights<1>(u - f, t.w); else rs_weights<3>(u - f, t.w);
                for (int k = 0; k < (order == 1 ? 2 : 4); k++) {
                    t.idx[k] = rs_mirror((int)f + (order == 1 ? 0 : -1) + k, dims[a]);
                    if (t.idx[k] < 0 || t.idx[k] >= dims[a]) return mad_fail(ctx, MAD_EDOM, "%s: axis %d: tap %d of output %d outside the source", who, a, k, j);
                }
            }
    }
    // scratch: source, coefficients, intermediates, output, small tables -- the ctx's, reused from call to call
    const size_t bytes_pref = 2 * RS_K * sizeof(double), bytes_small = 3 * bytes_pref + n_tab * sizeof(AxisTap) + 64;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n_src + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (n_out + 4) * 4));
    if (order == 3) MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (n_src + 4) * 8));
    if (!general) {
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), (n_t1 + 4) * 8));
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), (n_t2 + 4) * 8));
    }
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), bytes_small));
    float *d_src = scratch<float>(ctx, S_TMP_H), *d_out = scratch<float>(ctx, S_TMP_I);
    double *d_coef = scratch<double>(ctx, S_TMP_A), *d_t1 = scratch<double>(ctx, S_TMP_B), *d_t2 = scratch<double>(ctx, S_TMP_C);
    char *d_small = scratch<char>(ctx, S_TMP_G);
    AxisTap *d_tab = (AxisTap *)(d_small + 3 * bytes_pref);
    MAD_HIP(hipMemcpyAsync(d_src, grid, n_src * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!general) MAD_HIP(hipMemcpyAsync(d_tab, tab.data(), n_tab * sizeof(AxisTap), hipMemcpyHostToDevice, ctx->stream));
    double h_pref[3][2 * RS_K];
    if (order == 3) MAD_TRY(rs_prefilter(ctx, dims, d_src, d_coef, d_small, h_pref));
    if (general) {
        if (order == 1) rs_general<1, float>(ctx, d_src, d_out, G);
        else rs_general<3, double>(ctx, d_coef, d_out, G);
    } else {
        if (order == 1) rs_separable<1, float>(ctx, d_src, dims, out_dims, d_tab, d_t1, d_t2, d_out, ax);
        else rs_separable<3, double>(ctx, d_coef, dims, out_dims, d_tab, d_t1, d_t2, d_out, ax);
    }
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out, d_out, n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// ---------------------------------------------------------------------------
// the average over a set of motions
// ---------------------------------------------------------------------------

#define SYMZ_MAX_OPS 64

// out[j] = (float)((sum over g of v_g) / n_ops), v_g = rs_value of the source moved by operator g at voxel j of the source's own
// lattice, the sum from +0.0 in the order g = 0, 1, ...; ops[g] = A[9] then b[3].  The bricks and their order over the XCDs are
// k_resample's; the operators are uniform over the launch, so their coefficients are scalar loads.
template <int ORDER, typename SRC>
__global__ __launch_bounds__(RS_THREADS) void k_symmetrize(const SRC *__restrict__ src, float *__restrict__ out, const double *__restrict__ ops, int n_ops,
                                                           int nx, int ny, int nz, unsigned bricks_y, unsigned bricks_z, unsigned n_bricks,
                                                           unsigned per_xcd) {
    const unsigned brick = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (brick >= n_bricks) return;
    const unsigned bz = brick % bricks_z, t = brick / bricks_z, by = t % bricks_y, bx = t / bricks_y;
    const int jx = (int)(bx * RS_BX + (threadIdx.x >> 6)), jy = (int)(by * RS_BY + ((threadIdx.x >> 3) & 7)),
              jz = (int)(bz * RS_BZ + (threadIdx.x & 7) * 4);
    if (jx >= nx || jy >= ny || jz >= nz) return;
    const int nv = nz - jz < 4 ? nz - jz : 4;
    const size_t o = ((size_t)jx * ny + jy) * (size_t)nz + jz;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    RsGeo G;
    G.n[0] = G.m[0] = nx; G.n[1] = G.m[1] = ny; G.n[2] = G.m[2] = nz;
    for (int g = 0; g < n_ops; g++) {
        const double *q = ops + (size_t)12 * g;
#pragma unroll
        for (int k = 0; k < 9; k++) G.A[k] = q[k];
#pragma unroll
        for (int k = 0; k < 3; k++) G.b[k] = q[9 + k];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < nv) acc[k] += rs_value<ORDER, SRC>(src, G, jx, jy, jz + k);
    }
    const double n = (double)n_ops;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < nv) out[o + k] = (float)(acc[k] / n);
}

extern "C" int mad_map_symmetrize(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp, int32_t n_ops,
                                  const double *R9, const double *T3, int order, float *out) {
    const char *who = "mad_map_symmetrize";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !origin || !R9 || !T3 || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (order != 1 && order != 3) return mad_fail(ctx, MAD_EINVAL, "%s: order %d (1 or 3)", who, order);
    if (n_ops < 1 || n_ops > SYMZ_MAX_OPS) return mad_fail(ctx, MAD_EINVAL, "%s: %d operators (1 .. %d)", who, n_ops, SYMZ_MAX_OPS);
    for (int k = 0; k < 3; k++)
        if (dims[k] < 2) return mad_fail(ctx, MAD_EINVAL, "%s: source of %d x %d x %d voxels: every axis needs 2", who, dims[0], dims[1], dims[2]);
    if (!rs_finite(origin, 3) || !std::isfinite(voxsp) || !rs_finite(R9, 9 * n_ops) || !rs_finite(T3, 3 * n_ops))
        return mad_fail(ctx, MAD_EINVAL, "%s: a number that is not finite", who);
    if (!(voxsp > 0)) return mad_fail(ctx, MAD_EINVAL, "%s: voxsp %g", who, voxsp);
    size_t n_src = 0;
    if (!rs_voxels(dims, &n_src))
        return mad_fail(ctx, MAD_EINVAL, "%s: %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
    std::vector<double> ops((size_t)12 * n_ops);
    for (int g = 0; g < n_ops; g++) {
        double dev = 0.0, det = 0.0;
        if (!rs_rotation_ok(R9 + 9 * g, &dev, &det))
            return mad_fail(ctx, MAD_EINVAL, "%s: R of operator %d is no rotation (max|R R^T - I| = %g, det %g)", who, g, dev, det);
        rs_fold(R9 + 9 * g, T3 + 3 * g, origin, voxsp, origin, voxsp, &ops[(size_t)12 * g], &ops[(size_t)12 * g + 9]);
        if (!rs_finite(&ops[(size_t)12 * g], 12)) return mad_fail(ctx, MAD_EINVAL, "%s: operator %d moves the map too far for float64", who, g);
    }
    const size_t bytes_pref = 2 * RS_K * sizeof(double), bytes_ops = ops.size() * sizeof(double);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n_src + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (n_src + 4) * 4));
    if (order == 3) MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (n_src + 4) * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), 3 * bytes_pref + bytes_ops + 64));
    float *d_src = scratch<float>(ctx, S_TMP_H), *d_out = scratch<float>(ctx, S_TMP_I);
    double *d_coef = scratch<double>(ctx, S_TMP_A);
    char *d_small = scratch<char>(ctx, S_TMP_G);
    double *d_ops = (double *)(d_small + 3 * bytes_pref);
    MAD_HIP(hipMemcpyAsync(d_src, grid, n_src * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_ops, ops.data(), bytes_ops, hipMemcpyHostToDevice, ctx->stream));
    double h_pref[3][2 * RS_K];
    if (order == 3) MAD_TRY(rs_prefilter(ctx, dims, d_src, d_coef, d_small, h_pref));      // once per call, whatever n_ops
    const unsigned bx = (unsigned)mad_ceil_div(dims[0], RS_BX), by = (unsigned)mad_ceil_div(dims[1], RS_BY), bz = (unsigned)mad_ceil_div(dims[2], RS_BZ);
    const unsigned n_bricks = bx * by * bz, per_xcd = (n_bricks + 7) / 8;
    mad_timer_begin(ctx, MAD_T_SYM_AVERAGE);
    if (order == 1)
        hipLaunchKernelGGL((k_symmetrize<1, float>), dim3(per_xcd * 8), dim3(RS_THREADS), 0, ctx->stream, (const float *)d_src, d_out, (const double *)d_ops,
                           (int)n_ops, dims[0], dims[1], dims[2], by, bz, n_bricks, per_xcd);
    else
        hipLaunchKernelGGL((k_symmetrize<3, double>), dim3(per_xcd * 8), dim3(RS_THREADS), 0, ctx->stream, (const double *)d_coef, d_out,
                           (const double *)d_ops, (int)n_ops, dims[0], dims[1], dims[2], by, bz, n_bricks, per_xcd);
    mad_timer_end(ctx, MAD_T_SYM_AVERAGE);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out, d_out, n_src * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}
