// mad_mapops.hip -- a map against a map: Dmap.mask_with (mad/Dmap.py:99-151) and Dmap.get_CCC_with_dmap (mad/Dmap.py:260-372).
//
// Both kernels stream grids of float32 [x][y][z] (z fastest) as flat arrays in chunks of four voxels -- one 16-byte load per lane,
// a wave reads 1 KiB in a piece -- and split a chunk's flat index into (x, y, z) once, carrying over the row ends from voxel to
// voxel.  The voxels of the OTHER grid that belong to a chunk are consecutive along z as well, but start wherever the offset
// between the grids puts them: four 4-byte loads per lane, still contiguous across the wave.
//
// Determinism: no floating-point atomics.  k_map_ccc leaves MAPCCC_WGS partial sums per second map -- always that many, whatever
// the sizes and however many maps share the launch -- and k_map_ccc_combine adds them in a fixed order: the same inputs give the
// same bits, run to run, alone or in a batch.
#include <algorithm>
#include <vector>

#include "mad_common.h"

#define MAPOP_THREADS 256
#define MAPCCC_WGS 512          // workgroups = partial sums per second map (and for the count of grid 1)
#define MAPCCC_MAX_N 32767      // second maps in one call (gridDim.y, with one slice for grid 1)

// ---------------------------------------------------------------------------
// mask_with
// ---------------------------------------------------------------------------

struct MaskArgs {
    float *g;                   // grid 1, edited in place
    const float *mask;          // grid 2
    unsigned long long n;       // voxels of grid 1
    int ny, nz;                 // grid 1
    int my, mz;                 // grid 2
    int lo[3], hi[3];           // planes of grid 1 that python's slices leave: lo <= i < hi
    int sh[3];                  // mask index = grid index - sh
    int use_mask;               // 0: the reference's slice of the mask is empty (np.where of nothing zeroes nothing)
};

// Dmap.py:141-151 in one pass: a voxel outside the kept range of any axis, or inside it over a mask voxel < float32(1e-8)
// (numpy compares a float32 array with a python scalar in float32), becomes 0; every other voxel is not written at all.
__global__ __launch_bounds__(MAPOP_THREADS) void k_map_mask(const MaskArgs A) {
    const float thr = (float)1e-8;
    const size_t n_chunk = (size_t)((A.n + 3) >> 2);
    for (size_t c = (size_t)blockIdx.x * MAPOP_THREADS + threadIdx.x; c < n_chunk; c += (size_t)gridDim.x * MAPOP_THREADS) {
        const size_t i0 = c << 2;
        const bool full = i0 + 4 <= A.n;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (full) {
            const float4 q = *(const float4 *)(A.g + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int k = 0; k < 4; k++)
                if (i0 + k < A.n) v[k] = A.g[i0 + k];
        }
        const unsigned t = (unsigned)i0 / (unsigned)A.nz;
        int z = (int)((unsigned)i0 - t * (unsigned)A.nz), y = (int)(t % (unsigned)A.ny), x = (int)(t / (unsigned)A.ny);
        bool changed = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            bool keep = x >= A.lo[0] && x < A.hi[0] && y >= A.lo[1] && y < A.hi[1] && z >= A.lo[2] && z < A.hi[2];
            if (keep && A.use_mask && (full || i0 + k < A.n)) {
                const float m = A.mask[((size_t)(x - A.sh[0]) * A.my + (y - A.sh[1])) * A.mz + (z - A.sh[2])];
                keep = !(m < thr);
            }
            if (!keep && __float_as_uint(v[k]) != 0u) { v[k] = 0.f; changed = true; }
            if (++z == A.nz) { z = 0; if (++y == A.ny) { y = 0; x++; } }
        }
        if (!changed) continue;
        if (full) *(float4 *)(A.g + i0) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int k = 0; k < 4; k++)
                if (i0 + k < A.n) A.g[i0 + k] = v[k];
    }
}

// One axis of Dmap.py:118-149 with python's slice semantics.  s = round(o2 / voxsp - o1 / voxsp) (half to even), min = max(s, 0),
// max = min(n1, n2 + s); `grid[:min] = 0` and `grid[max:] = 0` leave the planes of `grid[min:max]` -- a NEGATIVE max counts from the
// end in both --, and the mask is read through `mask[min - s : max - s]`.
struct MaskAxis { long lo, hi, m_lo, m_hi; };
static MaskAxis mask_axis(long n1, long n2, double o1, double o2, double voxsp) {
    const long s = py_round(o2 / voxsp - o1 / voxsp);
    const long mn = s > 0 ? s : 0, mx = n1 < n2 + s ? n1 : n2 + s;
    const long ms = mn - s, me = mx - s;
    MaskAxis a;
    a.lo = mn < n1 ? mn : n1;
    a.hi = mx < 0 ? (n1 + mx > 0 ? n1 + mx : 0) : (mx < n1 ? mx : n1);
    a.m_lo = ms < n2 ? ms : n2;
    a.m_hi = me < 0 ? (n2 + me > 0 ? n2 + me : 0) : (me < n2 ? me : n2);
    if (a.hi < a.lo) a.hi = a.lo;
    if (a.m_hi < a.m_lo) a.m_hi = a.m_lo;
    return a;
}

// (origins within 1e15 voxels of 0: their differences are rounded to long)
static int map_check(mad_ctx *ctx, const char *who, const int32_t d[3], const double o[3], double voxsp, size_t *n) {
    for (int k = 0; k < 3; k++) {
        if (d[k] <= 0) return mad_fail(ctx, MAD_EINVAL, "%s: empty grid (%d x %d x %d)", who, d[0], d[1], d[2]);
        if (!(fabs(o[k] / voxsp) < 1e15)) return mad_fail(ctx, MAD_EINVAL, "%s: origin %g at voxsp %g", who, o[k], voxsp);
    }
    const unsigned long long v = (unsigned long long)d[0] * (unsigned long long)d[1];
    if (v >= (1ull << 32) || v * (unsigned long long)d[2] >= (1ull << 32))
        return mad_fail(ctx, MAD_EINVAL, "%s: %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, d[0], d[1], d[2]);
    *n = (size_t)(v * (unsigned long long)d[2]);
    return MAD_OK;
}

extern "C" int mad_map_mask(mad_ctx *ctx, float *grid1, const int32_t d1[3], const double o1[3], const float *mask, const int32_t d2[3],
                            const double o2[3], double voxsp) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !mask || !d1 || !d2 || !o1 || !o2) return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_mask: NULL argument") : MAD_EINVAL;
    if (!(voxsp > 0) || !(voxsp < 1e15)) return mad_fail(ctx, MAD_EINVAL, "mad_map_mask: voxsp %g", voxsp);
    size_t n1 = 0, n2 = 0;
    MAD_TRY(map_check(ctx, "mad_map_mask", d1, o1, voxsp, &n1));
    MAD_TRY(map_check(ctx, "mad_map_mask", d2, o2, voxsp, &n2));
    MaskArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n1; A.ny = d1[1]; A.nz = d1[2]; A.my = d2[1]; A.mz = d2[2];
    bool left = true, selected = true;      // something of the map is left / of the mask is selected
    for (int k = 0; k < 3; k++) {
        const MaskAxis a = mask_axis(d1[k], d2[k], o1[k], o2[k], voxsp);
        A.lo[k] = (int)a.lo; A.hi[k] = (int)a.hi; A.sh[k] = (int)(a.lo - a.m_lo);
        if (a.hi == a.lo) left = false;
        if (a.m_hi == a.m_lo) selected = false;
    }
    A.use_mask = left && selected ? 1 : 0;
    if (A.use_mask)      // where both slices are non-empty they are equally long (0 <= min <= max): every mask index is inside grid 2
        for (int k = 0; k < 3; k++)
            if (A.lo[k] - A.sh[k] < 0 || A.hi[k] - A.sh[k] > d2[k]) return mad_fail(ctx, MAD_EDOM, "mad_map_mask: axis %d: the two slices differ", k);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n1 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (n2 + 4) * 4));
    A.g = scratch<float>(ctx, S_TMP_H);
    float *d_mask = scratch<float>(ctx, S_TMP_I);
    A.mask = d_mask;
    MAD_HIP(hipMemcpyAsync(A.g, grid1, n1 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (A.use_mask) MAD_HIP(hipMemcpyAsync(d_mask, mask, n2 * 4, hipMemcpyHostToDevice, ctx->stream));
    const int blocks = (int)std::min<int64_t>(mad_ceil_div((int64_t)((n1 + 3) >> 2), MAPOP_THREADS), (int64_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(k_map_mask, dim3(blocks), dim3(MAPOP_THREADS), 0, ctx->stream, A);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(grid1, A.g, n1 * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// ---------------------------------------------------------------------------
// multiply by a soft mask
// ---------------------------------------------------------------------------

struct MulArgs {
    float *g;                   // grid 1, edited in place
    const float *mask;          // grid 2
    unsigned long long n;       // voxels of grid 1
    int ny, nz;                 // grid 1
    int my, mz;                 // grid 2
    int lo[3], hi[3];           // the mask's box in grid 1: lo <= i < hi (empty on an axis: the boxes do not meet)
    int sh[3];                  // mask index = grid index - sh
};

// g = (float)((double)g * (double)m) under the mask's box, +0 outside it; a voxel under m == 1 is not written (every bit stays).
// The walk over chunks of four voxels is k_map_mask's.
__global__ __launch_bounds__(MAPOP_THREADS) void k_map_multiply(const MulArgs A) {
    const size_t n_chunk = (size_t)((A.n + 3) >> 2);
    for (size_t c = (size_t)blockIdx.x * MAPOP_THREADS + threadIdx.x; c < n_chunk; c += (size_t)gridDim.x * MAPOP_THREADS) {
        const size_t i0 = c << 2;
        const bool full = i0 + 4 <= A.n;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (full) {
            const float4 q = *(const float4 *)(A.g + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int k = 0; k < 4; k++)
                if (i0 + k < A.n) v[k] = A.g[i0 + k];
        }
        const unsigned t = (unsigned)i0 / (unsigned)A.nz;
        int z = (int)((unsigned)i0 - t * (unsigned)A.nz), y = (int)(t % (unsigned)A.ny), x = (int)(t / (unsigned)A.ny);
        bool changed = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (full || i0 + k < A.n) {
                const bool in = x >= A.lo[0] && x < A.hi[0] && y >= A.lo[1] && y < A.hi[1] && z >= A.lo[2] && z < A.hi[2];
                if (in) {
                    const float m = A.mask[((size_t)(x - A.sh[0]) * A.my + (y - A.sh[1])) * A.mz + (z - A.sh[2])];
                    if (m != 1.f) { v[k] = (float)((double)v[k] * (double)m); changed = true; }
                } else if (__float_as_uint(v[k]) != 0u) { v[k] = 0.f; changed = true; }
            }
            if (++z == A.nz) { z = 0; if (++y == A.ny) { y = 0; x++; } }
        }
        if (!changed) continue;
        if (full) *(float4 *)(A.g + i0) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int k = 0; k < 4; k++)
                if (i0 + k < A.n) A.g[i0 + k] = v[k];
    }
}

extern "C" int mad_map_multiply(mad_ctx *ctx, float *grid1, const int32_t d1[3], const double o1[3], const float *mask, const int32_t d2[3],
                                const double o2[3], double voxsp) {
    const char *who = "mad_map_multiply";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !mask || !d1 || !d2 || !o1 || !o2) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (!(voxsp > 0) || !(voxsp < 1e15)) return mad_fail(ctx, MAD_EINVAL, "%s: voxsp %g", who, voxsp);
    size_t n1 = 0, n2 = 0;
    MAD_TRY(map_check(ctx, who, d1, o1, voxsp, &n1));
    MAD_TRY(map_check(ctx, who, d2, o2, voxsp, &n2));
    MulArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n1; A.ny = d1[1]; A.nz = d1[2]; A.my = d2[1]; A.mz = d2[2];
    bool meet = true;
    for (int k = 0; k < 3; k++) {
        const long s = py_round(o2[k] / voxsp - o1[k] / voxsp);      // mad_map_mask's offset (mask_axis)
        const long lo = s > 0 ? s : 0, hi = (long)d1[k] < (long)d2[k] + s ? (long)d1[k] : (long)d2[k] + s;
        if (hi <= lo) { meet = false; continue; }      // (s itself may be far outside an int)
        A.lo[k] = (int)lo; A.hi[k] = (int)hi; A.sh[k] = (int)s;      // 0 <= lo - s and hi - s <= d2: every mask index is inside grid 2
    }
    if (!meet)
        for (int k = 0; k < 3; k++) { A.lo[k] = 0; A.hi[k] = 0; A.sh[k] = 0; }
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n1 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (n2 + 4) * 4));
    A.g = scratch<float>(ctx, S_TMP_H);
    float *d_mask = scratch<float>(ctx, S_TMP_I);
    A.mask = d_mask;
    MAD_HIP(hipMemcpyAsync(A.g, grid1, n1 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (meet) MAD_HIP(hipMemcpyAsync(d_mask, mask, n2 * 4, hipMemcpyHostToDevice, ctx->stream));
    const int blocks = (int)std::min<int64_t>(mad_ceil_div((int64_t)((n1 + 3) >> 2), MAPOP_THREADS), (int64_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(k_map_multiply, dim3(blocks), dim3(MAPOP_THREADS), 0, ctx->stream, A);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(grid1, A.g, n1 * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// ---------------------------------------------------------------------------
// get_CCC_with_dmap
// ---------------------------------------------------------------------------

struct MapJob {
    unsigned long long off2;      // where grid 2 begins in the pool (elements, a multiple of 4)
    unsigned long long n2;        // its voxels
    int d2[3];
    int s1[3], s2[3], e[3];       // the common box: start in grid 1, start in grid 2, extent (0: the boxes miss each other)
};

// Slice blockIdx.y < n_jobs: ONE pass over second map blockIdx.y.  Every voxel counts towards n2 (m2 > iso); a voxel inside the common
// box fetches its voxel of grid 1 and adds to c1 (m1 > iso inside the box), common, S1, S2 and D (Dmap.py:354-366; float32
// comparisons, float64 sums: the product of two float32 is exact there).
// Slice blockIdx.y == n_jobs: the voxels of grid 1 OUTSIDE the box of the first second map, counted (m1 > iso); with that map's c1
// they are the whole-grid count of grid 1 (Dmap.py:354) -- once per call, and no voxel of grid 1 is read twice for one map.
// part_f [slice][workgroup][3] = S1, S2, D; part_i [slice][workgroup][3] = n2, common, c1 (the last slice: count, 0, 0).
__global__ __launch_bounds__(MAPOP_THREADS) void k_map_ccc(const MapJob *__restrict__ jobs, int n_jobs, const float *__restrict__ g1, int ax,
                                                           int ay, int az, const float *__restrict__ pool, float iso,
                                                           double *__restrict__ part_f, long long *__restrict__ part_i) {
    __shared__ double wf[MAPOP_THREADS / MAD_WAVE][3];
    __shared__ int wi[MAPOP_THREADS / MAD_WAVE][3];
    const bool count1 = (int)blockIdx.y == n_jobs;
    const MapJob &J = jobs[count1 ? 0 : blockIdx.y];
    double S1 = 0, S2 = 0, D = 0;
    int c2 = 0, com = 0, c1 = 0;      // a thread sees at most 2^32 / (MAPCCC_WGS * 256) * 4 voxels
    const unsigned ex = J.e[0], ey = J.e[1], ez = J.e[2];
    if (!count1) {
        const float *g2 = pool + J.off2;
        const size_t n = (size_t)J.n2, n_chunk = (n + 3) >> 2;
        const unsigned ny = J.d2[1], nz = J.d2[2];
        for (size_t c = (size_t)blockIdx.x * MAPOP_THREADS + threadIdx.x; c < n_chunk; c += (size_t)gridDim.x * MAPOP_THREADS) {
            const size_t i0 = c << 2;
            const int nv = i0 + 4 <= n ? 4 : (int)(n - i0);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (nv == 4) {
                const float4 q = *(const float4 *)(g2 + i0);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int k = 0; k < nv; k++) v[k] = g2[i0 + k];
            }
            const unsigned t = (unsigned)i0 / nz;
            unsigned z = (unsigned)i0 - t * nz, y = t % ny, x = t / ny;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k < nv) {
                    const float m2 = v[k];
                    c2 += m2 > iso ? 1 : 0;
                    const unsigned bx = x - (unsigned)J.s2[0], by = y - (unsigned)J.s2[1], bz = z - (unsigned)J.s2[2];      // below the start: wraps past any extent
                    if (bx < ex && by < ey && bz < ez) {
                        const float m1 = g1[((size_t)(J.s1[0] + bx) * ay + (J.s1[1] + by)) * az + (J.s1[2] + bz)];
                        c1 += m1 > iso ? 1 : 0;
                        com += (m2 != 0.f && m2 > iso && m1 > iso) ? 1 : 0;      // np.count_nonzero of the selected VALUES (:355)
                        const double a = m1, b = m2;
                        if (m2 > 0.f) S1 += a * a;      // :362
                        if (m1 > 0.f) S2 += b * b;      // :363 (dividing grid 1 by a norm does not change which voxels are > 0)
                        D += a * b;                     // :366
                    }
                }
                if (++z == nz) { z = 0; if (++y == ny) { y = 0; x++; } }
            }
        }
    } else {
        const size_t n = (size_t)ax * ay * az, n_chunk = (n + 3) >> 2;
        const unsigned ny = ay, nz = az;
        for (size_t c = (size_t)blockIdx.x * MAPOP_THREADS + threadIdx.x; c < n_chunk; c += (size_t)gridDim.x * MAPOP_THREADS) {
            const size_t i0 = c << 2;
            const int nv = i0 + 4 <= n ? 4 : (int)(n - i0);
            const unsigned t = (unsigned)i0 / nz;
            unsigned z = (unsigned)i0 - t * nz, y = t % ny, x = t / ny;
            const unsigned bx0 = x - (unsigned)J.s1[0], by0 = y - (unsigned)J.s1[1], bz0 = z - (unsigned)J.s1[2];
            // all four voxels in one row and inside the box: the map's own pass has counted them, nothing to read
            if (nv == 4 && z + 3 < nz && bx0 < ex && by0 < ey && bz0 < ez && bz0 + 3 < ez) continue;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (nv == 4) {
                const float4 q = *(const float4 *)(g1 + i0);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int k = 0; k < nv; k++) v[k] = g1[i0 + k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k < nv) {
                    const unsigned bx = x - (unsigned)J.s1[0], by = y - (unsigned)J.s1[1], bz = z - (unsigned)J.s1[2];
                    if (!(bx < ex && by < ey && bz < ez)) c2 += v[k] > iso ? 1 : 0;
                }
                if (++z == nz) { z = 0; if (++y == ny) { y = 0; x++; } }
            }
        }
    }
    S1 = wave_sum_f64(S1); S2 = wave_sum_f64(S2); D = wave_sum_f64(D);
    c2 = wave_sum_i32(c2); com = wave_sum_i32(com); c1 = wave_sum_i32(c1);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { wf[w][0] = S1; wf[w][1] = S2; wf[w][2] = D; wi[w][0] = c2; wi[w][1] = com; wi[w][2] = c1; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const size_t o = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + threadIdx.x;
        part_f[o] = ((wf[0][threadIdx.x] + wf[1][threadIdx.x]) + wf[2][threadIdx.x]) + wf[3][threadIdx.x];
        part_i[o] = (long long)wi[0][threadIdx.x] + wi[1][threadIdx.x] + wi[2][threadIdx.x] + wi[3][threadIdx.x];
    }
}
static_assert(MAPOP_THREADS == 4 * MAD_WAVE, "k_map_ccc adds four waves");

// One workgroup: wave w takes slices w, w + 4, ...; lane l adds partials l, l + 64, ... in that order, then the lanes are added by
// the butterfly of wave_sum_f64.  out_f / out_i [slice][3].
__global__ __launch_bounds__(MAPOP_THREADS) void k_map_ccc_combine(int n_slices, int n_part, const double *__restrict__ part_f,
                                                                   const long long *__restrict__ part_i, double *__restrict__ out_f,
                                                                   long long *__restrict__ out_i) {
    const int lane = lane_id();
    for (int s = threadIdx.x >> 6; s < n_slices; s += MAPOP_THREADS / MAD_WAVE) {
        double f[3] = {0, 0, 0};
        long long c[3] = {0, 0, 0};
        for (int p = lane; p < n_part; p += MAD_WAVE)
#pragma unroll
            for (int q = 0; q < 3; q++) {
                f[q] += part_f[((size_t)s * n_part + p) * 3 + q];
                c[q] += part_i[((size_t)s * n_part + p) * 3 + q];
            }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            f[q] = wave_sum_f64(f[q]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c[q] += __shfl_xor(c[q], o, MAD_WAVE);
        }
        if (lane < 3) {
            out_f[(size_t)s * 3 + lane] = lane == 0 ? f[0] : (lane == 1 ? f[1] : f[2]);
            out_i[(size_t)s * 3 + lane] = lane == 0 ? c[0] : (lane == 1 ? c[1] : c[2]);
        }
    }
}

extern "C" int mad_map_ccc(mad_ctx *ctx, const float *grid1, const int32_t d1[3], const double o1[3], int n, const float *const *grids2,
                           const int32_t *dims2, const double *origins2, double voxsp, double isovalue, double *out) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !d1 || !o1 || !grids2 || !dims2 || !origins2 || !out)
        return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_ccc: NULL argument") : MAD_EINVAL;
    if (n <= 0 || n > MAPCCC_MAX_N) return mad_fail(ctx, MAD_EINVAL, "mad_map_ccc: %d second maps in one call (1 .. %d)", n, MAPCCC_MAX_N);
    if (!(voxsp > 0) || !(voxsp < 1e15)) return mad_fail(ctx, MAD_EINVAL, "mad_map_ccc: voxsp %g", voxsp);
    if (!(isovalue == isovalue)) return mad_fail(ctx, MAD_EINVAL, "mad_map_ccc: isovalue NaN");
    size_t n1 = 0, tot = 0;
    MAD_TRY(map_check(ctx, "mad_map_ccc", d1, o1, voxsp, &n1));
    std::vector<MapJob> jobs(n);
    for (int j = 0; j < n; j++) {
        if (!grids2[j]) return mad_fail(ctx, MAD_EINVAL, "mad_map_ccc: second map %d is NULL", j);
        size_t n2 = 0;
        MAD_TRY(map_check(ctx, "mad_map_ccc", dims2 + 3 * j, origins2 + 3 * j, voxsp, &n2));
        MapJob &J = jobs[j];
        memset(&J, 0, sizeof(J));
        J.off2 = tot; J.n2 = n2;
        tot += (n2 + 3) & ~(size_t)3;      // every map begins on a 16-byte boundary
        long mn1[3], mn2[3], e[3];
        const bool any = ccc_overlap(d1, o1, dims2 + 3 * j, origins2 + 3 * j, voxsp, mn1, mn2, e) && e[0] > 0 && e[1] > 0 && e[2] > 0;
        for (int k = 0; k < 3; k++) {
            J.d2[k] = dims2[3 * j + k];
            J.s1[k] = any ? (int)mn1[k] : 0; J.s2[k] = any ? (int)mn2[k] : 0; J.e[k] = any ? (int)e[k] : 0;
            // the box lies inside both grids (ccc_overlap clamps its slices like python): nothing is fetched out of bounds
            if (any && (J.s1[k] < 0 || J.s2[k] < 0 || J.s1[k] + J.e[k] > d1[k] || J.s2[k] + J.e[k] > J.d2[k]))
                return mad_fail(ctx, MAD_EDOM, "mad_map_ccc: second map %d: box outside a grid on axis %d", j, k);
        }
    }
    const size_t n_slices = (size_t)n + 1, bytes_jobs = ((size_t)n * sizeof(MapJob) + 15) & ~(size_t)15;
    const size_t bytes_part = n_slices * MAPCCC_WGS * 3 * 8, bytes_out = n_slices * 3 * 8;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n1 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (tot + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), bytes_jobs + 2 * bytes_part + 2 * bytes_out));
    float *g1 = scratch<float>(ctx, S_TMP_H), *pool = scratch<float>(ctx, S_TMP_I);
    char *blk = scratch<char>(ctx, S_TMP_G);
    MapJob *d_jobs = (MapJob *)blk;
    double *part_f = (double *)(blk + bytes_jobs), *out_f = (double *)(blk + bytes_jobs + 2 * bytes_part);
    long long *part_i = (long long *)(blk + bytes_jobs + bytes_part), *out_i = (long long *)(blk + bytes_jobs + 2 * bytes_part + bytes_out);
    MAD_HIP(hipMemcpyAsync(g1, grid1, n1 * 4, hipMemcpyHostToDevice, ctx->stream));      // once, however many second maps
    for (int j = 0; j < n; j++) MAD_HIP(hipMemcpyAsync(pool + jobs[j].off2, grids2[j], (size_t)jobs[j].n2 * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(MapJob), hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_CCC);
    hipLaunchKernelGGL(k_map_ccc, dim3(MAPCCC_WGS, (unsigned)n_slices), dim3(MAPOP_THREADS), 0, ctx->stream, (const MapJob *)d_jobs, n,
                       (const float *)g1, d1[0], d1[1], d1[2], (const float *)pool, (float)isovalue, part_f, part_i);
    hipLaunchKernelGGL(k_map_ccc_combine, dim3(1), dim3(MAPOP_THREADS), 0, ctx->stream, (int)n_slices, MAPCCC_WGS, (const double *)part_f,
                       (const long long *)part_i, out_f, out_i);
    mad_timer_end(ctx, MAD_T_CCC);
    MAD_HIP(hipGetLastError());
    std::vector<double> hf(n_slices * 3);
    std::vector<long long> hi(n_slices * 3);
    MAD_HIP(hipMemcpyAsync(hf.data(), out_f, bytes_out, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(hi.data(), out_i, bytes_out, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    const long long c_1 = hi[(size_t)n * 3] + hi[2];      // grid 1 above the isovalue: outside the first map's box + inside it
    for (int j = 0; j < n; j++) {
        const long long c_2 = hi[(size_t)j * 3], common = hi[(size_t)j * 3 + 1], smaller = c_1 < c_2 ? c_1 : c_2;
        if (!common || !smaller) { out[j] = 0.0; continue; }      // Dmap.py:356-357
        out[j] = hf[(size_t)j * 3 + 2] / (sqrt(hf[(size_t)j * 3]) * sqrt(hf[(size_t)j * 3 + 1])) * (double)common / (double)smaller;
    }
    return MAD_OK;
}
