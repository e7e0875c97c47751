// mad_zone.hip -- a map cut around a structure, or with the structure erased: the "zone" operation.  The contract is DESIGN.md
// section 4i: voxel j sits at p_a = origin_a + voxsp * j_a, D2 is the minimum over the atoms of (dx*dx + dy*dy) + dz*dz (float64, no
// FMA), the weight is 1 where D2 <= radius^2, 0 where D2 >= (radius + soft)^2 and a raised cosine of sqrt(D2) in between, `erase`
// takes 1 - w; a voxel of weight 1 is not written, one of weight 0 becomes +0.0f, any other (float)((double)g * w).
//
//   k_zone_count / k_zone_scan / k_zone_fill   the atoms within reach of the map's box, binned into a uniform cell grid
//   k_map_zone                                 a workgroup per brick of 4 x 8 x 32 voxels, the atoms in reach of it staged through LDS
//
// Determinism: a minimum does not depend on the order of its terms, so neither the order of the atoms inside a cell (integer atomics
// hand out the slots) nor the order in which a workgroup stages them reaches a result.  The two counts are integer tallies.  No
// floating-point atomics.
#include <algorithm>

#include "mad_common.h"

#define ZN_THREADS 256
#define ZN_BX 4                 // a workgroup's brick is 4 x 8 x 32 voxels, a lane's share 1 x 1 x 4 (the brick of k_resample)
#define ZN_BY 8
#define ZN_BZ 32
#define ZN_CHUNK 1024           // atoms of one LDS chunk (24 KiB)
#define ZN_MAXC 64              // cells per axis at most: 64^3 cells, whatever the reach is against the box
#define ZN_SCAN_THREADS 1024
#define ZN_ROUND (1u << 22)     // workgroups of one launch of k_map_zone
static_assert(ZN_BX * ZN_BY * (ZN_BZ / 4) == ZN_THREADS, "one lane per four z voxels of the brick");
static_assert(ZN_CHUNK >= 2 * ZN_THREADS, "a staging step adds up to ZN_THREADS atoms to a chunk that is not full");

struct ZoneGeo {
    int n[3];                   // voxels
    int nc[3];                  // cells
    double o[3], voxsp;         // voxel j of axis a at o[a] + voxsp * j
    double lo[3], hi[3];        // the first and the last voxel of every axis: o + voxsp * 0, o + voxsp * (n - 1)
    double glo[3], h;           // cell c of axis a begins at glo[a] + h * c
    double radius, soft, r2, R, R2;
};

// zone_box_d2, the squared distance from an atom to a box that both culls below use, is in mad_common.h (k_group_fit shares it)

// cell of coordinate v on axis a, before clamping; monotone in v
__device__ __forceinline__ double zone_cell_f(const ZoneGeo &G, int a, double v) { return floor((v - G.glo[a]) / G.h); }
__device__ __forceinline__ int zone_clamp_cell(const ZoneGeo &G, int a, double c) {
    return c < 0.0 ? 0 : (c > (double)(G.nc[a] - 1) ? G.nc[a] - 1 : (int)c);
}

// cell_of[i] = the atom's cell, or -1 where it is farther than R from the box (boxd2 > R2: it is dropped, never clamped into an edge
// cell);
// cnt[cell] counts.
__global__ __launch_bounds__(ZN_THREADS) void k_zone_count(const double *__restrict__ atoms, unsigned n_atoms, const ZoneGeo G,
                                                           int *__restrict__ cell_of, unsigned *__restrict__ cnt) {
    const unsigned i = blockIdx.x * ZN_THREADS + threadIdx.x;
    if (i >= n_atoms) return;
    const double x[3] = {atoms[3 * (size_t)i], atoms[3 * (size_t)i + 1], atoms[3 * (size_t)i + 2]};
    int cell = -1;
    if (zone_box_d2(x, G.lo, G.hi) <= G.R2) {
        const int cx = zone_clamp_cell(G, 0, zone_cell_f(G, 0, x[0])), cy = zone_clamp_cell(G, 1, zone_cell_f(G, 1, x[1])),
                  cz = zone_clamp_cell(G, 2, zone_cell_f(G, 2, x[2]));
        cell = (cx * G.nc[1] + cy) * G.nc[2] + cz;
        atomicAdd(cnt + cell, 1u);
    }
    cell_of[i] = cell;
}

// One workgroup: start[c] = atoms in the cells before c (start[n_cells] = all that were kept), cursor[c] = start[c].
__global__ __launch_bounds__(ZN_SCAN_THREADS) void k_zone_scan(const unsigned *__restrict__ cnt, int n_cells, unsigned *__restrict__ start,
                                                               unsigned *__restrict__ cursor) {
    __shared__ int warp_tot[ZN_SCAN_THREADS / MAD_WAVE + 1];
    const int per = (n_cells + ZN_SCAN_THREADS - 1) / ZN_SCAN_THREADS, c0 = threadIdx.x * per, c1 = c0 + per < n_cells ? c0 + per : n_cells;
    int s = 0;
    for (int c = c0; c < c1; c++) s += (int)cnt[c];
    int total = 0;
    int run = block_excl_scan(s, warp_tot, &total);
    for (int c = c0; c < c1; c++) {
        start[c] = (unsigned)run;
        cursor[c] = (unsigned)run;
        run += (int)cnt[c];
    }
    if (c0 < n_cells && c1 == n_cells) start[n_cells] = (unsigned)run;
}

__global__ __launch_bounds__(ZN_THREADS) void k_zone_fill(const double *__restrict__ atoms, unsigned n_atoms, const int *__restrict__ cell_of,
                                                          unsigned *__restrict__ cursor, double *__restrict__ sorted) {
    const unsigned i = blockIdx.x * ZN_THREADS + threadIdx.x;
    if (i >= n_atoms) return;
    const int cell = cell_of[i];
    if (cell < 0) return;
    const size_t slot = atomicAdd(cursor + cell, 1u);
    sorted[3 * slot] = atoms[3 * (size_t)i];
    sorted[3 * slot + 1] = atoms[3 * (size_t)i + 1];
    sorted[3 * slot + 2] = atoms[3 * (size_t)i + 2];
}

// the n staged atoms against the lane's four voxels
__device__ __forceinline__ void zone_min_chunk(const double *s_at, int n, double px, double py, const double pz[4], double D2[4]) {
    for (int a = 0; a < n; a++) {      // every lane reads the same address: a broadcast
        const double dx = px - s_at[3 * a], dy = py - s_at[3 * a + 1], az = s_at[3 * a + 2];
        const double t = dx * dx + dy * dy;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double dz = pz[k] - az, d2 = t + dz * dz;
            D2[k] = d2 < D2[k] ? d2 : D2[k];
        }
    }
}

// Workgroup w = wg0 + blockIdx.x takes brick (w & 7) * per_xcd + (w >> 3) of the bricks counted z fastest (k_resample's order; wg0 is
// a multiple of 8: the launch is cut into rounds of ZN_ROUND workgroups, since a grid may not have 2^32 threads).  The cells that can
// hold an atom within R of the brick are those from cell(bl - R) - 1 to cell(bh + R) + 1 per axis (bl, bh: the brick's first and
// last voxel; the cell function is monotone, the spare cell on either side covers its rounding and the clamping of the binned
// index).  Along z those cells are one contiguous run of the sorted atoms per (cx, cy); the workgroup walks the runs ZN_THREADS
// atoms at a time, keeps the atoms with zone_box_d2(brick) <= R2 in the LDS chunk, and works a chunk off when the next step might
// not fit.  counts[0] += voxels with D2 <= r2, counts[1] += voxels with r2 < D2 < R2.
__global__ __launch_bounds__(ZN_THREADS) void k_map_zone(float *__restrict__ g, const double *__restrict__ sorted, const unsigned *__restrict__ start,
                                                         unsigned long long *__restrict__ counts, const ZoneGeo G, int erase, unsigned bricks_y,
                                                         unsigned bricks_z, unsigned n_bricks, unsigned per_xcd, unsigned wg0) {
    __shared__ double s_at[ZN_CHUNK * 3];
    __shared__ int s_n;
    __shared__ int s_cnt[ZN_THREADS / MAD_WAVE][2];
    const unsigned wg = wg0 + blockIdx.x, brick = (wg & 7u) * per_xcd + (wg >> 3);
    if (brick >= n_bricks) return;      // the whole workgroup
    const unsigned bz = brick % bricks_z, bt = brick / bricks_z, by = bt % bricks_y, bx = bt / bricks_y;
    const int j0[3] = {(int)(bx * ZN_BX), (int)(by * ZN_BY), (int)(bz * ZN_BZ)};
    const int jx = j0[0] + (int)(threadIdx.x >> 6), jy = j0[1] + (int)((threadIdx.x >> 3) & 7), jz = j0[2] + (int)(threadIdx.x & 7) * 4;
    const int nv = (jx < G.n[0] && jy < G.n[1] && jz < G.n[2]) ? (G.n[2] - jz < 4 ? G.n[2] - jz : 4) : 0;
    const double px = G.o[0] + G.voxsp * (double)jx, py = G.o[1] + G.voxsp * (double)jy;
    double pz[4], D2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        pz[k] = G.o[2] + G.voxsp * (double)(jz + k);
        D2[k] = INFINITY;
    }
    // the brick's own box and its cells
    const int bdim[3] = {ZN_BX, ZN_BY, ZN_BZ};
    double bl[3], bh[3];
    int clo[3], chi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int last = j0[a] + bdim[a] - 1 < G.n[a] - 1 ? j0[a] + bdim[a] - 1 : G.n[a] - 1;
        bl[a] = G.o[a] + G.voxsp * (double)j0[a];
        bh[a] = G.o[a] + G.voxsp * (double)last;
        clo[a] = zone_clamp_cell(G, a, zone_cell_f(G, a, bl[a] - G.R) - 1.0);
        chi[a] = zone_clamp_cell(G, a, zone_cell_f(G, a, bh[a] + G.R) + 1.0);
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int staged = 0;
    bool any = false;
    for (int cx = clo[0]; cx <= chi[0]; cx++)
        for (int cy = clo[1]; cy <= chi[1]; cy++) {
            const int row = (cx * G.nc[1] + cy) * G.nc[2];
            const unsigned a0 = start[row + clo[2]], a1 = start[row + chi[2] + 1];
            for (unsigned base = a0; base < a1; base += ZN_THREADS) {
                if (staged + ZN_THREADS > ZN_CHUNK) {
                    any = true;
                    zone_min_chunk(s_at, staged, px, py, pz, D2);
                    __syncthreads();
                    if (threadIdx.x == 0) s_n = 0;
                    staged = 0;
                    __syncthreads();
                }
                const unsigned i = base + threadIdx.x;
                if (i < a1) {
                    const double x[3] = {sorted[3 * (size_t)i], sorted[3 * (size_t)i + 1], sorted[3 * (size_t)i + 2]};
                    if (zone_box_d2(x, bl, bh) <= G.R2) {
                        const int slot = atomicAdd(&s_n, 1);      // at most staged + ZN_THREADS <= ZN_CHUNK
                        s_at[3 * slot] = x[0]; s_at[3 * slot + 1] = x[1]; s_at[3 * slot + 2] = x[2];
                    }
                }
                __syncthreads();
                staged = s_n;
                __syncthreads();      // nobody adds to s_n before everybody has read it
            }
        }
    any = any || staged > 0;      // the same in every lane
    zone_min_chunk(s_at, staged, px, py, pz, D2);
    const size_t o = ((size_t)jx * G.n[1] + jy) * (size_t)G.n[2] + jz;
    const bool wide = nv == 4 && (o & 3) == 0;
    int n_in = 0, n_edge = 0;
    if (!any) {      // no atom within R of the brick: erase leaves it alone, keep stores zeros without loading
        if (!erase) {
            if (wide) *(float4 *)(g + o) = make_float4(0.f, 0.f, 0.f, 0.f);
            else
                for (int k = 0; k < nv; k++) g[o + k] = 0.f;
        }
    } else if (nv > 0) {
        double w[4];
        bool part = false, all0 = true, none1 = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double wk = 1.0;
            if (k < nv) {
                if (D2[k] <= G.r2) { wk = 1.0; n_in++; }
                else if (D2[k] >= G.R2) wk = 0.0;
                else { wk = 0.5 + 0.5 * cos(M_PI * ((sqrt(D2[k]) - G.radius) / G.soft)); n_edge++; }
                if (erase) wk = 1.0 - wk;
                part = part || (wk != 0.0 && wk != 1.0);
                all0 = all0 && wk == 0.0;
                none1 = none1 && wk != 1.0;
            }
            w[k] = wk;
        }
        if (wide && all0) *(float4 *)(g + o) = make_float4(0.f, 0.f, 0.f, 0.f);
        else if (wide && part) {
            const float4 q = *(const float4 *)(g + o);
            float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (w[k] != 1.0) v[k] = w[k] == 0.0 ? 0.f : (float)((double)v[k] * w[k]);
            if (none1) *(float4 *)(g + o) = make_float4(v[0], v[1], v[2], v[3]);
            else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (w[k] != 1.0) g[o + k] = v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < nv && w[k] != 1.0) g[o + k] = w[k] == 0.0 ? 0.f : (float)((double)g[o + k] * w[k]);
        }
    }
    n_in = wave_sum_i32(n_in);
    n_edge = wave_sum_i32(n_edge);
    if (lane_id() == 0) { s_cnt[threadIdx.x >> 6][0] = n_in; s_cnt[threadIdx.x >> 6][1] = n_edge; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int t = 0;
        for (int wv = 0; wv < ZN_THREADS / MAD_WAVE; wv++) t += s_cnt[wv][threadIdx.x];
        if (t) atomicAdd(counts + threadIdx.x, (unsigned long long)t);
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

extern "C" int mad_map_zone(mad_ctx *ctx, float *grid, const int32_t dims[3], const double origin[3], double voxsp, const double *atoms,
                            int64_t n_atoms, double radius, double soft, int erase, int64_t counts[2]) {
    const char *who = "mad_map_zone";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !origin) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (n_atoms < 0) return mad_fail(ctx, MAD_EINVAL, "%s: %lld atoms", who, (long long)n_atoms);
    if (n_atoms > 0 && !atoms) return mad_fail(ctx, MAD_EINVAL, "%s: NULL atoms", who);
    if (n_atoms >= (1ll << 31)) return mad_fail(ctx, MAD_EINVAL, "%s: %lld atoms: 2^31 or more are not supported", who, (long long)n_atoms);
    for (int k = 0; k < 3; k++)
        if (dims[k] < 1) return mad_fail(ctx, MAD_EINVAL, "%s: grid of %d x %d x %d voxels", who, dims[0], dims[1], dims[2]);
    if (!std::isfinite(voxsp) || !std::isfinite(radius) || !std::isfinite(soft) || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) ||
        !std::isfinite(origin[2]))
        return mad_fail(ctx, MAD_EINVAL, "%s: a number that is not finite", who);
    if (!(voxsp > 0)) return mad_fail(ctx, MAD_EINVAL, "%s: voxsp %g", who, voxsp);
    if (radius < 0 || soft < 0 || radius + soft == 0)
        return mad_fail(ctx, MAD_EINVAL, "%s: radius %g, soft %g (neither negative, not both 0)", who, radius, soft);
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 32) || vxy * (unsigned long long)dims[2] >= (1ull << 32))
        return mad_fail(ctx, MAD_EINVAL, "%s: %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
    const size_t n_vox = (size_t)(vxy * (unsigned long long)dims[2]);
    for (int64_t i = 0; i < 3 * n_atoms; i++)
        if (!std::isfinite(atoms[i])) return mad_fail(ctx, MAD_EINVAL, "%s: atom %lld has a coordinate that is not finite", who, (long long)(i / 3));

    ZoneGeo G;
    memset(&G, 0, sizeof(G));
    G.voxsp = voxsp; G.radius = radius; G.soft = soft;
    G.r2 = radius * radius; G.R = radius + soft; G.R2 = G.R * G.R;
    double ext = 0.0, scale = 0.0, ghi[3];
    for (int a = 0; a < 3; a++) {
        G.n[a] = dims[a]; G.o[a] = origin[a];
        G.lo[a] = origin[a] + voxsp * 0.0;
        G.hi[a] = origin[a] + voxsp * (double)(dims[a] - 1);
        G.glo[a] = G.lo[a] - G.R;
        ghi[a] = G.hi[a] + G.R;
        if (!std::isfinite(G.glo[a]) || !std::isfinite(ghi[a]) || !std::isfinite(ghi[a] - G.glo[a]))
            return mad_fail(ctx, MAD_EINVAL, "%s: the box grown by radius + soft is too large for float64", who);
        ext = std::max(ext, ghi[a] - G.glo[a]);
        scale = std::max(scale, std::max(fabs(G.glo[a]), fabs(ghi[a])));
    }
    // the cell edge: at least R; at least 1/64 of the longest side of the grown box (64^3 cells at most); and far above the
    // rounding of a coordinate (2^-40 of the largest one), which the spare cell on either side of a brick's range has to cover
    G.h = std::max(G.R, std::max(ext / (double)ZN_MAXC, scale * ldexp(1.0, -40)));
    int n_cells = 1;
    for (int a = 0; a < 3; a++) {
        const double c = ceil((ghi[a] - G.glo[a]) / G.h);
        G.nc[a] = c < 1.0 ? 1 : (c > (double)ZN_MAXC ? ZN_MAXC : (int)c);
        n_cells *= G.nc[a];
    }

    const unsigned bx = (unsigned)mad_ceil_div(dims[0], ZN_BX), by = (unsigned)mad_ceil_div(dims[1], ZN_BY), bz = (unsigned)mad_ceil_div(dims[2], ZN_BZ);
    const unsigned n_bricks = bx * by * bz, per_xcd = (n_bricks + 7) / 8;      // a brick holds a voxel: fewer than 2^32, in fact than 2^31
    const size_t bytes_tab = ((size_t)n_cells + 1) * 4, off_cnt = 64, off_start = off_cnt + ((bytes_tab + 63) & ~(size_t)63),
                 off_cursor = off_start + ((bytes_tab + 63) & ~(size_t)63);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n_vox + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), ((size_t)n_atoms + 1) * 24));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), ((size_t)n_atoms + 1) * 24));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), ((size_t)n_atoms + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), off_cursor + ((bytes_tab + 63) & ~(size_t)63)));
    float *d_g = scratch<float>(ctx, S_TMP_H);
    double *d_atoms = scratch<double>(ctx, S_TMP_A), *d_sorted = scratch<double>(ctx, S_TMP_B);
    int *d_cell_of = scratch<int>(ctx, S_TMP_C);
    char *blk = scratch<char>(ctx, S_TMP_G);
    unsigned long long *d_counts = (unsigned long long *)blk;
    unsigned *d_cnt = (unsigned *)(blk + off_cnt), *d_start = (unsigned *)(blk + off_start), *d_cursor = (unsigned *)(blk + off_cursor);
    MAD_HIP(hipMemcpyAsync(d_g, grid, n_vox * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemsetAsync(d_counts, 0, 16, ctx->stream));
    if (n_atoms > 0) {
        MAD_HIP(hipMemcpyAsync(d_atoms, atoms, (size_t)n_atoms * 24, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemsetAsync(d_cnt, 0, bytes_tab, ctx->stream));
        const unsigned blocks = (unsigned)mad_ceil_div(n_atoms, ZN_THREADS);
        hipLaunchKernelGGL(k_zone_count, dim3(blocks), dim3(ZN_THREADS), 0, ctx->stream, (const double *)d_atoms, (unsigned)n_atoms, G, d_cell_of, d_cnt);
        hipLaunchKernelGGL(k_zone_scan, dim3(1), dim3(ZN_SCAN_THREADS), 0, ctx->stream, (const unsigned *)d_cnt, n_cells, d_start, d_cursor);
        hipLaunchKernelGGL(k_zone_fill, dim3(blocks), dim3(ZN_THREADS), 0, ctx->stream, (const double *)d_atoms, (unsigned)n_atoms,
                           (const int *)d_cell_of, d_cursor, d_sorted);
    } else
        MAD_HIP(hipMemsetAsync(d_start, 0, bytes_tab, ctx->stream));      // every cell empty
    for (unsigned long long wg0 = 0; wg0 < (unsigned long long)per_xcd * 8; wg0 += ZN_ROUND) {
        const unsigned n_wg = (unsigned)std::min<unsigned long long>(ZN_ROUND, (unsigned long long)per_xcd * 8 - wg0);
        hipLaunchKernelGGL(k_map_zone, dim3(n_wg), dim3(ZN_THREADS), 0, ctx->stream, d_g, (const double *)d_sorted, (const unsigned *)d_start, d_counts,
                           G, erase ? 1 : 0, by, bz, n_bricks, per_xcd, (unsigned)wg0);
    }
    MAD_HIP(hipGetLastError());
    unsigned long long h_counts[2] = {0, 0};
    MAD_HIP(hipMemcpyAsync(grid, d_g, n_vox * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(h_counts, d_counts, 16, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (counts) { counts[0] = (int64_t)h_counts[0]; counts[1] = (int64_t)h_counts[1]; }
    return MAD_OK;
}
