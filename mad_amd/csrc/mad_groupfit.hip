// mad_groupfit.hip -- a placed model scored per group of atoms (residue, chain, ...) against a map: for every group the number of
// voxels of the map within a radius of the group's atoms and five sums of the map and of the model's density over them.  The
// contract is DESIGN.md section 4k: voxel j of grid 1 sits at p_a = origin1_a + voxsp * j_a, its squared distance to an atom is
// d2 = (dx*dx + dy*dy) + dz*dz (float64, no FMA: section 4i's expressions), it is a member of group g iff some atom of g has
// d2 <= radius * radius; a = g1[j] clamped at the isovalue, b = g2[j - s] clamped likewise or 0 outside grid 2, and the sums are
// {a*a, b*b, a*b, a, b} over the members.
//
//   gf_plan (mad_groupfit_plan.h)   on the host: the checks, the shift s, one work item per (group, brick of 8 x 8 x 16 voxels)
//   k_group_fit                     a workgroup per item: the group's atoms in reach of the brick staged through LDS, membership as a
//                                   flag per voxel, then the count and the five sums of the brick -> partial[item]
//   k_group_fold                    a workgroup per group: its partials added in a fixed order
//
// Determinism: membership is an OR over the atoms, so the order in which a workgroup stages them (integer LDS atomics hand out the
// slots) reaches no result.  A lane adds its voxels in voxel order, a wave adds its lanes and a workgroup its waves in fixed trees,
// k_group_fold gives thread t the partials first + t, first + t + 256, ... in this order and reduces by the same trees.  No
// floating-point atomics; nothing depends on what ran before.
#include <algorithm>
#include <new>

#include "mad_common.h"
#include "mad_groupfit_plan.h"

#define GF_THREADS 256
#define GF_CHUNK 1024           // atoms of one LDS chunk (24 KiB), as k_map_zone
#define GF_ROUND (1u << 22)     // workgroups of one launch: a grid may not have 2^32 threads
static_assert(GF_BX * GF_BY * (GF_BZ / 4) == GF_THREADS, "one lane per four z voxels of the brick");
static_assert(GF_CHUNK >= 2 * GF_THREADS, "a staging step adds up to GF_THREADS atoms to a chunk that is not full");

struct GroupGeo {
    int n1[3], n2[3];           // voxels of the two grids
    long long s[3];             // voxel j of grid 1 is voxel j - s of grid 2
    double o[3], voxsp;         // voxel j of grid 1, axis a, at o[a] + voxsp * j
    double r2;                  // radius * radius
    float iso;                  // (float)isovalue
};

// the n staged atoms against the lane's four voxels: bit k of m is set once voxel k is within reach of one (bits of voxels the lane
// does not have come in set).  A lane whose voxels are all members stops.
__device__ __forceinline__ unsigned gf_test_chunk(const double *s_at, int n, double px, double py, const double pz[4], double r2, unsigned m) {
    for (int a = 0; a < n && m != 15u; a++) {      // every lane reads the same address: a broadcast
        const double dx = px - s_at[3 * a], dy = py - s_at[3 * a + 1], az = s_at[3 * a + 2];
        const double t = dx * dx + dy * dy;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double dz = pz[k] - az, d2 = t + dz * dz;
            m |= (d2 <= r2 ? 1u : 0u) << k;
        }
    }
    return m;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, MAD_WAVE);
    return v;
}

// Workgroup wg0 + blockIdx.x takes one item: the brick of GF_BX x GF_BY x GF_BZ voxels of grid 1 that begins at the item's voxel
// (clipped to the grid), for the item's group.  It walks the group's atoms GF_THREADS at a time, keeps those with zone_box_d2(brick)
// <= r2 in the LDS chunk -- the monotone bound of mad_common.h: an atom it drops has d2 > r2 to every voxel of the brick -- and works
// a chunk off when the next step might not fit.  pn[item] = members, ps[item][5] = their sums.
__global__ __launch_bounds__(GF_THREADS) void k_group_fit(const float *__restrict__ g1, const float *__restrict__ g2, const double *__restrict__ atoms,
                                                          const long long *__restrict__ first_atom, const int4 *__restrict__ items,
                                                          unsigned *__restrict__ pn, double *__restrict__ ps, const GroupGeo G, unsigned n_items,
                                                          unsigned wg0) {
    __shared__ double s_at[GF_CHUNK * 3];
    __shared__ int s_n;
    __shared__ double s_red[GF_THREADS / MAD_WAVE][6];
    const unsigned item = wg0 + blockIdx.x;
    if (item >= n_items) return;      // the whole workgroup
    const int4 it = items[item];
    const unsigned a0 = (unsigned)first_atom[it.x], a1 = (unsigned)first_atom[it.x + 1];
    const int j0[3] = {it.y, it.z, it.w};
    const int jx = j0[0] + (int)(threadIdx.x >> 5), jy = j0[1] + (int)((threadIdx.x >> 2) & 7), jz = j0[2] + (int)(threadIdx.x & 3) * 4;
    const int nv = (jx < G.n1[0] && jy < G.n1[1] && jz < G.n1[2]) ? (G.n1[2] - jz < 4 ? G.n1[2] - jz : 4) : 0;
    const unsigned valid = (1u << nv) - 1u;
    const double px = G.o[0] + G.voxsp * (double)jx, py = G.o[1] + G.voxsp * (double)jy;
    double pz[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pz[k] = G.o[2] + G.voxsp * (double)(jz + k);
    const int bdim[3] = {GF_BX, GF_BY, GF_BZ};
    double bl[3], bh[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int last = j0[a] + bdim[a] - 1 < G.n1[a] - 1 ? j0[a] + bdim[a] - 1 : G.n1[a] - 1;
        bl[a] = G.o[a] + G.voxsp * (double)j0[a];
        bh[a] = G.o[a] + G.voxsp * (double)last;
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int staged = 0;
    unsigned m = 15u & ~valid;
    for (unsigned base = a0; base < a1; base += GF_THREADS) {
        if (staged + GF_THREADS > GF_CHUNK) {
            m = gf_test_chunk(s_at, staged, px, py, pz, G.r2, m);
            __syncthreads();
            if (threadIdx.x == 0) s_n = 0;
            staged = 0;
            __syncthreads();
        }
        const unsigned i = base + threadIdx.x;
        if (i < a1) {
            const double x[3] = {atoms[3 * (size_t)i], atoms[3 * (size_t)i + 1], atoms[3 * (size_t)i + 2]};
            if (zone_box_d2(x, bl, bh) <= G.r2) {
                const int slot = atomicAdd(&s_n, 1);      // at most staged + GF_THREADS <= GF_CHUNK
                s_at[3 * slot] = x[0]; s_at[3 * slot + 1] = x[1]; s_at[3 * slot + 2] = x[2];
            }
        }
        __syncthreads();
        staged = s_n;
        __syncthreads();      // nobody adds to s_n before everybody has read it
    }
    m = gf_test_chunk(s_at, staged, px, py, pz, G.r2, m) & valid;

    // the lane's members, in voxel order
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (m) {
        const size_t o = ((size_t)jx * G.n1[1] + jy) * (size_t)G.n1[2] + jz;
        float v1[4] = {0.f, 0.f, 0.f, 0.f};
        if (nv == 4 && (o & 3) == 0) {
            const float4 q = *(const float4 *)(g1 + o);
            v1[0] = q.x; v1[1] = q.y; v1[2] = q.z; v1[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((m >> k) & 1u) v1[k] = g1[o + k];
        }
        const long long kx = (long long)jx - G.s[0], ky = (long long)jy - G.s[1], kz0 = (long long)jz - G.s[2];
        const bool in_xy = kx >= 0 && kx < G.n2[0] && ky >= 0 && ky < G.n2[1];
        const size_t row2 = in_xy ? ((size_t)kx * G.n2[1] + (size_t)ky) * (size_t)G.n2[2] : 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if ((m >> k) & 1u) {
                const double a = v1[k] < G.iso ? 0.0 : (double)v1[k];
                const long long kz = kz0 + k;
                double b = 0.0;
                if (in_xy && kz >= 0 && kz < G.n2[2]) {
                    const float v2 = g2[row2 + (size_t)kz];
                    b = v2 < G.iso ? 0.0 : (double)v2;
                }
                s[0] += a * a; s[1] += b * b; s[2] += a * b; s[3] += a; s[4] += b;
            }
    }
    const int cnt = wave_sum_i32(__popc(m));
#pragma unroll
    for (int q = 0; q < 5; q++) s[q] = wave_sum_f64(s[q]);
    if (lane_id() == 0) {
        s_red[threadIdx.x >> 6][0] = (double)cnt;
#pragma unroll
        for (int q = 0; q < 5; q++) s_red[threadIdx.x >> 6][q + 1] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double t = s_red[0][threadIdx.x];
        for (int wv = 1; wv < GF_THREADS / MAD_WAVE; wv++) t += s_red[wv][threadIdx.x];
        if (threadIdx.x == 0) pn[item] = (unsigned)t;      // a count of at most 1 024: exact
        else ps[5 * (size_t)item + threadIdx.x - 1] = t;
    }
}

// Workgroup g0 + blockIdx.x adds the partials of one group: thread t those at first + t, first + t + GF_THREADS, ... in this order,
// then the lanes of a wave and the four waves in the trees of k_group_fit.  A group without items gets zeros.
__global__ __launch_bounds__(GF_THREADS) void k_group_fold(const unsigned *__restrict__ pn, const double *__restrict__ ps,
                                                           const unsigned *__restrict__ first_item, long long *__restrict__ n_vox,
                                                           double *__restrict__ sums, unsigned n_groups, unsigned g0) {
    __shared__ double s_red[GF_THREADS / MAD_WAVE][5];
    __shared__ unsigned long long s_cnt[GF_THREADS / MAD_WAVE];
    const unsigned g = g0 + blockIdx.x;
    if (g >= n_groups) return;      // the whole workgroup
    const unsigned i0 = first_item[g], i1 = first_item[g + 1];
    unsigned long long c = 0;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned i = i0 + threadIdx.x; i < i1; i += GF_THREADS) {      // (i1 < 2^31: no wrap)
        c += pn[i];
#pragma unroll
        for (int q = 0; q < 5; q++) s[q] += ps[5 * (size_t)i + q];
    }
    c = wave_sum_u64(c);
#pragma unroll
    for (int q = 0; q < 5; q++) s[q] = wave_sum_f64(s[q]);
    if (lane_id() == 0) {
        s_cnt[threadIdx.x >> 6] = c;
#pragma unroll
        for (int q = 0; q < 5; q++) s_red[threadIdx.x >> 6][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double t = s_red[0][threadIdx.x];
        for (int wv = 1; wv < GF_THREADS / MAD_WAVE; wv++) t += s_red[wv][threadIdx.x];
        sums[5 * (size_t)g + threadIdx.x] = t;
    } else if (threadIdx.x == 5) {
        unsigned long long t = 0;
        for (int wv = 0; wv < GF_THREADS / MAD_WAVE; wv++) t += s_cnt[wv];
        n_vox[g] = (long long)t;
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

extern "C" int mad_map_group_fit(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3], const float *grid2,
                                 const int32_t dims2[3], const double origin2[3], double voxsp, const double *atoms, const int64_t *first_atom,
                                 int32_t n_groups, double radius, double isovalue, int64_t *n_vox, double *sums) {
    const char *who = "mad_map_group_fit";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !grid2) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (n_groups > 0 && (!n_vox || !sums)) return mad_fail(ctx, MAD_EINVAL, "%s: NULL output", who);
    GfPlan P;
    char msg[256];
    try {
        if (!gf_plan(dims1, origin1, dims2, origin2, voxsp, atoms, first_atom, n_groups, radius, isovalue, P, msg, sizeof(msg)))
            return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    } catch (const std::bad_alloc &) {
        return mad_fail(ctx, MAD_ENOMEM, "%s: no host memory for the work list", who);
    }
    if (n_groups == 0) return MAD_OK;

    GroupGeo G;
    memset(&G, 0, sizeof(G));
    for (int a = 0; a < 3; a++) { G.n1[a] = dims1[a]; G.n2[a] = dims2[a]; G.s[a] = P.s[a]; G.o[a] = origin1[a]; }
    G.voxsp = voxsp; G.r2 = radius * radius; G.iso = (float)isovalue;
    const size_t nv1 = (size_t)dims1[0] * dims1[1] * dims1[2], nv2 = (size_t)dims2[0] * dims2[1] * dims2[2];
    const size_t n_atoms = (size_t)first_atom[n_groups], n_items = P.first_item[n_groups], ng = (size_t)n_groups;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (nv1 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (nv2 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (n_atoms + 1) * 24));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), (ng + 1) * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), (n_items + 1) * 16));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), (ng + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), (n_items + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), (n_items + 1) * 40));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), ng * 48));
    float *d_g1 = scratch<float>(ctx, S_TMP_H), *d_g2 = scratch<float>(ctx, S_TMP_I);
    double *d_atoms = scratch<double>(ctx, S_TMP_A), *d_ps = scratch<double>(ctx, S_TMP_F);
    long long *d_first_atom = scratch<long long>(ctx, S_TMP_B);
    int4 *d_items = scratch<int4>(ctx, S_TMP_C);
    unsigned *d_first_item = scratch<unsigned>(ctx, S_TMP_D), *d_pn = scratch<unsigned>(ctx, S_TMP_E);
    long long *d_nvox = scratch<long long>(ctx, S_TMP_G);
    double *d_sums = (double *)(d_nvox + ng);
    static_assert(sizeof(long long) == sizeof(int64_t), "first_atom and n_vox cross the bus as they are");
    MAD_HIP(hipMemcpyAsync(d_g1, grid1, nv1 * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_g2, grid2, nv2 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_atoms > 0) MAD_HIP(hipMemcpyAsync(d_atoms, atoms, n_atoms * 24, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_first_atom, first_atom, (ng + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_first_item, P.first_item.data(), (ng + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_items > 0) MAD_HIP(hipMemcpyAsync(d_items, P.items.data(), n_items * 16, hipMemcpyHostToDevice, ctx->stream));
    for (size_t wg0 = 0; wg0 < n_items; wg0 += GF_ROUND) {
        const unsigned n_wg = (unsigned)std::min<size_t>(GF_ROUND, n_items - wg0);
        hipLaunchKernelGGL(k_group_fit, dim3(n_wg), dim3(GF_THREADS), 0, ctx->stream, (const float *)d_g1, (const float *)d_g2, (const double *)d_atoms,
                           (const long long *)d_first_atom, (const int4 *)d_items, d_pn, d_ps, G, (unsigned)n_items, (unsigned)wg0);
    }
    for (size_t g0 = 0; g0 < ng; g0 += GF_ROUND) {
        const unsigned n_wg = (unsigned)std::min<size_t>(GF_ROUND, ng - g0);
        hipLaunchKernelGGL(k_group_fold, dim3(n_wg), dim3(GF_THREADS), 0, ctx->stream, (const unsigned *)d_pn, (const double *)d_ps,
                           (const unsigned *)d_first_item, d_nvox, d_sums, (unsigned)n_groups, (unsigned)g0);
    }
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(n_vox, d_nvox, ng * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(sums, d_sums, ng * 40, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}
