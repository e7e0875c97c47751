// mad_envelope.hip -- a soft mask made from a map itself: threshold, grow by `extend`, raised-cosine edge of `soft`.  The contract is
// DESIGN.md section 4r (mad_amd/envelope.py::envelope_numpy restates it): a voxel is a seed where (double)g > threshold; d2 is the
// exact squared distance in whole voxels to the nearest seed wherever that is at most Rv^2, the sentinel INT32_MAX elsewhere; the
// weight follows mad_map_zone's expressions on D2 = d2 * voxsp^2.
//
//   k_env_z        min-plus along z, the contiguous axis, straight from the float32 map: a wavefront per 64 outputs of a line, the
//                  line's window staged in LDS as 0 (seed) / sentinel
//   k_env_axis     min-plus along y or x: a thread per voxel in flat order, so z (and then y) runs across the lanes and every tap is
//                  one coalesced load; the window is walked outward and left once j * j reaches the lane's running minimum
//   k_env_weight   d2 -> sentinel beyond Rv^2, the weight, and three tallies as per-workgroup partials
//   k_env_counts   the partials added in a fixed order
//
// out[i] = min over |j - i| <= Rv of in[j] + (i - j)^2 over int32 is separable and exact: after the three passes a voxel holds the
// minimum of dx^2 + dy^2 + dz^2 over the seeds with |dx|, |dy|, |dz| <= Rv.  A seed at d2 <= Rv^2 is inside that cube, so every
// value <= Rv^2 is the true minimum; larger values may miss a nearer seed outside the cube and become the sentinel.
//
// Determinism: integers throughout the distance (a minimum does not depend on the order of its terms), integer tallies; the weight
// is a function of one voxel's d2.  No floating-point atomics.
#include <algorithm>

#include "mad_common.h"
#include "mad_envelope_plan.h"

static_assert(ENV_THREADS == ENV_WAVES * MAD_WAVE && ENV_SEG == MAD_WAVE, "a wavefront per unit of the pass along z");

// Unit u = blockIdx.x * ENV_WAVES + wave (mad_envelope_plan.h).  *bad is raised for a voxel that is not finite.
__global__ __launch_bounds__(ENV_THREADS) void k_env_z(const float *__restrict__ g, int nz, unsigned segs, unsigned long long units, int Rv,
                                                       double thr, unsigned *__restrict__ out, int *__restrict__ bad) {
    __shared__ unsigned s_win[ENV_WAVES][ENV_ZW];
    const int lane = (int)lane_id(), wv = (int)(threadIdx.x >> 6);
    const unsigned long long u = (unsigned long long)blockIdx.x * ENV_WAVES + (unsigned)wv;
    const bool live = u < units;
    const unsigned line = live ? (unsigned)(u / segs) : 0u, seg = live ? (unsigned)(u % segs) : 0u;
    const int z0 = (int)seg * ENV_SEG, len = env_win_len(Rv);
    const size_t base = (size_t)line * (size_t)nz;
    unsigned *win = s_win[wv];
    if (live) {
        bool any_bad = false;
        for (int k = lane; k < len; k += MAD_WAVE) {
            const long long z = (long long)z0 - Rv + k;      // (z0 + Rv + 63 may pass 2^31)
            unsigned v = ENV_SENT;
            if (z >= 0 && z < nz) {
                const float f = g[base + (size_t)z];
                if (!(fabsf(f) <= 3.4028234663852886e38f)) any_bad = true;
                if ((double)f > thr) v = 0u;
            }
            win[k] = v;
        }
        if (any_bad) atomicOr(bad, 1);
    }
    __syncthreads();
    if (live && z0 + lane < nz) out[base + (size_t)(z0 + lane)] = env_walk(win, env_win_centre(lane, Rv), Rv);
}

// Thread i = voxel i in flat order; the axis has n entries `stride` apart, this voxel is entry (i / stride) % n.
__global__ __launch_bounds__(ENV_THREADS) void k_env_axis(const unsigned *__restrict__ in, unsigned n_vox, unsigned stride, int n, int Rv,
                                                          unsigned *__restrict__ out) {
    const unsigned i = blockIdx.x * ENV_THREADS + threadIdx.x;
    if (i >= n_vox) return;
    const int p = (int)((i / stride) % (unsigned)n);
    unsigned m = env_step(ENV_SENT, in[i], 0u);
    const int lo = p < Rv ? p : Rv, hi = n - 1 - p < Rv ? n - 1 - p : Rv, far = lo > hi ? lo : hi;
    unsigned off = 0;      // j * stride: both taps lie inside the grid where they are read, so it stays below n_vox
    for (int j = 1; j <= far; j++) {
        const unsigned t = (unsigned)(j * j);
        if (t >= m) break;
        off += stride;
        if (j <= lo) m = env_step(m, in[i - off], t);
        if (j <= hi) m = env_step(m, in[i + off], t);
    }
    out[i] = m;
}

struct EnvWeight {
    unsigned n_vox, Rv2;
    double vv, extend, soft, r2, R2;
};

// part [workgroup][3] = seeds, core (D2 <= r2), edge (r2 < D2 < R2): the branch taken, as mad_map_zone counts
__global__ __launch_bounds__(ENV_THREADS) void k_env_weight(const unsigned *__restrict__ d2raw, const EnvWeight W, float *__restrict__ mask,
                                                            int *__restrict__ d2, unsigned long long *__restrict__ part) {
    __shared__ int s_cnt[ENV_WAVES][3];
    int n_seed = 0, n_core = 0, n_edge = 0;      // a thread sees at most 2^31 / (ENV_WGS * ENV_THREADS) voxels
    for (unsigned i = blockIdx.x * ENV_THREADS + threadIdx.x; i < W.n_vox; i += ENV_WGS * ENV_THREADS) {
        unsigned v = d2raw[i];
        if (v > W.Rv2) v = ENV_SENT;
        double w = 0.0;
        if (v != ENV_SENT) {
            const double D2 = (double)v * W.vv;
            if (D2 <= W.r2) { w = 1.0; n_core++; }
            else if (D2 >= W.R2) w = 0.0;
            else { w = 0.5 + 0.5 * cos(M_PI * ((sqrt(D2) - W.extend) / W.soft)); n_edge++; }
            if (v == 0u) n_seed++;
        }
        mask[i] = (float)w;
        d2[i] = (int)v;
    }
    n_seed = wave_sum_i32(n_seed);
    n_core = wave_sum_i32(n_core);
    n_edge = wave_sum_i32(n_edge);
    if (lane_id() == 0) { s_cnt[threadIdx.x >> 6][0] = n_seed; s_cnt[threadIdx.x >> 6][1] = n_core; s_cnt[threadIdx.x >> 6][2] = n_edge; }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long t = 0;
        for (int wv = 0; wv < ENV_WAVES; wv++) t += s_cnt[wv][threadIdx.x];
        part[(size_t)blockIdx.x * 3 + threadIdx.x] = (unsigned long long)t;
    }
}

// One workgroup: thread q < 3 adds the ENV_WGS partials of tally q in ascending order.
__global__ __launch_bounds__(MAD_WAVE) void k_env_counts(const unsigned long long *__restrict__ part, unsigned long long *__restrict__ out) {
    if (threadIdx.x >= 3) return;
    unsigned long long t = 0;
    for (int p = 0; p < ENV_WGS; p++) t += part[(size_t)p * 3 + threadIdx.x];
    out[threadIdx.x] = t;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

extern "C" int mad_map_envelope(mad_ctx *ctx, const float *grid, const int32_t dims[3], double voxsp, double threshold, double extend,
                                double soft, float *mask_out, int32_t *d2_out, int64_t counts[3]) {
    const char *who = "mad_map_envelope";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !mask_out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    EnvPlan P;
    char msg[320];
    const int rc = env_plan(dims, voxsp, threshold, extend, soft, P, msg, sizeof(msg));
    if (rc != ENV_OK) return mad_fail(ctx, rc == ENV_EDOM ? MAD_EDOM : MAD_EINVAL, "%s", msg);
    const size_t n_vox = P.n_vox;
    const unsigned sy = (unsigned)dims[2], sx = (unsigned)dims[1] * (unsigned)dims[2];      // < 2^31: the grid has fewer voxels

    const size_t off_part = 64, off_cnt = off_part + (size_t)ENV_WGS * 3 * 8;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n_vox + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), (n_vox + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), (n_vox + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), off_cnt + 64));
    float *d_g = scratch<float>(ctx, S_TMP_H);
    unsigned *d_a = scratch<unsigned>(ctx, S_TMP_C), *d_b = scratch<unsigned>(ctx, S_TMP_D);
    char *blk = scratch<char>(ctx, S_TMP_G);
    int *d_bad = (int *)blk;
    unsigned long long *d_part = (unsigned long long *)(blk + off_part), *d_cnt = (unsigned long long *)(blk + off_cnt);
    MAD_HIP(hipMemcpyAsync(d_g, grid, n_vox * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemsetAsync(d_bad, 0, 64, ctx->stream));
    // z: map -> a;  y: a -> b;  x: b -> a;  weight: a -> the mask (over the map's copy) and d2 (over b).  An axis of one entry has no
    // taps, but its pass still runs: the buffers alternate the same way for every shape.
    mad_timer_begin(ctx, MAD_T_ENV_Z);
    hipLaunchKernelGGL(k_env_z, dim3(P.wgs_z), dim3(ENV_THREADS), 0, ctx->stream, (const float *)d_g, dims[2], P.segs, P.units, P.Rv, threshold,
                       d_a, d_bad);
    mad_timer_end(ctx, MAD_T_ENV_Z);
    mad_timer_begin(ctx, MAD_T_ENV_Y);
    hipLaunchKernelGGL(k_env_axis, dim3(P.wgs_flat), dim3(ENV_THREADS), 0, ctx->stream, (const unsigned *)d_a, P.n_vox, sy, dims[1], P.Rv, d_b);
    mad_timer_end(ctx, MAD_T_ENV_Y);
    mad_timer_begin(ctx, MAD_T_ENV_X);
    hipLaunchKernelGGL(k_env_axis, dim3(P.wgs_flat), dim3(ENV_THREADS), 0, ctx->stream, (const unsigned *)d_b, P.n_vox, sx, dims[0], P.Rv, d_a);
    mad_timer_end(ctx, MAD_T_ENV_X);
    EnvWeight W;
    W.n_vox = P.n_vox; W.Rv2 = P.Rv2; W.vv = P.vv; W.extend = P.extend; W.soft = P.soft; W.r2 = P.r2; W.R2 = P.R2;
    mad_timer_begin(ctx, MAD_T_ENV_WEIGHT);
    hipLaunchKernelGGL(k_env_weight, dim3(ENV_WGS), dim3(ENV_THREADS), 0, ctx->stream, (const unsigned *)d_a, W, d_g, (int *)d_b, d_part);
    hipLaunchKernelGGL(k_env_counts, dim3(1), dim3(MAD_WAVE), 0, ctx->stream, (const unsigned long long *)d_part, d_cnt);
    mad_timer_end(ctx, MAD_T_ENV_WEIGHT);
    MAD_HIP(hipGetLastError());
    int h_bad = 0;
    unsigned long long h_cnt[3] = {0, 0, 0};
    MAD_HIP(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(h_cnt, d_cnt, 24, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (h_bad) return mad_fail(ctx, MAD_EDOM, "%s: the map holds a voxel that is not finite", who);      // nothing has been written
    MAD_HIP(hipMemcpyAsync(mask_out, d_g, n_vox * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (d2_out) MAD_HIP(hipMemcpyAsync(d2_out, d_b, n_vox * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (counts) { counts[0] = (int64_t)h_cnt[0]; counts[1] = (int64_t)h_cnt[1]; counts[2] = (int64_t)h_cnt[2]; }
    return MAD_OK;
}
