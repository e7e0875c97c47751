// mad_symmetry.hip -- the self-correlation of a map under a batch of rigid motions: for every operator g the
// sums (n, sum a, sum b, sum a^2, sum b^2, sum a b) over the lattice points j of a ball, a = grid[j] and b = the float32 that
// mad_map_resample(order 1, R_g, T_g, onto the map's own lattice) writes at j.  The value b comes from mad_resample_taps.h, the code
// mad_map_resample itself runs; the sums are paired as fourier.tree_sum pairs them (runs of 256 by halving, level after level).
//
//   k_sym_score   workgroup (run, batch): the run's 256 points once, then SYM_OPS_WG operators over them; one record per operator
//   k_sym_level   one level of the tree over every slot of a chunk
//
// Determinism: no atomics; the pairing is fixed by the box alone, not by the launch, the chunking or the operators per workgroup.
#include <vector>

#include "mad_common.h"
#include "mad_resample_taps.h"
#include "mad_symmetry_plan.h"

static_assert(SYM_RUN == 256, "the halving below is written for four waves of 64");

// v[0 .. 2] of the 256 threads -> their three sums in tree_sum's pairing, valid in thread 0.  s: [SYM_REC][SYM_RUN] of LDS that no
// thread still reads.  One barrier: the steps 128 and 64 read LDS, the steps 32 .. 1 stay inside wave 0.
__device__ __forceinline__ void sym_run_sum(double (*s)[SYM_RUN], unsigned t, double v[SYM_REC]) {
#pragma unroll
    for (int k = 0; k < SYM_REC; k++) s[k][t] = v[k];
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int k = 0; k < SYM_REC; k++) {
            double x = (s[k][t] + s[k][t + 128]) + (s[k][t + 64] + s[k][t + 192]);
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) x = x + __shfl_down(x, h, 64);
            v[k] = x;
        }
    }
}

// ops[g] = A[9], b[3] of operator g of the chunk (u = b + A j, folded on the host as mad_map_resample folds it).  part: slot g of
// n_slots holds n_runs records; slot n_ops (the last) takes the points' own sums (n, sum a, sum a^2), written by batch 0.
__global__ __launch_bounds__(SYM_RUN) void k_sym_score(const float *__restrict__ grid, const SymBox B, const double *__restrict__ ops, int n_ops,
                                                       double *__restrict__ part) {
    __shared__ double s[2][SYM_REC][SYM_RUN];
    const unsigned t = threadIdx.x, run = blockIdx.x;
    const uint64_t i = (uint64_t)run * SYM_RUN + t;
    int32_t j[3] = {0, 0, 0};
    const bool counts = i < B.n_box && sym_point(B, i, j);
    const double a = counts ? (double)grid[((size_t)j[0] * (size_t)B.n[1] + (size_t)j[1]) * (size_t)B.n[2] + (size_t)j[2]] : 0.0;
    double v[SYM_REC];
    if (blockIdx.y == 0) {      // uniform over the workgroup
        v[0] = counts ? 1.0 : 0.0; v[1] = a; v[2] = a * a;
        sym_run_sum(s[1], t, v);
        if (t == 0) {
            double *rec = part + ((size_t)n_ops * B.n_runs + run) * SYM_REC;
            rec[0] = v[0]; rec[1] = v[1]; rec[2] = v[2];
        }
    }
    RsGeo G;
    G.n[0] = G.m[0] = B.n[0]; G.n[1] = G.m[1] = B.n[1]; G.n[2] = G.m[2] = B.n[2];
    const int g0 = (int)blockIdx.y * SYM_OPS_WG;
    for (int k = 0; k < SYM_OPS_WG && g0 + k < n_ops; k++) {
        const double *q = ops + (size_t)12 * (g0 + k);
#pragma unroll
        for (int e = 0; e < 9; e++) G.A[e] = q[e];
#pragma unroll
        for (int e = 0; e < 3; e++) G.b[e] = q[9 + e];
        const double b = counts ? (double)rs_sample<1, float>(grid, G, j[0], j[1], j[2]) : 0.0;
        v[0] = b; v[1] = b * b; v[2] = a * b;      // 24 x 24 bits: exact
        // the buffers alternate: wave 0 may still read the other one, and it has left this one before the barrier in between
        sym_run_sum(s[k & 1], t, v);
        if (t == 0) {
            double *rec = part + ((size_t)(g0 + k) * B.n_runs + run) * SYM_REC;
            rec[0] = v[0]; rec[1] = v[1]; rec[2] = v[2];
        }
    }
}

// One level of tree_sum over every slot: out[slot][b] = the sums of run b of in[slot][0 .. n_in - 1] (the last run zero-padded),
// m = ceil(n_in / 256) records per slot.
__global__ __launch_bounds__(SYM_RUN) void k_sym_level(const double *__restrict__ in, unsigned n_in, unsigned m, double *__restrict__ out) {
    __shared__ double s[SYM_REC][SYM_RUN];
    const unsigned t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * SYM_RUN + t;
    const double *rec = in + ((size_t)blockIdx.y * n_in + i) * SYM_REC;
    double v[SYM_REC];
    const bool has = i < n_in;
#pragma unroll
    for (int k = 0; k < SYM_REC; k++) v[k] = has ? rec[k] : 0.0;
    sym_run_sum(s, t, v);
    if (t == 0) {
        double *o = out + ((size_t)blockIdx.y * m + blockIdx.x) * SYM_REC;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

extern "C" int mad_map_symmetry_score(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp,
                                      const double ball_centre[3], double radius, int32_t stride, int32_t n_ops, const double *R9, const double *T3,
                                      double *out) {
    const char *who = "mad_map_symmetry_score";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !origin || !ball_centre || !R9 || !T3 || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    SymPlan P;
    char msg[256];
    if (!sym_plan(dims, origin, voxsp, ball_centre, radius, stride, n_ops, ctx->sym_scratch, P, msg, sizeof(msg))) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    if (!rs_finite(R9, 9 * n_ops) || !rs_finite(T3, 3 * n_ops)) return mad_fail(ctx, MAD_EINVAL, "%s: a number that is not finite", who);
    std::vector<double> ops((size_t)12 * n_ops);
    for (int g = 0; g < n_ops; g++) {
        double dev = 0.0, det = 0.0;
        if (!rs_rotation_ok(R9 + (size_t)9 * g, &dev, &det))
            return mad_fail(ctx, MAD_EINVAL, "%s: R of operator %d is no rotation (max|R R^T - I| = %g, det %g)", who, g, dev, det);
        rs_fold(R9 + (size_t)9 * g, T3 + (size_t)3 * g, origin, voxsp, origin, voxsp, &ops[(size_t)12 * g], &ops[(size_t)12 * g + 9]);
        if (!rs_finite(&ops[(size_t)12 * g], 12)) return mad_fail(ctx, MAD_EINVAL, "%s: operator %d moves the map too far for float64", who, g);
    }
    ctx->last_sym_chunks = P.n_chunks;
    ctx->last_sym_scratch = (int64_t)P.scratch_bytes;
    const SymBox &B = P.box;
    if (B.n_box == 0) {      // an empty box: n = 0 and zero sums, nothing launched
        for (size_t k = 0; k < (size_t)6 * n_ops; k++) out[k] = 0.0;
        return MAD_OK;
    }
    const size_t n_src = (size_t)dims[0] * dims[1] * dims[2];
    const size_t slots = (size_t)P.ops_chunk + 1, b_a = slots * P.rec_a * SYM_REC * sizeof(double), b_b = slots * P.rec_b * SYM_REC * sizeof(double);
    const size_t b_ops = (size_t)P.ops_chunk * 12 * sizeof(double);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n_src + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), b_a + 64));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), b_b + 64));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), b_ops + 64));
    float *d_src = scratch<float>(ctx, S_TMP_H);
    double *buf[2] = {scratch<double>(ctx, S_TMP_A), scratch<double>(ctx, S_TMP_B)}, *d_ops = scratch<double>(ctx, S_TMP_G);
    std::vector<double> rec(slots * SYM_REC);
    MAD_HIP(hipMemcpyAsync(d_src, grid, n_src * 4, hipMemcpyHostToDevice, ctx->stream));
    for (int c = 0; c < P.n_chunks; c++) {
        const int g0 = c * P.ops_chunk, n = std::min(P.ops_chunk, n_ops - g0);
        MAD_HIP(hipMemcpyAsync(d_ops, &ops[(size_t)12 * g0], (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        mad_timer_begin(ctx, MAD_T_SYM_SCORE);      // one interval around a chunk: every operator of it is in the one grid
        hipLaunchKernelGGL(k_sym_score, dim3(B.n_runs, (unsigned)mad_ceil_div(n, SYM_OPS_WG)), dim3(SYM_RUN), 0, ctx->stream, (const float *)d_src, B,
                           (const double *)d_ops, n, buf[0]);
        int cur = 0;
        for (int l = 0; l < P.n_levels; l++, cur ^= 1)
            hipLaunchKernelGGL(k_sym_level, dim3(P.level_n[l + 1], (unsigned)(n + 1)), dim3(SYM_RUN), 0, ctx->stream, (const double *)buf[cur], P.level_n[l],
                               P.level_n[l + 1], buf[cur ^ 1]);
        mad_timer_end(ctx, MAD_T_SYM_SCORE);
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(rec.data(), buf[cur], (size_t)(n + 1) * SYM_REC * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));      // per chunk, never per operator: the next chunk reuses d_ops and the buffers
        const double *pts = &rec[(size_t)n * SYM_REC];
        for (int g = 0; g < n; g++) {
            double *o = out + (size_t)6 * (g0 + g);
            const double *r = &rec[(size_t)g * SYM_REC];
            o[0] = pts[0]; o[1] = pts[1]; o[2] = r[0]; o[3] = pts[2]; o[4] = r[1]; o[5] = r[2];
        }
    }
    return MAD_OK;
}

extern "C" int mad_last_symmetry_plan(mad_ctx *ctx, int32_t *ops_per_workgroup, int32_t *n_chunks, int64_t *scratch_bytes) {
    if (!ctx) return MAD_EINVAL;
    if (ops_per_workgroup) *ops_per_workgroup = SYM_OPS_WG;
    if (n_chunks) *n_chunks = ctx->last_sym_chunks;
    if (scratch_bytes) *scratch_bytes = ctx->last_sym_scratch;
    return MAD_OK;
}
