// Pose filter (MaD._filter_dsc_pairs, reference MaD.py:456-553): the greedy clustering of the k best poses by the RMSD of the
// moved anchor cloud, decided on the device wherever the float64 result is certain.
//
//   k_pose_d2      d2(i, j) = sum((cloud(j) - cloud(i))**2) / N for every j < i, cloud(s) = (hi - s.hi_coord) @ R(s).T + s.lo_coord:
//                  the packed lower triangle, all matches of a launch in one grid.  One wave per (i, 4 consecutive j): the lanes
//                  stride over the N cloud points, pose i's cloud point is formed once and used against the four j.  The grid is
//                  the triangle: row i has ceil(i / 16) workgroups.
//   k_pose_greedy  one wave per match walks rows 1..n-1 against the current leaders and writes owner / d2min per row; it stops at
//                  the first row whose decision lies inside the guard band (the caller then runs the host function for that match).
//
// float64, no fused multiply-add (the Makefile's -ffp-contract=off), no atomics: every sum is a fixed tree, two calls give the
// same bits.  tools/check_filter_tier.py is the numpy model of both kernels and of the band.
#include "mad_common.h"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

// The band.  u = 2^-53.  A cloud coordinate passes through at most MAD_FILT_POS_C roundings, on the device
// and in numpy (BLAS, fused or not); a d2 through 3N - 1 additions in any order plus MAD_FILT_SUM_C more (squares, differences,
// the division, the square root of the reference, the squared threshold).
#define MAD_FILT_U 1.1102230246251565e-16
#define MAD_FILT_POS_C 6.0
#define MAD_FILT_SUM_C 12.0
#define MAD_FILT_SQRT3 1.7320508075688772      // a point's error vector against the bound of its components
#define MAD_FILT_SAFETY 4.0
#define MAD_FILT_JT 4            // columns j per wave
#define MAD_FILT_WAVES 4         // waves per workgroup of k_pose_d2
#define MAD_FILT_COLS (MAD_FILT_JT * MAD_FILT_WAVES)      // columns j per workgroup
#define MAD_FILT_BATCH 16        // matches per launch, at most
#define MAD_FILT_D2_BYTES ((size_t)256 << 20)      // ... and d2 triangles per launch (one match may exceed it alone: 64 MiB at 4 096 rows does not)

enum { ROW_HI = 8, ROW_LO = 11, ROW_R = 14, ROW_LEN = 23 };

struct FiltJob {
    const double *rows;          // [n][23]
    const double *cx, *cy, *cz;  // the hi cloud, one array per axis
    double *d2;                  // packed lower triangle: d2(i, j) at i (i - 1) / 2 + j, j < i
    int32_t *owner;              // [n]
    double *d2min;               // [n]
    int32_t *meta;               // n_done, status
    int n, N;
    double c_sum, delta;         // band(d) = 2 SAFETY (c_sum d + 2 sqrt(d) delta + delta^2)
};
struct FiltBatch {
    int n_jobs;
    long long first[MAD_FILT_BATCH + 1];
    FiltJob job[MAD_FILT_BATCH];
};

struct Pose {
    double a[3], b[3], R[9];
};
__device__ __forceinline__ Pose load_pose(const double *__restrict__ row) {
    Pose P;
    for (int k = 0; k < 3; k++) P.a[k] = row[ROW_HI + k];
    for (int k = 0; k < 3; k++) P.b[k] = row[ROW_LO + k];
    for (int k = 0; k < 9; k++) P.R[k] = row[ROW_R + k];
    return P;
}
// one point of np.dot(hi - a, R.T) + b, rounded product by product
__device__ __forceinline__ void move_point(const Pose &P, double hx, double hy, double hz, double &x, double &y, double &z) {
    const double u0 = hx - P.a[0], u1 = hy - P.a[1], u2 = hz - P.a[2];
    x = ((P.R[0] * u0 + P.R[1] * u1) + P.R[2] * u2) + P.b[0];
    y = ((P.R[3] * u0 + P.R[4] * u1) + P.R[5] * u2) + P.b[1];
    z = ((P.R[6] * u0 + P.R[7] * u1) + P.R[8] * u2) + P.b[2];
}

// workgroups of k_pose_d2 before row group g, and for a match of n rows
__host__ __device__ static inline long long d2_blocks_before(long long g) { return MAD_FILT_COLS / 2 * g * (g + 1); }
static inline long long d2_blocks(long long n) {
    if (n < 2) return 0;
    const long long g = (n - 1) / MAD_FILT_COLS, rem = (n - 1) % MAD_FILT_COLS;
    return d2_blocks_before(g) + rem * (g + 1);
}

__global__ __launch_bounds__(64 * MAD_FILT_WAVES) void k_pose_d2(const FiltBatch B) {
    int jb = 0;
    while (jb + 1 < B.n_jobs && (long long)blockIdx.x >= B.first[jb + 1]) jb++;
    const FiltJob &J = B.job[jb];
    const long long blk = (long long)blockIdx.x - B.first[jb];
    // rows i = C g + 1 .. C g + C (C = MAD_FILT_COLS) have g + 1 workgroups each; C g (g + 1) / 2 workgroups lie before group g
    int g = (int)((sqrt(1.0 + 8.0 * (double)blk / MAD_FILT_COLS) - 1.0) * 0.5);
    while (d2_blocks_before(g + 1) <= blk) g++;
    while (d2_blocks_before(g) > blk) g--;
    const int r = (int)(blk - d2_blocks_before(g));
    const int i = MAD_FILT_COLS * g + 1 + r / (g + 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j0 = (r % (g + 1)) * MAD_FILT_COLS + wave * MAD_FILT_JT;
    if (i >= J.n || j0 >= i) return;      // (the last workgroup of a row may have waves beyond j = i - 1)
    const Pose Pi = load_pose(J.rows + (size_t)i * ROW_LEN);
    Pose Pj[MAD_FILT_JT];
#pragma unroll
    for (int t = 0; t < MAD_FILT_JT; t++) Pj[t] = load_pose(J.rows + (size_t)min(j0 + t, i - 1) * ROW_LEN);
    double acc[MAD_FILT_JT] = {};
    for (int p = lane; p < J.N; p += 64) {
        const double hx = J.cx[p], hy = J.cy[p], hz = J.cz[p];
        double xi, yi, zi;
        move_point(Pi, hx, hy, hz, xi, yi, zi);
#pragma unroll
        for (int t = 0; t < MAD_FILT_JT; t++) {
            double x, y, z;
            move_point(Pj[t], hx, hy, hz, x, y, z);
            const double ex = x - xi, ey = y - yi, ez = z - zi;
            acc[t] += (ex * ex + ey * ey) + ez * ez;
        }
    }
#pragma unroll
    for (int t = 0; t < MAD_FILT_JT; t++) {
        double v = acc[t];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0 && j0 + t < i) J.d2[(size_t)i * (i - 1) / 2 + j0 + t] = v / (double)J.N;
    }
}

__device__ __forceinline__ double filt_band(double d, double c_sum, double delta) {
    return 2.0 * MAD_FILT_SAFETY * ((c_sum * d + 2.0 * sqrt(d) * delta) + delta * delta);
}

__global__ __launch_bounds__(64) void k_pose_greedy(const FiltBatch B, double t2) {
    __shared__ int32_t leader[MAD_POSE_CLUSTER_MAX_N];
    const FiltJob &J = B.job[blockIdx.x];
    const int lane = threadIdx.x, n = J.n;
    if (n == 0) {
        if (lane == 0) J.meta[0] = 0, J.meta[1] = 0;
        return;
    }
    if (lane == 0) leader[0] = 0, J.owner[0] = 0, J.d2min[0] = 0.0;
    __syncthreads();
    int nl = 1, i = 1, status = 0;
    double stop_d2 = NAN;
    for (; i < n; i++) {
        const double *__restrict__ row = J.d2 + (size_t)i * (i - 1) / 2;
        double m1 = INFINITY, m2 = INFINITY;
        int i1 = 0x7fffffff;
        bool bad = J.N == 0;      // the reference divides by zero: left to it
        if (!bad)
            for (int c = lane; c < nl; c += 64) {      // c ascends within a lane: an equal value never displaces an earlier leader
                const double d = row[leader[c]];
                bad |= !(d <= DBL_MAX);
                if (d < m1) m2 = m1, m1 = d, i1 = c;
                else if (d < m2) m2 = d;
            }
        for (int o = 32; o > 0; o >>= 1) {      // smallest (lowest leader index on equal values) and second smallest of the wave
            const double o1 = __shfl_xor(m1, o, 64), o2 = __shfl_xor(m2, o, 64);
            const int oi = __shfl_xor(i1, o, 64);
            if (o1 < m1 || (o1 == m1 && oi < i1)) m2 = fmin(m1, o2), m1 = o1, i1 = oi;
            else m2 = fmin(m2, o1);
        }
        const bool anybad = __any(bad);
        const bool lead = m1 - t2 > filt_band(m1, J.c_sum, J.delta);
        const bool join = t2 - m1 > filt_band(t2, J.c_sum, J.delta) && (m2 > DBL_MAX || m2 - m1 > filt_band(m2, J.c_sum, J.delta));
        if (anybad || !(lead || join)) {
            status = 1;
            stop_d2 = anybad ? NAN : m1;
            break;
        }
        if (lane == 0) {
            J.owner[i] = lead ? i : leader[i1];
            J.d2min[i] = m1;
            if (lead) leader[nl] = i;
        }
        nl += lead;
        __syncthreads();
    }
    for (int r = i + lane; r < n; r += 64) J.owner[r] = -1, J.d2min[r] = r == i ? stop_d2 : NAN;
    if (lane == 0) J.meta[0] = i, J.meta[1] = status;
}

static inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

static inline size_t d2_bytes(size_t n) { return up16(n * (n ? n - 1 : 0) / 2 * 8); }

// One launch of each kernel for up to MAD_FILT_BATCH matches of the call.
static int cluster_chunk(mad_ctx *ctx, int nm, const double *const *rows, const int32_t *n_rows, const double *const *cloud,
                         const int32_t *n_cloud, double rmsd_thresh, int32_t *const *owner_out, double *const *d2min_out,
                         int32_t *n_done_out, int32_t *status_out) {
    size_t b_in = 0, b_d2 = 0, b_out = 0;
    for (int m = 0; m < nm; m++) {
        const size_t n = n_rows[m], N = n_cloud[m];
        b_in += up16(n * ROW_LEN * 8) + 3 * up16(N * 8);
        b_d2 += d2_bytes(n);
        b_out += up16(n * 8) + up16(n * 4) + 16;
    }
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_FILT_IN), b_in + 16));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_FILT_D2), b_d2 + 16));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_FILT_OUT), b_out));
    std::vector<char> h_in(b_in + 16), h_out(b_out);
    char *d_in = scratch<char>(ctx, S_FILT_IN), *d_d2 = scratch<char>(ctx, S_FILT_D2), *d_out = scratch<char>(ctx, S_FILT_OUT);
    FiltBatch B;
    std::memset(&B, 0, sizeof B);
    B.n_jobs = nm;
    size_t o_in = 0, o_d2 = 0, o_out = 0;
    std::vector<size_t> at_out(nm);
    for (int m = 0; m < nm; m++) {
        FiltJob &J = B.job[m];
        const size_t n = n_rows[m], N = n_cloud[m];
        J.n = (int)n;
        J.N = (int)N;
        B.first[m + 1] = B.first[m] + (N > 0 ? d2_blocks((long long)n) : 0);
        // inputs: the first n rows as they are, the cloud one axis after the other; and the magnitudes the band is made of
        double A = 0, Bm = 0, Rn = 0, H = 0;
        bool nan = false;      // fmax drops a NaN: keep it
        J.rows = (const double *)(d_in + o_in);
        if (n) std::memcpy(h_in.data() + o_in, rows[m], n * ROW_LEN * 8);
        for (size_t i = 0; i < n; i++) {
            const double *s = rows[m] + i * ROW_LEN;
            for (int k = 0; k < 3; k++) {
                A = std::fmax(A, std::fabs(s[ROW_HI + k]));
                Bm = std::fmax(Bm, std::fabs(s[ROW_LO + k]));
                const double rs = (std::fabs(s[ROW_R + 3 * k]) + std::fabs(s[ROW_R + 3 * k + 1])) + std::fabs(s[ROW_R + 3 * k + 2]);
                Rn = std::fmax(Rn, rs);
                nan |= std::isnan(s[ROW_HI + k]) || std::isnan(s[ROW_LO + k]) || std::isnan(rs);
            }
        }
        o_in += up16(n * ROW_LEN * 8);
        const double **axes[3] = {&J.cx, &J.cy, &J.cz};
        for (int a = 0; a < 3; a++) {
            double *dst = (double *)(h_in.data() + o_in);
            *axes[a] = (const double *)(d_in + o_in);
            for (size_t p = 0; p < N; p++) {
                dst[p] = cloud[m][3 * p + a];
                H = std::fmax(H, std::fabs(dst[p]));
                nan |= std::isnan(dst[p]);
            }
            o_in += up16(N * 8);
        }
        const double X = nan ? NAN : Rn * (H + A) + Bm;      // bound of a cloud coordinate and of every partial sum on the way to it
        J.c_sum = (3.0 * (double)N + MAD_FILT_SUM_C) * MAD_FILT_U;
        J.delta = 2.0 * MAD_FILT_POS_C * MAD_FILT_SQRT3 * MAD_FILT_U * X;      // length of the error of a difference of two cloud points
        J.d2 = (double *)(d_d2 + o_d2);
        o_d2 += d2_bytes(n);
        at_out[m] = o_out;
        J.d2min = (double *)(d_out + o_out);
        J.owner = (int32_t *)(d_out + o_out + up16(n * 8));
        J.meta = (int32_t *)(d_out + o_out + up16(n * 8) + up16(n * 4));
        o_out += up16(n * 8) + up16(n * 4) + 16;
    }
    const long long blocks = B.first[nm];
    if (blocks >= ((long long)1 << 31)) return mad_fail(ctx, MAD_EDOM, "mad_pose_cluster_many: %lld workgroups in one launch", blocks);
    const auto run = [&]() -> int {
        if (b_in) MAD_HIP(hipMemcpyAsync(d_in, h_in.data(), b_in, hipMemcpyHostToDevice, ctx->stream));
        if (blocks) hipLaunchKernelGGL(k_pose_d2, dim3((unsigned)blocks), dim3(64 * MAD_FILT_WAVES), 0, ctx->stream, B);
        hipLaunchKernelGGL(k_pose_greedy, dim3(nm), dim3(64), 0, ctx->stream, B, rmsd_thresh * rmsd_thresh);
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(h_out.data(), d_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));
        return MAD_OK;
    };
    const int rc = run();
    if (rc != MAD_OK) {      // h_in / h_out may still be the source / target of a copy in flight: wait before they go
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    for (int m = 0; m < nm; m++) {
        const size_t n = n_rows[m];
        const char *src = h_out.data() + at_out[m];
        if (n) std::memcpy(d2min_out[m], src, n * 8), std::memcpy(owner_out[m], src + up16(n * 8), n * 4);
        const int32_t *meta = (const int32_t *)(src + up16(n * 8) + up16(n * 4));
        n_done_out[m] = meta[0];
        status_out[m] = meta[1];
    }
    return MAD_OK;
}

extern "C" int mad_pose_cluster_many(mad_ctx *ctx, int n_match, const double *const *rows, const int32_t *n_rows,
                                     const double *const *cloud, const int32_t *n_cloud, double rmsd_thresh, int32_t *const *owner_out,
                                     double *const *d2min_out, int32_t *n_done_out, int32_t *status_out) {
    if (!ctx) return MAD_EINVAL;
    if (n_match < 0) return mad_fail(ctx, MAD_EINVAL, "mad_pose_cluster_many: n_match = %d", n_match);
    if (n_match == 0) return MAD_OK;
    if (!rows || !n_rows || !cloud || !n_cloud || !owner_out || !d2min_out || !n_done_out || !status_out) return MAD_EINVAL;
    if (!(rmsd_thresh >= 0) || !std::isfinite(rmsd_thresh)) return mad_fail(ctx, MAD_EINVAL, "mad_pose_cluster_many: rmsd_thresh = %g", rmsd_thresh);
    for (int m = 0; m < n_match; m++) {
        if (n_rows[m] < 0 || n_cloud[m] < 0) return mad_fail(ctx, MAD_EINVAL, "mad_pose_cluster_many: match %d has n = %d, N = %d", m, n_rows[m], n_cloud[m]);
        if (n_rows[m] > MAD_POSE_CLUSTER_MAX_N)
            return mad_fail(ctx, MAD_EDOM, "mad_pose_cluster_many: match %d has %d rows, the d2 triangle is sized for %d", m, n_rows[m], MAD_POSE_CLUSTER_MAX_N);
        if ((n_rows[m] && (!rows[m] || !owner_out[m] || !d2min_out[m])) || (n_cloud[m] && !cloud[m])) return MAD_EINVAL;
    }
    mad_use_lane(ctx, 0);
    for (int m0 = 0, nm; m0 < n_match; m0 += nm) {      // a launch: up to MAD_FILT_BATCH matches and MAD_FILT_D2_BYTES of triangles
        size_t bytes = d2_bytes((size_t)n_rows[m0]);
        for (nm = 1; m0 + nm < n_match && nm < MAD_FILT_BATCH && bytes + d2_bytes((size_t)n_rows[m0 + nm]) <= MAD_FILT_D2_BYTES; nm++)
            bytes += d2_bytes((size_t)n_rows[m0 + nm]);
        MAD_TRY(cluster_chunk(ctx, nm, rows + m0, n_rows + m0, cloud + m0, n_cloud + m0, rmsd_thresh, owner_out + m0, d2min_out + m0,
                              n_done_out + m0, status_out + m0));
    }
    return MAD_OK;
}
