// mad_segment.hip -- a Gaussian on a map, and a map cut into segments: watershed regions of the density, grouped by following their
// maxima through progressively smoothed copies of the map (the scheme of Segger).  The contract is DESIGN.md section 4j and the comment
// on mad_map_smooth / mad_map_segment in include/mad_amd.h: only comparisons decide a label, and the smoothing is float64 in a fixed
// order of operations (the build's -ffp-contract=off keeps products and sums apart).
//
//   k_seg_smooth_axis                      one axis of the separable Gaussian, taps outside the grid are 0.0 (zero extension)
//   k_seg_parent                           a workgroup per tile of 8 x 8 x 64 voxels staged in LDS with a one-voxel halo: the parent of
//                                          every voxel (the greatest of its 27-neighbourhood in the order), -1 for background
//   k_seg_jump                             pointer jumping in place until a pass changes nothing: p[i] = the root of i
//   k_seg_count / k_seg_scan_blocks / k_seg_assign
//                                          root flags -> exclusive scan over workgroups -> region ids in ascending L of the roots,
//                                          with the roots' indices and values (the regions' peaks) in scan order
//   k_seg_label                            labels = id[root], region sizes by integer atomics
//   k_seg_gather / k_seg_relabel           a region's point moved to its root in a smoothed map; region ids replaced by group ids
//
// Determinism: parents are comparisons; the jumping has one fixed point (every value ever stored in p[i] is an ancestor of i, and an
// aligned 32-bit store is whole); ids, roots and peaks come from a scan; sizes are integer sums.  No floating-point atomics.
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "mad_common.h"
#include "mad_segment_scan.h"      // SG_THREADS, and the jumping and numbering kernels with their constants

#define SG_TX 8                  // a workgroup's tile: 8 x 8 x 64 voxels, a wavefront per z row of 64 (lanes along z: loads coalesce)
#define SG_TY 8
#define SG_TZ 64
#define SG_HX (SG_TX + 2)
#define SG_HY (SG_TY + 2)
#define SG_HZ (SG_TZ + 2)
#define SG_MAX_R (1 << 20)       // taps of one side at most (sigma up to 2^18 voxels)
static_assert(SG_TZ == MAD_WAVE, "a wavefront per z row of the tile");
static_assert(SG_HX * SG_HY * SG_HZ * 4 < 30 * 1024, "the staged tile leaves room for two workgroups and more per CU");

struct SegDims {
    int n[3];
};

// ---------------------------------------------------------------------------
// smoothing
// ---------------------------------------------------------------------------

// out[i] = in[i] * w[0], then for k = R .. 1: += (in[i - k st] + in[i + k st]) * w[k], a tap outside the grid being 0.0.  One thread
// per voxel, z fastest, so that a wavefront's reads of every tap are contiguous whatever the axis.
template <typename Tin, typename Tout>
__global__ __launch_bounds__(SG_THREADS) void k_seg_smooth_axis(const Tin *__restrict__ in, SegDims d, int axis, int R, const double *__restrict__ w,
                                                                Tout *__restrict__ out, unsigned n_vox) {
    const unsigned i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= n_vox) return;
    const unsigned st = axis == 0 ? (unsigned)d.n[1] * (unsigned)d.n[2] : (axis == 1 ? (unsigned)d.n[2] : 1u);
    const int n = d.n[axis], pos = (int)((i / st) % (unsigned)n);
    double a = (double)in[i] * w[0];
    for (int k = R; k >= 1; k--) {
        const double lo = pos - k >= 0 ? (double)in[i - (unsigned)k * st] : 0.0;      // (k <= pos < n: the product stays below n_vox)
        const double hi = pos + k < n ? (double)in[i + (unsigned)k * st] : 0.0;
        a += (lo + hi) * w[k];
    }
    out[i] = (Tout)a;
}

// ---------------------------------------------------------------------------
// watershed
// ---------------------------------------------------------------------------

// Workgroup b owns tile (b / bz / by, b / bz % by, b % bz).  The tile and its halo go to LDS with background voxels and voxels
// outside the grid replaced by NaN, which no comparison below ever selects; the 27 values of a voxel are then LDS reads.  The
// neighbourhood is walked in ascending L with a strict >, so of equal values the one with the smallest L wins: the order of the
// contract without comparing an index.  *bad is raised for a voxel of the grid that is not finite.
__global__ __launch_bounds__(SG_THREADS) void k_seg_parent(const float *__restrict__ g, SegDims d, double thr, unsigned by, unsigned bz,
                                                           int *__restrict__ parent, int *__restrict__ bad) {
    __shared__ float s_v[SG_HX * SG_HY * SG_HZ];
    const unsigned b = blockIdx.x, tz = b % bz, bt = b / bz, ty = bt % by, tx = bt / by;
    const int x0 = (int)tx * SG_TX, y0 = (int)ty * SG_TY, z0 = (int)tz * SG_TZ;
    const int lane = (int)lane_id(), wv = (int)(threadIdx.x >> 6);
    const float nan = __builtin_nanf("");
    bool any_bad = false;
    for (int row = wv; row < SG_HX * SG_HY; row += SG_THREADS / MAD_WAVE) {
        const int hx = row / SG_HY, hy = row % SG_HY, gx = x0 - 1 + hx, gy = y0 - 1 + hy;
        const bool row_ok = gx >= 0 && gx < d.n[0] && gy >= 0 && gy < d.n[1];
        const long long base = ((long long)gx * d.n[1] + gy) * d.n[2];
#pragma unroll
        for (int part = 0; part < 2; part++) {
            const int hz = lane + part * MAD_WAVE;
            if (hz < SG_HZ) {
                const int gz = z0 - 1 + hz;
                float v = nan;
                if (row_ok && gz >= 0 && gz < d.n[2]) {
                    v = g[base + gz];
                    if (!(fabsf(v) <= 3.4028234663852886e38f)) any_bad = true;
                    if (!((double)v > thr)) v = nan;
                }
                s_v[row * SG_HZ + hz] = v;
            }
        }
    }
    if (any_bad) atomicOr(bad, 1);
    __syncthreads();
    for (int row = wv; row < SG_TX * SG_TY; row += SG_THREADS / MAD_WAVE) {
        const int cx = row / SG_TY, cy = row % SG_TY, x = x0 + cx, y = y0 + cy, z = z0 + lane;
        if (x >= d.n[0] || y >= d.n[1] || z >= d.n[2]) continue;
        const int L = (int)(((long long)x * d.n[1] + y) * d.n[2] + z);
        const float c = s_v[((cx + 1) * SG_HY + (cy + 1)) * SG_HZ + lane + 1];
        int best = -1;
        if (c == c) {      // foreground
            float bv = -INFINITY;
            best = L;      // (a foreground value is above -inf, so the voxel itself is taken unless an earlier equal or a greater one is)
            const int sx = d.n[1] * d.n[2], sy = d.n[2];
#pragma unroll
            for (int dx = -1; dx <= 1; dx++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dz = -1; dz <= 1; dz++) {
                        const float v = s_v[((cx + 1 + dx) * SG_HY + (cy + 1 + dy)) * SG_HZ + lane + 1 + dz];
                        if (v > bv) { bv = v; best = L + dx * sx + dy * sy + dz; }      // (false for a staged NaN: background, or outside the grid)
                    }
        }
        parent[L] = best;
    }
}

// k_seg_jump, k_seg_count, k_seg_scan_blocks, k_seg_assign: mad_segment_scan.h (shared with mad_components.hip)

// lab[i] = lab[root of i], 0 for background, in place: a root reads and writes its own id, nobody else's slot is read.  A wavefront
// whose 64 voxels share one region adds 64 to its size once.
__global__ __launch_bounds__(SG_THREADS) void k_seg_label(const int *__restrict__ p, int *__restrict__ lab, unsigned n_vox,
                                                          unsigned long long *__restrict__ size_tab) {
    const unsigned i = blockIdx.x * SG_THREADS + threadIdx.x;
    int id = 0;
    if (i < n_vox) {
        const int r = p[i];
        id = r < 0 ? 0 : lab[r];
    }
    const int first = __builtin_amdgcn_readfirstlane(id);
    if (__all(id == first)) {
        if (first > 0 && lane_id() == 0) atomicAdd(size_tab + (first - 1), (unsigned long long)MAD_WAVE);
    } else if (id > 0)
        atomicAdd(size_tab + (id - 1), 1ull);
    if (i < n_vox) lab[i] = id;
}

__global__ __launch_bounds__(SG_THREADS) void k_seg_gather(const int *__restrict__ q, int *__restrict__ point, int n) {
    const int r = (int)(blockIdx.x * SG_THREADS + threadIdx.x);
    if (r >= n) return;
    const int pt = point[r];
    if (pt >= 0) point[r] = q[pt];      // (every voxel of a smoothed map is foreground; a point never leaves the grid either way)
}

__global__ __launch_bounds__(SG_THREADS) void k_seg_points_init(const long long *__restrict__ root_tab, int *__restrict__ point, int n) {
    const int r = (int)(blockIdx.x * SG_THREADS + threadIdx.x);
    if (r < n) point[r] = (int)root_tab[r];
}

__global__ __launch_bounds__(SG_THREADS) void k_seg_relabel(int *__restrict__ lab, const int *__restrict__ group, unsigned n_vox) {
    const unsigned i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= n_vox) return;
    const int id = lab[i];
    if (id > 0) lab[i] = group[id - 1];
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

// The taps of the contract: w_k = exp(-0.5 k k / (sigma sigma)) / (w_0 + 2 (w_1 + w_2 + ...)), float64, libm exp.
static void seg_taps(double sigma, std::vector<double> &w) {
    const int R = (int)(4.0 * sigma + 0.5);
    w.resize((size_t)R + 1);
    for (int k = 0; k <= R; k++) w[k] = exp(-0.5 * (double)k * (double)k / (sigma * sigma));
    double s = 0.0;
    for (int k = 1; k <= R; k++) s += w[k];
    const double norm = w[0] + 2.0 * s;
    for (int k = 0; k <= R; k++) w[k] /= norm;
}

static bool seg_sigma_ok(double sigma) { return std::isfinite(sigma) && sigma > 0.0 && 4.0 * sigma + 0.5 < (double)SG_MAX_R; }

static int seg_check_dims(mad_ctx *ctx, const char *who, const int32_t dims[3], size_t *n_vox) {
    for (int k = 0; k < 3; k++)
        if (dims[k] < 1) return mad_fail(ctx, MAD_EINVAL, "%s: grid of %d x %d x %d voxels", who, dims[0], dims[1], dims[2]);
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 31) || vxy * (unsigned long long)dims[2] >= (1ull << 31))
        return mad_fail(ctx, MAD_EINVAL, "%s: %d x %d x %d voxels: grids of 2^31 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
    *n_vox = (size_t)(vxy * (unsigned long long)dims[2]);
    return MAD_OK;
}

// three passes: d_in (float32) -> a -> b -> d_out (float32; may be d_in or a's memory: the last pass reads b only)
static void seg_smooth_device(mad_ctx *ctx, const float *d_in, SegDims D, unsigned n_vox, int R, const double *d_w, double *a, double *b, float *d_out) {
    const unsigned nb = (unsigned)mad_ceil_div(n_vox, SG_THREADS);
    mad_timer_begin(ctx, MAD_T_SEG_SMOOTH);
    hipLaunchKernelGGL((k_seg_smooth_axis<float, double>), dim3(nb), dim3(SG_THREADS), 0, ctx->stream, d_in, D, 0, R, d_w, a, n_vox);
    hipLaunchKernelGGL((k_seg_smooth_axis<double, double>), dim3(nb), dim3(SG_THREADS), 0, ctx->stream, (const double *)a, D, 1, R, d_w, b, n_vox);
    hipLaunchKernelGGL((k_seg_smooth_axis<double, float>), dim3(nb), dim3(SG_THREADS), 0, ctx->stream, (const double *)b, D, 2, R, d_w, d_out, n_vox);
    mad_timer_end(ctx, MAD_T_SEG_SMOOTH);
}

extern "C" int mad_map_smooth(mad_ctx *ctx, const float *grid, const int32_t dims[3], double sigma_vox, float *out) {
    const char *who = "mad_map_smooth";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    size_t n_vox = 0;
    MAD_TRY(seg_check_dims(ctx, who, dims, &n_vox));
    if (!seg_sigma_ok(sigma_vox)) return mad_fail(ctx, MAD_EINVAL, "%s: sigma %g voxels (positive, finite, below 2^18)", who, sigma_vox);
    std::vector<double> w;
    seg_taps(sigma_vox, w);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), n_vox * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), n_vox * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), n_vox * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), 64 + w.size() * 8));
    float *d_g = scratch<float>(ctx, S_TMP_H);
    double *d_w = (double *)(scratch<char>(ctx, S_TMP_G) + 64);
    const SegDims D = {{dims[0], dims[1], dims[2]}};
    MAD_HIP(hipMemcpyAsync(d_g, grid, n_vox * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_w, w.data(), w.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    seg_smooth_device(ctx, d_g, D, (unsigned)n_vox, (int)w.size() - 1, d_w, scratch<double>(ctx, S_TMP_A), scratch<double>(ctx, S_TMP_B), d_g);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out, d_g, n_vox * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// parents of d_v (foreground: v > thr) into d_p, then jumped to roots.  d_ctl[0]: a voxel is not finite; d_ctl[1]: the pass stored.
static int seg_roots(mad_ctx *ctx, const float *d_v, SegDims D, unsigned n_vox, double thr, int *d_p, int *d_ctl) {
    const unsigned bx = (unsigned)mad_ceil_div(D.n[0], SG_TX), by = (unsigned)mad_ceil_div(D.n[1], SG_TY), bz = (unsigned)mad_ceil_div(D.n[2], SG_TZ);
    mad_timer_begin(ctx, MAD_T_SEG_PARENT);
    hipLaunchKernelGGL(k_seg_parent, dim3(bx * by * bz), dim3(SG_THREADS), 0, ctx->stream, d_v, D, thr, by, bz, d_p, d_ctl);      // a tile holds a voxel: fewer than 2^31
    mad_timer_end(ctx, MAD_T_SEG_PARENT);
    MAD_HIP(hipGetLastError());
    const unsigned nb = (unsigned)mad_ceil_div(n_vox, SG_THREADS);
    for (;;) {      // a pass takes every pointer that is not at its root at least one ancestor up, and SG_JUMP_HOPS where the chain allows
        int changed = 0;
        MAD_HIP(hipMemsetAsync(d_ctl + 1, 0, 4, ctx->stream));
        mad_timer_begin(ctx, MAD_T_SEG_JUMP);
        hipLaunchKernelGGL(k_seg_jump, dim3(nb), dim3(SG_THREADS), 0, ctx->stream, d_p, n_vox, d_ctl + 1);
        mad_timer_end(ctx, MAD_T_SEG_JUMP);
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(&changed, d_ctl + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));
        if (!changed) break;
    }
    return MAD_OK;
}

extern "C" int mad_map_segment(mad_ctx *ctx, const float *grid, const int32_t dims[3], double threshold, int32_t steps, double step,
                               int64_t stop_at, int32_t *labels, int64_t *root, float *peak, int64_t *size, int32_t *group, int64_t cap,
                               int64_t *n_regions, int64_t *history, int32_t *steps_done) {
    const char *who = "mad_map_segment";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !labels || !n_regions || !history || !steps_done)
        return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    size_t n_vox_z = 0;
    MAD_TRY(seg_check_dims(ctx, who, dims, &n_vox_z));
    if (threshold != threshold) return mad_fail(ctx, MAD_EINVAL, "%s: the threshold is not a number", who);
    if (steps < 0 || !(step > 0.0) || !std::isfinite(step) || stop_at < 0 || cap < 0)
        return mad_fail(ctx, MAD_EINVAL, "%s: steps %d, step %g, stop_at %lld, capacity %lld", who, steps, step, (long long)stop_at, (long long)cap);
    if (steps > 0 && !seg_sigma_ok((double)steps * step))
        return mad_fail(ctx, MAD_EINVAL, "%s: the last sigma, %g voxels, is not below 2^18", who, (double)steps * step);
    const unsigned n_vox = (unsigned)n_vox_z;
    const SegDims D = {{dims[0], dims[1], dims[2]}};

    // the taps of every step, one table
    std::vector<double> taps, w;
    std::vector<size_t> tap_off((size_t)steps + 1, 0);
    for (int s = 1; s <= steps; s++) {
        seg_taps((double)s * step, w);
        tap_off[s] = taps.size();
        taps.insert(taps.end(), w.begin(), w.end());
    }
    const int n_blocks = (int)mad_ceil_div(n_vox, SG_SCAN_PER);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), n_vox_z * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), n_vox_z * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), n_vox_z * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), 64 + taps.size() * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), 2 * ((size_t)n_blocks + 1) * 4));
    float *d_g = scratch<float>(ctx, S_TMP_H);
    int *d_p = scratch<int>(ctx, S_TMP_C), *d_lab = scratch<int>(ctx, S_TMP_D);
    int *d_ctl = scratch<int>(ctx, S_TMP_G);      // [0] a voxel is not finite, [1] a jumping pass stored
    double *d_taps = (double *)(scratch<char>(ctx, S_TMP_G) + 64);
    int *d_cnt = scratch<int>(ctx, S_TMP_F), *d_off = d_cnt + n_blocks + 1;

    MAD_HIP(hipMemcpyAsync(d_g, grid, n_vox_z * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemsetAsync(d_ctl, 0, 64, ctx->stream));
    if (!taps.empty()) MAD_HIP(hipMemcpyAsync(d_taps, taps.data(), taps.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    MAD_TRY(seg_roots(ctx, d_g, D, n_vox, threshold, d_p, d_ctl));
    mad_timer_begin(ctx, MAD_T_SEG_SCAN);
    hipLaunchKernelGGL(k_seg_count, dim3(n_blocks), dim3(SG_THREADS), 0, ctx->stream, (const int *)d_p, n_vox, d_cnt);
    hipLaunchKernelGGL(k_seg_scan_blocks, dim3(1), dim3(SG_SCAN_THREADS), 0, ctx->stream, (const int *)d_cnt, n_blocks, d_off);
    mad_timer_end(ctx, MAD_T_SEG_SCAN);
    MAD_HIP(hipGetLastError());
    int h_bad = 0, h_n = 0;
    MAD_HIP(hipMemcpyAsync(&h_bad, d_ctl, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(&h_n, d_off + n_blocks, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (h_bad) return mad_fail(ctx, MAD_EDOM, "%s: the map holds a voxel that is not finite", who);
    const int n = h_n;

    // the region tables: [root int64 n][size uint64 n][peak float32 n][point int32 n][group int32 n]
    const size_t n8 = ((size_t)n + 1) * 8, n4 = (((size_t)n + 1) * 4 + 7) & ~(size_t)7;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), 2 * n8 + 3 * n4));
    char *tab = scratch<char>(ctx, S_TMP_I);
    long long *d_root = (long long *)tab;
    unsigned long long *d_size = (unsigned long long *)(tab + n8);
    float *d_peak = (float *)(tab + 2 * n8);
    int *d_point = (int *)(tab + 2 * n8 + n4), *d_group = (int *)(tab + 2 * n8 + 2 * n4);
    const unsigned nb = (unsigned)mad_ceil_div(n_vox, SG_THREADS), nbr = (unsigned)std::max<int64_t>(1, mad_ceil_div(n, SG_THREADS));
    MAD_HIP(hipMemsetAsync(d_size, 0, n8, ctx->stream));
    mad_timer_begin(ctx, MAD_T_SEG_SCAN);
    hipLaunchKernelGGL(k_seg_assign, dim3(n_blocks), dim3(SG_THREADS), 0, ctx->stream, (const int *)d_p, (const float *)d_g, n_vox, (const int *)d_off,
                       d_lab, d_root, d_peak);
    hipLaunchKernelGGL(k_seg_label, dim3(nb), dim3(SG_THREADS), 0, ctx->stream, (const int *)d_p, d_lab, n_vox, d_size);
    mad_timer_end(ctx, MAD_T_SEG_SCAN);
    MAD_HIP(hipGetLastError());

    // grouping: a region's point follows the roots of the smoothed maps; the <= n points of a step are grouped on the host
    history[0] = n;
    int done = 0;
    std::vector<int> points, sorted;
    if (n > 0 && steps > 0) {
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), n_vox_z * 8));
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), n_vox_z * 8));
        double *d_a = scratch<double>(ctx, S_TMP_A), *d_b = scratch<double>(ctx, S_TMP_B);
        float *d_s = (float *)d_a;      // the smoothed map takes the first buffer's place: the last pass reads the second only
        hipLaunchKernelGGL(k_seg_points_init, dim3(nbr), dim3(SG_THREADS), 0, ctx->stream, (const long long *)d_root, d_point, n);
        points.resize((size_t)n);
        for (int s = 1; s <= steps; s++) {
            const int R = (int)((s < steps ? tap_off[s + 1] : taps.size()) - tap_off[s]) - 1;
            seg_smooth_device(ctx, d_g, D, n_vox, R, d_taps + tap_off[s], d_a, d_b, d_s);
            MAD_HIP(hipGetLastError());
            MAD_TRY(seg_roots(ctx, d_s, D, n_vox, -INFINITY, d_p, d_ctl + 2));      // every voxel foreground: a smoothed map is finite
            hipLaunchKernelGGL(k_seg_gather, dim3(nbr), dim3(SG_THREADS), 0, ctx->stream, (const int *)d_p, d_point, n);
            MAD_HIP(hipGetLastError());
            MAD_HIP(hipMemcpyAsync(points.data(), d_point, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
            MAD_HIP(hipStreamSynchronize(ctx->stream));
            sorted = points;
            std::sort(sorted.begin(), sorted.end());
            history[s] = (int64_t)(std::unique(sorted.begin(), sorted.end()) - sorted.begin());
            done = s;
            if (stop_at > 0 && history[s] <= stop_at) break;
        }
    }
    // groups, numbered by their smallest region
    std::vector<int32_t> h_group((size_t)n);
    int m = 0;
    if (done > 0) {
        std::unordered_map<int, int> of_point;
        of_point.reserve((size_t)n * 2);
        for (int r = 0; r < n; r++) {
            auto it = of_point.find(points[(size_t)r]);
            if (it == of_point.end()) it = of_point.emplace(points[(size_t)r], ++m).first;
            h_group[(size_t)r] = it->second;
        }
    } else
        for (int r = 0; r < n; r++) h_group[(size_t)r] = ++m;
    if (m < n) {
        MAD_HIP(hipMemcpyAsync(d_group, h_group.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_seg_relabel, dim3(nb), dim3(SG_THREADS), 0, ctx->stream, d_lab, (const int *)d_group, n_vox);
        MAD_HIP(hipGetLastError());
    }
    MAD_HIP(hipMemcpyAsync(labels, d_lab, n_vox_z * 4, hipMemcpyDeviceToHost, ctx->stream));
    const bool fits = (int64_t)n <= cap;
    if (fits && n > 0) {
        if (root) MAD_HIP(hipMemcpyAsync(root, d_root, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (size) MAD_HIP(hipMemcpyAsync(size, d_size, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (peak) MAD_HIP(hipMemcpyAsync(peak, d_peak, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (fits && group) memcpy(group, h_group.data(), (size_t)n * 4);
    *n_regions = n;
    *steps_done = done;
    if (!fits) return mad_fail(ctx, MAD_ENOSPC, "%s: %d regions, capacity %lld", who, n, (long long)cap);
    return MAD_OK;
}
