// mad_confidence.hip -- a full sort of a map's voxels, its order statistics, and the confidence map of Beckers, Jakobi and Sachse
// (IUCrJ 2019): noise from solvent boxes, a p-value per voxel, q-values that control the false discovery rate over all voxels, and the
// densities at which given rates are met.  DESIGN.md section 4w has the contract; mad_amd/confidence.py restates it with numpy;
// mad_confidence_plan.h holds the arithmetic and everything the host decides.
//
//   k_cf_count / mad_scan_i32 / k_cf_scatter   one pass of the radix sort (descending float32, keys only, least significant digit
//                                              first): the digits of every tile counted in LDS, the digit-major table scanned, the
//                                              keys ranked inside their tile (ballots per wavefront, counters per wavefront in LDS),
//                                              ordered by digit in LDS and written out in runs.  Kernels in stream order; none waits
//                                              for another workgroup.  The first pass reads the floats and forms the keys, the last
//                                              writes floats.
//   k_cf_noise / k_cf_tree                     the samples of the noise boxes summed by fourier.tree_sum's pairing, a level a launch
//   k_cf_r / k_cf_q_carry / k_cf_q_apply       r[j] = p[j] (N c) / (j + 1) along the descending keys, its reverse running minimum
//                                              (block minima, their exclusive suffix minimum, the apply) capped at 1
//   k_cf_lookup / k_cf_levels                  every voxel finds its value among the sorted ones (its q, its confidence); every level
//                                              its count and its density
//
// No float atomic anywhere, no sum whose order can vary: a call gives the same bits every time.
#include <utility>
#include <vector>

#include "mad_common.h"
#include "mad_confidence_plan.h"

static_assert(CF_THREADS == 4 * MAD_WAVE && CF_WAVES == 4, "four wavefronts: the scatter names their counters");

// ---------------------------------------------------------------------------
// the sort
// ---------------------------------------------------------------------------

// the lanes of the wavefront that are valid and hold the digit d of this lane (for a valid lane; others get no meaning)
__device__ __forceinline__ unsigned long long cf_match(unsigned d, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < CF_BITS; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

// tab[digit][tile] = the keys of the tile whose digit of this pass is `digit`.  FIRST: `in` holds float32 bits; the voxels that are not
// finite are counted into *bad.  The lanes of a wavefront that hold one digit add their number once.
template <bool FIRST>
__global__ __launch_bounds__(CF_THREADS) void k_cf_count(const uint32_t *__restrict__ in, unsigned n, unsigned tiles, int pass,
                                                         int32_t *__restrict__ tab, int *__restrict__ bad) {
    __shared__ unsigned s_h[CF_RADIX];
    const unsigned t = threadIdx.x, lane = lane_id(), tile = blockIdx.x;
    s_h[t] = 0u;
    __syncthreads();
    int not_finite = 0;
#pragma unroll 4
    for (unsigned r = 0; r < CF_ROUNDS; r++) {
        const unsigned i = cf_key_index(tile, t >> 6, r, lane);
        const bool valid = i < n;
        unsigned u = valid ? in[i] : 0u;
        if (FIRST) {
            not_finite += (valid && !cf_bits_finite(u)) ? 1 : 0;
            u = cf_key(u);
        }
        const unsigned d = cf_digit(u, pass);
        const unsigned long long m = cf_match(d, valid);
        if (valid && (m & lanemask_lt()) == 0ull) atomicAdd(s_h + d, (unsigned)__popcll(m));      // the first lane of its group
    }
    __syncthreads();
    tab[cf_table_index(t, tile, tiles)] = (int32_t)s_h[t];
    if (FIRST) {
        not_finite = wave_sum_i32(not_finite);
        if (lane == 0 && not_finite > 0) atomicAdd(bad, not_finite);
    }
}

// The keys of tile b go to out[off[digit][b] + their rank among the keys of the tile with that digit], the rank in the order of the
// tile: a stable pass.  off = the exclusive prefix sum of k_cf_count's table.  LAST: the values are written, not the keys.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(CF_THREADS) void k_cf_scatter(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, unsigned n, unsigned tiles,
                                                           int pass, const int32_t *__restrict__ off) {
    __shared__ unsigned s_keys[CF_TILE];
    __shared__ unsigned s_cnt[CF_WAVES][CF_RADIX];      // while ranking: the keys of a wavefront with a digit so far; then: those of the wavefronts before it
    __shared__ unsigned s_start[CF_RADIX];              // where a digit begins in s_keys
    __shared__ unsigned s_gbase[CF_RADIX];              // off[digit][tile] - s_start[digit] (modulo 2^32)
    __shared__ int warp_tot[CF_WAVES + 1];
    const unsigned t = threadIdx.x, lane = lane_id(), w = t >> 6, tile = blockIdx.x;
#pragma unroll
    for (int k = 0; k < CF_WAVES; k++) s_cnt[k][t] = 0u;
    unsigned key[CF_ROUNDS], rank[CF_ROUNDS];
#pragma unroll
    for (unsigned r = 0; r < CF_ROUNDS; r++) {
        const unsigned i = cf_key_index(tile, w, r, lane);
        const unsigned u = i < n ? in[i] : 0u;
        key[r] = FIRST ? cf_key(u) : u;
    }
    __syncthreads();
    const unsigned long long lt = lanemask_lt();
#pragma unroll
    for (unsigned r = 0; r < CF_ROUNDS; r++) {
        const bool valid = cf_key_index(tile, w, r, lane) < n;
        const unsigned d = cf_digit(key[r], pass);
        unsigned long long m = cf_match(d, valid);      // (every lane takes the ballots)
        if (!valid) m = 1ull << lane;
        const int leader = __ffsll((long long)m) - 1;
        unsigned pre = 0u;
        if (valid && (int)lane == leader) {      // one lane per digit the wavefront holds: no two write one counter
            pre = s_cnt[w][d];
            s_cnt[w][d] = pre + (unsigned)__popcll(m);
        }
        pre = (unsigned)__shfl((int)pre, leader);
        rank[r] = pre + (unsigned)__popcll(m & lt);
    }
    __syncthreads();
    {   // lane t is digit t: the wavefronts' counts become the counts of the wavefronts before, the totals the digits' starts
        const unsigned c0 = s_cnt[0][t], c1 = s_cnt[1][t], c2 = s_cnt[2][t], c3 = s_cnt[3][t];
        s_cnt[0][t] = 0u;
        s_cnt[1][t] = c0;
        s_cnt[2][t] = c0 + c1;
        s_cnt[3][t] = c0 + c1 + c2;
        int total = 0;
        const unsigned start = (unsigned)block_excl_scan((int)(c0 + c1 + c2 + c3), warp_tot, &total);
        s_start[t] = start;
        s_gbase[t] = (unsigned)off[cf_table_index(t, tile, tiles)] - start;
    }
    __syncthreads();
#pragma unroll
    for (unsigned r = 0; r < CF_ROUNDS; r++) {
        if (cf_key_index(tile, w, r, lane) < n) {
            const unsigned d = cf_digit(key[r], pass);
            s_keys[s_start[d] + s_cnt[w][d] + rank[r]] = key[r];      // below the tile's valid keys: every term counts keys of this tile
        }
    }
    __syncthreads();
    const unsigned n_valid = min((unsigned)CF_TILE, n - tile * (unsigned)CF_TILE);
#pragma unroll 4
    for (unsigned r = 0; r < CF_ROUNDS; r++) {
        const unsigned pos = r * CF_THREADS + t;
        if (pos < n_valid) {
            const unsigned k = s_keys[pos];
            out[s_gbase[cf_digit(k, pass)] + pos] = LAST ? cf_unkey(k) : k;      // inside this digit's run of this tile: below n
        }
    }
}

// out[i] = sorted[k[i] - 1]
__global__ __launch_bounds__(CF_THREADS) void k_cf_pick(const float *__restrict__ sorted, const long long *__restrict__ k, unsigned n_k,
                                                        float *__restrict__ out) {
    const unsigned i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < n_k) out[i] = sorted[k[i] - 1];
}

// ---------------------------------------------------------------------------
// the noise
// ---------------------------------------------------------------------------

// s[0] <- the sum of s[0 .. 255] by halving: x[:128] + x[128:], then 64, ... 1 (a run of fourier.tree_sum)
__device__ __forceinline__ void cf_run_sum(double *s, unsigned t) {
    __syncthreads();
    for (unsigned h = CF_RUN / 2; h >= 1; h >>= 1) {
        if (t < h) s[t] = s[t] + s[t + h];
        __syncthreads();
    }
}

// part[b] = the sum of run b of the samples (square = 0) or of their squared distances from mean (square = 1); the last run zero-padded
__global__ __launch_bounds__(CF_RUN) void k_cf_noise(const float *__restrict__ g, int ny, int nz, int n_boxes, const int32_t *__restrict__ boxes,
                                                     const long long *__restrict__ first, unsigned n_samples, double mean, int square,
                                                     double *__restrict__ part) {
    __shared__ double s[CF_RUN];
    const unsigned t = threadIdx.x;
    const unsigned long long i = (unsigned long long)blockIdx.x * CF_RUN + t;
    double v = 0.0;
    if (i < n_samples) {
        const double x = (double)g[cf_sample_voxel((int64_t)i, n_boxes, boxes, (const int64_t *)first, ny, nz)];
        const double d = x - mean;
        v = square ? d * d : x;
    }
    s[t] = v;
    cf_run_sum(s, t);
    if (t == 0) part[blockIdx.x] = s[0];
}

// one level of tree_sum: out[b] = the sum of run b of in[0 .. n_in)
__global__ __launch_bounds__(CF_RUN) void k_cf_tree(const double *__restrict__ in, unsigned n_in, double *__restrict__ out) {
    __shared__ double s[CF_RUN];
    const unsigned t = threadIdx.x;
    const unsigned long long i = (unsigned long long)blockIdx.x * CF_RUN + t;
    s[t] = i < n_in ? in[i] : 0.0;
    cf_run_sum(s, t);
    if (t == 0) out[blockIdx.x] = s[0];
}

// ---------------------------------------------------------------------------
// p, q
// ---------------------------------------------------------------------------

__device__ __forceinline__ double cf_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, MAD_WAVE));
    return v;
}

// s[t] <- min of s[t ..] over the workgroup's lanes; returns the minimum over the lanes after t (+inf for the last)
__device__ __forceinline__ double cf_block_suffix_min(double *s, double v, unsigned t, unsigned T) {
    s[t] = v;
    for (unsigned o = 1; o < T; o <<= 1) {
        __syncthreads();
        const double x = t + o < T ? s[t + o] : INFINITY;
        __syncthreads();
        s[t] = fmin(s[t], x);
    }
    __syncthreads();
    const double after = t + 1 < T ? s[t + 1] : INFINITY;
    __syncthreads();
    return after;
}

// r[j] = p[j] (N c) / (j + 1), p = erfc(((s[j] - mean) / sd) / sqrt 2) / 2, in the contract's order; blk_min[b] = the least r of
// workgroup b's CF_QBLOCK values.  A minimum is exact in any order.
__global__ __launch_bounds__(CF_THREADS) void k_cf_r(const float *__restrict__ sorted, unsigned n, double mean, double sd, double nc,
                                                     double *__restrict__ r, double *__restrict__ blk_min) {
    __shared__ double s_m[CF_WAVES];
    const unsigned t = threadIdx.x;
    double m = INFINITY;
#pragma unroll 2
    for (unsigned e = 0; e < CF_QPER; e++) {
        const unsigned long long j = (unsigned long long)blockIdx.x * CF_QBLOCK + e * CF_THREADS + t;
        if (j < n) {
            const double z = ((double)sorted[j] - mean) / sd;
            const double p = 0.5 * erfc(z / 1.4142135623730951);
            const double v = p * nc / (double)(j + 1ull);
            r[j] = v;
            m = fmin(m, v);
        }
    }
    m = cf_wave_min(m);
    if (lane_id() == 0) s_m[t >> 6] = m;
    __syncthreads();
    if (t == 0) blk_min[blockIdx.x] = fmin(fmin(s_m[0], s_m[1]), fmin(s_m[2], s_m[3]));
}

// One workgroup: carry[b] = the least of blk_min[b + 1 ..], +inf for the last.
__global__ __launch_bounds__(1024) void k_cf_q_carry(const double *__restrict__ blk_min, unsigned nb, double *__restrict__ carry) {
    __shared__ double s[1024];
    const unsigned t = threadIdx.x, per = (nb + 1023u) / 1024u;
    const unsigned long long c0l = (unsigned long long)t * per;
    const unsigned c0 = c0l < nb ? (unsigned)c0l : nb, c1 = c0l + per < nb ? (unsigned)(c0l + per) : nb;
    double m = INFINITY;
    for (unsigned c = c0; c < c1; c++) m = fmin(m, blk_min[c]);
    double run = cf_block_suffix_min(s, m, t, 1024u);
    for (unsigned c = c1; c > c0; c--) {
        carry[c - 1] = run;
        run = fmin(run, blk_min[c - 1]);
    }
}

// q[j] = min(1, r[j], r[j + 1], ...) in place: lane t takes CF_QPER consecutive values
__global__ __launch_bounds__(CF_THREADS) void k_cf_q_apply(double *__restrict__ q, unsigned n, const double *__restrict__ carry) {
    __shared__ double s[CF_THREADS];
    const unsigned t = threadIdx.x;
    const unsigned long long j0 = (unsigned long long)blockIdx.x * CF_QBLOCK + (unsigned long long)t * CF_QPER;
    double m[CF_QPER];
#pragma unroll
    for (int e = 0; e < CF_QPER; e++) m[e] = j0 + e < n ? q[j0 + e] : INFINITY;
#pragma unroll
    for (int e = CF_QPER - 2; e >= 0; e--) m[e] = fmin(m[e], m[e + 1]);
    const double after = fmin(fmin(cf_block_suffix_min(s, m[0], t, CF_THREADS), carry[blockIdx.x]), 1.0);
#pragma unroll
    for (int e = 0; e < CF_QPER; e++)
        if (j0 + e < n) q[j0 + e] = fmin(m[e], after);
}

// Voxel i finds its value among the sorted ones (equal values have equal q: any of them): q_out[i] (may be NULL) = its q,
// conf[i] = (float)(1 - q).
__global__ __launch_bounds__(CF_THREADS) void k_cf_lookup(const uint32_t *__restrict__ grid, const uint32_t *__restrict__ sorted,
                                                          const double *__restrict__ qs, unsigned n, float *__restrict__ conf,
                                                          double *__restrict__ q_out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * CF_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long j = cf_find_key(sorted, (int64_t)n, cf_key(grid[i]));
    const double q = j >= 0 ? qs[j] : 1.0;      // (a finite voxel is found)
    conf[i] = (float)(1.0 - q);
    if (q_out) q_out[i] = q;
}

// level l: count[l] = the voxels with q <= levels[l], value[l] = the least density among them (NaN where there is none)
__global__ __launch_bounds__(CF_THREADS) void k_cf_levels(const double *__restrict__ qs, const float *__restrict__ sorted, unsigned n, int n_levels,
                                                          const double *__restrict__ levels, long long *__restrict__ count, float *__restrict__ value) {
    const int l = (int)(blockIdx.x * CF_THREADS + threadIdx.x);
    if (l >= n_levels) return;
    const long long c = cf_level_count(qs, (int64_t)n, levels[l]);
    count[l] = c;
    value[l] = c > 0 ? sorted[c - 1] : __builtin_nanf("");
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

struct CfDevice {
    uint32_t *grid = nullptr;      // the voxels' bits, as given
    float *sorted = nullptr;       // descending
};

// The grid to the device (S_TMP_H) and sorted (into S_TMP_C or S_TMP_D; the other holds keys).  MAD_EDOM, before anything is copied
// back, for a voxel that is not finite.
static int cf_sort(mad_ctx *ctx, const char *who, const float *grid, const CfPlan &P, CfDevice &R) {
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), P.key_bytes));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), P.key_bytes));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), P.key_bytes));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), 2 * P.table_bytes));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), 64));
    uint32_t *d_g = scratch<uint32_t>(ctx, S_TMP_H), *d_a = scratch<uint32_t>(ctx, S_TMP_C), *d_b = scratch<uint32_t>(ctx, S_TMP_D);
    int32_t *d_tab = scratch<int32_t>(ctx, S_TMP_F), *d_off = (int32_t *)(scratch<char>(ctx, S_TMP_F) + P.table_bytes);
    int *d_bad = scratch<int>(ctx, S_TMP_G);
    MAD_HIP(hipMemcpyAsync(d_g, grid, P.key_bytes, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemsetAsync(d_bad, 0, 64, ctx->stream));
    const dim3 wgs(P.tiles), th(CF_THREADS);
    const uint32_t *in = d_g;
    uint32_t *out = d_a;
    mad_timer_begin(ctx, MAD_T_CF_SORT);
    for (int pass = 0; pass < CF_PASSES; pass++) {
        if (pass == 0) hipLaunchKernelGGL((k_cf_count<true>), wgs, th, 0, ctx->stream, in, P.n, P.tiles, pass, d_tab, d_bad);
        else hipLaunchKernelGGL((k_cf_count<false>), wgs, th, 0, ctx->stream, in, P.n, P.tiles, pass, d_tab, d_bad);
        MAD_TRY(mad_scan_i32(ctx, d_tab, d_off, (int64_t)P.table));
        if (pass == 0) hipLaunchKernelGGL((k_cf_scatter<true, false>), wgs, th, 0, ctx->stream, in, out, P.n, P.tiles, pass, (const int32_t *)d_off);
        else if (pass == CF_PASSES - 1) hipLaunchKernelGGL((k_cf_scatter<false, true>), wgs, th, 0, ctx->stream, in, out, P.n, P.tiles, pass, (const int32_t *)d_off);
        else hipLaunchKernelGGL((k_cf_scatter<false, false>), wgs, th, 0, ctx->stream, in, out, P.n, P.tiles, pass, (const int32_t *)d_off);
        in = out;
        out = out == d_a ? d_b : d_a;
    }
    mad_timer_end(ctx, MAD_T_CF_SORT);
    MAD_HIP(hipGetLastError());
    int h_bad = 0;
    MAD_HIP(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (h_bad) return mad_fail(ctx, MAD_EDOM, "%s: the map holds %d voxels that are not finite (NaN or Inf)", who, h_bad);
    R.grid = d_g;
    R.sorted = (float *)in;
    return MAD_OK;
}

extern "C" int mad_map_sort(mad_ctx *ctx, const float *grid, int64_t n, float *out_desc) {
    const char *who = "mad_map_sort";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !out_desc) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    CfPlan P;
    char msg[320];
    if (cf_plan(who, n, P, msg, sizeof msg) != CF_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    CfDevice R;
    MAD_TRY(cf_sort(ctx, who, grid, P, R));
    MAD_HIP(hipMemcpyAsync(out_desc, R.sorted, P.key_bytes, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

extern "C" int mad_map_kth(mad_ctx *ctx, const float *grid, int64_t n, int64_t n_k, const int64_t *k, float *out) {
    const char *who = "mad_map_kth";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !k || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    CfPlan P;
    char msg[320];
    if (cf_plan(who, n, P, msg, sizeof msg) != CF_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    if (cf_kth_args(who, n, n_k, k, msg, sizeof msg) != CF_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    CfDevice R;
    MAD_TRY(cf_sort(ctx, who, grid, P, R));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), (size_t)n_k * 12));
    long long *d_k = scratch<long long>(ctx, S_TMP_E);
    float *d_out = (float *)(d_k + n_k);
    MAD_HIP(hipMemcpyAsync(d_k, k, (size_t)n_k * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_cf_pick, dim3((unsigned)mad_ceil_div(n_k, CF_THREADS)), dim3(CF_THREADS), 0, ctx->stream, (const float *)R.sorted,
                       (const long long *)d_k, (unsigned)n_k, d_out);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out, d_out, (size_t)n_k * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// tree_sum of the samples (square = 0) or of their squared distances from mean -> *sum.  part_a holds ceil(n / 256) doubles, part_b
// ceil of that / 256, rec one.
static int cf_noise_sum(mad_ctx *ctx, const float *d_g, const int32_t dims[3], int32_t n_boxes, const int32_t *d_boxes, const long long *d_first,
                        unsigned n_samples, double mean, int square, double *part_a, double *part_b, double *rec, double *sum) {
    unsigned runs = (unsigned)mad_ceil_div(n_samples, CF_RUN);
    mad_timer_begin(ctx, MAD_T_CF_NOISE);
    hipLaunchKernelGGL(k_cf_noise, dim3(runs), dim3(CF_RUN), 0, ctx->stream, d_g, dims[1], dims[2], n_boxes, d_boxes, d_first, n_samples, mean, square,
                       runs == 1 ? rec : part_a);
    double *in = part_a, *out = part_b;
    while (runs > 1) {
        const unsigned m = (unsigned)mad_ceil_div(runs, CF_RUN);
        hipLaunchKernelGGL(k_cf_tree, dim3(m), dim3(CF_RUN), 0, ctx->stream, (const double *)in, runs, m == 1 ? rec : out);
        std::swap(in, out);
        runs = m;
    }
    mad_timer_end(ctx, MAD_T_CF_NOISE);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(sum, rec, 8, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

extern "C" int mad_map_confidence(mad_ctx *ctx, const float *grid, const int32_t dims[3], int32_t n_boxes, const int32_t *boxes, double c,
                                  int32_t n_levels, const double *levels, float *out_confidence, double *out_q, float *out_sorted,
                                  double *out_q_sorted, int64_t *out_level_count, float *out_level_value, double stats[3]) {
    const char *who = "mad_map_confidence";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !boxes || !out_confidence || !stats || (n_levels > 0 && (!levels || !out_level_count || !out_level_value)))
        return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    CfPlan P;
    char msg[320];
    if (cf_plan_dims(who, dims, P, msg, sizeof msg) != CF_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    if (cf_levels(who, c, n_levels, levels, msg, sizeof msg) != CF_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    std::vector<int64_t> first((size_t)(n_boxes > 0 && n_boxes <= CF_MAX_BOXES ? n_boxes : 0) + 1);
    int64_t n_samples = 0;
    if (cf_boxes(who, dims, n_boxes, boxes, first.data(), &n_samples, msg, sizeof msg) != CF_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);

    CfDevice R;
    MAD_TRY(cf_sort(ctx, who, grid, P, R));

    // small things: [first int64 n_boxes + 1][boxes int32 4 n_boxes][levels double][counts int64][values float][rec double][parts]
    const size_t runs_a = (size_t)mad_ceil_div(n_samples, CF_RUN), runs_b = (size_t)mad_ceil_div((int64_t)runs_a, CF_RUN);
    const size_t nl = (size_t)(n_levels > 0 ? n_levels : 1), nb8 = ((size_t)n_boxes + 1) * 8, nb16 = (size_t)n_boxes * 16;
    const size_t small = nb8 + nb16 + nl * 24 + 8 + (runs_a + runs_b) * 8 + 2 * (size_t)P.q_blocks * 8;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), small));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (size_t)P.n * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_J), (size_t)P.n * (out_q ? 12 : 4)));
    char *sm = scratch<char>(ctx, S_TMP_E);
    long long *d_first = (long long *)sm;
    int32_t *d_boxes = (int32_t *)(sm + nb8);
    double *d_levels = (double *)(sm + nb8 + nb16);
    long long *d_count = (long long *)(d_levels + nl);
    double *d_rec = (double *)(d_count + nl), *d_part_a = d_rec + 1, *d_part_b = d_part_a + runs_a;
    double *d_blk = d_part_b + runs_b, *d_carry = d_blk + P.q_blocks;
    float *d_value = (float *)(d_carry + P.q_blocks);
    double *d_qs = scratch<double>(ctx, S_TMP_I);
    double *d_q = out_q ? scratch<double>(ctx, S_TMP_J) : nullptr;
    float *d_conf = (float *)(scratch<char>(ctx, S_TMP_J) + (out_q ? (size_t)P.n * 8 : 0));
    MAD_HIP(hipMemcpyAsync(d_first, first.data(), nb8, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_boxes, boxes, nb16, hipMemcpyHostToDevice, ctx->stream));
    if (n_levels > 0) MAD_HIP(hipMemcpyAsync(d_levels, levels, (size_t)n_levels * 8, hipMemcpyHostToDevice, ctx->stream));

    // mean = tree_sum(s) / n, var = tree_sum((s - mean)^2) / (n - 1): the divisions here, IEEE on either side
    double sum = 0.0, sum2 = 0.0;
    MAD_TRY(cf_noise_sum(ctx, (const float *)R.grid, dims, n_boxes, d_boxes, d_first, (unsigned)n_samples, 0.0, 0, d_part_a, d_part_b, d_rec, &sum));
    const double mean = sum / (double)n_samples;
    MAD_TRY(cf_noise_sum(ctx, (const float *)R.grid, dims, n_boxes, d_boxes, d_first, (unsigned)n_samples, mean, 1, d_part_a, d_part_b, d_rec, &sum2));
    const double var = sum2 / (double)(n_samples - 1);
    if (!(var > 0.0) || !std::isfinite(var))
        return mad_fail(ctx, MAD_EDOM,
                        "%s: the %lld voxels of the noise boxes have variance %g: no noise to measure there (a map already masked to a "
                        "constant has none in its corners); bring boxes= that lie in the solvent",
                        who, (long long)n_samples, var);
    const double sd = sqrt(var), nc = (double)P.n * c;

    mad_timer_begin(ctx, MAD_T_CF_Q);
    hipLaunchKernelGGL(k_cf_r, dim3(P.q_blocks), dim3(CF_THREADS), 0, ctx->stream, (const float *)R.sorted, P.n, mean, sd, nc, d_qs, d_blk);
    hipLaunchKernelGGL(k_cf_q_carry, dim3(1), dim3(1024), 0, ctx->stream, (const double *)d_blk, P.q_blocks, d_carry);
    hipLaunchKernelGGL(k_cf_q_apply, dim3(P.q_blocks), dim3(CF_THREADS), 0, ctx->stream, d_qs, P.n, (const double *)d_carry);
    mad_timer_end(ctx, MAD_T_CF_Q);
    mad_timer_begin(ctx, MAD_T_CF_LOOKUP);
    hipLaunchKernelGGL(k_cf_lookup, dim3((unsigned)mad_ceil_div(P.n, CF_THREADS)), dim3(CF_THREADS), 0, ctx->stream, (const uint32_t *)R.grid,
                       (const uint32_t *)R.sorted, (const double *)d_qs, P.n, d_conf, d_q);
    if (n_levels > 0)
        hipLaunchKernelGGL(k_cf_levels, dim3((unsigned)mad_ceil_div(n_levels, CF_THREADS)), dim3(CF_THREADS), 0, ctx->stream, (const double *)d_qs,
                           (const float *)R.sorted, P.n, n_levels, (const double *)d_levels, d_count, d_value);
    mad_timer_end(ctx, MAD_T_CF_LOOKUP);
    MAD_HIP(hipGetLastError());

    MAD_HIP(hipMemcpyAsync(out_confidence, d_conf, P.key_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_q) MAD_HIP(hipMemcpyAsync(out_q, d_q, (size_t)P.n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_sorted) MAD_HIP(hipMemcpyAsync(out_sorted, R.sorted, P.key_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_q_sorted) MAD_HIP(hipMemcpyAsync(out_q_sorted, d_qs, (size_t)P.n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n_levels > 0) {
        MAD_HIP(hipMemcpyAsync(out_level_count, d_count, (size_t)n_levels * 8, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipMemcpyAsync(out_level_value, d_value, (size_t)n_levels * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    stats[0] = mean;
    stats[1] = var;
    stats[2] = (double)n_samples;
    return MAD_OK;
}
