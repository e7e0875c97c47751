// mad_components.hip -- the connected components of the voxels of a map above a threshold, and a map with its small components
// ("dust") replaced by a fill value.  The contract is DESIGN.md section 4t and the comment on mad_map_components / mad_map_dust in
// include/mad_amd.h: only comparisons and integers decide a label, so every output is the same bits every call.
//
//   k_cc_tile                              a workgroup per tile of 8 x 8 x 64 voxels: a union-find over the tile's voxels in LDS (runs
//                                          along z by ballot, then the forward half of the neighbourhood with atomicMin on roots),
//                                          written out as p[L] = the smallest L of L's component WITHIN the tile, -1 for background
//   k_cc_border                            voxels on a tile face: a union on the global p with every forward neighbour in another tile
//   k_seg_jump, k_seg_count, k_seg_scan_blocks, k_seg_assign (mad_segment_scan.h)
//                                          pointers jumped to the roots; ids in ascending L of the roots, root table
//   k_cc_label                             labels = id[root]; sizes summed per wavefront, then per workgroup in LDS, then by integer
//                                          atomics (k_seg_label adds per voxel: right for a watershed's small regions, but a component
//                                          can be most of the map, and a million adds to one address take 18 ms)
//   k_cc_select                            mad_map_dust: a foreground voxel of a component that is not kept becomes the fill value
//
// Determinism: a link only ever points from a voxel to one of smaller L in its component, and no union is lost, so the jumping ends with
// every voxel at the smallest L of its component whatever order the atomics landed in; ids come from a scan; sizes are integer sums.
// No loop waits for another workgroup: every iteration of a find or a union ends or strictly lowers an index.  No floating-point atomics.
#include <vector>

#include "mad_common.h"
#include "mad_components_plan.h"
#include "mad_segment_scan.h"

static_assert(CC_TZ == MAD_WAVE, "a wavefront per z row of the tile");
static_assert(CC_THREADS == SG_THREADS, "one workgroup size throughout");
static_assert(CC_TILE * 4 < 30 * 1024, "the tile's union-find (LDS atomics are 32-bit: an int per voxel) leaves room for two workgroups and more per CU");

struct CcDims {
    int n[3];
};

// The root of x in the LDS forest: parents only ever fall, a root is its own parent.  Relaxed workgroup-scope loads (a plain ds_read):
// whatever is read was stored at some time, hence is an ancestor of x or a member of its component below it.
__device__ __forceinline__ int cc_find_lds(int *s, int x) {
    for (;;) {
        const int q = __hip_atomic_load(s + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q == x) return x;
        x = q;      // q < x
    }
}

// a and b become one tree: the larger root is hung under the smaller one.  atomicMin returns what the slot held: the node itself
// means the link is made; anything else (< a) was a's parent meanwhile, of a's component, and is united with b in turn.  max(a, b)
// falls strictly from one iteration to the next.
__device__ __forceinline__ void cc_union_lds(int *s, int a, int b) {
    a = cc_find_lds(s, a);
    b = cc_find_lds(s, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(s + a, b);
        if (old == a) break;
        a = cc_find_lds(s, old);
        b = cc_find_lds(s, b);
    }
}

// The same two on the global forest, between workgroups.  The loads are plain: one may be served by a cache that an atomic of another
// workgroup has not reached.  Such a value was stored in that slot at some time, so it names a member of the same component with a
// smaller or equal L (section 4t argues why that costs a round and never a merge); the link itself is made by the atomic alone.
__device__ __forceinline__ int cc_find(const int *p, int x) {
    for (;;) {
        const int q = p[x];
        if (q == x) return x;
        x = q;      // q < x
    }
}

__device__ __forceinline__ void cc_union(int *p, int a, int b) {
    a = cc_find(p, a);
    b = cc_find(p, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(p + a, b);
        if (old == a) break;
        a = cc_find(p, old);
        b = cc_find(p, b);
    }
}

// Workgroup b owns tile (b / bz / by, b / bz % by, b % bz), a wavefront takes a z row at a time.  s_p[l] is the parent of local voxel
// l = cc_local(cx, cy, cz), -1 for background and for voxels outside the grid.  A row's runs of foreground along z start as flat
// trees under their first voxel (a ballot), which is the offset (0, 0, 1) done; the other forward offsets are unions.  A pair
// (l, m) whose predecessors along z (l - 1, m - 1) are both foreground is skipped: the runs join l - 1 to l and m - 1 to m, and the
// pair (l - 1, m - 1) has the same offset.  *bad is raised for a voxel of the grid that is not finite.
template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void k_cc_tile(const float *__restrict__ g, CcDims d, double thr, unsigned by, unsigned bz,
                                                        int *__restrict__ p, int *__restrict__ bad) {
    __shared__ int s_p[CC_TILE];
    const unsigned b = blockIdx.x, tz = b % bz, bt = b / bz, ty = bt % by, tx = bt / by;
    const int x0 = (int)tx * CC_TX, y0 = (int)ty * CC_TY, z0 = (int)tz * CC_TZ;
    const int lane = (int)lane_id(), wv = (int)(threadIdx.x >> 6);
    bool any_bad = false;
    for (int row = wv; row < CC_ROWS; row += CC_THREADS / MAD_WAVE) {
        const int cx = row / CC_TY, cy = row % CC_TY, x = x0 + cx, y = y0 + cy, z = z0 + lane;
        bool fg = false;
        if (x < d.n[0] && y < d.n[1] && z < d.n[2]) {
            const float v = g[((long long)x * d.n[1] + y) * d.n[2] + z];
            if (!(fabsf(v) <= 3.4028234663852886e38f)) any_bad = true;
            fg = (double)v > thr;
        }
        const unsigned long long m = __ballot(fg);
        const unsigned long long gaps = ~m & ((1ull << lane) - 1ull);      // background lanes below this one
        const int start = gaps ? 64 - __clzll((long long)gaps) : 0;       // one past the highest of them: where this lane's run begins
        s_p[cc_local(cx, cy, lane)] = fg ? cc_local(cx, cy, start) : -1;
    }
    if (any_bad) atomicOr(bad, 1);
    __syncthreads();
    for (int row = wv; row < CC_ROWS; row += CC_THREADS / MAD_WAVE) {
        const int cx = row / CC_TY, cy = row % CC_TY, l = cc_local(cx, cy, lane);
        if (s_p[l] < 0) continue;      // (the sign of an entry never changes)
        const bool prev = lane > 0 && s_p[l - 1] >= 0;
#pragma unroll
        for (int dx = 0; dx <= 1; dx++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dz = -1; dz <= 1; dz++) {
                    if (!cc_is_forward(dx, dy, dz, CONN) || (dx == 0 && dy == 0)) continue;
                    const int ncx = cx + dx, ncy = cy + dy, ncz = lane + dz;
                    if (!cc_in_tile(ncx, ncy, ncz)) continue;      // (another tile's, or none: k_cc_border)
                    const int m = cc_local(ncx, ncy, ncz);
                    if (s_p[m] < 0) continue;
                    if (prev && ncz > 0 && s_p[m - 1] >= 0) continue;
                    cc_union_lds(s_p, l, m);
                }
    }
    __syncthreads();
    for (int row = wv; row < CC_ROWS; row += CC_THREADS / MAD_WAVE) {
        const int cx = row / CC_TY, cy = row % CC_TY, x = x0 + cx, y = y0 + cy, z = z0 + lane;
        if (x >= d.n[0] || y >= d.n[1] || z >= d.n[2]) continue;
        const int l = cc_local(cx, cy, lane);
        int out = -1;
        if (s_p[l] >= 0) {
            const int r = cc_find_lds(s_p, l);      // (nothing is stored any more: the root itself)
            const int rx = r / (CC_TY * CC_TZ), ry = r / CC_TZ % CC_TY, rz = r % CC_TZ;
            out = (int)(((long long)(x0 + rx) * d.n[1] + (y0 + ry)) * d.n[2] + (z0 + rz));
        }
        p[((long long)x * d.n[1] + y) * d.n[2] + z] = out;
    }
}

// The same tiles, CC_BORDER_Y workgroups to each (blockIdx.y), a wavefront per z row: the dependent loads of a find are then hidden
// behind many wavefronts and not queued up in one.  A foreground voxel on a tile face is united with each foreground forward
// neighbour that lies inside the grid and in another tile; rows off the faces take part with their two end voxels only.  Every pair
// of neighbouring voxels in different tiles is met once, from its member with the smaller L.  As in k_cc_tile a pair (L, M) is
// skipped where its predecessors along z (L - 1, M - 1) are both foreground, in the tiles of L and of M, and a pair of this kernel
// themselves (the row is on a face): k_cc_tile has joined L - 1 to L and M - 1 to M.
template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void k_cc_border(CcDims d, unsigned by, unsigned bz, int *p) {
    const unsigned b = blockIdx.x, tz = b % bz, bt = b / bz, ty = bt % by, tx = bt / by;
    const int x0 = (int)tx * CC_TX, y0 = (int)ty * CC_TY, z0 = (int)tz * CC_TZ;
    const int lane = (int)lane_id(), row = (int)blockIdx.y * (CC_THREADS / MAD_WAVE) + (int)(threadIdx.x >> 6);
    const int cx = row / CC_TY, cy = row % CC_TY, x = x0 + cx, y = y0 + cy, z = z0 + lane;
    if (x >= d.n[0] || y >= d.n[1] || z >= d.n[2] || !cc_on_face(cx, cy, lane)) return;
    const int sx = d.n[1] * d.n[2], sy = d.n[2];
    const int L = (int)(((long long)x * d.n[1] + y) * d.n[2] + z);
    if (p[L] < 0) return;
    const bool prev = cc_row_on_face(cx, cy) && lane > 0 && p[L - 1] >= 0;
#pragma unroll
    for (int dx = 0; dx <= 1; dx++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dz = -1; dz <= 1; dz++) {
                if (!cc_is_forward(dx, dy, dz, CONN)) continue;
                if (cc_in_tile(cx + dx, cy + dy, lane + dz)) continue;      // (k_cc_tile's)
                const int X = x + dx, Y = y + dy, Z = z + dz;
                if (X >= d.n[0] || Y < 0 || Y >= d.n[1] || Z < 0 || Z >= d.n[2]) continue;      // (dx >= 0)
                const int M = L + dx * sx + dy * sy + dz;
                if (p[M] < 0) continue;
                if (prev && Z % CC_TZ != 0 && p[M - 1] >= 0) continue;      // (M - 1 is in M's tile)
                cc_union(p, L, M);
            }
}

// lab[i] = lab[root of i], 0 for background, in place (a root reads and writes its own id, nobody else's slot is read), and the sizes.
// A workgroup takes CC_LABEL_PER consecutive voxels.  The lanes of a wavefront that hold one id add their number once, to a table
// of CC_LABEL_SLOTS (id, count) pairs in LDS; an id whose slot another id holds goes to the size table at once, the slots at the end.
// Integer sums: the order shows nowhere.
__global__ __launch_bounds__(CC_THREADS) void k_cc_label(const int *__restrict__ p, int *__restrict__ lab, unsigned n_vox,
                                                         unsigned long long *__restrict__ size_tab) {
    __shared__ int s_key[CC_LABEL_SLOTS];
    __shared__ unsigned s_cnt[CC_LABEL_SLOTS];
    for (int k = (int)threadIdx.x; k < CC_LABEL_SLOTS; k += CC_THREADS) {
        s_key[k] = 0;
        s_cnt[k] = 0u;
    }
    __syncthreads();
    const int lane = (int)lane_id();
    for (int j = 0; j < CC_LABEL_PER / CC_THREADS; j++) {
        const unsigned long long i = (unsigned long long)blockIdx.x * CC_LABEL_PER + (unsigned)j * CC_THREADS + threadIdx.x;
        int id = 0;
        if (i < n_vox) {
            const int r = p[i];
            id = r < 0 ? 0 : lab[r];
            lab[i] = id;
        }
        unsigned long long todo = __ballot(id > 0);
        while (todo) {      // one round per id the wavefront holds
            const int src = __ffsll((long long)todo) - 1;
            const int first = __shfl(id, src);
            const unsigned long long same = __ballot(id == first);
            if (lane == src) {
                const unsigned c = (unsigned)__popcll(same);
                const int h = first & (CC_LABEL_SLOTS - 1);
                const int held = atomicCAS(s_key + h, 0, first);
                if (held == 0 || held == first) atomicAdd(s_cnt + h, c);      // (at most CC_LABEL_PER in all: no overflow)
                else atomicAdd(size_tab + (first - 1), (unsigned long long)c);
            }
            todo &= ~same;
        }
    }
    __syncthreads();
    for (int k = (int)threadIdx.x; k < CC_LABEL_SLOTS; k += CC_THREADS)
        if (s_key[k] > 0) atomicAdd(size_tab + (s_key[k] - 1), (unsigned long long)s_cnt[k]);
}

// g[i] = fill where i is foreground (lab[i] > 0) and its component is not kept; every other voxel keeps its bits.
__global__ __launch_bounds__(CC_THREADS) void k_cc_select(float *__restrict__ g, const int *__restrict__ lab, const int *__restrict__ flag,
                                                          float fill, unsigned n_vox) {
    const unsigned i = blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n_vox) return;
    const int id = lab[i];
    if (id > 0 && !flag[id - 1]) g[i] = fill;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

struct CcDevice {
    float *g = nullptr;      // the grid
    int *lab = nullptr;      // labels
    long long *root = nullptr;
    unsigned long long *size = nullptr;
    int *flag = nullptr;     // room for one int per component
    int n = 0;
};

template <int CONN>
static void cc_launch_forest(mad_ctx *ctx, const CcPlan &P, const float *d_g, double thr, int *d_p, int *d_ctl) {
    const CcDims D = {{P.n[0], P.n[1], P.n[2]}};
    mad_timer_begin(ctx, MAD_T_CC_TILE);
    hipLaunchKernelGGL((k_cc_tile<CONN>), dim3(P.tiles), dim3(CC_THREADS), 0, ctx->stream, d_g, D, thr, P.by, P.bz, d_p, d_ctl);
    mad_timer_end(ctx, MAD_T_CC_TILE);
    mad_timer_begin(ctx, MAD_T_CC_BORDER);
    hipLaunchKernelGGL((k_cc_border<CONN>), dim3(P.tiles, CC_BORDER_Y), dim3(CC_THREADS), 0, ctx->stream, D, P.by, P.bz, d_p);
    mad_timer_end(ctx, MAD_T_CC_BORDER);
}

// The grid to the device, the forest, the jumping, ids, labels, root and size tables: all left on the device (S_TMP_H: grid, S_TMP_D:
// labels, S_TMP_I: tables).  MAD_EDOM before anything is copied back.
static int cc_label(mad_ctx *ctx, const char *who, const float *grid, const CcPlan &P, double thr, CcDevice &R) {
    const size_t n_vox_z = P.n_vox;
    const unsigned n_vox = P.n_vox;
    const int n_blocks = (int)mad_ceil_div(n_vox, SG_SCAN_PER);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), n_vox_z * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), n_vox_z * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), n_vox_z * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), 64));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), 2 * ((size_t)n_blocks + 1) * 4));
    float *d_g = scratch<float>(ctx, S_TMP_H);
    int *d_p = scratch<int>(ctx, S_TMP_C), *d_lab = scratch<int>(ctx, S_TMP_D);
    int *d_ctl = scratch<int>(ctx, S_TMP_G);      // [0] a voxel is not finite, [1] a jumping pass stored
    int *d_cnt = scratch<int>(ctx, S_TMP_F), *d_off = d_cnt + n_blocks + 1;

    MAD_HIP(hipMemcpyAsync(d_g, grid, n_vox_z * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemsetAsync(d_ctl, 0, 64, ctx->stream));
    if (P.conn == 6) cc_launch_forest<6>(ctx, P, d_g, thr, d_p, d_ctl);
    else if (P.conn == 18) cc_launch_forest<18>(ctx, P, d_g, thr, d_p, d_ctl);
    else cc_launch_forest<26>(ctx, P, d_g, thr, d_p, d_ctl);
    MAD_HIP(hipGetLastError());
    const unsigned nb = (unsigned)mad_ceil_div(n_vox, SG_THREADS);
    for (;;) {      // a pass takes every pointer that is not at its root at least one ancestor up: the passes end
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

    // the component tables: [root int64 n][size uint64 n][peak float32 n (k_seg_assign's, not used)][flag int32 n]
    const size_t n8 = ((size_t)n + 1) * 8, n4 = (((size_t)n + 1) * 4 + 7) & ~(size_t)7;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), 2 * n8 + 2 * n4));
    char *tab = scratch<char>(ctx, S_TMP_I);
    R.g = d_g;
    R.lab = d_lab;
    R.root = (long long *)tab;
    R.size = (unsigned long long *)(tab + n8);
    float *d_peak = (float *)(tab + 2 * n8);
    R.flag = (int *)(tab + 2 * n8 + n4);
    R.n = n;
    MAD_HIP(hipMemsetAsync(R.size, 0, n8, ctx->stream));
    mad_timer_begin(ctx, MAD_T_SEG_SCAN);
    hipLaunchKernelGGL(k_seg_assign, dim3(n_blocks), dim3(SG_THREADS), 0, ctx->stream, (const int *)d_p, (const float *)d_g, n_vox, (const int *)d_off,
                       d_lab, R.root, d_peak);
    mad_timer_end(ctx, MAD_T_SEG_SCAN);
    mad_timer_begin(ctx, MAD_T_CC_LABEL);
    hipLaunchKernelGGL(k_cc_label, dim3((unsigned)mad_ceil_div(n_vox, CC_LABEL_PER)), dim3(CC_THREADS), 0, ctx->stream, (const int *)d_p, d_lab, n_vox, R.size);
    mad_timer_end(ctx, MAD_T_CC_LABEL);
    MAD_HIP(hipGetLastError());
    return MAD_OK;
}

extern "C" int mad_map_components(mad_ctx *ctx, const float *grid, const int32_t dims[3], double threshold, int32_t connectivity,
                                  int32_t *labels, int64_t *root, int64_t *size, int64_t cap, int64_t *n_components) {
    const char *who = "mad_map_components";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !labels || !n_components) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    CcPlan P;
    char msg[320];
    if (cc_plan(who, dims, threshold, connectivity, P, msg, sizeof msg) != CC_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    if (cap < 0) return mad_fail(ctx, MAD_EINVAL, "%s: capacity %lld", who, (long long)cap);
    CcDevice R;
    MAD_TRY(cc_label(ctx, who, grid, P, threshold, R));
    MAD_HIP(hipMemcpyAsync(labels, R.lab, (size_t)P.n_vox * 4, hipMemcpyDeviceToHost, ctx->stream));
    const bool fits = (int64_t)R.n <= cap;
    if (fits && R.n > 0) {
        if (root) MAD_HIP(hipMemcpyAsync(root, R.root, (size_t)R.n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (size) MAD_HIP(hipMemcpyAsync(size, R.size, (size_t)R.n * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    *n_components = R.n;
    if (!fits) return mad_fail(ctx, MAD_ENOSPC, "%s: %d components, capacity %lld", who, R.n, (long long)cap);
    return MAD_OK;
}

extern "C" int mad_map_dust(mad_ctx *ctx, const float *grid, const int32_t dims[3], double threshold, int32_t connectivity,
                            int64_t min_size, int64_t keep, float fill, float *out, int64_t counts[4]) {
    const char *who = "mad_map_dust";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    CcPlan P;
    char msg[320];
    if (cc_plan(who, dims, threshold, connectivity, P, msg, sizeof msg) != CC_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    if (cc_dust_args(who, threshold, min_size, keep, fill, msg, sizeof msg) != CC_OK) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    CcDevice R;
    MAD_TRY(cc_label(ctx, who, grid, P, threshold, R));
    // the ranking of the n sizes on the host
    const size_t n = (size_t)R.n;
    std::vector<int64_t> h_root(n), h_size(n);
    std::vector<int32_t> h_flag;
    int64_t c[4] = {0, 0, 0, 0};
    if (n > 0) {
        MAD_HIP(hipMemcpyAsync(h_root.data(), R.root, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipMemcpyAsync(h_size.data(), R.size, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));
    }
    cc_select((int64_t)n, h_root.data(), h_size.data(), min_size, keep, h_flag, c);
    if (c[1] < c[0]) {      // something is dropped
        MAD_HIP(hipMemcpyAsync(R.flag, h_flag.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
        mad_timer_begin(ctx, MAD_T_CC_SELECT);
        hipLaunchKernelGGL(k_cc_select, dim3((unsigned)mad_ceil_div(P.n_vox, CC_THREADS)), dim3(CC_THREADS), 0, ctx->stream, R.g, (const int *)R.lab,
                           (const int *)R.flag, fill, P.n_vox);
        mad_timer_end(ctx, MAD_T_CC_SELECT);
        MAD_HIP(hipGetLastError());
    }
    MAD_HIP(hipMemcpyAsync(out, R.g, (size_t)P.n_vox * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (counts)
        for (int k = 0; k < 4; k++) counts[k] = c[k];
    return MAD_OK;
}
