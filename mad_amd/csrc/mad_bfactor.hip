// mad_bfactor.hip -- a model's density with a Gaussian width per atom, and the B-factors of a placed model refined against the map
// (restated in mad_amd/bfactor.py), for gfx950.
//
//   mad_model_density_b   k_bf_gather        a workgroup per brick of 8 x 8 x 8 voxels of the box; the atoms of the cells in reach of it
//                                            go through LDS a chunk at a time, and every lane adds, in float64, the atoms that reach its
//                                            voxels: cells ascending, atoms ascending within a cell, whatever the chunk and the threads
//   mad_bfactor_refine    per cycle, queued without a look from the host:
//                         k_bf_gather        rho at the present B into the float64 box
//                         k_bf_sums0 / k_bf_tree   <D, rho>, <rho, rho>, <D, D> over the box in fourier.tree_sum's pairing, a level a launch
//                         k_bf_grad          a wave per atom walks the voxels of its reach, lanes strided over them, one butterfly
//                         k_bf_step          one workgroup: the groups' sums (atoms ascending), the largest, the move, the batch's
//                                            bookkeeping, and the flag `done` that every later launch reads first
// The slots of a chunk are ranks from a prefix sum over contiguous runs of the sorted atoms, not the order of an atomic: the order of a
// voxel's sum is a property of the inputs.  No floating-point atomic anywhere.
#include <algorithm>
#include <cstring>
#include <vector>

#include "mad_common.h"
#include "mad_bfactor_plan.h"

struct BfGeo {
    int n[3];                      // the lattice
    double o[3], vs;
    int blo[3], bdim[3];           // the box
    long long voxels;
    double v0, K, two_pi, rmax;
    double glo[3], edge;           // the cell grid
    int cdim[3];
    int bricks[3];
};

struct BfState {
    double tot[3];                 // <D, rho>, <rho, rho>, <D, D> of the present cycle
    double lossv;                  // <r, r> where it was asked for
    double step, scale0, cc0, loss0, scale, cc, loss;
    int done, converged, last, batch, err;
};

struct BfArgs {
    BfGeo G;
    const float *D;                // the lattice
    double *rho;                   // the box
    int n_atoms, n_groups;
    const double *x, *mass;
    const int *group;              // per atom its group (NULL: b is per atom)
    double *b, *b_prev, *gg;       // per group
    double *ga;                    // per atom
    const long long *first;        // n_groups + 1
    const unsigned char *fixed;    // nullable
    const int *order, *start;
    int chunk;
    double *part_a, *part_b;
    BfState *S;
    double b_min, b_max, min_step;
};

__device__ __forceinline__ double bf_b_of(const BfArgs &A, int a) { return A.b[A.group ? A.group[a] : a]; }

// ---------------------------------------------------------------------------
// the gather
// ---------------------------------------------------------------------------
#define BF_NV 8      // voxels of a lane at most (64 threads)

__device__ __forceinline__ void bf_add_chunk(const double *s_at, int staged, const double px[BF_NV], const double py[BF_NV], const double pz[BF_NV],
                                             unsigned valid, double acc[BF_NV]) {
#pragma unroll
    for (int k = 0; k < BF_NV; k++) {
        if (!((valid >> k) & 1u)) continue;
        double sum = acc[k];
        for (int a = 0; a < staged; a++) {      // every lane reads the same address: a broadcast
            const double *q = s_at + BF_STAGE * a;
            const double dx = px[k] - q[0], dy = py[k] - q[1], dz = pz[k] - q[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= q[3]) sum = sum + q[5] * exp(-(d2 / q[4]));
        }
        acc[k] = sum;
    }
}

__global__ __launch_bounds__(BF_MAX_THREADS) void k_bf_gather(BfArgs A, int force) {
    extern __shared__ double s_at[];      // A.chunk x BF_STAGE
    __shared__ int s_scan[BF_MAX_THREADS / MAD_WAVE + 1];
    if (!force && A.S->done) return;
    const BfGeo &G = A.G;
    const int tid = threadIdx.x, T = blockDim.x;
    const int bz = blockIdx.x % G.bricks[2], bt = blockIdx.x / G.bricks[2], by = bt % G.bricks[1], bx = bt / G.bricks[1];
    const int j0[3] = {bx * BF_BRICK, by * BF_BRICK, bz * BF_BRICK};      // in the box
    double px[BF_NV], py[BF_NV], pz[BF_NV], acc[BF_NV];
    long long at[BF_NV];
    unsigned valid = 0;
#pragma unroll
    for (int k = 0; k < BF_NV; k++) {
        const int q = k * T + tid;
        const int jx = j0[0] + (q >> 6), jy = j0[1] + ((q >> 3) & 7), jz = j0[2] + (q & 7);
        acc[k] = 0.0;
        px[k] = G.o[0] + G.vs * (double)(G.blo[0] + jx);
        py[k] = G.o[1] + G.vs * (double)(G.blo[1] + jy);
        pz[k] = G.o[2] + G.vs * (double)(G.blo[2] + jz);
        at[k] = ((long long)jx * G.bdim[1] + jy) * G.bdim[2] + jz;
        if (q < BF_BRICK_VOXELS && jx < G.bdim[0] && jy < G.bdim[1] && jz < G.bdim[2]) valid |= 1u << k;
    }
    int c0[3], c1[3];
    double bl[3], bh[3];      // the brick's first and last voxel
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int last = min(j0[d] + BF_BRICK - 1, G.bdim[d] - 1);
        bf_cell_range(G.o[d], G.vs, G.blo[d] + j0[d], G.blo[d] + last, G.rmax, G.glo[d], G.edge, G.cdim[d], c0[d], c1[d]);
        bl[d] = G.o[d] + G.vs * (double)(G.blo[d] + j0[d]);
        bh[d] = G.o[d] + G.vs * (double)(G.blo[d] + last);
    }
    // Along z the cells in reach are one contiguous run of the sorted atoms per (cx, cy).  The workgroup walks the runs `batch` atoms at
    // a time; an atom whose distance to the brick's box exceeds its own reach adds to none of the brick's voxels (zone_box_d2 is <= every
    // voxel's d2, rounding included) and is dropped; the others take the next slots in the order of the run, by an exclusive scan of
    // the keep flags, and a chunk is worked off when the next batch might not fit.
    const int batch = min(T, A.chunk);
    int staged = 0;
    for (int cx = c0[0]; cx <= c1[0]; cx++)
        for (int cy = c0[1]; cy <= c1[1]; cy++) {
            const int row = (cx * G.cdim[1] + cy) * G.cdim[2];
            const int a1 = A.start[row + c1[2] + 1];
            for (int base = A.start[row + c0[2]]; base < a1; base += batch) {
                if (staged + batch > A.chunk) {      // the same in every thread
                    __syncthreads();
                    bf_add_chunk(s_at, staged, px, py, pz, valid, acc);
                    __syncthreads();
                    staged = 0;
                }
                int keep = 0;
                double x[3] = {0.0, 0.0, 0.0}, v = 1.0, m = 0.0;
                if (tid < batch && base + tid < a1) {
                    const int a = A.order[base + tid];
                    x[0] = A.x[3 * a]; x[1] = A.x[3 * a + 1]; x[2] = A.x[3 * a + 2];
                    v = G.v0 + bf_b_of(A, a) / G.K;
                    m = A.mass[a];
                    keep = zone_box_d2(x, bl, bh) <= 9.0 * v ? 1 : 0;
                }
                int total;
                const int slot = staged + block_excl_scan(keep, s_scan, &total);      // at most staged + batch <= A.chunk
                if (keep) {
                    const double t = G.two_pi * v;
                    double *q = s_at + BF_STAGE * slot;
                    q[0] = x[0]; q[1] = x[1]; q[2] = x[2];
                    q[3] = 9.0 * v; q[4] = 2.0 * v; q[5] = m / (t * sqrt(t));
                }
                staged += total;
            }
        }
    __syncthreads();
    bf_add_chunk(s_at, staged, px, py, pz, valid, acc);
#pragma unroll
    for (int k = 0; k < BF_NV; k++)
        if ((valid >> k) & 1u) A.rho[at[k]] = acc[k];
}

// ---------------------------------------------------------------------------
// the sums: fourier.tree_sum's pairing over the box, voxels counted z fastest
// ---------------------------------------------------------------------------
// s[c][0] <- the sum of s[c][0 .. 255] by halving, c < C: x[:128] + x[128:], then 64, ... 1
template <int C>
__device__ __forceinline__ void bf_run(double (*s)[BF_RUN]) {
    __syncthreads();
    for (int h = BF_RUN / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int c = 0; c < C; c++) s[c][threadIdx.x] = s[c][threadIdx.x] + s[c][threadIdx.x + h];
        __syncthreads();
    }
}

__device__ __forceinline__ size_t bf_lattice_index(const BfGeo &G, long long i) {
    const int jz = (int)(i % G.bdim[2]);
    const long long t = i / G.bdim[2];
    const int jy = (int)(t % G.bdim[1]), jx = (int)(t / G.bdim[1]);
    return ((size_t)(G.blo[0] + jx) * G.n[1] + (G.blo[1] + jy)) * (size_t)G.n[2] + (G.blo[2] + jz);
}

// level 0.  loss == 0: out[c * stride + run] = the run's sums of D rho, rho rho, D D;  loss == 1: of r r alone, r = s rho - D
__global__ __launch_bounds__(BF_RUN) void k_bf_sums0(BfArgs A, int loss, int force, double *out, long long stride) {
    __shared__ double s[3][BF_RUN];
    if (!force && A.S->done) return;
    const long long i = (long long)blockIdx.x * BF_RUN + threadIdx.x;
    double d = 0.0, r = 0.0;
    if (i < A.G.voxels) {
        d = (double)A.D[bf_lattice_index(A.G, i)];
        r = A.rho[i];
    }
    if (loss) {
        const double sc = A.S->tot[0] / A.S->tot[1], e = i < A.G.voxels ? sc * r - d : 0.0;
        s[0][threadIdx.x] = e * e;
        bf_run<1>(s);
        if (threadIdx.x == 0) out[blockIdx.x] = s[0][0];
    } else {
        s[0][threadIdx.x] = d * r; s[1][threadIdx.x] = r * r; s[2][threadIdx.x] = d * d;
        bf_run<3>(s);
        if (threadIdx.x < 3) out[threadIdx.x * stride + blockIdx.x] = s[threadIdx.x][0];
    }
}

// one more level: out[c * out_stride + b] = the sum of run b of in[c * in_stride + 0 .. n_in) (the last run zero-padded)
__global__ __launch_bounds__(BF_RUN) void k_bf_tree(const BfState *S, int force, const double *in, long long n_in, long long in_stride, double *out,
                                                    long long out_stride, int ncomp) {
    __shared__ double s[3][BF_RUN];
    if (!force && S->done) return;
    const long long i = (long long)blockIdx.x * BF_RUN + threadIdx.x;
    for (int c = 0; c < 3; c++) s[c][threadIdx.x] = (c < ncomp && i < n_in) ? in[c * in_stride + i] : 0.0;
    bf_run<3>(s);
    if ((int)threadIdx.x < ncomp) out[threadIdx.x * out_stride + blockIdx.x] = s[threadIdx.x][0];
}

// what the host asks for at the first cycle and after the last: 0: scale0, cc0 (and the refusal of <rho, rho> == 0); 1: loss0;
// 2: scale, cc; 3: loss
__global__ void k_bf_note(BfState *S, int which, int force) {
    if (!force && S->done) return;
    const double dr = S->tot[0], rr = S->tot[1], dd = S->tot[2];
    if (which == 0) {
        if (rr == 0.0) { S->err = 1; S->done = 1; return; }
        S->scale0 = dr / rr; S->cc0 = dr / sqrt(dd * rr);
    } else if (which == 1) S->loss0 = S->lossv;
    else if (which == 2) { S->scale = dr / rr; S->cc = dr / sqrt(dd * rr); }
    else S->loss = S->lossv;
}

// ---------------------------------------------------------------------------
// the gradient: g_a = (s sum_p (r(p) e_a(p)) (d2 / (2 v v) - 1.5 / v)) / K over the voxels atom a reaches
// ---------------------------------------------------------------------------
#define BF_GRAD_THREADS 256

__device__ __forceinline__ int bf_clamp_q(double q, int lo, int hi) { return q < (double)lo ? lo : (q > (double)hi ? hi : (int)q); }

__global__ __launch_bounds__(BF_GRAD_THREADS) void k_bf_grad(BfArgs A) {
    if (A.S->done) return;
    const BfGeo &G = A.G;
    const int a = blockIdx.x * (BF_GRAD_THREADS / MAD_WAVE) + (threadIdx.x >> 6), lane = lane_id();
    if (a >= A.n_atoms) return;      // the whole wave
    const double sc = A.S->tot[0] / A.S->tot[1];
    const double v = G.v0 + bf_b_of(A, a) / G.K, reach = 3.0 * sqrt(v), nine_v = 9.0 * v, two_v = 2.0 * v, t = G.two_pi * v;
    const double coef = A.mass[a] / (t * sqrt(t)), w1 = 2.0 * (v * v), w2 = 1.5 / v;
    const double x[3] = {A.x[3 * a], A.x[3 * a + 1], A.x[3 * a + 2]};
    int lo[3], ext[3];
    bool none = false;
#pragma unroll
    for (int d = 0; d < 3; d++) {      // a voxel more on either side than the reach: the test below decides
        const double ql = floor((x[d] - reach - G.o[d]) / G.vs), qh = ceil((x[d] + reach - G.o[d]) / G.vs);
        const int first = G.blo[d], last = G.blo[d] + G.bdim[d] - 1;
        if (!(qh >= (double)first) || !(ql <= (double)last)) none = true;
        lo[d] = bf_clamp_q(ql, first, last);
        ext[d] = bf_clamp_q(qh, first, last) - lo[d] + 1;
    }
    const long long count = none ? 0 : (long long)ext[0] * ext[1] * ext[2];
    double acc = 0.0;
    for (long long k = lane; k < count; k += MAD_WAVE) {
        const long long kt = k / ext[2];
        const int jz = lo[2] + (int)(k % ext[2]), jy = lo[1] + (int)(kt % ext[1]), jx = lo[0] + (int)(kt / ext[1]);
        const double dx = (G.o[0] + G.vs * (double)jx) - x[0], dy = (G.o[1] + G.vs * (double)jy) - x[1], dz = (G.o[2] + G.vs * (double)jz) - x[2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= nine_v) {
            const double e = coef * exp(-(d2 / two_v));
            const size_t bi = ((size_t)(jx - G.blo[0]) * G.bdim[1] + (jy - G.blo[1])) * (size_t)G.bdim[2] + (jz - G.blo[2]);
            const double r = sc * A.rho[bi] - (double)A.D[((size_t)jx * G.n[1] + jy) * (size_t)G.n[2] + jz];
            acc = acc + (r * e) * (d2 / w1 - w2);
        }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) A.ga[a] = (sc * acc) / G.K;
}

// ---------------------------------------------------------------------------
// the step: one workgroup
// ---------------------------------------------------------------------------
#define BF_STEP_THREADS 256

// the largest v of the workgroup, in every thread; *flag counts the threads that raised `bad`
__device__ __forceinline__ double bf_block_max(double v, bool bad, double *s_red, int *s_flag, bool &any_bad) {
    v = wave_max_f64(v);
    if (threadIdx.x == 0) *s_flag = 0;
    __syncthreads();
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = v;
    if (bad) *s_flag = 1;
    __syncthreads();
    double m = s_red[0];
    for (int k = 1; k < BF_STEP_THREADS / MAD_WAVE; k++) m = fmax(m, s_red[k]);
    any_bad = *s_flag != 0;
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(BF_STEP_THREADS) void k_bf_step(BfArgs A, int cycle) {
    __shared__ double s_red[BF_STEP_THREADS / MAD_WAVE];
    __shared__ int s_flag;
    BfState *S = A.S;
    if (S->done) return;
    const int tid = threadIdx.x;
    // a group's gradient: its atoms' in ascending order
    double lm = 0.0;
    bool bad = false;
    for (int g = tid; g < A.n_groups; g += BF_STEP_THREADS) {
        double sum = 0.0;
        for (long long a = A.first[g]; a < A.first[g + 1]; a++) sum = sum + A.ga[a];
        A.gg[g] = sum;
        if (sum != sum) bad = true;
        else if (!(A.fixed && A.fixed[g])) lm = fmax(lm, fabs(sum));
    }
    bool any_bad;
    const double mx = bf_block_max(lm, bad, s_red, &s_flag, any_bad);
    const double step = S->step;
    const int batch = S->batch + 1;
    __syncthreads();      // everybody has read the state
    if (any_bad || mx == 0.0) {
        if (tid == 0) { S->done = 1; S->converged = any_bad ? 0 : 1; S->last = cycle; }
        return;
    }
    double ld = 0.0;
    for (int g = tid; g < A.n_groups; g += BF_STEP_THREADS) {
        if (A.fixed && A.fixed[g]) continue;
        double b = A.b[g] - step * (A.gg[g] / mx);
        b = b < A.b_min ? A.b_min : b;
        b = b > A.b_max ? A.b_max : b;
        A.b[g] = b;
        if (batch == BF_BATCH) {
            ld = fmax(ld, fabs(b - A.b_prev[g]));
            A.b_prev[g] = b;
        }
    }
    double next = step;
    if (batch == BF_BATCH) {
        const double moved = bf_block_max(ld, false, s_red, &s_flag, any_bad);
        if (moved < step) next = step * 0.5;
    }
    if (tid == 0) {
        S->step = next;
        S->batch = batch == BF_BATCH ? 0 : batch;
        if (next < A.min_step) { S->done = 1; S->converged = 1; S->last = cycle; }
    }
}

// ---------------------------------------------------------------------------
// the host
// ---------------------------------------------------------------------------
static inline size_t bf_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct BfCall {
    BfArgs A;
    BfBox box;
    BfCells cells;
    BfPlan plan;
};

// Everything both entry points share: the box, the cell grid, the plan, the scratch and the uploads.  n_b values of b (per group, or per
// atom when group is NULL).
static int bf_prepare(mad_ctx *ctx, const char *who, const float *grid, const int32_t dims[3], const double origin[3], double voxsp, int64_t n_atoms,
                      const double *coords, const double *masses, double resolution, double b_max, int64_t n_groups, const int64_t *first_atom,
                      const double *b, const uint8_t *fixed, int32_t cycles, BfCall &c) {
    const size_t n = (size_t)n_atoms, ng = (size_t)n_groups;
    std::vector<uint8_t> keep;
    bf_box(dims, origin, voxsp, n_atoms, coords, resolution, b_max, c.box, keep);
    if (c.box.kept == 0) return mad_fail(ctx, MAD_EDOM, "%s: coords: no atom reaches the lattice (reach %g A at b_max = %g)", who, c.box.rmax, b_max);
    bf_cells(n_atoms, coords, keep, c.box.kept, c.box.rmax, c.cells);
    c.plan = bf_plan(c.box, ctx->bf_chunk, ctx->bf_threads);
    if (c.plan.runs[c.plan.levels - 1] != 1 || c.plan.n_bricks > 0x7fffffffLL) return mad_fail(ctx, MAD_EINVAL, "%s: a box of %lld voxels", who, (long long)c.box.voxels);
    for (int d = 0; d < 3; d++) { ctx->last_bf[d] = c.box.lo[d]; ctx->last_bf[3 + d] = c.box.dim[d]; ctx->last_bf[6 + d] = c.plan.bricks[d]; ctx->last_bf[9 + d] = c.cells.g.dim[d]; }
    ctx->last_bf[12] = c.plan.chunk; ctx->last_bf[13] = c.plan.threads; ctx->last_bf[14] = cycles;
    ctx->last_bf_kept = c.box.kept;

    const size_t lattice = (size_t)dims[0] * dims[1] * dims[2], voxels = (size_t)c.box.voxels, cells = (size_t)c.cells.g.cells, kept = (size_t)c.box.kept;
    const size_t o_mass = bf_up(n * 24), o_ga = o_mass + bf_up(n * 8), o_group = o_ga + bf_up(n * 8);
    const size_t o_prev = bf_up(ng * 8), o_gg = 2 * o_prev, o_first = 3 * o_prev, o_fixed = o_first + bf_up((ng + 1) * 8);
    const size_t runs0 = (size_t)c.plan.runs[0], runs1 = c.plan.levels > 1 ? (size_t)c.plan.runs[1] : 1;
    if (grid) MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), lattice * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), voxels * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), o_group + n * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), bf_up(kept * 4) + (cells + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), o_fixed + ng));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), bf_up(3 * runs0 * 8) + 3 * runs1 * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), sizeof(BfState)));

    BfArgs &A = c.A;
    memset(&A, 0, sizeof A);
    BfGeo &G = A.G;
    for (int d = 0; d < 3; d++) {
        G.n[d] = dims[d]; G.o[d] = origin[d]; G.blo[d] = c.box.lo[d]; G.bdim[d] = c.box.dim[d];
        G.glo[d] = c.cells.g.lo[d]; G.cdim[d] = c.cells.g.dim[d]; G.bricks[d] = c.plan.bricks[d];
    }
    G.vs = voxsp; G.voxels = c.box.voxels; G.v0 = bf_v0(resolution); G.K = bf_K(); G.two_pi = 2.0 * M_PI; G.rmax = c.box.rmax; G.edge = c.cells.g.edge;
    A.D = grid ? scratch<float>(ctx, S_TMP_A) : nullptr;
    A.rho = scratch<double>(ctx, S_TMP_B);
    A.n_atoms = (int)n; A.n_groups = (int)ng;
    char *at = scratch<char>(ctx, S_TMP_C), *gr = scratch<char>(ctx, S_TMP_E), *cl = scratch<char>(ctx, S_TMP_D), *pt = scratch<char>(ctx, S_TMP_F);
    A.x = (const double *)at; A.mass = (const double *)(at + o_mass); A.ga = (double *)(at + o_ga);
    A.group = first_atom ? (const int *)(at + o_group) : nullptr;
    A.b = (double *)gr; A.b_prev = (double *)(gr + o_prev); A.gg = (double *)(gr + o_gg);
    A.first = (const long long *)(gr + o_first);
    A.fixed = fixed ? (const unsigned char *)(gr + o_fixed) : nullptr;
    A.order = (const int *)cl; A.start = (const int *)(cl + bf_up(kept * 4));
    A.chunk = c.plan.chunk;
    A.part_a = (double *)pt; A.part_b = (double *)(pt + bf_up(3 * runs0 * 8));
    A.S = scratch<BfState>(ctx, S_TMP_G);

    std::vector<int32_t> group;
    if (first_atom) {
        group.resize(n);
        for (size_t g = 0; g < ng; g++)
            for (int64_t a = first_atom[g]; a < first_atom[g + 1]; a++) group[(size_t)a] = (int32_t)g;
    }
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // nothing of an earlier call still reads the scratch that is rewritten below
    if (grid) MAD_HIP(hipMemcpyAsync((void *)A.D, grid, lattice * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync((void *)A.x, coords, n * 24, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync((void *)A.mass, masses, n * 8, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(A.b, b, ng * 8, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(A.b_prev, b, ng * 8, hipMemcpyHostToDevice, ctx->stream));
    if (first_atom) {
        MAD_HIP(hipMemcpyAsync((void *)A.group, group.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)A.first, first_atom, (ng + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    if (fixed) MAD_HIP(hipMemcpyAsync((void *)A.fixed, fixed, ng, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync((void *)A.order, c.cells.order.data(), kept * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync((void *)A.start, c.cells.start.data(), (cells + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemsetAsync(A.S, 0, sizeof(BfState), ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // the host vectors above end with this function
    return MAD_OK;
}

static void bf_launch_gather(mad_ctx *ctx, const BfCall &c, int force) {
    mad_timer_begin(ctx, MAD_T_BF_GATHER);
    hipLaunchKernelGGL(k_bf_gather, dim3((unsigned)c.plan.n_bricks), dim3(c.plan.threads), (size_t)c.plan.chunk * BF_STAGE * 8, ctx->stream, c.A, force);
    mad_timer_end(ctx, MAD_T_BF_GATHER);
}

// the levels of one sum over the box: the three products into S->tot, or <r, r> into S->lossv
static void bf_launch_sums(mad_ctx *ctx, const BfCall &c, int loss, int force) {
    const BfArgs &A = c.A;
    const int ncomp = loss ? 1 : 3;
    double *total = loss ? &A.S->lossv : A.S->tot;
    double *bufs[2] = {A.part_a, A.part_b};
    mad_timer_begin(ctx, MAD_T_BF_SUMS);
    const bool only = c.plan.levels == 1;
    hipLaunchKernelGGL(k_bf_sums0, dim3((unsigned)c.plan.runs[0]), dim3(BF_RUN), 0, ctx->stream, A, loss, force, only ? total : bufs[0], only ? 1LL : (long long)c.plan.runs[0]);
    for (int l = 1; l < c.plan.levels; l++) {
        const bool last = l == c.plan.levels - 1;
        hipLaunchKernelGGL(k_bf_tree, dim3((unsigned)c.plan.runs[l]), dim3(BF_RUN), 0, ctx->stream, (const BfState *)A.S, force, (const double *)bufs[(l - 1) & 1],
                           (long long)c.plan.runs[l - 1], (long long)c.plan.runs[l - 1], last ? total : bufs[l & 1], last ? 1LL : (long long)c.plan.runs[l], ncomp);
    }
    mad_timer_end(ctx, MAD_T_BF_SUMS);
}

// the box of the device into the float64 lattice `out` (zero elsewhere)
static int bf_download_box(mad_ctx *ctx, const BfCall &c, const int32_t dims[3], double *out) {
    std::vector<double> host((size_t)c.box.voxels);
    MAD_HIP(hipMemcpyAsync(host.data(), c.A.rho, host.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    memset(out, 0, (size_t)dims[0] * dims[1] * dims[2] * 8);
    for (int x = 0; x < c.box.dim[0]; x++)
        for (int y = 0; y < c.box.dim[1]; y++)
            memcpy(out + ((size_t)(c.box.lo[0] + x) * dims[1] + (c.box.lo[1] + y)) * (size_t)dims[2] + c.box.lo[2],
                   host.data() + ((size_t)x * c.box.dim[1] + y) * (size_t)c.box.dim[2], (size_t)c.box.dim[2] * 8);
    return MAD_OK;
}

extern "C" int mad_model_density_b(mad_ctx *ctx, const int32_t dims[3], const double origin[3], double voxsp, int64_t n_atoms, const double *coords,
                                   const double *masses, const double *b_atom, double resolution, double b_max, double *rho, int32_t box[6]) {
    if (!ctx) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    const char *who = "mad_model_density_b";
    if (!rho) return mad_fail(ctx, MAD_EINVAL, "%s: NULL rho", who);
    char msg[256];
    if (!bf_check_lattice(who, dims, origin, voxsp, msg, sizeof msg) || !bf_check_atoms(who, n_atoms, coords, masses, resolution, msg, sizeof msg) ||
        !bf_check_limits(who, 0.0, b_max, msg, sizeof msg) || !bf_check_b(who, "b_atom", n_atoms, b_atom, 0.0, b_max, msg, sizeof msg))
        return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    BfCall c;
    MAD_TRY(bf_prepare(ctx, who, nullptr, dims, origin, voxsp, n_atoms, coords, masses, resolution, b_max, n_atoms, nullptr, b_atom, nullptr, 0, c));
    bf_launch_gather(ctx, c, 1);
    MAD_HIP(hipGetLastError());
    MAD_TRY(bf_download_box(ctx, c, dims, rho));
    if (box)
        for (int d = 0; d < 3; d++) { box[d] = c.box.lo[d]; box[3 + d] = c.box.dim[d]; }
    return MAD_OK;
}

extern "C" int mad_bfactor_refine(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp, int64_t n_atoms,
                                  const double *coords, const double *masses, int64_t n_groups, const int64_t *first_atom, const double *b0,
                                  const uint8_t *fixed, double resolution, double b_min, double b_max, int n_cycles, double max_step, double min_step,
                                  double *b_out, double *stats, int32_t *converged, int32_t *last_cycle, double *rho) {
    if (!ctx) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    const char *who = "mad_bfactor_refine";
    if (!grid || !b_out || !stats || !converged || !last_cycle)
        return mad_fail(ctx, MAD_EINVAL, "%s: NULL %s", who, !grid ? "grid" : !b_out ? "b_out" : !stats ? "stats" : !converged ? "converged" : "last_cycle");
    char msg[256];
    if (!bf_check_lattice(who, dims, origin, voxsp, msg, sizeof msg) || !bf_check_atoms(who, n_atoms, coords, masses, resolution, msg, sizeof msg) ||
        !bf_check_groups(who, n_atoms, n_groups, first_atom, msg, sizeof msg) || !bf_check_limits(who, b_min, b_max, msg, sizeof msg) ||
        !bf_check_b(who, "b0", n_groups, b0, b_min, b_max, msg, sizeof msg) || !bf_check_cycles(who, n_cycles, max_step, min_step, msg, sizeof msg))
        return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    BfCall c;
    MAD_TRY(bf_prepare(ctx, who, grid, dims, origin, voxsp, n_atoms, coords, masses, resolution, b_max, n_groups, first_atom, b0, fixed, n_cycles, c));
    BfArgs &A = c.A;
    A.b_min = b_min; A.b_max = b_max; A.min_step = min_step;
    BfState init;
    memset(&init, 0, sizeof init);
    init.step = max_step; init.last = n_cycles - 1;
    MAD_HIP(hipMemcpyAsync(A.S, &init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    const unsigned grad_blocks = (unsigned)mad_ceil_div(n_atoms, BF_GRAD_THREADS / MAD_WAVE);
    for (int cycle = 0; cycle < n_cycles; cycle++) {
        bf_launch_gather(ctx, c, 0);
        bf_launch_sums(ctx, c, 0, 0);
        if (cycle == 0) {
            hipLaunchKernelGGL(k_bf_note, dim3(1), dim3(1), 0, ctx->stream, A.S, 0, 0);
            bf_launch_sums(ctx, c, 1, 0);
            hipLaunchKernelGGL(k_bf_note, dim3(1), dim3(1), 0, ctx->stream, A.S, 1, 0);
        }
        mad_timer_begin(ctx, MAD_T_BF_GRAD);
        hipLaunchKernelGGL(k_bf_grad, dim3(grad_blocks), dim3(BF_GRAD_THREADS), 0, ctx->stream, A);
        mad_timer_end(ctx, MAD_T_BF_GRAD);
        mad_timer_begin(ctx, MAD_T_BF_STEP);
        hipLaunchKernelGGL(k_bf_step, dim3(1), dim3(BF_STEP_THREADS), 0, ctx->stream, A, cycle);
        mad_timer_end(ctx, MAD_T_BF_STEP);
    }
    // rho, the scale, the correlation and the loss at the B the run ended with, whatever `done` says
    bf_launch_gather(ctx, c, 1);
    bf_launch_sums(ctx, c, 0, 1);
    hipLaunchKernelGGL(k_bf_note, dim3(1), dim3(1), 0, ctx->stream, A.S, 2, 1);
    bf_launch_sums(ctx, c, 1, 1);
    hipLaunchKernelGGL(k_bf_note, dim3(1), dim3(1), 0, ctx->stream, A.S, 3, 1);
    MAD_HIP(hipGetLastError());
    BfState S;
    MAD_HIP(hipMemcpyAsync(&S, A.S, sizeof S, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(b_out, A.b, (size_t)n_groups * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (S.err) return mad_fail(ctx, MAD_EDOM, "%s: <rho, rho> == 0 over the box: the model has no density on the lattice", who);
    stats[0] = S.scale; stats[1] = S.loss0; stats[2] = S.loss; stats[3] = S.cc0; stats[4] = S.cc; stats[5] = S.step; stats[6] = S.scale0;
    *converged = S.converged; *last_cycle = S.last;
    if (rho) MAD_TRY(bf_download_box(ctx, c, dims, rho));
    return MAD_OK;
}

extern "C" int mad_last_bfactor_plan(mad_ctx *ctx, int32_t box[6], int32_t bricks[3], int32_t cells[3], int32_t *chunk, int32_t *threads, int32_t *cycles,
                                     int64_t *kept) {
    if (!ctx) return MAD_EINVAL;
    for (int d = 0; d < 6; d++) if (box) box[d] = ctx->last_bf[d];
    for (int d = 0; d < 3; d++) {
        if (bricks) bricks[d] = ctx->last_bf[6 + d];
        if (cells) cells[d] = ctx->last_bf[9 + d];
    }
    if (chunk) *chunk = ctx->last_bf[12];
    if (threads) *threads = ctx->last_bf[13];
    if (cycles) *cycles = ctx->last_bf[14];
    if (kept) *kept = ctx->last_bf_kept;
    return MAD_OK;
}
