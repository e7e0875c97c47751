// mad_flexfit.hip -- flexible fitting: the atoms of a model climb the map's gradient one by one, held together by an elastic
// network of springs between the atoms that started within a cutoff of each other, for gfx950.
//
//   mad_flex_network   k_fx_cells, k_fx_fill   the atoms into a cell grid over their bounding box (integer atomics, one scan)
//                      k_fx_degree             per atom the neighbours in its 27 cells: the degree (then one scan: first[])
//                      k_fx_rows               the same walk again: the row, sorted ascending by atom index, and its rest lengths
//                      Integers and per-atom float64 only: the same network as flexfit.network_numpy, bit for bit.
//   mad_flex_fit       k_fx_fit                the whole run in ONE launch of persistent workgroups, at most one per compute unit.
//                      Thread t of all T owns atoms t, t + T, ...  A step is: forces of the own atoms (the gather of k_refine and
//                      the spring sum in ascending neighbour order), their largest length to one word by a 64-bit integer atomic
//                      maximum on the bit pattern, a grid barrier, the update of the own atoms, a grid barrier.
// A neighbour's coordinates are written by another compute unit, whose stores never refresh this one's L1: coordinates, the
// words of the maxima and the partial sums of g0 are stored and loaded with 8-byte agent-scope atomics on both sides, never with
// plain accesses, and every barrier is k_refine's hand-off (every storing wave drains its stores, the workgroup meets, one lane
// arrives and polls).  No floating-point atomic anywhere: the same bits every call, on every plan.
// The gather and the barrier are copies of mad_refine.hip's, which is left as it is.
#include <algorithm>
#include <climits>
#include <vector>

#include "mad_common.h"
#include "mad_flexfit_plan.h"

static_assert(FX_MAX_DEGREE == MAD_FLEX_MAX_DEGREE, "mad_flexfit_plan.h and include/mad_amd.h");

// ---------------------------------------------------------------------------
// the network
// ---------------------------------------------------------------------------
struct FxNetArgs {
    int n;
    const double *x;             // n x 3
    double lo[3], edge, c2;      // the grid's corner and edge; cutoff x cutoff
    int dim[3];
    int *cell;                   // per atom
    int *count;                  // per cell (k_fx_cells), then the fill cursor (k_fx_fill)
    const int *start;            // cells + 1
    int *atoms;                  // the atoms cell by cell
    int *deg;                    // per atom
    const int *first;            // n + 1
    int *nbr;
    double *rest;
    int *err;                    // the lowest atom above FX_MAX_DEGREE (INT_MAX: none)
};

__global__ __launch_bounds__(256) void k_fx_cells(FxNetArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const int cx = fx_cell_of(A.x[3 * i], A.lo[0], A.edge, A.dim[0]), cy = fx_cell_of(A.x[3 * i + 1], A.lo[1], A.edge, A.dim[1]),
              cz = fx_cell_of(A.x[3 * i + 2], A.lo[2], A.edge, A.dim[2]);
    const int c = (cx * A.dim[1] + cy) * A.dim[2] + cz;
    A.cell[i] = c;
    atomicAdd(&A.count[c], 1);
}

// (the order inside a cell is that of the atomics; the rows are sorted afterwards)
__global__ __launch_bounds__(256) void k_fx_fill(FxNetArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const int c = A.cell[i];
    const int at = A.start[c] + atomicAdd(&A.count[c], 1);
    if (at < A.start[c + 1]) A.atoms[at] = i;
}

// f(j, d2) for every other atom j of the 27 cells around atom i with d2 = (dx dx + dy dy) + dz dz <= cutoff^2, dx = x_j - x_i
template <class F>
__device__ __forceinline__ void fx_neighbours(const FxNetArgs &A, int i, F &&f) {
    const double x = A.x[3 * i], y = A.x[3 * i + 1], z = A.x[3 * i + 2];
    const int c = A.cell[i];
    const int cz = c % A.dim[2], cy = (c / A.dim[2]) % A.dim[1], cx = c / (A.dim[2] * A.dim[1]);
    for (int ax = max(cx - 1, 0); ax <= min(cx + 1, A.dim[0] - 1); ax++)
        for (int ay = max(cy - 1, 0); ay <= min(cy + 1, A.dim[1] - 1); ay++)
            for (int az = max(cz - 1, 0); az <= min(cz + 1, A.dim[2] - 1); az++) {
                const int cc = (ax * A.dim[1] + ay) * A.dim[2] + az;
                for (int k = A.start[cc]; k < A.start[cc + 1]; k++) {
                    const int j = A.atoms[k];
                    if (j == i) continue;
                    const double dx = A.x[3 * j] - x, dy = A.x[3 * j + 1] - y, dz = A.x[3 * j + 2] - z;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 <= A.c2) f(j, d2);
                }
            }
}

__global__ __launch_bounds__(256) void k_fx_degree(FxNetArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    int deg = 0;
    fx_neighbours(A, i, [&](int, double) { deg++; });
    A.deg[i] = deg;
    if (deg > FX_MAX_DEGREE) atomicMin(A.err, i);
}

// the row of atom i: every neighbour is put where it belongs among those written so far (an insertion sort in the row itself)
__global__ __launch_bounds__(256) void k_fx_rows(FxNetArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const int r0 = A.first[i], cap = A.first[i + 1] - r0;
    int *row = A.nbr + r0;
    double *rest = A.rest + r0;
    int have = 0;
    fx_neighbours(A, i, [&](int j, double d2) {
        if (have >= cap) return;      // (cannot happen: k_fx_degree counted the same pairs)
        int at = have;
        while (at > 0 && row[at - 1] > j) { row[at] = row[at - 1]; rest[at] = rest[at - 1]; at--; }
        row[at] = j; rest[at] = sqrt(d2);
        have++;
    });
}

extern "C" int mad_flex_network(mad_ctx *ctx, int64_t n_atoms, const double *coords, double cutoff, int32_t *first, int64_t cap_springs,
                                int32_t *nbr, double *rest, int64_t *n_springs) {
    if (!ctx) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    const char *who = "mad_flex_network";
    if (!first || !n_springs) return mad_fail(ctx, MAD_EINVAL, "%s: NULL %s", who, !first ? "first" : "n_springs");
    if (cap_springs < 0 || (cap_springs > 0 && (!nbr || !rest))) return mad_fail(ctx, MAD_EINVAL, "%s: NULL %s or cap_springs = %lld", who, !nbr ? "nbr" : "rest", (long long)cap_springs);
    char msg[256];
    FxGrid g;
    if (!fx_check_network_args(who, n_atoms, coords, cutoff, g, msg, sizeof msg)) return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    const int n = (int)n_atoms;
    const size_t cells = (size_t)g.cells;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), (size_t)n * 24));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (size_t)n * 4 + cells * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), (cells + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), (size_t)n * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), (size_t)n * 4 + ((size_t)n + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), 256));
    FxNetArgs A;
    A.n = n;
    A.x = scratch<double>(ctx, S_TMP_E);
    for (int d = 0; d < 3; d++) { A.lo[d] = g.lo[d]; A.dim[d] = g.dim[d]; }
    A.edge = g.edge; A.c2 = cutoff * cutoff;
    A.cell = scratch<int>(ctx, S_TMP_A); A.count = A.cell + n;
    A.start = scratch<int>(ctx, S_TMP_B);
    A.atoms = scratch<int>(ctx, S_TMP_C);
    A.deg = scratch<int>(ctx, S_TMP_F); A.first = A.deg + n;
    A.nbr = nullptr; A.rest = nullptr;
    A.err = scratch<int>(ctx, S_TMP_G);
    const unsigned blocks = (unsigned)mad_ceil_div(n, 256);
    const int none = INT_MAX;
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // nothing of an earlier call still reads the scratch that is rewritten below
    mad_timer_begin(ctx, MAD_T_FLEX_NETWORK);
    MAD_HIP(hipMemcpyAsync((void *)A.x, coords, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(A.err, &none, 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemsetAsync(A.count, 0, cells * 4, ctx->stream));
    hipLaunchKernelGGL(k_fx_cells, dim3(blocks), dim3(256), 0, ctx->stream, A);
    MAD_TRY(mad_scan_i32(ctx, A.count, (int32_t *)A.start, (int64_t)cells));
    MAD_HIP(hipMemsetAsync(A.count, 0, cells * 4, ctx->stream));
    hipLaunchKernelGGL(k_fx_fill, dim3(blocks), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_fx_degree, dim3(blocks), dim3(256), 0, ctx->stream, A);
    MAD_TRY(mad_scan_i32(ctx, A.deg, (int32_t *)A.first, n));
    mad_timer_end(ctx, MAD_T_FLEX_NETWORK);
    MAD_HIP(hipGetLastError());
    int bad = INT_MAX, total = 0;
    MAD_HIP(hipMemcpyAsync(&bad, A.err, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(&total, A.first + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (bad != INT_MAX) {
        int deg = 0;
        MAD_HIP(hipMemcpy(&deg, A.deg + bad, 4, hipMemcpyDeviceToHost));
        return mad_fail(ctx, MAD_EDOM, "%s: atom %d has %d neighbours within cutoff = %g (MAD_FLEX_MAX_DEGREE = %d)", who, bad, deg, cutoff, FX_MAX_DEGREE);
    }
    *n_springs = total;
    if (total > cap_springs) return mad_fail(ctx, MAD_ENOSPC, "%s: %d springs, cap_springs = %lld", who, total, (long long)cap_springs);
    if (total > 0) {
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), (size_t)total * 4));
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (size_t)total * 8));
        A.nbr = scratch<int>(ctx, S_TMP_D); A.rest = scratch<double>(ctx, S_TMP_H);
        mad_timer_begin(ctx, MAD_T_FLEX_NETWORK);
        hipLaunchKernelGGL(k_fx_rows, dim3(blocks), dim3(256), 0, ctx->stream, A);
        mad_timer_end(ctx, MAD_T_FLEX_NETWORK);
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(nbr, A.nbr, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipMemcpyAsync(rest, A.rest, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MAD_HIP(hipMemcpyAsync(first, A.first, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// ---------------------------------------------------------------------------
// the fit
// ---------------------------------------------------------------------------
struct FxOut {
    double step, g0;
    int converged, last_step;
};

// the words the workgroups meet through, each on a 64-byte line of its own
#define FX_W_ARRIVE 0
#define FX_W_FORCE 8       // two slots: the step's largest |F| as the bit pattern of the non-negative double
#define FX_W_MOVE 24       // two slots: the batch's largest displacement, the same way
#define FX_WORDS 40
#define FX_NAN_BITS 0x7ff8000000000000ull      // above the pattern of every finite double and of +inf

struct FxArgs {
    const float4 *grad;
    int nx, ny, nz;
    double o[3], del[3], vs;
    int n;
    double *x;                   // n x 3: the coordinates, updated in place by their owners between the step's two barriers
    double *prv;                 // n x 3: at the last batch boundary (owner only)
    double *F;                   // n x 3: the step's forces (owner only)
    const double *w;             // nullable
    const unsigned char *fixed;  // nullable
    const int *first, *nbr;
    const double *rest;
    double stiffness;
    int n_steps;
    double max_step, min_step;
    unsigned long long *words;   // FX_WORDS, zeroed before the launch
    double *sum_a, *sum_b;       // n and ceil(n / FX_RUN): the levels of g0's sum
    FxOut *out;
};

__device__ __forceinline__ double fx_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void fx_store(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// All workgroups of the launch meet (they are all resident: fx_plan).  Every wave drains its own stores, the workgroup meets, one
// lane arrives on the counter and polls it; 8-byte agent-scope atomics on both sides, as group_reduce of mad_refine.hip.
__device__ __forceinline__ void fx_barrier(const FxArgs &A, unsigned long long &epoch) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (gridDim.x > 1 && threadIdx.x == 0) {
        __hip_atomic_fetch_add(A.words + FX_W_ARRIVE, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long want = (unsigned long long)gridDim.x * (epoch + 1);
        while (__hip_atomic_load(A.words + FX_W_ARRIVE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) __builtin_amdgcn_s_sleep(2);
    }
    epoch++;
    __syncthreads();
}

// the workgroup's maximum of v (a thread with `nan` set makes it a NaN) added to the word by an integer atomic maximum
__device__ __forceinline__ void fx_publish_max(double v, bool nan, unsigned long long *word, double *s_red, int *s_flag) {
    v = wave_max_f64(v);
    if (threadIdx.x == 0) *s_flag = 0;
    __syncthreads();
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = v;
    if (nan) *s_flag = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = s_red[0];
        for (int k = 1; k < (int)(blockDim.x >> 6); k++) a = fmax(a, s_red[k]);
        const unsigned long long bits = *s_flag ? FX_NAN_BITS : (unsigned long long)__double_as_longlong(a);
        if (bits != 0) __hip_atomic_fetch_max(word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// k_refine's gather of the gradient texels at p (mad_refine.hip): false, and g = 0, unless p lies strictly inside the map
__device__ __forceinline__ bool fx_gather(const FxArgs &A, const double p[3], double g[3]) {
    g[0] = g[1] = g[2] = 0.0;
    const bool inside = (p[0] > A.o[0]) && (p[0] < A.o[0] + A.nx * A.vs - A.vs) && (p[1] > A.o[1]) && (p[1] < A.o[1] + A.ny * A.vs - A.vs) &&
                        (p[2] > A.o[2]) && (p[2] < A.o[2] + A.nz * A.vs - A.vs);
    if (!inside) return false;
    const int dims[3] = {A.nx, A.ny, A.nz};
    int i0[3];
    double y[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        int ii = (int)floor((p[d] - A.o[d]) / A.vs);
        ii = max(0, min(ii, dims[d] - 2));
        while (ii > 0 && p[d] < A.o[d] + ii * A.del[d]) ii--;
        while (ii < dims[d] - 2 && p[d] >= A.o[d] + (ii + 1) * A.del[d]) ii++;
        const double g0 = A.o[d] + ii * A.del[d], g1 = A.o[d] + (ii + 1) * A.del[d];
        i0[d] = ii;
        y[d] = (p[d] - g0) / (g1 - g0);
    }
#pragma unroll
    for (int cx = 0; cx < 2; cx++)
#pragma unroll
        for (int cy = 0; cy < 2; cy++)
#pragma unroll
            for (int cz = 0; cz < 2; cz++) {
                double wgt = 1.0;
                wgt = wgt * (cx ? y[0] : 1 - y[0]);
                wgt = wgt * (cy ? y[1] : 1 - y[1]);
                wgt = wgt * (cz ? y[2] : 1 - y[2]);
                const float4 t = A.grad[((size_t)(i0[0] + cx) * A.ny + (i0[1] + cy)) * A.nz + (i0[2] + cz)];
                g[0] = g[0] + (double)t.x * wgt;
                g[1] = g[1] + (double)t.y * wgt;
                g[2] = g[2] + (double)t.z * wgt;
            }
    return true;
}

__global__ __launch_bounds__(FX_MAX_THREADS) void k_fx_fit(FxArgs A) {
    __shared__ double s_run[FX_RUN];
    __shared__ double s_red[FX_MAX_THREADS / MAD_WAVE];
    __shared__ int s_flag;
    const int tid = threadIdx.x, T = blockDim.x;
    const int64_t n = A.n, own0 = (int64_t)blockIdx.x * T + tid, stride = (int64_t)gridDim.x * T;
    unsigned long long epoch = 0;

    // g0 = sqrt(sum_i |w_i g_i|^2 / n) at the start coordinates, the sum in fourier.tree_sum's pairing: runs of 256 consecutive
    // terms, each halved 128 + 128, 64 + 64, ..., and the runs' sums again, level by level; a level's runs are dealt over the
    // workgroups, so the pairing does not depend on the plan
    for (int64_t i = own0; i < n; i += stride) {
        const double p[3] = {A.x[3 * i], A.x[3 * i + 1], A.x[3 * i + 2]};      // (the host's copy: nobody has stored yet)
        double g[3];
        fx_gather(A, p, g);
        const double w = A.w ? A.w[i] : 1.0;
        const double a = w * g[0], b = w * g[1], c = w * g[2];
        fx_store(A.sum_a + i, (a * a + b * b) + c * c);
        A.prv[3 * i] = p[0]; A.prv[3 * i + 1] = p[1]; A.prv[3 * i + 2] = p[2];
    }
    fx_barrier(A, epoch);
    double *in = A.sum_a, *out = A.sum_b;
    int64_t terms = n;
    do {
        const int64_t runs = (terms + FX_RUN - 1) / FX_RUN;
        for (int64_t r = blockIdx.x; r < runs; r += gridDim.x) {
            for (int k = tid; k < FX_RUN; k += T) s_run[k] = r * FX_RUN + k < terms ? fx_load(in + r * FX_RUN + k) : 0.0;
            __syncthreads();
            for (int h = FX_RUN / 2; h >= 1; h >>= 1) {
                for (int k = tid; k < h; k += T) s_run[k] = s_run[k] + s_run[k + h];
                __syncthreads();
            }
            if (tid == 0) fx_store(out + r, s_run[0]);
            __syncthreads();
        }
        fx_barrier(A, epoch);
        double *t = in; in = out; out = t;
        terms = runs;
    } while (terms > 1);
    const double g0 = sqrt(fx_load(in) / (double)n);
    if (blockIdx.x == 0 && tid == 0) { A.out->g0 = g0; A.out->step = A.max_step; A.out->converged = 0; A.out->last_step = -1; }
    if (g0 == 0.0) return;      // no atom feels the map: the host refuses

    double step = A.max_step;
    int batch = 0, conv = 0, last = A.n_steps - 1;
    for (int s = 0; s < A.n_steps; s++) {
        // 1: the forces of the own atoms
        unsigned long long *word = A.words + FX_W_FORCE + 8 * (s & 1);
        double lm = 0.0;
        bool bad = false;
        for (int64_t i = own0; i < n; i += stride) {
            double *F = A.F + 3 * i;
            if (A.fixed && A.fixed[i]) { F[0] = F[1] = F[2] = 0.0; continue; }
            const double p[3] = {fx_load(A.x + 3 * i), fx_load(A.x + 3 * i + 1), fx_load(A.x + 3 * i + 2)};
            double g[3];
            fx_gather(A, p, g);
            const double w = A.w ? A.w[i] : 1.0;
            double f0 = (w * g[0]) / g0, f1 = (w * g[1]) / g0, f2 = (w * g[2]) / g0;
            for (int e = A.first[i]; e < A.first[i + 1]; e++) {
                const int j = A.nbr[e];
                const double dx = fx_load(A.x + 3 * j) - p[0], dy = fx_load(A.x + 3 * j + 1) - p[1], dz = fx_load(A.x + 3 * j + 2) - p[2];
                const double d = sqrt((dx * dx + dy * dy) + dz * dz);
                if (d == 0.0) continue;
                const double t = (A.stiffness * (d - A.rest[e])) / d;
                f0 = f0 + t * dx; f1 = f1 + t * dy; f2 = f2 + t * dz;
            }
            F[0] = f0; F[1] = f1; F[2] = f2;
            const double len = sqrt((f0 * f0 + f1 * f1) + f2 * f2);
            if (len != len || p[0] != p[0] || p[1] != p[1] || p[2] != p[2]) bad = true;
            else lm = fmax(lm, len);
        }
        // 2: the largest of all
        fx_publish_max(lm, bad, word, s_red, &s_flag);
        // 3
        fx_barrier(A, epoch);
        const double m = __longlong_as_double((long long)__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        // the other slot is the next step's: nobody reads it any more, nobody adds to it before the barrier below
        if (blockIdx.x == 0 && tid == 0) __hip_atomic_store(A.words + FX_W_FORCE + 8 * ((s + 1) & 1), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (m != m) { conv = 0; last = s; break; }      // a coordinate or a force is a NaN
        if (m == 0.0) { conv = 1; last = s; break; }
        // 4: the own atoms move; at a batch boundary, how far since the last one
        const double scale = step / m;
        batch++;
        const bool batch_end = batch == FX_BATCH;
        unsigned long long *mword = A.words + FX_W_MOVE + 8 * ((s / FX_BATCH) & 1);
        double ld = 0.0;
        for (int64_t i = own0; i < n; i += stride) {
            if (A.fixed && A.fixed[i]) continue;
            const double *F = A.F + 3 * i;
            const double x = fx_load(A.x + 3 * i) + F[0] * scale, y = fx_load(A.x + 3 * i + 1) + F[1] * scale, z = fx_load(A.x + 3 * i + 2) + F[2] * scale;
            fx_store(A.x + 3 * i, x); fx_store(A.x + 3 * i + 1, y); fx_store(A.x + 3 * i + 2, z);
            if (batch_end) {
                double *q = A.prv + 3 * i;
                const double a = x - q[0], b = y - q[1], c = z - q[2];
                ld = fmax(ld, sqrt((a * a + b * b) + c * c));
                q[0] = x; q[1] = y; q[2] = z;
            }
        }
        if (batch_end) fx_publish_max(ld, false, mword, s_red, &s_flag);
        // 5
        fx_barrier(A, epoch);
        if (batch_end) {
            const double moved = __longlong_as_double((long long)__hip_atomic_load(mword, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            // the other slot is the next batch's: it was last read a batch ago and is next added to three barriers from here
            if (blockIdx.x == 0 && tid == 0) __hip_atomic_store(A.words + FX_W_MOVE + 8 * ((s / FX_BATCH + 1) & 1), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (moved < step) step *= 0.5;
            batch = 0;
        }
        if (step < A.min_step) { conv = 1; last = s; break; }
    }
    if (blockIdx.x == 0 && tid == 0) { A.out->step = step; A.out->converged = conv; A.out->last_step = last; }
}

static inline size_t fx_up(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" int mad_flex_fit(mad_ctx *ctx, int64_t n_atoms, const double *coords, const double *weights, const uint8_t *fixed, const int32_t *first,
                            const int32_t *nbr, const double *rest, double stiffness, int n_steps, double max_step, double min_step,
                            double *coords_out, int32_t *converged, int32_t *last_step, double *step, double *g0) {
    if (!ctx) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    const char *who = "mad_flex_fit";
    if (!coords_out || !converged || !last_step || !step || !g0)
        return mad_fail(ctx, MAD_EINVAL, "%s: NULL %s", who, !coords_out ? "coords_out" : !converged ? "converged" : !last_step ? "last_step" : !step ? "step" : "g0");
    const DensityDev &d = ctx->dens;
    char msg[256];
    if (!fx_check_fit_args(who, d.grad != nullptr, n_atoms, coords, weights, stiffness, n_steps, max_step, min_step, msg, sizeof msg) ||
        !fx_check_network(who, n_atoms, first, nbr, rest, msg, sizeof msg))
        return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    const size_t n = (size_t)n_atoms, springs = (size_t)first[n];
    const FxPlan P = fx_plan(ctx->n_cu, n_atoms, ctx->flex_groups, ctx->flex_threads);
    ctx->last_flex_groups = P.groups; ctx->last_flex_threads = P.threads; ctx->last_flex_apt = P.atoms_per_thread; ctx->last_flex_springs = (int64_t)springs;

    // S_TMP_E: x, prv, F.  S_TMP_F: [weights][fixed].  S_TMP_D / S_TMP_H: nbr, rest.  S_TMP_A: first.  S_TMP_B: the sum's two levels.
    // S_TMP_G: [words][out]
    const size_t runs = (n + FX_RUN - 1) / FX_RUN;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), n * 72));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), fx_up(n * 8) + n));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), springs * 4 + 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), springs * 8 + 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (n + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), fx_up(n * 8) + runs * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), fx_up(FX_WORDS * 8) + sizeof(FxOut)));
    FxArgs A;
    A.grad = d.grad; A.nx = d.nx; A.ny = d.ny; A.nz = d.nz; A.vs = d.vs;
    for (int i = 0; i < 3; i++) {
        A.o[i] = d.o[i];
        volatile double t = d.o[i] + d.vs;      // np.arange's element step, as refine_device
        A.del[i] = t - d.o[i];
    }
    A.n = (int)n;
    A.x = scratch<double>(ctx, S_TMP_E); A.prv = A.x + 3 * n; A.F = A.x + 6 * n;
    char *wf = scratch<char>(ctx, S_TMP_F);
    A.w = weights ? (const double *)wf : nullptr;
    A.fixed = fixed ? (const unsigned char *)(wf + fx_up(n * 8)) : nullptr;
    A.first = scratch<int>(ctx, S_TMP_A); A.nbr = scratch<int>(ctx, S_TMP_D); A.rest = scratch<double>(ctx, S_TMP_H);
    A.stiffness = stiffness; A.n_steps = n_steps; A.max_step = max_step; A.min_step = min_step;
    char *sm = scratch<char>(ctx, S_TMP_G);
    A.words = (unsigned long long *)sm; A.out = (FxOut *)(sm + fx_up(FX_WORDS * 8));
    A.sum_a = scratch<double>(ctx, S_TMP_B); A.sum_b = (double *)(scratch<char>(ctx, S_TMP_B) + fx_up(n * 8));
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // nothing of an earlier call still reads the scratch that is rewritten below
    MAD_HIP(hipMemcpyAsync(A.x, coords, n * 24, hipMemcpyHostToDevice, ctx->stream));
    if (weights) MAD_HIP(hipMemcpyAsync((void *)A.w, weights, n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (fixed) MAD_HIP(hipMemcpyAsync((void *)A.fixed, fixed, n, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync((void *)A.first, first, (n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (springs) {
        MAD_HIP(hipMemcpyAsync((void *)A.nbr, nbr, springs * 4, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)A.rest, rest, springs * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    MAD_HIP(hipMemsetAsync(sm, 0, fx_up(FX_WORDS * 8) + sizeof(FxOut), ctx->stream));
    mad_timer_begin(ctx, MAD_T_FLEX_STEPS);
    hipLaunchKernelGGL(k_fx_fit, dim3(P.groups), dim3(P.threads), 0, ctx->stream, A);
    mad_timer_end(ctx, MAD_T_FLEX_STEPS);
    MAD_HIP(hipGetLastError());
    FxOut o;
    MAD_HIP(hipMemcpyAsync(&o, A.out, sizeof o, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(coords_out, A.x, n * 24, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    *g0 = o.g0;
    if (o.g0 == 0.0) return mad_fail(ctx, MAD_EDOM, "%s: no atom feels the map (the gradient is zero at every atom inside it)", who);
    *converged = o.converged; *last_step = o.last_step; *step = o.step;
    return MAD_OK;
}

extern "C" int mad_last_flex_plan(mad_ctx *ctx, int32_t *workgroups, int32_t *threads, int32_t *atoms_per_thread, int64_t *springs) {
    if (!ctx) return MAD_EINVAL;
    if (workgroups) *workgroups = ctx->last_flex_groups;
    if (threads) *threads = ctx->last_flex_threads;
    if (atoms_per_thread) *atoms_per_thread = ctx->last_flex_apt;
    if (springs) *springs = ctx->last_flex_springs;
    return MAD_OK;
}
