// mad_jointfit.hip -- the placed bodies of an assembly refined together against the map, for gfx950.
//
// A round is one batch of refine_pdb (structure_utils.py:58-161): every body that still moves takes four steps of k_refine's
// gradient ascent, not against the map but against the map minus what the OTHER bodies explain, F_b = map - s (M - rho_b), and
// that field is re-made before every round from where the bodies then stand:
//   k_jf_splat, k_jf_blur x 3   rho_b on a cube of the map's own lattice around body b (2^-36 fixed-point splat as k_splat_b, the
//                               separable Gaussian of structure_to_density in float64), only for bodies that moved last round
//   k_jf_accum                  M = sum of the rho_b in ascending b per voxel, and per-workgroup partial sums of <map, M>, <M, M>
//   k_jf_scale                  one workgroup adds the partials in a fixed order: s stays on the device
//   k_jf_texels                 body b's np.gradient texels of float32(F_b) over its cube, from map, M and rho_b directly
//   k_jf_steps                  the round's steps of all moving bodies: k_refine's loop with its state kept between launches
// mad_assembly_refine_symmetric (section 4z) runs the same round over the images of asymmetric units under a point group's operators,
// with k_jf_init_sym and k_jf_steps_sym in the place of the last: the images of a unit take one common step.
// The host enqueues rounds and never waits between them; once no body moves every kernel returns at its first instruction.
// No floating-point atomic anywhere: the same bits every call.  block_reduce, group_reduce, rod_mat, unit_vec and the gather are
// copies of mad_refine.hip's, which is left as it is.
#include <vector>

#include "mad_common.h"
#include "mad_jointfit_plan.h"

#define JF_WAVES (JF_THREADS / MAD_WAVE)
#define JF_DOT_WGS 1024      // workgroups (partial sums) of k_jf_accum at most

struct JfBody {
    long long atom0, n;          // its atoms in the coordinate and mass arrays
    double cen[3], maxd;         // start centre and farthest atom (k_jf_init)
    double rot[9], trans[3], step;
    int active;                  // takes steps: neither fixed nor converged nor stopped by a NaN
    int conv, last;
    int moved;                   // the round whose steps moved it last (-1: none yet): rho_b is re-made in the round after
    int lo[3], e[3];             // its cube on the lattice; lo is re-placed by the kernel that moves the body
    int edge;
    int g0, G;                   // its workgroups in k_jf_init / k_jf_steps
    long long vox0;              // its cube in the box buffers
};

struct JfCtl {
    int n_moving;                // bodies that still take steps
    int rounds;                  // rounds in which steps were taken
    int err;                     // an atom inside the map lay outside its body's cube (cannot happen by jf_box_edge)
    int pad;
    double s;
};

struct JfArgs {
    JfBody *body;
    JfCtl *ctl;
    int n_bodies, round;
    const float *map;
    int nx, ny, nz;
    double o[3], del[3], vs;
    const double *mass;
    double *cur, *ini, *prv;     // all atoms x 3: current, start, last batch boundary
    long long *fix;              // box buffer A: the splat, fixed point
    double *bufa, *bufb;         // box buffers (bufa aliases fix); rho_b ends in bufb
    double *M;                   // lattice
    float4 *tex;                 // box texels
    int r;
    const double *taps;
    double *dot;                 // JF_DOT_WGS x 2 partial sums
    int dot_wgs;
    double *scale;               // nullable: s per round
    int n_steps;
    double max_step, min_step;
    unsigned long long *arrive;  // per body (k_jf_steps_sym: per unit), zeroed before every launch that reduces over a body's workgroups
    double *partial;             // n_bodies x 2 x JF_MAX_G x 8 (k_jf_steps_sym: 2 x workgroups x 8, a unit's members side by side)
};

// mad_assembly_refine_symmetric: the operators, and where the units' own coordinates live (section 4z)
struct JfSym {
    int K;                       // operators; image (u, g) is body u K + g
    int n_wgs;                   // workgroups of k_jf_init_sym / k_jf_steps_sym: the stride of the two slots of A.partial
    const double *op_rot, *op_trans;
    const double *uini;          // the units' start coordinates, unit after unit
    double *wcur, *wprv;         // laid out as A.cur (the images' coordinates): every image's own copy of its unit's coordinates, now
                                 // and at the last batch boundary
};

// ---------------------------------------------------------------------------
// reductions and small matrices (mad_refine.hip)
// ---------------------------------------------------------------------------

// fixed-order block reduction of NV doubles per thread (sum or max); result valid in all threads
template <int NV, bool IS_MAX>
__device__ __forceinline__ void jf_block_reduce(double *v, double *lds /* JF_WAVES * NV + NV */) {
    const int lane = lane_id(), w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = IS_MAX ? wave_max_f64(v[i]) : wave_sum_f64(v[i]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; i++) lds[w * NV + i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < NV; i++) {
            double a = lds[i];
            for (int k = 1; k < (int)(blockDim.x >> 6); k++) a = IS_MAX ? fmax(a, lds[k * NV + i]) : a + lds[k * NV + i];
            lds[JF_WAVES * NV + i] = a;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = lds[JF_WAVES * NV + i];
}

// The same over the G workgroups of one body: publish, arrive, wait, combine in a fixed order (8-byte agent-scope atomics on both
// sides, two slots used alternately; see group_reduce in mad_refine.hip).  All workgroups of the launch are resident.
template <int NV, bool IS_MAX>
__device__ __forceinline__ void jf_group_reduce(double *v, double *lds, const JfArgs &A, int b, int G, int g, unsigned &epoch) {
    jf_block_reduce<NV, IS_MAX>(v, lds);
    if (G == 1) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        double *slot = A.partial + ((size_t)(b * 2 + (epoch & 1)) * JF_MAX_G) * 8;
        for (int i = 0; i < NV; i++) __hip_atomic_store(slot + g * 8 + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(A.arrive + b, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long want = (unsigned long long)G * (epoch + 1);
        while (__hip_atomic_load(A.arrive + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) __builtin_amdgcn_s_sleep(2);
        for (int i = 0; i < NV; i++) {
            double a = __hip_atomic_load(slot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int k = 1; k < G; k++) {
                const double c = __hip_atomic_load(slot + k * 8 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a = IS_MAX ? fmax(a, c) : a + c;
            }
            lds[JF_WAVES * NV + i] = a;
        }
    }
    epoch++;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = lds[JF_WAVES * NV + i];
}

// math_utils.py:15-27
__device__ __forceinline__ void jf_rod_mat(const double ax[3], double angle, double *m) {
    const double a = cos(angle / 2.0), s = sin(angle / 2.0);
    const double b = -ax[0] * s, c = -ax[1] * s, d = -ax[2] * s;
    const double aa = a * a, bb = b * b, cc = c * c, dd = d * d;
    const double bc = b * c, ad = a * d, ac = a * c, ab = a * b, bd = b * d, cd = c * d;
    m[0] = aa + bb - cc - dd; m[1] = 2 * (bc + ad); m[2] = 2 * (bd - ac);
    m[3] = 2 * (bc - ad); m[4] = aa + cc - bb - dd; m[5] = 2 * (cd + ab);
    m[6] = 2 * (bd + ac); m[7] = 2 * (cd - ab); m[8] = aa + dd - bb - cc;
}

// math_utils.py:5-13: a vector that cannot be normalised is returned as is
__device__ __forceinline__ void jf_unit_vec(const double v[3], double o[3]) {
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (n == 0.0 || n != n) { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; return; }
    o[0] = v[0] / n; o[1] = v[1] / n; o[2] = v[2] / n;
}

template <int MAXA, class F>
__device__ __forceinline__ void jf_atoms(int64_t first, int64_t stride, int64_t n, F &&f) {
    if (MAXA > 0) {
#pragma unroll
        for (int s = 0; s < (MAXA > 0 ? MAXA : 1); s++) {
            const int64_t i = first + s * stride;
            if (i < n) f(s, i);
            __builtin_amdgcn_sched_barrier(0);      // one atom at a time, as k_refine
        }
    } else {
        for (int64_t i = first; i < n; i += stride) f(0, i);
    }
}

// the body and the workgroup of it that block `blk` is (bodies' workgroups lie back to back: g0, G)
__device__ __forceinline__ int jf_body_of(const JfArgs &A, int blk) {
    int b = 0;
    while (b + 1 < A.n_bodies && blk >= A.body[b + 1].g0) b++;
    return b;
}

__device__ __forceinline__ void jf_place(const JfArgs &A, JfBody &B) {
    const int dims[3] = {A.nx, A.ny, A.nz};
    for (int d = 0; d < 3; d++) B.lo[d] = jf_box_lo(B.cen[d] + B.trans[d], A.o[d], A.vs, B.edge, dims[d]);
}

// ---------------------------------------------------------------------------
// the start of a run: structure_utils.py:65-67 per body, summed as k_refine sums them
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(JF_THREADS) void k_jf_init(JfArgs A) {
    __shared__ double red[JF_WAVES * 3 + 3];
    const int b = jf_body_of(A, blockIdx.x);
    JfBody &B = A.body[b];
    const int G = B.G, grp = blockIdx.x - B.g0, tid = threadIdx.x;
    const int64_t n = B.n, first = (int64_t)grp * blockDim.x + tid, stride = (int64_t)G * blockDim.x;
    const double *cur = A.cur + (size_t)B.atom0 * 3;
    double *ini = A.ini + (size_t)B.atom0 * 3, *prv = A.prv + (size_t)B.atom0 * 3;
    unsigned epoch = 0;
    double v[3] = {0, 0, 0};
    for (int64_t i = first; i < n; i += stride) {
        const double x = cur[3 * i], y = cur[3 * i + 1], z = cur[3 * i + 2];
        ini[3 * i] = x; ini[3 * i + 1] = y; ini[3 * i + 2] = z;
        prv[3 * i] = x; prv[3 * i + 1] = y; prv[3 * i + 2] = z;
        v[0] += x; v[1] += y; v[2] += z;
    }
    jf_group_reduce<3, false>(v, red, A, b, G, grp, epoch);
    const double cen0 = v[0] / (double)n, cen1 = v[1] / (double)n, cen2 = v[2] / (double)n;
    v[0] = 0;
    for (int64_t i = first; i < n; i += stride) {
        const double a = cur[3 * i] - cen0, c = cur[3 * i + 1] - cen1, d = cur[3 * i + 2] - cen2;
        v[0] = fmax(v[0], sqrt(a * a + c * c + d * d));
    }
    jf_group_reduce<1, true>(v, red, A, b, G, grp, epoch);
    if (tid == 0 && grp == 0) {
        B.cen[0] = cen0; B.cen[1] = cen1; B.cen[2] = cen2; B.maxd = v[0];
        for (int i = 0; i < 9; i++) B.rot[i] = (i % 4 == 0) ? 1.0 : 0.0;
        B.trans[0] = B.trans[1] = B.trans[2] = 0;
        B.step = A.max_step;
        jf_place(A, B);
    }
}

// ---------------------------------------------------------------------------
// the model: rho_b per box, M per voxel, s
// ---------------------------------------------------------------------------

// rho_b is re-made in this round: the body moved in the round before, or nothing has been made yet
__device__ __forceinline__ bool jf_stale(const JfArgs &A, const JfBody &B) { return A.round == 0 || B.moved == A.round - 1; }

// Trilinear, mass-weighted splat of body blockIdx.y's current atoms into its box, 2^-36 fixed point (integer atomics commute).  An
// atom counts when its cell index i0 satisfies 0 <= i0 <= n - 2 on every axis of the MAP, i.e. 0 <= (p - o) / vs < n - 1.
__global__ __launch_bounds__(256) void k_jf_splat(JfArgs A) {
    if (A.ctl->n_moving == 0) return;
    const JfBody &B = A.body[blockIdx.y];
    if (!jf_stale(A, B)) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B.n) return;
    const double *p = A.cur + 3 * (size_t)(B.atom0 + i);
    const int dims[3] = {A.nx, A.ny, A.nz};
    int c0[3];
    double w[3][2];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double g = (p[d] - A.o[d]) / A.vs;
        if (!(g >= 0.0) || !(g < (double)(dims[d] - 1))) return;
        const double fl = floor(g), f = g - fl;
        c0[d] = (int)fl - B.lo[d];
        if (c0[d] < 0 || c0[d] + 1 >= B.e[d]) { A.ctl->err = 1; return; }
        w[d][0] = 1.0 - f; w[d][1] = f;
    }
    const double m = A.mass[B.atom0 + i];
    long long *grid = A.fix + B.vox0;
#pragma unroll
    for (int dx = 0; dx < 2; dx++)
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dz = 0; dz < 2; dz++) {
                const long long q = __double2ll_rn(ldexp(((m * w[0][dx]) * w[1][dy]) * w[2][dz], JF_FIX_BITS));
                atomicAdd((unsigned long long *)&grid[((size_t)(c0[0] + dx) * B.e[1] + (c0[1] + dy)) * B.e[2] + (c0[2] + dz)], (unsigned long long)q);
            }
}

// One pass of the separable Gaussian along `axis` over every stale box: out[p] = sum over t = 0 .. 2 r, ascending, of
// in[p + t - r] taps[t], terms outside the box left out (they are zeros of the lattice, or lie beyond it).  FIRST: the input is the
// fixed-point splat.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_jf_blur(JfArgs A, int axis, const double *__restrict__ in_all, double *__restrict__ out_all) {
    if (A.ctl->n_moving == 0) return;
    const JfBody &B = A.body[blockIdx.y];
    if (!jf_stale(A, B)) return;
    const int e0 = B.e[0], e1 = B.e[1], e2 = B.e[2];
    const size_t n = (size_t)e0 * e1 * e2;
    const double *in = in_all + B.vox0;
    double *out = out_all + B.vox0;
    const int dn = axis == 0 ? e0 : (axis == 1 ? e1 : e2);
    const size_t st = axis == 0 ? (size_t)e1 * e2 : (axis == 1 ? (size_t)e2 : 1);
    const int r = A.r;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int z = (int)(i % e2), y = (int)((i / e2) % e1), x = (int)(i / ((size_t)e2 * e1));
        const int pos = axis == 0 ? x : (axis == 1 ? y : z);
        const size_t base = i - (size_t)pos * st;
        double acc = 0;
        for (int t = 0; t <= 2 * r; t++) {
            const int s = pos + t - r;
            if (s < 0 || s >= dn) continue;
            const double val = FIRST ? ldexp((double)((const long long *)in)[base + (size_t)s * st], -JF_FIX_BITS) : in[base + (size_t)s * st];
            acc += val * A.taps[t];
        }
        out[i] = acc;
    }
}

// rho_b at lattice voxel (x, y, z): 0 outside its box
__device__ __forceinline__ double jf_rho_at(const JfArgs &A, const JfBody &B, int x, int y, int z) {
    const int bx = x - B.lo[0], by = y - B.lo[1], bz = z - B.lo[2];
    if (bx < 0 || by < 0 || bz < 0 || bx >= B.e[0] || by >= B.e[1] || bz >= B.e[2]) return 0.0;
    return A.bufb[B.vox0 + ((size_t)bx * B.e[1] + by) * B.e[2] + bz];
}

// M per voxel, the boxes that hold it added in ascending b, and this workgroup's part of <map, M> and <M, M> (a fixed set of
// voxels per thread, a fixed tree over the threads): dot[2 blockIdx.x ..]
__global__ __launch_bounds__(256) void k_jf_accum(JfArgs A) {
    __shared__ int s_lo[JF_MAX_BODIES][3], s_e[JF_MAX_BODIES][3];
    __shared__ long long s_v0[JF_MAX_BODIES];
    __shared__ double wt[4][2];
    if (A.ctl->n_moving == 0) return;
    for (int b = threadIdx.x; b < A.n_bodies; b += 256) {
        for (int d = 0; d < 3; d++) { s_lo[b][d] = A.body[b].lo[d]; s_e[b][d] = A.body[b].e[d]; }
        s_v0[b] = A.body[b].vox0;
    }
    __syncthreads();
    const size_t n = (size_t)A.nx * A.ny * A.nz;
    double dm = 0, mm = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int z = (int)(i % A.nz), y = (int)((i / A.nz) % A.ny), x = (int)(i / ((size_t)A.nz * A.ny));
        double m = 0.0;
        for (int b = 0; b < A.n_bodies; b++) {
            const int bx = x - s_lo[b][0], by = y - s_lo[b][1], bz = z - s_lo[b][2];
            if (bx < 0 || by < 0 || bz < 0 || bx >= s_e[b][0] || by >= s_e[b][1] || bz >= s_e[b][2]) continue;
            m = m + A.bufb[s_v0[b] + ((size_t)bx * s_e[b][1] + by) * s_e[b][2] + bz];
        }
        A.M[i] = m;
        dm += (double)A.map[i] * m;
        mm += m * m;
    }
    dm = wave_sum_f64(dm); mm = wave_sum_f64(mm);
    if (lane_id() == 0) { wt[threadIdx.x >> 6][0] = dm; wt[threadIdx.x >> 6][1] = mm; }
    __syncthreads();
    if (threadIdx.x < 2) A.dot[2 * blockIdx.x + threadIdx.x] = ((wt[0][threadIdx.x] + wt[1][threadIdx.x]) + wt[2][threadIdx.x]) + wt[3][threadIdx.x];
}

// s = <map, M> / <M, M> (0 when <M, M> is 0) from the partial sums: thread t adds partials t, t + 256, ..., then the fixed tree
__global__ __launch_bounds__(256) void k_jf_scale(JfArgs A) {
    __shared__ double wt[4][2];
    if (A.ctl->n_moving == 0) return;
    double dm = 0, mm = 0;
    for (int i = threadIdx.x; i < A.dot_wgs; i += 256) { dm += A.dot[2 * i]; mm += A.dot[2 * i + 1]; }
    dm = wave_sum_f64(dm); mm = wave_sum_f64(mm);
    if (lane_id() == 0) { wt[threadIdx.x >> 6][0] = dm; wt[threadIdx.x >> 6][1] = mm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double d = ((wt[0][0] + wt[1][0]) + wt[2][0]) + wt[3][0], q = ((wt[0][1] + wt[1][1]) + wt[2][1]) + wt[3][1];
        const double s = q == 0.0 ? 0.0 : d / q;
        A.ctl->s = s;
        if (A.scale) A.scale[A.round] = s;
        A.ctl->rounds = A.round + 1;
    }
}

// ---------------------------------------------------------------------------
// the field: body b's np.gradient texels of F_b = float32(map - s (M - rho_b)) over its box
// ---------------------------------------------------------------------------
__device__ __forceinline__ float jf_field_at(const JfArgs &A, const JfBody &B, double s, int x, int y, int z) {
    const size_t i = ((size_t)x * A.ny + y) * A.nz + z;
    const double other = A.M[i] - jf_rho_at(A, B, x, y, z);
    return (float)((double)A.map[i] - s * other);
}

__global__ __launch_bounds__(256) void k_jf_texels(JfArgs A) {
    if (A.ctl->n_moving == 0) return;
    const JfBody &B = A.body[blockIdx.y];
    if (!B.active) return;
    const double s = A.ctl->s;
    const int e1 = B.e[1], e2 = B.e[2];
    const size_t n = (size_t)B.e[0] * e1 * e2;
    float4 *tex = A.tex + B.vox0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int x = B.lo[0] + (int)(i / ((size_t)e2 * e1)), y = B.lo[1] + (int)((i / e2) % e1), z = B.lo[2] + (int)(i % e2);
        // np.gradient: one-sided at the MAP's faces only (grad1 of mad_refine.hip)
        float g[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const int c = d == 0 ? x : (d == 1 ? y : z), nd = d == 0 ? A.nx : (d == 1 ? A.ny : A.nz);
            const int lo = c == 0 ? c : c - 1, hi = c == nd - 1 ? c : c + 1;
            const float fh = jf_field_at(A, B, s, d == 0 ? hi : x, d == 1 ? hi : y, d == 2 ? hi : z);
            const float fl = jf_field_at(A, B, s, d == 0 ? lo : x, d == 1 ? lo : y, d == 2 ? lo : z);
            g[d] = __fdiv_rn(__fsub_rn(fh, fl), hi - lo == 2 ? 2.0f : 1.0f);
        }
        tex[i] = make_float4(g[0], g[1], g[2], 0.f);
    }
}

// map - s M as float32 over the lattice (mad_assembly_density)
__global__ __launch_bounds__(256) void k_jf_residual(JfArgs A, float *__restrict__ out) {
    const size_t n = (size_t)A.nx * A.ny * A.nz;
    const double s = A.ctl->s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (float)((double)A.map[i] - s * A.M[i]);
}

// ---------------------------------------------------------------------------
// the steps of a round: k_refine's loop (mad_refine.hip) over the steps JF_BATCH round .. of every moving body, against the body's
// own texels.  MAXA > 0: a thread keeps its atoms in registers for the round.  The body's transform, step size and
// batch-boundary coordinates live in global memory between rounds; a round starts at a batch boundary.
// ---------------------------------------------------------------------------
template <int MAXA>
__global__ __launch_bounds__(MAXA > 0 ? JF_THREADS_REG : JF_THREADS) void k_jf_steps(JfArgs A) {
    constexpr bool REG = MAXA > 0;
    double r_ini[REG ? MAXA : 1][3], r_cur[REG ? MAXA : 1][3], r_prv[REG ? MAXA : 1][3];
    __shared__ double red[JF_WAVES * 7 + 7];
    __shared__ double s_rot[9], s_trans[3], s_upd[12];
    __shared__ double s_step;
    const int b = jf_body_of(A, blockIdx.x);
    JfBody &B = A.body[b];
    if (!B.active) return;
    const int G = B.G, grp = blockIdx.x - B.g0, tid = threadIdx.x;
    const int64_t n = B.n, first = (int64_t)grp * blockDim.x + tid, stride = (int64_t)G * blockDim.x;
    unsigned epoch = 0;
    double *cur = A.cur + (size_t)B.atom0 * 3;
    const double *ini = A.ini + (size_t)B.atom0 * 3;
    double *prv = A.prv + (size_t)B.atom0 * 3;
    const float4 *tex = A.tex + B.vox0;
    const int lo0 = B.lo[0], lo1 = B.lo[1], lo2 = B.lo[2], e0 = B.e[0], e1 = B.e[1], e2 = B.e[2];
    const double cen0 = B.cen[0], cen1 = B.cen[1], cen2 = B.cen[2], maxd = B.maxd;
    if (tid == 0) {
        for (int i = 0; i < 9; i++) s_rot[i] = B.rot[i];
        for (int i = 0; i < 3; i++) s_trans[i] = B.trans[i];
        s_step = B.step;
    }
    if (REG)
        jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
            for (int d = 0; d < 3; d++) { r_ini[s][d] = ini[3 * i + d]; r_prv[s][d] = prv[3 * i + d]; r_cur[s][d] = cur[3 * i + d]; }
        });
    __syncthreads();
    auto write_back = [&](bool boundary) {      // REG: the coordinates leave the registers once per round
        if (REG) jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
            for (int d = 0; d < 3; d++) { cur[3 * i + d] = r_cur[s][d]; if (boundary) prv[3 * i + d] = r_prv[s][d]; }
        });
    };
    // what the body is left as: its transform for the next round, or its result
    auto leave = [&](int conv, int last, bool moving) {
        if (tid == 0 && grp == 0) {
            for (int i = 0; i < 9; i++) B.rot[i] = s_rot[i];
            for (int i = 0; i < 3; i++) B.trans[i] = s_trans[i];
            B.step = s_step;
            B.conv = conv; B.last = last; B.moved = A.round;
            jf_place(A, B);
            if (!moving) { B.active = 0; atomicSub(&A.ctl->n_moving, 1); }
        }
    };

    const int step0 = JF_BATCH * A.round, step1 = step0 + jf_round_steps(A.n_steps, A.round);
    int batch = 0, step = step0, conv = 0;
    bool boundary = false;
    double v[7];
    for (step = step0; step < step1; step++) {
        const double r0 = s_rot[0], r1 = s_rot[1], r2 = s_rot[2], r3 = s_rot[3], r4 = s_rot[4], r5 = s_rot[5], r6 = s_rot[6],
                     r7 = s_rot[7], r8 = s_rot[8];
        const double ct0 = cen0 + s_trans[0], ct1 = cen1 + s_trans[1], ct2 = cen2 + s_trans[2];
        const double step_size = s_step;
        for (int i = 0; i < 7; i++) v[i] = 0;
        jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
            // :91-96 re-apply the accumulated transform to the start coordinates
            const double a = (REG ? r_ini[s][0] : ini[3 * i]) - cen0, bb = (REG ? r_ini[s][1] : ini[3 * i + 1]) - cen1, c = (REG ? r_ini[s][2] : ini[3 * i + 2]) - cen2;
            const double p0 = (a * r0 + bb * r3 + c * r6) + ct0;
            const double p1 = (a * r1 + bb * r4 + c * r7) + ct1;
            const double p2 = (a * r2 + bb * r5 + c * r8) + ct2;
            if (REG) { r_cur[s][0] = p0; r_cur[s][1] = p1; r_cur[s][2] = p2; }
            else { cur[3 * i] = p0; cur[3 * i + 1] = p1; cur[3 * i + 2] = p2; }
            if (p0 != p0 || p1 != p1 || p2 != p2) v[6] = 1.0;
            // :101-103 atoms strictly inside the map
            const bool inside = (p0 > A.o[0]) && (p0 < A.o[0] + A.nx * A.vs - A.vs) && (p1 > A.o[1]) &&
                                (p1 < A.o[1] + A.ny * A.vs - A.vs) && (p2 > A.o[2]) && (p2 < A.o[2] + A.nz * A.vs - A.vs);
            if (!inside) return;
            // :106 trilinear interpolation of the gradient (scipy RegularGridInterpolator, linear)
            const double p[3] = {p0, p1, p2};
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
            const int b0 = i0[0] - lo0, b1 = i0[1] - lo1, b2 = i0[2] - lo2;
            if (b0 < 0 || b1 < 0 || b2 < 0 || b0 + 1 >= e0 || b1 + 1 >= e1 || b2 + 1 >= e2) { A.ctl->err = 1; return; }
            double g[3] = {0, 0, 0};
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
                        const float4 t = tex[((size_t)(b0 + cx) * e1 + (b1 + cy)) * e2 + (b2 + cz)];
                        g[0] = g[0] + (double)t.x * wgt;
                        g[1] = g[1] + (double)t.y * wgt;
                        g[2] = g[2] + (double)t.z * wgt;
                    }
            v[0] += g[0]; v[1] += g[1]; v[2] += g[2];
            // :121-122 torque about the START centroid
            const double c0 = p0 - cen0, c1 = p1 - cen1, c2 = p2 - cen2;
            v[3] += g[1] * c2 - g[2] * c1;
            v[4] += g[2] * c0 - g[0] * c2;
            v[5] += g[0] * c1 - g[1] * c0;
        });
        jf_group_reduce<7, false>(v, red, A, b, G, grp, epoch);
        if (v[6] != 0.0) {      // :97-98
            write_back(false);
            leave(0, step, false);
            return;
        }
        const bool is_trans = (step % 2) == 0;
        if (tid == 0) {
            if (is_trans) {      // :111-116
                double u[3];
                jf_unit_vec(v, u);
                for (int d = 0; d < 3; d++) { u[d] *= step_size; s_upd[d] = u[d]; s_trans[d] += u[d]; }
            } else {             // :123-138
                double ax[3], sm[9], nr[9];
                jf_unit_vec(v + 3, ax);
                jf_rod_mat(ax, step_size / maxd, sm);
                for (int i = 0; i < 9; i++) s_upd[i] = sm[i];
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) nr[3 * i + j] = s_rot[3 * i] * sm[j] + s_rot[3 * i + 1] * sm[3 + j] + s_rot[3 * i + 2] * sm[6 + j];
                for (int i = 0; i < 9; i++) s_rot[i] = nr[i];
            }
        }
        __syncthreads();
        batch++;
        const bool batch_end = batch == JF_BATCH;
        double mn = 0;
        if (is_trans) {
            const double u0 = s_upd[0], u1 = s_upd[1], u2 = s_upd[2];
            jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
                const double x = (REG ? r_cur[s][0] : cur[3 * i]) + u0, yv = (REG ? r_cur[s][1] : cur[3 * i + 1]) + u1, z = (REG ? r_cur[s][2] : cur[3 * i + 2]) + u2;
                if (REG) { r_cur[s][0] = x; r_cur[s][1] = yv; r_cur[s][2] = z; }
                else { cur[3 * i] = x; cur[3 * i + 1] = yv; cur[3 * i + 2] = z; }
                if (batch_end) {
                    const double a = (REG ? r_prv[s][0] : prv[3 * i]) - x, bb = (REG ? r_prv[s][1] : prv[3 * i + 1]) - yv, c = (REG ? r_prv[s][2] : prv[3 * i + 2]) - z;
                    mn = fmax(mn, sqrt(a * a + bb * bb + c * c));
                    if (REG) { r_prv[s][0] = x; r_prv[s][1] = yv; r_prv[s][2] = z; }
                    else { prv[3 * i] = x; prv[3 * i + 1] = yv; prv[3 * i + 2] = z; }
                }
            });
        } else {
            const double m0 = s_upd[0], m1 = s_upd[1], m2 = s_upd[2], m3 = s_upd[3], m4 = s_upd[4], m5 = s_upd[5],
                         m6 = s_upd[6], m7 = s_upd[7], m8 = s_upd[8];
            const double n0 = -1 * cen0 - s_trans[0], n1 = -1 * cen1 - s_trans[1], n2 = -1 * cen2 - s_trans[2];
            jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
                const double a = (REG ? r_cur[s][0] : cur[3 * i]) + n0, bb = (REG ? r_cur[s][1] : cur[3 * i + 1]) + n1, c = (REG ? r_cur[s][2] : cur[3 * i + 2]) + n2;
                const double x = (a * m0 + bb * m3 + c * m6) + ct0;
                const double yv = (a * m1 + bb * m4 + c * m7) + ct1;
                const double z = (a * m2 + bb * m5 + c * m8) + ct2;
                if (REG) { r_cur[s][0] = x; r_cur[s][1] = yv; r_cur[s][2] = z; }
                else { cur[3 * i] = x; cur[3 * i + 1] = yv; cur[3 * i + 2] = z; }
                if (batch_end) {
                    const double pa = (REG ? r_prv[s][0] : prv[3 * i]) - x, pb = (REG ? r_prv[s][1] : prv[3 * i + 1]) - yv, pc = (REG ? r_prv[s][2] : prv[3 * i + 2]) - z;
                    mn = fmax(mn, sqrt(pa * pa + pb * pb + pc * pc));
                    if (REG) { r_prv[s][0] = x; r_prv[s][1] = yv; r_prv[s][2] = z; }
                    else { prv[3 * i] = x; prv[3 * i + 1] = yv; prv[3 * i + 2] = z; }
                }
            });
        }
        if (batch_end) {      // :141-147
            double mv[1] = {mn};
            jf_group_reduce<1, true>(mv, red, A, b, G, grp, epoch);
            if (tid == 0 && mv[0] < s_step) s_step *= 0.5;
            batch = 0;
            boundary = true;
        }
        __syncthreads();
        if (s_step < A.min_step) { conv = 1; break; }      // :150-152
    }
    if (step == step1) step = step1 - 1;
    write_back(boundary);
    leave(conv, step, conv == 0 && step1 < A.n_steps);
}

// ---------------------------------------------------------------------------
// Units under the operators of a point group.  The bodies of the model are the images: body u K + g is
// unit u under operator g, with G workgroups as any body.  The K G workgroups of a unit's images form ONE reduction group,
// image-major: workgroup (g, w) holds slice w of the unit's atoms in the UNIT's frame, maps them through operator g, gathers from
// image g's texels and pulls the gradients back; the group's sums are the unit's force and torque, every workgroup applies the
// same update to its slice, and writes image g's coordinates of that slice for the next splat.  Every image's JfBody carries its own
// copy of the unit's state (the same bits in all of them), written by the image's workgroup 0.  Operator 0 is the identity and
// applies no arithmetic, so that K = 1 computes k_jf_init's and k_jf_steps' bits.
// ---------------------------------------------------------------------------

// a value that is the same in every lane, kept in scalar registers
__device__ __forceinline__ double jf_uniform(double x) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
    return __hiloint2double(hi, lo);
}

// jf_group_reduce over the `members` workgroups of a unit, of which this is number m (ascending g, then ascending w).  The unit's
// slots begin at its first workgroup's index, slot0, in either half of A.partial.  Thread 0 publishes and waits; then the
// partials are fetched by many threads at once into part[members * NV] and thread i adds component i in ascending m.
template <int NV, bool IS_MAX>
__device__ __forceinline__ void jf_group_reduce_sym(double *v, double *lds, double *part, const JfArgs &A, const JfSym &S, int u, int slot0,
                                                    int members, int m, unsigned &epoch) {
    jf_block_reduce<NV, IS_MAX>(v, lds);
    if (members == 1) return;
    __syncthreads();
    double *slot = A.partial + ((size_t)(epoch & 1) * S.n_wgs + slot0) * 8;
    if (threadIdx.x == 0) {
        for (int i = 0; i < NV; i++) __hip_atomic_store(slot + m * 8 + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(A.arrive + u, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long want = (unsigned long long)members * (epoch + 1);
        while (__hip_atomic_load(A.arrive + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) __builtin_amdgcn_s_sleep(2);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < members * NV; t += blockDim.x)
        part[t] = __hip_atomic_load(slot + (t / NV) * 8 + t % NV, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x < NV) {
        double a = part[threadIdx.x];
        for (int k = 1; k < members; k++) {
            const double c = part[k * NV + threadIdx.x];
            a = IS_MAX ? fmax(a, c) : a + c;
        }
        lds[JF_WAVES * NV + threadIdx.x] = a;
    }
    epoch++;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = lds[JF_WAVES * NV + i];
}

// image g's box around the image of the unit's centre, with the unit's edge
__device__ __forceinline__ void jf_place_sym(const JfArgs &A, const JfSym &S, JfBody &B, int g) {
    const int dims[3] = {A.nx, A.ny, A.nz};
    const double c[3] = {B.cen[0] + B.trans[0], B.cen[1] + B.trans[1], B.cen[2] + B.trans[2]};
    double q[3] = {c[0], c[1], c[2]};
    if (g != 0) jf_image(S.op_rot + 9 * g, S.op_trans + 3 * g, c, q);
    for (int d = 0; d < 3; d++) B.lo[d] = jf_box_lo(q[d], A.o[d], A.vs, B.edge, dims[d]);
}

// k_jf_init per unit; every image gets its coordinates, its copies of the unit's and its box.  Only image 0's workgroups add to the
// sums (the others publish zeros, which change neither a sum nor a maximum of distances).
__global__ __launch_bounds__(JF_THREADS) void k_jf_init_sym(JfArgs A, JfSym S) {
    __shared__ double red[JF_WAVES * 3 + 3];
    __shared__ double part[JF_SYM_MAX_MEMBERS * 3];
    const int b = jf_body_of(A, blockIdx.x);
    JfBody &B = A.body[b];
    const int K = S.K, im = b % K, u = b / K;
    const int G = B.G, grp = blockIdx.x - B.g0, tid = threadIdx.x;
    const int slot0 = A.body[b - im].g0, members = K * G, m = im * G + grp;
    const int64_t n = B.n, first = (int64_t)grp * blockDim.x + tid, stride = (int64_t)G * blockDim.x;
    const double *ini = S.uini + (size_t)(A.body[b - im].atom0 / K) * 3;
    double *img = A.cur + (size_t)B.atom0 * 3, *cur = S.wcur + (size_t)B.atom0 * 3, *prv = S.wprv + (size_t)B.atom0 * 3;
    const double *R = S.op_rot + 9 * im, *T = S.op_trans + 3 * im;
    unsigned epoch = 0;
    double v[3] = {0, 0, 0};
    for (int64_t i = first; i < n; i += stride) {
        const double p[3] = {ini[3 * i], ini[3 * i + 1], ini[3 * i + 2]};
        double q[3] = {p[0], p[1], p[2]};
        if (im != 0) jf_image(R, T, p, q);
        for (int d = 0; d < 3; d++) { cur[3 * i + d] = p[d]; prv[3 * i + d] = p[d]; img[3 * i + d] = q[d]; }
        if (im == 0) { v[0] += p[0]; v[1] += p[1]; v[2] += p[2]; }
    }
    jf_group_reduce_sym<3, false>(v, red, part, A, S, u, slot0, members, m, epoch);
    const double cen0 = v[0] / (double)n, cen1 = v[1] / (double)n, cen2 = v[2] / (double)n;
    v[0] = 0;
    if (im == 0)
        for (int64_t i = first; i < n; i += stride) {
            const double a = ini[3 * i] - cen0, c = ini[3 * i + 1] - cen1, d = ini[3 * i + 2] - cen2;
            v[0] = fmax(v[0], sqrt(a * a + c * c + d * d));
        }
    jf_group_reduce_sym<1, true>(v, red, part, A, S, u, slot0, members, m, epoch);
    if (tid == 0 && grp == 0) {
        B.cen[0] = cen0; B.cen[1] = cen1; B.cen[2] = cen2; B.maxd = v[0];
        for (int i = 0; i < 9; i++) B.rot[i] = (i % 4 == 0) ? 1.0 : 0.0;
        B.trans[0] = B.trans[1] = B.trans[2] = 0;
        B.step = A.max_step;
        jf_place_sym(A, S, B, im);
    }
}

// k_jf_steps for the workgroups of a unit's images.  cur, prv: this image's copies of the unit's coordinates (MAXA > 0: in registers
// for the round); img: the image's coordinates, written once per round for the next splat.
template <int MAXA>
__global__ __launch_bounds__(MAXA > 0 ? JF_THREADS_REG : JF_THREADS) void k_jf_steps_sym(JfArgs A, JfSym S) {
    constexpr bool REG = MAXA > 0;
    double r_ini[REG ? MAXA : 1][3], r_cur[REG ? MAXA : 1][3], r_prv[REG ? MAXA : 1][3];
    __shared__ double red[JF_WAVES * 7 + 7];
    __shared__ double part[JF_SYM_MAX_MEMBERS * 7];
    __shared__ double s_rot[9], s_trans[3], s_upd[12];
    __shared__ double s_step;
    const int b = jf_body_of(A, blockIdx.x);
    JfBody &B = A.body[b];
    if (!B.active) return;
    const int K = S.K, im = b % K, u = b / K;
    const int G = B.G, grp = blockIdx.x - B.g0, tid = threadIdx.x;
    const int slot0 = A.body[b - im].g0, members = K * G, m = im * G + grp;
    const int64_t n = B.n, first = (int64_t)grp * blockDim.x + tid, stride = (int64_t)G * blockDim.x;
    unsigned epoch = 0;
    double *img = A.cur + (size_t)B.atom0 * 3, *cur = S.wcur + (size_t)B.atom0 * 3, *prv = S.wprv + (size_t)B.atom0 * 3;
    const double *ini = S.uini + (size_t)(A.body[b - im].atom0 / K) * 3;
    const float4 *tex = A.tex + B.vox0;
    const int lo0 = B.lo[0], lo1 = B.lo[1], lo2 = B.lo[2], e0 = B.e[0], e1 = B.e[1], e2 = B.e[2];
    const double cen0 = B.cen[0], cen1 = B.cen[1], cen2 = B.cen[2], maxd = B.maxd;
    // the operator (row-major R for row vectors, T), uniform over the workgroup
    const double R0 = jf_uniform(S.op_rot[9 * im]), R1 = jf_uniform(S.op_rot[9 * im + 1]), R2 = jf_uniform(S.op_rot[9 * im + 2]),
                 R3 = jf_uniform(S.op_rot[9 * im + 3]), R4 = jf_uniform(S.op_rot[9 * im + 4]), R5 = jf_uniform(S.op_rot[9 * im + 5]),
                 R6 = jf_uniform(S.op_rot[9 * im + 6]), R7 = jf_uniform(S.op_rot[9 * im + 7]), R8 = jf_uniform(S.op_rot[9 * im + 8]);
    const double T0 = jf_uniform(S.op_trans[3 * im]), T1 = jf_uniform(S.op_trans[3 * im + 1]), T2 = jf_uniform(S.op_trans[3 * im + 2]);
    if (tid == 0) {
        for (int i = 0; i < 9; i++) s_rot[i] = B.rot[i];
        for (int i = 0; i < 3; i++) s_trans[i] = B.trans[i];
        s_step = B.step;
    }
    if (REG)
        jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
            for (int d = 0; d < 3; d++) { r_ini[s][d] = ini[3 * i + d]; r_prv[s][d] = prv[3 * i + d]; r_cur[s][d] = cur[3 * i + d]; }
        });
    __syncthreads();
    // the unit's coordinates leave the registers (REG) and the image's are written, once per round
    auto write_back = [&](bool boundary) {
        jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
            const double x = REG ? r_cur[s][0] : cur[3 * i], y = REG ? r_cur[s][1] : cur[3 * i + 1], z = REG ? r_cur[s][2] : cur[3 * i + 2];
            if (REG) {
                cur[3 * i] = x; cur[3 * i + 1] = y; cur[3 * i + 2] = z;
                if (boundary) for (int d = 0; d < 3; d++) prv[3 * i + d] = r_prv[s][d];
            }
            if (im == 0) { img[3 * i] = x; img[3 * i + 1] = y; img[3 * i + 2] = z; }
            else {
                img[3 * i] = ((x * R0 + y * R3) + z * R6) + T0;
                img[3 * i + 1] = ((x * R1 + y * R4) + z * R7) + T1;
                img[3 * i + 2] = ((x * R2 + y * R5) + z * R8) + T2;
            }
        });
    };
    // what the image is left as: the unit's transform for the next round, or its result; image 0 counts the unit
    auto leave = [&](int conv, int last, bool moving) {
        if (tid == 0 && grp == 0) {
            for (int i = 0; i < 9; i++) B.rot[i] = s_rot[i];
            for (int i = 0; i < 3; i++) B.trans[i] = s_trans[i];
            B.step = s_step;
            B.conv = conv; B.last = last; B.moved = A.round;
            jf_place_sym(A, S, B, im);
            if (!moving) { B.active = 0; if (im == 0) atomicSub(&A.ctl->n_moving, 1); }
        }
    };

    const int step0 = JF_BATCH * A.round, step1 = step0 + jf_round_steps(A.n_steps, A.round);
    int batch = 0, step = step0, conv = 0;
    bool boundary = false;
    double v[7];
    for (step = step0; step < step1; step++) {
        const double r0 = s_rot[0], r1 = s_rot[1], r2 = s_rot[2], r3 = s_rot[3], r4 = s_rot[4], r5 = s_rot[5], r6 = s_rot[6],
                     r7 = s_rot[7], r8 = s_rot[8];
        const double ct0 = cen0 + s_trans[0], ct1 = cen1 + s_trans[1], ct2 = cen2 + s_trans[2];
        const double step_size = s_step;
        for (int i = 0; i < 7; i++) v[i] = 0;
        jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
            // the unit's coordinates: the accumulated transform re-applied to the start coordinates, as k_jf_steps
            const double a = (REG ? r_ini[s][0] : ini[3 * i]) - cen0, bb = (REG ? r_ini[s][1] : ini[3 * i + 1]) - cen1, c = (REG ? r_ini[s][2] : ini[3 * i + 2]) - cen2;
            const double p0 = (a * r0 + bb * r3 + c * r6) + ct0;
            const double p1 = (a * r1 + bb * r4 + c * r7) + ct1;
            const double p2 = (a * r2 + bb * r5 + c * r8) + ct2;
            if (REG) { r_cur[s][0] = p0; r_cur[s][1] = p1; r_cur[s][2] = p2; }
            else { cur[3 * i] = p0; cur[3 * i + 1] = p1; cur[3 * i + 2] = p2; }
            if (p0 != p0 || p1 != p1 || p2 != p2) v[6] = 1.0;
            // the image of the atom: where it gathers
            double q0 = p0, q1 = p1, q2 = p2;
            if (im != 0) {
                q0 = ((p0 * R0 + p1 * R3) + p2 * R6) + T0;
                q1 = ((p0 * R1 + p1 * R4) + p2 * R7) + T1;
                q2 = ((p0 * R2 + p1 * R5) + p2 * R8) + T2;
            }
            const bool inside = (q0 > A.o[0]) && (q0 < A.o[0] + A.nx * A.vs - A.vs) && (q1 > A.o[1]) &&
                                (q1 < A.o[1] + A.ny * A.vs - A.vs) && (q2 > A.o[2]) && (q2 < A.o[2] + A.nz * A.vs - A.vs);
            if (!inside) return;
            const double p[3] = {q0, q1, q2};
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
            const int b0 = i0[0] - lo0, b1 = i0[1] - lo1, b2 = i0[2] - lo2;
            if (b0 < 0 || b1 < 0 || b2 < 0 || b0 + 1 >= e0 || b1 + 1 >= e1 || b2 + 1 >= e2) { A.ctl->err = 1; return; }
            double g[3] = {0, 0, 0};
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
                        const float4 t = tex[((size_t)(b0 + cx) * e1 + (b1 + cy)) * e2 + (b2 + cz)];
                        g[0] = g[0] + (double)t.x * wgt;
                        g[1] = g[1] + (double)t.y * wgt;
                        g[2] = g[2] + (double)t.z * wgt;
                    }
            // the gradient in the unit's frame: h = g R^T
            if (im != 0) {
                const double h0 = (g[0] * R0 + g[1] * R1) + g[2] * R2, h1 = (g[0] * R3 + g[1] * R4) + g[2] * R5, h2 = (g[0] * R6 + g[1] * R7) + g[2] * R8;
                g[0] = h0; g[1] = h1; g[2] = h2;
            }
            v[0] += g[0]; v[1] += g[1]; v[2] += g[2];
            // torque about the unit's START centroid, over the unit's own coordinates
            const double c0 = p0 - cen0, c1 = p1 - cen1, c2 = p2 - cen2;
            v[3] += g[1] * c2 - g[2] * c1;
            v[4] += g[2] * c0 - g[0] * c2;
            v[5] += g[0] * c1 - g[1] * c0;
        });
        jf_group_reduce_sym<7, false>(v, red, part, A, S, u, slot0, members, m, epoch);
        if (v[6] != 0.0) {
            write_back(false);
            leave(0, step, false);
            return;
        }
        const bool is_trans = (step % 2) == 0;
        if (tid == 0) {
            if (is_trans) {
                double uv[3];
                jf_unit_vec(v, uv);
                for (int d = 0; d < 3; d++) { uv[d] *= step_size; s_upd[d] = uv[d]; s_trans[d] += uv[d]; }
            } else {
                double ax[3], sm[9], nr[9];
                jf_unit_vec(v + 3, ax);
                jf_rod_mat(ax, step_size / maxd, sm);
                for (int i = 0; i < 9; i++) s_upd[i] = sm[i];
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) nr[3 * i + j] = s_rot[3 * i] * sm[j] + s_rot[3 * i + 1] * sm[3 + j] + s_rot[3 * i + 2] * sm[6 + j];
                for (int i = 0; i < 9; i++) s_rot[i] = nr[i];
            }
        }
        __syncthreads();
        batch++;
        const bool batch_end = batch == JF_BATCH;
        double mn = 0;
        if (is_trans) {
            const double u0 = s_upd[0], u1 = s_upd[1], u2 = s_upd[2];
            jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
                const double x = (REG ? r_cur[s][0] : cur[3 * i]) + u0, yv = (REG ? r_cur[s][1] : cur[3 * i + 1]) + u1, z = (REG ? r_cur[s][2] : cur[3 * i + 2]) + u2;
                if (REG) { r_cur[s][0] = x; r_cur[s][1] = yv; r_cur[s][2] = z; }
                else { cur[3 * i] = x; cur[3 * i + 1] = yv; cur[3 * i + 2] = z; }
                if (batch_end) {
                    const double a = (REG ? r_prv[s][0] : prv[3 * i]) - x, bb = (REG ? r_prv[s][1] : prv[3 * i + 1]) - yv, c = (REG ? r_prv[s][2] : prv[3 * i + 2]) - z;
                    mn = fmax(mn, sqrt(a * a + bb * bb + c * c));
                    if (REG) { r_prv[s][0] = x; r_prv[s][1] = yv; r_prv[s][2] = z; }
                    else { prv[3 * i] = x; prv[3 * i + 1] = yv; prv[3 * i + 2] = z; }
                }
            });
        } else {
            const double m0 = s_upd[0], m1 = s_upd[1], m2 = s_upd[2], m3 = s_upd[3], m4 = s_upd[4], m5 = s_upd[5],
                         m6 = s_upd[6], m7 = s_upd[7], m8 = s_upd[8];
            const double n0 = -1 * cen0 - s_trans[0], n1 = -1 * cen1 - s_trans[1], n2 = -1 * cen2 - s_trans[2];
            jf_atoms<MAXA>(first, stride, n, [&](int s, int64_t i) {
                const double a = (REG ? r_cur[s][0] : cur[3 * i]) + n0, bb = (REG ? r_cur[s][1] : cur[3 * i + 1]) + n1, c = (REG ? r_cur[s][2] : cur[3 * i + 2]) + n2;
                const double x = (a * m0 + bb * m3 + c * m6) + ct0;
                const double yv = (a * m1 + bb * m4 + c * m7) + ct1;
                const double z = (a * m2 + bb * m5 + c * m8) + ct2;
                if (REG) { r_cur[s][0] = x; r_cur[s][1] = yv; r_cur[s][2] = z; }
                else { cur[3 * i] = x; cur[3 * i + 1] = yv; cur[3 * i + 2] = z; }
                if (batch_end) {
                    const double pa = (REG ? r_prv[s][0] : prv[3 * i]) - x, pb = (REG ? r_prv[s][1] : prv[3 * i + 1]) - yv, pc = (REG ? r_prv[s][2] : prv[3 * i + 2]) - z;
                    mn = fmax(mn, sqrt(pa * pa + pb * pb + pc * pc));
                    if (REG) { r_prv[s][0] = x; r_prv[s][1] = yv; r_prv[s][2] = z; }
                    else { prv[3 * i] = x; prv[3 * i + 1] = yv; prv[3 * i + 2] = z; }
                }
            });
        }
        if (batch_end) {      // decided on the unit's own coordinates; every image holds the same ones
            double mv[1] = {mn};
            jf_group_reduce_sym<1, true>(mv, red, part, A, S, u, slot0, members, m, epoch);
            if (tid == 0 && mv[0] < s_step) s_step *= 0.5;
            batch = 0;
            boundary = true;
        }
        __syncthreads();
        if (s_step < A.min_step) { conv = 1; break; }
    }
    if (step == step1) step = step1 - 1;
    write_back(boundary);
    leave(conv, step, conv == 0 && step1 < A.n_steps);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

struct JfRun {
    JfArgs A;
    JfPlan P;
    JfSym S;
    bool sym = false;
    std::vector<double> image_mass;
    std::vector<JfBody> bodies;
    int n_wgs = 0;        // of k_jf_init / k_jf_steps
    bool reg = true;
    unsigned box_blocks = 1, atom_blocks = 1, lat_blocks = 1;
    size_t n_vox = 0, arrive_bytes = 0;
};

static inline size_t jf_up(size_t v) { return (v + 255) & ~(size_t)255; }

// plan, device buffers, uploads.  refine: the coordinate copies, the texels and the reduction words as well.  n_ops > 0: the
// n_bodies given are units, and the bodies of the run are their n_bodies x n_ops images.
static int jf_setup(mad_ctx *ctx, const char *who, int n_bodies, const double *atoms, const double *mass, const int64_t *first_atom,
                    const uint8_t *fixed, double resolution, bool refine, int n_steps, double max_step, double min_step, JfRun &R,
                    int n_ops = 0, const double *op_rot = nullptr, const double *op_trans = nullptr, bool sym = false) {
    const DensityDev &d = ctx->dens;
    const int32_t dims[3] = {d.nx, d.ny, d.nz};
    char msg[256];
    if (!(sym ? jf_plan_sym(who, d.grid ? dims : nullptr, d.o, d.vs, n_bodies, atoms, mass, first_atom, n_ops, op_rot, op_trans, resolution, n_steps, max_step, min_step, R.P, msg, sizeof msg)
              : jf_plan(who, d.grid ? dims : nullptr, d.o, d.vs, n_bodies, atoms, mass, first_atom, resolution, refine, n_steps, max_step, min_step, R.P, msg, sizeof msg)))
        return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    const int n_units = n_bodies, K = sym ? n_ops : 1;
    const size_t n_unit_atoms = (size_t)first_atom[n_units];
    n_bodies = n_units * K;
    R.sym = sym;
    const JfPlan &P = R.P;
    JfArgs &A = R.A;
    memset(&A, 0, sizeof A);
    R.n_vox = (size_t)d.nx * d.ny * d.nz;
    const size_t n_box = (size_t)P.vox0[n_bodies], n_at = (size_t)P.n_atoms;
    const int rounds = refine ? jf_rounds(n_steps) : 1;
    A.dot_wgs = (int)std::min<size_t>(mad_ceil_div((int64_t)R.n_vox, 256), JF_DOT_WGS);

    // workgroups per body and the form of the steps kernel
    R.bodies.assign(n_bodies, JfBody());
    R.reg = !ctx->jf_no_reg;
    int g0 = 0;
    for (int b = 0; b < n_bodies; b++) {
        JfBody &B = R.bodies[b];
        memset(&B, 0, sizeof B);
        const int u = b / K, g = b % K;      // (K = 1: the body itself)
        B.n = first_atom[u + 1] - first_atom[u]; B.atom0 = first_atom[u] * K + g * B.n;
        B.G = jf_groups(ctx->n_cu, n_bodies, B.n, ctx->jf_split);
        B.g0 = g0; g0 += B.G;
        if (!jf_fits_registers(B.n, B.G)) R.reg = false;
        B.active = refine && !(fixed && fixed[u]);
        B.conv = 0; B.last = -1; B.moved = -1;
        B.edge = P.edge[b]; B.vox0 = P.vox0[b];
        for (int k = 0; k < 3; k++) { B.lo[k] = P.lo[b][k]; B.e[k] = P.e[b][k]; B.cen[k] = P.cen[b][k]; }
        B.maxd = P.max_dist[b];
        for (int i = 0; i < 9; i++) B.rot[i] = (i % 4 == 0) ? 1.0 : 0.0;
        B.step = max_step;
    }
    R.n_wgs = g0;
    // k_jf_steps_sym waits on all workgroups of a unit's images: every one of them has to be resident
    if (sym && g0 > ctx->n_cu) return mad_fail(ctx, MAD_EINVAL, "%s: n_units x n_ops: %d workgroups on %d compute units", who, g0, ctx->n_cu);
    ctx->last_jf_wgs = g0; ctx->last_jf_reg = R.reg ? 1 : 0; ctx->last_jf_G = R.bodies[0].G;

    // one block of small things: [ctl 64][arrive B x 8, padded][partial B x 2 x JF_MAX_G x 8 doubles][bodies][taps][dot][scale][operators K x 12]
    R.arrive_bytes = jf_up((size_t)n_bodies * 8);
    const size_t o_arr = 256, o_part = o_arr + R.arrive_bytes, o_body = o_part + jf_up((size_t)n_bodies * 2 * JF_MAX_G * 64);
    const size_t o_taps = o_body + jf_up((size_t)n_bodies * sizeof(JfBody)), o_dot = o_taps + jf_up((2 * JF_MAX_R + 1) * 8);
    const size_t o_scale = o_dot + jf_up((size_t)JF_DOT_WGS * 16), o_ops = o_scale + jf_up((size_t)rounds * 8), small = o_ops + jf_up((size_t)K * 96);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), small));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), n_box * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), n_box * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), R.n_vox * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), n_at * 24 * (refine ? 3 : 1) + (sym ? n_unit_atoms * 24 : 0)));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), n_at * 8));
    if (refine) MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), n_box * sizeof(float4)));
    char *sm = scratch<char>(ctx, S_TMP_G);
    A.ctl = (JfCtl *)sm; A.arrive = (unsigned long long *)(sm + o_arr); A.partial = (double *)(sm + o_part);
    A.body = (JfBody *)(sm + o_body); A.taps = (const double *)(sm + o_taps); A.dot = (double *)(sm + o_dot);
    A.scale = (double *)(sm + o_scale);
    A.n_bodies = n_bodies; A.round = 0;
    A.map = d.grid; A.nx = d.nx; A.ny = d.ny; A.nz = d.nz; A.vs = d.vs;
    for (int i = 0; i < 3; i++) {
        A.o[i] = d.o[i];
        volatile double t = d.o[i] + d.vs;      // np.arange's element step, as refine_device
        A.del[i] = t - d.o[i];
    }
    A.mass = scratch<double>(ctx, S_TMP_F);
    A.cur = scratch<double>(ctx, S_TMP_E);
    A.ini = refine ? A.cur + n_at * 3 : nullptr; A.prv = refine ? A.cur + n_at * 6 : nullptr;
    A.fix = scratch<long long>(ctx, S_TMP_A); A.bufa = scratch<double>(ctx, S_TMP_A); A.bufb = scratch<double>(ctx, S_TMP_B);
    A.M = scratch<double>(ctx, S_TMP_C);
    A.tex = refine ? scratch<float4>(ctx, S_TMP_D) : nullptr;
    A.r = P.r; A.n_steps = n_steps; A.max_step = max_step; A.min_step = min_step;
    if (sym) {      // the units' start coordinates behind the three image-sized arrays; the operators behind the scales
        double *ops = (double *)(sm + o_ops);
        R.S.K = K; R.S.n_wgs = R.n_wgs;
        R.S.op_rot = ops; R.S.op_trans = ops + 9 * (size_t)K;
        R.S.wcur = A.ini; R.S.wprv = A.prv;
        R.S.uini = A.cur + n_at * 9;
        A.ini = nullptr;
        R.image_mass.resize(n_at);
        for (int b = 0; b < n_bodies; b++)
            for (long long i = 0; i < R.bodies[b].n; i++) R.image_mass[R.bodies[b].atom0 + i] = mass[first_atom[b / K] + i];
    }

    JfCtl c;
    memset(&c, 0, sizeof c);
    c.n_moving = 0;
    for (int b = 0; b < n_bodies; b += K) c.n_moving += R.bodies[b].active;      // units (K = 1: bodies)
    if (!refine) c.n_moving = 1;      // mad_assembly_density: the model kernels run once
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // nothing of an earlier call still reads the scratch that is rewritten below
    MAD_HIP(hipMemcpyAsync(A.ctl, &c, sizeof c, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(A.body, R.bodies.data(), (size_t)n_bodies * sizeof(JfBody), hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync((void *)A.taps, P.taps, (size_t)(2 * P.r + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(sym ? (double *)R.S.uini : A.cur, atoms, n_unit_atoms * 24, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync((void *)A.mass, sym ? R.image_mass.data() : mass, n_at * 8, hipMemcpyHostToDevice, ctx->stream));
    if (sym) {
        MAD_HIP(hipMemcpyAsync((void *)R.S.op_rot, op_rot, (size_t)K * 72, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)R.S.op_trans, op_trans, (size_t)K * 24, hipMemcpyHostToDevice, ctx->stream));
    }
    MAD_HIP(hipMemsetAsync(A.scale, 0, jf_up((size_t)rounds * 8), ctx->stream));
    R.box_blocks = (unsigned)std::min<int64_t>(mad_ceil_div(P.max_box, 256), 4096);
    R.atom_blocks = (unsigned)mad_ceil_div(P.max_atoms, 256);
    R.lat_blocks = (unsigned)std::min<size_t>(mad_ceil_div((int64_t)R.n_vox, 256), (size_t)ctx->n_cu * 16);
    return MAD_OK;
}

// rho_b of the stale boxes, M, s: five launches and a memset behind one another
static int jf_model(mad_ctx *ctx, JfRun &R) {
    const JfArgs &A = R.A;
    const dim3 boxes(R.box_blocks, A.n_bodies);
    mad_timer_begin(ctx, MAD_T_JF_MODEL);
    MAD_HIP(hipMemsetAsync(A.fix, 0, (size_t)R.P.vox0[A.n_bodies] * 8, ctx->stream));
    hipLaunchKernelGGL(k_jf_splat, dim3(R.atom_blocks, A.n_bodies), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_jf_blur<true>, boxes, dim3(256), 0, ctx->stream, A, 0, (const double *)A.bufa, A.bufb);
    hipLaunchKernelGGL(k_jf_blur<false>, boxes, dim3(256), 0, ctx->stream, A, 1, (const double *)A.bufb, A.bufa);
    hipLaunchKernelGGL(k_jf_blur<false>, boxes, dim3(256), 0, ctx->stream, A, 2, (const double *)A.bufa, A.bufb);
    mad_timer_end(ctx, MAD_T_JF_MODEL);
    mad_timer_begin(ctx, MAD_T_JF_FIELD);
    hipLaunchKernelGGL(k_jf_accum, dim3(A.dot_wgs), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_jf_scale, dim3(1), dim3(256), 0, ctx->stream, A);
    MAD_HIP(hipGetLastError());
    return MAD_OK;
}

extern "C" int mad_assembly_density(mad_ctx *ctx, int n_bodies, const double *atoms, const double *mass, const int64_t *first_atom,
                                    double resolution, double *model, double *scale, float *residual) {
    if (!ctx) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    if (!scale) return mad_fail(ctx, MAD_EINVAL, "mad_assembly_density: NULL scale");
    JfRun R;
    MAD_TRY(jf_setup(ctx, "mad_assembly_density", n_bodies, atoms, mass, first_atom, nullptr, resolution, false, 1, 0.0, 0.0, R));
    MAD_TRY(jf_model(ctx, R));
    const JfArgs &A = R.A;
    if (residual) {
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), R.n_vox * 4));
        hipLaunchKernelGGL(k_jf_residual, dim3(R.lat_blocks), dim3(256), 0, ctx->stream, A, scratch<float>(ctx, S_TMP_H));
        MAD_HIP(hipGetLastError());
    }
    mad_timer_end(ctx, MAD_T_JF_FIELD);
    JfCtl c;
    MAD_HIP(hipMemcpyAsync(&c, A.ctl, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
    if (model) MAD_HIP(hipMemcpyAsync(model, A.M, R.n_vox * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (residual) MAD_HIP(hipMemcpyAsync(residual, mad_sb(ctx, S_TMP_H).p, R.n_vox * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (c.err) return mad_fail(ctx, MAD_EDOM, "mad_assembly_density: an atom inside the map lies outside its body's box");
    *scale = c.s;
    return MAD_OK;
}

// mad_assembly_refine (n_ops = 0: the n_bodies are bodies) and mad_assembly_refine_symmetric (they are units, with n_ops images each)
static int jf_refine(mad_ctx *ctx, const char *who, int n_bodies, const double *atoms, const double *mass, const int64_t *first_atom,
                     const uint8_t *fixed, bool sym, int n_ops, const double *op_rot, const double *op_trans, double resolution, int n_steps,
                     double max_step, double min_step, double *coords, double *rot, double *trans, int32_t *converged, int32_t *last_step,
                     double *scale_per_round, int32_t *n_rounds) {
    if (!ctx) return MAD_EINVAL;
    mad_use_lane(ctx, 0);
    if (!coords || !rot || !trans || !converged || !last_step || !n_rounds)
        return mad_fail(ctx, MAD_EINVAL, "%s: NULL %s", who, !coords ? "coords" : !rot ? "rot" : !trans ? "trans" : !converged ? "converged" : !last_step ? "last_step" : "n_rounds");
    JfRun R;
    MAD_TRY(jf_setup(ctx, who, n_bodies, atoms, mass, first_atom, fixed, resolution, true, n_steps, max_step, min_step, R, n_ops, op_rot, op_trans, sym));
    JfArgs &A = R.A;
    const JfSym &S = R.S;
    const int n_units = n_bodies, K = sym ? n_ops : 1;
    n_bodies = n_units * K;      // the bodies of the model: the images
    const int rounds = jf_rounds(n_steps);
    const unsigned threads = R.reg ? JF_THREADS_REG : JF_THREADS;
    MAD_HIP(hipMemsetAsync(A.arrive, 0, R.arrive_bytes, ctx->stream));
    if (sym) hipLaunchKernelGGL(k_jf_init_sym, dim3(R.n_wgs), dim3(threads), 0, ctx->stream, A, S);
    else hipLaunchKernelGGL(k_jf_init, dim3(R.n_wgs), dim3(threads), 0, ctx->stream, A);
    MAD_HIP(hipGetLastError());
    // The rounds are enqueued without a wait between them.  Every 8th round a copy of the control words is sent to pinned memory
    // behind the round; once a copy that has ARRIVED (hipEventQuery, which does not block) shows no moving body, enqueueing stops.
    // Rounds enqueued past that point return at once.
    JfCtl *seen = nullptr;
    hipEvent_t ev = nullptr;
    MAD_HIP(hipHostMalloc((void **)&seen, sizeof(JfCtl), hipHostMallocDefault));
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(seen); return mad_fail(ctx, MAD_EHIP, "%s: hipEventCreate", who); }
    bool in_flight = false;
    int rc = MAD_OK;
    for (int round = 0; round < rounds && rc == MAD_OK; round++) {
        if (in_flight && hipEventQuery(ev) == hipSuccess) {
            in_flight = false;
            if (seen->n_moving == 0) break;
        }
        A.round = round;
        rc = jf_model(ctx, R);
        if (rc != MAD_OK) break;
        hipLaunchKernelGGL(k_jf_texels, dim3(R.box_blocks, n_bodies), dim3(256), 0, ctx->stream, A);
        mad_timer_end(ctx, MAD_T_JF_FIELD);
        mad_timer_begin(ctx, MAD_T_JF_STEPS);
        if (hipMemsetAsync(A.arrive, 0, R.arrive_bytes, ctx->stream) != hipSuccess) rc = mad_fail(ctx, MAD_EHIP, "%s: hipMemsetAsync", who);
        if (sym && R.reg) hipLaunchKernelGGL(k_jf_steps_sym<JF_MAXA>, dim3(R.n_wgs), dim3(threads), 0, ctx->stream, A, S);
        else if (sym) hipLaunchKernelGGL(k_jf_steps_sym<0>, dim3(R.n_wgs), dim3(threads), 0, ctx->stream, A, S);
        else if (R.reg) hipLaunchKernelGGL(k_jf_steps<JF_MAXA>, dim3(R.n_wgs), dim3(threads), 0, ctx->stream, A);
        else hipLaunchKernelGGL(k_jf_steps<0>, dim3(R.n_wgs), dim3(threads), 0, ctx->stream, A);
        mad_timer_end(ctx, MAD_T_JF_STEPS);
        if (hipGetLastError() != hipSuccess) rc = mad_fail(ctx, MAD_EHIP, "%s: launch failed in round %d", who, round);
        if (rc == MAD_OK && !in_flight && round % 8 == 7) {
            if (hipMemcpyAsync(seen, A.ctl, sizeof(JfCtl), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && hipEventRecord(ev, ctx->stream) == hipSuccess) in_flight = true;
        }
    }
    JfCtl c;
    memset(&c, 0, sizeof c);
    const size_t n_at = (size_t)R.P.n_atoms;
    if (rc == MAD_OK) {
        hipError_t e = hipMemcpyAsync(&c, A.ctl, sizeof c, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(R.bodies.data(), A.body, (size_t)n_bodies * sizeof(JfBody), hipMemcpyDeviceToHost, ctx->stream);
        // a unit's coordinates are those of its image 0
        for (int u = 0; u < n_units && e == hipSuccess; u += sym ? 1 : n_units)
            e = hipMemcpyAsync(coords + 3 * first_atom[u], A.cur + 3 * first_atom[u] * K, (sym ? (size_t)(first_atom[u + 1] - first_atom[u]) : n_at) * 24, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && scale_per_round) e = hipMemcpyAsync(scale_per_round, A.scale, (size_t)rounds * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) rc = mad_fail(ctx, MAD_EHIP, "%s: read-back: %s", who, hipGetErrorString(e));
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    (void)hipEventDestroy(ev);
    (void)hipHostFree(seen);
    if (rc != MAD_OK) return rc;
    if (es != hipSuccess) return mad_fail(ctx, MAD_EHIP, "%s: %s", who, hipGetErrorString(es));
    if (c.err) return mad_fail(ctx, MAD_EDOM, "%s: an atom inside the map lies outside its body's box", who);
    for (int b = 0; b < n_units; b++) {
        const JfBody &B = R.bodies[(size_t)b * K];
        for (int i = 0; i < 9; i++) rot[9 * b + i] = B.rot[i];
        for (int i = 0; i < 3; i++) trans[3 * b + i] = B.trans[i];
        converged[b] = B.conv; last_step[b] = B.last;
    }
    *n_rounds = c.rounds;
    return MAD_OK;
}

extern "C" int mad_assembly_refine(mad_ctx *ctx, int n_bodies, const double *atoms, const double *mass, const int64_t *first_atom,
                                   const uint8_t *fixed, double resolution, int n_steps, double max_step, double min_step, double *coords,
                                   double *rot, double *trans, int32_t *converged, int32_t *last_step, double *scale_per_round,
                                   int32_t *n_rounds) {
    return jf_refine(ctx, "mad_assembly_refine", n_bodies, atoms, mass, first_atom, fixed, false, 0, nullptr, nullptr, resolution, n_steps, max_step,
                     min_step, coords, rot, trans, converged, last_step, scale_per_round, n_rounds);
}

// n_ops = 1 runs the symmetric kernels too: there is no dispatch to mad_assembly_refine
extern "C" int mad_assembly_refine_symmetric(mad_ctx *ctx, int n_units, const double *atoms, const double *mass, const int64_t *first_atom,
                                             const uint8_t *fixed, int n_ops, const double *op_rot, const double *op_trans, double resolution,
                                             int n_steps, double max_step, double min_step, double *coords, double *rot, double *trans,
                                             int32_t *converged, int32_t *last_step, double *scale_per_round, int32_t *n_rounds) {
    return jf_refine(ctx, "mad_assembly_refine_symmetric", n_units, atoms, mass, first_atom, fixed, true, n_ops, op_rot, op_trans, resolution,
                     n_steps, max_step, min_step, coords, rot, trans, converged, last_step, scale_per_round, n_rounds);
}

// workgroups per body of body 0, the kernel form (1: registers) and the workgroups of the steps kernel in the last refinement
extern "C" int mad_last_assembly_plan(mad_ctx *ctx, int *G, int *in_registers, int *workgroups) {
    if (!ctx) return MAD_EINVAL;
    if (G) *G = ctx->last_jf_G;
    if (in_registers) *in_registers = ctx->last_jf_reg;
    if (workgroups) *workgroups = ctx->last_jf_wgs;
    return MAD_OK;
}
