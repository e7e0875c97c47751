// mad_qscore.hip -- the Q-score of Pintilie et al. 2020 per atom of a placed model: the map sampled on 8 points of every radial shell
// that are closer to the atom than to any other atom, correlated with a fixed reference profile.  The contract is DESIGN.md section
// 4u and mad_amd/localfit.py::qscore_numpy restates it: a candidate is p_a = x_a + R * dir_a, kept iff every other atom b has
// D2 = (dx*dx + dy*dy) + dz*dz > R*R with dx = p_x - b_x (float64, no FMA: section 4i's expressions); the first point set with 8 kept
// candidates gives the shell its points, the first 8 in table order; the samples are trilinear.
//
//   qs_plan (mad_qscore_plan.h)       on the host: the checks, the per-shell tables, the cell grid over the atoms' box
//   k_qs_cell / k_qs_count / k_qs_scan / k_qs_fill_atoms / k_qs_fill_order
//                                     the atoms, and the scored entries, sorted by cell
//   k_qscore                          one wave per scored atom: its neighbours staged in LDS and sorted by distance, a lane per
//                                     candidate against the nearest, a lane per neighbour for the survivors, ballots for the
//                                     picks, 8 points x 8 corners gathered by the 64 lanes, the five sums
//   the host                          q from the three centred sums (sqrt and the division in IEEE arithmetic)
//
// Determinism: a candidate's fate is an AND over the neighbours, so neither the order of the atoms inside a cell (integer atomics
// hand out the slots) nor the order in which a wave stages or sorts them reaches a result; the picks are ballots in table order; the
// sums run over the slots [shell][point] in a fixed order (lane l adds the slots l, l + 64, ..., the lanes combine in the butterfly
// of wave_sum_f64).  No floating-point atomics; nothing depends on what ran before.
#include <algorithm>
#include <new>
#include <vector>

#include "mad_common.h"
#include "mad_qscore_plan.h"

#define QS_THREADS (QS_WAVES * MAD_WAVE)
#define QS_BIN_THREADS 256
#define QS_SCAN_THREADS 1024
#define QS_ROUND (1u << 22)     // workgroups of one launch: a grid may not have 2^32 threads
#define QS_NEAR 16              // the nearest neighbours, tested with a lane per candidate; the rest with a lane per neighbour
static_assert(QS_CHUNK % MAD_WAVE == 0, "a lane owns QS_CHUNK / 64 entries of the chunk when it is sorted");
static_assert(QS_POINTS * 8 == MAD_WAVE, "8 points x 8 corners are one wave");
static_assert(QS_MAX_TRIES * QS_POINTS <= 512, "a set is at most 8 rounds of 64 candidates");

struct QsGeo {
    int n[3];                   // voxels
    int nc[3];                  // cells
    double o[3], voxsp;
    double glo[3], h;
    int n_r, n_tries;
    double cut_max;             // cut of the last shell
};

// tab: [0] radii, [1] ref, [2] R * R, [3] cut, QS_MAX_R doubles each
#define QS_TAB_R(tab, k) ((tab)[k])
#define QS_TAB_REF(tab, k) ((tab)[QS_MAX_R + (k)])
#define QS_TAB_R2(tab, k) ((tab)[2 * QS_MAX_R + (k)])
#define QS_TAB_CUT(tab, k) ((tab)[3 * QS_MAX_R + (k)])

__global__ __launch_bounds__(QS_BIN_THREADS) void k_qs_cell(const double *__restrict__ atoms, unsigned n_atoms, const QsGeo G,
                                                            int *__restrict__ cell_of) {
    const unsigned i = blockIdx.x * QS_BIN_THREADS + threadIdx.x;
    if (i >= n_atoms) return;
    const int cx = qs_cell(atoms[3 * (size_t)i], G.glo[0], G.h, G.nc[0]), cy = qs_cell(atoms[3 * (size_t)i + 1], G.glo[1], G.h, G.nc[1]),
              cz = qs_cell(atoms[3 * (size_t)i + 2], G.glo[2], G.h, G.nc[2]);
    cell_of[i] = (cx * G.nc[1] + cy) * G.nc[2] + cz;
}

// entry j is atom index[j] (index == NULL: atom j); cnt[its cell] counts
__global__ __launch_bounds__(QS_BIN_THREADS) void k_qs_count(const int *__restrict__ cell_of, const long long *__restrict__ index, unsigned m,
                                                             unsigned *__restrict__ cnt) {
    const unsigned j = blockIdx.x * QS_BIN_THREADS + threadIdx.x;
    if (j >= m) return;
    atomicAdd(cnt + cell_of[index ? (size_t)index[j] : (size_t)j], 1u);
}

// One workgroup: start[c] = entries in the cells before c (start[n_cells] = all), cursor[c] = start[c]  (k_zone_scan's form).
__global__ __launch_bounds__(QS_SCAN_THREADS) void k_qs_scan(const unsigned *__restrict__ cnt, int n_cells, unsigned *__restrict__ start,
                                                             unsigned *__restrict__ cursor) {
    __shared__ int warp_tot[QS_SCAN_THREADS / MAD_WAVE + 1];
    const int per = (n_cells + QS_SCAN_THREADS - 1) / QS_SCAN_THREADS, c0 = threadIdx.x * per, c1 = c0 + per < n_cells ? c0 + per : n_cells;
    int s = 0;
    for (int c = c0; c < c1; c++) s += (int)cnt[c];
    int total = 0;
    int run = block_excl_scan(s, warp_tot, &total);
    for (int c = c0; c < c1; c++) {
        start[c] = (unsigned)run;
        cursor[c] = (unsigned)run;
        run += (int)cnt[c];
    }
    if (c0 < n_cells && c1 == n_cells) start[n_cells] = (unsigned)run;
}

__global__ __launch_bounds__(QS_BIN_THREADS) void k_qs_fill_atoms(const double *__restrict__ atoms, unsigned n_atoms, const int *__restrict__ cell_of,
                                                                  unsigned *__restrict__ cursor, double *__restrict__ sorted, int *__restrict__ sorted_id) {
    const unsigned i = blockIdx.x * QS_BIN_THREADS + threadIdx.x;
    if (i >= n_atoms) return;
    const size_t slot = atomicAdd(cursor + cell_of[i], 1u);
    sorted[3 * slot] = atoms[3 * (size_t)i];
    sorted[3 * slot + 1] = atoms[3 * (size_t)i + 1];
    sorted[3 * slot + 2] = atoms[3 * (size_t)i + 2];
    sorted_id[slot] = (int)i;
}

__global__ __launch_bounds__(QS_BIN_THREADS) void k_qs_fill_order(const int *__restrict__ cell_of, const long long *__restrict__ index, unsigned m,
                                                                  unsigned *__restrict__ cursor, int *__restrict__ order) {
    const unsigned j = blockIdx.x * QS_BIN_THREADS + threadIdx.x;
    if (j >= m) return;
    order[atomicAdd(cursor + cell_of[(size_t)index[j]], 1u)] = (int)j;
}

struct QsWave {
    const double *sorted;
    const int *sorted_id;
    const unsigned *start;
    int c_lo[3], c_hi[3];       // the cells around the atom's own, clipped
    int nc1, nc2;
    int self;
    double x[3];
    double cut_max;
};

// Chunk c of the atom's neighbours into nb[QS_CHUNK][4] = {x, y, z, d2}, ascending in d2: the other atoms (by index) of the 27 cells
// with d2 <= cut_max, numbered in the order of the walk, of which chunk c takes the numbers c * QS_CHUNK .. + QS_CHUNK - 1.
// -> the entries of the chunk; *total = all neighbours (only from a walk with c == 0, which is never cut short).
__device__ __forceinline__ int qs_stage(const QsWave &W, double *nb, int c, int *total) {
    const int lane = (int)lane_id(), first = c * QS_CHUNK, last = first + QS_CHUNK;
    int seen = 0;
    for (int cx = W.c_lo[0]; cx <= W.c_hi[0]; cx++)
        for (int cy = W.c_lo[1]; cy <= W.c_hi[1]; cy++) {
            const int row = (cx * W.nc1 + cy) * W.nc2;
            const unsigned a0 = W.start[row + W.c_lo[2]], a1 = W.start[row + W.c_hi[2] + 1];      // z runs fastest: one run of the sorted atoms
            for (unsigned base = a0; base < a1; base += MAD_WAVE) {
                const unsigned i = base + (unsigned)lane;
                bool keep = false;
                double b[3] = {0.0, 0.0, 0.0}, d2 = 0.0;
                if (i < a1) {
                    b[0] = W.sorted[3 * (size_t)i]; b[1] = W.sorted[3 * (size_t)i + 1]; b[2] = W.sorted[3 * (size_t)i + 2];
                    d2 = qs_d2(b, W.x);
                    keep = W.sorted_id[i] != W.self && d2 <= W.cut_max;
                }
                const unsigned long long ball = __ballot(keep);
                const int ord = seen + __popcll(ball & lanemask_lt());
                if (keep && ord >= first && ord < last) {
                    double *e = nb + 4 * (ord - first);
                    e[0] = b[0]; e[1] = b[1]; e[2] = b[2]; e[3] = d2;
                }
                seen += __popcll(ball);
            }
        }
    if (total) *total = seen;
    const int n_c = seen <= first ? 0 : (seen - first < QS_CHUNK ? seen - first : QS_CHUNK);
    // rank sort by (d2, slot): near neighbours shadow the most candidates, and a shell stops at the last one within its cut
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the lanes' writes above before the wave's reads (LDS operations of a wave execute in order)
    double own[QS_CHUNK / MAD_WAVE][4];
    int rank[QS_CHUNK / MAD_WAVE];
#pragma unroll
    for (int q = 0; q < QS_CHUNK / MAD_WAVE; q++) {
        const int e = q * MAD_WAVE + lane;
        rank[q] = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) own[q][t] = e < n_c ? nb[4 * e + t] : 0.0;
    }
    for (int a = 0; a < n_c; a++) {
        const double da = nb[4 * a + 3];      // a broadcast
#pragma unroll
        for (int q = 0; q < QS_CHUNK / MAD_WAVE; q++) {
            const int e = q * MAD_WAVE + lane;
            rank[q] += (da < own[q][3] || (da == own[q][3] && a < e)) ? 1 : 0;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // every read of the old order before the first write of the new
#pragma unroll
    for (int q = 0; q < QS_CHUNK / MAD_WAVE; q++)
        if (q * MAD_WAVE + lane < n_c) {
#pragma unroll
            for (int t = 0; t < 4; t++) nb[4 * rank[q] + t] = own[q][t];
        }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return n_c;
}

// entries of the sorted chunk with d2 <= cut
__device__ __forceinline__ int qs_within(const double *nb, int n_c, double cut) {
    int m = 0;
#pragma unroll
    for (int q = 0; q < QS_CHUNK / MAD_WAVE; q++) {
        const int e = q * MAD_WAVE + (int)lane_id();
        m += __popcll(__ballot(e < n_c && nb[4 * e + 3] <= cut));
    }
    return m;
}

// the lanes' candidates p against the first m entries of the chunk: `live` is the ballot of the candidates still kept, one scalar that
// every neighbour ANDs its ballot into; the wave leaves once it is 0
__device__ __forceinline__ unsigned long long qs_test(const double *nb, int m, const double p[3], double r2, unsigned long long live) {
    for (int a = 0; a < m && live != 0ull; a++) {      // every lane reads the same address: a broadcast
        const double dx = p[0] - nb[4 * a], dy = p[1] - nb[4 * a + 1], dz = p[2] - nb[4 * a + 2];
        const double D2 = (dx * dx + dy * dy) + dz * dz;
        live &= __ballot(D2 > r2);
    }
    return live;
}

// v of lane l (uniform) in every lane
__device__ __forceinline__ double qs_bcast(double v, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Wave w0 + (its number in the grid) takes entry j = order[.] of the scored list: atom index[j] (index == NULL: atom j).  Outputs at
// row j: n_out[j] = samples, sums[3 j ..] = {sum du dv, sum du du, sum dv dv}; tries_used [n_r], picked [n_r][8], values [n_r][8] where
// the pointers are not NULL.
__global__ __launch_bounds__(QS_THREADS) void k_qscore(const float *__restrict__ g, const double *__restrict__ atoms, const double *__restrict__ sorted,
                                                       const int *__restrict__ sorted_id, const unsigned *__restrict__ start,
                                                       const int *__restrict__ cell_of, const long long *__restrict__ index,
                                                       const int *__restrict__ order, unsigned m_scored, const double *__restrict__ tab,
                                                       const double *__restrict__ dirs, const QsGeo G, int *__restrict__ n_out,
                                                       double *__restrict__ sums, int *__restrict__ tries_out, int *__restrict__ picked_out,
                                                       double *__restrict__ values_out, unsigned w0) {
    __shared__ double s_nb[QS_WAVES][QS_CHUNK * 4];
    __shared__ double s_val[QS_WAVES][QS_MAX_R * QS_POINTS];
    __shared__ int s_pick[QS_WAVES][QS_POINTS];
    __shared__ int s_np[QS_WAVES][QS_MAX_R];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)lane_id();      // the wave's number, known to be uniform: the atom, its cells and every loop bound below live in scalar registers
    const unsigned long long w = (unsigned long long)w0 + (unsigned long long)blockIdx.x * QS_WAVES + (unsigned)wv;
    if (w >= m_scored) return;      // the whole wave; the kernel has no workgroup barrier
    double *nb = s_nb[wv], *val = s_val[wv];
    int *pick = s_pick[wv], *np = s_np[wv];
    const int j = order[w];
    const size_t atom = index ? (size_t)index[j] : (size_t)j;

    QsWave W;
    W.sorted = sorted; W.sorted_id = sorted_id; W.start = start;
    W.nc1 = G.nc[1]; W.nc2 = G.nc[2];
    W.self = (int)atom;
    W.cut_max = G.cut_max;
    {
        const int cell = cell_of[atom];
        const int c3[3] = {cell / (G.nc[1] * G.nc[2]), (cell / G.nc[2]) % G.nc[1], cell % G.nc[2]};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            W.x[a] = atoms[3 * atom + a];
            W.c_lo[a] = c3[a] > 0 ? c3[a] - 1 : 0;
            W.c_hi[a] = c3[a] < G.nc[a] - 1 ? c3[a] + 1 : G.nc[a] - 1;
        }
    }
    int total = 0;
    int n_c = qs_stage(W, nb, 0, &total);
    const int n_chunks = (total + QS_CHUNK - 1) / QS_CHUNK;      // with one chunk (or none) the staging above serves every shell
    double far[QS_CHUNK / MAD_WAVE][3];      // one chunk: the lane's own entries of it, for the tests with a lane per neighbour
#pragma unroll
    for (int q = 0; q < QS_CHUNK / MAD_WAVE; q++) {
        const int e = q * MAD_WAVE + lane;
#pragma unroll
        for (int t = 0; t < 3; t++) far[q][t] = e < n_c ? nb[4 * e + t] : 0.0;
    }

    const int pt = lane >> 3, cx = (lane >> 2) & 1, cy = (lane >> 1) & 1, cz = lane & 1;
    for (int k = 0; k < G.n_r; k++) {
        const double R = QS_TAB_R(tab, k), r2 = QS_TAB_R2(tab, k), cut = QS_TAB_CUT(tab, k);
        int npk = QS_POINTS, used = 0;
        if (R > 0.0) {
            const int m_one = n_chunks <= 1 ? qs_within(nb, n_c, cut) : 0, m_near = m_one < QS_NEAR ? m_one : QS_NEAR;
            npk = 0;
            for (int t = 1; t <= G.n_tries; t++) {
                const int n_set = QS_POINTS * t, off = 4 * t * (t - 1);
                int got = 0;      // the carry across the rounds of a set larger than 64
                for (int r0 = 0; r0 < n_set && got < QS_POINTS; r0 += MAD_WAVE) {
                    const int ci = r0 + lane;
                    const bool valid = ci < n_set;
                    const size_t di = (size_t)(off + (valid ? ci : 0));
                    const double p[3] = {W.x[0] + R * dirs[3 * di], W.x[1] + R * dirs[3 * di + 1], W.x[2] + R * dirs[3 * di + 2]};
                    // a lane per candidate against the nearest neighbours, which shadow most of them
                    unsigned long long live = __ballot(valid);
                    if (n_chunks <= 1) live = qs_test(nb, m_near, p, r2, live);
                    else
                        for (int c = 0; c < n_chunks && live != 0ull; c++) {      // more neighbours than a chunk: every chunk again for every round
                            n_c = qs_stage(W, nb, c, nullptr);
                            live = qs_test(nb, qs_within(nb, n_c, cut), p, r2, live);      // the kept mask ANDed across the chunks
                        }
                    // the survivors in table order, each against the rest of the chunk with a lane per neighbour (the same expression on
                    // the same operands: the same decision), until the shell has its points
                    while (live != 0ull && got < QS_POINTS) {
                        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
                        live &= live - 1ull;
                        if (m_one > QS_NEAR) {      // (one chunk)
                            const double c0 = qs_bcast(p[0], l), c1 = qs_bcast(p[1], l), c2 = qs_bcast(p[2], l);
                            bool hit = false;
#pragma unroll
                            for (int q = 0; q < QS_CHUNK / MAD_WAVE; q++) {
                                const int e = q * MAD_WAVE + lane;
                                const double dx = c0 - far[q][0], dy = c1 - far[q][1], dz = c2 - far[q][2];
                                const double D2 = (dx * dx + dy * dy) + dz * dz;
                                hit = hit || (e >= QS_NEAR && e < m_one && !(D2 > r2));
                            }
                            if (__ballot(hit) != 0ull) continue;
                        }
                        if (lane == 0) pick[got] = off + r0 + l;
                        got++;
                    }
                }
                if (got >= QS_POINTS || t == G.n_tries) {
                    used = t;
                    npk = got;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the picks before their readers
        }
        // 8 points x 8 corners
        const bool have = pt < npk;
        const int di = (R > 0.0 && have) ? pick[pt] : -1;
        double f[3];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double p = di >= 0 ? W.x[a] + R * dirs[3 * (size_t)di + a] : W.x[a];
            f[a] = (p - G.o[a]) / G.voxsp;
            inside = inside && f[a] >= -1.0 && f[a] <= (double)G.n[a];
        }
        double tq[3] = {0.0, 0.0, 0.0}, v = 0.0;
        if (inside) {
            const double fl[3] = {floor(f[0]), floor(f[1]), floor(f[2])};
            const int ix = (int)fl[0] + cx, iy = (int)fl[1] + cy, iz = (int)fl[2] + cz;      // -1 .. n + 1
#pragma unroll
            for (int a = 0; a < 3; a++) tq[a] = f[a] - fl[a];
            if (have && ix >= 0 && ix < G.n[0] && iy >= 0 && iy < G.n[1] && iz >= 0 && iz < G.n[2])
                v = (double)g[((size_t)ix * (size_t)G.n[1] + (size_t)iy) * (size_t)G.n[2] + (size_t)iz];
        }
        // along z, then y, then x: the lane of corner (0, 0, 0) ends with the sample
        double hi = __shfl_xor(v, 1, MAD_WAVE);
        v = v + tq[2] * (hi - v);
        hi = __shfl_xor(v, 2, MAD_WAVE);
        v = v + tq[1] * (hi - v);
        hi = __shfl_xor(v, 4, MAD_WAVE);
        v = v + tq[0] * (hi - v);
        if (!(have && inside)) v = 0.0;
        if ((lane & 7) == 0) {
            val[k * QS_POINTS + pt] = v;
            if (picked_out) picked_out[((size_t)j * G.n_r + k) * QS_POINTS + pt] = di;
            if (values_out) values_out[((size_t)j * G.n_r + k) * QS_POINTS + pt] = v;
        }
        if (lane == 0) {
            np[k] = npk;
            if (tries_out) tries_out[(size_t)j * G.n_r + k] = used;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // pick[] is read before the next shell rewrites it
    }

    // the score's sums over the slots [shell][point]; a slot without a point adds 0
    const int n_slots = G.n_r * QS_POINTS;
    int n = 0;
    double su = 0.0, sv = 0.0;
    for (int s = lane; s < n_slots; s += MAD_WAVE) {
        const bool has = (s & 7) < np[s >> 3];
        n += has ? 1 : 0;
        su += has ? val[s] : 0.0;
        sv += has ? QS_TAB_REF(tab, s >> 3) : 0.0;
    }
    n = wave_sum_i32(n);
    su = wave_sum_f64(su);
    sv = wave_sum_f64(sv);
    const double mu = su / (double)n, mv = sv / (double)n;
    double suv = 0.0, suu = 0.0, svv = 0.0;
    for (int s = lane; s < n_slots; s += MAD_WAVE) {
        const bool has = (s & 7) < np[s >> 3];
        const double du = has ? val[s] - mu : 0.0, dv = has ? QS_TAB_REF(tab, s >> 3) - mv : 0.0;
        suv += du * dv;
        suu += du * du;
        svv += dv * dv;
    }
    suv = wave_sum_f64(suv);
    suu = wave_sum_f64(suu);
    svv = wave_sum_f64(svv);
    if (lane == 0) {
        n_out[j] = n;
        sums[3 * (size_t)j] = suv;
        sums[3 * (size_t)j + 1] = suu;
        sums[3 * (size_t)j + 2] = svv;
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

extern "C" int mad_map_qscore(mad_ctx *ctx, const float *grid, const int32_t dims[3], const double origin[3], double voxsp, const double *atoms,
                              int64_t n_atoms, const int64_t *index, int64_t n_index, const double *radii, const double *ref, int32_t n_r,
                              const double *dirs, int32_t n_tries, double *q, int32_t *n_samples, int32_t *tries_used, int32_t *picked,
                              double *values) {
    const char *who = "mad_map_qscore";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    QsPlan P;
    char msg[256];
    if (!qs_plan(dims, origin, voxsp, atoms, n_atoms, index, n_index, radii, ref, n_r, dirs, n_tries, P, msg, sizeof(msg)))
        return mad_fail(ctx, MAD_EINVAL, "%s", msg);
    if (P.n_atoms == 0 || P.n_scored == 0) return MAD_OK;
    if (!q || !n_samples) return mad_fail(ctx, MAD_EINVAL, "%s: NULL output", who);

    QsGeo G;
    memset(&G, 0, sizeof(G));
    for (int a = 0; a < 3; a++) { G.n[a] = P.n[a]; G.nc[a] = P.nc[a]; G.o[a] = P.o[a]; G.glo[a] = P.glo[a]; }
    G.voxsp = P.voxsp; G.h = P.h; G.n_r = P.n_r; G.n_tries = P.n_tries; G.cut_max = P.cut[P.n_r - 1];
    double h_tab[4 * QS_MAX_R];
    memset(h_tab, 0, sizeof(h_tab));
    for (int k = 0; k < P.n_r; k++) {
        h_tab[k] = radii[k]; h_tab[QS_MAX_R + k] = ref[k]; h_tab[2 * QS_MAX_R + k] = P.r2[k]; h_tab[3 * QS_MAX_R + k] = P.cut[k];
    }
    const size_t n_vox = (size_t)dims[0] * dims[1] * dims[2], n = (size_t)P.n_atoms, m = (size_t)P.n_scored, nr = (size_t)P.n_r;
    const size_t bytes_tab = (((size_t)P.n_cells + 1) * 4 + 63) & ~(size_t)63;
    const size_t bytes_dirs = ((size_t)P.n_dirs * 24 + 63) & ~(size_t)63;
    const size_t bytes_n = (m * 4 + 63) & ~(size_t)63;
    const size_t bytes_tries = tries_used ? (m * nr * 4 + 63) & ~(size_t)63 : 0, bytes_picked = picked ? (m * nr * QS_POINTS * 4 + 63) & ~(size_t)63 : 0,
                 bytes_values = values ? m * nr * QS_POINTS * 8 : 0;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n_vox + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), (n + 1) * 24));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), (n + 1) * 24));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_C), (n + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_D), (n + 1) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_E), (m + 1) * 12));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_F), bytes_n + m * 24));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), 4 * bytes_tab));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), bytes_dirs + sizeof(h_tab)));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_J), bytes_tries + bytes_picked + bytes_values + 64));
    float *d_g = scratch<float>(ctx, S_TMP_H);
    double *d_atoms = scratch<double>(ctx, S_TMP_A), *d_sorted = scratch<double>(ctx, S_TMP_B);
    int *d_cell_of = scratch<int>(ctx, S_TMP_C), *d_sorted_id = scratch<int>(ctx, S_TMP_D);
    long long *d_index = scratch<long long>(ctx, S_TMP_E);
    int *d_order = (int *)(d_index + m);
    int *d_n = scratch<int>(ctx, S_TMP_F);
    double *d_sums = (double *)(scratch<char>(ctx, S_TMP_F) + bytes_n);
    char *blk = scratch<char>(ctx, S_TMP_G);
    unsigned *d_cnt = (unsigned *)blk, *d_start = (unsigned *)(blk + bytes_tab), *d_cursor = (unsigned *)(blk + 2 * bytes_tab),
             *d_start_m = (unsigned *)(blk + 3 * bytes_tab);
    double *d_dirs = scratch<double>(ctx, S_TMP_I), *d_tab = (double *)(scratch<char>(ctx, S_TMP_I) + bytes_dirs);
    char *det = scratch<char>(ctx, S_TMP_J);
    int *d_tries = tries_used ? (int *)det : nullptr, *d_picked = picked ? (int *)(det + bytes_tries) : nullptr;
    double *d_values = values ? (double *)(det + bytes_tries + bytes_picked) : nullptr;
    static_assert(sizeof(long long) == sizeof(int64_t), "index crosses the bus as it is");

    MAD_HIP(hipMemcpyAsync(d_g, grid, n_vox * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_atoms, atoms, n * 24, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_dirs, dirs, (size_t)P.n_dirs * 24, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_tab, h_tab, sizeof(h_tab), hipMemcpyHostToDevice, ctx->stream));
    if (index) MAD_HIP(hipMemcpyAsync(d_index, index, m * 8, hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_QSCORE);
    const unsigned blocks_n = (unsigned)mad_ceil_div((int64_t)n, QS_BIN_THREADS), blocks_m = (unsigned)mad_ceil_div((int64_t)m, QS_BIN_THREADS);
    MAD_HIP(hipMemsetAsync(d_cnt, 0, bytes_tab, ctx->stream));
    hipLaunchKernelGGL(k_qs_cell, dim3(blocks_n), dim3(QS_BIN_THREADS), 0, ctx->stream, (const double *)d_atoms, (unsigned)n, G, d_cell_of);
    hipLaunchKernelGGL(k_qs_count, dim3(blocks_n), dim3(QS_BIN_THREADS), 0, ctx->stream, (const int *)d_cell_of, (const long long *)nullptr, (unsigned)n, d_cnt);
    hipLaunchKernelGGL(k_qs_scan, dim3(1), dim3(QS_SCAN_THREADS), 0, ctx->stream, (const unsigned *)d_cnt, P.n_cells, d_start, d_cursor);
    hipLaunchKernelGGL(k_qs_fill_atoms, dim3(blocks_n), dim3(QS_BIN_THREADS), 0, ctx->stream, (const double *)d_atoms, (unsigned)n, (const int *)d_cell_of,
                       d_cursor, d_sorted, d_sorted_id);
    const int *d_order_used = d_sorted_id;      // every atom is scored: the sorted atoms are the order
    if (index) {      // the scored entries by cell, with a start table of their own (d_start stays the atoms')
        MAD_HIP(hipMemsetAsync(d_cnt, 0, bytes_tab, ctx->stream));
        hipLaunchKernelGGL(k_qs_count, dim3(blocks_m), dim3(QS_BIN_THREADS), 0, ctx->stream, (const int *)d_cell_of, (const long long *)d_index, (unsigned)m, d_cnt);
        hipLaunchKernelGGL(k_qs_scan, dim3(1), dim3(QS_SCAN_THREADS), 0, ctx->stream, (const unsigned *)d_cnt, P.n_cells, d_start_m, d_cursor);
        hipLaunchKernelGGL(k_qs_fill_order, dim3(blocks_m), dim3(QS_BIN_THREADS), 0, ctx->stream, (const int *)d_cell_of, (const long long *)d_index, (unsigned)m,
                           d_cursor, d_order);
        d_order_used = d_order;
    }
    const unsigned long long n_wg = (unsigned long long)mad_ceil_div((int64_t)m, QS_WAVES);
    for (unsigned long long wg0 = 0; wg0 < n_wg; wg0 += QS_ROUND) {
        const unsigned wgs = (unsigned)std::min<unsigned long long>(QS_ROUND, n_wg - wg0);
        hipLaunchKernelGGL(k_qscore, dim3(wgs), dim3(QS_THREADS), 0, ctx->stream, (const float *)d_g, (const double *)d_atoms, (const double *)d_sorted,
                           (const int *)d_sorted_id, (const unsigned *)d_start, (const int *)d_cell_of, index ? (const long long *)d_index : nullptr,
                           d_order_used, (unsigned)m, (const double *)d_tab, (const double *)d_dirs, G, d_n, d_sums, d_tries, d_picked, d_values,
                           (unsigned)(wg0 * QS_WAVES));
    }
    mad_timer_end(ctx, MAD_T_QSCORE);
    MAD_HIP(hipGetLastError());
    std::vector<double> h_sums;
    try {
        h_sums.resize(3 * m);
    } catch (const std::bad_alloc &) {
        return mad_fail(ctx, MAD_ENOMEM, "%s: no host memory for the sums of %zu atoms", who, m);
    }
    MAD_HIP(hipMemcpyAsync(n_samples, d_n, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(h_sums.data(), d_sums, m * 24, hipMemcpyDeviceToHost, ctx->stream));
    if (tries_used) MAD_HIP(hipMemcpyAsync(tries_used, d_tries, m * nr * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (picked) MAD_HIP(hipMemcpyAsync(picked, d_picked, m * nr * QS_POINTS * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (values) MAD_HIP(hipMemcpyAsync(values, d_values, m * nr * QS_POINTS * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t j = 0; j < m; j++) {
        const double suv = h_sums[3 * j], suu = h_sums[3 * j + 1], svv = h_sums[3 * j + 2];
        q[j] = (n_samples[j] < 2 || suu == 0.0 || svv == 0.0) ? (double)NAN : suv / (sqrt(suu) * sqrt(svv));
    }
    return MAD_OK;
}
