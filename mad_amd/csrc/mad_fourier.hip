// mad_fourier.hip -- Fourier shell correlation of two maps (mad_map_fsc), the 3-D transform under it (mad_map_fft), radial filters
// (mad_map_filter, mad_map_ifft), the scan of a model over every translation of a map (mad_map_scan) and over rotations as well
// (mad_map_search, mad_map_rotate).
// DESIGN.md section 4l has the contract; mad_amd/fourier.py restates it with numpy.
//
// Both float32 grids go onto ONE cubic complex128 lattice of edge N (a power of two, 8 .. 1024): grid 1 in the real part, grid 2
// in the imaginary part, zero elsewhere (k_fft_pack).  Three passes of in-place 1-D transforms (k_fft_lines, one form per axis)
// give Z = FFT(g1 + i g2); k_fsc_shells separates the two spectra, F1(k) = (Z(k) + conj Z(-k)) / 2 and
// F2(k) = (Z(k) - conj Z(-k)) / (2i), and sums |F1|^2, |F2|^2 and Re(F1 conj(F2 phi)) per shell; k_fsc_sum adds the workgroups'
// tables.  All arithmetic is float64 without fused multiply-adds; no FFT library is linked.
//
// k_fft_lines.  A workgroup transforms a TILE of FFT_L = 8 lines of length N held in LDS.  For the x and y passes the eight lines
// are eight neighbouring z, so that every global access is a full 128-byte piece (8 complex128); for the z pass they are eight
// neighbouring y, one contiguous run of 8 N elements.  The LDS image is [n][line] with a row of ROW elements: element n of a line
// sits next to element n of the neighbouring lines, a butterfly's lanes run over the line index first, and eight lanes always
// touch 128 contiguous bytes -- whatever power of two separates the n of two lanes, it never separates their banks.  ROW = 8 does
// that for the x and y passes.  In the z pass the tile is FILLED along n (lane k writes row k): with ROW = 8 the eight lanes of a
// 16-byte store group would all land on the same four banks, so its rows are padded to ROW = 9 elements (row k begins k * 144 bytes
// in: eight consecutive rows begin on eight different 16-byte slots of the 128-byte store window).
// The transform is a radix-4 Stockham scheme (decimation in frequency; autosort, no bit reversal) with one radix-2 stage at the
// end when log2 N is odd.  A stage reads butterfly j's inputs at j + k N / 4 (k = 0 .. 3), the same places in every stage, and
// writes its outputs at q + s (4 p + k) with j = p s + q, s = 4^stage.  Instead of a second LDS image every thread takes all the
// inputs of its BPT butterflies into registers, the workgroup meets at a barrier, and then the outputs go back into the same
// image: a tile of 8 x 1024 is 128 KiB (144 KiB padded) and fits the CU's 160 KiB once, not twice.
// Twiddles exp(-2 pi i k / N) come from a table the host computes (angles reduced exactly to the first octant before cos / sin),
// uploaded once per N; w, w^2 and w^3 are three table reads, not products.  The order of every sum is fixed by the indices alone:
// the same input gives the same bits every run.
//
// k_fsc_shells.  A wave takes a brick of 2 x 4 x 8 lattice points (8 along z: 128-byte pieces of Z(k); Z(-k) is the mirrored
// brick).  A brick spans at most 9 shells: the lanes leave their terms in the wave's staging rows in LDS, lane 16 q + d adds those
// of shell smin + d among lanes 16 q .. 16 q + 15 in lane order, and lane d adds the four quarters in order into the WAVE's own
// table in LDS (no cross-lane shuffles: sixteen broadcast reads per lane).  Waves take bricks in a fixed order, a workgroup adds
// its four tables in order into its slot of the partial tables, and k_fsc_sum adds the slots in order: no floating-point
// atomics anywhere, the same bits every run.
//
// Radial filters (mad_map_filter) and the inverse transform (mad_map_ifft): DESIGN.md section 4m.  The grids sit at lattice index
// (0, 0, 0), Z = FFT(g1 + i g2) as above; k_fft_gain multiplies Z(k) by a real gain looked up by r2 = |k|^2 and conjugates, the same
// three k_fft_lines passes follow (ifft(X) = conj(FFT(conj X)) / N^3), and k_fft_unpack writes Re Z / N^3 over grid 1's box and
// -(Im Z) / N^3 over grid 2's as float32.  A gain that depends on r2 alone is real and even, so the two maps stay apart.
//
// The translation scan (mad_map_scan: k_scan_pack, k_scan_product, k_scan_score, k_scan_peaks) and the
// rotational search (mad_map_search: k_search_rotate, k_search_stats, k_search_score and the pruned form of k_fft_lines; section 4o)
// are at the end of the file.  They are one correlation: the score of an offset and the rule that keeps the best one are stated once
// (scan_score_at, scan_keep), and so is the host's set-up (CorrPlan and the corr_ functions); the scan adds its templates' statistics
// from the host, the search its rotations, their records on the device and the pruned passes.
//
// On the host every entry point owns its lattices through a `Lattices`, which waits for the stream and frees them on every way out.
#include <algorithm>
#include <vector>

#include "mad_fft_common.h"

#define FFT_L 8                 // lines per tile
#define FFT_MIN_N 8
#define FFT_MAX_N 1024
#define FFT_MAX_THREADS 512
#define FSC_THREADS 256
#define FSC_MAX_WGS 1024        // partial tables (fewer when the lattice has fewer than 4 bricks per workgroup)

// ---------------------------------------------------------------------------
// the lattice
// ---------------------------------------------------------------------------

struct PackArgs {
    const float *g1, *g2;       // g2 may be NULL
    int d1[3], d2[3];
    int p1[3], p2[3];           // lattice index of voxel (0, 0, 0) of either grid
    int logN;
};

__global__ __launch_bounds__(256) void k_fft_pack(const PackArgs A, double2 *__restrict__ Z) {
    const int logN = A.logN;
    const unsigned m = (1u << logN) - 1u;
    const size_t n = (size_t)1 << (3 * logN);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned c = (unsigned)i & m, b = (unsigned)(i >> logN) & m, a = (unsigned)(i >> (2 * logN));
        double2 v = make_double2(0.0, 0.0);
        const unsigned x1 = a - (unsigned)A.p1[0], y1 = b - (unsigned)A.p1[1], z1 = c - (unsigned)A.p1[2];      // below the start: wraps past any extent
        if (x1 < (unsigned)A.d1[0] && y1 < (unsigned)A.d1[1] && z1 < (unsigned)A.d1[2])
            v.x = (double)A.g1[((size_t)x1 * A.d1[1] + y1) * A.d1[2] + z1];
        if (A.g2) {
            const unsigned x2 = a - (unsigned)A.p2[0], y2 = b - (unsigned)A.p2[1], z2 = c - (unsigned)A.p2[2];
            if (x2 < (unsigned)A.d2[0] && y2 < (unsigned)A.d2[1] && z2 < (unsigned)A.d2[2])
                v.y = (double)A.g2[((size_t)x2 * A.d2[1] + y2) * A.d2[2] + z2];
        }
        Z[i] = v;
    }
}

// ---------------------------------------------------------------------------
// 1-D transforms
// ---------------------------------------------------------------------------

// (c_add, c_sub, c_mul, c_muli and the host's unit_root: mad_fft_common.h)

// AXIS 0 / 1 / 2: lines along x / y / z.  One workgroup per tile, N^2 / 8 tiles; blockDim.x * BPT = max(2 N, 64) butterflies of a
// radix-4 stage (a thread of the smallest lattices may have none).  Dynamic LDS: N * ROW * 16 bytes.
// PRUNE (mad_map_search): a 2-D grid selects a corner of the tile grid -- tile = blockIdx.y * (N / 8) +
// blockIdx.x, i.e. blockIdx.x is the tile along z (AXIS 2: along y) and blockIdx.y the plane (AXIS 0: y, AXIS 1 and 2: x) -- and the
// third argument carries the live length above its low byte (live << 8 | logN): elements n >= live of a line are taken as +0, not
// loaded.  Every tile is still written whole.  The other forms take neither an argument nor a branch for it.
template <int AXIS, int BPT, bool PRUNE = false>
__global__ __launch_bounds__(FFT_MAX_THREADS) void k_fft_lines(double2 *__restrict__ Z, const double2 *__restrict__ tw, int logN) {
    extern __shared__ __attribute__((aligned(16))) double2 fft_img[];
    constexpr int ROW = AXIS == 2 ? FFT_L + 1 : FFT_L;
    int live = 0;
    if (PRUNE) { live = logN >> 8; logN &= 255; }
    const int N = 1 << logN, T = (int)blockDim.x, t = (int)threadIdx.x;
    const int tile = PRUNE ? (int)(blockIdx.y << (logN - 3)) + (int)blockIdx.x : (int)blockIdx.x;
    size_t base, sN, sL;
    if (AXIS == 2) {
        base = (size_t)tile * FFT_L << logN; sN = 1; sL = (size_t)N;
    } else {
        const size_t z0 = (size_t)(tile & ((N >> 3) - 1)) << 3, u = (size_t)(tile >> (logN - 3));
        if (AXIS == 0) { base = (u << logN) + z0; sN = (size_t)N << logN; }      // u = y
        else { base = (u << (2 * logN)) + z0; sN = (size_t)N; }                    // u = x
        sL = 1;
    }
    const int E = FFT_L << logN;
#pragma unroll 4
    for (int e = t; e < E; e += T) {
        const int n = AXIS == 2 ? (e & (N - 1)) : (e >> 3), l = AXIS == 2 ? (e >> logN) : (e & 7);
        if (!PRUNE || n < live) fft_img[n * ROW + l] = Z[base + (size_t)n * sN + (size_t)l * sL];
        else fft_img[n * ROW + l] = make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int quarter = N >> 2, nb = 2 * N;      // butterflies of a radix-4 stage in the tile
    int len = N, ls = 0;
    for (; len >= 4; len >>= 2, ls += 2) {
        const int s = 1 << ls;
        double2 r[BPT][4];
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            const int bi = i * T + t;
            if (bi < nb) {
                const int l = bi & 7, j = bi >> 3;
#pragma unroll
                for (int k = 0; k < 4; k++) r[i][k] = fft_img[(j + k * quarter) * ROW + l];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            const int bi = i * T + t;
            if (bi < nb) {
                const int l = bi & 7, j = bi >> 3, q = j & (s - 1), ps = j - q;      // ps = p s: the twiddle of p / len is tw[p s]
                const double2 w1 = tw[ps], w2 = tw[2 * ps], w3 = tw[3 * ps];
                const double2 apc = c_add(r[i][0], r[i][2]), amc = c_sub(r[i][0], r[i][2]);
                const double2 bpd = c_add(r[i][1], r[i][3]), jbmd = c_muli(c_sub(r[i][1], r[i][3]));
                const int o = q + 4 * ps;
                fft_img[o * ROW + l] = c_add(apc, bpd);
                fft_img[(o + s) * ROW + l] = c_mul(w1, c_sub(amc, jbmd));
                fft_img[(o + 2 * s) * ROW + l] = c_mul(w2, c_sub(apc, bpd));
                fft_img[(o + 3 * s) * ROW + l] = c_mul(w3, c_add(amc, jbmd));
            }
        }
        __syncthreads();
    }
    if (len == 2) {      // log2 N odd: one radix-2 stage, every pair read and written by one thread
        const int half = N >> 1;
#pragma unroll
        for (int i = 0; i < 2 * BPT; i++) {
            const int bi = i * T + t;
            if (bi < 2 * nb) {
                const int l = bi & 7, j = bi >> 3;
                const double2 a = fft_img[j * ROW + l], b = fft_img[(j + half) * ROW + l];
                fft_img[j * ROW + l] = c_add(a, b);
                fft_img[(j + half) * ROW + l] = c_sub(a, b);
            }
        }
        __syncthreads();
    }
#pragma unroll 4
    for (int e = t; e < E; e += T) {
        const int n = AXIS == 2 ? (e & (N - 1)) : (e >> 3), l = AXIS == 2 ? (e >> logN) : (e & 7);
        Z[base + (size_t)n * sN + (size_t)l * sL] = fft_img[n * ROW + l];
    }
}

// ---------------------------------------------------------------------------
// filters and the inverse transform
// ---------------------------------------------------------------------------

// Z(k) <- (Re Z g, -(Im Z g)), g = gain[r2(k)], r2 = i^2 + j^2 + k^2 over the signed frequencies (a if a < N / 2, else a - N);
// gain NULL: g = scale for every k (scale 1.0: the conjugate alone, the same bits).  Every 16-byte element is read and written once,
// coalesced along z.  The gain is an 8-byte gather that within a z line spans (N / 2)^2 + 1 entries, a cache line per lane beyond
// the first few z: it, not the stream, set the kernel's time when every element made its own.  The lines (a, b), (N - a, b),
// (a, N - b) and (N - a, N - b) have the same r2 at every z, so a workgroup takes a piece of all four and gathers once for them:
// blockIdx.y = a and blockIdx.z = b run over 0 .. N / 2 (index N / 2 is the frequency -N / 2, its own mirror image, as 0 is), and
// blockIdx.x * blockDim.x + threadIdx.x = z with blockDim.x = min(N, 256).
__global__ __launch_bounds__(256) void k_fft_gain(double2 *__restrict__ Z, const double *__restrict__ gain, double scale, int logN) {
    const int N = 1 << logN, half = N >> 1;
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x), a = (int)blockIdx.y, b = (int)blockIdx.z;
    if (c >= N || a > half || b > half) return;
    const int fk = c < half ? c : c - N;
    const double g = gain ? gain[a * a + b * b + fk * fk] : scale;      // at most 3 (N / 2)^2 = 786 432
    const int a2 = (N - a) & (N - 1), b2 = (N - b) & (N - 1);
    const bool ma = a2 != a, mb = b2 != b;      // uniform over the workgroup
    const size_t i0 = (((((size_t)a) << logN) + b) << logN) + c, i1 = (((((size_t)a2) << logN) + b) << logN) + c;
    const size_t i2 = (((((size_t)a) << logN) + b2) << logN) + c, i3 = (((((size_t)a2) << logN) + b2) << logN) + c;
    const double2 z = make_double2(0.0, 0.0);
    const double2 v0 = Z[i0], v1 = ma ? Z[i1] : z, v2 = mb ? Z[i2] : z, v3 = ma && mb ? Z[i3] : z;
    Z[i0] = make_double2(v0.x * g, -(v0.y * g));
    if (ma) Z[i1] = make_double2(v1.x * g, -(v1.y * g));
    if (mb) Z[i2] = make_double2(v2.x * g, -(v2.y * g));
    if (ma && mb) Z[i3] = make_double2(v3.x * g, -(v3.y * g));
}

// out[x][y][z] = (float)(Re Z(x, y, z) * scale) (IMAG: -(Im Z) * scale) over the box d at lattice index (0, 0, 0): one output
// voxel per lane, runs of d[2] lattice elements along z read, float32 written coalesced.  n = d[0] d[1] d[2] < 2^32.
template <bool IMAG>
__global__ __launch_bounds__(256) void k_fft_unpack(const double2 *__restrict__ Z, int logN, double scale, float *__restrict__ out,
                                                    unsigned d1, unsigned d2, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned j = (unsigned)i, t = j / d2, z = j - t * d2, x = t / d1, y = t - x * d1;
        const double2 v = Z[(((((size_t)x) << logN) + y) << logN) + z];
        out[i] = (float)(IMAG ? -v.y * scale : v.x * scale);
    }
}

// ---------------------------------------------------------------------------
// shells
// ---------------------------------------------------------------------------

// part_f [workgroup][shell][3] = P1, P2, C; part_i [workgroup][shell] = lattice points.  Dynamic LDS: 4 waves x (N / 2 + 1) shells
// x (3 doubles + 1 int), besides 14 KiB of static staging rows.  phi [3][N]: the phase ramp per axis.
__global__ __launch_bounds__(FSC_THREADS) void k_fsc_shells(const double2 *__restrict__ Z, const double2 *__restrict__ phi, int logN,
                                                            double *__restrict__ part_f, long long *__restrict__ part_i) {
    extern __shared__ __attribute__((aligned(16))) double fsc_tab[];
    // staging rows per wave: every lane's three terms and shell, then the sums of the four quarters of the wave per shell offset
    __shared__ double st_v[FSC_THREADS / MAD_WAVE][MAD_WAVE][3], st_p[FSC_THREADS / MAD_WAVE][4][16][3];
    __shared__ int st_s[FSC_THREADS / MAD_WAVE][MAD_WAVE], st_n[FSC_THREADS / MAD_WAVE][4][16];
    const int N = 1 << logN, SH = (N >> 1) + 1, W = FSC_THREADS / MAD_WAVE;
    double *acc = fsc_tab;                          // [W][SH][3]
    int *cnt = (int *)(fsc_tab + W * SH * 3);       // [W][SH]
    for (int i = threadIdx.x; i < W * SH * 3; i += FSC_THREADS) acc[i] = 0.0;
    for (int i = threadIdx.x; i < W * SH; i += FSC_THREADS) cnt[i] = 0;
    __syncthreads();
    const int lane = (int)lane_id(), w = (int)(threadIdx.x >> 6);
    double *my_acc = acc + (size_t)w * SH * 3;
    int *my_cnt = cnt + w * SH;
    const size_t n_brick = (size_t)1 << (3 * logN - 6);
    const unsigned m = (unsigned)N - 1u;
    for (size_t br = (size_t)blockIdx.x * W + w; br < n_brick; br += (size_t)gridDim.x * W) {
        const unsigned bc = (unsigned)br & ((unsigned)(N >> 3) - 1u), bb = (unsigned)(br >> (logN - 3)) & ((unsigned)(N >> 2) - 1u);
        const unsigned ba = (unsigned)(br >> (2 * logN - 5));
        const unsigned a = 2u * ba + (unsigned)(lane >> 5), b = 4u * bb + (unsigned)((lane >> 3) & 3), c = 8u * bc + (unsigned)(lane & 7);
        const unsigned ma = (N - a) & m, mb = (N - b) & m, mc = (N - c) & m;
        const double2 z = Z[(((((size_t)a) << logN) + b) << logN) + c], zm = Z[(((((size_t)ma) << logN) + mb) << logN) + mc];
        const double f1x = (z.x + zm.x) * 0.5, f1y = (z.y - zm.y) * 0.5;      // (Z(k) + conj Z(-k)) / 2
        const double f2x = (z.y + zm.y) * 0.5, f2y = (zm.x - z.x) * 0.5;      // (Z(k) - conj Z(-k)) / (2i)
        const double2 ph = c_mul(c_mul(phi[a], phi[N + b]), phi[2 * N + c]);
        const double2 g = c_mul(make_double2(f2x, f2y), ph);
        double p1 = f1x * f1x + f1y * f1y, p2 = f2x * f2x + f2y * f2y, cr = f1x * g.x + f1y * g.y;      // Re(F1 conj(F2 phi))
        const int fi = (int)a < (N >> 1) ? (int)a : (int)a - N, fj = (int)b < (N >> 1) ? (int)b : (int)b - N, fk = (int)c < (N >> 1) ? (int)c : (int)c - N;
        const int r2 = fi * fi + fj * fj + fk * fk;
        int sh = (int)(sqrt((double)r2) + 0.5);      // floor(sqrt(r2) + 0.5) = the t with t^2 - t < r2 <= t^2 + t, fixed up in integers
        while (sh * sh + sh < r2) sh++;
        while (sh > 0 && sh * sh - sh >= r2) sh--;
        // The brick's terms by shell, through the wave's staging rows in LDS (a wave's LDS operations complete in order: what its
        // lanes stored is what its lanes read next; no other wave touches these rows).  The shells of a brick lie within 8 of the
        // smallest (its diagonal is sqrt(1 + 9 + 49) < 8 frequencies long).  Lane 16 q + d adds, for shell smin + d, the terms of
        // lanes 16 q .. 16 q + 15 in lane order; lane d < 16 then adds the four quarters in order and the sum goes into the table.
        const int smin = -wave_max_i32(-sh);
        st_v[w][lane][0] = p1; st_v[w][lane][1] = p2; st_v[w][lane][2] = cr;
        st_s[w][lane] = sh < SH ? sh : -1;      // the lattice corners beyond N / 2 are dropped
        __builtin_amdgcn_wave_barrier();
        const int d = lane & 15, q = lane >> 4, mine = smin + d;
        double a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int an = 0;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const bool hit = st_s[w][16 * q + e] == mine;
            a1 += hit ? st_v[w][16 * q + e][0] : 0.0;
            a2 += hit ? st_v[w][16 * q + e][1] : 0.0;
            a3 += hit ? st_v[w][16 * q + e][2] : 0.0;
            an += hit ? 1 : 0;
        }
        st_p[w][q][d][0] = a1; st_p[w][q][d][1] = a2; st_p[w][q][d][2] = a3;
        st_n[w][q][d] = an;
        __builtin_amdgcn_wave_barrier();
        if (lane < 16 && mine < SH) {
            const int n = st_n[w][0][d] + st_n[w][1][d] + st_n[w][2][d] + st_n[w][3][d];
            if (n) {
                my_acc[mine * 3] += ((st_p[w][0][d][0] + st_p[w][1][d][0]) + st_p[w][2][d][0]) + st_p[w][3][d][0];
                my_acc[mine * 3 + 1] += ((st_p[w][0][d][1] + st_p[w][1][d][1]) + st_p[w][2][d][1]) + st_p[w][3][d][1];
                my_acc[mine * 3 + 2] += ((st_p[w][0][d][2] + st_p[w][1][d][2]) + st_p[w][2][d][2]) + st_p[w][3][d][2];
                my_cnt[mine] += n;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SH * 3; i += FSC_THREADS)
        part_f[(size_t)blockIdx.x * SH * 3 + i] = ((acc[i] + acc[SH * 3 + i]) + acc[2 * SH * 3 + i]) + acc[3 * SH * 3 + i];
    for (int i = threadIdx.x; i < SH; i += FSC_THREADS)
        part_i[(size_t)blockIdx.x * SH + i] = (long long)cnt[i] + cnt[SH + i] + cnt[2 * SH + i] + cnt[3 * SH + i];
}
static_assert(FSC_THREADS == 4 * MAD_WAVE, "k_fsc_shells adds four wave tables");

// out_f [shell][3], out_i [shell]: the workgroups' slots added in order, one thread per number
__global__ __launch_bounds__(256) void k_fsc_sum(int n_part, int SH, const double *__restrict__ part_f, const long long *__restrict__ part_i,
                                                 double *__restrict__ out_f, long long *__restrict__ out_i) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < SH * 3) {
        double v = 0.0;
        for (int p = 0; p < n_part; p++) v += part_f[(size_t)p * SH * 3 + i];
        out_f[i] = v;
    } else if (i < SH * 4) {
        long long v = 0;
        for (int p = 0; p < n_part; p++) v += part_i[(size_t)p * SH + (i - SH * 3)];
        out_i[i - SH * 3] = v;
    }
}

// ---------------------------------------------------------------------------
// phase randomisation and the mask on the lattice
// ---------------------------------------------------------------------------

// u in [0, 1) for draw n of a seed: splitmix64's finaliser on seed + golden * n, the top 53 bits (fourier.splitmix_u)
__device__ __forceinline__ double fsc_splitmix_u(unsigned long long seed, unsigned long long n) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * n;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

// |f| (cos theta + i sin theta), theta = 2 pi u
__device__ __forceinline__ double2 fsc_rephase(double2 f, double u) {
    const double mag = sqrt(f.x * f.x + f.y * f.y), th = 6.283185307179586 * u;
    double s, c;
    sincos(th, &s, &c);
    return make_double2(mag * c, mag * s);
}

// In place on Z, one thread per lattice point L, acting only where L < L', the index of -k: a pair (k, -k) belongs to one thread, a
// self-conjugate point (L == L') to none.  Where shell(k) >= shell_r -- the corners beyond N / 2 included -- the spectra get new
// phases: draw 2 L + 1 for F1, 2 L + 2 for F2.  PAIR: Z = FFT(g1 + i g2), F1 and F2 as k_fsc_shells separates them, written back as
// Z(k) = F1' + i F2' and Z(-k) = conj(F1') + i conj(F2').  Not PAIR: Z is one spectrum, F1 = Z(k), Z(-k) = conj(F1').
template <bool PAIR>
__global__ __launch_bounds__(256) void k_fsc_randomize(double2 *Z, int logN, int shell_r, unsigned long long seed) {
    const int N = 1 << logN;
    const unsigned m = (unsigned)N - 1u;
    const size_t n = (size_t)1 << (3 * logN);
    for (size_t L = (size_t)blockIdx.x * 256 + threadIdx.x; L < n; L += (size_t)gridDim.x * 256) {
        const unsigned c = (unsigned)L & m, b = (unsigned)(L >> logN) & m, a = (unsigned)(L >> (2 * logN));
        const unsigned ma = (N - a) & m, mb = (N - b) & m, mc = (N - c) & m;
        const size_t Lm = (((((size_t)ma) << logN) + mb) << logN) + mc;
        if (L >= Lm) continue;
        const int fi = (int)a < (N >> 1) ? (int)a : (int)a - N, fj = (int)b < (N >> 1) ? (int)b : (int)b - N, fk = (int)c < (N >> 1) ? (int)c : (int)c - N;
        const int r2 = fi * fi + fj * fj + fk * fk;
        int sh = (int)(sqrt((double)r2) + 0.5);      // k_fsc_shells' shell
        while (sh * sh + sh < r2) sh++;
        while (sh > 0 && sh * sh - sh >= r2) sh--;
        if (sh < shell_r) continue;
        const double2 z = Z[L];
        if (PAIR) {
            const double2 zm = Z[Lm];
            const double2 f1 = make_double2((z.x + zm.x) * 0.5, (z.y - zm.y) * 0.5), f2 = make_double2((z.y + zm.y) * 0.5, (zm.x - z.x) * 0.5);
            const double2 g1 = fsc_rephase(f1, fsc_splitmix_u(seed, 2ull * L + 1ull)), g2 = fsc_rephase(f2, fsc_splitmix_u(seed, 2ull * L + 2ull));
            Z[L] = make_double2(g1.x - g2.y, g1.y + g2.x);
            Z[Lm] = make_double2(g1.x + g2.y, g2.x - g1.y);
        } else {
            const double2 g1 = fsc_rephase(z, fsc_splitmix_u(seed, 2ull * L + 1ull));
            Z[L] = g1;
            Z[Lm] = make_double2(g1.x, -g1.y);
        }
    }
}

struct LatMask {
    const float *mask;
    int d[3];
    int p[3];                   // lattice index of the mask's voxel (0, 0, 0); may be negative, or N where the mask misses the lattice
    int logN;
};

// Z(L) = (Re Z scale m, +-(Im Z) scale m) with m the mask's voxel at lattice point L, (+0, +0) outside the mask's box.  CONJ: the
// conjugate that ends an inverse transform (ifft(X) = conj(FFT(conj X)) / N^3), with scale = 1 / N^3.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_fft_mask(double2 *__restrict__ Z, const LatMask A, double scale) {
    const int logN = A.logN;
    const unsigned m = (1u << logN) - 1u;
    const size_t n = (size_t)1 << (3 * logN);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned c = (unsigned)i & m, b = (unsigned)(i >> logN) & m, a = (unsigned)(i >> (2 * logN));
        const unsigned x = a - (unsigned)A.p[0], y = b - (unsigned)A.p[1], z = c - (unsigned)A.p[2];      // below the start: wraps past any extent
        double2 v = make_double2(0.0, 0.0);
        if (x < (unsigned)A.d[0] && y < (unsigned)A.d[1] && z < (unsigned)A.d[2]) {
            const double w = (double)A.mask[((size_t)x * A.d[1] + y) * A.d[2] + z];
            const double2 t = Z[i];
            v = make_double2((t.x * scale) * w, ((CONJ ? -t.y : t.y) * scale) * w);
        }
        Z[i] = v;
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

struct FourierPlan {
    int N, logN;
    int p1[3], p2[3];
    double delta[3];
};

static const double fourier_zero[3] = {0.0, 0.0, 0.0};      // the origin of a grid that has none, with voxsp 1

static int fourier_check(mad_ctx *ctx, const char *who, const int32_t d[3], const double o[3], double voxsp) {
    for (int k = 0; k < 3; k++) {
        if (d[k] <= 0) return mad_fail(ctx, MAD_EINVAL, "%s: empty grid (%d x %d x %d)", who, d[0], d[1], d[2]);
        if (!(fabs(o[k]) <= 1.7e308) || !(fabs(o[k] / voxsp) < 1e15)) return mad_fail(ctx, MAD_EINVAL, "%s: origin %g at voxsp %g", who, o[k], voxsp);
    }
    const unsigned long long v = (unsigned long long)d[0] * (unsigned long long)d[1];
    if (v >= (1ull << 32) || v * (unsigned long long)d[2] >= (1ull << 32))
        return mad_fail(ctx, MAD_EINVAL, "%s: %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, d[0], d[1], d[2]);
    return MAD_OK;
}

// the placement of fourier.plan_box; d2 / o2 NULL: grid 1 alone
static int fourier_plan(mad_ctx *ctx, const char *who, const int32_t d1[3], const double o1[3], const int32_t *d2, const double *o2,
                        double voxsp, FourierPlan *P) {
    long extent = 0;
    for (int k = 0; k < 3; k++) {
        long s = 0;
        P->delta[k] = 0.0;
        if (d2) {
            const double d = o2[k] / voxsp - o1[k] / voxsp;
            s = py_round(d);
            P->delta[k] = d - (double)s;
        }
        const long lo = s < 0 ? s : 0;
        const long e1 = (long)d1[k] - lo, e2 = d2 ? (long)d2[k] + s - lo : 0;
        if (e1 > FFT_MAX_N || e2 > FFT_MAX_N)
            return mad_fail(ctx, MAD_EDOM, "%s: the union box is %ld voxels long on axis %d, more than %d", who, e1 > e2 ? e1 : e2, k, FFT_MAX_N);
        P->p1[k] = (int)-lo;
        P->p2[k] = (int)(s - lo);
        extent = std::max(extent, std::max(e1, e2));
    }
    P->N = FFT_MIN_N; P->logN = 3;
    while (P->N < extent) { P->N <<= 1; P->logN++; }
    return MAD_OK;
}

// One pass of k_fft_lines.  `grid` and `arg` select the form: every tile, dim3(N^2 / 8) with arg = logN, or (PRUNE, section 4o) the
// tiles_x x planes tiles at the low corner of the tile grid, dim3(tiles_x, planes) with arg = live << 8 | logN.  The limit on dynamic
// LDS is raised once per process for each instantiation.
template <int AXIS, int BPT, bool PRUNE> static int fft_launch(mad_ctx *ctx, double2 *Z, const double2 *tw, int logN, int threads, dim3 grid, int arg) {
    const size_t lds = ((size_t)(AXIS == 2 ? FFT_L + 1 : FFT_L) << logN) * sizeof(double2);
    static bool attr = false;
    if (!attr) { MAD_HIP(hipFuncSetAttribute((const void *)k_fft_lines<AXIS, BPT, PRUNE>, hipFuncAttributeMaxDynamicSharedMemorySize, FFT_MAX_N * (FFT_L + 1) * 16)); attr = true; }
    hipLaunchKernelGGL((k_fft_lines<AXIS, BPT, PRUNE>), grid, dim3(threads), lds, ctx->stream, Z, tw, arg);
    return MAD_OK;
}
template <int AXIS, bool PRUNE> static int fft_axis(mad_ctx *ctx, double2 *Z, int logN, dim3 grid, int arg) {
    // butterflies per thread: as few as 512 threads allow, or what the test hook asks for where that still fits
    const int N = 1 << logN, least = N <= 256 ? 1 : (N == 512 ? 2 : 4), bpt = std::max(ctx->fft_bpt, least);
    const int threads = std::max(2 * N / bpt, MAD_WAVE);
    const double2 *tw = (const double2 *)ctx->fft_tw.p;
    if (bpt == 1) return fft_launch<AXIS, 1, PRUNE>(ctx, Z, tw, logN, threads, grid, arg);
    if (bpt == 2) return fft_launch<AXIS, 2, PRUNE>(ctx, Z, tw, logN, threads, grid, arg);
    return fft_launch<AXIS, 4, PRUNE>(ctx, Z, tw, logN, threads, grid, arg);
}

// the twiddles exp(-2 pi i k / N) of the lattice edge N on the device, uploaded when N changes
static int fourier_twiddles(mad_ctx *ctx, int N) {
    if (ctx->fft_tw_n == N) return MAD_OK;
    std::vector<double> tw((size_t)2 * N);
    for (int k = 0; k < N; k++) {
        double c, s;
        unit_root(k, N, &c, &s);
        tw[2 * k] = c; tw[2 * k + 1] = -s;      // exp(-2 pi i k / N)
    }
    MAD_TRY(mad_reserve(ctx, ctx->fft_tw, (size_t)FFT_MAX_N * 16));
    ctx->fft_tw_n = 0;
    MAD_HIP(hipMemcpy(ctx->fft_tw.p, tw.data(), (size_t)N * 16, hipMemcpyHostToDevice));
    ctx->fft_tw_n = N;
    return MAD_OK;
}

// the free-memory check, judged before anything is allocated: the lattice, what the scratch buffers of the grids (n1, n2 voxels;
// either may be 0) would grow by, and extra_bytes
static int fourier_room(mad_ctx *ctx, const char *who, int N, int logN, size_t n1, size_t n2, size_t extra_bytes) {
    const size_t bytes_Z = ((size_t)16 << (3 * logN));
    size_t free_b = 0, total_b = 0;
    MAD_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t grow1 = mad_sb(ctx, S_TMP_H).cap >= (n1 + 4) * 4 ? 0 : (n1 + 4) * 5, grow2 = mad_sb(ctx, S_TMP_I).cap >= (n2 + 4) * 4 ? 0 : (n2 + 4) * 5;
    const size_t need = bytes_Z + grow1 + grow2 + extra_bytes + ((size_t)8 << 20);
    if (need > free_b)
        return mad_fail(ctx, MAD_ENOMEM, "%s: a lattice of %d^3 needs %zu MiB of device memory, %zu MiB are free", who, N, need >> 20, free_b >> 20);
    return MAD_OK;
}

static int fourier_alloc(mad_ctx *ctx, const char *who, int N, int logN, double2 **Zout) {
    const size_t bytes_Z = ((size_t)16 << (3 * logN));
    double2 *Z = nullptr;
    if (hipMalloc((void **)&Z, bytes_Z) != hipSuccess) {
        (void)hipGetLastError();
        return mad_fail(ctx, MAD_ENOMEM, "%s: hipMalloc of the %d^3 lattice (%zu MiB) failed", who, N, bytes_Z >> 20);
    }
    *Zout = Z;
    return MAD_OK;
}

// The three passes of k_fft_lines along z, y, x over every tile.  With P (section 4o) pass a transforms only the P[a].tiles_x x
// P[a].planes tiles at the low corner of the tile grid and takes its lines as P[a].live elements long.
struct PrunedPass { int tiles_x, planes, live; };
template <int AXIS> static int fft_pass(mad_ctx *ctx, double2 *Z, int logN, const PrunedPass *P) {
    if (!P) return fft_axis<AXIS, false>(ctx, Z, logN, dim3(1u << (2 * logN - 3)), logN);      // N^2 / 8 tiles
    return fft_axis<AXIS, true>(ctx, Z, logN, dim3((unsigned)P->tiles_x, (unsigned)P->planes), (P->live << 8) | logN);
}
static int fourier_passes(mad_ctx *ctx, double2 *Z, int logN, const PrunedPass *P = nullptr) {
    MAD_TRY(fft_pass<2>(ctx, Z, logN, P));
    MAD_TRY(fft_pass<1>(ctx, Z, logN, P ? P + 1 : P));
    return fft_pass<0>(ctx, Z, logN, P ? P + 2 : P);
}

// the full passes inside an interval of the "fft" timer of their own
static int fourier_passes_timed(mad_ctx *ctx, double2 *Z, int logN) {
    mad_timer_begin(ctx, MAD_T_FFT);
    const int rc = fourier_passes(ctx, Z, logN);
    mad_timer_end(ctx, MAD_T_FFT);
    return rc;
}

// workgroups of 256 for a streaming kernel over n elements (grid-stride beyond 16 per CU)
static unsigned fourier_blocks(mad_ctx *ctx, size_t n) {
    return (unsigned)std::min<int64_t>(mad_ceil_div((int64_t)n, 256), (int64_t)ctx->n_cu * 16);
}

// The lattices of one call, at most three.  Constructed empty and filled by fourier_alloc alone, so that a refusal allocates nothing.
// On every way out of the entry point each lattice is freed after a wait for the stream: kernels may still be running on it, and
// copies from pageable host memory may still be reading their source.
struct Lattices {
    mad_ctx *ctx;
    double2 *Z[3] = {nullptr, nullptr, nullptr};
    explicit Lattices(mad_ctx *c) : ctx(c) {}
    Lattices(const Lattices &) = delete;
    Lattices &operator=(const Lattices &) = delete;
    ~Lattices() {
        for (double2 *z : Z)
            if (z) {
                (void)hipStreamSynchronize(ctx->stream);
                (void)hipFree(z);
            }
    }
};

// *logN of a lattice edge N that the caller hands in; refuses an N that is no power of two from FFT_MIN_N to FFT_MAX_N
static int fourier_log2(mad_ctx *ctx, const char *who, int N, int *logN) {
    for (*logN = 0; (1 << *logN) < N && *logN < 11;) ++*logN;
    if (N < FFT_MIN_N || N > FFT_MAX_N || (1 << *logN) != N)
        return mad_fail(ctx, MAD_EINVAL, "%s: N = %d (a power of two from %d to %d)", who, N, FFT_MIN_N, FFT_MAX_N);
    return MAD_OK;
}

// what every entry point with origins checks before it plans: the spacing, either grid (g2 false: grid 1 alone), then the plan
static int fourier_plan_checked(mad_ctx *ctx, const char *who, const int32_t *d1, const double *o1, bool g2, const int32_t *d2, const double *o2,
                                double voxsp, FourierPlan *P) {
    if (!(voxsp > 0) || !(voxsp < 1e15)) return mad_fail(ctx, MAD_EINVAL, "%s: voxsp %g", who, voxsp);
    MAD_TRY(fourier_check(ctx, who, d1, o1, voxsp));
    if (g2) MAD_TRY(fourier_check(ctx, who, d2, o2, voxsp));
    return fourier_plan(ctx, who, d1, o1, g2 ? d2 : nullptr, g2 ? o2 : nullptr, voxsp, P);
}

// k_fft_pack's arguments for the grids in S_TMP_H and S_TMP_I (d2 NULL: grid 1 alone) under a plan
static PackArgs fourier_pack_args(mad_ctx *ctx, const FourierPlan &P, const int32_t *d1, const int32_t *d2) {
    PackArgs A;
    memset(&A, 0, sizeof(A));
    A.g1 = scratch<float>(ctx, S_TMP_H);
    A.g2 = d2 ? scratch<float>(ctx, S_TMP_I) : nullptr;
    A.logN = P.logN;
    for (int k = 0; k < 3; k++) { A.d1[k] = d1[k]; A.p1[k] = P.p1[k]; A.d2[k] = d2 ? d2[k] : 0; A.p2[k] = P.p2[k]; }
    return A;
}

// The lattice of a plan: judges the memory, allocates *Zout (a slot of the caller's Lattices), uploads, packs and transforms.  The
// grids stay in S_TMP_H and S_TMP_I.
static int fourier_forward(mad_ctx *ctx, const char *who, const float *g1, const int32_t *d1, const float *g2, const int32_t *d2,
                           size_t extra_bytes, const FourierPlan &P, double2 **Zout) {
    const int N = P.N, logN = P.logN;
    const size_t n1 = (size_t)d1[0] * d1[1] * d1[2], n2 = g2 ? (size_t)d2[0] * d2[1] * d2[2] : 0;
    MAD_TRY(fourier_room(ctx, who, N, logN, n1, n2, extra_bytes));
    MAD_TRY(fourier_twiddles(ctx, N));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (n1 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (n2 + 4) * 4));
    MAD_TRY(fourier_alloc(ctx, who, N, logN, Zout));
    const PackArgs A = fourier_pack_args(ctx, P, d1, g2 ? d2 : nullptr);
    MAD_HIP(hipMemcpyAsync((void *)A.g1, g1, n1 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (g2) MAD_HIP(hipMemcpyAsync((void *)A.g2, g2, n2 * 4, hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_FFT);
    hipLaunchKernelGGL(k_fft_pack, dim3(fourier_blocks(ctx, (size_t)1 << (3 * logN))), dim3(256), 0, ctx->stream, A, *Zout);
    const int rc = fourier_passes(ctx, *Zout, logN);
    mad_timer_end(ctx, MAD_T_FFT);
    if (rc != MAD_OK) return rc;
    MAD_HIP(hipGetLastError());
    return MAD_OK;
}

extern "C" int mad_map_fft(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3], const float *grid2,
                           const int32_t dims2[3], const double origin2[3], double voxsp, int32_t *N_out, double *spectrum) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !dims1 || !origin1 || (grid2 && (!dims2 || !origin2)) || (!N_out && !spectrum))
        return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_fft: NULL argument") : MAD_EINVAL;
    FourierPlan P;
    MAD_TRY(fourier_plan_checked(ctx, "mad_map_fft", dims1, origin1, grid2 != nullptr, dims2, origin2, voxsp, &P));
    if (!spectrum) {      // the size query: the checks and the plan, nothing allocated or launched
        *N_out = P.N;
        return MAD_OK;
    }
    Lattices L(ctx);
    MAD_TRY(fourier_forward(ctx, "mad_map_fft", grid1, dims1, grid2, dims2, 0, P, &L.Z[0]));
    if (N_out) *N_out = P.N;
    MAD_HIP(hipMemcpyAsync(spectrum, L.Z[0], (size_t)16 << (3 * P.logN), hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// the shell sums of the transformed lattice Z under the plan's phase ramp -> sums [N / 2 + 1][3], count [N / 2 + 1] (may be NULL)
static int fsc_shell_tables(mad_ctx *ctx, const double2 *Z, const FourierPlan &P, double *sums, int64_t *count) {
    const int N = P.N, logN = P.logN, SH = N / 2 + 1;
    const int64_t n_brick = (int64_t)1 << (3 * logN - 6);
    const int wgs = (int)std::min<int64_t>(std::max<int64_t>(n_brick / 4, 1), FSC_MAX_WGS);
    const size_t b_phi = (size_t)3 * N * 16, b_pf = (size_t)wgs * SH * 24, b_pi = (size_t)wgs * SH * 8, b_of = (((size_t)SH * 24) + 15) & ~(size_t)15;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), b_phi + b_pf + b_pi + b_of + (size_t)SH * 8));
    char *blk = scratch<char>(ctx, S_TMP_G);
    double2 *phi = (double2 *)blk;
    double *part_f = (double *)(blk + b_phi), *out_f = (double *)(blk + b_phi + b_pf + b_pi);
    long long *part_i = (long long *)(blk + b_phi + b_pf), *out_i = (long long *)(blk + b_phi + b_pf + b_pi + b_of);
    std::vector<double> h_phi((size_t)6 * N);
    for (int ax = 0; ax < 3; ax++)
        for (int a = 0; a < N; a++) {
            const double f = (double)(a < N / 2 ? a : a - N);
            const double ang = 2.0 * M_PI * (f * P.delta[ax]) / (double)N;
            h_phi[((size_t)ax * N + a) * 2] = cos(ang);
            h_phi[((size_t)ax * N + a) * 2 + 1] = -sin(ang);
        }
    MAD_HIP(hipMemcpyAsync(phi, h_phi.data(), b_phi, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // h_phi is pageable: the copy has left it before it goes out of scope
    const size_t lds = (size_t)(FSC_THREADS / MAD_WAVE) * SH * 28 + 16;
    static bool attr = false;
    if (!attr) { MAD_HIP(hipFuncSetAttribute((const void *)k_fsc_shells, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (FFT_MAX_N / 2 + 1) * 28 + 16)); attr = true; }
    mad_timer_begin(ctx, MAD_T_FSC);
    hipLaunchKernelGGL(k_fsc_shells, dim3(wgs), dim3(FSC_THREADS), lds, ctx->stream, Z, (const double2 *)phi, logN, part_f, part_i);
    hipLaunchKernelGGL(k_fsc_sum, dim3((unsigned)mad_ceil_div(SH * 4, 256)), dim3(256), 0, ctx->stream, wgs, SH, (const double *)part_f,
                       (const long long *)part_i, out_f, out_i);
    mad_timer_end(ctx, MAD_T_FSC);
    MAD_HIP(hipGetLastError());
    std::vector<long long> h_cnt(SH);
    MAD_HIP(hipMemcpyAsync(sums, out_f, (size_t)SH * 24, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(h_cnt.data(), out_i, (size_t)SH * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    if (count)
        for (int s = 0; s < SH; s++) count[s] = (int64_t)h_cnt[s];
    return MAD_OK;
}

// what the shell tables of the largest lattice need beside the lattice: 1024 x 513 x 32 bytes of partial tables
static const size_t FSC_EXTRA_BYTES = (size_t)FSC_MAX_WGS * (FFT_MAX_N / 2 + 1) * 32 + ((size_t)1 << 20);

extern "C" int mad_map_fsc(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3], const float *grid2,
                           const int32_t dims2[3], const double origin2[3], double voxsp, int32_t *N_out, double *sums, int64_t *count,
                           int64_t cap_shells) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !dims1 || !origin1 || !grid2 || !dims2 || !origin2 || !sums || !count)
        return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_fsc: NULL argument") : MAD_EINVAL;
    FourierPlan P;
    MAD_TRY(fourier_plan_checked(ctx, "mad_map_fsc", dims1, origin1, true, dims2, origin2, voxsp, &P));
    if (N_out) *N_out = P.N;
    if (cap_shells < P.N / 2 + 1)      // the capacity is judged before anything is allocated or launched
        return mad_fail(ctx, MAD_ENOSPC, "mad_map_fsc: room for %lld shells, the %d^3 lattice has %d", (long long)cap_shells, P.N, P.N / 2 + 1);
    Lattices L(ctx);
    MAD_TRY(fourier_forward(ctx, "mad_map_fsc", grid1, dims1, grid2, dims2, FSC_EXTRA_BYTES, P, &L.Z[0]));
    return fsc_shell_tables(ctx, L.Z[0], P, sums, count);
}

// ---------------------------------------------------------------------------
// the masked curve and its phase-randomised correction
// ---------------------------------------------------------------------------

static int filter_gain_launch(mad_ctx *ctx, double2 *Z, const double *gain, double scale, int logN);

// FSC's convention for one shell of a sums table: C / sqrt(P1 P2), 0 where P1 P2 is not positive
static double fsc_value(const double *sums, int s) {
    const double pp = sums[3 * s] * sums[3 * s + 1];
    return pp > 0 ? sums[3 * s + 2] / sqrt(pp) : 0.0;
}

extern "C" int mad_map_fsc_masked(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3], const float *grid2,
                                  const int32_t dims2[3], const double origin2[3], double voxsp, const float *mask, const int32_t dimsm[3],
                                  const double originm[3], int32_t shell_r, double t_r, uint64_t seed, double *sums_unmasked,
                                  double *sums_masked, double *sums_random, int64_t *count, int32_t *N_out, int32_t *shell_r_out) {
    const char *who = "mad_map_fsc_masked";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !dims1 || !origin1 || !grid2 || !dims2 || !origin2 || !mask || !dimsm || !originm || !sums_unmasked || !sums_masked ||
        !sums_random || !count)
        return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (!(voxsp > 0) || !(voxsp < 1e15)) return mad_fail(ctx, MAD_EINVAL, "%s: voxsp %g", who, voxsp);
    MAD_TRY(fourier_check(ctx, who, dimsm, originm, voxsp));
    if (shell_r < 0 && !(t_r == t_r)) return mad_fail(ctx, MAD_EINVAL, "%s: no shell and a threshold that is not a number", who);
    const size_t n_m = (size_t)dimsm[0] * dimsm[1] * dimsm[2];
    const size_t grow_m = mad_sb(ctx, S_TMP_J).cap >= (n_m + 4) * 4 ? 0 : (n_m + 4) * 5;
    FourierPlan P;
    MAD_TRY(fourier_plan_checked(ctx, who, dims1, origin1, true, dims2, origin2, voxsp, &P));      // the mask first, then the grids
    Lattices L(ctx);
    MAD_TRY(fourier_forward(ctx, who, grid1, dims1, grid2, dims2, FSC_EXTRA_BYTES + grow_m, P, &L.Z[0]));
    double2 *Z = L.Z[0];
    const int N = P.N, logN = P.logN, SH = N / 2 + 1;
    if (N_out) *N_out = N;
    // the mask against grid 1 by whole voxels (mad_map_multiply's placement); what is left of its offset is rounded away
    LatMask M;
    memset(&M, 0, sizeof(M));
    M.logN = logN;
    bool meets = true;
    long pm[3];
    for (int k = 0; k < 3; k++) {
        pm[k] = (long)P.p1[k] + py_round(originm[k] / voxsp - origin1[k] / voxsp);
        if (pm[k] >= N || pm[k] + (long)dimsm[k] <= 0) meets = false;
    }
    for (int k = 0; k < 3; k++) { M.d[k] = dimsm[k]; M.p[k] = meets ? (int)pm[k] : N; }      // -2^31 < -dm < pm < N where they meet
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_J), (n_m + 4) * 4));
    M.mask = scratch<float>(ctx, S_TMP_J);
    MAD_HIP(hipMemcpyAsync((void *)M.mask, mask, n_m * 4, hipMemcpyHostToDevice, ctx->stream));
    // 1. the curve without the mask, and from it the shell the randomisation begins at
    MAD_TRY(fsc_shell_tables(ctx, Z, P, sums_unmasked, count));
    int sr = shell_r;
    if (sr < 0) {
        sr = SH;
        for (int s = 1; s < SH; s++)
            if (fsc_value(sums_unmasked, s) < t_r) { sr = s; break; }
    }
    if (shell_r_out) *shell_r_out = sr;
    // 2. new phases from that shell on, back to real space, times the mask, forward again
    const unsigned blocks = fourier_blocks(ctx, (size_t)1 << (3 * logN));
    mad_timer_begin(ctx, MAD_T_FSC);
    hipLaunchKernelGGL(k_fsc_randomize<true>, dim3(blocks), dim3(256), 0, ctx->stream, Z, logN, sr, (unsigned long long)seed);
    filter_gain_launch(ctx, Z, nullptr, 1.0, logN);      // conj(X)
    mad_timer_end(ctx, MAD_T_FSC);
    MAD_TRY(fourier_passes_timed(ctx, Z, logN));
    mad_timer_begin(ctx, MAD_T_FSC);
    hipLaunchKernelGGL(k_fft_mask<true>, dim3(blocks), dim3(256), 0, ctx->stream, Z, M, ldexp(1.0, -3 * logN));
    mad_timer_end(ctx, MAD_T_FSC);
    MAD_TRY(fourier_passes_timed(ctx, Z, logN));
    MAD_HIP(hipGetLastError());
    MAD_TRY(fsc_shell_tables(ctx, Z, P, sums_random, nullptr));
    // 3. the two grids again (they are still in their buffers: the lattice is packed anew, not kept), times the mask, forward
    mad_timer_begin(ctx, MAD_T_FFT);
    hipLaunchKernelGGL(k_fft_pack, dim3(blocks), dim3(256), 0, ctx->stream, fourier_pack_args(ctx, P, dims1, dims2), Z);
    hipLaunchKernelGGL(k_fft_mask<false>, dim3(blocks), dim3(256), 0, ctx->stream, Z, M, 1.0);
    const int rc = fourier_passes(ctx, Z, logN);
    mad_timer_end(ctx, MAD_T_FFT);
    if (rc != MAD_OK) return rc;
    MAD_HIP(hipGetLastError());
    return fsc_shell_tables(ctx, Z, P, sums_masked, nullptr);
}

extern "C" int mad_map_phase_randomize(mad_ctx *ctx, double *spectrum, int32_t N, int32_t shell_r, uint64_t seed) {
    const char *who = "mad_map_phase_randomize";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !spectrum) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    int logN;
    MAD_TRY(fourier_log2(ctx, who, N, &logN));
    if (shell_r < 0) return mad_fail(ctx, MAD_EINVAL, "%s: shell %d (0 or more)", who, shell_r);
    MAD_TRY(fourier_room(ctx, who, N, logN, 0, 0, 0));
    Lattices L(ctx);
    MAD_TRY(fourier_alloc(ctx, who, N, logN, &L.Z[0]));
    const size_t bytes_Z = (size_t)16 << (3 * logN);
    MAD_HIP(hipMemcpyAsync(L.Z[0], spectrum, bytes_Z, hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_FSC);
    hipLaunchKernelGGL(k_fsc_randomize<false>, dim3(fourier_blocks(ctx, (size_t)1 << (3 * logN))), dim3(256), 0, ctx->stream, L.Z[0], logN, shell_r,
                       (unsigned long long)seed);
    mad_timer_end(ctx, MAD_T_FSC);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(spectrum, L.Z[0], bytes_Z, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// ---------------------------------------------------------------------------
// radial filters
// ---------------------------------------------------------------------------

// k_fft_gain over the whole lattice: z in pieces of min(N, 256), a and b over 0 .. N / 2
static int filter_gain_launch(mad_ctx *ctx, double2 *Z, const double *gain, double scale, int logN) {
    const int N = 1 << logN, threads = std::min(N, 256);
    hipLaunchKernelGGL(k_fft_gain, dim3((unsigned)(N / threads), (unsigned)(N / 2 + 1), (unsigned)(N / 2 + 1)), dim3(threads), 0, ctx->stream, Z, gain,
                       scale, logN);
    return MAD_OK;
}

extern "C" int mad_map_filter(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const float *grid2, const int32_t dims2[3],
                              int32_t pad, const double *gain, int64_t n_gain, int32_t *N_out, float *out1, float *out2) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !dims1 || (grid2 && !dims2) || (!gain && !N_out) || (gain && !out1))
        return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_filter: NULL argument") : MAD_EINVAL;
    if (gain && (grid2 != nullptr) != (out2 != nullptr))
        return mad_fail(ctx, MAD_EINVAL, "mad_map_filter: grid2 and out2 go together (%s is NULL)", grid2 ? "out2" : "grid2");
    MAD_TRY(fourier_check(ctx, "mad_map_filter", dims1, fourier_zero, 1.0));
    if (grid2) MAD_TRY(fourier_check(ctx, "mad_map_filter", dims2, fourier_zero, 1.0));
    if (pad < 0) return mad_fail(ctx, MAD_EINVAL, "mad_map_filter: pad %d (0 or more)", pad);
    int64_t longest = 0;
    for (int k = 0; k < 3; k++) longest = std::max<int64_t>(longest, std::max<int64_t>(dims1[k], grid2 ? dims2[k] : 0));
    if (longest + pad > FFT_MAX_N)
        return mad_fail(ctx, MAD_EDOM, "mad_map_filter: the longest axis and the pad are %lld + %d voxels, more than %d", (long long)longest, pad, FFT_MAX_N);
    FourierPlan P;
    memset(&P, 0, sizeof(P));
    P.N = FFT_MIN_N; P.logN = 3;
    while (P.N < longest + pad) { P.N <<= 1; P.logN++; }
    if (N_out) *N_out = P.N;
    if (!gain) return MAD_OK;      // the size query
    const int N = P.N, logN = P.logN;
    const int64_t want = (int64_t)3 * (N / 2) * (N / 2) + 1;
    if (n_gain != want)
        return mad_fail(ctx, MAD_EINVAL, "mad_map_filter: a gain table of %lld entries, the %d^3 lattice needs %lld", (long long)n_gain, N, (long long)want);
    for (int64_t i = 0; i < n_gain; i++)
        if (!(fabs(gain[i]) <= 1.7976931348623157e308)) return mad_fail(ctx, MAD_EINVAL, "mad_map_filter: gain[%lld] is not finite", (long long)i);
    const size_t b_gain = (size_t)n_gain * 8, grow_g = mad_sb(ctx, S_TMP_G).cap >= b_gain ? 0 : b_gain + b_gain / 4;
    Lattices L(ctx);
    MAD_TRY(fourier_forward(ctx, "mad_map_filter", grid1, dims1, grid2, dims2, grow_g, P, &L.Z[0]));
    double2 *Z = L.Z[0];
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), b_gain));
    double *d_gain = scratch<double>(ctx, S_TMP_G);
    MAD_HIP(hipMemcpyAsync(d_gain, gain, b_gain, hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_FILTER);
    filter_gain_launch(ctx, Z, d_gain, 1.0, logN);
    mad_timer_end(ctx, MAD_T_FILTER);
    MAD_TRY(fourier_passes_timed(ctx, Z, logN));
    // the grids were consumed by k_fft_pack: their buffers take the outputs
    const size_t n1 = (size_t)dims1[0] * dims1[1] * dims1[2], n2 = grid2 ? (size_t)dims2[0] * dims2[1] * dims2[2] : 0;
    const double scale = ldexp(1.0, -3 * logN);
    float *o1 = scratch<float>(ctx, S_TMP_H), *o2 = scratch<float>(ctx, S_TMP_I);
    mad_timer_begin(ctx, MAD_T_FILTER);
    hipLaunchKernelGGL(k_fft_unpack<false>, dim3(fourier_blocks(ctx, n1)), dim3(256), 0, ctx->stream, (const double2 *)Z, logN, scale, o1,
                       (unsigned)dims1[1], (unsigned)dims1[2], n1);
    if (grid2)
        hipLaunchKernelGGL(k_fft_unpack<true>, dim3(fourier_blocks(ctx, n2)), dim3(256), 0, ctx->stream, (const double2 *)Z, logN, scale, o2,
                           (unsigned)dims2[1], (unsigned)dims2[2], n2);
    mad_timer_end(ctx, MAD_T_FILTER);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out1, o1, n1 * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (grid2) MAD_HIP(hipMemcpyAsync(out2, o2, n2 * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

extern "C" int mad_map_ifft(mad_ctx *ctx, const double *spectrum, int32_t N, double *out) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !spectrum || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_ifft: NULL argument") : MAD_EINVAL;
    int logN;
    MAD_TRY(fourier_log2(ctx, "mad_map_ifft", N, &logN));
    MAD_TRY(fourier_room(ctx, "mad_map_ifft", N, logN, 0, 0, 0));
    MAD_TRY(fourier_twiddles(ctx, N));
    Lattices L(ctx);
    MAD_TRY(fourier_alloc(ctx, "mad_map_ifft", N, logN, &L.Z[0]));
    double2 *Z = L.Z[0];
    const size_t bytes_Z = (size_t)16 << (3 * logN);
    MAD_HIP(hipMemcpyAsync(Z, spectrum, bytes_Z, hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_FILTER);
    filter_gain_launch(ctx, Z, nullptr, 1.0, logN);      // conj(X)
    mad_timer_end(ctx, MAD_T_FILTER);
    MAD_TRY(fourier_passes_timed(ctx, Z, logN));
    mad_timer_begin(ctx, MAD_T_FILTER);
    filter_gain_launch(ctx, Z, nullptr, ldexp(1.0, -3 * logN), logN);      // conj(.) / N^3: a power of two, exact
    mad_timer_end(ctx, MAD_T_FILTER);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out, Z, bytes_Z, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}

// ---------------------------------------------------------------------------
// translation scan
// ---------------------------------------------------------------------------
// mad_map_scan scores every whole-voxel translation u of a template inside a map by fast local correlation (Roseman's scheme):
// C(u) = sum m(u + x) g(x), E(u) = sum m(u + x)^2 w(x) and, centred, A(u) = sum m(u + x) w(x), with w = [g > iso] and g zeroed
// outside w.  Map and template sit at lattice index (0, 0, 0); Zm = FFT(m + i m^2) stays for the call, per template
// Zt = FFT(g w + i w); k_scan_product leaves conj(M conj(G) + i M2 conj(W)) in Zt (and conj(M conj(W)) in a third lattice), the
// three k_fft_lines passes turn that into N^3 conj(C + i E), and k_scan_score forms the score over the box of offsets whose
// template lies wholly inside the map (none of them wraps around the lattice) and keeps the best template per offset.

#define SCAN_CAP0 4096      // peak candidates the list holds before it is grown to the count and k_scan_peaks runs again

// TPL false: Z = m + i m^2 over the map's box.  TPL true: Z = g w + i w over the template's, w = 1 where g > iso.  Zero elsewhere.
template <bool TPL>
__global__ __launch_bounds__(256) void k_scan_pack(const float *__restrict__ g, unsigned d0, unsigned d1, unsigned d2, double iso, int logN,
                                                   double2 *__restrict__ Z) {
    const unsigned m = (1u << logN) - 1u;
    const size_t n = (size_t)1 << (3 * logN);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned c = (unsigned)i & m, b = (unsigned)(i >> logN) & m, a = (unsigned)(i >> (2 * logN));
        double2 v = make_double2(0.0, 0.0);
        if (a < d0 && b < d1 && c < d2) {
            const double x = (double)g[((size_t)a * d1 + b) * d2 + c];
            if (!TPL) v = make_double2(x, x * x);      // 24 x 24 bits: exact
            else if (x > iso) v = make_double2(x, 1.0);
        }
        Z[i] = v;
    }
}

// In place on the template's lattice.  With M, M2 split from Zm and G, W from Zt as k_fsc_shells splits a pair, X = M conj(G) and
// Y = M2 conj(W): P(k) = X + i Y, and because all four signals are real P(-k) = conj(X) + i conj(Y).  A thread owns k and -k, reads
// both lattices at both and writes conj P(k) = conj(X) - i conj(Y) and conj P(-k) = X - i Y (Zq, mode 1: conj Q(k) = conj(R),
// conj Q(-k) = R, R = M conj(W)), ready for ifft(P) = conj(FFT(conj P)) / N^3.  A workgroup takes the z line (a, b) and its mirror
// image (N - a, N - b) whole -- thread c pairs (a, b, c) with (N - a, N - b, N - c) --, so that both lines are read and written
// end to end.  blockIdx.y = a runs over 0 .. N / 2 and blockIdx.x = b over 0 .. N - 1; where a is its own mirror image (0, N / 2)
// the pair of lines belongs to the smaller b, and a line that is its own mirror image pairs c with N - c inside itself (c <= N / 2;
// 0 and N / 2 are their own pair and are written once).
// blockDim.x = min(N, 256), on purpose one pair of lines per workgroup at every N: below N = 64 that is part of a wave (8 to 32
// lanes) and at N = 64 one wave, on lattices of at most 4 MiB whose whole product is a few microseconds beside the launches of the
// six line passes around it; packing several pairs of lines into a workgroup for them was not built and not measured.
__global__ __launch_bounds__(256) void k_scan_product(const double2 *__restrict__ Zm, double2 *__restrict__ Zt, double2 *__restrict__ Zq, int logN) {
    const int N = 1 << logN, msk = N - 1;
    const int b = (int)blockIdx.x, a = (int)blockIdx.y;
    const int a2 = (N - a) & msk, b2 = (N - b) & msk;
    if (a > (N >> 1) || b >= N || (a2 == a && b > b2)) return;
    const bool self = a2 == a && b2 == b;      // uniform over the workgroup
    const size_t l0 = ((((size_t)a) << logN) + b) << logN, l1 = ((((size_t)a2) << logN) + b2) << logN;
    for (int c = (int)threadIdx.x; c < N; c += (int)blockDim.x) {
        const int c2 = (N - c) & msk;
        if (self && c > c2) continue;
        const size_t i = l0 + c, j = l1 + c2;
        const double2 zm = Zm[i], zn = Zm[j], zt = Zt[i], zu = Zt[j];
        const double mx = (zm.x + zn.x) * 0.5, my = (zm.y - zn.y) * 0.5;      // M  = (Zm(k) + conj Zm(-k)) / 2
        const double sx = (zm.y + zn.y) * 0.5, sy = (zn.x - zm.x) * 0.5;      // M2 = (Zm(k) - conj Zm(-k)) / (2i)
        const double gx = (zt.x + zu.x) * 0.5, gy = (zt.y - zu.y) * 0.5;      // G
        const double wx = (zt.y + zu.y) * 0.5, wy = (zu.x - zt.x) * 0.5;      // W
        const double Xx = mx * gx + my * gy, Xy = my * gx - mx * gy;          // M conj(G)
        const double Yx = sx * wx + sy * wy, Yy = sy * wx - sx * wy;          // M2 conj(W)
        Zt[i] = make_double2(Xx - Yy, -(Xy + Yx));
        if (j != i) Zt[j] = make_double2(Xx + Yy, Xy - Yx);
        if (Zq) {
            const double Rx = mx * wx + my * wy, Ry = my * wx - mx * wy;      // M conj(W)
            Zq[i] = make_double2(Rx, -Ry);
            if (j != i) Zq[j] = make_double2(Rx, Ry);
        }
    }
}

struct ScoreStat { double n_w, G, gbar; };      // of one template or rotation; G: G' in mode 1

struct ScoreArgs {
    int logN, mode, idx;         // idx: the template's or rotation's index; index 0 initialises best / best_i
    unsigned D1, D2;             // the offset box [D0][D1][D2]
    size_t nD;
    double scale;                // 1 / N^3
    double floor;                // mad_map_scan: e_min; mad_map_search: e_fill, the floor is e_fill n_w
    ScoreStat st;                // mad_map_scan: the template's, from the host; mad_map_search reads the rotation's record instead
};

// offset q of the box [D0][D1][D2] in linear order -> (x, y, z)
__device__ __forceinline__ void scan_offset(unsigned q, unsigned D1, unsigned D2, unsigned &x, unsigned &y, unsigned &z) {
    const unsigned t = q / D2;
    z = q - t * D2; x = t / D1; y = t - x * D1;
}

// The score of the offset at lattice index `at`.  Zt holds N^3 conj(C + i E), Zq (mode 1) N^3 conj(A).  The offset is scored where
// E > e_min (E' in mode 1): -> whether it is, *s its float32 score (0 where it is not).
__device__ __forceinline__ bool scan_score_at(const double2 *__restrict__ Zt, const double2 *__restrict__ Zq, size_t at, int mode, double scale,
                                              const ScoreStat &st, double e_min, float *s) {
    const double2 v = Zt[at];
    double c = v.x * scale, e = -(v.y * scale);
    if (mode) {
        const double a = Zq[at].x * scale;
        c = c - a * st.gbar;
        e = e - (a * a) / st.n_w;
    }
    const bool scored = e > e_min;
    *s = scored ? (float)(c / sqrt(e * st.G)) : 0.0f;
    return scored;
}

// best / best_i take what index 0 gives, whatever it is, and after it a strictly greater float32 score only, so the lowest index
// keeps a tie; best_i is -1 where nothing has scored the offset.
__device__ __forceinline__ void scan_keep(float *__restrict__ best, int *__restrict__ best_i, size_t i, int idx, bool scored, float s) {
    if (idx == 0) { best[i] = s; best_i[i] = scored ? 0 : -1; }
    else if (scored && (best_i[i] < 0 || s > best[i])) { best[i] = s; best_i[i] = idx; }
}

// Over the box of offsets alone, grid-stride in workgroups of 256: every offset scored (skip: none is) and kept.
__device__ __forceinline__ void scan_score_box(const double2 *__restrict__ Zt, const double2 *__restrict__ Zq, const ScoreArgs &A, const ScoreStat &st,
                                               double e_min, bool skip, float *__restrict__ best, int *__restrict__ best_i) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < A.nD; i += (size_t)gridDim.x * 256) {
        bool scored = false;
        float s = 0.0f;
        if (!skip) {
            unsigned x, y, z;
            scan_offset((unsigned)i, A.D1, A.D2, x, y, z);
            scored = scan_score_at(Zt, Zq, (((((size_t)x) << A.logN) + y) << A.logN) + z, A.mode, A.scale, st, e_min, &s);
        }
        scan_keep(best, best_i, i, A.idx, scored, s);
    }
}

// mad_map_scan: the template's statistics and the floor come with the arguments
__global__ __launch_bounds__(256) void k_scan_score(const double2 *__restrict__ Zt, const double2 *__restrict__ Zq, const ScoreArgs A,
                                                    float *__restrict__ best, int *__restrict__ best_t) {
    scan_score_box(Zt, Zq, A, A.st, A.floor, false, best, best_t);
}

// An offset is a peak when a template scored it, its score is at least min_score and every neighbour of the 26 inside the box is
// smaller, or equal with a larger linear index.  Peaks are appended through an integer counter in any order (the host sorts);
// *count ends as the number found, of which the first cap are in the list.
__global__ __launch_bounds__(256) void k_scan_peaks(const float *__restrict__ best, const int *__restrict__ best_t, unsigned D0, unsigned D1,
                                                    unsigned D2, size_t nD, double min_score, unsigned cap, unsigned *__restrict__ count,
                                                    unsigned *__restrict__ list) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nD; i += (size_t)gridDim.x * 256) {
        if (best_t[i] < 0) continue;
        const float s = best[i];
        if (!((double)s >= min_score)) continue;
        const unsigned q = (unsigned)i;
        unsigned x, y, z;
        scan_offset(q, D1, D2, x, y, z);
        bool peak = true;
        for (int dx = -1; dx <= 1 && peak; dx++)
            for (int dy = -1; dy <= 1 && peak; dy++)
                for (int dz = -1; dz <= 1; dz++) {
                    const unsigned nx = x + (unsigned)dx, ny = y + (unsigned)dy, nz = z + (unsigned)dz;      // below 0: wraps past any extent
                    if ((dx == 0 && dy == 0 && dz == 0) || nx >= D0 || ny >= D1 || nz >= D2) continue;
                    const size_t j = ((size_t)nx * D1 + ny) * D2 + nz;
                    const float v = best[j];
                    if (!(v < s || (v == s && j > i))) { peak = false; break; }
                }
        if (peak) {
            const unsigned pos = atomicAdd(count, 1u);
            if (pos < cap) list[pos] = q;
        }
    }
}

// ---------------------------------------------------------------------------
// the correlation set-up mad_map_scan and mad_map_search share
// ---------------------------------------------------------------------------

struct CorrPlan {
    int N, logN;
    int n_lat;                   // lattices: the map's and the template's, mode 1: a third
    unsigned D[3];               // the box of offsets
    size_t n1, nD;               // voxels of the map, offsets
    unsigned wg_Z, wg_D;         // workgroups of 256 over the lattice and over the box
    int threads;                 // of k_scan_product
    // the output block, S_TMP_G once corr_setup has run: best | best_i (b_best bytes each) | count (16 bytes) | the caller's tail
    size_t b_best;
    char *blk;
    float *best() const { return (float *)blk; }
    int *best_i() const { return (int *)(blk + b_best); }
    unsigned *count() const { return (unsigned *)(blk + 2 * b_best); }
    char *tail() const { return blk + 2 * b_best + 16; }
};

// The peaks of the score volume on the device (C.best(), C.best_i() over the box C.D) and the volume itself, to the host.  The list
// in S_TMP_J holds `cap` candidates; where more were found and some are wanted it grows to the count and the kernel runs again, while
// best is still on the device.
static int scan_peaks_out(mad_ctx *ctx, const char *who, int timer, const CorrPlan &C, double min_score, int64_t k, float *best, int32_t *best_t,
                          double *peaks, int64_t *n_peaks, int64_t *n_found) {
    const float *d_best = C.best();
    const int *d_best_t = C.best_i();
    unsigned *d_count = C.count();
    const unsigned *D = C.D, wg_D = C.wg_D;
    const size_t nD = C.nD;
    unsigned cap = SCAN_CAP0, found = 0;
    for (int pass = 0; pass < 2; pass++) {
        MAD_HIP(hipMemsetAsync(d_count, 0, 16, ctx->stream));
        mad_timer_begin(ctx, timer);
        hipLaunchKernelGGL(k_scan_peaks, dim3(wg_D), dim3(256), 0, ctx->stream, d_best, d_best_t, D[0], D[1], D[2], nD, min_score, cap, d_count,
                           scratch<unsigned>(ctx, S_TMP_J));
        mad_timer_end(ctx, timer);
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(&found, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));
        if (found <= cap || k == 0) break;
        if (pass == 1) return mad_fail(ctx, MAD_EHIP, "%s: %u peaks after %u were counted", who, found, cap);
        size_t free_b = 0, total_b = 0;
        MAD_HIP(hipMemGetInfo(&free_b, &total_b));
        if ((size_t)found * 5 + ((size_t)8 << 20) > free_b)
            return mad_fail(ctx, MAD_ENOMEM, "%s: a list of %u peaks needs %zu MiB of device memory, %zu MiB are free", who, found,
                            ((size_t)found * 5) >> 20, free_b >> 20);
        MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_J), (size_t)found * 4));
        cap = found;
    }
    const size_t n_list = k == 0 ? 0 : (size_t)std::min(found, cap);
    std::vector<unsigned> list(n_list);
    MAD_HIP(hipMemcpyAsync(best, d_best, nD * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(best_t, d_best_t, nD * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (n_list) MAD_HIP(hipMemcpyAsync(list.data(), scratch<unsigned>(ctx, S_TMP_J), n_list * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    // score descending, then linear index ascending: the order of the list does not depend on the order of the appends
    std::sort(list.begin(), list.end(), [best](unsigned p, unsigned q) { return best[p] > best[q] || (best[p] == best[q] && p < q); });
    const int64_t n_out = std::min<int64_t>(k, (int64_t)n_list);
    for (int64_t p = 0; p < n_out; p++) {
        const unsigned q = list[(size_t)p], t = q / D[2];
        peaks[5 * p] = (double)(t / D[1]); peaks[5 * p + 1] = (double)(t % D[1]); peaks[5 * p + 2] = (double)(q % D[2]);
        peaks[5 * p + 3] = (double)best[q]; peaks[5 * p + 4] = (double)best_t[q];
    }
    *n_peaks = n_out;
    *n_found = (int64_t)found;
    return MAD_OK;
}

// What both refuse after their own checks, in this order: mode, k, a map longer than FFT_MAX_N, and `ext` voxels (`what`: "the
// templates are", "the cube is") that do not fit into the map.  -> N, logN, the box of offsets, and the answer to the size query.
static int corr_plan(mad_ctx *ctx, const char *who, const char *what, const int32_t *d1, const int32_t *ext, int32_t mode, int64_t k, int32_t *N_out,
                     CorrPlan *C) {
    if (mode != 0 && mode != 1) return mad_fail(ctx, MAD_EINVAL, "%s: mode %d (0 un-centred, 1 centred)", who, mode);
    if (k < 0) return mad_fail(ctx, MAD_EINVAL, "%s: k = %lld (0 or more)", who, (long long)k);
    int longest = 0;
    for (int a = 0; a < 3; a++) longest = std::max(longest, (int)d1[a]);
    if (longest > FFT_MAX_N) return mad_fail(ctx, MAD_EDOM, "%s: the map's longest axis is %d voxels, more than %d", who, longest, FFT_MAX_N);
    for (int a = 0; a < 3; a++)
        if (ext[a] > d1[a])
            return mad_fail(ctx, MAD_EDOM, "%s: %s %d voxels long on axis %d, the map %d: no offset keeps that inside", who, what, ext[a], a, d1[a]);
    C->N = FFT_MIN_N; C->logN = 3;
    while (C->N < longest) { C->N <<= 1; C->logN++; }
    C->n_lat = mode ? 3 : 2;
    for (int a = 0; a < 3; a++) C->D[a] = (unsigned)(d1[a] - ext[a] + 1);
    C->n1 = (size_t)d1[0] * d1[1] * d1[2];
    C->nD = (size_t)C->D[0] * C->D[1] * C->D[2];
    if (N_out) *N_out = C->N;
    return MAD_OK;
}

// Everything up to the map's transform.  The memory is judged before anything is allocated: n2 voxels go into S_TMP_I beside the map
// in S_TMP_H, `tail` bytes of the caller's behind the output block in S_TMP_G.  Then the twiddles, the four scratch buffers, the
// lattices, and Zm = L->Z[0] = FFT(m + i m^2).
static int corr_setup(mad_ctx *ctx, const char *who, const float *map, const int32_t *d1, size_t n2, size_t tail, CorrPlan *C, Lattices *L) {
    const int N = C->N, logN = C->logN;
    C->b_best = (C->nD * 4 + 15) & ~(size_t)15;
    const size_t b_out = 2 * C->b_best + 16 + tail, b_list = (size_t)SCAN_CAP0 * 4;
    const size_t grow_g = mad_sb(ctx, S_TMP_G).cap >= b_out ? 0 : b_out + b_out / 4, grow_j = mad_sb(ctx, S_TMP_J).cap >= b_list ? 0 : b_list + b_list / 4;
    MAD_TRY(fourier_room(ctx, who, N, logN, C->n1, n2, (size_t)(C->n_lat - 1) * ((size_t)16 << (3 * logN)) + grow_g + grow_j));
    MAD_TRY(fourier_twiddles(ctx, N));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (C->n1 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (n2 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), b_out));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_J), b_list));
    for (int l = 0; l < C->n_lat; l++) MAD_TRY(fourier_alloc(ctx, who, N, logN, &L->Z[l]));
    C->blk = scratch<char>(ctx, S_TMP_G);
    C->wg_Z = fourier_blocks(ctx, (size_t)1 << (3 * logN));
    C->wg_D = fourier_blocks(ctx, C->nD);
    C->threads = std::min(N, 256);
    float *d_map = scratch<float>(ctx, S_TMP_H);
    MAD_HIP(hipMemcpyAsync(d_map, map, C->n1 * 4, hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_SCAN);
    hipLaunchKernelGGL(k_scan_pack<false>, dim3(C->wg_Z), dim3(256), 0, ctx->stream, (const float *)d_map, (unsigned)d1[0], (unsigned)d1[1], (unsigned)d1[2],
                       0.0, logN, L->Z[0]);
    mad_timer_end(ctx, MAD_T_SCAN);
    MAD_TRY(fourier_passes_timed(ctx, L->Z[0], logN));
    MAD_HIP(hipGetLastError());
    return MAD_OK;
}

// k_scan_score's and k_search_score's arguments but for what changes from launch to launch: the index and, in the scan, the statistics
static ScoreArgs corr_score_args(const CorrPlan &C, int mode, double floor) {
    ScoreArgs A;
    memset(&A, 0, sizeof(A));
    A.logN = C.logN; A.mode = mode; A.D1 = C.D[1]; A.D2 = C.D[2]; A.nD = C.nD; A.scale = ldexp(1.0, -3 * C.logN); A.floor = floor;
    return A;
}

extern "C" int mad_map_scan(mad_ctx *ctx, const float *map, const int32_t dims1[3], int32_t n_t, const float *const *templates,
                            const int32_t dims2[3], double iso, double e_min, int32_t mode, double min_score, int64_t k, float *best,
                            int32_t *best_t, double *peaks, int64_t *n_peaks, int64_t *n_found, int32_t *N_out) {
    const char *who = "mad_map_scan";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !dims1 || !dims2 || (!best && !N_out) || (best && (!map || !templates || !best_t || !n_peaks || !n_found || (k > 0 && !peaks))))
        return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (n_t < 1) return mad_fail(ctx, MAD_EINVAL, "%s: %d templates (1 or more)", who, n_t);
    MAD_TRY(fourier_check(ctx, who, dims1, fourier_zero, 1.0));
    MAD_TRY(fourier_check(ctx, who, dims2, fourier_zero, 1.0));
    if (!(fabs(iso) <= 1.7e308) || !(fabs(min_score) <= 1.7e308) || !(e_min >= 0.0 && e_min <= 1.7e308))
        return mad_fail(ctx, MAD_EINVAL, "%s: iso %g, e_min %g, min_score %g (finite, e_min 0 or more)", who, iso, e_min, min_score);
    CorrPlan C;
    MAD_TRY(corr_plan(ctx, who, "the templates are", dims1, dims2, mode, k, N_out, &C));
    if (!best) return MAD_OK;      // the size query
    const size_t n2 = (size_t)dims2[0] * dims2[1] * dims2[2];

    // n_w, G and the sum of every template, in voxel order in float64, before anything is allocated
    std::vector<ScoreStat> st((size_t)n_t);
    for (int32_t j = 0; j < n_t; j++) {
        if (!templates[j]) return mad_fail(ctx, MAD_EINVAL, "%s: template %d is NULL", who, j);
        double n_w = 0.0, G = 0.0, S = 0.0;
        for (size_t i = 0; i < n2; i++) {
            const double x = (double)templates[j][i];
            if (x > iso) { n_w += 1.0; G += x * x; S += x; }
        }
        if (!(n_w > 0.0)) return mad_fail(ctx, MAD_EINVAL, "%s: template %d has no voxel above iso = %g", who, j, iso);
        st[j].n_w = n_w; st[j].G = G; st[j].gbar = 0.0;
        if (!(G > 0.0 && G <= 1.7e308)) return mad_fail(ctx, MAD_EINVAL, "%s: template %d has G = %g under its mask", who, j, G);
        if (mode) {
            st[j].gbar = S / n_w;
            st[j].G = G - n_w * (st[j].gbar * st[j].gbar);
            if (!(st[j].G > 0.0)) return mad_fail(ctx, MAD_EINVAL, "%s: template %d is constant under its mask (G' = %g)", who, j, st[j].G);
        }
    }

    Lattices L(ctx);
    MAD_TRY(corr_setup(ctx, who, map, dims1, n2, 0, &C, &L));
    double2 *Zm = L.Z[0], *Zt = L.Z[1], *Zq = L.Z[2];
    float *d_tpl = scratch<float>(ctx, S_TMP_I);
    const int N = C.N, logN = C.logN;

    ScoreArgs A = corr_score_args(C, mode, e_min);
    for (int32_t j = 0; j < n_t; j++) {
        MAD_HIP(hipMemcpyAsync(d_tpl, templates[j], n2 * 4, hipMemcpyHostToDevice, ctx->stream));
        mad_timer_begin(ctx, MAD_T_SCAN);
        hipLaunchKernelGGL(k_scan_pack<true>, dim3(C.wg_Z), dim3(256), 0, ctx->stream, (const float *)d_tpl, (unsigned)dims2[0], (unsigned)dims2[1],
                           (unsigned)dims2[2], iso, logN, Zt);
        mad_timer_end(ctx, MAD_T_SCAN);
        MAD_TRY(fourier_passes_timed(ctx, Zt, logN));
        mad_timer_begin(ctx, MAD_T_SCAN);
        hipLaunchKernelGGL(k_scan_product, dim3((unsigned)N, (unsigned)(N / 2 + 1)), dim3(C.threads), 0, ctx->stream, (const double2 *)Zm, Zt, Zq, logN);
        mad_timer_end(ctx, MAD_T_SCAN);
        mad_timer_begin(ctx, MAD_T_FFT);      // one interval for both inverse transforms
        int rc = fourier_passes(ctx, Zt, logN);
        if (rc == MAD_OK && mode) rc = fourier_passes(ctx, Zq, logN);
        mad_timer_end(ctx, MAD_T_FFT);
        if (rc != MAD_OK) return rc;
        A.idx = j; A.st = st[j];
        mad_timer_begin(ctx, MAD_T_SCAN);
        hipLaunchKernelGGL(k_scan_score, dim3(C.wg_D), dim3(256), 0, ctx->stream, (const double2 *)Zt, (const double2 *)Zq, A, C.best(), C.best_i());
        mad_timer_end(ctx, MAD_T_SCAN);
        MAD_HIP(hipGetLastError());
    }
    return scan_peaks_out(ctx, who, MAD_T_SCAN, C, min_score, k, best, best_t, peaks, n_peaks, n_found);
}

// ---------------------------------------------------------------------------
// rotational search
// ---------------------------------------------------------------------------
// mad_map_search scores every whole-voxel translation of every rotation of ONE base template: per rotation the template is sampled
// from the base grid into a cube of edge e (k_search_rotate: gather, trilinear interpolation, cast to float32, mask, the lattice
// write of g w + i w and the first level of the sums n_w, G, S), k_search_stats finishes the sums into a record in device memory,
// the pruned line passes transform only what is not zero on the way in and only what k_search_score reads on the way out, and
// k_search_score takes n_w, G and S from the record.  Nothing comes back to the host between the first rotation and the last.

#define SEARCH_RUN 256      // elements of a run of tree_sum (fourier.py), and the workgroup of k_search_rotate / k_search_stats

struct SearchRotateArgs {
    const float *g0;             // the base grid, dims d0
    int d0[3];
    unsigned e, n_runs;          // the cube's edge; ceil(e^3 / 256) runs
    size_t n_box;                // e^3 <= 2^30
    int logN;                    // of the lattice Z (unused without one)
    double c0[3], c2, iso;
};

// s[k][0] <- the sum of s[k][0 .. 255] by halving, k = 0 .. 2: x[:128] + x[128:], then 64, ... 1 (fourier.tree_sum's run)
__device__ __forceinline__ void search_run_sum(double (*s)[SEARCH_RUN], unsigned t) {
    __syncthreads();
    for (unsigned h = SEARCH_RUN / 2; h >= 1; h >>= 1) {
        if (t < h) {
            s[0][t] = s[0][t] + s[0][t + h];
            s[1][t] = s[1][t] + s[1][t + h];
            s[2][t] = s[2][t] + s[2][t + h];
        }
        __syncthreads();
    }
}

// Workgroup b < n_runs takes run b of the cube in linear [x][y][z] order: voxel x samples the base grid at
// p = c0 + (x - c2) @ R^T (R row-major in device memory), trilinear with corners beyond the grid 0 (a point at or beyond -1 or d on an
// axis has none inside: 0), float64 in the contract's order, rounded to float32.  out_g (may be NULL): that float32.  Z (may be NULL):
// g w + i w at lattice index x.  part[b][3] = the run's sums of w, g^2 w and g w.  Workgroups b >= n_runs (launched only for full
// passes, search_prune = 0) write +0 to every lattice element outside the cube, grid-stride.
__global__ __launch_bounds__(SEARCH_RUN) void k_search_rotate(const SearchRotateArgs A, const double *__restrict__ R, double2 *__restrict__ Z,
                                                               float *__restrict__ out_g, double *__restrict__ part) {
    __shared__ double s[3][SEARCH_RUN];
    const unsigned t = threadIdx.x;
    if (blockIdx.x >= A.n_runs) {      // uniform over the workgroup
        const unsigned m = (1u << A.logN) - 1u;
        const size_t n = (size_t)1 << (3 * A.logN), step = (size_t)(gridDim.x - A.n_runs) * SEARCH_RUN;
        for (size_t i = (size_t)(blockIdx.x - A.n_runs) * SEARCH_RUN + t; i < n; i += step) {
            const unsigned c = (unsigned)i & m, b = (unsigned)(i >> A.logN) & m, a = (unsigned)(i >> (2 * A.logN));
            if (a >= A.e || b >= A.e || c >= A.e) Z[i] = make_double2(0.0, 0.0);
        }
        return;
    }
    const size_t i = (size_t)blockIdx.x * SEARCH_RUN + t;
    double vw = 0.0, vg = 0.0, vs = 0.0;
    if (i < A.n_box) {
        const unsigned q = (unsigned)i, xy = q / A.e, z = q - xy * A.e, x = xy / A.e, y = xy - x * A.e;
        const double d0 = (double)x - A.c2, d1 = (double)y - A.c2, d2 = (double)z - A.c2;
        const double px = A.c0[0] + ((d0 * R[0] + d1 * R[1]) + d2 * R[2]);
        const double py = A.c0[1] + ((d0 * R[3] + d1 * R[4]) + d2 * R[5]);
        const double pz = A.c0[2] + ((d0 * R[6] + d1 * R[7]) + d2 * R[8]);
        float g = 0.0f;
        if (px > -1.0 && px < (double)A.d0[0] && py > -1.0 && py < (double)A.d0[1] && pz > -1.0 && pz < (double)A.d0[2]) {
            const double fx = floor(px), fy = floor(py), fz = floor(pz);
            const double tx = px - fx, ty = py - fy, tz = pz - fz;
            const int ix = (int)fx, iy = (int)fy, iz = (int)fz;      // -1 .. d - 1
            double v[2][2][2];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const unsigned ux = (unsigned)(ix + a), uy = (unsigned)(iy + b), uz = (unsigned)(iz + c);      // -1 wraps past any extent
                        v[a][b][c] = ux < (unsigned)A.d0[0] && uy < (unsigned)A.d0[1] && uz < (unsigned)A.d0[2]
                                         ? (double)A.g0[((size_t)ux * (unsigned)A.d0[1] + uy) * (unsigned)A.d0[2] + uz] : 0.0;
                    }
            const double v00 = v[0][0][0] + tz * (v[0][0][1] - v[0][0][0]), v01 = v[0][1][0] + tz * (v[0][1][1] - v[0][1][0]);
            const double v10 = v[1][0][0] + tz * (v[1][0][1] - v[1][0][0]), v11 = v[1][1][0] + tz * (v[1][1][1] - v[1][1][0]);
            const double v0 = v00 + ty * (v01 - v00), v1 = v10 + ty * (v11 - v10);
            g = (float)(v0 + tx * (v1 - v0));
        }
        if (out_g) out_g[i] = g;
        const double gd = (double)g;
        const bool w = gd > A.iso;
        if (Z) Z[(((((size_t)x) << A.logN) + y) << A.logN) + z] = w ? make_double2(gd, 1.0) : make_double2(0.0, 0.0);
        if (w) { vw = 1.0; vg = gd * gd; vs = gd; }      // 24 x 24 bits: exact
    }
    s[0][t] = vw; s[1][t] = vg; s[2][t] = vs;
    search_run_sum(s, t);
    if (t < 3) part[(size_t)blockIdx.x * 3 + t] = s[t][0];
}

// One level of tree_sum: out[b][3] = the sums of run b of in[n_in][3] (the last run zero-padded).  The host launches level after
// level until one record is left; the last level writes the rotation's record (n_w, G, S).
__global__ __launch_bounds__(SEARCH_RUN) void k_search_stats(const double *__restrict__ in, unsigned n_in, double *__restrict__ out) {
    __shared__ double s[3][SEARCH_RUN];
    const unsigned t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * SEARCH_RUN + t;
    const bool has = i < n_in;
    s[0][t] = has ? in[i * 3] : 0.0; s[1][t] = has ? in[i * 3 + 1] : 0.0; s[2][t] = has ? in[i * 3 + 2] : 0.0;
    search_run_sum(s, t);
    if (t < 3) out[(size_t)blockIdx.x * 3 + t] = s[t][0];
}

// mad_map_search: n_w, G and S come from the rotation's record rec[3]; gbar, G' and the floor are formed here in the contract's
// order.  A rotation with n_w = 0, G outside (0, 1.7e308] or (mode 1) G' <= 0 is skipped: it scores no offset, and *skipped is 1.
__global__ __launch_bounds__(256) void k_search_score(const double2 *__restrict__ Zt, const double2 *__restrict__ Zq, const ScoreArgs A,
                                                      const double *__restrict__ rec, float *__restrict__ best, int *__restrict__ best_r,
                                                      int *__restrict__ skipped) {
    const double S = rec[2];
    ScoreStat st = {rec[0], rec[1], 0.0};
    bool skip = !(st.n_w > 0.0) || !(st.G > 0.0 && st.G <= 1.7e308);
    if (!skip && A.mode) {
        st.gbar = S / st.n_w;
        st.G = st.G - st.n_w * (st.gbar * st.gbar);
        skip = !(st.G > 0.0);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *skipped = skip ? 1 : 0;
    if (skip && A.idx != 0) return;      // rotation 0 still initialises best / best_r
    scan_score_box(Zt, Zq, A, st, A.floor * st.n_w, skip, best, best_r);
}

// k_search_rotate and the levels of k_search_stats of one rotation; the record ends in rec.  part_a holds n_runs records, part_b
// ceil(n_runs / 256).  fill_wgs > 0: that many more workgroups zero the lattice outside the cube.
static void search_rotate_launch(mad_ctx *ctx, const SearchRotateArgs &A, const double *R, double2 *Z, float *out_g, double *part_a, double *part_b,
                                 double *rec, unsigned fill_wgs) {
    hipLaunchKernelGGL(k_search_rotate, dim3(A.n_runs + fill_wgs), dim3(SEARCH_RUN), 0, ctx->stream, A, R, Z, out_g, A.n_runs == 1 ? rec : part_a);
    double *in = part_a, *out = part_b;
    for (unsigned n = A.n_runs; n > 1;) {
        const unsigned m = (n + SEARCH_RUN - 1) / SEARCH_RUN;
        hipLaunchKernelGGL(k_search_stats, dim3(m), dim3(SEARCH_RUN), 0, ctx->stream, (const double *)in, n, m == 1 ? rec : out);
        std::swap(in, out);
        n = m;
    }
}

// finite, and max |R R^T - I| <= 1e-6
static bool search_rotation_ok(const double *R) {
    for (int i = 0; i < 9; i++)
        if (!(fabs(R[i]) <= 1.7e308)) return false;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double d = (R[3 * a] * R[3 * b] + R[3 * a + 1] * R[3 * b + 1]) + R[3 * a + 2] * R[3 * b + 2] - (a == b ? 1.0 : 0.0);
            if (!(fabs(d) <= 1e-6)) return false;
        }
    return true;
}

// what mad_map_search and mad_map_rotate refuse about the base template, the cube and the mask
static int search_check(mad_ctx *ctx, const char *who, const int32_t *d0, const double *c0, int32_t e, double iso) {
    MAD_TRY(fourier_check(ctx, who, d0, fourier_zero, 1.0));
    if (e < 1) return mad_fail(ctx, MAD_EINVAL, "%s: edge %d (1 or more)", who, e);
    for (int a = 0; a < 3; a++)
        if (!(fabs(c0[a]) <= 1.7e308)) return mad_fail(ctx, MAD_EINVAL, "%s: centre c0[%d] = %g is not finite", who, a, c0[a]);
    if (!(fabs(iso) <= 1.7e308)) return mad_fail(ctx, MAD_EINVAL, "%s: iso %g is not finite", who, iso);
    return MAD_OK;
}

static void search_rotate_args(SearchRotateArgs *A, const float *d_base, const int32_t *d0, const double *c0, int32_t e, double iso, int logN) {
    memset(A, 0, sizeof(*A));
    A->g0 = d_base;
    for (int a = 0; a < 3; a++) { A->d0[a] = d0[a]; A->c0[a] = c0[a]; }
    A->e = (unsigned)e;
    A->n_box = (size_t)e * e * e;
    A->n_runs = (unsigned)((A->n_box + SEARCH_RUN - 1) / SEARCH_RUN);
    A->logN = logN;
    A->c2 = ((double)e - 1.0) / 2.0;
    A->iso = iso;
}

extern "C" int mad_map_search(mad_ctx *ctx, const float *map, const int32_t dims1[3], const float *base, const int32_t dims0[3], const double c0[3],
                              int32_t edge, const double *rotations, int32_t n_r, double iso, double e_fill, int32_t mode, double min_score, int64_t k,
                              float *best, int32_t *best_r, double *peaks, int64_t *n_peaks, int64_t *n_found, int32_t *n_skipped, int32_t *N_out) {
    const char *who = "mad_map_search";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !dims1 || !dims0 || !c0 || (!best && !N_out) ||
        (best && (!map || !base || !rotations || !best_r || !n_peaks || !n_found || !n_skipped || (k > 0 && !peaks))))
        return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    if (n_r < 1) return mad_fail(ctx, MAD_EINVAL, "%s: %d rotations (1 or more)", who, n_r);
    MAD_TRY(fourier_check(ctx, who, dims1, fourier_zero, 1.0));
    MAD_TRY(search_check(ctx, who, dims0, c0, edge, iso));
    if (!(fabs(min_score) <= 1.7e308) || !(e_fill >= 0.0 && e_fill <= 1.7e308))
        return mad_fail(ctx, MAD_EINVAL, "%s: e_fill %g, min_score %g (finite, e_fill 0 or more)", who, e_fill, min_score);
    CorrPlan C;
    const int32_t cube[3] = {edge, edge, edge};
    MAD_TRY(corr_plan(ctx, who, "the cube is", dims1, cube, mode, k, N_out, &C));
    if (!best) return MAD_OK;      // the size query
    for (int32_t j = 0; j < n_r; j++)
        if (!search_rotation_ok(rotations + (size_t)9 * j))
            return mad_fail(ctx, MAD_EINVAL, "%s: rotation %d is not finite or not orthonormal (max |R R^T - I| > 1e-6)", who, j);
    const int N = C.N, logN = C.logN, e = edge;
    const size_t n0 = (size_t)dims0[0] * dims0[1] * dims0[2];

    // behind the output block: the rotations, their records and skip flags, and the partial sums of k_search_rotate / k_search_stats
    SearchRotateArgs RA;
    search_rotate_args(&RA, nullptr, dims0, c0, e, iso, logN);
    const size_t n_pb = (RA.n_runs + SEARCH_RUN - 1) / SEARCH_RUN;
    const size_t b_rot = (size_t)n_r * 72, b_rec = (size_t)n_r * 24, b_skip = ((size_t)n_r * 4 + 15) & ~(size_t)15;
    const size_t b_pa = (size_t)RA.n_runs * 24, b_pb = n_pb * 24;
    Lattices L(ctx);
    MAD_TRY(corr_setup(ctx, who, map, dims1, n0, b_rot + b_rec + b_skip + b_pa + b_pb, &C, &L));
    double2 *Zm = L.Z[0], *Zt = L.Z[1], *Zq = L.Z[2];
    float *d_base = scratch<float>(ctx, S_TMP_I);
    double *d_rot = (double *)C.tail(), *d_rec = (double *)(C.tail() + b_rot);
    int *d_skip = (int *)((char *)d_rec + b_rec);
    double *part_a = (double *)((char *)d_skip + b_skip), *part_b = (double *)((char *)part_a + b_pa);
    const bool prune = ctx->search_prune != 0;
    RA.g0 = d_base;

    // the base grid and the rotations go up once, as the map has
    MAD_HIP(hipMemcpyAsync(d_base, base, n0 * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_rot, rotations, b_rot, hipMemcpyHostToDevice, ctx->stream));

    ScoreArgs SA = corr_score_args(C, mode, e_fill);
    // tiles of 8 that cover the cube's lines (forward: only the cube is not zero) and the offsets' (inverse: only the box is read)
    const int nt = N / FFT_L, te = (e + FFT_L - 1) / FFT_L, tD2 = ((int)C.D[2] + FFT_L - 1) / FFT_L;
    const PrunedPass fwd[3] = {{te, e, e}, {nt, e, e}, {nt, N, e}}, inv[3] = {{nt, N, N}, {tD2, N, N}, {tD2, (int)C.D[1], N}};
    int rc = MAD_OK;
    mad_timer_begin(ctx, MAD_T_SEARCH);      // one interval around every rotation: no event, and so no wait, per rotation
    for (int32_t j = 0; j < n_r && rc == MAD_OK; j++) {
        double *rec = d_rec + (size_t)3 * j;
        search_rotate_launch(ctx, RA, d_rot + (size_t)9 * j, Zt, nullptr, part_a, part_b, rec, prune ? 0u : C.wg_Z);
        rc = fourier_passes(ctx, Zt, logN, prune ? fwd : nullptr);
        if (rc != MAD_OK) break;
        hipLaunchKernelGGL(k_scan_product, dim3((unsigned)N, (unsigned)(N / 2 + 1)), dim3(C.threads), 0, ctx->stream, (const double2 *)Zm, Zt, Zq, logN);
        for (int l = 1; l < C.n_lat && rc == MAD_OK; l++) rc = fourier_passes(ctx, L.Z[l], logN, prune ? inv : nullptr);
        if (rc != MAD_OK) break;
        SA.idx = j;
        hipLaunchKernelGGL(k_search_score, dim3(C.wg_D), dim3(256), 0, ctx->stream, (const double2 *)Zt, (const double2 *)Zq, SA, (const double *)rec,
                           C.best(), C.best_i(), d_skip + j);
    }
    mad_timer_end(ctx, MAD_T_SEARCH);
    if (rc != MAD_OK) return rc;
    MAD_HIP(hipGetLastError());
    std::vector<int> h_skip((size_t)n_r);
    MAD_HIP(hipMemcpyAsync(h_skip.data(), d_skip, (size_t)n_r * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));      // the one synchronisation before the peak search
    int32_t skipped = 0;
    for (int32_t j = 0; j < n_r; j++) skipped += h_skip[(size_t)j] != 0;
    MAD_TRY(scan_peaks_out(ctx, who, MAD_T_SEARCH, C, min_score, k, best, best_r, peaks, n_peaks, n_found));
    *n_skipped = skipped;
    return MAD_OK;
}

extern "C" int mad_map_rotate(mad_ctx *ctx, const float *base, const int32_t dims0[3], const double c0[3], int32_t edge, const double R[9], double iso,
                              float *out, double stats[3]) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !base || !dims0 || !c0 || !R || !out || !stats) return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_rotate: NULL argument") : MAD_EINVAL;
    const char *who = "mad_map_rotate";
    MAD_TRY(search_check(ctx, who, dims0, c0, edge, iso));
    if (edge > FFT_MAX_N) return mad_fail(ctx, MAD_EDOM, "%s: edge %d, more than %d", who, edge, FFT_MAX_N);
    if (!search_rotation_ok(R)) return mad_fail(ctx, MAD_EINVAL, "%s: the rotation is not finite or not orthonormal (max |R R^T - I| > 1e-6)", who);
    SearchRotateArgs RA;
    search_rotate_args(&RA, nullptr, dims0, c0, edge, iso, 0);
    const size_t n0 = (size_t)dims0[0] * dims0[1] * dims0[2], n_pb = (RA.n_runs + SEARCH_RUN - 1) / SEARCH_RUN;
    const size_t b_pa = (size_t)RA.n_runs * 24, b_pb = n_pb * 24, b_blk = 96 + b_pa + b_pb;
    size_t free_b = 0, total_b = 0;
    MAD_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t need = (RA.n_box + n0 + 8) * 5 + b_blk * 2 + ((size_t)8 << 20);
    if (need > free_b) return mad_fail(ctx, MAD_ENOMEM, "%s: %zu MiB of device memory needed, %zu MiB are free", who, need >> 20, free_b >> 20);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), (RA.n_box + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), (n0 + 4) * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), b_blk));
    float *d_out = scratch<float>(ctx, S_TMP_H), *d_base = scratch<float>(ctx, S_TMP_I);
    char *blk = scratch<char>(ctx, S_TMP_G);
    double *d_R = (double *)blk, *d_rec = (double *)(blk + 72), *part_a = (double *)(blk + 96), *part_b = (double *)(blk + 96 + b_pa);
    RA.g0 = d_base;
    MAD_HIP(hipMemcpyAsync(d_base, base, n0 * 4, hipMemcpyHostToDevice, ctx->stream));
    MAD_HIP(hipMemcpyAsync(d_R, R, 72, hipMemcpyHostToDevice, ctx->stream));
    mad_timer_begin(ctx, MAD_T_SEARCH);
    search_rotate_launch(ctx, RA, d_R, nullptr, d_out, part_a, part_b, d_rec, 0u);
    mad_timer_end(ctx, MAD_T_SEARCH);
    MAD_HIP(hipGetLastError());
    MAD_HIP(hipMemcpyAsync(out, d_out, RA.n_box * 4, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipMemcpyAsync(stats, d_rec, 24, hipMemcpyDeviceToHost, ctx->stream));
    MAD_HIP(hipStreamSynchronize(ctx->stream));
    return MAD_OK;
}
