// mad_localres.hip -- local resolution of a map by windowed Fourier shell correlation (mad_map_local_fsc), and a map's amplitudes
// scaled to a reference box by box (mad_map_local_scale): one front end, one forward transform, two tails.
// DESIGN.md section 4p has the contract of the first and mad_amd/fourier.py restates it as local_fsc_numpy; section 4v and
// local_scale_numpy are the second's.
//
// Per sample point of a lattice over grid 1 a cubic box of edge w = 8, 16 or 32 voxels is cut out of both grids (zero outside either),
// multiplied by a separable periodic Hann window and transformed as Z = FFT(w1 + i w2); the two spectra are separated, summed per
// shell exactly as section 4l does on the whole lattice, and the crossing of the curve with the threshold is the sample's value.
// All arithmetic is float64 without fused multiply-adds, no floating-point atomics, every sum in an order fixed by indices alone.
//
// w = 8 and 16: k_lr_box, one workgroup of w^2 threads per box (w = 8: one wave), load to result in LDS.
//   The image is complex128 [x][y][z] with rows of w + 1 elements.  A pass is w^2 lines of w points; a thread takes a whole line into
//   registers, runs an in-place radix-2 decimation-in-frequency transform there (twiddles with a constant index: scalar loads; the
//   products by 1 and -i are moves) and puts element i back at the bit-reversed place, so the image is in natural order after every
//   pass and the three passes are separated by barriers alone.
//   Banks.  MI355X serves a 16-byte read of a wave in four groups of 16 lanes over 64 banks of 4 bytes -- not consecutive lanes: the
//   groups are {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- and a 16-byte write in eight groups of 8 consecutive
//   lanes over 32 banks.  In the z pass lane k holds line k, and consecutive lines begin (w + 1) * 16 bytes apart: 68 dwords at
//   w = 16, 36 at w = 8.  The start bank of lane k is 4 k mod 64 at w = 16: within every read group the sixteen lanes (k = 0-3, 12-15,
//   20-27: 4 k = 0-12, 48-60, 80-108 = 16-44 mod 64, and so on) begin on sixteen different multiples of four banks, and the eight
//   lanes of a write group on eight different ones mod 32.  At w = 8 it is 36 k mod 64, which over k = 0-3, 12-15, 20-27 gives
//   0, 36, 8, 44, 48, 20, 56, 28, 16, 52, 24, 60, 32, 4, 40, 12: all different again.  Without the pad every lane would begin on
//   bank 0.  The fill and the y and x passes run the lanes over z, lane t at (u, v) = (t / w, t mod w); at w = 16 a read group then
//   holds eight lanes of one row and eight of the next, and the next row begins 68 dwords later: the pad moves
//   it by four banks, so one lane of the group lands on a bank another uses (lane 27 at dword 68 + 44 = bank 48, lane 12 at bank 48):
//   5 cycles for that group instead of 4.  That is the pad's price.
//   Shell sums: the host lists the box's lattice points with shell <= w / 2 in shell order and cuts the list into chunks that do not
//   span shells, at most one per thread.  A thread adds its chunk's P1, P2, C in list order (four points' reads in flight at a time),
//   the chunk sums of a shell are added in eight contiguous pieces (four at w = 8) by a thread each and the pieces in order by one,
//   a lane per shell forms fsc_s and lane 0 walks the curve.  That is the fixed order; nothing is atomic.  The ramp's three tables sit in LDS beside the image.
// w = 32: the box is 512 KiB and goes through a scratch buffer in batches of LR32_BATCH boxes (32 MiB: inside the Infinity Cache):
//   k_lr32_planes packs, windows and transforms two y-z planes per workgroup in LDS, k_lr32_xlines transforms the x lines in place
//   from registers (lanes over z: every access of a wave is 1 KiB contiguous), k_lr32_shells is the tail of k_lr_box on global memory.
// mad_map_local_scale runs the same fill and line passes (k_lr_box<W, true>; k_lr32_planes and k_lr32_xlines as they are) and ends in
//   ls_tail: its list holds every point of the box, the corners beyond shell w / 2 in the last shell's bucket, and a point gives P1, P2
//   and D = Re F1 (-1)^(a + b + c) where the other tail gives P1, P2 and C.  The chunk, piece and shell sums are lr_reduce's, shared;
//   a lane per shell forms the gain, one lane adds gain_s D_s in shell order and divides by w^3: the centre of the rescaled box.
//   No ramp (amplitudes do not see one), so no phi in LDS.
#include <algorithm>
#include <vector>

#include "mad_fft_common.h"
#include "mad_localscale_plan.h"

#define LR32_BATCH 64

struct LrTab {                     // views into ctx->lr_tab[i]
    const double *h;               // [w] the window
    const double2 *tw;             // [w] exp(-2 pi i k / w)
    const int2 *chunk;             // [n_chunks] first and one-past-last entry of pts
    const int *shell_c0;           // [w / 2 + 2] first chunk of every shell, and the end
    const unsigned short *pts;     // a << 10 | b << 5 | c, by shell, then by linear index
    int n_chunks;
};

struct LrArgs {
    const float *g1, *g2;
    int d1[3], d2[3];
    long long s[3];                // grid 2's voxel j sits at grid 1's index j + s
    int n_lat[3];                  // the sample lattice
    int step;
    const unsigned *list;          // linear sample indices, the selected ones in ascending order
    const double2 *phi;            // [3][w]
    double voxsp, thr;
    double *res;                   // [samples]
    int *shell;                    // [samples]
    double *sums;                  // [samples][w / 2 + 1][3] or NULL
    double *out;                   // mad_map_local_scale: [samples] the centre of the rescaled box
    double *gains;                 // [samples][w / 2 + 1] or NULL
};

template <int W> __device__ __forceinline__ constexpr int lr_brev(int i) {
    int r = 0;
    for (int b = 1; b < W; b <<= 1) { r = (r << 1) | (i & 1); i >>= 1; }
    return r;
}

// in-place radix-2 decimation in frequency: v[i] leaves as X[lr_brev(i)]; tw[k] = exp(-2 pi i k / W)
template <int W> __device__ __forceinline__ void lr_fft(double2 (&v)[W], const double2 *__restrict__ tw) {
#pragma unroll
    for (int len = W; len >= 2; len >>= 1) {
        const int half = len >> 1, stride = W / len;
#pragma unroll
        for (int b = 0; b < W; b += len) {
#pragma unroll
            for (int j = 0; j < half; j++) {
                const double2 a = v[b + j], c = v[b + j + half];
                v[b + j] = c_add(a, c);
                const double2 d = c_sub(a, c);
                const int k = j * stride;
                if (k == 0) v[b + j + half] = d;
                else if (k == W / 4) v[b + j + half] = make_double2(d.y, -d.x);      // times -i
                else v[b + j + half] = c_mul(d, tw[k]);
            }
        }
    }
}

// one line of an image: element n at p[n * stride]
template <int W, class P> __device__ __forceinline__ void lr_line(P p, int stride, const double2 *__restrict__ tw) {
    double2 v[W];
#pragma unroll
    for (int n = 0; n < W; n++) v[n] = p[n * stride];
    lr_fft<W>(v, tw);
#pragma unroll
    for (int n = 0; n < W; n++) p[lr_brev<W>(n) * stride] = v[n];
}

// where sample `idx` of the list sits: the grid-1 voxel of box index 0 on every axis
template <int W> __device__ __forceinline__ void lr_corner(const LrArgs &A, unsigned smp, int lo[3]) {
    const unsigned t = smp / (unsigned)A.n_lat[2], mz = smp - t * (unsigned)A.n_lat[2], mx = t / (unsigned)A.n_lat[1], my = t - mx * (unsigned)A.n_lat[1];
    lo[0] = (int)mx * A.step - W / 2; lo[1] = (int)my * A.step - W / 2; lo[2] = (int)mz * A.step - W / 2;
}

// the windowed pair at box index (x, y, z): (g1 h, g2 h), a voxel outside either grid 0 for that grid
__device__ __forceinline__ double2 lr_voxel(const LrArgs &A, int gx, double hx, bool okyz1, size_t off1, bool okyz2, size_t off2, double hy, double hz) {
    float v1 = 0.f, v2 = 0.f;
    if (okyz1 && (unsigned)gx < (unsigned)A.d1[0]) v1 = A.g1[(size_t)gx * A.d1[1] * A.d1[2] + off1];
    const long long jx = (long long)gx - A.s[0];
    if (okyz2 && jx >= 0 && jx < (long long)A.d2[0]) v2 = A.g2[(size_t)jx * A.d2[1] * A.d2[2] + off2];
    const double hw = (hx * hy) * hz;
    return make_double2((double)v1 * hw, (double)v2 * hw);
}

// the curve and its crossing: the expressions of fourier.FSC and FSC.resolution in their order
__device__ __forceinline__ double lr_fsc(const double *s3) {
    const double pp = s3[0] * s3[1];
    return pp > 0.0 ? s3[2] / sqrt(pp) : 0.0;
}
// fsc [W / 2 + 1]: the curve (a lane per shell made it); one lane walks it: comparisons first, the four divisions once
__device__ __forceinline__ void lr_crossing(const double *fsc, int W, double voxsp, double thr, double *res, int *shell) {
    const int SH = W / 2 + 1;
    int s = 1;
    while (s < SH && !(fsc[s] < thr)) s++;
    if (s == SH) {
        *res = 2.0 * voxsp;
        *shell = 0;
        return;
    }
    const double span = (double)W * voxsp, a = fsc[s - 1], b = fsc[s], fs = (double)s / span;
    double f = fs;
    if (a >= thr) {
        const double fp = (double)(s - 1) / span;
        f = fp + (fs - fp) * ((a - thr) / (a - b));
    }
    *res = 1.0 / f;
    *shell = s;
}

// Split, ramp, shell sums, curve and crossing of one box whose Z(k) is at Z[(a W + b) PZ + c]; phi [3][W] the ramp (LDS).  LDS of the
// caller: part n_chunks x 3 doubles, part2 LR_G(W) x 3 (W / 2 + 1), tab 3 (W / 2 + 1).  Every thread of the workgroup calls it, and
// the workgroup has LR_T(W) threads.  The order of every sum: a chunk's points in list order; the chunks of a shell in LR_G
// contiguous pieces, each in chunk order; the pieces in order.
template <int W> constexpr int LR_T() { return W == 32 ? 512 : W * W; }
template <int W> constexpr int LR_G() { return LR_T<W>() / (3 * (W / 2 + 1)) >= 8 ? 8 : 4; }

// part [n_chunks][3], the three sums of every chunk, written by the callers' threads before the call -> tab [W / 2 + 1][3], the three
// sums of every shell, and `keep` (global, may be NULL) the same.  Begins and ends with a barrier.
template <int W>
__device__ __forceinline__ void lr_reduce(const LrTab &Tb, const double *part, double *part2, double *tab, double *keep) {
    constexpr int SH = W / 2 + 1, G = LR_G<W>();
    static_assert(G * 3 * SH <= LR_T<W>(), "one thread per piece");
    const int t = (int)threadIdx.x;
    __syncthreads();
    if (t < G * 3 * SH) {
        const int g = t / (3 * SH), j = t - g * (3 * SH), s = j / 3, q = j - 3 * s;
        const int lo = Tb.shell_c0[s], n = Tb.shell_c0[s + 1] - lo;
        double v = 0.0;
        for (int c = lo + n * g / G; c < lo + n * (g + 1) / G; c++) v += part[3 * c + q];
        part2[t] = v;
    }
    __syncthreads();
    if (t < 3 * SH) {
        double v = part2[t];
#pragma unroll
        for (int g = 1; g < G; g++) v += part2[g * 3 * SH + t];
        tab[t] = v;
        if (keep) keep[t] = v;
    }
    __syncthreads();
}

template <int W, int PZ, class P>
__device__ __forceinline__ void lr_tail(P Z, const double2 *phi, const LrArgs &A, const LrTab &Tb, unsigned smp, double *part, double *part2,
                                        double *tab) {
    constexpr int SH = W / 2 + 1, T = LR_T<W>();
    const int t = (int)threadIdx.x;
    for (int c = t; c < Tb.n_chunks; c += T) {
        const int2 ch = Tb.chunk[c];
        double p1 = 0.0, p2 = 0.0, cr = 0.0;
#pragma unroll 4
        for (int e = ch.x; e < ch.y; e++) {      // (unrolled: the list reads and the gathers of four points are in flight together)
            const unsigned pt = Tb.pts[e];
            const int a = (int)(pt >> 10), b = (int)((pt >> 5) & 31u), cc = (int)(pt & 31u);
            const int ma = (W - a) & (W - 1), mb = (W - b) & (W - 1), mc = (W - cc) & (W - 1);
            const double2 z = Z[(a * W + b) * PZ + cc], zm = Z[(ma * W + mb) * PZ + mc];
            const double f1x = (z.x + zm.x) * 0.5, f1y = (z.y - zm.y) * 0.5;      // (Z(k) + conj Z(-k)) / 2
            const double f2x = (z.y + zm.y) * 0.5, f2y = (zm.x - z.x) * 0.5;      // (Z(k) - conj Z(-k)) / (2i)
            const double2 ph = c_mul(c_mul(phi[a], phi[W + b]), phi[2 * W + cc]);
            const double2 g = c_mul(make_double2(f2x, f2y), ph);
            p1 += f1x * f1x + f1y * f1y;
            p2 += f2x * f2x + f2y * f2y;
            cr += f1x * g.x + f1y * g.y;      // Re(F1 conj(F2 phi))
        }
        part[3 * c] = p1; part[3 * c + 1] = p2; part[3 * c + 2] = cr;
    }
    lr_reduce<W>(Tb, part, part2, tab, A.sums ? A.sums + (size_t)smp * (3 * SH) : nullptr);
    if (t < SH) part2[t] = lr_fsc(tab + 3 * t);      // (part2 has been read: the barrier that ends lr_reduce)
    __syncthreads();
    if (t == 0) {
        double r;
        int sh;
        lr_crossing(part2, W, A.voxsp, A.thr, &r, &sh);
        A.res[smp] = r;
        A.shell[smp] = sh;
    }
}

// The tail of mad_map_local_scale: split, shell sums, gains and the centre of the rescaled box, Z and the LDS as lr_tail has them
// (no ramp).  Tb lists every point of the box, the corners in shell W / 2's bucket.  Per point P1 += |F1|^2, P2 += |F2|^2 and
// D += Re F1 (-1)^(a + b + c): exp(2 pi i k . (W / 2, W / 2, W / 2) / W) is that sign, and F1(-k) = conj F1(k) makes the imaginary
// parts cancel over a shell, so (1 / W^3) sum_s gain_s D_s is the real part of the inverse transform of gain F1 at the box's centre.
// The order of every sum is lr_tail's; one lane adds the W / 2 + 1 products in shell order.
template <int W, int PZ, class P>
__device__ __forceinline__ void ls_tail(P Z, const LrArgs &A, const LrTab &Tb, unsigned smp, double *part, double *part2, double *tab) {
    constexpr int SH = W / 2 + 1, T = LR_T<W>();
    const int t = (int)threadIdx.x;
    for (int c = t; c < Tb.n_chunks; c += T) {
        const int2 ch = Tb.chunk[c];
        double p1 = 0.0, p2 = 0.0, d = 0.0;
#pragma unroll 4
        for (int e = ch.x; e < ch.y; e++) {
            const unsigned pt = Tb.pts[e];
            const int a = (int)(pt >> 10), b = (int)((pt >> 5) & 31u), cc = (int)(pt & 31u);
            const int ma = (W - a) & (W - 1), mb = (W - b) & (W - 1), mc = (W - cc) & (W - 1);
            const double2 z = Z[(a * W + b) * PZ + cc], zm = Z[(ma * W + mb) * PZ + mc];
            const double f1x = (z.x + zm.x) * 0.5, f1y = (z.y - zm.y) * 0.5;      // (Z(k) + conj Z(-k)) / 2
            const double f2x = (z.y + zm.y) * 0.5, f2y = (zm.x - z.x) * 0.5;      // (Z(k) - conj Z(-k)) / (2i)
            p1 += f1x * f1x + f1y * f1y;
            p2 += f2x * f2x + f2y * f2y;
            d += ((a + b + cc) & 1) ? -f1x : f1x;
        }
        part[3 * c] = p1; part[3 * c + 1] = p2; part[3 * c + 2] = d;
    }
    lr_reduce<W>(Tb, part, part2, tab, nullptr);
    if (t < SH) {      // (part2 has been read: the barrier that ends lr_reduce)
        const double p1 = tab[3 * t], p2 = tab[3 * t + 1];
        double g = 0.0;
        if (p1 > 0.0) {
            g = sqrt(p2 / p1);
            if (!(g <= 1.7976931348623157e308)) g = 0.0;      // a quotient that is not finite: no gain
        }
        part2[t] = g;
        if (A.gains) A.gains[(size_t)smp * SH + t] = g;
    }
    __syncthreads();
    if (t == 0) {
        double v = 0.0;
        for (int s = 0; s < SH; s++) v += part2[s] * tab[3 * s + 2];
        A.out[smp] = v / (double)(W * W * W);
    }
}

// k_lr_box's dynamic LDS is lsp_box_lds(W, n_chunks, !SCALE): the image W^2 (W + 1) complex128, the ramp 3 W complex128 (not SCALE),
// then the doubles of the tail; the plan header's thread and piece counts are the kernels'
static_assert(LR_T<8>() == 64 && LR_T<16>() == 256 && LR_T<32>() == 512 && LR_G<8>() == 4 && LR_G<16>() == 8 && LR_G<32>() == 8, "mad_localscale_plan.h");

// SCALE: mad_map_local_scale -- the same fill and passes, no ramp, ls_tail
template <int W, bool SCALE>
__global__ __launch_bounds__(W * W) void k_lr_box(const LrArgs A, const LrTab Tb, unsigned first) {
    extern __shared__ __attribute__((aligned(16))) double2 lr_img[];
    constexpr int PZ = W + 1, SH = W / 2 + 1;
    double2 *phi = lr_img + W * W * PZ;
    double *part = (double *)(phi + (SCALE ? 0 : 3 * W)), *part2 = part + 3 * Tb.n_chunks, *tab = part2 + LR_G<W>() * 3 * SH;
    if (!SCALE && threadIdx.x < 3 * W) phi[threadIdx.x] = A.phi[threadIdx.x];
    const unsigned smp = A.list[first + blockIdx.x];
    int lo[3];
    lr_corner<W>(A, smp, lo);
    const int t = (int)threadIdx.x, u = t / W, v = t - u * W;      // u, v: the two box indices a thread's line is fixed by
    {      // fill: a thread takes (y, z) = (u, v) at every x; the lanes run over z
        const int gy = lo[1] + u, gz = lo[2] + v;
        const long long jy = (long long)gy - A.s[1], jz = (long long)gz - A.s[2];
        const bool ok1 = (unsigned)gy < (unsigned)A.d1[1] && (unsigned)gz < (unsigned)A.d1[2];
        const bool ok2 = jy >= 0 && jy < (long long)A.d2[1] && jz >= 0 && jz < (long long)A.d2[2];
        const size_t off1 = ok1 ? (size_t)gy * A.d1[2] + gz : 0, off2 = ok2 ? (size_t)jy * A.d2[2] + (size_t)jz : 0;
        const double hy = Tb.h[u], hz = Tb.h[v];
#pragma unroll
        for (int x = 0; x < W; x++) lr_img[(x * W + u) * PZ + v] = lr_voxel(A, lo[0] + x, Tb.h[x], ok1, off1, ok2, off2, hy, hz);
    }
    __syncthreads();
    lr_line<W>(lr_img + (u * W + v) * PZ, 1, Tb.tw);                 // along z: (x, y) = (u, v)
    __syncthreads();
    lr_line<W>(lr_img + u * W * PZ + v, PZ, Tb.tw);                  // along y: (x, z) = (u, v)
    __syncthreads();
    lr_line<W>(lr_img + u * PZ + v, W * PZ, Tb.tw);                  // along x: (y, z) = (u, v)
    __syncthreads();
    if constexpr (SCALE) ls_tail<W, PZ>((const double2 *)lr_img, A, Tb, smp, part, part2, tab);
    else lr_tail<W, PZ>((const double2 *)lr_img, (const double2 *)phi, A, Tb, smp, part, part2, tab);
}

// ---------------------------------------------------------------------------
// w = 32: through the scratch buffer Zb [box of the batch][x][y][z]
// ---------------------------------------------------------------------------

// blockIdx.x: the pair of planes x = 2 blockIdx.x, + 1; blockIdx.y: the box of the batch (list entry first + blockIdx.y)
__global__ __launch_bounds__(64) void k_lr32_planes(const LrArgs A, const LrTab Tb, unsigned first, double2 *__restrict__ Zb) {
    constexpr int W = 32, PZ = W + 1;
    __shared__ __attribute__((aligned(16))) double2 img[2 * W * PZ];
    const unsigned smp = A.list[first + blockIdx.y];
    int lo[3];
    lr_corner<W>(A, smp, lo);
    const int t = (int)threadIdx.x, pl = t >> 5, v = t & 31, x = 2 * (int)blockIdx.x + pl;
    double2 *mine = img + pl * W * PZ;
    {      // fill: a thread takes z = v of its plane at every y
        const int gx = lo[0] + x, gz = lo[2] + v;
        const long long jz = (long long)gz - A.s[2];
        const bool z1 = (unsigned)gz < (unsigned)A.d1[2], z2 = jz >= 0 && jz < (long long)A.d2[2];
        const double hx = Tb.h[x], hz = Tb.h[v];
#pragma unroll 4
        for (int y = 0; y < W; y++) {
            const int gy = lo[1] + y;
            const long long jy = (long long)gy - A.s[1];
            const bool ok1 = z1 && (unsigned)gy < (unsigned)A.d1[1], ok2 = z2 && jy >= 0 && jy < (long long)A.d2[1];
            const size_t off1 = ok1 ? (size_t)gy * A.d1[2] + gz : 0, off2 = ok2 ? (size_t)jy * A.d2[2] + (size_t)jz : 0;
            mine[y * PZ + v] = lr_voxel(A, gx, hx, ok1, off1, ok2, off2, Tb.h[y], hz);
        }
    }
    __syncthreads();
    lr_line<W>(mine + v * PZ, 1, Tb.tw);      // along z: y = v
    __syncthreads();
    {      // along y: z = v, from LDS into registers and out to the scratch buffer
        double2 r[W];
#pragma unroll
        for (int n = 0; n < W; n++) r[n] = mine[n * PZ + v];
        lr_fft<W>(r, Tb.tw);
        double2 *out = Zb + ((size_t)blockIdx.y * W + x) * W * W + v;
#pragma unroll
        for (int n = 0; n < W; n++) out[lr_brev<W>(n) * W] = r[n];
    }
}

// blockIdx.x * 64 + threadIdx.x: the line (y, z) of box blockIdx.y
__global__ __launch_bounds__(64) void k_lr32_xlines(const LrTab Tb, double2 *__restrict__ Zb) {
    constexpr int W = 32;
    lr_line<W>(Zb + (size_t)blockIdx.y * W * W * W + blockIdx.x * 64 + threadIdx.x, W * W, Tb.tw);
}

#define LR32_TAIL_THREADS 512
__global__ __launch_bounds__(LR32_TAIL_THREADS) void k_lr32_shells(const LrArgs A, const LrTab Tb, unsigned first, const double2 *__restrict__ Zb) {
    constexpr int W = 32;
    __shared__ __attribute__((aligned(16))) double2 phi[3 * W];
    __shared__ double part[3 * LR32_TAIL_THREADS], part2[LR_G<W>() * 3 * (W / 2 + 1)], tab[3 * (W / 2 + 1)];
    if (threadIdx.x < 3 * W) phi[threadIdx.x] = A.phi[threadIdx.x];
    __syncthreads();
    lr_tail<W, W>(Zb + (size_t)blockIdx.x * W * W * W, (const double2 *)phi, A, Tb, A.list[first + blockIdx.x], part, part2, tab);
}

__global__ __launch_bounds__(LR32_TAIL_THREADS) void k_ls32_shells(const LrArgs A, const LrTab Tb, unsigned first, const double2 *__restrict__ Zb) {
    constexpr int W = 32;
    __shared__ double part[3 * LR32_TAIL_THREADS], part2[LR_G<W>() * 3 * (W / 2 + 1)], tab[3 * (W / 2 + 1)];
    ls_tail<W, W>(Zb + (size_t)blockIdx.x * W * W * W, A, Tb, A.list[first + blockIdx.x], part, part2, tab);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

static int lr_slot(int W) { return W == 8 ? 0 : (W == 16 ? 1 : 2); }
static_assert(LR_T<32>() == LR32_TAIL_THREADS, "k_lr32_shells, k_ls32_shells");

// byte offsets of the table's parts
struct LrLayout { size_t h, tw, chunk, c0, pts, bytes; };
static LrLayout lr_layout(int W, int n_chunks, int n_pts) {
    LrLayout L;
    L.h = 0;
    L.tw = L.h + (size_t)W * 8;
    L.chunk = L.tw + (size_t)W * 16;
    L.c0 = L.chunk + (size_t)n_chunks * 8;
    L.pts = (L.c0 + (size_t)(W / 2 + 2) * 4 + 15) & ~(size_t)15;
    L.bytes = (L.pts + (size_t)n_pts * 2 + 15) & ~(size_t)15;
    return L;
}

// the window, the twiddles and the shell-ordered point list of edge W on the device, built when first asked for; `corners`: the list
// of mad_map_local_scale (every point, the corners in the last shell's bucket), a table of its own
static int lr_tables(mad_ctx *ctx, int W, bool corners, LrTab *Tb) {
    const int slot = lr_slot(W) + (corners ? 3 : 0);
    if (!ctx->lr_n[slot][0]) {
        LsPlan P;
        lsp_plan(W, corners, P);
        const int n_chunks = P.n_chunks(), n_pts = P.n_pts();
        const LrLayout L = lr_layout(W, n_chunks, n_pts);
        std::vector<char> blob(L.bytes, 0);
        double *h = (double *)(blob.data() + L.h), *tw = (double *)(blob.data() + L.tw);
        for (int n = 0; n < W; n++) {
            double c, s;
            unit_root(n, W, &c, &s);
            h[n] = 0.5 - 0.5 * c;
            tw[2 * n] = c; tw[2 * n + 1] = -s;
        }
        std::copy(P.chunk.begin(), P.chunk.end(), (int *)(blob.data() + L.chunk));
        std::copy(P.c0.begin(), P.c0.end(), (int *)(blob.data() + L.c0));
        std::copy(P.pts.begin(), P.pts.end(), (unsigned short *)(blob.data() + L.pts));
        MAD_TRY(mad_reserve(ctx, ctx->lr_tab[slot], L.bytes));
        MAD_HIP(hipMemcpy(ctx->lr_tab[slot].p, blob.data(), L.bytes, hipMemcpyHostToDevice));
        ctx->lr_n[slot][0] = n_chunks; ctx->lr_n[slot][1] = n_pts; ctx->lr_n[slot][2] = P.per;
    }
    const LrLayout L = lr_layout(W, ctx->lr_n[slot][0], ctx->lr_n[slot][1]);
    const char *p = (const char *)ctx->lr_tab[slot].p;
    Tb->h = (const double *)(p + L.h); Tb->tw = (const double2 *)(p + L.tw); Tb->chunk = (const int2 *)(p + L.chunk);
    Tb->shell_c0 = (const int *)(p + L.c0); Tb->pts = (const unsigned short *)(p + L.pts); Tb->n_chunks = ctx->lr_n[slot][0];
    return MAD_OK;
}

static int lr_check_grid(mad_ctx *ctx, const char *who, const int32_t d[3], const double o[3], double voxsp) {
    for (int k = 0; k < 3; k++) {
        if (d[k] <= 0) return mad_fail(ctx, MAD_EINVAL, "%s: empty grid (%d x %d x %d)", who, d[0], d[1], d[2]);
        if (!(fabs(o[k]) <= 1.7e308)) return mad_fail(ctx, MAD_EINVAL, "%s: origin %g", who, o[k]);
    }
    const unsigned long long v = (unsigned long long)d[0] * (unsigned long long)d[1];
    if (v >= (1ull << 32) || v * (unsigned long long)d[2] >= (1ull << 32))
        return mad_fail(ctx, MAD_EINVAL, "%s: %d x %d x %d voxels: grids of 2^32 voxels or more are not supported", who, d[0], d[1], d[2]);
    return MAD_OK;
}

// A grid may not have 2^32 threads: the boxes go in rounds of at most LR_ROUND workgroups, one after the
// other on the stream, each with its offset into the list.  The attribute is set on every call: it belongs to the device the call
// runs on, and setting it costs nothing.
#define LR_ROUND ((size_t)1 << 22)
template <int W, bool SCALE> static int lr_launch_box(mad_ctx *ctx, const LrArgs &A, const LrTab &Tb, size_t n_sel) {
    const size_t lds = lsp_box_lds(W, Tb.n_chunks, !SCALE);
    MAD_HIP(hipFuncSetAttribute((const void *)k_lr_box<W, SCALE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (size_t first = 0; first < n_sel; first += LR_ROUND)
        hipLaunchKernelGGL((k_lr_box<W, SCALE>), dim3((unsigned)std::min(LR_ROUND, n_sel - first)), dim3(W * W), lds, ctx->stream, A, Tb, (unsigned)first);
    return MAD_OK;
}
static_assert(LR_ROUND * 16 * 16 < ((size_t)1 << 32), "threads of a round of k_lr_box<16>");

// what mad_reserve would allocate to bring a buffer to `need` bytes (its 25 % slack included), 0 where the buffer holds them already
static size_t lr_growth(const DevBuf &b, size_t need) { return b.cap >= need ? 0 : need + need / 4 + 512; }

// The front end of both calls.  scale == false: mad_map_local_fsc, `resolution`, `shell` and `sums` ([samples][SH][3]) its outputs.
// scale == true: mad_map_local_scale, `resolution` is its `out`, `sums` its `gains` ([samples][SH]), `shell` and `thr` are not used.
static int map_local_run(mad_ctx *ctx, bool scale, const float *g1, const int32_t *d1, const double *o1, const float *g2, const int32_t *d2,
                         const double *o2, double voxsp, int32_t W, int32_t step, double thr, const uint8_t *select, double *resolution,
                         int32_t *shell, double *sums, int32_t *n_out) {
    const char *who = scale ? "mad_map_local_scale" : "mad_map_local_fsc";
    if (W != 8 && W != 16 && W != 32) return mad_fail(ctx, MAD_EINVAL, "%s: box %d (8, 16 or 32)", who, W);
    if (step < 1) return mad_fail(ctx, MAD_EINVAL, "%s: step %d (1 or more)", who, step);
    if (!scale && !(thr > -1.0 && thr < 1.0)) return mad_fail(ctx, MAD_EINVAL, "%s: threshold %g (inside (-1, 1))", who, thr);
    if (!(voxsp > 0) || !(voxsp < 1e15)) return mad_fail(ctx, MAD_EINVAL, "%s: voxsp %g", who, voxsp);
    MAD_TRY(lr_check_grid(ctx, who, d1, o1, voxsp));
    MAD_TRY(lr_check_grid(ctx, who, d2, o2, voxsp));
    LrArgs A;
    memset(&A, 0, sizeof(A));
    double delta[3];
    for (int k = 0; k < 3; k++) {
        const double d = o2[k] / voxsp - o1[k] / voxsp;
        if (!(fabs(d) < 1e15)) return mad_fail(ctx, MAD_EDOM, "%s: the origins are %g voxels apart on axis %d (1e15 or more)", who, d, k);
        const long s = py_round(d);
        delta[k] = d - (double)s;
        A.s[k] = (long long)s;
        A.d1[k] = d1[k]; A.d2[k] = d2[k];
        A.n_lat[k] = (d1[k] - 1) / step + 1;
    }
    for (int k = 0; k < 3; k++) n_out[k] = A.n_lat[k];
    if (!resolution) return MAD_OK;      // the size query
    const int SH = W / 2 + 1;
    const size_t n = (size_t)A.n_lat[0] * A.n_lat[1] * A.n_lat[2], n1 = (size_t)d1[0] * d1[1] * d1[2], n2 = (size_t)d2[0] * d2[1] * d2[2];
    std::vector<unsigned> list;
    list.reserve(select ? 0 : n);
    for (size_t i = 0; i < n; i++)
        if (!select || select[i]) list.push_back((unsigned)i);
    const size_t n_sel = list.size();
    if (n_sel >= ((size_t)1 << 31)) return mad_fail(ctx, MAD_EDOM, "%s: %zu samples selected (2^31 or more)", who, n_sel);
    // device memory, judged before anything is allocated: the grids, the list and the ramp, the outputs, the scratch of w = 32
    const size_t b_list = ((n_sel + 4) * 4 + 15) & ~(size_t)15, b_phi = scale ? 0 : (size_t)3 * W * 16, n_per = (size_t)SH * (scale ? 1 : 3);
    const size_t b_res = n * 8, b_shell = scale ? 0 : (n * 4 + 15) & ~(size_t)15, b_sums = sums ? n * n_per * 8 : 0;
    const size_t b_scratch = W == 32 ? (size_t)std::min<size_t>(std::max<size_t>(n_sel, 1), LR32_BATCH) * W * W * W * 16 : 0;
    const size_t need_h = (n1 + 4) * 4, need_i = (n2 + 4) * 4, need_g = b_list + b_phi + b_scratch, need_j = b_res + b_shell + b_sums;
    if (n_sel == 0) {      // nothing to compute: nothing allocated or launched
        std::fill(resolution, resolution + n, 0.0);
        if (!scale) std::fill(shell, shell + n, -1);
        if (sums) std::fill(sums, sums + n * n_per, 0.0);
        return MAD_OK;
    }
    {      // buffer by buffer: what each would have to grow by (a buffer that is released to grow gives its bytes back first)
        size_t free_b = 0, total_b = 0;
        MAD_HIP(hipMemGetInfo(&free_b, &total_b));
        const DevBuf *buf[4] = {&mad_sb(ctx, S_TMP_H), &mad_sb(ctx, S_TMP_I), &mad_sb(ctx, S_TMP_G), &mad_sb(ctx, S_TMP_J)};
        const size_t need[4] = {need_h, need_i, need_g, need_j};
        size_t grow = (size_t)8 << 20, back = 0;
        for (int k = 0; k < 4; k++)
            if (lr_growth(*buf[k], need[k])) { grow += lr_growth(*buf[k], need[k]); back += buf[k]->cap; }
        if (grow > free_b + back)
            return mad_fail(ctx, MAD_ENOMEM, "%s: %zu samples of box %d need %zu MiB more device memory, %zu MiB are free", who, n, W, (grow - back) >> 20, free_b >> 20);
    }
    LrTab Tb;
    MAD_TRY(lr_tables(ctx, W, scale, &Tb));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), need_h));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), need_i));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), need_g));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_J), need_j));
    char *blk = scratch<char>(ctx, S_TMP_G), *out = scratch<char>(ctx, S_TMP_J);
    double2 *Zb = (double2 *)(blk + b_list + b_phi);
    A.g1 = scratch<float>(ctx, S_TMP_H); A.g2 = scratch<float>(ctx, S_TMP_I);
    A.step = step; A.voxsp = voxsp; A.thr = thr;
    A.list = (const unsigned *)blk; A.phi = (const double2 *)(blk + b_list);
    double *const d_res = (double *)out, *const d_sums = sums ? (double *)(out + b_res + b_shell) : nullptr;
    if (scale) { A.out = d_res; A.gains = d_sums; }
    else { A.res = d_res; A.shell = (int *)(out + b_res); A.sums = d_sums; }
    std::vector<double> h_phi((size_t)6 * W);
    for (int ax = 0; ax < 3; ax++)
        for (int a = 0; a < W; a++) {
            const double f = (double)(a < W / 2 ? a : a - W);
            const double ang = 2.0 * M_PI * (f * delta[ax]) / (double)W;
            h_phi[((size_t)ax * W + a) * 2] = cos(ang);
            h_phi[((size_t)ax * W + a) * 2 + 1] = -sin(ang);
        }
    // `list` and `h_phi` are pageable and read by asynchronous copies: whatever happens below, the stream is waited for before this
    // function, which owns them, returns
    const auto enqueue = [&]() -> int {
        MAD_HIP(hipMemcpyAsync((void *)A.g1, g1, n1 * 4, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)A.g2, g2, n2 * 4, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)A.list, list.data(), n_sel * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!scale) MAD_HIP(hipMemcpyAsync((void *)A.phi, h_phi.data(), b_phi, hipMemcpyHostToDevice, ctx->stream));      // (amplitudes see no ramp)
        if (n_sel < n) {      // what no box writes: 0.0, -1 and zero sums (or gains)
            MAD_HIP(hipMemsetAsync(d_res, 0, b_res, ctx->stream));
            if (!scale) MAD_HIP(hipMemsetAsync(A.shell, 0xff, n * 4, ctx->stream));
            if (sums) MAD_HIP(hipMemsetAsync(d_sums, 0, b_sums, ctx->stream));
        }
        const int timer = scale ? MAD_T_LOCALSCALE : MAD_T_LOCALRES;
        mad_timer_begin(ctx, timer);
        int rc = MAD_OK;
        if (W == 8) rc = scale ? lr_launch_box<8, true>(ctx, A, Tb, n_sel) : lr_launch_box<8, false>(ctx, A, Tb, n_sel);
        else if (W == 16) rc = scale ? lr_launch_box<16, true>(ctx, A, Tb, n_sel) : lr_launch_box<16, false>(ctx, A, Tb, n_sel);
        else {
            for (size_t first = 0; first < n_sel; first += LR32_BATCH) {      // batch after batch on the stream, no host synchronisation
                const unsigned nb = (unsigned)std::min<size_t>(LR32_BATCH, n_sel - first);
                hipLaunchKernelGGL(k_lr32_planes, dim3(16, nb), dim3(64), 0, ctx->stream, A, Tb, (unsigned)first, Zb);
                hipLaunchKernelGGL(k_lr32_xlines, dim3(16, nb), dim3(64), 0, ctx->stream, Tb, Zb);
                if (scale) hipLaunchKernelGGL(k_ls32_shells, dim3(nb), dim3(LR32_TAIL_THREADS), 0, ctx->stream, A, Tb, (unsigned)first, (const double2 *)Zb);
                else hipLaunchKernelGGL(k_lr32_shells, dim3(nb), dim3(LR32_TAIL_THREADS), 0, ctx->stream, A, Tb, (unsigned)first, (const double2 *)Zb);
            }
        }
        mad_timer_end(ctx, timer);
        if (rc != MAD_OK) return rc;
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(resolution, d_res, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (!scale) MAD_HIP(hipMemcpyAsync(shell, A.shell, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (sums) MAD_HIP(hipMemcpyAsync(sums, d_sums, b_sums, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));
        return MAD_OK;
    };
    const int rc = enqueue();
    if (rc != MAD_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

extern "C" int mad_map_local_fsc(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3], const float *grid2,
                                 const int32_t dims2[3], const double origin2[3], double voxsp, int32_t box, int32_t step, double threshold,
                                 const uint8_t *select, double *resolution, int32_t *shell, double *sums, int32_t n_out[3]) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !dims1 || !origin1 || !grid2 || !dims2 || !origin2 || !n_out || (resolution && !shell))
        return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_local_fsc: NULL argument") : MAD_EINVAL;
    const int rc = map_local_run(ctx, false, grid1, dims1, origin1, grid2, dims2, origin2, voxsp, box, step, threshold, select, resolution, shell,
                                 sums, n_out);
    return rc;
}

extern "C" int mad_map_local_scale(mad_ctx *ctx, const float *grid1, const int32_t dims1[3], const double origin1[3], const float *grid2,
                                   const int32_t dims2[3], const double origin2[3], double voxsp, int32_t box, int32_t step,
                                   const uint8_t *select, double *out, double *gains, int32_t n_out[3]) {
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid1 || !dims1 || !origin1 || !grid2 || !dims2 || !origin2 || !n_out)
        return ctx ? mad_fail(ctx, MAD_EINVAL, "mad_map_local_scale: NULL argument") : MAD_EINVAL;
    return map_local_run(ctx, true, grid1, dims1, origin1, grid2, dims2, origin2, voxsp, box, step, 0.0, select, out, nullptr, gains, n_out);
}
