// mad_localfilter.hip -- a low-pass whose width varies from voxel to voxel (mad_map_local_filter).  DESIGN.md section 4q has the
// contract; mad_amd/fourier.py restates it as local_sigma_numpy / local_filter_numpy.
//
// Every output voxel is the map under the Gaussian of its own resolution d: sigma = d / (voxsp pi sqrt(2)) voxels, interpolated
// trilinearly from a field of samples at every step-th voxel, truncated at R = max(1, (int)(4 sigma + 0.5)) taps either way and
// zero-extended as mad_map_smooth does, normalised by the cube of the tap sum.  Once sigma differs per voxel the three passes of
// k_seg_smooth_axis no longer separate, so this is the direct gather: (2 R + 1)^3 taps per voxel, float64, no atomics on data.
//
// k_lf_tile: a workgroup of LF_THREADS = 512 threads owns a tile of 8 x 8 x 32 outputs, four per thread, the lanes along z.
//   1. Every thread interpolates sigma of its outputs from the eight samples around each (the field is small and stays in L2); the
//      tile's largest radius H is reduced through one LDS word.  The halo is H, not the global cap: at R = 24 no tile would fit.
//   2. The tile and its halo are staged in LDS as float32 (the input is float32: exact, and half the bytes), a voxel outside the
//      grid as 0.0, in planes of (8 + 2 H) rows of (32 + 2 H) floats.  8 + 2 H planes are needed along x; where they do not fit into
//      the launch's LDS they are staged in slabs of as many as fit (lf_slab), and a thread carries its sum over dx from slab to slab
//      through a private float64 slot of LDS.  H <= 8 fits at once (110 KiB); at H = 24 a slab is 8 planes.
//   3. Per output: the R + 1 weights w_k = exp(q k k) in registers (LfW: two vectors of 16 float64, no memory behind them); then
//      S = sum_dx w_|dx| (sum_dy w_|dy| (sum_dz ...)) with the loops over dx and dy run by the whole wave over the wave's largest R,
//      Rw -- so that all lanes read the same rows of LDS, 32 consecutive floats per half wave, free of bank conflicts.  The code of
//      the loops is specialised on Rw (lf_planes<RW, UNI>, 24 x 2 copies): the 2 Rw + 1 reads of a row are issued together with
//      compile-time offsets and no branch between them.  UNI: every lane that takes part has R == Rw, the common case of a smooth
//      field; otherwise a lane keeps its sums unchanged wherever |dx|, |dy| or k exceeds its own R, so that what lies beyond a
//      lane's R never enters its result: a bad voxel (inf, NaN) spoils exactly the outputs whose kernel covers it.  The innermost
//      sum pairs the taps, a = fma(w_k, g[-k] + g[+k], a), k ascending: the order is fixed by the inputs alone, so two calls give
//      the same bits.
// Work per pair of taps: one ds_read2_b32 (or two ds_read_b32), two float32 -> float64 conversions, an add and an fma.
#include <algorithm>

#include "mad_common.h"
#include "mad_localfilter_plan.h"

struct LfArgs {
    const float *g;
    const double *res;             // [m0][m1][m2]
    int n[3], m[3];
    int step;
    double inv;                    // voxsp * K
    double *out64;
    float *out;
    double *sigma;                 // or NULL
    unsigned ty, tz;               // tiles along y and z
    unsigned lds;                  // the launch's dynamic LDS
};

// one axis of the contract: j0 = min(i / s, m - 1), j1 = min(j0 + 1, m - 1), f = (i - j0 s) / s, 0.0 where j1 == j0
__device__ __forceinline__ void lf_axis(int i, int s, int m, int *j0, int *j1, double *f) {
    const int a = min(i / s, m - 1), b = min(a + 1, m - 1);
    *j0 = a;
    *j1 = b;
    *f = b == a ? 0.0 : (double)(i - a * s) / (double)s;
}
__device__ __forceinline__ double lf_lerp(double a, double b, double f) { return a + (b - a) * f; }

// sigma in voxels at voxel (x, y, z): trilinear along z, then y, then x, then d / (voxsp K) -- the contract's operations in its order
__device__ __forceinline__ double lf_sigma(const LfArgs &A, int x, int y, int z) {
    int x0, x1, y0, y1, z0, z1;
    double fx, fy, fz;
    lf_axis(x, A.step, A.m[0], &x0, &x1, &fx);
    lf_axis(y, A.step, A.m[1], &y0, &y1, &fy);
    lf_axis(z, A.step, A.m[2], &z0, &z1, &fz);
    const double *r00 = A.res + ((size_t)x0 * A.m[1] + y0) * A.m[2], *r01 = A.res + ((size_t)x0 * A.m[1] + y1) * A.m[2];
    const double *r10 = A.res + ((size_t)x1 * A.m[1] + y0) * A.m[2], *r11 = A.res + ((size_t)x1 * A.m[1] + y1) * A.m[2];
    const double c00 = lf_lerp(r00[z0], r00[z1], fz), c01 = lf_lerp(r01[z0], r01[z1], fz);
    const double c10 = lf_lerp(r10[z0], r10[z1], fz), c11 = lf_lerp(r11[z0], r11[z1], fz);
    const double c0 = lf_lerp(c00, c01, fy), c1 = lf_lerp(c10, c11, fy);
    return lf_lerp(c0, c1, fx) / A.inv;
}

// the largest v of the wavefront, in a scalar register; every lane of the wave calls it
__device__ __forceinline__ int lf_wave_max(int v) {
#pragma unroll
    for (int o = MAD_WAVE / 2; o; o >>= 1) v = max(v, __shfl_xor(v, o, MAD_WAVE));
    return __builtin_amdgcn_readfirstlane(v);
}

// The weights of one output, k = 0 .. LF_MAX_R, as two vectors of 16 float64: values, not memory, so they stay in registers.  In the
// unrolled loops k is a compile-time constant and lf_w names a register; in the loops over dx and dy k is the same in every lane
// of the wave and the element is moved out through the index register.
typedef double lf_v16 __attribute__((ext_vector_type(16)));
struct LfW {
    lf_v16 lo, hi;
};
static_assert(LF_MAX_R < 32, "LfW holds 32 weights");
__device__ __forceinline__ double lf_w(const LfW &w, int k) { return k < 16 ? w.lo[k] : w.hi[k - 16]; }
__device__ __forceinline__ void lf_w_set(LfW &w, int k, double v) {
    if (k < 16) w.lo[k] = v;
    else w.hi[k - 16] = v;
}

// sum_dz w_|dz| row[dz] over |dz| <= R.  RW: the wave's largest R, a template parameter, so that the 2 RW + 1 reads of the row are
// issued together and no branch separates them; UNI: every lane of the wave that takes part in anything has R == RW.  Otherwise a
// lane keeps its sum as it was for k > R: what lies beyond its own R never enters it.
template <int RW, bool UNI> __device__ __forceinline__ double lf_row(const float *row, const LfW &w, int R) {
    double a = lf_w(w, 0) * (double)row[0];
#pragma unroll
    for (int k = 1; k <= RW; k++) {
        const double b = fma(lf_w(w, k), (double)row[-k] + (double)row[k], a);
        a = UNI || k <= R ? b : a;
    }
    return a;
}

// sx + sum_dx w_|dx| (sum_dy w_|dy| (row sums)) over the planes d_lo .. d_hi of the staged slab; p: the lane's voxel in plane d_lo.
// dx and dy are the same in every lane: all lanes read the same rows of LDS.
template <int RW, bool UNI>
__device__ __forceinline__ double lf_planes(const float *p, int plane, int pz, const LfW &w, int R, int d_lo, int d_hi, double sx) {
    for (int dx = d_lo; dx <= d_hi; dx++, p += plane) {
        const int ax = dx < 0 ? -dx : dx;
        double sy = 0.0;
#pragma unroll 1
        for (int dy = -RW; dy <= RW; dy++) {
            const int ay = dy < 0 ? -dy : dy;
            const double b = fma(lf_w(w, ay), lf_row<RW, UNI>(p + dy * pz, w, R), sy);
            sy = UNI || ay <= R ? b : sy;
        }
        const double b = fma(lf_w(w, ax), sy, sx);
        sx = ax <= R ? b : sx;
    }
    return sx;
}

__global__ __launch_bounds__(LF_THREADS) void k_lf_tile(const LfArgs A, unsigned first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lf_lds[];
    double *S = (double *)lf_lds;                        // [LF_PER_THREAD][LF_THREADS]: slot [i][t] is thread t's alone
    int *ctl = (int *)(lf_lds + LF_LDS_SUMS);
    float *img = (float *)(lf_lds + LF_LDS_HEAD);
    const unsigned tile = first + blockIdx.x, tz = tile % A.tz, tt = tile / A.tz, ty = tt % A.ty, tx = tt / A.ty;
    const int x0 = (int)tx * LF_TX, y0 = (int)ty * LF_TY, z0 = (int)tz * LF_TZ;
    const int t = (int)threadIdx.x, lz = t & (LF_TZ - 1), ly = (t / LF_TZ) % LF_TY, lx = t / (LF_TY * LF_TZ) * LF_PER_THREAD;
    const int y = y0 + ly, z = z0 + lz;
    const bool in_yz = y < A.n[1] && z < A.n[2];
    const size_t n12 = (size_t)A.n[1] * A.n[2], at = (size_t)y * A.n[2] + z;

    // 1. sigma of the thread's outputs, the tile's largest radius
    if (t == 0) ctl[0] = 0;
    __syncthreads();
    int r_mine = 0;
#pragma unroll
    for (int i = 0; i < LF_PER_THREAD; i++) {
        const int x = x0 + lx + i;
        S[i * LF_THREADS + t] = 0.0;
        if (in_yz && x < A.n[0]) {
            const double sg = lf_sigma(A, x, y, z);
            if (A.sigma) A.sigma[(size_t)x * n12 + at] = sg;
            r_mine = max(r_mine, lf_radius(sg));
        }
    }
    r_mine = lf_wave_max(r_mine);
    if (lane_id() == 0) atomicMax(&ctl[0], r_mine);
    __syncthreads();
    const int H = ctl[0];
    const LfSlab sl = lf_slab(H, A.lds);
    const int x_end = x0 + LF_TX + H;                    // one past the last plane the tile needs

    for (int s = 0; s < sl.n_slabs; s++) {
        const int xs = x0 - H + s * sl.planes, np = min(sl.planes, x_end - xs);
        const bool last = s == sl.n_slabs - 1;
        if (s) __syncthreads();                          // the slab before has been read
        // 2. planes xs .. xs + np - 1: a wavefront per row, the lanes along z
        for (int r = t / MAD_WAVE; r < np * sl.py; r += LF_THREADS / MAD_WAVE) {
            const int p = r / sl.py, gx = xs + p, gy = y0 - H + (r - p * sl.py);
            const bool ok = gx >= 0 && gx < A.n[0] && gy >= 0 && gy < A.n[1];
            const float *src = A.g + (ok ? (size_t)gx * n12 + (size_t)gy * A.n[2] : 0);
            for (int rz = (int)lane_id(); rz < sl.pz; rz += MAD_WAVE) {
                const int gz = z0 - H + rz;
                img[r * sl.pz + rz] = ok && gz >= 0 && gz < A.n[2] ? src[gz] : 0.f;
            }
        }
        __syncthreads();
        // 3. the thread's outputs, one after the other; x is the same in every lane of a wave
#pragma unroll 1
        for (int i = 0; i < LF_PER_THREAD; i++) {
            const int x = x0 + lx + i;
            const bool mine = in_yz && x < A.n[0];
            const double sg = mine ? lf_sigma(A, x, y, z) : 1.0;
            const int R = mine ? lf_radius(sg) : -1;     // -1: the lane takes part in nothing
            const int Rw = lf_wave_max(R);
            if (Rw < 0) continue;
            const int d_lo = max(-Rw, xs - x), d_hi = min(Rw, xs + np - 1 - x);
            if (d_lo > d_hi && !last) continue;
            LfW w;
            w.lo = 0.0;
            w.hi = 0.0;
            const double q = -0.5 / (sg * sg);
#pragma unroll
            for (int k = 0; k <= LF_MAX_R; k++)
                if (k <= Rw && k <= R) lf_w_set(w, k, exp(q * (double)(k * k)));
            double sx = S[i * LF_THREADS + t];
            const int plane = sl.py * sl.pz;
            const float *p = img + ((ly + H) * sl.pz + lz + H) + (x + d_lo - xs) * plane;
            const bool uni = __all(R < 0 || R == Rw) != 0;
#define LF_CASE(r) \
    case r: sx = uni ? lf_planes<r, true>(p, plane, sl.pz, w, R, d_lo, d_hi, sx) : lf_planes<r, false>(p, plane, sl.pz, w, R, d_lo, d_hi, sx); break;
            switch (Rw) {
                LF_CASE(1) LF_CASE(2) LF_CASE(3) LF_CASE(4) LF_CASE(5) LF_CASE(6) LF_CASE(7) LF_CASE(8) LF_CASE(9) LF_CASE(10) LF_CASE(11) LF_CASE(12)
                LF_CASE(13) LF_CASE(14) LF_CASE(15) LF_CASE(16) LF_CASE(17) LF_CASE(18) LF_CASE(19) LF_CASE(20) LF_CASE(21) LF_CASE(22) LF_CASE(23)
                LF_CASE(24)
            }
#undef LF_CASE
            static_assert(LF_MAX_R == 24, "the cases above");
            if (!last) {
                S[i * LF_THREADS + t] = sx;
            } else if (mine) {
                double sum = 0.0;                        // W = w_0 + 2 (w_R + ... + w_1), from R down to 1
#pragma unroll
                for (int k = LF_MAX_R; k >= 1; k--)
                    if (k <= R) sum += lf_w(w, k);
                const double W = lf_w(w, 0) + 2.0 * sum, v = sx / ((W * W) * W);
                A.out64[(size_t)x * n12 + at] = v;
                A.out[(size_t)x * n12 + at] = (float)v;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

extern "C" int mad_map_local_filter(mad_ctx *ctx, const float *grid, const int32_t dims[3], double voxsp, const double *res,
                                    const int32_t rdims[3], int32_t step, float *out, double *out64, double *sigma) {
    const char *who = "mad_map_local_filter";
    if (ctx) mad_use_lane(ctx, 0);
    if (!ctx || !grid || !dims || !res || !rdims || !out) return ctx ? mad_fail(ctx, MAD_EINVAL, "%s: NULL argument", who) : MAD_EINVAL;
    LfPlan P;
    char msg[320];
    const int bad = lf_plan(dims, voxsp, res, rdims, step, M_PI * sqrt(2.0), P, msg, sizeof(msg));
    if (bad != LF_OK) return mad_fail(ctx, bad == LF_EDOM ? MAD_EDOM : MAD_EINVAL, "%s", msg);      // nothing allocated or launched
    const size_t n = P.n_vox;
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_H), n * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_I), n * 4));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_A), n * 8));
    if (sigma) MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_B), n * 8));
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_TMP_G), P.n_res * 8));
    LfArgs A;
    memset(&A, 0, sizeof(A));
    A.g = scratch<float>(ctx, S_TMP_H);
    A.out = scratch<float>(ctx, S_TMP_I);
    A.out64 = scratch<double>(ctx, S_TMP_A);
    A.sigma = sigma ? scratch<double>(ctx, S_TMP_B) : nullptr;
    A.res = scratch<double>(ctx, S_TMP_G);
    for (int a = 0; a < 3; a++) { A.n[a] = P.n[a]; A.m[a] = P.m[a]; }
    A.step = P.step;
    A.inv = P.inv;
    A.ty = P.tiles[1];
    A.tz = P.tiles[2];
    A.lds = P.lds;
    // `grid` and `res` are pageable and read by asynchronous copies: the stream is waited for before this function returns
    const auto enqueue = [&]() -> int {
        MAD_HIP(hipMemcpyAsync((void *)A.g, grid, n * 4, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)A.res, res, P.n_res * 8, hipMemcpyHostToDevice, ctx->stream));
        // the attribute belongs to the device the call runs on, and setting it costs nothing
        MAD_HIP(hipFuncSetAttribute((const void *)k_lf_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds));
        mad_timer_begin(ctx, MAD_T_LOCALFILTER);
        for (unsigned long long f = 0; f < P.n_tiles; f += LF_ROUND)      // a grid may not have 2^32 threads
            hipLaunchKernelGGL(k_lf_tile, dim3((unsigned)std::min<unsigned long long>(LF_ROUND, P.n_tiles - f)), dim3(LF_THREADS), P.lds,
                               ctx->stream, A, (unsigned)f);
        mad_timer_end(ctx, MAD_T_LOCALFILTER);
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(out, A.out, n * 4, hipMemcpyDeviceToHost, ctx->stream));      // (out may be grid: it has been uploaded)
        if (out64) MAD_HIP(hipMemcpyAsync(out64, A.out64, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (sigma) MAD_HIP(hipMemcpyAsync(sigma, A.sigma, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));
        return MAD_OK;
    };
    const int rc = enqueue();
    if (rc != MAD_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}
