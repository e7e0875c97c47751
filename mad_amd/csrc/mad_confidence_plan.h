// mad_confidence_plan.h -- the host side of mad_map_sort, mad_map_kth and mad_map_confidence: the arithmetic of
// the radix sort (tiles, the digit table, the buffers), the argument checks, the validation of the noise boxes, the key transform
// and the search over the monotone q-values that the device shares.  Plain C++ without a HIP type, so that it also compiles into a
// stand-alone host program (check_confidence_plan.cpp) for a host sanitizer.
//
// The sort.  float32 voxels, descending, keys only, least significant digit first: CF_PASSES passes of CF_BITS bits.  8 bits x 4
// passes: a pass reads the keys twice (digit counts, scatter) and writes them once, 12 B per key, 48 B per key in all; 11 bits x 3
// passes would move 36 B, but its digit table has 2048 rows per tile and the per-wave counters of the scatter (CF_WAVES x 2048 x 4 B
// = 32 KB beside the 16 KB of keys) would leave three workgroups per CU where this leaves seven, and its table is 8 x the size.
// A workgroup of CF_THREADS lanes takes a tile of CF_TILE consecutive keys; wavefront w takes the keys [w CF_WAVE_KEYS, (w + 1)
// CF_WAVE_KEYS) of it in CF_ROUNDS rounds of 64, so that the order of the keys of a tile is (wavefront, round, lane) and a rank inside
// the tile is stable.  The table of a pass is digit-major, tab[digit][tile], one uint32 per entry: its exclusive prefix sum in linear
// order is, for (digit, tile), the keys with a smaller digit plus the keys with this digit in earlier tiles -- where the first key of
// this digit of this tile goes.  The sum of the table is N < 2^31.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#if defined(__HIPCC__)
#define CF_HD __host__ __device__
#else
#define CF_HD
#endif

#define CF_THREADS 256
#define CF_WAVES (CF_THREADS / 64)
#define CF_BITS 8
#define CF_RADIX (1 << CF_BITS)
#define CF_PASSES (32 / CF_BITS)
#define CF_ROUNDS 16                                  // keys of one lane of a tile
#define CF_WAVE_KEYS (64 * CF_ROUNDS)                 // keys of one wavefront of a tile
#define CF_TILE (CF_THREADS * CF_ROUNDS)              // 4096 keys: 16 KB of LDS in the scatter
#define CF_RUN 256                                    // a run of fourier.tree_sum, and the workgroup of the noise kernels
#define CF_QPER 8                                     // consecutive q-values of one lane of the running minimum
#define CF_QBLOCK (CF_THREADS * CF_QPER)              // ... and of one workgroup
#define CF_MAX_BOXES 4096
#define CF_MAX_LEVELS 256
#define CF_MAX_K (1 << 20)

static_assert(CF_PASSES * CF_BITS == 32, "whole digits");
static_assert(CF_RADIX == CF_THREADS, "a lane per digit where the scatter turns counts into offsets");
static_assert(CF_TILE * 4 + (CF_WAVES + 2) * CF_RADIX * 4 < 32 * 1024, "the scatter's LDS leaves room for five workgroups per CU and more");

// The key of a float's bits u: ascending uint32 order of the keys is DESCENDING order of the values.  -0.0 is +0.0 first, so that the
// key is a function of the value.  (The usual monotone image is u ^ 0x80000000 for u >= 0 and ~u below; this is its complement.)
CF_HD static inline uint32_t cf_key(uint32_t u) {
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? u : ~(u | 0x80000000u);
}
CF_HD static inline uint32_t cf_unkey(uint32_t k) { return (k & 0x80000000u) ? k : (~k & 0x7fffffffu); }
CF_HD static inline bool cf_bits_finite(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }
CF_HD static inline uint32_t cf_digit(uint32_t key, int pass) { return (key >> (pass * CF_BITS)) & (uint32_t)(CF_RADIX - 1); }

// q[0 .. n) ascends (a reverse running minimum read forwards): how many are <= alpha.  The device's level search and the host's.
CF_HD static inline int64_t cf_level_count(const double *q, int64_t n, double alpha) {
    int64_t lo = 0, hi = n;      // q[lo - 1] <= alpha < q[hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (q[mid] <= alpha) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// sorted[0 .. n): the bits of float32 values that descend (their keys ascend).  An index that holds the value of `key`, or -1.  The
// look-up of every voxel (its value is in the array: never -1 there); integer compares, so that a denormal is no special case.
CF_HD static inline int64_t cf_find_key(const uint32_t *sorted, int64_t n, uint32_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const uint32_t k = cf_key(sorted[mid]);
        if (k == key) return mid;
        if (k < key) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

struct CfPlan {
    uint32_t n = 0;               // keys
    uint32_t tiles = 0;           // workgroups of the count and scatter kernels
    uint32_t table = 0;           // entries of one pass's digit table (its scan writes one more)
    uint32_t q_blocks = 0;        // workgroups of the running minimum
    size_t key_bytes = 0;         // one buffer of keys; the sort holds the input and two of these
    size_t table_bytes = 0;       // table and scanned table: 2 x (table + 1) uint32, rounded up to 256 B each
};

enum { CF_OK = 0, CF_EINVAL = 1 };

// CF_OK, or what every entry refuses with a message in msg.  n: the voxels (keys).
static inline int cf_plan(const char *who, int64_t n, CfPlan &P, char *msg, size_t msg_len) {
    if (n < 1) { snprintf(msg, msg_len, "%s: %lld voxels", who, (long long)n); return CF_EINVAL; }
    if (n >= (1ll << 31)) {
        snprintf(msg, msg_len, "%s: %lld voxels: 2^31 voxels or more are not supported", who, (long long)n);
        return CF_EINVAL;
    }
    P.n = (uint32_t)n;
    P.tiles = (P.n + (uint32_t)CF_TILE - 1u) / (uint32_t)CF_TILE;      // <= 2^19
    P.table = P.tiles * (uint32_t)CF_RADIX;                            // <= 2^27
    P.q_blocks = (P.n + (uint32_t)CF_QBLOCK - 1u) / (uint32_t)CF_QBLOCK;
    P.key_bytes = (size_t)P.n * 4;
    P.table_bytes = (((size_t)P.table + 1) * 4 + 255) & ~(size_t)255;
    return CF_OK;
}

static inline int cf_plan_dims(const char *who, const int32_t dims[3], CfPlan &P, char *msg, size_t msg_len) {
    for (int a = 0; a < 3; a++)
        if (dims[a] < 1) { snprintf(msg, msg_len, "%s: grid of %d x %d x %d voxels", who, dims[0], dims[1], dims[2]); return CF_EINVAL; }
    const unsigned long long vxy = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (vxy >= (1ull << 31) || vxy * (unsigned long long)dims[2] >= (1ull << 31)) {
        snprintf(msg, msg_len, "%s: %d x %d x %d voxels: grids of 2^31 voxels or more are not supported", who, dims[0], dims[1], dims[2]);
        return CF_EINVAL;
    }
    return cf_plan(who, (long long)(vxy * (unsigned long long)dims[2]), P, msg, msg_len);
}

// where key number i of the array sits: (tile, wavefront, round, lane), and back
CF_HD static inline uint32_t cf_key_index(uint32_t tile, uint32_t wave, uint32_t round, uint32_t lane) {
    return tile * (uint32_t)CF_TILE + wave * (uint32_t)CF_WAVE_KEYS + round * 64u + lane;      // tile < 2^19: below 2^31 + CF_TILE
}
// the entry of (digit, tile) in a pass's table
CF_HD static inline uint32_t cf_table_index(uint32_t digit, uint32_t tile, uint32_t tiles) { return digit * tiles + tile; }

// mad_map_kth: ranks 1 .. n
static inline int cf_kth_args(const char *who, int64_t n, int64_t n_k, const int64_t *k, char *msg, size_t msg_len) {
    if (n_k < 1 || n_k > CF_MAX_K) { snprintf(msg, msg_len, "%s: %lld ranks (1 .. %d)", who, (long long)n_k, CF_MAX_K); return CF_EINVAL; }
    for (int64_t i = 0; i < n_k; i++)
        if (k[i] < 1 || k[i] > n) {
            snprintf(msg, msg_len, "%s: rank %lld of %lld voxels (1 is the largest, %lld the smallest)", who, (long long)k[i], (long long)n, (long long)n);
            return CF_EINVAL;
        }
    return CF_OK;
}

// The noise boxes: boxes[b] = {x, y, z of the corner, edge}, a cube inside the grid.  first[b] = samples before box b (first has
// n_boxes + 1 entries), *n_samples their number: 2 or more and below 2^31.
static inline int cf_boxes(const char *who, const int32_t dims[3], int32_t n_boxes, const int32_t *boxes, int64_t *first, int64_t *n_samples,
                           char *msg, size_t msg_len) {
    if (n_boxes < 1 || n_boxes > CF_MAX_BOXES) { snprintf(msg, msg_len, "%s: %d noise boxes (1 .. %d)", who, n_boxes, CF_MAX_BOXES); return CF_EINVAL; }
    int64_t n = 0;
    for (int32_t b = 0; b < n_boxes; b++) {
        const int32_t *c = boxes + 4 * (size_t)b, e = c[3];
        if (e < 1) { snprintf(msg, msg_len, "%s: noise box %d has edge %d", who, b, e); return CF_EINVAL; }
        for (int a = 0; a < 3; a++)
            if (c[a] < 0 || c[a] > dims[a] - e) {      // (e >= 1: no overflow; dims[a] - e < 0 refuses every corner)
                snprintf(msg, msg_len, "%s: noise box %d (corner %d %d %d, edge %d) is not inside the grid of %d x %d x %d voxels", who, b, c[0], c[1],
                         c[2], e, dims[0], dims[1], dims[2]);
                return CF_EINVAL;
            }
        first[b] = n;
        n += (int64_t)e * e * e;      // each below 2^31 (inside the grid), at most 4096 of them
        if (n >= (1ll << 31)) { snprintf(msg, msg_len, "%s: 2^31 noise samples or more are not supported", who); return CF_EINVAL; }
    }
    first[n_boxes] = n;
    if (n < 2) { snprintf(msg, msg_len, "%s: %lld noise sample: a variance needs 2 or more", who, (long long)n); return CF_EINVAL; }
    *n_samples = n;
    return CF_OK;
}

// sample number i (box by box, each in the order of the file) -> the linear index of its voxel
CF_HD static inline uint32_t cf_sample_voxel(int64_t i, int32_t n_boxes, const int32_t *boxes, const int64_t *first, int32_t ny, int32_t nz) {
    int32_t lo = 0, hi = n_boxes - 1;      // the last box with first[b] <= i
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) / 2;
        if (first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const int32_t *c = boxes + 4 * lo;
    const uint32_t e = (uint32_t)c[3], r = (uint32_t)(i - first[lo]);
    const uint32_t xy = r / e, z = r - xy * e, x = xy / e, y = xy - x * e;
    return (((uint32_t)c[0] + x) * (uint32_t)ny + ((uint32_t)c[1] + y)) * (uint32_t)nz + ((uint32_t)c[2] + z);
}

static inline int cf_levels(const char *who, double c, int32_t n_levels, const double *levels, char *msg, size_t msg_len) {
    if (!(c >= 1.0) || !std::isfinite(c)) { snprintf(msg, msg_len, "%s: c = %g (1 for Benjamini-Hochberg, the harmonic number of the voxels for Benjamini-Yekutieli)", who, c); return CF_EINVAL; }
    if (n_levels < 0 || n_levels > CF_MAX_LEVELS) { snprintf(msg, msg_len, "%s: %d levels (0 .. %d)", who, n_levels, CF_MAX_LEVELS); return CF_EINVAL; }
    for (int32_t l = 0; l < n_levels; l++)
        if (!(levels[l] >= 0.0 && levels[l] <= 1.0)) { snprintf(msg, msg_len, "%s: level %g (a false discovery rate, 0 .. 1)", who, levels[l]); return CF_EINVAL; }
    return CF_OK;
}
