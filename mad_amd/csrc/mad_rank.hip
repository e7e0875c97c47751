// Assembly ranking (MaD._build_from_single, reference MaD.py:684-694, and MaD._build_models, MaD.py:797-807): the head of the
// sorted list of all n_copies-subsets of one subunit's solutions, and of all picks of one sub-complex per subunit, found by
// ordered enumeration with prefix pruning on the device.
//
//   k_rank<false>  the c-subsets of n solutions in lexicographic order (itertools.combinations).  Key: the MAXIMUM of the
//                  subset's pairwise overlaps, as the dense order-preserving integer rank of the table's distinct values -- a
//                  maximum is exact, so (max, rank of the subset) is the reference's stable sort, bit for bit.
//   k_rank<true>   the product of g contiguous groups, last group fastest (itertools.product).  Key: the float64 sum of the
//                  pick's full k x k block, added in one fixed order (the table is folded to a packed triangle
//                  S(a, b) = overlap[a, b] + overlap[b, a], S(a, a) = overlap[a, a] on the host); its bits order like the value
//                  because every term is >= +0.
//   k_rank_final   one workgroup: merges the workgroups' lists (TOP) or sorts the collected entries (BELOW).
//
// The rank space of a launch is cut into contiguous runs, one per thread.  A thread unranks its first item and then walks
// successors; the key is kept per prefix position in LDS (acc[level][thread]), so a step of the last position re-reads only that
// position's pairs, and a prefix whose key already lies beyond the bound jumps over every item that shares it (the count comes
// from the same binomial / block-size table that unranks).  Keys only grow along a prefix: a maximum over more pairs, a sum of
// more non-negative terms (rounded additions of non-negative numbers are monotonic).
// No floating-point atomics; the only atomics are integer minima of the bound and integer counters.  Two calls give the same bits:
// the answer is fixed by the total order (key, rank), whatever order the workgroups run in.
#include "mad_common.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#define MAD_RANK_M 1024                 // a workgroup's candidate buffer (TOP): 2 x MAD_RANK_MAX_TOP
#define MAD_RANK_STEPS 128              // items or jumps of a thread between two barriers of its workgroup
#define MAD_RANK_SAT ((1ll << 47) - 1)  // the subset's rank inside the packed 64-bit bound of k_rank<false>, saturating
#define MAD_RANK_LAUNCH_ITEMS (1ll << 26)      // rank range of one launch: 6.4 ms at the slowest unpruned rate measured, 1.05e10 subsets / s at c = 16
#define MAD_RANK_BUDGET (1ll << 34)            // evaluated items of one call, by default: 0.4 - 1.6 s at the unpruned rates
#define MAD_RANK_MAX_LAUNCHES 16384
#define MAD_RANK_U 1.1102230246251565e-16
static_assert(MAD_RANK_M == 2 * MAD_RANK_MAX_TOP && MAD_RANK_MAX_N <= 256 && MAD_RANK_MAX_K == 16, "k_rank's LDS image");

enum { CTL_BOUND = 0, CTL_ZRANK, CTL_EVAL, CTL_SKIP, CTL_COUNT, CTL_NOUT, CTL_WORDS = 8 };

struct RankArgs {
    const unsigned long long *tab;      // <false>: uint16 [n][n] dense ranks; <true>: float64 packed triangle S(a, b) at b (b + 1) / 2 + a, a <= b
    const long long *aux;               // <false>: C(m, k) at 16 m + k, m < n, k < 16; <true>: [0..15] block sizes, [16..32] group_first
    unsigned long long *ctl;            // CTL_*
    unsigned long long *lists;          // TOP: per workgroup [cap][2] = (key, rank), sorted
    int *list_n;                        // TOP: entries of each workgroup's list
    unsigned long long *out;            // [MAD_RANK_MAX_OUT][2]
    int tab_words, aux_words;           // 8-byte words to stage
    int n, k;                           // k = n_copies or the number of groups
    int mode, prune, cap;
    unsigned long long thr;             // BELOW: the largest key kept
    long long lo, hi, run;              // the launch's rank range, and ranks per thread
};

template <bool MODELS> struct RankLds;
template <> struct RankLds<false> {
    static constexpr int T = 256;
    typedef unsigned short acc_t;
    unsigned long long bufp[MAD_RANK_M];
    long long bufr[MAD_RANK_M];
    long long aux[MAD_RANK_MAX_N * MAD_RANK_MAX_K];
    unsigned long long lp;
    long long lr;
    unsigned short tab[MAD_RANK_MAX_N * MAD_RANK_MAX_N];
    unsigned short acc[MAD_RANK_MAX_K][T];
    unsigned char pos[MAD_RANK_MAX_K][T];
    int cnt;
};
template <> struct RankLds<true> {
    static constexpr int T = 128;
    typedef double acc_t;
    unsigned long long bufp[MAD_RANK_M];
    long long bufr[MAD_RANK_M];
    long long aux[48];
    unsigned long long lp;
    long long lr;
    double tab[MAD_RANK_MAX_N * (MAD_RANK_MAX_N + 1) / 2];
    double acc[MAD_RANK_MAX_K][T];
    unsigned char pos[MAD_RANK_MAX_K][T];
    int cnt;
};
// two workgroups per CU (160 KiB of LDS): DESIGN.md section 4f has the sums
static_assert(sizeof(RankLds<false>) <= 80 * 1024 && sizeof(RankLds<true>) <= 80 * 1024, "k_rank: two workgroups per CU");

__device__ __forceinline__ bool rank_after(unsigned long long p, long long r, unsigned long long bp, long long br) {
    return p > bp || (p == bp && r > br);
}

// bitonic sort of N (a power of two) entries in LDS, ascending by (key, rank); every thread of the workgroup calls it
template <int T> __device__ void rank_sort(unsigned long long *p, long long *r, int N) {
    for (int k2 = 2; k2 <= N; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = threadIdx.x; i < N; i += T) {
                const int l = i ^ j2;
                if (l > i) {
                    const unsigned long long pa = p[i], pb = p[l];
                    const long long ra = r[i], rb = r[l];
                    if (rank_after(pa, ra, pb, rb) == ((i & k2) == 0)) p[i] = pb, r[i] = rb, p[l] = pa, r[l] = ra;
                }
            }
            __syncthreads();
        }
}

// the global bound: an upper bound of the cap-th smallest (key, rank) of the whole call
template <bool MODELS> __device__ __forceinline__ void rank_bound_load(const unsigned long long *ctl, unsigned long long &bp, long long &br) {
    const unsigned long long w = __hip_atomic_load(ctl + CTL_BOUND, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (MODELS) {
        // a sum has no room for the rank beside it.  CTL_ZRANK serves the common class, sums of exactly 0: "cap picks of sum 0 have
        // ranks <= Z".  Both words only fall, and either alone is a valid bound.
        const unsigned long long z = __hip_atomic_load(ctl + CTL_ZRANK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (z != (unsigned long long)LLONG_MAX) bp = 0, br = (long long)z;
        else bp = w, br = LLONG_MAX;
    } else if (w == ~0ull) bp = w, br = LLONG_MAX;
    else {
        bp = w >> 47;
        br = (long long)(w & (unsigned long long)MAD_RANK_SAT);
        if (br == MAD_RANK_SAT) br = LLONG_MAX;      // saturated: the key alone bounds
    }
}
template <bool MODELS> __device__ __forceinline__ void rank_bound_publish(unsigned long long *ctl, unsigned long long p, long long r) {
    if (MODELS) {
        if (p == 0) atomicMin(ctl + CTL_ZRANK, (unsigned long long)r);
        else atomicMin(ctl + CTL_BOUND, p);
    } else
        atomicMin(ctl + CTL_BOUND, (p << 47) | (unsigned long long)(r < MAD_RANK_SAT ? r : MAD_RANK_SAT));
}

// sorts the first min(cnt, M) entries of the buffer, keeps the best cap, and tightens the bounds with the cap-th
template <bool MODELS> __device__ void rank_compact(RankLds<MODELS> &L, int cap, unsigned long long *ctl) {
    constexpr int T = RankLds<MODELS>::T;
    const int m = min(L.cnt, MAD_RANK_M);
    __syncthreads();
    int N = 2;      // the power of two that holds what is filled (at most MAD_RANK_M): a small cap compacts often, on few entries
    while (N < m) N <<= 1;
    for (int i = m + threadIdx.x; i < N; i += T) L.bufp[i] = ~0ull, L.bufr[i] = LLONG_MAX;
    __syncthreads();
    rank_sort<T>(L.bufp, L.bufr, N);
    if (threadIdx.x == 0) {
        L.cnt = min(m, cap);
        if (m >= cap && cap > 0) {
            L.lp = L.bufp[cap - 1], L.lr = L.bufr[cap - 1];
            rank_bound_publish<MODELS>(ctl, L.lp, L.lr);
        }
    }
    __syncthreads();
}

template <bool MODELS> __global__ __launch_bounds__(RankLds<MODELS>::T) void k_rank(const RankArgs A) {
    constexpr int T = RankLds<MODELS>::T;
    typedef typename RankLds<MODELS>::acc_t acc_t;
    __shared__ RankLds<MODELS> L;
    const int tid = threadIdx.x, n = A.n, K = A.k, cap = A.cap;
    const bool top = A.mode == MAD_RANK_TOP;
    for (int i = tid; i < A.tab_words; i += T) ((unsigned long long *)L.tab)[i] = A.tab[i];
    for (int i = tid; i < A.aux_words; i += T) L.aux[i] = A.aux[i];
    if (tid == 0) L.cnt = 0, L.lp = ~0ull, L.lr = LLONG_MAX;
    __syncthreads();
    if (top) {      // the list this workgroup left behind in the call's earlier launches
        const int m = min(A.list_n[blockIdx.x], cap);
        const unsigned long long *src = A.lists + (size_t)blockIdx.x * cap * 2;
        for (int i = tid; i < m; i += T) L.bufp[i] = src[2 * i], L.bufr[i] = (long long)src[2 * i + 1];
        if (tid == 0) {
            L.cnt = m;
            if (m >= cap && cap > 0) L.lp = src[2 * (cap - 1)], L.lr = (long long)src[2 * (cap - 1) + 1];
        }
        __syncthreads();
    }
    const long long *first = L.aux + 16;      // <true> only
    long long rank = A.lo + ((long long)blockIdx.x * T + tid) * A.run;
    if (rank > A.hi) rank = A.hi;
    const long long run_end = rank + A.run < A.hi ? rank + A.run : A.hi;
    bool active = rank < run_end;
    if (active) {      // unrank
        long long r = rank;
        if (MODELS) {
            for (int l = 0; l < K; l++) {
                const long long w = L.aux[l], d = r / w;
                r -= d * w;
                L.pos[l][tid] = (unsigned char)(first[l] + d);
            }
        } else {
            int v = 0;
            for (int l = 0; l < K; l++, v++) {
                for (; v < n - K + l; v++) {
                    const long long c = L.aux[(n - 1 - v) * 16 + (K - 1 - l)];
                    if (r < c) break;
                    r -= c;
                }
                L.pos[l][tid] = (unsigned char)v;
            }
        }
    }
    // position `lvl` moves on (with carry), everything behind it falls to its lowest value; returns the first position that changed
    const auto advance = [&](int lvl) -> int {
        int q = lvl;
        for (; q >= 0; q--) {
            const int v = L.pos[q][tid] + 1;
            if (MODELS ? v < (int)first[q + 1] : v <= n - K + q) {
                L.pos[q][tid] = (unsigned char)v;
                break;
            }
        }
        if (q < 0) return -1;
        for (int l = q + 1; l < K; l++) L.pos[l][tid] = (unsigned char)(MODELS ? (int)first[l] : L.pos[l - 1][tid] + 1);
        return q;
    };
    // items from the current one to the last that shares positions 0 .. lvl with it
    const auto left_in_block = [&](int lvl) -> long long {
        long long size, off = 0;
        if (MODELS) {
            size = lvl + 1 < K ? L.aux[lvl] : 1;
            for (int l = lvl + 1; l < K; l++) off += (long long)(L.pos[l][tid] - (int)first[l]) * L.aux[l];
        } else {
            size = L.aux[(n - 1 - L.pos[lvl][tid]) * 16 + (K - 1 - lvl)];
            for (int l = lvl + 1; l < K; l++)
                for (int v = L.pos[l - 1][tid] + 1; v < L.pos[l][tid]; v++) off += L.aux[(n - 1 - v) * 16 + (K - 1 - l)];
        }
        return size - off;
    };
    int j = 0;      // positions j .. K - 1 have no key yet
    unsigned long long n_eval = 0, n_skip = 0;
    for (;;) {
        unsigned long long bp = A.thr;
        long long br = LLONG_MAX;
        if (top) {
            rank_bound_load<MODELS>(A.ctl, bp, br);
            const unsigned long long lp = L.lp;
            const long long lr = L.lr;
            if (rank_after(bp, br, lp, lr)) bp = lp, br = lr;
        }
        for (int steps = 0; active && steps < MAD_RANK_STEPS; steps++) {
            bool jumped = false;
            for (int lvl = j; lvl < K; lvl++) {
                const int b = L.pos[lvl][tid];
                acc_t a;
                if (MODELS) {
                    const double *col = (const double *)L.tab + b * (b + 1) / 2;
                    double t = col[b];
                    for (int i = 0; i < lvl; i++) t += col[L.pos[i][tid]];
                    a = (acc_t)(lvl ? (double)L.acc[lvl - 1][tid] + t : t);
                } else {
                    const unsigned short *row = (const unsigned short *)L.tab + b * n;
                    unsigned m = lvl ? (unsigned)L.acc[lvl - 1][tid] : 0u;
                    for (int i = 0; i < lvl; i++) m = max(m, (unsigned)row[L.pos[i][tid]]);
                    a = (acc_t)m;
                }
                L.acc[lvl][tid] = a;
                if (A.prune && lvl < K - 1) {
                    const unsigned long long p = MODELS ? (unsigned long long)__double_as_longlong((double)a) : (unsigned long long)a;
                    if (rank_after(p, rank, bp, br)) {      // every item of this prefix has a key >= p and a rank >= this one
                        long long e = rank + left_in_block(lvl);
                        if (e > run_end) e = run_end;
                        n_skip += (unsigned long long)(e - rank);
                        rank = e;
                        j = rank < run_end ? advance(lvl) : 0;
                        if (j < 0) rank = run_end;
                        jumped = true;
                        break;
                    }
                }
            }
            if (!jumped) {
                const acc_t a = L.acc[K - 1][tid];
                const unsigned long long p = MODELS ? (unsigned long long)__double_as_longlong((double)a) : (unsigned long long)a;
                j = K;
                if (!rank_after(p, rank, bp, br)) {
                    if (top) {
                        const int slot = atomicAdd(&L.cnt, 1);
                        if (slot >= MAD_RANK_M) break;      // full: the item is taken again after the workgroup has compacted
                        L.bufp[slot] = p, L.bufr[slot] = rank;
                    } else {
                        const unsigned long long slot = atomicAdd(A.ctl + CTL_COUNT, 1ull);
                        if (slot < (unsigned long long)cap) A.out[2 * slot] = p, A.out[2 * slot + 1] = (unsigned long long)rank;
                    }
                }
                n_eval++;
                rank++;
                if (rank < run_end) {
                    j = advance(K - 1);
                    if (j < 0) rank = run_end;
                }
            }
            active = rank < run_end;
        }
        const int any = __syncthreads_or(active);
        const int filled = L.cnt;
        __syncthreads();      // (the next round's appends must not reach a thread that has yet to read the count)
        if (top && filled > cap) rank_compact<MODELS>(L, cap, A.ctl);
        if (!any) break;
    }
    if (top) {
        rank_compact<MODELS>(L, cap, A.ctl);
        const int m = L.cnt;
        unsigned long long *dst = A.lists + (size_t)blockIdx.x * cap * 2;
        for (int i = tid; i < m; i += T) dst[2 * i] = L.bufp[i], dst[2 * i + 1] = (unsigned long long)L.bufr[i];
        if (tid == 0) A.list_n[blockIdx.x] = m;
    }
    for (int o = 32; o > 0; o >>= 1) n_eval += __shfl_xor(n_eval, o, 64), n_skip += __shfl_xor(n_skip, o, 64);
    if ((tid & 63) == 0) {
        if (n_eval) atomicAdd(A.ctl + CTL_EVAL, n_eval);
        if (n_skip) atomicAdd(A.ctl + CTL_SKIP, n_skip);
    }
}

template <bool MODELS> __global__ __launch_bounds__(256) void k_rank_final(const RankArgs A, int n_lists) {
    __shared__ unsigned long long P[MAD_RANK_MAX_OUT];
    __shared__ long long R[MAD_RANK_MAX_OUT];
    __shared__ int cnt;
    const int tid = threadIdx.x, cap = A.cap;
    int m;
    if (A.mode == MAD_RANK_TOP) {
        unsigned long long bp;
        long long br;
        rank_bound_load<MODELS>(A.ctl, bp, br);
        if (tid == 0) cnt = 0;
        __syncthreads();
        for (int w = 0; w < n_lists; w++) {
            const int lm = min(A.list_n[w], cap);
            const unsigned long long *src = A.lists + (size_t)w * cap * 2;
            for (int i = tid; i < lm; i += 256) {
                const unsigned long long p = src[2 * i];
                const long long r = (long long)src[2 * i + 1];
                if (!rank_after(p, r, bp, br)) {
                    const int slot = atomicAdd(&cnt, 1);      // (room for a whole list is kept free below)
                    P[slot] = p, R[slot] = r;
                }
            }
            __syncthreads();
            m = cnt;
            __syncthreads();
            if (m > MAD_RANK_MAX_OUT - MAD_RANK_MAX_TOP) {
                for (int i = m + tid; i < MAD_RANK_MAX_OUT; i += 256) P[i] = ~0ull, R[i] = LLONG_MAX;
                __syncthreads();
                rank_sort<256>(P, R, MAD_RANK_MAX_OUT);
                if (rank_after(bp, br, P[cap - 1], R[cap - 1])) bp = P[cap - 1], br = R[cap - 1];
                __syncthreads();
                if (tid == 0) cnt = cap;
                __syncthreads();
            }
        }
        m = cnt;
    } else {
        const unsigned long long c = A.ctl[CTL_COUNT];
        m = (int)(c < (unsigned long long)cap ? c : (unsigned long long)cap);
        for (int i = tid; i < m; i += 256) P[i] = A.out[2 * i], R[i] = (long long)A.out[2 * i + 1];
    }
    int N = 2;
    while (N < m) N <<= 1;
    for (int i = m + tid; i < N; i += 256) P[i] = ~0ull, R[i] = LLONG_MAX;
    __syncthreads();
    rank_sort<256>(P, R, N);
    m = min(m, cap);
    for (int i = tid; i < m; i += 256) A.out[2 * i] = P[i], A.out[2 * i + 1] = (unsigned long long)R[i];
    if (tid == 0) A.ctl[CTL_NOUT] = (unsigned long long)m;
}

// ------------------------------------------------------------------------------------------------------------------ host
static inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

struct RankJob {
    bool models;
    int n, k;
    std::vector<unsigned long long> tab, aux;      // the device images, in 8-byte words
    long long space;
    long long launch_items, budget;
    bool prune;
};
struct RankPass {
    std::vector<unsigned long long> key;
    std::vector<long long> rank;
    long long total = 0;       // BELOW: entries within the threshold; TOP: entries returned
    bool exhausted = false;    // the budget ran out
};

// One pass over the whole rank space: launches over rank ranges, the bound and the workgroups' lists carried in device memory.
static int rank_pass(mad_ctx *ctx, const RankJob &J, int mode, int cap, unsigned long long thr, RankPass &out) {
    const int T = J.models ? RankLds<true>::T : RankLds<false>::T;
    const int max_grid = 2 * ctx->n_cu;
    const size_t b_ctl = 64, b_tab = up16(J.tab.size() * 8), b_aux = up16(J.aux.size() * 8), b_ln = up16((size_t)max_grid * 4);
    const size_t b_lists = mode == MAD_RANK_TOP ? up16((size_t)max_grid * cap * 16) : 0, b_out = (size_t)MAD_RANK_MAX_OUT * 16;
    mad_use_lane(ctx, 0);
    MAD_TRY(mad_reserve(ctx, mad_sb(ctx, S_RANK), b_ctl + b_tab + b_aux + b_ln + b_lists + b_out + 16));
    char *base = scratch<char>(ctx, S_RANK);
    RankArgs A;
    std::memset(&A, 0, sizeof A);
    A.ctl = (unsigned long long *)base;
    A.tab = (const unsigned long long *)(base + b_ctl);
    A.aux = (const long long *)(base + b_ctl + b_tab);
    A.list_n = (int *)(base + b_ctl + b_tab + b_aux);
    A.lists = (unsigned long long *)(base + b_ctl + b_tab + b_aux + b_ln);
    A.out = (unsigned long long *)(base + b_ctl + b_tab + b_aux + b_ln + b_lists);
    A.tab_words = (int)J.tab.size(), A.aux_words = (int)J.aux.size();
    A.n = J.n, A.k = J.k, A.mode = mode, A.prune = J.prune ? 1 : 0, A.cap = cap, A.thr = thr;
    unsigned long long ctl[CTL_WORDS] = {~0ull, (unsigned long long)LLONG_MAX, 0, 0, 0, 0, 0, 0};
    const auto run = [&]() -> int {
        MAD_HIP(hipMemcpyAsync(base, ctl, sizeof ctl, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)A.tab, J.tab.data(), J.tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemcpyAsync((void *)A.aux, J.aux.data(), J.aux.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        MAD_HIP(hipMemsetAsync(A.list_n, 0, b_ln, ctx->stream));
        int n_lists = 0;
        for (long long lo = 0; lo < J.space; lo += J.launch_items) {
            if (ctx->last_rank_launches >= MAD_RANK_MAX_LAUNCHES) {
                out.exhausted = true;
                break;
            }
            A.lo = lo;
            A.hi = J.space - lo > J.launch_items ? lo + J.launch_items : J.space;
            const long long items = A.hi - A.lo;
            const int grid = (int)std::max<long long>(1, std::min<long long>(max_grid, mad_ceil_div(items, (long long)T * 64)));
            A.run = mad_ceil_div(items, (long long)grid * T);
            n_lists = std::max(n_lists, grid);
            if (J.models) hipLaunchKernelGGL(k_rank<true>, dim3(grid), dim3(T), 0, ctx->stream, A);
            else hipLaunchKernelGGL(k_rank<false>, dim3(grid), dim3(T), 0, ctx->stream, A);
            MAD_HIP(hipGetLastError());
            MAD_HIP(hipMemcpyAsync(ctl, base, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
            MAD_HIP(hipStreamSynchronize(ctx->stream));
            ctx->last_rank_launches++;
            if (A.hi < J.space && (long long)ctl[CTL_EVAL] + ctx->last_rank_evaluated > J.budget) {      // (a pass that is complete is kept)
                out.exhausted = true;
                break;
            }
        }
        ctx->last_rank_evaluated += (long long)ctl[CTL_EVAL];
        ctx->last_rank_skipped += (long long)ctl[CTL_SKIP];
        if (out.exhausted) return MAD_OK;
        if (J.models) hipLaunchKernelGGL(k_rank_final<true>, dim3(1), dim3(256), 0, ctx->stream, A, n_lists);
        else hipLaunchKernelGGL(k_rank_final<false>, dim3(1), dim3(256), 0, ctx->stream, A, n_lists);
        MAD_HIP(hipGetLastError());
        MAD_HIP(hipMemcpyAsync(ctl, base, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
        MAD_HIP(hipStreamSynchronize(ctx->stream));
        const size_t m = (size_t)ctl[CTL_NOUT];
        std::vector<unsigned long long> h(2 * m + 2);
        if (m) MAD_HIP(hipMemcpy(h.data(), A.out, m * 16, hipMemcpyDeviceToHost));
        out.key.resize(m), out.rank.resize(m);
        for (size_t i = 0; i < m; i++) out.key[i] = h[2 * i], out.rank[i] = (long long)h[2 * i + 1];
        out.total = mode == MAD_RANK_TOP ? (long long)m : (long long)ctl[CTL_COUNT];
        return MAD_OK;
    };
    const int rc = run();
    if (rc != MAD_OK) (void)hipStreamSynchronize(ctx->stream);      // the copies read and write this frame
    return rc;
}

static void rank_plan_reset(mad_ctx *ctx) {
    ctx->last_rank_launches = ctx->last_rank_evaluated = ctx->last_rank_skipped = 0;
    ctx->last_rank_band_extra = 0;
}

static bool rank_table_ok(const double *t, int n) {
    for (size_t i = 0; i < (size_t)n * n; i++)
        if (!(t[i] >= 0.0) || !(t[i] <= DBL_MAX)) return false;
    return true;
}

static bool rank_no_prune() {
    const char *e = std::getenv("MAD_RANK_NO_PRUNE");
    return e && e[0] == '1' && e[1] == 0;
}

// C(m, k) for m <= n, k <= 16, saturating
static long long binom_sat(int m, int k) {
    if (k < 0 || k > m) return 0;
    unsigned __int128 c = 1;
    for (int i = 1; i <= k; i++) {
        c = c * (unsigned)(m - k + i) / (unsigned)i;
        if (c > (unsigned __int128)LLONG_MAX) return LLONG_MAX;
    }
    return (long long)c;
}

extern "C" int mad_rank_copies(mad_ctx *ctx, const double *overlap, int n, int n_copies, int mode, double max_overlap, int64_t cap,
                               int64_t launch_items, int64_t budget, int32_t *idx_out, double *key_out, int64_t *rank_out,
                               int64_t *n_out, int64_t *n_total, int32_t *status) {
    if (!ctx) return MAD_EINVAL;
    if (!overlap || !n_out || !n_total || !status || n < 0 || cap < 0 || (cap && (!idx_out || !key_out || !rank_out)))
        return mad_fail(ctx, MAD_EINVAL, "mad_rank_copies: null pointer, n = %d or cap = %lld", n, (long long)cap);
    if (mode != MAD_RANK_TOP && mode != MAD_RANK_BELOW) return mad_fail(ctx, MAD_EINVAL, "mad_rank_copies: mode = %d", mode);
    *n_out = *n_total = 0;
    *status = 0;
    rank_plan_reset(ctx);
    const int c = n_copies;
    if (n > MAD_RANK_MAX_N || c > MAD_RANK_MAX_K || c < 2 || c > n)
        return mad_fail(ctx, MAD_EDOM, "mad_rank_copies: n = %d (at most %d), n_copies = %d (2 .. min(n, %d))", n, MAD_RANK_MAX_N, c, MAD_RANK_MAX_K);
    if (!rank_table_ok(overlap, n)) return mad_fail(ctx, MAD_EDOM, "mad_rank_copies: an overlap is negative or not finite");
    if (mode == MAD_RANK_BELOW && std::isnan(max_overlap)) return mad_fail(ctx, MAD_EDOM, "mad_rank_copies: max_overlap is NaN");
    RankJob J;
    J.models = false, J.n = n, J.k = c;
    J.space = binom_sat(n, c);
    if (J.space == LLONG_MAX) return mad_fail(ctx, MAD_EDOM, "mad_rank_copies: C(%d, %d) does not fit an int64", n, c);
    J.launch_items = launch_items > 0 ? launch_items : MAD_RANK_LAUNCH_ITEMS;
    J.budget = budget > 0 ? budget : MAD_RANK_BUDGET;
    J.prune = !rank_no_prune();
    // dense order-preserving ranks of the distinct pair values (the reference reads overlap[a, b], a < b, only)
    std::vector<double> vals;
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++) vals.push_back(overlap[(size_t)a * n + b] + 0.0);
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    J.tab.assign(((size_t)n * n * 2 + 7) / 8, 0);
    unsigned short *tab = (unsigned short *)J.tab.data();
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++) {
            const unsigned short r = (unsigned short)(std::lower_bound(vals.begin(), vals.end(), overlap[(size_t)a * n + b] + 0.0) - vals.begin());
            tab[(size_t)a * n + b] = tab[(size_t)b * n + a] = r;
        }
    J.aux.assign((size_t)n * 16, 0);
    for (int m = 0; m < n; m++)
        for (int k = 0; k < 16; k++) J.aux[(size_t)m * 16 + k] = (unsigned long long)binom_sat(m, k);
    int dev_cap;
    unsigned long long thr = ~0ull;
    if (mode == MAD_RANK_TOP) {
        const long long want = std::min<long long>(cap, J.space);
        if (want > MAD_RANK_MAX_TOP) return mad_fail(ctx, MAD_EDOM, "mad_rank_copies: the first %lld entries asked for, at most %d", want, MAD_RANK_MAX_TOP);
        dev_cap = (int)want;
        if (dev_cap == 0) return MAD_OK;
    } else {
        const long long below = std::upper_bound(vals.begin(), vals.end(), max_overlap) - vals.begin();
        if (below == 0) return MAD_OK;      // every subset holds a pair above the threshold
        thr = (unsigned long long)(below - 1);
        dev_cap = (int)std::min<long long>(cap, MAD_RANK_MAX_OUT);
    }
    RankPass P;
    MAD_TRY(rank_pass(ctx, J, mode, dev_cap, thr, P));
    if (P.exhausted) {
        *status = 1;
        return MAD_OK;
    }
    *n_total = P.total;
    if (mode == MAD_RANK_BELOW && P.total > dev_cap) return mad_fail(ctx, MAD_ENOSPC, "mad_rank_copies: %lld subsets within the threshold, room for %d", (long long)P.total, dev_cap);
    for (size_t e = 0; e < P.key.size(); e++) {
        long long r = P.rank[e];
        int v = 0;
        for (int l = 0; l < c; l++, v++) {
            for (; v < n - c + l; v++) {
                const long long cnt = binom_sat(n - 1 - v, c - 1 - l);
                if (r < cnt) break;
                r -= cnt;
            }
            idx_out[e * c + l] = v;
        }
        key_out[e] = vals[(size_t)P.key[e]];
        rank_out[e] = P.rank[e];
    }
    *n_out = (int64_t)P.key.size();
    return MAD_OK;
}

// what a device sum may differ by from numpy's sum of the same k x k block, both ways, as a factor on the cap-th device sum
static double rank_band_factor(int k) { return 1.0 + 8.0 * (double)k * (double)k * MAD_RANK_U; }

extern "C" int mad_rank_models(mad_ctx *ctx, const double *overlap, int n, const int32_t *group_first, int n_groups, int64_t cap,
                               int64_t out_cap, int64_t launch_items, int64_t budget, int32_t *idx_out, double *key_out,
                               int64_t *rank_out, int64_t *n_out, int64_t *n_total, int32_t *status) {
    if (!ctx) return MAD_EINVAL;
    if (!overlap || !group_first || !n_out || !n_total || !status || n < 0 || cap < 0 || out_cap < cap || (out_cap && (!idx_out || !key_out || !rank_out)))
        return mad_fail(ctx, MAD_EINVAL, "mad_rank_models: null pointer, n = %d, cap = %lld or out_cap = %lld", n, (long long)cap, (long long)out_cap);
    *n_out = *n_total = 0;
    *status = 0;
    rank_plan_reset(ctx);
    const int g = n_groups;
    if (n > MAD_RANK_MAX_N || g > MAD_RANK_MAX_K || g < 1)
        return mad_fail(ctx, MAD_EDOM, "mad_rank_models: n = %d (at most %d), %d groups (1 .. %d)", n, MAD_RANK_MAX_N, g, MAD_RANK_MAX_K);
    if (group_first[0] != 0 || group_first[g] != n) return mad_fail(ctx, MAD_EDOM, "mad_rank_models: the groups do not cover rows 0 .. %d", n);
    for (int l = 0; l < g; l++)
        if (group_first[l + 1] < group_first[l]) return mad_fail(ctx, MAD_EDOM, "mad_rank_models: group %d ends before it begins", l);
    if (!rank_table_ok(overlap, n)) return mad_fail(ctx, MAD_EDOM, "mad_rank_models: an overlap is negative or not finite");
    RankJob J;
    J.models = true, J.n = n, J.k = g;
    J.aux.assign(48, 0);
    long long w = 1;      // (at most 6^16 picks from 96 rows: no overflow)
    for (int l = g - 1; l >= 0; l--) {
        J.aux[l] = (unsigned long long)w;
        w *= group_first[l + 1] - group_first[l];
    }
    for (int l = 0; l <= g; l++) J.aux[16 + l] = (unsigned long long)group_first[l];
    J.space = w;
    J.launch_items = launch_items > 0 ? launch_items : MAD_RANK_LAUNCH_ITEMS;
    J.budget = budget > 0 ? budget : MAD_RANK_BUDGET;
    J.prune = !rank_no_prune();
    const long long want = std::min<long long>(cap, J.space);
    if (want > MAD_RANK_MAX_TOP) return mad_fail(ctx, MAD_EDOM, "mad_rank_models: the first %lld entries asked for, at most %d", want, MAD_RANK_MAX_TOP);
    if (want == 0) return MAD_OK;
    J.tab.assign((size_t)n * (n + 1) / 2, 0);
    for (int b = 0; b < n; b++) {
        double *col = (double *)J.tab.data() + (size_t)b * (b + 1) / 2;
        for (int a = 0; a < b; a++) col[a] = (overlap[(size_t)a * n + b] + overlap[(size_t)b * n + a]) + 0.0;
        col[b] = overlap[(size_t)b * n + b] + 0.0;
    }
    RankPass P;
    MAD_TRY(rank_pass(ctx, J, MAD_RANK_TOP, (int)want, ~0ull, P));
    if (!P.exhausted && P.key.size() == (size_t)want && P.key.back() != 0) {
        // second pass: everything up to the cap-th device sum widened by the band.  (A cap-th sum of exactly 0 needs none: a device
        // sum of 0 has only zero terms, numpy's sum is 0 too, and the rank decides inside that class.)
        double t;
        std::memcpy(&t, &P.key.back(), 8);
        const double wide = std::nextafter(t * rank_band_factor(g), INFINITY);
        unsigned long long thr;
        std::memcpy(&thr, &wide, 8);
        const int dev_cap = (int)std::min<long long>(out_cap, MAD_RANK_MAX_OUT);
        RankPass Q;
        MAD_TRY(rank_pass(ctx, J, MAD_RANK_BELOW, dev_cap, thr, Q));
        if (!Q.exhausted && Q.total > dev_cap) {
            *n_total = Q.total;
            return mad_fail(ctx, MAD_ENOSPC, "mad_rank_models: %lld picks within the band of the %lld-th sum, room for %d", Q.total, want, dev_cap);
        }
        P = Q;
        ctx->last_rank_band_extra = !Q.exhausted && Q.total > want;
    }
    if (P.exhausted) {
        *status = 1;
        return MAD_OK;
    }
    *n_total = (int64_t)P.key.size();
    for (size_t e = 0; e < P.key.size(); e++) {
        long long r = P.rank[e];
        for (int l = 0; l < g; l++) {
            const long long d = r / (long long)J.aux[l];
            r -= d * (long long)J.aux[l];
            idx_out[e * g + l] = group_first[l] + (int32_t)d;
        }
        std::memcpy(&key_out[e], &P.key[e], 8);
        rank_out[e] = P.rank[e];
    }
    *n_out = (int64_t)P.key.size();
    return MAD_OK;
}

extern "C" int mad_last_rank_plan(mad_ctx *ctx, int64_t *launches, int64_t *evaluated, int64_t *skipped, int32_t *band_extra) {
    if (!ctx) return MAD_EINVAL;
    if (launches) *launches = ctx->last_rank_launches;
    if (evaluated) *evaluated = ctx->last_rank_evaluated;
    if (skipped) *skipped = ctx->last_rank_skipped;
    if (band_extra) *band_extra = ctx->last_rank_band_extra;
    return MAD_OK;
}
