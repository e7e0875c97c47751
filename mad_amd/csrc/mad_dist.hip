// mad_dist.hip -- the exchanges between the GPUs of a sharded step (mad_dist_init, mad_dist_or_allreduce,
// mad_dist_allgather_topk) and the merge of the shards' top-k records on the device (k_shard_merge).
//
// RCCL is never linked: the six entry points used are resolved with dlopen / dlsym the first time mad_dist_unique_id or
// mad_dist_init (with an id) is called.  A process that has imported torch has one RCCL mapped already (torch's own copy, soname
// librccl.so.1); dlopen by that soname hands back that copy, so the process keeps exactly one -- the concern MAD_OWN_HIP_RUNTIME
// handles for the HIP runtime.  rccl.h is included for its types only.
#include "mad_common.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {

struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;      // one per process, never unloaded (RCCL keeps threads and device state of its own)

struct DistComm {
    int nranks = 1, rank = 0;
    bool rehearsal = true;
    ncclComm_t comm = nullptr;
    const uint8_t *peer_or = nullptr;      // rehearsal: what the absent ranks contribute to an OR-reduce of peer_n flags
    int64_t peer_n = 0;
};

int rccl_load(mad_ctx *ctx) {
    if (g_rccl.handle) return MAD_OK;
    static const char *names[] = {"librccl.so.1", "librccl.so"};
    char tried[400] = {0};
    void *h = nullptr;
    for (const char *n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
        const char *why = dlerror();
        const size_t at = strlen(tried);
        snprintf(tried + at, sizeof(tried) - at, "%s%s (%s)", at ? "; " : "", n, why ? why : "?");
    }
    if (!h) return mad_fail(ctx, MAD_ENODEV, "RCCL cannot be loaded, tried dlopen of %s", tried);
    RcclApi api;
    api.handle = h;
    const char *missing = nullptr;
    auto sym = [&](const char *name) { void *p = dlsym(h, name); if (!p && !missing) missing = name; return p; };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
    api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    if (missing) {
        dlclose(h);
        return mad_fail(ctx, MAD_ENODEV, "RCCL (dlopen of librccl.so.1, then librccl.so) has no symbol %s", missing);
    }
    g_rccl = api;
    return MAD_OK;
}

#define MAD_RCCL(call)                                                                                     \
    do {                                                                                                   \
        ncclResult_t r__ = (call);                                                                         \
        if (r__ != ncclSuccess) return mad_fail(ctx, MAD_EHIP, "%s failed: %s", #call, g_rccl.GetErrorString(r__)); \
    } while (0)

inline DistComm *comm_of(mad_ctx *ctx) { return ctx ? (DistComm *)ctx->dist : nullptr; }
inline hipStream_t stream_of(mad_ctx *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->lane_stream[0]; }

}  // namespace

// flags[i] = max(flags[i], peer[i]): the OR of bytes 0 / 1, as ncclMax forms it
__global__ void k_or_bytes(uint8_t *__restrict__ flags, const uint8_t *__restrict__ peer, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t a = flags[i], b = peer[i];
        flags[i] = a > b ? a : b;
    }
}

// The merge of nranks shard records [m, flags, |hi cloud|, pairs][k x 23 rows][k counts][k pair ranks] into one (the order of
// dist.merge_topk: count descending, global pair rank ascending, entries of equal key in the order of the records).  One
// workgroup.  Entry i = (record i / k, position i % k) is valid when its position is below its record's m; a valid entry's key is
// (max count - count) << 40 | pair rank (k_topk_selected's), every other entry's is ~0.  Up to 1024 entries, an entry's place is the
// number of smaller (key, i): n broadcast reads of LDS per thread; beyond, a bitonic network over cap = the next power of two
// (keys and the entries' indices side by side in LDS), one barrier per stage.  Then all lanes gather the winners' 184-byte rows
// as 64-bit words, bit for bit.  Everything read from the records is range-checked before it becomes an index or a key.
// LDS: cap x 10 bytes (+ cap x 2 for the short form), 80 KiB at the bound of 8192 entries.
#define SM_THREADS 1024
__global__ __launch_bounds__(SM_THREADS) void k_shard_merge(const double *__restrict__ all, int nranks, int k, int rec, int cap, int counting,
                                                            double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *key = (unsigned long long *)smem;
    unsigned short *src = (unsigned short *)(smem + (size_t)cap * 8);
    unsigned short *ord = src + cap;      // short form only
    __shared__ int s_maxc, s_flags, s_bad, s_valid;
    __shared__ unsigned long long s_pairs;
    const int N = nranks * k, tid = threadIdx.x;
    const size_t off_cnt = 4 + (size_t)k * MAD_RESULT_COLS, off_rank = off_cnt + k;
    if (tid == 0) { s_maxc = 0; s_flags = 0; s_bad = 0; s_valid = 0; s_pairs = 0; }
    __syncthreads();
    const double lhi0 = all[2];
    {      // the records' heads
        int fl = 0, bad = 0;
        unsigned long long pr = 0;
        for (int s = tid; s < nranks; s += SM_THREADS) {
            const double *r = all + (size_t)s * rec;
            const double m = r[0], f = r[1], p = r[3];
            if (!(m >= 0 && m <= (double)k)) bad = 1;      // (NaN fails every test)
            if (f >= 0 && f < 2147483648.0) fl |= (int)f; else bad = 1;
            if (!(r[2] == lhi0)) bad = 1;
            if (p >= 0 && p < 9.0e15) pr += (unsigned long long)p; else bad = 1;
        }
        if (fl) atomicOr(&s_flags, fl);
        if (bad) atomicOr(&s_bad, 1);
        if (pr) atomicAdd(&s_pairs, pr);
    }
    auto entry = [&](int i, double *c, double *p) -> bool {      // valid and within the key's range?  *c, *p: its count and pair rank
        const int s = i / k, t = i - s * k;
        const double *r = all + (size_t)s * rec;
        const double md = r[0];
        const int m = (md >= 0 && md <= (double)k) ? (int)md : 0;
        if (t >= m) return false;
        *c = r[off_cnt + t];
        *p = r[off_rank + t];
        return true;
    };
    {      // the largest count, the number of valid entries
        int mx = 0, nv = 0, bad = 0;
        for (int i = tid; i < N; i += SM_THREADS) {
            double c, p;
            if (!entry(i, &c, &p)) continue;
            if (c >= 0 && c < 16777216.0 && p >= 0 && p < 1099511627776.0) { mx = max(mx, (int)c); nv++; }
            else bad = 1;
        }
        if (mx) atomicMax(&s_maxc, mx);
        if (nv) atomicAdd(&s_valid, nv);
        if (bad) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    const int flags = s_flags | (s_bad ? MAD_SHARD_FLAG_MISMATCH : 0);
    const int n_out = flags ? 0 : min(s_valid, k);
    const int maxc = s_maxc;
    const unsigned short *win = counting ? ord : src;
    if (n_out > 0) {      // (uniform over the workgroup)
        for (int i = tid; i < cap; i += SM_THREADS) {
            unsigned long long kv = ~0ull;
            double c, p;
            if (i < N && entry(i, &c, &p)) kv = ((unsigned long long)(maxc - (int)c) << 40) | (unsigned long long)p;
            key[i] = kv;
            src[i] = (unsigned short)i;
        }
        __syncthreads();
        if (counting) {
            if (tid < N) {
                const unsigned long long mine = key[tid];
                int place = 0;
                for (int j = 0; j < N; j++) {
                    const unsigned long long o = key[j];
                    place += (o < mine || (o == mine && j < tid)) ? 1 : 0;
                }
                if (place < n_out) ord[place] = (unsigned short)tid;
            }
            __syncthreads();
        } else {
            const int half = cap >> 1;
            for (int kk = 2; kk <= cap; kk <<= 1)
                for (int j = kk >> 1; j > 0; j >>= 1) {
                    for (int q = tid; q < half; q += SM_THREADS) {
                        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), ixj = i | j;
                        const unsigned long long a = key[i], b = key[ixj];
                        const unsigned short sa = src[i], sb = src[ixj];
                        const bool up = (i & kk) == 0;
                        const bool gt = a > b || (a == b && sa > sb);
                        if (gt == up) { key[i] = b; key[ixj] = a; src[i] = sb; src[ixj] = sa; }
                    }
                    __syncthreads();
                }
        }
    }
    // the merged record: rows, counts and ranks as 64-bit words (NaN payloads and signed zeros travel unchanged), zeros behind them
    const unsigned long long *a64 = (const unsigned long long *)all;
    unsigned long long *o64 = (unsigned long long *)out;
    const int n_words = k * MAD_RESULT_COLS;
    for (int e = tid; e < n_words; e += SM_THREADS) {
        const int o = e / MAD_RESULT_COLS, c = e - o * MAD_RESULT_COLS;
        unsigned long long v = 0;
        if (o < n_out) {
            const int idx = win[o], s = idx / k, t = idx - s * k;
            v = a64[(size_t)s * rec + 4 + (size_t)t * MAD_RESULT_COLS + c];
        }
        o64[4 + e] = v;
    }
    for (int o = tid; o < k; o += SM_THREADS) {
        unsigned long long vc = 0, vr = 0;
        if (o < n_out) {
            const int idx = win[o], s = idx / k, t = idx - s * k;
            vc = a64[(size_t)s * rec + off_cnt + t];
            vr = a64[(size_t)s * rec + off_rank + t];
        }
        o64[off_cnt + o] = vc;
        o64[off_rank + o] = vr;
    }
    if (tid == 0) { out[0] = (double)n_out; out[1] = (double)flags; out[2] = lhi0; out[3] = (double)s_pairs; }
}

static int shard_merge_check(mad_ctx *ctx, const char *who, int nranks, int64_t k) {
    if (nranks < 1 || k < 1) return mad_fail(ctx, MAD_EINVAL, "%s: %d records of k = %lld", who, nranks, (long long)k);
    if ((int64_t)nranks * k > MAD_SHARD_MERGE_MAX)
        return mad_fail(ctx, MAD_EDOM, "%s: %d records x k = %lld is more than the %d entries one workgroup sorts in LDS (merge on the host)", who, nranks,
                        (long long)k, MAD_SHARD_MERGE_MAX);
    return MAD_OK;
}

static int shard_merge_launch(mad_ctx *ctx, const double *d_all, int nranks, int64_t k, double *d_merged) {
    const int N = nranks * (int)k;
    int cap = 64;
    while (cap < N) cap <<= 1;
    const int counting = N <= SM_THREADS ? 1 : 0;
    const size_t lds = (size_t)cap * (counting ? 12 : 10);
    if (lds > 48 * 1024) MAD_HIP(hipFuncSetAttribute((const void *)k_shard_merge, hipFuncAttributeMaxDynamicSharedMemorySize, MAD_SHARD_MERGE_MAX * 10));
    hipLaunchKernelGGL(k_shard_merge, dim3(1), dim3(SM_THREADS), lds, ctx->stream, d_all, nranks, (int)k, (int)mad_match_shard_record_doubles(k), cap,
                       counting, d_merged);
    MAD_HIP(hipGetLastError());
    return MAD_OK;
}

extern "C" int mad_match_shard_merge(mad_ctx *ctx, const mad_set *hi, const double *d_all, int nranks, int64_t k, double *d_merged) {
    if (!ctx || !hi || !d_all || !d_merged || (const double *)d_merged == d_all) return MAD_EINVAL;
    MAD_TRY(shard_merge_check(ctx, "mad_match_shard_merge", nranks, k));
    mad_use_lane(ctx, hi->lane);
    return shard_merge_launch(ctx, d_all, nranks, k, d_merged);
}

// ---- the communicator ------------------------------------------------------------------------------------------------

extern "C" int mad_dist_unique_id(mad_ctx *ctx, void *id128) {
    if (!ctx || !id128) return MAD_EINVAL;
    static_assert(sizeof(ncclUniqueId) == MAD_DIST_ID_BYTES, "MAD_DIST_ID_BYTES");
    MAD_TRY(rccl_load(ctx));
    ncclUniqueId id;
    MAD_RCCL(g_rccl.GetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return MAD_OK;
}

extern "C" int mad_dist_init(mad_ctx *ctx, int nranks, int rank, const void *id128) {
    if (!ctx) return MAD_EINVAL;
    if (ctx->dist) return mad_fail(ctx, MAD_EINVAL, "mad_dist_init: the context has a communicator already (mad_dist_destroy first)");
    if (nranks < 1 || rank < 0 || rank >= nranks) return mad_fail(ctx, MAD_EINVAL, "mad_dist_init: rank %d of %d", rank, nranks);
    DistComm *c = new DistComm();
    c->nranks = nranks;
    c->rank = rank;
    c->rehearsal = id128 == nullptr;
    if (id128) {
        int rc = rccl_load(ctx);
        if (rc == MAD_OK) {
            ncclUniqueId id;
            memcpy(&id, id128, sizeof(id));
            hipError_t e = hipSetDevice(ctx->device);
            if (e != hipSuccess) rc = mad_fail(ctx, MAD_EHIP, "hipSetDevice(%d): %s", ctx->device, hipGetErrorString(e));
            else {
                ncclResult_t r = g_rccl.CommInitRank(&c->comm, nranks, id, rank);
                if (r != ncclSuccess) rc = mad_fail(ctx, MAD_EHIP, "ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, g_rccl.GetErrorString(r));
            }
        }
        if (rc != MAD_OK) { delete c; return rc; }
    }
    ctx->dist = c;
    return MAD_OK;
}

extern "C" int mad_dist_destroy(mad_ctx *ctx) {
    if (!ctx) return MAD_EINVAL;
    DistComm *c = comm_of(ctx);
    if (!c) return MAD_OK;
    ctx->dist = nullptr;
    int rc = MAD_OK;
    if (c->comm) {      // nothing of the communicator may be in flight when it goes
        (void)hipSetDevice(ctx->device);
        for (int l = 0; l < MAD_LANES; l++) (void)hipStreamSynchronize(ctx->lane_stream[l]);
        ncclResult_t r = g_rccl.CommDestroy(c->comm);
        if (r != ncclSuccess) rc = mad_fail(ctx, MAD_EHIP, "ncclCommDestroy failed: %s", g_rccl.GetErrorString(r));
    }
    delete c;
    return rc;
}

extern "C" int mad_dist_info(mad_ctx *ctx, int *nranks, int *rank, int *rehearsal) {
    DistComm *c = comm_of(ctx);
    if (!ctx) return MAD_EINVAL;
    if (!c) return mad_fail(ctx, MAD_EINVAL, "mad_dist_info: no communicator (mad_dist_init)");
    if (nranks) *nranks = c->nranks;
    if (rank) *rank = c->rank;
    if (rehearsal) *rehearsal = c->rehearsal ? 1 : 0;
    return MAD_OK;
}

extern "C" int mad_dist_rehearse_flags(mad_ctx *ctx, const uint8_t *d_peer_or, int64_t n) {
    DistComm *c = comm_of(ctx);
    if (!ctx) return MAD_EINVAL;
    if (!c || !c->rehearsal) return mad_fail(ctx, MAD_EINVAL, "mad_dist_rehearse_flags: needs a rehearsal communicator");
    if (d_peer_or && n < 1) return mad_fail(ctx, MAD_EINVAL, "mad_dist_rehearse_flags: n = %lld", (long long)n);
    c->peer_or = d_peer_or;
    c->peer_n = d_peer_or ? n : 0;
    return MAD_OK;
}

extern "C" int mad_dist_or_allreduce(mad_ctx *ctx, void *stream, uint8_t *d_flags, int64_t n) {
    DistComm *c = comm_of(ctx);
    if (!ctx || !d_flags || n < 0) return MAD_EINVAL;
    if (!c) return mad_fail(ctx, MAD_EINVAL, "mad_dist_or_allreduce: no communicator (mad_dist_init)");
    if (n == 0) return MAD_OK;
    hipStream_t s = stream_of(ctx, stream);
    if (c->rehearsal) {
        if (!c->peer_or) return MAD_OK;      // the identity
        if (c->peer_n != n) return mad_fail(ctx, MAD_EINVAL, "mad_dist_or_allreduce: %lld flags, the rehearsal's peers have %lld", (long long)n, (long long)c->peer_n);
        hipLaunchKernelGGL(k_or_bytes, dim3((unsigned)std::min<int64_t>(mad_ceil_div(n, 256), 1024)), dim3(256), 0, s, d_flags, c->peer_or, n);
        MAD_HIP(hipGetLastError());
        return MAD_OK;
    }
    MAD_RCCL(g_rccl.AllReduce(d_flags, d_flags, (size_t)n, ncclUint8, ncclMax, c->comm, s));
    return MAD_OK;
}

static int allgather_on(mad_ctx *ctx, DistComm *c, hipStream_t s, const void *d_send, void *d_recv, int64_t bytes) {
    if (c->rehearsal) {
        void *slot = (char *)d_recv + (size_t)c->rank * (size_t)bytes;
        if (slot != d_send) MAD_HIP(hipMemcpyAsync(slot, d_send, (size_t)bytes, hipMemcpyDeviceToDevice, s));
        return MAD_OK;
    }
    MAD_RCCL(g_rccl.AllGather(d_send, d_recv, (size_t)bytes, ncclUint8, c->comm, s));
    return MAD_OK;
}

extern "C" int mad_dist_allgather(mad_ctx *ctx, void *stream, const void *d_send, void *d_recv, int64_t bytes_per_rank) {
    DistComm *c = comm_of(ctx);
    if (!ctx || !d_send || !d_recv || bytes_per_rank < 0) return MAD_EINVAL;
    if (!c) return mad_fail(ctx, MAD_EINVAL, "mad_dist_allgather: no communicator (mad_dist_init)");
    if (bytes_per_rank == 0) return MAD_OK;
    return allgather_on(ctx, c, stream_of(ctx, stream), d_send, d_recv, bytes_per_rank);
}

extern "C" int mad_dist_allgather_topk(mad_ctx *ctx, const mad_set *hi, const double *d_mine, double *d_all, int64_t k, double *d_merged) {
    DistComm *c = comm_of(ctx);
    if (!ctx || !hi || !d_mine || !d_all || !d_merged || d_merged == d_all) return MAD_EINVAL;
    if (!c) return mad_fail(ctx, MAD_EINVAL, "mad_dist_allgather_topk: no communicator (mad_dist_init)");
    MAD_TRY(shard_merge_check(ctx, "mad_dist_allgather_topk", c->nranks, k));
    mad_use_lane(ctx, hi->lane);
    MAD_TRY(allgather_on(ctx, c, ctx->stream, d_mine, d_all, mad_match_shard_record_doubles(k) * 8));
    return shard_merge_launch(ctx, d_all, c->nranks, k, d_merged);
}

extern "C" int mad_dist_scratch(mad_ctx *ctx, int lane, int which, int64_t bytes, void **d_out) {
    if (!ctx || !d_out) return MAD_EINVAL;
    if (lane < 0 || lane >= MAD_LANES || which < 0 || which >= MAD_DIST_BUFS || bytes < 0)
        return mad_fail(ctx, MAD_EINVAL, "mad_dist_scratch: lane %d, buffer %d, %lld bytes", lane, which, (long long)bytes);
    mad_use_lane(ctx, lane);
    MAD_TRY(mad_reserve(ctx, ctx->dist_buf[lane][which], (size_t)bytes));
    *d_out = ctx->dist_buf[lane][which].p;
    return MAD_OK;
}

extern "C" int mad_dist_copy(mad_ctx *ctx, void *dst, const void *src, int64_t bytes, int kind) {
    if (!ctx || !dst || !src || bytes < 0 || (kind != 0 && kind != 1)) return MAD_EINVAL;
    MAD_HIP(hipSetDevice(ctx->device));
    MAD_HIP(hipDeviceSynchronize());
    if (bytes > 0) MAD_HIP(hipMemcpy(dst, src, (size_t)bytes, kind == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return MAD_OK;
}
