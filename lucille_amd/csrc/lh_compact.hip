/*
 * lh_compact.hip -- lh_accel_compact_device: the records of a ray batch -> the list of the rays a caller goes on with (the rays that
 * hit, for their shadow rays; the paths that survived, for the next bounce), in the form lh_accel_intersect_device_indexed takes:
 * ids and their count, both on the device, nothing read back.
 *
 * Two passes over the candidates, tiles of LH_CT_TILE entries per 256-thread workgroup:
 *   k_compact<false>  counts the selected entries of every tile (wave ballots, popcounts);
 *   k_compact_scan    one workgroup turns the tile counts into exclusive offsets and writes the total;
 *   k_compact<true>   tests the entries again and stores the selected ids at offset + rank.
 * A thread takes entries tile + j * 256 + tid, j = 0 .. 7 (coalesced loads); an id's rank is the selected entries of the rounds
 * before its own, of the waves before its own in its round (four counts through LDS) and of the lanes before its own (the
 * ballot): the output keeps the order of the input list whatever the grid does -- no atomics, no order left to the scheduler.
 * The records are read twice; the test is one word (or byte) per entry.  Both passes read the input list and count, so the outputs
 * must not alias them (refused).
 */
#include "lh_internal.h"

#define LH_CT_ROUNDS 8u
#define LH_CT_TILE   (256u * LH_CT_ROUNDS)
#define LH_CT_SCAN   1024u

namespace {

struct CompactIn {
    const uint32_t *prim;       /* closest-hit records: the prim words, `stride` words apart (1: SoA, 4: lh_rec16_t) -- or NULL ... */
    const uint8_t  *occ;        /* ... any-hit bytes */
    uint32_t stride;
    uint32_t want;              /* 1: the entries whose record is a hit / whose byte is non-zero; 0: the others */
    uint32_t n;                 /* records */
    const uint32_t *index;      /* the input list, or NULL: the identity list */
    const uint32_t *count;      /* its length on the device (clamped to m), or NULL */
    uint32_t m;                 /* list entries at most */
};

template <bool SCATTER>
__global__ __launch_bounds__(256) void k_compact(const CompactIn in, uint32_t *__restrict__ partial, uint32_t *__restrict__ out)
{
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    uint32_t m = in.m;
    if (in.count) { const uint32_t c = *in.count; if (c < m) m = c; }
    const uint32_t tile = blockIdx.x * LH_CT_TILE;                 /* m <= 2^30: no wrap */
    uint32_t running = SCATTER ? partial[blockIdx.x] : 0u;
    if (tile < m) {                                                /* workgroup-uniform */
        for (uint32_t j = 0; j < LH_CT_ROUNDS; j++) {
            const uint32_t k = tile + j * 256u + tid;
            bool sel = false; uint32_t id = 0u;
            if (k < m) {
                id = in.index ? in.index[k] : k;
                if (id < in.n) {
                    const uint32_t hit = in.prim ? (in.prim[(size_t)id * in.stride] != LH_MISS_PRIM) : (in.occ[id] != 0);
                    sel = hit == in.want;
                }
            }
            const unsigned long long b = __ballot(sel);
            if (lane == 0u) wsum[w] = (uint32_t)__popcll(b);
            __syncthreads();
            const uint32_t s0 = wsum[0], s1 = wsum[1], s2 = wsum[2], s3 = wsum[3];
            if (SCATTER && sel) {
                const uint32_t before = (w > 0u ? s0 : 0u) + (w > 1u ? s1 : 0u) + (w > 2u ? s2 : 0u);
                out[running + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = id;
            }
            running += s0 + s1 + s2 + s3;
            __syncthreads();
        }
    }
    if (!SCATTER && tid == 0u) partial[blockIdx.x] = running;
}

/* exclusive scan of the tile counts in place, the total to *total: one workgroup, a contiguous run of tiles per thread */
__global__ __launch_bounds__(LH_CT_SCAN) void k_compact_scan(uint32_t *__restrict__ partial, uint32_t ntiles, uint32_t *__restrict__ total)
{
    __shared__ uint32_t sums[LH_CT_SCAN];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + LH_CT_SCAN - 1u) / LH_CT_SCAN;
    const uint32_t k0 = tid * per < ntiles ? tid * per : ntiles, k1 = k0 + per < ntiles ? k0 + per : ntiles;
    uint32_t mine = 0u;
    for (uint32_t k = k0; k < k1; k++) mine += partial[k];
    sums[tid] = mine;
    __syncthreads();
    for (uint32_t off = 1u; off < LH_CT_SCAN; off <<= 1) {         /* inclusive scan of the threads' sums */
        const uint32_t add = tid >= off ? sums[tid - off] : 0u;
        __syncthreads();
        sums[tid] += add;
        __syncthreads();
    }
    uint32_t run = sums[tid] - mine;
    for (uint32_t k = k0; k < k1; k++) { const uint32_t c = partial[k]; partial[k] = run; run += c; }
    if (tid == LH_CT_SCAN - 1u) *total = sums[tid];
}

/* the tile counts of the calls on one stream of one device: calls on a stream are ordered, so they share a block; other streams get their own */
#define LH_CT_SLOTS 8
struct Scratch { int device; hipStream_t stream; uint32_t *p; size_t cap; bool used; };
Scratch g_scratch[LH_CT_SLOTS];
pthread_mutex_t g_scratch_mu = PTHREAD_MUTEX_INITIALIZER;

uint32_t *scratch_for(int device, hipStream_t s, size_t words)
{
    Scratch *sl = NULL, *free_sl = NULL;
    for (int k = 0; k < LH_CT_SLOTS; k++) {
        if (g_scratch[k].used && g_scratch[k].device == device && g_scratch[k].stream == s) { sl = &g_scratch[k]; break; }
        if (!g_scratch[k].used && !free_sl) free_sl = &g_scratch[k];
    }
    if (!sl) sl = free_sl;
    if (!sl) {                               /* more streams than slots: wait for the device(s), then recycle slot 0 */
        if (hipDeviceSynchronize() != hipSuccess) return NULL;
        sl = &g_scratch[0];
        if (sl->device != device) { (void)hipFree(sl->p); sl->p = NULL; sl->cap = 0; }       /* hipFree waits for the work that may still read it */
    }
    if (sl->cap < words) {
        size_t cap = 4096;
        while (cap < words) cap *= 2;
        if (sl->p) (void)hipFree(sl->p);      /* hipFree waits for the work that may still read it */
        sl->p = NULL; sl->cap = 0;
        if (hipMalloc((void **)&sl->p, cap * sizeof(uint32_t)) != hipSuccess) { sl->p = NULL; sl->used = false; return NULL; }
        sl->cap = cap;
    }
    sl->device = device; sl->stream = s; sl->used = true;
    return sl->p;
}

} /* namespace */

extern "C" int lh_accel_compact_device(size_t n, int record_format, const void *d_prim_or_rec16, const void *d_occluded, int select,
                                       const void *d_index_in, size_t n_index_in, const void *d_count_in,
                                       void *d_index_out, void *d_count_out, void *stream)
{
    const char *what = "lh_accel_compact_device";
    if (select != LH_SELECT_HIT && select != LH_SELECT_MISS && select != LH_SELECT_OCCLUDED && select != LH_SELECT_UNOCCLUDED)
        return fail("%s: unknown select %d", what, select);
    const bool closest = select == LH_SELECT_HIT || select == LH_SELECT_MISS;
    if (closest && record_format != LH_REC_F64 && record_format != LH_REC16) return fail("%s: unknown record format %d", what, record_format);
    if (closest && !d_prim_or_rec16) return fail("%s: LH_SELECT_HIT / LH_SELECT_MISS read the closest-hit records: prim_or_rec16 is NULL", what);
    if (closest && ((uintptr_t)d_prim_or_rec16 & (record_format == LH_REC16 ? 15u : 3u)) != 0) return fail("%s: the record array is not aligned to its records", what);
    if (!closest && !d_occluded) return fail("%s: LH_SELECT_OCCLUDED / LH_SELECT_UNOCCLUDED read the any-hit bytes: occluded is NULL", what);
    if (!d_index_out || !d_count_out) return fail("%s: the output list and its count are NULL", what);
    if ((((uintptr_t)d_index_in | (uintptr_t)d_count_in | (uintptr_t)d_index_out | (uintptr_t)d_count_out) & 3u) != 0)
        return fail("%s: lists and counts are 32-bit words: a pointer is not 4-byte aligned", what);
    if (n > 0xFFFFFFFFull) return fail("%s: ray ids are 32 bits wide: 2^32 - 1 records at most (%zu given)", what, n);
    /* the candidates: the given list, or (no list, no count, n_index_in == 0) all n records */
    const size_t m = (d_index_in || d_count_in || n_index_in) ? n_index_in : n;
    if (m > ((size_t)1 << 30)) return fail("%s: a list holds 2^30 entries at most (%zu given)", what, m);
    /* both passes read the input list and its count, and the second one runs after the output count and beside the output list's stores:
     * compacting a list in place would read what it is overwriting */
    if (d_count_in && d_count_in == d_count_out) return fail("%s: the output count must not alias the input count", what);
    if (d_index_in) {
        const uintptr_t i0 = (uintptr_t)d_index_in, i1 = i0 + 4u * m, o0 = (uintptr_t)d_index_out, o1 = o0 + 4u * m;
        if (i0 < o1 && o0 < i1) return fail("%s: the output list must not overlap the input list", what);
    }
    {
        const uintptr_t c = (uintptr_t)d_count_out, o0 = (uintptr_t)d_index_out, i0 = (uintptr_t)d_index_in, k = (uintptr_t)d_count_in;
        if ((c >= o0 && c < o0 + 4u * m) || (d_index_in && c >= i0 && c < i0 + 4u * m) || (d_count_in && k >= o0 && k < o0 + 4u * m))
            return fail("%s: a count must not lie inside a list that the call reads or writes", what);
    }
    hipStream_t s = (hipStream_t)stream;
    if (m == 0 || n == 0) { HIPCHK(hipMemsetAsync(d_count_out, 0, sizeof(uint32_t), s)); return 0; }
    const uint32_t ntiles = (uint32_t)((m + LH_CT_TILE - 1u) / LH_CT_TILE);
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    /* the lock is held until the three kernels are enqueued: a thread that recycles a slot meanwhile waits, then synchronises the device first */
    struct Hold { Hold() { pthread_mutex_lock(&g_scratch_mu); } ~Hold() { pthread_mutex_unlock(&g_scratch_mu); } } hold;
    uint32_t *partial = scratch_for(device, s, ntiles);
    if (!partial) return fail("%s: no device memory for %u tile counts", what, ntiles);
    CompactIn in;
    in.prim = closest ? (const uint32_t *)d_prim_or_rec16 : NULL; in.occ = closest ? NULL : (const uint8_t *)d_occluded;
    in.stride = record_format == LH_REC16 ? 4u : 1u;
    in.want = (select == LH_SELECT_HIT || select == LH_SELECT_OCCLUDED) ? 1u : 0u;
    in.n = (uint32_t)n; in.index = (const uint32_t *)d_index_in; in.count = (const uint32_t *)d_count_in; in.m = (uint32_t)m;
    hipLaunchKernelGGL((k_compact<false>), dim3(ntiles), dim3(256), 0, s, in, partial, (uint32_t *)NULL);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(LH_CT_SCAN), 0, s, partial, ntiles, (uint32_t *)d_count_out);
    hipLaunchKernelGGL((k_compact<true>), dim3(ntiles), dim3(256), 0, s, in, partial, (uint32_t *)d_index_out);
    HIPCHK(hipGetLastError());
    return 0;
}
