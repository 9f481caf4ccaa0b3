/*
 * lh_order.hip -- a ray dump in bin order (lh_order.h): the passes that make the ordered copy of a dump's rays and bring its records back.
 *
 *   k_order_count        keys + the histogram of every block                  reads org (and dir when the key has the octant)
 *   k_order_scan_*       the run table: offset[block][bin]                    (small)
 *   k_order_copy         the stable partition: ordered org, dir; dest[i]      reads org, dir; writes the copy
 *   ... the walk of the ordered copy (lh_launch_trace, as for a caller's dump: lh_query.hip lh_launch) ...
 *   k_order_back         caller's record i = ordered record dest[i]           reads dest, the ordered records; writes the caller's arrays
 *
 * 64 bins (6-bit keys), blocks of LH_ORDER_BLOCK rays, one workgroup per block.  The copy and the way back take a block in tiles of 1 024
 * consecutive rays and sort a tile in LDS first: in bin order a tile is 64 pieces of 16 rays on average, each piece contiguous in the ordered
 * copy, so neighbouring lanes store (load) neighbouring addresses -- a lane per 8 bytes of a run, not a lane per run.  The pieces of one
 * bin follow each other from tile to tile and block to block: the lines a tile leaves half written are finished by the same workgroup's next tile,
 * in the same L2.  fp64 rays, fp64 records or any-hit bytes.
 */
#include "lh_internal.h"
#include "lh_order.h"

#define ORD_T      256                  /* threads of a workgroup */
#define ORD_NB     64u                  /* bins: one per lane of a wave */
#define ORD_TILE   1024u                /* rays sorted in LDS at a time */
#define ORD_PER    (ORD_TILE / ORD_T)   /* ... a thread's share: rays s * 256 + t of the tile */
#define ORD_SLICES (ORD_TILE / 64u)     /* wave-sized slices of a tile, in ray order: slice s * 4 + w */
#define ORD_CHUNKS (ORD_T * 48 / 16)    /* 16-byte pieces of the count's stage */

struct OrdRays { const char *org, *dir; size_t n; lh_order_grid_t g; };

/* 16 bytes at `off` of an array of nbytes (a multiple of 8): nothing is read beyond its end */
__device__ __forceinline__ uint4 ord_load16(const char *base, size_t off, size_t nbytes)
{
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (off + 16 <= nbytes) r = *(const uint4 *)(base + off);
    else if (off + 8 <= nbytes) { const uint2 h = *(const uint2 *)(base + off); r.x = h.x; r.y = h.y; }
    return r;
}

/* pass 1: counts[block][bin].  The rays arrive in LDS by 16-byte loads (a block starts on a multiple of 16 bytes when the arrays do: lh_order_run
 * checks that), 12 KiB a step: org and dir of 256 rays (OCT: the key has the octant), or org of 512 */
template <bool OCT>
__global__ __launch_bounds__(ORD_T) void k_order_count(OrdRays a, uint32_t *counts)
{
    constexpr uint32_t STEP = OCT ? ORD_T : 2 * ORD_T;
    __shared__ uint4 stage[2][ORD_CHUNKS];
    __shared__ uint32_t hist[ORD_NB];
    const size_t first = (size_t)blockIdx.x * LH_ORDER_BLOCK, nbytes = a.n * 24u;
    const size_t m = a.n - first < LH_ORDER_BLOCK ? a.n - first : LH_ORDER_BLOCK;
    const uint32_t nstep = (uint32_t)((m + STEP - 1) / STEP);
    uint4 v[3];
    auto fetch = [&](size_t r0) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint32_t q = threadIdx.x + ORD_T * j;
            const bool o = !OCT || q < ORD_CHUNKS / 2;
            v[j] = ord_load16(o ? a.org : a.dir, r0 * 24u + (size_t)(o ? q : q - ORD_CHUNKS / 2) * 16u, nbytes);
        }
    };
    if (threadIdx.x < ORD_NB) hist[threadIdx.x] = 0u;
    fetch(first);
#pragma unroll
    for (int j = 0; j < 3; j++) stage[0][threadIdx.x + ORD_T * j] = v[j];
    __syncthreads();
    for (uint32_t p = 0; p < nstep; p++) {
        const bool more = p + 1 < nstep;
        if (more) fetch(first + (size_t)(p + 1) * STEP);
        const double *so = (const double *)stage[p & 1];
        if (OCT) {
            const double *sd = so + 3 * ORD_T;
            if ((size_t)p * STEP + threadIdx.x < m) atomicAdd(&hist[lh_order_key(so + 3 * threadIdx.x, sd + 3 * threadIdx.x, &a.g)], 1u);
        } else {
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t i = threadIdx.x + ORD_T * h;
                if ((size_t)p * STEP + i < m) atomicAdd(&hist[lh_order_key(so + 3 * i, so + 3 * i, &a.g)], 1u);          /* no octant: dir is not looked at */
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < 3; j++) stage[(p + 1) & 1][threadIdx.x + ORD_T * j] = v[j];
        }
        __syncthreads();
    }
    if (threadIdx.x < ORD_NB) counts[(size_t)blockIdx.x * ORD_NB + threadIdx.x] = hist[threadIdx.x];
}

/* exclusive scan of one word per thread over the workgroup; *total: the sum */
__device__ __forceinline__ uint32_t ord_block_scan(uint32_t x, uint32_t *lds, uint32_t *total)
{
    const uint32_t t = threadIdx.x, nt = blockDim.x;
    uint32_t incl = x;
    lds[t] = x;
    __syncthreads();
    for (uint32_t s = 1; s < nt; s *= 2) {
        const uint32_t y = t >= s ? lds[t - s] : 0u;
        __syncthreads();
        incl += y; lds[t] = incl;
        __syncthreads();
    }
    *total = lds[nt - 1];
    return incl - x;
}

/* the scan over blocks within a bin: a workgroup per bin, a thread per stretch of consecutive blocks */
__global__ __launch_bounds__(ORD_T) void k_order_scan_blocks(const uint32_t *counts, uint32_t *offset, uint32_t *bintotal, uint32_t nblocks)
{
    __shared__ uint32_t lds[ORD_T];
    const uint32_t bin = blockIdx.x, per = (nblocks + ORD_T - 1) / ORD_T;
    const uint32_t lo = threadIdx.x * per < nblocks ? threadIdx.x * per : nblocks, hi = lo + per < nblocks ? lo + per : nblocks;
    uint32_t sum = 0u, total;
    for (uint32_t b = lo; b < hi; b++) sum += counts[(size_t)b * ORD_NB + bin];
    uint32_t run = ord_block_scan(sum, lds, &total);
    for (uint32_t b = lo; b < hi; b++) { offset[(size_t)b * ORD_NB + bin] = run; run += counts[(size_t)b * ORD_NB + bin]; }
    if (threadIdx.x == 0) bintotal[bin] = total;
}

/* ... and over bins: one wave */
__global__ void k_order_scan_bins(const uint32_t *bintotal, uint32_t *binbase)
{
    __shared__ uint32_t lds[ORD_NB];
    uint32_t total;
    binbase[threadIdx.x] = ord_block_scan(bintotal[threadIdx.x], lds, &total);
}

/* pass 2: the stable partition, a tile at a time.  A ray's rank among the tile's rays of its key = (those of the tile's earlier slices: cnt[][], scanned in
 * place by wave 0) + (those of its own slice's lower lanes: ballots); its slot in the sorted tile = start[key] + rank; its place in the ordered copy =
 * (where the block's run of the key has got to: base[key]) + rank.  The tile is sorted into LDS and written out 8 bytes a lane in slot order */
__global__ __launch_bounds__(ORD_T) void k_order_copy(OrdRays a, const uint32_t *offset, const uint32_t *binbase, double *oorg, double *odir, uint32_t *dest, uint16_t *slots)
{
    __shared__ double img[2][ORD_TILE * 3];
    __shared__ uint32_t cnt[ORD_SLICES][ORD_NB], sdest[ORD_TILE];
    __shared__ uint32_t start[ORD_NB], gbase[ORD_NB], base[ORD_NB];
    const size_t first = (size_t)blockIdx.x * LH_ORDER_BLOCK;
    const size_t m = a.n - first < LH_ORDER_BLOCK ? a.n - first : LH_ORDER_BLOCK;
    const uint32_t ntiles = (uint32_t)((m + ORD_TILE - 1) / ORD_TILE);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const double *org = (const double *)a.org, *dir = (const double *)a.dir;
    double o[ORD_PER][3], d[ORD_PER][3];
    auto fetch = [&](size_t tile0, uint32_t mt) {
#pragma unroll
        for (uint32_t s = 0; s < ORD_PER; s++) {
            const uint32_t j = s * ORD_T + threadIdx.x;
            const size_t r = 3 * (tile0 + (j < mt ? j : 0u));
#pragma unroll
            for (int c = 0; c < 3; c++) { o[s][c] = org[r + c]; d[s][c] = dir[r + c]; }
        }
    };
    if (w == 0) base[lane] = binbase[lane] + offset[(size_t)blockIdx.x * ORD_NB + lane];          /* base belongs to wave 0 */
    fetch(first, (uint32_t)(m < ORD_TILE ? m : ORD_TILE));
    for (uint32_t tile = 0; tile < ntiles; tile++) {
        const size_t tile0 = first + (size_t)tile * ORD_TILE;
        const uint32_t mt = (uint32_t)(first + m - tile0 < ORD_TILE ? first + m - tile0 : ORD_TILE);
        uint32_t key[ORD_PER], rank[ORD_PER];
#pragma unroll
        for (uint32_t s = 0; s < ORD_PER; s++) {
            const bool valid = s * ORD_T + threadIdx.x < mt;
            key[s] = valid ? lh_order_key(o[s], d[s], &a.g) : 0u;
            unsigned long long mine = __ballot(valid), have = mine;          /* lanes of the slice with my key; with the key this lane reports (its own number) */
#pragma unroll
            for (uint32_t i = 0; i < 6; i++) {
                const unsigned long long b = __ballot((key[s] >> i) & 1u);
                mine &= ((key[s] >> i) & 1u) ? b : ~b;
                have &= ((lane >> i) & 1u) ? b : ~b;
            }
            rank[s] = __popcll(mine & ((1ull << lane) - 1ull));
            cnt[s * (ORD_T / 64) + w][lane] = __popcll(have);
        }
        __syncthreads();
        if (w == 0) {
            uint32_t run = 0u;
            for (uint32_t q = 0; q < ORD_SLICES; q++) { const uint32_t c = cnt[q][lane]; cnt[q][lane] = run; run += c; }
            uint32_t incl = run;
#pragma unroll
            for (uint32_t s = 1; s < 64; s *= 2) { const uint32_t y = __shfl_up(incl, s); if (lane >= s) incl += y; }
            start[lane] = incl - run; gbase[lane] = base[lane]; base[lane] += run;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < ORD_PER; s++) {
            const uint32_t j = s * ORD_T + threadIdx.x;
            if (j < mt) {
                const uint32_t p = cnt[s * (ORD_T / 64) + w][key[s]] + rank[s], slot = start[key[s]] + p, at = gbase[key[s]] + p;
#pragma unroll
                for (int c = 0; c < 3; c++) { img[0][3 * slot + c] = o[s][c]; img[1][3 * slot + c] = d[s][c]; }
                sdest[slot] = at; dest[tile0 + j] = at; slots[tile0 + j] = (uint16_t)slot;
            }
        }
        if (tile + 1 < ntiles) fetch(tile0 + ORD_TILE, (uint32_t)(first + m - tile0 - ORD_TILE < ORD_TILE ? first + m - tile0 - ORD_TILE : ORD_TILE));
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 3 * mt; e += ORD_T) {
            const uint32_t slot = e / 3u, at = sdest[slot];
            if (at < a.n) {          /* at < n by construction; the test costs nothing and keeps a dump its caller rewrites meanwhile inside the copy */
                const size_t g = 3 * (size_t)at + (e - 3u * slot);
                oorg[g] = img[0][e]; odir[g] = img[1][e];
            }
        }
        /* no barrier here: the next tile writes cnt before its first barrier (last read above the third), img and sdest behind its second */
    }
}

/* pass 3: the caller's records, a tile at a time: the tile's places in the ordered copy into slot order (the copy noted every ray's slot), the records
 * loaded in that order -- neighbouring lanes, neighbouring records -- into LDS at their rays' positions, and stored in ray order */
template <bool CLOSEST>
__global__ __launch_bounds__(ORD_T) void k_order_back(size_t n, const uint32_t *dest, const uint16_t *slots, const uint32_t *sprim, const double *st, const double *su,
                                                      const double *sv, const uint8_t *socc, uint32_t *prim, double *t, double *u, double *v, uint8_t *occ)
{
    __shared__ uint32_t sdest[ORD_TILE];
    __shared__ uint16_t sray[ORD_TILE];
    __shared__ double bt[CLOSEST ? ORD_TILE : 1], bu[CLOSEST ? ORD_TILE : 1], bv[CLOSEST ? ORD_TILE : 1];
    __shared__ uint32_t bp[CLOSEST ? ORD_TILE : 1];
    __shared__ uint8_t bo[CLOSEST ? 1 : ORD_TILE];
    const size_t first = (size_t)blockIdx.x * LH_ORDER_BLOCK;
    const size_t m = n - first < LH_ORDER_BLOCK ? n - first : LH_ORDER_BLOCK;
    const uint32_t ntiles = (uint32_t)((m + ORD_TILE - 1) / ORD_TILE);
    for (uint32_t tile = 0; tile < ntiles; tile++) {
        const size_t tile0 = first + (size_t)tile * ORD_TILE;
        const uint32_t mt = (uint32_t)(first + m - tile0 < ORD_TILE ? first + m - tile0 : ORD_TILE);
#pragma unroll
        for (uint32_t s = 0; s < ORD_PER; s++) {
            const uint32_t j = s * ORD_T + threadIdx.x;
            if (j < mt) { const uint32_t slot = slots[tile0 + j] & (ORD_TILE - 1u); sdest[slot] = dest[tile0 + j]; sray[slot] = (uint16_t)j; }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < ORD_PER; s++) {
            const uint32_t j = s * ORD_T + threadIdx.x;
            if (j < mt) {
                const uint32_t at = sdest[j] < n ? sdest[j] : 0u, i = sray[j] & (ORD_TILE - 1u);
                if (CLOSEST) { bp[i] = sprim[at]; bt[i] = st[at]; bu[i] = su[at]; bv[i] = sv[at]; }
                else bo[i] = socc[at];
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < ORD_PER; s++) {
            const uint32_t j = s * ORD_T + threadIdx.x;
            if (j < mt) {
                if (CLOSEST) { prim[tile0 + j] = bp[j]; t[tile0 + j] = bt[j]; u[tile0 + j] = bu[j]; v[tile0 + j] = bv[j]; }
                else occ[tile0 + j] = bo[j];
            }
        }
        /* no barrier here: the next tile writes sdest / sray before its first barrier (last read above the second), the records behind it */
    }
}

/* passes 1 and 2 on `stream`: the rays of the plan's dump (fp64, org and dir on 16-byte boundaries, a 6-bit key) -> their ordered copy, dest[] and slot[] in the workspace */
int lh_order_run(const lh_order_plan_t *p, const lh_order_grid_t *g, const void *d_org, const void *d_dir, void *d_ws, hipStream_t stream)
{
    if (!p || p->n == 0 || p->n > ((size_t)1 << 30) || p->nbins != ORD_NB || p->block != LH_ORDER_BLOCK || (((uintptr_t)d_org | (uintptr_t)d_dir) & 15u)) return -1;
    char *ws = (char *)d_ws;
    const OrdRays a = {(const char *)d_org, (const char *)d_dir, p->n, *g};
    uint32_t *counts = (uint32_t *)(ws + p->counts), *offset = (uint32_t *)(ws + p->offset), *bintotal = (uint32_t *)(ws + p->bintotal), *binbase = (uint32_t *)(ws + p->binbase);
    if (g->octant) hipLaunchKernelGGL(k_order_count<true>, dim3(p->nblocks), dim3(ORD_T), 0, stream, a, counts);
    else hipLaunchKernelGGL(k_order_count<false>, dim3(p->nblocks), dim3(ORD_T), 0, stream, a, counts);
    hipLaunchKernelGGL(k_order_scan_blocks, dim3(ORD_NB), dim3(ORD_T), 0, stream, counts, offset, bintotal, p->nblocks);
    hipLaunchKernelGGL(k_order_scan_bins, dim3(1), dim3(ORD_NB), 0, stream, bintotal, binbase);
    hipLaunchKernelGGL(k_order_copy, dim3(p->nblocks), dim3(ORD_T), 0, stream, a, offset, binbase, (double *)(ws + p->org), (double *)(ws + p->dir), (uint32_t *)(ws + p->dest),
                       (uint16_t *)(ws + p->slot));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* pass 3 on `stream`: the records of the ordered copy -> the caller's arrays (closest hit: prim, t, u, v; any hit: occ) */
int lh_order_back(const lh_order_plan_t *p, int closest, const void *d_ws, void *d_prim, void *d_t, void *d_u, void *d_v, void *d_occ, hipStream_t stream)
{
    const char *ws = (const char *)d_ws;
    const uint32_t *dest = (const uint32_t *)(ws + p->dest);
    const uint16_t *slots = (const uint16_t *)(ws + p->slot);
    if (closest)
        hipLaunchKernelGGL(k_order_back<true>, dim3(p->nblocks), dim3(ORD_T), 0, stream, p->n, dest, slots, (const uint32_t *)(ws + p->prim), (const double *)(ws + p->t),
                           (const double *)(ws + p->u), (const double *)(ws + p->v), (const uint8_t *)NULL, (uint32_t *)d_prim, (double *)d_t, (double *)d_u, (double *)d_v, (uint8_t *)NULL);
    else
        hipLaunchKernelGGL(k_order_back<false>, dim3(p->nblocks), dim3(ORD_T), 0, stream, p->n, dest, slots, (const uint32_t *)NULL, (const double *)NULL, (const double *)NULL,
                           (const double *)NULL, (const uint8_t *)(ws + p->occ), (uint32_t *)NULL, (double *)NULL, (double *)NULL, (double *)NULL, (uint8_t *)d_occ);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
