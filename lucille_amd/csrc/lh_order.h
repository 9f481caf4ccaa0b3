/*
 * lh_order.h -- the bin order of a ray dump (lh_order.hip): the key of a ray, the run table of a dump, the sizes of the workspace.
 * Plain C, host and device: the kernels, the host side and the CPU test (tests/test_order_key.py) read the same text.
 *
 * A large incoherent dump is traced from a copy in bin order (the key: the origin's cell on the scene's bounds, optionally under the direction octant), so that each XCD's L2 sees one region of the scene at a time, and its
 * records are copied back to the caller's slots.  Rays are binned in fixed blocks of consecutive rays with a stable partition: ray i of
 * block B with key k goes to
 *     dest[i] = offset[B][k] + (rays of block B before i that have key k)
 *     offset[B][k] = (rays of smaller keys in all blocks) + (rays of key k in earlier blocks)
 * which is the place a stable sort by key gives it -- and every (block, key) pair is one contiguous run of the ordered copy, on the
 * way in and on the way back.
 * The key, the block rule and the plan are defined here for keys of 3, 6 and 9 bits (8, 64, 512 bins; more bins grow the block), and the CPU test
 * checks them all; the device passes (lh_order.hip) are built for the 64-bin plans with blocks of LH_ORDER_BLOCK rays ALONE -- lh_order_run refuses
 * every other plan, and "dump_order_bits" accepts the two 6-bit keys only.  The key only decides order, never a record: every ray, NaN and infinite ones included, has a valid bin.
 */
#ifndef LH_ORDER_H
#define LH_ORDER_H

#include <stdint.h>
#include <stddef.h>
#include <string.h>

#if defined(__HIPCC__)
#define LH_ORDER_FN static inline __host__ __device__
#else
#define LH_ORDER_FN static inline
#endif

#define LH_ORDER_BLOCK     4096u       /* rays of a block at 64 bins or fewer */
#define LH_ORDER_MIN_RUN   48u         /* more bins: the block grows (by doubling) until an average run holds this many rays */
#define LH_DUMP_ORDER_BITS 2u          /* the default key ("dump_order_bits"; the device passes are built for 64 bins): 2 = the cell alone at two bits per axis -- what the
                                        * cost model of profiles/dump_order.md chose: it orders the walk nearly as well as the 9-bit keys, and pass 1 need not read dir;
                                        * 1 = one bit per axis under the direction octant */
#define LH_DUMP_ORDER_MIN  ((size_t)16000000)   /* the smallest dump that is ordered by default ("dump_order_min"; profiles/dump_order.md) */
#define LH_ORDER_ALIGN     256u        /* every array of the workspace starts on such a boundary */

/* the cells: `bits` bits per axis on the scene's bounds (grid_lo, grid_step of the device scene: the 16-bit grid of the nodes) */
typedef struct lh_order_grid { double lo[3], scale[3]; uint32_t bits, octant; } lh_order_grid_t;

LH_ORDER_FN lh_order_grid_t lh_order_grid(const float grid_lo[3], const float grid_step[3], uint32_t bits, uint32_t octant)
{
    lh_order_grid_t g; int k;
    g.bits = bits; g.octant = octant ? 1u : 0u;
    for (k = 0; k < 3; k++) { g.lo[k] = (double)grid_lo[k]; g.scale[k] = (double)(1u << bits) / (65535.0 * (double)grid_step[k]); }
    return g;
}

LH_ORDER_FN uint32_t lh_order_keybits(uint32_t bits, uint32_t octant) { return 3u * bits + (octant ? 3u : 0u); }
LH_ORDER_FN int      lh_order_valid(uint32_t bits, uint32_t octant) { const uint32_t kb = lh_order_keybits(bits, octant); return kb == 3u || kb == 6u || kb == 9u; }
LH_ORDER_FN uint32_t lh_order_nbins(uint32_t bits, uint32_t octant) { return 1u << lh_order_keybits(bits, octant); }

LH_ORDER_FN uint32_t lh_order_block(uint32_t bits, uint32_t octant)
{
    uint32_t b = LH_ORDER_BLOCK;
    while (b < LH_ORDER_MIN_RUN * lh_order_nbins(bits, octant)) b *= 2u;
    return b;
}

/* cell of one coordinate, clamped to [0, 2^bits - 1]; NaN -> 0.  The comparisons come first: a double is converted only when it lies in [0, 2^bits) */
LH_ORDER_FN uint32_t lh_order_cell(double x, double lo, double scale, uint32_t bits)
{
    const double f = (x - lo) * scale, top = (double)(1u << bits);
    if (!(f >= 0.0)) return 0u;
    if (f >= top) return (1u << bits) - 1u;
    return (uint32_t)f;
}

LH_ORDER_FN uint32_t lh_order_sign(double x)          /* the sign bit: -0.0 counts as negative, a NaN by its own bit */
{
    uint64_t w;
    memcpy(&w, &x, sizeof(w));
    return (uint32_t)(w >> 63);
}

/* the Morton code of the origin's cell, under the direction octant when the key has one */
LH_ORDER_FN uint32_t lh_order_key(const double org[3], const double dir[3], const lh_order_grid_t *g)
{
    const uint32_t cx = lh_order_cell(org[0], g->lo[0], g->scale[0], g->bits);
    const uint32_t cy = lh_order_cell(org[1], g->lo[1], g->scale[1], g->bits);
    const uint32_t cz = lh_order_cell(org[2], g->lo[2], g->scale[2], g->bits);
    const uint32_t octant = lh_order_sign(dir[0]) | (lh_order_sign(dir[1]) << 1) | (lh_order_sign(dir[2]) << 2);
    uint32_t m = 0u, b;
    for (b = 0; b < g->bits; b++)
        m |= (((cx >> b) & 1u) << (3u * b)) | (((cy >> b) & 1u) << (3u * b + 1u)) | (((cz >> b) & 1u) << (3u * b + 2u));
    return g->octant ? (octant << (3u * g->bits)) | m : m;
}

/* the workspace of one stream (lh_order.hip lh_order_run): byte offsets of its arrays and its size */
typedef struct lh_order_plan {
    size_t   n;
    uint32_t bits, octant, nbins, block, nblocks;
    size_t   org, dir, t, u, v, prim, occ, dest, slot, counts, offset, bintotal, binbase;      /* byte offsets; slot: a ray's place in its sorted tile (2 bytes), for the way back */
    size_t   bytes;
} lh_order_plan_t;

LH_ORDER_FN size_t lh_order_up(size_t x) { return (x + (LH_ORDER_ALIGN - 1u)) & ~(size_t)(LH_ORDER_ALIGN - 1u); }

/* n rays (1 .. 2^30), closest hit (prim, t, u, v: 28 bytes a ray) or any hit (a byte a ray) */
LH_ORDER_FN lh_order_plan_t lh_order_plan(size_t n, uint32_t bits, uint32_t octant, int closest)
{
    lh_order_plan_t p; size_t at = 0, table;
    p.n = n; p.bits = bits; p.octant = octant ? 1u : 0u; p.nbins = lh_order_nbins(bits, octant); p.block = lh_order_block(bits, octant);
    p.nblocks = (uint32_t)((n + p.block - 1u) / p.block);
    table = (size_t)p.nblocks * p.nbins * sizeof(uint32_t);
    p.org = at; at = lh_order_up(at + n * 24u);
    p.dir = at; at = lh_order_up(at + n * 24u);
    p.t = p.u = p.v = p.prim = p.occ = at;
    if (closest) {
        p.t = at; at = lh_order_up(at + n * 8u);
        p.u = at; at = lh_order_up(at + n * 8u);
        p.v = at; at = lh_order_up(at + n * 8u);
        p.prim = at; at = lh_order_up(at + n * 4u);
    } else {
        p.occ = at; at = lh_order_up(at + n);
    }
    p.dest = at; at = lh_order_up(at + n * 4u);
    p.slot = at; at = lh_order_up(at + n * 2u);
    p.counts = at; at = lh_order_up(at + table);
    p.offset = at; at = lh_order_up(at + table);
    p.bintotal = at; at = lh_order_up(at + p.nbins * sizeof(uint32_t));
    p.binbase = at; at = lh_order_up(at + p.nbins * sizeof(uint32_t));
    p.bytes = at;
    return p;
}

/* the run table in its defining order (the device computes the same numbers in parallel): counts[block][bin] -> offset[block][bin] */
LH_ORDER_FN void lh_order_offsets(const uint32_t *counts, uint32_t nblocks, uint32_t nbins, uint32_t *offset)
{
    uint32_t run = 0u, k, b;
    for (k = 0; k < nbins; k++)
        for (b = 0; b < nblocks; b++) { offset[(size_t)b * nbins + k] = run; run += counts[(size_t)b * nbins + k]; }
}

#if !defined(__HIPCC__)
/* the whole order on the host, as defined: keys -> counts -> offsets -> dest.  counts, offset: nblocks x nbins words; key (or NULL), dest: n words */
LH_ORDER_FN void lh_order_host(size_t n, const double *org, const double *dir, const lh_order_grid_t *g, uint32_t *key, uint32_t *counts,
                               uint32_t *offset, uint32_t *dest)
{
    const uint32_t nbins = lh_order_nbins(g->bits, g->octant), block = lh_order_block(g->bits, g->octant), nblocks = (uint32_t)((n + block - 1u) / block);
    size_t i;
    memset(counts, 0, (size_t)nblocks * nbins * sizeof(uint32_t));
    for (i = 0; i < n; i++) {
        const uint32_t k = lh_order_key(org + 3 * i, dir + 3 * i, g);
        if (key) key[i] = k;
        counts[(i / block) * nbins + k]++;
    }
    lh_order_offsets(counts, nblocks, nbins, offset);
    /* a block's rays in turn: `offset` of the block's row counts up as its rays are placed, and is restored afterwards */
    for (i = 0; i < n; i++) dest[i] = offset[(i / block) * nbins + lh_order_key(org + 3 * i, dir + 3 * i, g)]++;
    for (i = 0; i < (size_t)nblocks * nbins; i++) offset[i] -= counts[i];
}
#endif

#endif
