/*
 * lh_plan.h -- the geometry of a persistent launch, stated once: LDS stack rows, whether pushes are checked, how much of the top of the
 * tree a workgroup copies into LDS, how many workgroups a CU holds, which launches run the cooperative walk beside them, the cursor
 * chunk.  Plain C without HIP: the launchers (lh_kernels.hip), the grid's size (lh_commit.hip size_grid) and a stand-alone checker
 * (tests/cpu_model/lh_plan_check.c, tests/test_launch_plan.py) read the same rules.
 */
#ifndef LH_PLAN_H
#define LH_PLAN_H

#include "lh_device.h"

/* the walks of a batch's main kernel; template arguments of the kernels (part of their names): the values stay */
enum { LH_WALK_DIRECT = 0,          /* the textbook walk over the 2-wide fp32 nodes */
       LH_WALK_Q4 = 3,              /* the 4-wide nodes (the default) */
       LH_WALK_Q8 = 7,              /* the 8-wide nodes */
       LH_WALK_Q4_CHECKED = 8 };    /* the 4-wide nodes with a check before every push */

/* what is launched: a batch of rays (lh_launch_trace: the walk follows `variant` and the scene), or a fused stage whose rays are made in the kernel */
enum { LH_PLAN_BATCH = 0, LH_PLAN_AO = 1, LH_PLAN_DIRT = 2 };

/* what a launcher refuses */
enum { LH_PLAN_OK = 0,
       LH_PLAN_ERR_ROWS = 1,        /* the walk asks for more than LH_ROWS_UNCHECKED rows (a textbook walk over a tree deeper than 62 levels) */
       LH_PLAN_ERR_COOP = 2 };      /* the cooperative walk runs beside the launch and its ring would exceed LH_COOP_RING_MAX rows */

#define LH_DENSE_RAYS     65536u    /* rays from which a launch counts as filling the chip ("dense": checked rows, a fix-up queue and the cooperative walk beside it) */
#define LH_CU_LDS_BYTES   (160u * 1024u)    /* a CU's LDS */
#define LH_WG_LDS_BYTES   (64u * 1024u)     /* a workgroup's LDS up to which a CU holds what its size allows (LH_ROWS_UNCHECKED, lh_device.h) */
#define LH_ROW_BYTES      (LH_BLOCK * (uint32_t)sizeof(int))    /* one stack row of a 256-thread workgroup: 1 KiB */
#define LH_WGS_PER_CU_MAX 4u        /* 128 VGPRs: four workgroups per CU at most */
#define LH_COOP_RING_MAX  512u      /* the cooperative walk's ring at most */

typedef struct lh_plan {
    int      walk;                  /* LH_WALK_* */
    uint32_t rows;                  /* LDS stack rows (lh_dev_scene_t.stack_rows) */
    int      guard;                 /* the rows do not cover the tree's worst case: the walk checks before it pushes (stack_guard) */
    uint32_t top_nodes;             /* 4-wide nodes of the top of the tree copied into LDS behind the rows */
    size_t   lds_bytes;             /* dynamic LDS of the main kernel: rows + top_nodes */
    uint32_t wgs_per_cu;            /* workgroups per CU the top-of-tree rule counted on */
    uint32_t ray_chunk;             /* rays per cursor atomic, after the clamp */
    int      coop;                  /* the fix-up queue takes rays and the cooperative walk runs beside the launch */
    uint32_t ray_budget;            /* the visit budget: the scene's, or none where no queue takes the rays */
    uint32_t coop_rows;             /* the cooperative walk's ring (0: deeper than any ring) ... */
    size_t   coop_lds_bytes;        /* ... and its dynamic LDS */
    int      err;                   /* LH_PLAN_OK, or why the launch is refused */
} lh_plan_t;

/* persistent workgroups a CU holds beside each other: as many as their LDS stack rows let it -- at most 4: the walk's 128 VGPRs */
static inline uint32_t lh_plan_wgs_per_cu(uint32_t rows)
{
    const uint32_t wgs = rows ? LH_CU_LDS_BYTES / (rows * LH_ROW_BYTES) : LH_WGS_PER_CU_MAX;
    return wgs > LH_WGS_PER_CU_MAX ? LH_WGS_PER_CU_MAX : wgs;
}

/* LDS stack rows of a 4-wide walk over this scene.  3 * depth + 5 (or the builder's count of the deepest path) covers every
 * ray, but a launch that fills the chip is bound by rays in flight, and 128 VGPRs allow FOUR workgroups per CU: so a big launch
 * (`dense`) walks at most LH_ROWS_CHECKED rows -- four workgroups and the cooperative walk's in a CU's 160 KiB -- with a check
 * before every push, and the rare ray that would overrun its column goes to the cooperative walk.  Config-5 frame (the tree
 * asks for 59 rows: two workgroups per CU): 85.6 ms unchecked, 61.9 at 34 checked rows; S-soup-1M dump (44 rows: three) 2 234 ->
 * 2 278 Mrays/s.  (Rounds 2-3 measured the opposite for the frame -- 91 against 87 ms -- because the cooperative pass beside
 * the launch, which cannot be resident next to four 128-VGPR workgroups, kept its share of the queue after the launch had ended:
 * k_coop_walk.)  Small batches keep unchecked rows (up to 64): a handful of waves fills nothing, and without a queue an
 * overrunning ray would be left to k_fixups' sequential walk.  "stack_cap" forces a cap (8 .. 64). */
static inline uint32_t lh_plan_rows4(const lh_dev_scene_t *sc, int dense, int *guard)
{
    uint32_t need = sc->q4_stack ? sc->q4_stack : 3 * sc->q4_depth + 5;      /* the builder's own count of the deepest path, or the bound of any tree that deep */
    const uint32_t cap = (sc->stack_cap >= 8 && sc->stack_cap <= LH_ROWS_UNCHECKED) ? sc->stack_cap
                       : ((dense || need > LH_ROWS_UNCHECKED) ? LH_ROWS_CHECKED : LH_ROWS_UNCHECKED);
    *guard = need > cap;
    if (need > cap) need = cap;
    need = (need + 1u) & ~1u;
    if (need < 16 && !*guard) need = 16;
    return need;
}

/* the 8-wide walk pushes up to 7 per level and keeps a scratch row; beyond 48 rows (three workgroups per CU) the rare
 * ray that needs them is finished by the cooperative walk over the 4-wide nodes (always resident) */
static inline uint32_t lh_plan_rows8(const lh_dev_scene_t *sc, int *guard)
{
    uint32_t need = 7 * sc->q8_depth + 10;
    const uint32_t cap = (sc->stack_cap >= 16 && sc->stack_cap < 64) ? sc->stack_cap : 48;
    *guard = need > cap;
    if (need > cap) need = cap;
    need = (need + 1u) & ~1u;
    if (need < 16 && !*guard) need = 16;
    return need;
}

/* the textbook walk, 2-wide: one push per level + the sentinel */
static inline uint32_t lh_plan_rows_direct(const lh_dev_scene_t *sc)
{
    uint32_t need = sc->max_depth + 2;
    need = (need + 1u) & ~1u;
    return need < 16 ? 16 : need;
}

/* LDS stack rows the default walk launches with on this scene when the launch fills the chip: what sizes the grid */
static inline uint32_t lh_plan_trace_rows(const lh_dev_scene_t *sc)
{
    int guard;
    return lh_plan_rows4(sc, 1, &guard);
}

/* the cooperative walk's ring of stack rows: a power of two covering the tree's worst case (3 per level + sentinel + the
 * step's scratch slots); 0: the tree is deeper than any builder hands over */
static inline uint32_t lh_plan_coop_rows(const lh_dev_scene_t *sc)
{
    const uint32_t need = 3 * sc->q4_depth + 6;
    uint32_t r = 16;
    while (r < need) r <<= 1;
    return r <= LH_COOP_RING_MAX ? r : 0;
}

/* the cooperative walk's dynamic LDS: the stack ring, 2 x 64 exchange words, 4 x 16 stashed reference-walk entries */
static inline size_t lh_plan_coop_lds(uint32_t coop_rows)
{
    return ((size_t)coop_rows * 64 + 128 + 64) * sizeof(int);
}

/* nodes of the top of the tree a workgroup keeps in LDS behind its `rows` stack rows (node_step4): what the CU's 160 KiB leave
 * over once the workgroups its stack rows allow are resident -- never a workgroup fewer for it.  Measured (tools/top_probe.py,
 * r04): S-soup-1M 2 228 -> 2 249 Mrays/s on the host builder's tree, 2 212 -> 2 233 on the device builder's (144 nodes = 6.3 of a
 * ray's 42.5 node visits), config-5 AO frame 86.8 -> 86.2 ms: the requests that leave the CU for the hot top levels are not what
 * bounds the walk (profiles/README.md r04), so the gain is small; it is free.  sc.top_nodes: LH_TOP_AUTO, 0 (off), or a count. */
static inline uint32_t lh_plan_top_nodes(const lh_dev_scene_t *sc, uint32_t rows)
{
    uint32_t want = sc->top_nodes;
    if (want == 0u) return 0u;
    /* the CU's 160 KiB also hold the workgroup of the cooperative walk that runs NEXT TO this launch (k_coop_walk: one wave,
     * a ring of coop_rows x 64 entries): its stream has the higher priority, so it is placed first -- a persistent workgroup
     * that no longer fits beside it is one workgroup per CU fewer for the whole launch (r04: 2 240 -> 1 680 Mrays/s, the
     * config-5 frame 85 -> 128 ms with every spare byte given to the top of the tree).  A count set by the caller is held to
     * the same room (512 nodes beside 34 dense rows made 4 x 43 KiB and silently dropped a workgroup per CU) */
    const uint32_t crows = lh_plan_coop_rows(sc);
    const uint32_t coop = crows ? (uint32_t)lh_plan_coop_lds(crows) + 768u : 0u;      /* its workgroup's LDS and 768 bytes (its ring, its exchange words and a KiB); no ring: no cooperative walk */
    const uint32_t cu = LH_CU_LDS_BYTES - coop, stack = rows * LH_ROW_BYTES;
    const uint32_t wgs = lh_plan_wgs_per_cu(rows);      /* what size_grid() launches per CU: the same function */
    if (wgs == 0u || cu < wgs * stack) return 0u;
    uint32_t spare = (cu / wgs - stack) / 64u;
    /* a workgroup above 64 KiB of LDS halves what a CU holds (lh_device.h): the copy never takes a launch across that line (the
     * small launches' up to 64 unchecked rows are 64 KiB by themselves: no copy there) */
    if (stack <= LH_WG_LDS_BYTES) { const uint32_t room = (LH_WG_LDS_BYTES - stack) / 64u; if (spare > room) spare = room; }
    if (spare > LH_TOP_NODES_MAX) spare = LH_TOP_NODES_MAX;
    if (want == LH_TOP_AUTO || want > spare) want = spare;
    want &= ~15u;
    return want < sc->nq4nodes ? want : sc->nq4nodes;
}

/* rays per cursor atomic: the scene's setting, but never so large that a wave gets fewer than
 * ~4 ranges of a small batch (tail imbalance: late path-tracing bounces, small tiles) */
static inline uint32_t lh_plan_chunk(uint32_t ray_chunk, size_t n, int grid_blocks)
{
    const size_t waves = (size_t)(grid_blocks > 0 ? grid_blocks : 1) * (LH_BLOCK / 64);
    size_t c = n / (waves * 4);
    if (c < 64) c = 64;
    if (c < ray_chunk) ray_chunk = (uint32_t)c;
    return ray_chunk ? ray_chunk : 64;
}

/* the plan of one persistent launch of n rays over the launch's scene copy (its ray_chunk: the chunk before the clamp).  kind LH_PLAN_BATCH: a batch
 * of rays through `variant` (lh_launch_trace), have_queue: the launch has a fix-up queue; LH_PLAN_AO / LH_PLAN_DIRT: the fused stages (always the
 * 4-wide nodes, always a queue) */
static inline lh_plan_t lh_plan_launch(const lh_dev_scene_t *sc, size_t n, int kind, int variant, int grid_blocks, int have_queue)
{
    lh_plan_t p;
    int guard = 0;
    p.err = LH_PLAN_OK;
    p.ray_budget = sc->ray_budget;
    if (kind != LH_PLAN_BATCH) {
        p.rows = lh_plan_rows4(sc, n >= LH_DENSE_RAYS, &guard);
        p.walk = guard ? LH_WALK_Q4_CHECKED : LH_WALK_Q4;
        p.coop = 1;
    } else {
        if (variant == LH_VARIANT_DIRECT) {
            p.rows = lh_plan_rows_direct(sc); p.walk = LH_WALK_DIRECT;
        } else if (sc->prefer_q8 && sc->q8nodes) {
            p.rows = lh_plan_rows8(sc, &guard); p.walk = LH_WALK_Q8;
        } else {
            /* a launch that fills the chip walks at most LH_ROWS_CHECKED rows (four workgroups per CU), a ray that would overrun
             * them is finished by the cooperative walk; so does a very deep tree (chains of nested geometry, an LBVH over a
             * degenerate distribution) whose worst case does not fit 64 rows -- lh_plan_rows4 */
            p.rows = lh_plan_rows4(sc, n >= LH_DENSE_RAYS || sc->n_dev != NULL, &guard);
            p.walk = guard ? LH_WALK_Q4_CHECKED : LH_WALK_Q4;
        }
        /* small batches (one synchronous ray, a bucket of lucille's renderer): no visit budget, no second stream -- a ray the walk
         * cannot finish (LDS rows) stays flagged for k_fixups */
        p.coop = p.walk != LH_WALK_DIRECT && have_queue && (n >= LH_DENSE_RAYS || sc->n_dev != NULL);
        if (!p.coop) p.ray_budget = 0xFFFFFFFFu;
    }
    p.guard = guard;
    if (p.rows > LH_ROWS_UNCHECKED) p.err = LH_PLAN_ERR_ROWS;
    p.wgs_per_cu = lh_plan_wgs_per_cu(p.rows);
    p.top_nodes = (p.walk == LH_WALK_DIRECT || p.walk == LH_WALK_Q8) ? 0u : lh_plan_top_nodes(sc, p.rows);
    p.lds_bytes = (size_t)p.rows * LH_ROW_BYTES + (size_t)p.top_nodes * 64u;
    p.ray_chunk = lh_plan_chunk(sc->ray_chunk, n, grid_blocks);
    p.coop_rows = lh_plan_coop_rows(sc);
    p.coop_lds_bytes = lh_plan_coop_lds(p.coop_rows);
    if (p.coop && p.coop_rows == 0 && p.err == LH_PLAN_OK) p.err = LH_PLAN_ERR_COOP;
    return p;
}

#endif
