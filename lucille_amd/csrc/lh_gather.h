/*
 * lh_gather.h -- the gather stage's plan (lh_tile.hip ao_stage): which transport a stage runs, and whether it runs fused and late.  Plain C, no HIP:
 * read by lh_tile.hip, lh_device.h and lh_render.hip, and by tests/cpu_model/lh_gather_check.c (tests/test_gather_plan.py), as lh_plan.h is.
 *
 * fused: the gather rays are made inside the persistent kernel, nothing per ray goes through HBM but what the stage leaves (lh_launch_trace_gather).
 * late (with fused only): the hit count stays on the device, the buffers are sized for the worst case -- every sample / list entry hits -- and the
 * stage costs one host round trip, at its end.  fused and not late: the count is read first, it sizes the buffers and the launch.
 */
#ifndef LH_GATHER_H
#define LH_GATHER_H

#include <stddef.h>

/* what a stage leaves per gather ray, and so its kernels, scratch and resolve.  The sun-and-sky light is LH_GATHER_ENV with another light */
enum { LH_GATHER_AO = 0,          /* ambient occlusion: a count of occluded rays per hit slot (fused), a byte per ray (materialised) */
       LH_GATHER_DIRT = 1,        /* the dirtmap transport (lh_dirt.h): a double per ray, the t of its bounded closest hit */
       LH_GATHER_ENV = 2,         /* the environment-lit gather (lh_env.h): a byte per ray */
       LH_GATHER_LIGHT = 3,       /* direct light (lh_lights.h): N = the lights of the list, gather ray (slot, l) the shadow ray to light l; a byte per ray */
       LH_GATHER_AREA = 4,        /* area lights (lh_area.h): N = lights x samples, gather ray (slot, l, s) the shadow ray to a point drawn on light l's emitters; a byte per ray */
       LH_GATHER_KINDS = 5 };
/* who runs the stage: the tile pipeline (samples of a region) or a caller's batch of hit records (list entries) */
enum { LH_GATHER_TILE = 0, LH_GATHER_BATCH = 1 };

#define LH_SUN_LATE_MAX ((size_t)1 << 30)        /* slots up to which the sun's launch can take its count from the device (a list holds 2^30 entries) */
#define LH_ENV_LATE_MAX ((size_t)1 << 28)        /* gather rays (256 MiB of bytes) up to which a stage is sized for its worst case, the count left on the device */
#define LH_DIRT_CHUNK ((size_t)1 << 30)          /* rays of one bounded launch at most (a list holds 2^30 entries) */
#define LH_LIGHT_LATE_MAX ((size_t)1 << 28)      /* shadow rays (256 MiB of bytes) up to which a stage is sized for its worst case: the environment gather's cap, for the same byte per ray */
#define LH_DIRT_LATE_MAX ((size_t)1 << 27)       /* gather rays (1 GiB of t) up to which a stage is sized for its worst case, the count left on the device */

typedef struct lh_gather_plan { int fused, late; } lh_gather_plan_t;

/* entries: samples of the tile / entries of the list (every one may hit); N: gather rays per hit; ao_fused: set_param "ao_fused"; uniforms: the caller
 * replays its own random numbers; ao_group: set_param "ao_group", the grouped item order of the AO kernel; sun: the stage traces the sun's shadow
 * ray; sync: the caller asked for the count to be read first (LH_AO_SYNC, read per call where the tile is rendered) */
static inline lh_gather_plan_t lh_gather_plan(int kind, int where, size_t entries, size_t N, int ao_fused, int uniforms, int ao_group, int sun, int sync)
{
    const unsigned long long rays = (unsigned long long)entries * (unsigned long long)N;          /* the worst case */
    const int grouped = kind == LH_GATHER_AO && ao_group != 0;          /* the dirt, environment, light and area kernels have no grouped order */
    lh_gather_plan_t p;
    if (kind == LH_GATHER_LIGHT || kind == LH_GATHER_AREA) {
        /* no grouped order, no sun; a tile decides on the worst case as a batch does: entries x L (x S) < 2^31 (the 32-bit item index).  The light stage
         * draws nothing; replayed uniforms send the area stage to the ray kernel, which reads them from memory */
        p.fused = ao_fused && rays < (1ull << 31) && !(kind == LH_GATHER_AREA && uniforms);
        p.late = p.fused && rays <= LH_LIGHT_LATE_MAX && !(where == LH_GATHER_TILE && sync);
        return p;
    }
    p.fused = ao_fused && !uniforms;          /* replayed uniforms are read from memory by the ray kernel: materialised */
    if (where == LH_GATHER_BATCH) {
        /* a batch decides here, on the worst case; a tile that is not late reads the count and decides in the stage, on the hits it has */
        if (rays >= (1ull << 31)) p.fused = 0;          /* the persistent kernel's ray index has 32 bits */
        /* the grouped order needs the count on the host: a batch then runs materialised, a tile fused with the count read first (below) */
        if (grouped) p.fused = 0;
    }
    p.late = p.fused && rays < (1ull << 31);          /* the 32-bit ray index must cover the worst case */
    if (kind == LH_GATHER_DIRT && rays > LH_DIRT_LATE_MAX) p.late = 0;          /* a double per ray: the worst case is worth sizing for only while small */
    if (kind == LH_GATHER_ENV && rays > LH_ENV_LATE_MAX) p.late = 0;            /* a byte per ray: the same */
    if (grouped) p.late = 0;                                                     /* (a tile: see above) */
    if (sun && entries > LH_SUN_LATE_MAX) p.late = 0;                            /* the sun's launch is a list's: 2^30 entries */
    if (where == LH_GATHER_TILE && sync) p.late = 0;                             /* LH_AO_SYNC is the tile pipeline's knob: a batch does not consult it */
    return p;
}

#endif
