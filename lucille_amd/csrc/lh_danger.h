/*
 * lh_danger.h -- the pure arithmetic of the per-ray routing decision around zero-area triangles that stay in the traversal
 * tree (lh_bvh.h deg_dcap / danger, lh_walk.h ray_needs_ref_walk, lh_hostwalk.c lh_danger_hit): what the device compares a
 * ray's largest direction component with, which ray sources take that test at all, and the ONE box on the scene's 16-bit grid
 * the device asks.  The argument needs the routed rays to be a SUPERSET of the rays on which the reference can report such a
 * triangle, so every rounding here goes to the side that routes more.  Host code only (lh_commit.hip calls it at commit);
 * plain C so that tests/cpu_model links the same functions (tests/test_danger_routing_model.py).
 */
#ifndef LH_DANGER_H
#define LH_DANGER_H

#include <math.h>
#include <stdint.h>

#include "lh_bvh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lh_hostwalk.c: does the ray hit one of the first nd boxes of b->danger?  (a superset of the reference's test_ray_aabb) */
int lh_danger_hit(const lh_bvh_t *b, uint32_t nd, const double o[3], const double d[3]);

#ifdef __cplusplus
}
#endif

/* the cap the device holds (lh_dev_scene_t.deg_dcap, a float): the double cap rounded TOWARD ZERO, so that a ray the host walk
 * routes (D > cap, in double) is routed on the device as well (D > (double)float cap).  Rounded to nearest it was above the
 * double for half of all caps -- 1 / 3 became 0.3333333432674408 -- and the rays in between walked the traversal tree on the
 * device only.  INFINITY (no cap) stays INFINITY. */
static inline float lh_dcap_device(double cap)
{
    float f;
    if (!(cap < 3.0e38)) return INFINITY;
    f = (float)cap;
    if ((double)f > cap) f = nextafterf(f, 0.0f);
    return f;
}

/* lh_dev_scene_t.cap_srcs from the double cap: bit 0 (rays from arrays: any direction) it is finite; bits 1 and 2 (AO rays,
 * camera rays: unit vectors) a unit vector can exceed it -- a normalised direction's largest component is 1 up to a few
 * roundings, hence below 1 + 4 x 2^-52 and not below 1: a cap in [1 - 2^-25, 1) used to round to 1.0f and switched the test
 * off for them */
static inline uint32_t lh_dcap_srcs(double cap)
{
    return (cap < 3.0e38 ? 1u : 0u) | (cap < 1.0 + 4.0 * 2.220446049250313e-16 ? 6u : 0u);
}

/* the union box u (bmin xyz, bmax xyz) of the listed leaves' boxes on the grid (glo, gstep), a cell wider on every side, in
 * the nodes' packing (lo | hi << 16 per axis).  Returns 1 and w[3], with glo + lo * gstep <= u_lo and glo + hi * gstep >= u_hi
 * on every axis (in double) -- or 0: the box is not inside the grid (or not a number), every ray beyond the cap takes the
 * reference walk (LH_DANGER_ALL).  The boxes are those of lucille's own tree, which keeps the triangles the traversal tree
 * drops (two equal vertices: lh_bvh.c tri_dead_class), and the grid covers the traversal tree's triangles only: a dropped
 * triangle outside the others' bounds takes its leaf's box out of the grid.  Such a box used to be accepted up to a cell
 * outside and then clamped to the grid: the strip between the grid and the box's face belonged to the reference's box and
 * not to the device's, and a ray through it that the reference reports on the zero-area triangle walked the traversal tree,
 * which holds nothing out there. */
static inline int lh_danger_pack(const double u[6], const float glo[3], const float gstep[3], uint32_t w[3])
{
    int k;
    for (k = 0; k < 3; k++) {
        const double g0 = (double)glo[k], st = (double)gstep[k];
        double qlo, qhi;
        if (!(st > 0.0) || !(u[k] <= u[3 + k])) return 0;
        if (!(u[k] >= g0) || !(u[3 + k] <= g0 + 65535.0 * st)) return 0;          /* (also a NaN) */
        qlo = floor((u[k] - g0) / st) - 1.0; qhi = ceil((u[3 + k] - g0) / st) + 1.0;
        if (qlo < 0.0) qlo = 0.0;
        if (qhi > 65535.0) qhi = 65535.0;
        w[k] = (uint32_t)qlo | (uint32_t)qhi << 16;
    }
    return 1;
}

#endif
