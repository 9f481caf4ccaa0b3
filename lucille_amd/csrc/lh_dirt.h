/*
 * lh_dirt.h -- the rule of the dirtmap transport (ri_transport_dirtmap, src/transport/dirtmap.c:84-292), one statement of it for the
 * resolve kernels (lh_render.hip), the entry points (lh_tile.hip) and the test that checks it without a GPU (tests/test_dirt_rule.py).
 *
 * Dirtmap is ambient occlusion with a range: the same stratified cosine hemisphere about Ns, the origin P + eps Ns (eps = 1e-5,
 * dirtmap.c:98), the CLOSEST hit of every gather ray, weighted by where it lies between a near and a far clip (:110-111); beyond the far
 * clip a hit counts as no hit.  A gather ray's input here is one double: the t of its bounded closest-hit record with tmax = far_clip
 * (lh_tmax.h) -- the unbounded record's t if that is a hit with t < far_clip (fp64, strict), else the miss record's 1e38.
 *
 * The reference hard-codes base colour 1, dirt colour 0 and dirt_gain 1: pow(x, 1.0f / 1.0) is x and (1 - p) * 1 - p * 0 is 1 - p, so
 * neither pow nor a gain appears below.  Every operation is a single fp64 add, subtract or divide in the order written: there is no
 * product feeding a sum, hence nothing a compiler could contract.
 *
 * DESIGN.md 10.0b has the stage built on it; tests/test_gpu_dirt.py pins it to the oracle.
 */
#ifndef LH_DIRT_H
#define LH_DIRT_H

#include <stdint.h>

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

#define LH_DIRT_NEAR_DEFAULT 0.1         /* dirtmap.c:110 */
#define LH_DIRT_FAR_DEFAULT  0.5         /* :111 */
#define LH_DIRT_EPS_DEFAULT  1.0e-5      /* :98 */
#define LH_DIRT_FAR_MAX      1.0e38      /* RI_INFINITY: the t of a miss record; a far clip there bounds nothing */
#define LH_DIRT_SELF_EPS     1.0e-6      /* the smallest offset lh_ao.h's argument for the self-primitive skip covers */

/* accepted: all finite, 0 <= near_clip < far_clip <= 1e38, eps >= 0.  Everything else (NaN included: every comparison with it is
 * false; x - x is 0 for finite x alone) is refused */
LH_HD int lh_dirt_params_ok(double near_clip, double far_clip, double eps)
{
    if (!(near_clip >= 0.0 && near_clip < far_clip && far_clip <= LH_DIRT_FAR_MAX)) return 0;
    if (!(eps >= 0.0 && eps - eps == 0.0)) return 0;
    return 1;
}

/* the slot key's self-primitive skip (lh_ao.h) rests on the size of the offset: only from AO's 1e-6 on */
LH_HD int lh_dirt_selfskip(double eps) { return eps >= LH_DIRT_SELF_EPS; }

/* is the bounded record whose t this is a hit?  (a miss record carries 1e38 >= every accepted far clip) */
LH_HD int lh_dirt_hit(double t, double far_clip) { return t < far_clip; }

/* the weight of one gather ray (dirtmap.c:186-212 with mix_color :70-82): 1 for a miss, 0 up to the near clip, then the hit's place
 * between the clips */
LH_HD double lh_dirt_weight(double t, double near_clip, double far_clip)
{
    double a, b, q, x, p;
    if (!lh_dirt_hit(t, far_clip)) return 1.0;
    if (t <= near_clip) return 0.0;
    a = t - near_clip; b = far_clip - near_clip; q = a / b; x = 1.0 - q;
    p = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    return 1.0 - p;
}

/* the value of one hit from the N doubles of its gather rays, r = j * ntheta + i ascending (the loop order of dirtmap.c:146-147):
 * sum / N in fp64; *near_hits: how many of the N bounded records are hits.  The order is part of the contract */
LH_HD double lh_dirt_value(const double *t, int N, double near_clip, double far_clip, uint32_t *near_hits)
{
    double sum = 0.0;
    uint32_t nh = 0u;
    int r;
    for (r = 0; r < N; r++) {
        const double tr = t[r];
        if (lh_dirt_hit(tr, far_clip)) nh++;
        sum = sum + lh_dirt_weight(tr, near_clip, far_clip);
    }
    *near_hits = nh;
    return sum / (double)N;
}

#endif
