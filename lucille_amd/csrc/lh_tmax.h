/*
 * lh_tmax.h -- the scalar pieces of the per-ray maximum distance (lh_accel_intersect_device_tmax / _host_tmax), one statement of
 * the rule for the kernels (lh_walk.h, lh_kernels.hip), the host walk (lh_hostwalk.c) and the test that checks it without a GPU
 * (tests/test_tmax_rule.py).
 *
 * The contract: the answer of a bounded ray is the unbounded call's record R if R is a hit and R.t < tmax (fp64, strict), else a
 * miss.  A bound IS a double (an fp32 bound, widened).  The walk prunes with an fp32 bound that can only over-accept, the fp64
 * resolve accepts exactly t < tmax, and an accepted hit close enough to the bound that a partner beyond it may have gone unseen is
 * sent to the reference's own (unbounded) walk, whose record is filtered with the same comparison.  DESIGN.md has the argument.
 */
#ifndef LH_TMAX_H
#define LH_TMAX_H

#include <stdint.h>

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

#define LH_TMAX_T_INF      1.0e38        /* RI_INFINITY: the t of a miss record, and the bound of an unbounded ray */
#define LH_TMAX_TB_MAX     1.0e38f       /* the walk's culling bound without a per-ray bound (lane_init) */
#define LH_TMAX_TB_MIN     1.17549435e-38f   /* the smallest normal float: a culling bound is never a denormal (a flushed one would be 0) */
#define LH_TMAX_SURE_MIN   1.0e-30f      /* below it a certain fp32 hit never ends an any-hit ray: the fp64 test decides */
#define LH_TMAX_SURE_K     0.99999976158142089844f       /* 1 - 2^-22 */
#define LH_TMAX_NEAR_REL   2.0e-10       /* 2 x LH_FRAGILE_REL (lh_reftrace.h) */

/* a bound no t can satisfy: NaN, zero (either sign) and negatives.  Such a ray misses */
LH_HD int lh_tmax_dead(double tmax) { return !(tmax > 0.0); }

/* the fp32 culling bound of a live bound: tmax rounded UP to a float, never below the smallest normal, never above 1e38f (the bound every
 * unbounded walk starts with) -- as a real number >= min(tmax, 1e38f), so the slab tests and the triangle filter, which reject against
 * it, can only over-accept.  A dead bound: -1, which every slab test and every triangle fails (lh_walk.h LH_FORCE_REF_WALK's trick) */
LH_HD float lh_tmax_tb(double tmax)
{
    union { float f; uint32_t w; } c;
    if (lh_tmax_dead(tmax)) return -1.0f;
    if (!(tmax < (double)LH_TMAX_TB_MAX)) return LH_TMAX_TB_MAX;
    c.f = (float)tmax;                                   /* round to nearest; positive, finite, below 1e38f + an ulp */
    if ((double)c.f < tmax) c.w += 1u;                   /* the next float up (c.f >= +0) */
    if (c.f < LH_TMAX_TB_MIN) c.f = LH_TMAX_TB_MIN;
    if (c.f > LH_TMAX_TB_MAX) c.f = LH_TMAX_TB_MAX;
    return c.f;
}

/* what best.t starts at instead of LH_T_INF: resolve()'s strict `t < best.t` then accepts exactly the hits with t < tmax */
LH_HD double lh_tmax_best0(double tmax) { return (tmax < LH_TMAX_T_INF) ? tmax : LH_TMAX_T_INF; }

/* any hit: a CERTAIN fp32 hit whose t is at most t_hi ends the ray only below this threshold, which is below tmax for every
 * live bound: tb = lh_tmax_tb(tmax) is either clamped (tb <= tmax) or the float next above tmax, tb <= tmax (1 + 2^-23) for normal tb;
 * tb (1 - 2^-22) rounded is at most tb (1 - 2^-22)(1 + 2^-24) < tb (1 - 2^-23) <= tmax.  Below 1e-30f (where tb may be the clamp to
 * the smallest normal, above tmax) and for a dead bound: -1, no certain hit ends the ray */
LH_HD float lh_tmax_sure_below(float tb) { return (tb >= LH_TMAX_SURE_MIN) ? tb * LH_TMAX_SURE_K : -1.0f; }

/* an accepted hit at t so close below the bound that a second triangle within LH_FRAGILE_REL of it may lie at or beyond tmax, where
 * the bounded walk does not take it and resolve() cannot mark the pair: such a hit is marked fragile (bit 1) at retire.  Below the
 * threshold every partner within LH_FRAGILE_REL (|t' - t| <= 1e-10 max(t, t')) lies below tmax and is seen as in the unbounded walk */
LH_HD int lh_tmax_near(double t, double tmax) { return t >= tmax * (1.0 - LH_TMAX_NEAR_REL); }

/* the final accept, applied to the reference walk's (unbounded) record as well: strict, false for a NaN bound */
LH_HD int lh_tmax_accept(double t, double tmax) { return t < tmax; }

#endif
