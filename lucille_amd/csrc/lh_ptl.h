/*
 * lh_ptl.h -- the rule of direct light at the path tracer's vertices: what a hit of a bounce adds to its pixel from the light list.  One statement
 * of it for the kernel that applies it (lh_render.hip k_pt_direct), the host loop around it (lh_tile.hip pt_tile) and the test that checks it
 * without a GPU (tests/test_ptl_rule.py).  Plain C.
 *
 * Bounce d (0-based) of a pass traces the ray that arrives at path vertex d + 2.  A hit is any entry of bounce d whose prim is not LH_MISS_PRIM:
 * its path may go on, be ended by the roulette, or end at the vertex limit -- all three are lit.  A hit adds, per channel k = 0, 1, 2,
 *
 *   r_k = ((G_k * kd_k) * col_k) * value_k          four float32 operands, three IEEE multiplies in this order, nothing contracted
 *
 *   G      the throughput the arriving ray carries: 1, 1, 1 for camera rays, thr[i] otherwise;
 *   kd     the diffuse reflectance of the hit's material (the override material, or the mesh's);
 *   col    the vertex colour as pt_scatter (lh_pt.h) computes it, (float)((c0 * w + c1 * u) + c2 * v) in fp64 with w = 1 - u - v, 1 where the
 *          mesh has no colours (lh_ptl_colour);
 *   value  the three floats lh_lights_value (lh_lights.h) gives for this hit record, the call's light list and eps: the light stage's contract,
 *          unchanged -- origin P + eps Ns with Ns as the hit epilogue leaves it, one bounded any-hit shadow ray per light.
 *
 * r goes into the pixel of the path through pt_accumulate (lh_render.hip): a channel that is NaN or 0 adds nothing, the clamp is pt_fix's.  The
 * environment is collected where it always was; the lights of the list are delta lights that no sampled direction finds: nothing is counted twice.
 *
 * No 1 / pi is applied (a caller folds it into the lights' colours), no specular or transmissive lobe is lit, and there is no self-primitive skip:
 * a light behind the surface is shadowed by the hit's own triangle, as in the light stage.
 *
 * The kernels are compiled with -ffp-contract=off, a host program that includes this file must be too.
 */
#ifndef LH_PTL_H
#define LH_PTL_H

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

/* one channel of a hit's direct light */
LH_HD float lh_ptl_direct(float G, float kd, float col, float value)
{
    const float a = G * kd;
    const float b = a * col;
    return b * value;
}

/* one channel of the vertex colour from the three corners' (pt_scatter's lines): w = 1.0 - u - v is the caller's */
LH_HD float lh_ptl_colour(double c0, double c1, double c2, double w, double u, double v)
{
    const double a = c0 * w, b = c1 * u, c = c2 * v;
    return (float)((a + b) + c);
}

#endif
