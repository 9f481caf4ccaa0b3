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
 * Area lights (lh_area.h) at the path vertices.  A pass may carry a list of area lights beside, or instead of, the delta lights.  The area value of a
 * hit of bounce d is exactly what lh_accel_area_lights_device answers for that hit record, the call's area list and parameters, the seed
 * lh_ptl_area_seed(seed, d), the entry's key and no replayed uniforms; lh_area.h is unchanged -- origin P + eps Ns, no self-primitive skip, the
 * bound, the order of lights and samples.
 *
 *   key    the path is sample s of frame pixel (px, py) -- what pt_pixel (lh_pt.h) gives, frame coordinates, so tiles and bands agree:
 *          lh_ptl_area_key = ((uint64)py * width + px) * spp_total + (spp_begin + s), width the frame's.  The generator reads the low 34 bits of
 *          a key: a pass with area lights is refused unless width x height x spp_total <= 2^34 (lh_ptl_area_keys_ok, no product overflows);
 *   seed   lh_ptl_area_seed(seed, d) = seed + (uint64)(d + 1) * 0xD1B54A32D192ED03 modulo 2^64.  The bounce goes into the seed, not the key --
 *          34 bits do not hold pixel x sample x bounce, and the stage runs once per bounce anyway.  The path's own draws (pt_key) use `seed`
 *          itself: the streams differ;
 *   value  there is still ONE term per hit, r_k = ((G_k * kd_k) * col_k) * value_k.  With one kind of light value is that stage's three floats and
 *          nothing is added to them; with both, value_k = delta_k + area_k, one float32 add (lh_ptl_value).
 *
 * One term per entry: a pixel's sums take spp_count x (max_path_vertices - 1) <= 4096 terms of a pass with either kind of light.
 *
 * The kernels are compiled with -ffp-contract=off, a host program that includes this file must be too.
 */
#ifndef LH_PTL_H
#define LH_PTL_H

#include <stdint.h>

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

/* the key of an entry for the area stage's generator: sample spp_begin + s of frame pixel (px, py) of a frame `width` wide */
LH_HD uint64_t lh_ptl_area_key(int px, int py, int width, int spp_total, int spp_begin, int s)
{
    return ((uint64_t)py * (uint64_t)width + (uint64_t)px) * (uint64_t)spp_total + (uint64_t)(spp_begin + s);
}

/* the area stage's seed at bounce d (0-based) */
LH_HD uint64_t lh_ptl_area_seed(uint64_t seed, int d)
{
    return seed + (uint64_t)(d + 1) * 0xD1B54A32D192ED03ull;
}

/* one channel of `value` where a pass has both kinds of light */
LH_HD float lh_ptl_value(float delta, float area)
{
    return delta + area;
}

/* do the keys of every sample of the frame fit the generator's 34 bits?  width x height x spp_total <= 2^34, no product overflowing */
LH_HD int lh_ptl_area_keys_ok(int width, int height, int spp_total)
{
    const uint64_t keys = (uint64_t)1 << 34;
    if (width < 1 || height < 1 || spp_total < 1) return 0;
    const uint64_t pixels = (uint64_t)width * (uint64_t)height;          /* below 2^62 */
    return pixels <= keys && (uint64_t)spp_total <= keys / pixels;
}

#endif
