/*
 * lh_env.h -- the rule of the environment-lit gather (gather_sunsky's loop, src/transport/ambientocclusion.c:206-324, and
 * ri_ibl_sample_cosweight, src/render/ibl.c:52-227), one statement of it for the resolve kernels (lh_render.hip), the entry points
 * (lh_tile.hip) and the test that checks it without a GPU (tests/test_env_rule.py).
 *
 * The gather is ambient occlusion with a colour: the same stratified cosine hemisphere about Ns, the origin P + eps Ns (1e-5 in
 * gather_sunsky, 1e-4 in ibl.c), an ANY-hit answer per gather ray; a ray that is not occluded sees the environment in its direction
 * (ri_texture_ibl_fetch: env_fetch of lh_pt.h, constant white if the accelerator has none), an occluded ray sees nothing.  A gather
 * ray's input here is one byte (its any-hit answer) and three floats (the environment's colour in its direction).
 *
 * `scale` is the reference's m: 1 / M_PI in gather_sunsky (Lo = m * col / nsamples), pi * (1 / pi) = 1 in ri_ibl_sample_cosweight.
 * Every operation is a single fp64 add, multiply or divide in the order written; the one product feeds a quotient, not a sum: nothing a
 * compiler could contract.  The Preetham sky and the sun's shadow ray are another radiance source for the same sum: lh_sky.h states them (the sky's
 * colour of a direction, and the sun's term, which enters the sum after the N rays and before lh_env_finish); the sum itself stays here.
 *
 * DESIGN.md 10.0d has the stage built on it; tests/test_gpu_envgather.py pins it to the oracle.
 */
#ifndef LH_ENV_H
#define LH_ENV_H

#include <stdint.h>

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

#define LH_ENV_EPS_DEFAULT   1.0e-5      /* ambientocclusion.c:220 (ibl.c offsets by 1e-4) */
#define LH_ENV_SCALE_DEFAULT 1.0         /* ibl.c's pi * (1 / pi); gather_sunsky's is 0.3183098861837907 */
#define LH_ENV_SELF_EPS      1.0e-6      /* the smallest offset lh_ao.h's argument for the self-primitive skip covers (lh_dirt.h) */

/* accepted: both finite, eps >= 0, scale >= 0.  Everything else (NaN included: every comparison with it is false; x - x is 0 for
 * finite x alone) is refused */
LH_HD int lh_env_params_ok(double eps, double scale)
{
    if (!(eps >= 0.0 && eps - eps == 0.0)) return 0;
    if (!(scale >= 0.0 && scale - scale == 0.0)) return 0;
    return 1;
}

/* the slot key's self-primitive skip (lh_ao.h) rests on the size of the offset: only from AO's 1e-6 on (the compaction's one hit epilogue asks
 * lh_dirt_selfskip, the same threshold: LH_DIRT_SELF_EPS) */
LH_HD int lh_env_selfskip(double eps) { return eps >= LH_ENV_SELF_EPS; }

/* one unoccluded ray's colour channel into the running sum of its hit */
LH_HD double lh_env_add(double sum, float rad) { return sum + (double)rad; }

/* a channel of the hit's value from its sum over the N gather rays */
LH_HD float lh_env_finish(double scale, double sum, int N)
{
    const double m = scale * sum;
    return (float)(m / (double)N);
}

/* the value of one hit from the N bytes and the 3 N floats of its gather rays, r = j * ntheta + i ascending (the loop order of
 * ambientocclusion.c:251-252): per channel the sum of the unoccluded rays' colours, times scale, over N, in fp64, stored as float;
 * *count: how many of the N rays are occluded.  The order is part of the contract */
LH_HD void lh_env_value(const uint8_t *occ, const float *rad, int N, double scale, uint32_t *count, float value[3])
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    uint32_t c = 0u;
    int r;
    for (r = 0; r < N; r++) {
        if (occ[r]) { c++; continue; }
        s0 = lh_env_add(s0, rad[3 * r]); s1 = lh_env_add(s1, rad[3 * r + 1]); s2 = lh_env_add(s2, rad[3 * r + 2]);
    }
    *count = c;
    value[0] = lh_env_finish(scale, s0, N); value[1] = lh_env_finish(scale, s1, N); value[2] = lh_env_finish(scale, s2, N);
}

#endif
