/*
 * lh_lights.h -- the rule of direct light from a short list of lights: one shadow ray per hit and light (contribution_from_sunlight,
 * src/transport/ambientocclusion.c:153-199, for every kind of ri_light_t the reference knows: directional and point, light.h:26-32).  One
 * statement of it for the kernel that makes the rays (lh_kernels.hip: the light source of the persistent walk, its cooperative twin),
 * the materialised ray maker and the two resolves (lh_render.hip), the entry points (lh_tile.hip) and the test that checks it without a
 * GPU (tests/test_lights_rule.py).  Plain C.
 *
 * For a hit with origin O = P + eps Ns (the gather stages' origin: doubles 0-2 of a hit record) and shading normal Ns (doubles 9-11, taken
 * as it is, not normalised) and light l, everything in fp64 in the order written, nothing contracted:
 *   ray     directional: dir = v, unbounded (tmax = +inf).  Point: dir[k] = v[k] - O[k], not normalised, tmax = 1.0 -- the ray ends AT the
 *           light; the comparison is strict (lh_tmax.h: t < tmax), an occluder exactly at the light does not shadow it.
 *   weight  w = 1; with LH_LIGHT_COSINE nn = (Ns0 Ns0 + Ns1 Ns1) + Ns2 Ns2, dd the same sum of dir, nd = (Ns0 d0 + Ns1 d1) + Ns2 d2,
 *           c = nd / sqrt(nn * dd), w = c > 0 ? c : 0 (a NaN gives 0); with LH_LIGHT_INVSQ w = w / dd afterwards.
 *   dark    a ray whose direction is the zero vector or has a non-finite component is dark and is never handed to a walk; so is here a
 *           ray with !(w > 0): it could add nothing (lh_light_item gives both the bound 0.0).
 *   bit l   = !dark && w > 0 && the ray is open: the bounded any-hit answer (lh_accel_intersect_device_tmax) of (O, dir, tmax) is 0.
 *   value   sum_k = 0; for l = 0 .. L - 1 in list order: if (bit l) sum_k = sum_k + w * rgb_l[k]; value_k = (float)sum_k.  The order is
 *           part of the contract.  With no flags this is Lo[k] += light->col[k] of the reference, per light.
 * No self-primitive skip: a light behind the surface is shadowed by the hit's own triangle, as the sky's sun and as in the reference.
 *
 * The kernels are compiled with -ffp-contract=off, a host program that includes this file must be too.
 * DESIGN.md 10.0g has the stage built on it; tests/test_gpu_lights.py pins it to the oracle.
 */
#ifndef LH_LIGHTS_H
#define LH_LIGHTS_H

#include <math.h>
#include <stdint.h>

#include "../../include/lucille_hip.h"      /* lh_light_t, LH_LIGHT_*, LH_LIGHTS_MAX, lh_lights_params_t */

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

#define LH_LIGHT_FLAGS (LH_LIGHT_POINT | LH_LIGHT_COSINE | LH_LIGHT_INVSQ)          /* the defined bits */
#define LH_LIGHT_TMAX_INF ((double)INFINITY)          /* the bound of a directional light's ray: none (lh_tmax.h takes it as 1e38) */

/* a call's lights as the kernels take them: by value in their arguments (1 736 bytes; entries beyond the call's count are zero) */
typedef struct lh_light_tab { lh_light_t l[LH_LIGHTS_MAX]; } lh_light_tab_t;

/* finite: x - x is 0 for finite x alone (NaN: every comparison is false) */
LH_HD int lh_light_fin(double x) { return x - x == 0.0; }

/* accepted: eps finite and >= 0 */
LH_HD int lh_lights_params_ok(double eps) { return eps >= 0.0 && lh_light_fin(eps); }

/* accepted: v and rgb finite, a directional v not the zero vector, flags within the three bits, reserved 0, LH_LIGHT_INVSQ only with LH_LIGHT_POINT */
LH_HD int lh_light_ok(const lh_light_t *l)
{
    int k, ok = 1;
    for (k = 0; k < 3; k++) ok = ok && lh_light_fin(l->v[k]) && lh_light_fin(l->rgb[k]);
    if (!ok) return 0;
    if ((l->flags & ~(uint32_t)LH_LIGHT_FLAGS) != 0u || l->reserved != 0u) return 0;
    if ((l->flags & LH_LIGHT_INVSQ) && !(l->flags & LH_LIGHT_POINT)) return 0;
    if (!(l->flags & LH_LIGHT_POINT) && l->v[0] == 0.0 && l->v[1] == 0.0 && l->v[2] == 0.0) return 0;
    return 1;
}

/* a whole call's list: 1 <= n <= LH_LIGHTS_MAX, every light accepted, eps accepted */
LH_HD int lh_lights_ok(const lh_light_t *lights, int n, double eps)
{
    int l;
    if (!lh_lights_params_ok(eps) || !lights || n < 1 || n > LH_LIGHTS_MAX) return 0;
    for (l = 0; l < n; l++) if (!lh_light_ok(lights + l)) return 0;
    return 1;
}

/* the origin of a hit's shadow rays: what k_ao_setup leaves in doubles 0-2 of a hit record for the same eps */
LH_HD void lh_light_origin(const double P[3], const double Ns[3], double eps, double O[3])
{
    O[0] = P[0] + Ns[0] * eps; O[1] = P[1] + Ns[1] * eps; O[2] = P[2] + Ns[2] * eps;
}

/* the shadow ray of light l from O: its direction, and (returned) its bound -- +inf directional, 1.0 point, 0.0 for a ray that is dark without a walk */
LH_HD double lh_light_ray(const double O[3], const lh_light_t *l, double dir[3])
{
    double tmax = LH_LIGHT_TMAX_INF;
    if (l->flags & LH_LIGHT_POINT) { dir[0] = l->v[0] - O[0]; dir[1] = l->v[1] - O[1]; dir[2] = l->v[2] - O[2]; tmax = 1.0; }
    else { dir[0] = l->v[0]; dir[1] = l->v[1]; dir[2] = l->v[2]; }
    if (!(lh_light_fin(dir[0]) && lh_light_fin(dir[1]) && lh_light_fin(dir[2]))) return 0.0;
    if (dir[0] == 0.0 && dir[1] == 0.0 && dir[2] == 0.0) return 0.0;
    return tmax;
}

/* the weight of a ray that is open */
LH_HD double lh_light_weight(const double Ns[3], const double dir[3], uint32_t flags)
{
    const double dd = (dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2];
    double w = 1.0;
    if (flags & LH_LIGHT_COSINE) {
        const double nn = (Ns[0] * Ns[0] + Ns[1] * Ns[1]) + Ns[2] * Ns[2];
        const double nd = (Ns[0] * dir[0] + Ns[1] * dir[1]) + Ns[2] * dir[2];
        const double c = nd / sqrt(nn * dd);
        w = c > 0.0 ? c : 0.0;
    }
    if (flags & LH_LIGHT_INVSQ) w = w / dd;
    return w;
}

/* work item (hit, l) whole: the ray, its weight, and (returned) the bound it is traced under -- 0.0: not traced, its bit is clear whatever a walk
 * would answer (dark, or !(w > 0)) */
LH_HD double lh_light_item(const double O[3], const double Ns[3], const lh_light_t *l, double dir[3], double *w)
{
    const double tmax = lh_light_ray(O, l, dir);
    *w = lh_light_weight(Ns, dir, l->flags);
    return (tmax > 0.0 && *w > 0.0) ? tmax : 0.0;
}

/* one visible light's colour channel into the running sum of its hit */
LH_HD double lh_light_add(double sum, double w, double rgb) { return sum + w * rgb; }

/* the hit's mask and value from the any-hit bytes of its L items (occ[l] != 0: an occluder below the bound), in list order */
LH_HD uint32_t lh_lights_value(const double O[3], const double Ns[3], const lh_light_t *lights, int L, const uint8_t *occ, float value[3])
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    uint32_t mask = 0u;
    int l;
    for (l = 0; l < L; l++) {
        double dir[3], w;
        const double tmax = lh_light_item(O, Ns, lights + l, dir, &w);
        if (!(tmax > 0.0) || occ[l]) continue;
        mask |= 1u << l;
        s0 = lh_light_add(s0, w, lights[l].rgb[0]); s1 = lh_light_add(s1, w, lights[l].rgb[1]); s2 = lh_light_add(s2, w, lights[l].rgb[2]);
    }
    value[0] = (float)s0; value[1] = (float)s1; value[2] = (float)s2;
    return mask;
}

#endif
