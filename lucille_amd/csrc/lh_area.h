/*
 * lh_area.h -- the rule of direct light from area lights: triangle emitters sampled S times per hit (the mesh an ri_light_t carries: light->geom,
 * ri_light_attach_geom, src/render/light.c:107-111; the point and normal drawn on it: ri_light_sample_pos_and_normal, light.c:113-147, with
 * ri_normal_of_triangle, src/base/geometric.c:20-33, and ri_vector_normalize's guard, src/base/vector.h:75-87).  One statement of it for the kernels that
 * make the rays (lh_kernels.hip: ray source 4 of the persistent walk, its cooperative twin), the materialised ray maker and the two resolves
 * (lh_render.hip), the entry points (lh_tile.hip) and the test that checks it without a GPU (tests/test_area_rule.py).  Plain C.
 *
 * Everything in fp64 in the order written, nothing contracted:
 *   record  one per emitter triangle, made once when the table is set (lh_accel_set_emitters): 16 doubles = one aligned 128-byte line, v0 v1 v2 n area pad.
 *           e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2 as ri_vector_cross writes it; norm2 = (c0 c0 + c1 c1) + c2 c2, len = sqrt(norm2);
 *           n = c * (1.0 / len) where norm2 > (double)1.0e-17f, else n = c; area = 0.5 * len.
 *   sample  an area light is the run [first_tri, first_tri + ntris) of the table.  With three uniforms (x0, x1, x2): j = (int)(x0 * (double)ntris) clamped
 *           to [0, ntris - 1] (the reference reads out of bounds where the product rounds up to ntris); a NaN x0 makes the item dark.  s = sqrt(x1),
 *           t = x2, pos[k] = (double)(float)((v0[k] * (1.0 - s) + v1[k] * (s - t * s)) + (v2[k] * s) * t): the reference's parse and its rounding to
 *           float.  n is the record's.
 *   ray     from the gathers' origin O = P + eps Ns (doubles 0-2 of a hit record): dir = pos - O, not normalised, under the call's bound, 0 < bound <= 1.
 *           A caller whose emitter triangles are occluders too passes a little less than 1: the float-rounded pos lies off the triangle's plane.
 *           No self-primitive skip.  A non-finite or zero dir is dark.
 *   weight  w = 1; dd = (d0 d0 + d1 d1) + d2 d2; then in this order
 *           LH_AREA_COSINE  LH_LIGHT_COSINE's expression: nn = (Ns0 Ns0 + Ns1 Ns1) + Ns2 Ns2, nd = (Ns0 d0 + Ns1 d1) + Ns2 d2, c = nd / sqrt(nn * dd),
 *                           w = c > 0 ? c : 0;
 *           LH_AREA_FACING  cl = -((n0 d0 + n1 d1) + n2 d2) / sqrt(dd), w = w * (cl > 0 ? cl : 0): a one-sided emitter;
 *           LH_AREA_INVSQ   w = w / dd;
 *           LH_AREA_PDF     w = w * ((double)ntris * area_j): the pick is uniform by index, this is 1 / pdf.
 *   item    (hit, l, s) with a dark ray or !(w > 0) has the bound 0.0 and is never handed to a walk (lh_light_item's convention).
 *   value   sum_k = 0; for l in list order, for s = 0 .. S - 1: if item (l, s) is traced and open, sum_k = sum_k + w * rgb_l[k];
 *           value_k = (float)(sum_k / (double)S); bit l of the mask: any sample of light l is open.  The order is part of the contract.
 *   uniforms  replayed: 3 doubles per item in (hit slot, l, s) order.  Built in: c = ((key & LH_AREA_KEY_MASK) * (uint64)(L S) + (uint64)(l S + s)) * 4,
 *           k = (seed * 0x9E3779B97F4A7C15) ^ c, x_j = (double)mix32(k + j) * 2^-32 for j = 0, 1, 2 (lh_ao.h's lh_mix32).  The built-in path is the
 *           replay rule fed by this generator: one sampling rule, not two.
 *
 * The kernels are compiled with -ffp-contract=off, a host program that includes this file must be too.
 * DESIGN.md 10.0h has the stage built on it; tests/test_gpu_area.py pins it to the oracle.
 */
#ifndef LH_AREA_H
#define LH_AREA_H

#include <math.h>
#include <stdint.h>

#include "../../include/lucille_hip.h"      /* lh_area_light_t, LH_AREA_*, lh_area_params_t */

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

#define LH_AREA_FLAGS (LH_AREA_COSINE | LH_AREA_FACING | LH_AREA_INVSQ | LH_AREA_PDF)          /* the defined bits */
#define LH_AREA_KEY_MASK ((1ull << 34) - 1ull)          /* LH_SLOTKEY_MASK (lh_ao.h): the absolute sample position of a slot key */
#define LH_AREA_EMITTERS_MAX ((uint64_t)1 << 31)        /* a table holds fewer triangles than this */

/* one emitter triangle as the kernels gather it: one aligned 128-byte line */
typedef struct lh_emitter { double v0[3], v1[3], v2[3], n[3], area, pad[3]; } lh_emitter_t;

/* a call's lights as the kernels take them, by value in their arguments (1 272 bytes; entries beyond the call's count are zero), with what every item
 * needs beside them: the emitter table (device memory the accelerator owns), the samples per light, the bound of a traced ray, the replayed uniforms */
typedef struct lh_area_tab {
    lh_area_light_t l[LH_AREA_LIGHTS_MAX];
    const lh_emitter_t *emitters;
    const double *uniforms;          /* NULL: the built-in generator */
    double bound;
    int32_t L, S;
} lh_area_tab_t;

/* finite: x - x is 0 for finite x alone */
LH_HD int lh_area_fin(double x) { return x - x == 0.0; }

/* the record of a triangle given as 9 doubles */
LH_HD void lh_area_emitter(const double t[9], lh_emitter_t *e)
{
    const double e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
    double c[3];
    int k;
    c[0] = e1[1] * e2[2] - e1[2] * e2[1];
    c[1] = e1[2] * e2[0] - e1[0] * e2[2];
    c[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double norm2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2], len = sqrt(norm2);
    for (k = 0; k < 3; k++) { e->v0[k] = t[k]; e->v1[k] = t[3 + k]; e->v2[k] = t[6 + k]; }
    if (norm2 > (double)1.0e-17f) { const double r = 1.0 / len; e->n[0] = c[0] * r; e->n[1] = c[1] * r; e->n[2] = c[2] * r; }
    else { e->n[0] = c[0]; e->n[1] = c[1]; e->n[2] = c[2]; }
    e->area = 0.5 * len;
    e->pad[0] = e->pad[1] = e->pad[2] = 0.0;
}

/* accepted: eps finite and >= 0, bound finite with 0 < bound <= 1, 1 <= S <= LH_AREA_SAMPLES_MAX, reserved 0 */
LH_HD int lh_area_params_ok(const lh_area_params_t *p)
{
    return p->eps >= 0.0 && lh_area_fin(p->eps) && p->bound > 0.0 && p->bound <= 1.0 && p->nsamples >= 1 && p->nsamples <= LH_AREA_SAMPLES_MAX &&
           p->reserved == 0u;
}

/* accepted: rgb finite, flags within the four bits, reserved 0, ntris >= 1 and the run inside a table of `table_tris` triangles (no overflow: 64-bit sums) */
LH_HD int lh_area_light_ok(const lh_area_light_t *l, uint64_t table_tris)
{
    int k;
    for (k = 0; k < 3; k++) if (!lh_area_fin(l->rgb[k])) return 0;
    if ((l->flags & ~(uint32_t)LH_AREA_FLAGS) != 0u || l->reserved != 0u) return 0;
    if (l->ntris < 1u) return 0;
    return (uint64_t)l->first_tri + (uint64_t)l->ntris <= table_tris;
}

/* a whole call's list: 1 <= n <= LH_AREA_LIGHTS_MAX, every light accepted, the parameters accepted */
LH_HD int lh_area_lights_ok(const lh_area_light_t *lights, int n, const lh_area_params_t *p, uint64_t table_tris)
{
    int l;
    if (!p || !lh_area_params_ok(p) || !lights || n < 1 || n > LH_AREA_LIGHTS_MAX) return 0;
    for (l = 0; l < n; l++) if (!lh_area_light_ok(lights + l, table_tris)) return 0;
    return 1;
}

/* lh_ao.h's lh_mix32, for host and device */
LH_HD uint32_t lh_area_mix32(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return (uint32_t)(x >> 16);
}

/* the built-in uniforms of item (l, s) of the hit whose slot key is `key` */
LH_HD void lh_area_uniforms(unsigned long long key, unsigned long long seed, int L, int S, int l, int s, double x[3])
{
    const uint64_t c = ((key & LH_AREA_KEY_MASK) * (uint64_t)((int64_t)L * S) + (uint64_t)((int64_t)l * S + s)) * 4ull;
    const uint64_t k = ((uint64_t)seed * 0x9E3779B97F4A7C15ULL) ^ c;
    x[0] = (double)lh_area_mix32(k) * 2.3283064365386963e-10;
    x[1] = (double)lh_area_mix32(k + 1ull) * 2.3283064365386963e-10;
    x[2] = (double)lh_area_mix32(k + 2ull) * 2.3283064365386963e-10;
}

/* the triangle a light's sample falls on, as an offset into its run; -1: x0 is a NaN, the item is dark */
LH_HD int32_t lh_area_pick(double x0, uint32_t ntris)
{
    const double p = x0 * (double)ntris;
    if (!(x0 == x0)) return -1;
    if (!(p >= 1.0)) return 0;                                 /* (int) of anything below 1 is 0 or negative: clamped */
    if (p >= (double)ntris) return (int32_t)(ntris - 1u);      /* rounded up to ntris, or beyond the range */
    return (int32_t)p;
}

/* the point drawn on record e with (x1, x2) */
LH_HD void lh_area_point(const lh_emitter_t *e, double x1, double x2, double pos[3])
{
    const double s = sqrt(x1), t = x2;
    const double a = 1.0 - s, b = s - t * s;
    int k;
    for (k = 0; k < 3; k++) pos[k] = (double)(float)((e->v0[k] * a + e->v1[k] * b) + (e->v2[k] * s) * t);
}

/* the weight of a ray to a point of record e of a light of ntris triangles */
LH_HD double lh_area_weight(const double Ns[3], const double dir[3], const lh_emitter_t *e, uint32_t ntris, uint32_t flags)
{
    const double dd = (dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2];
    double w = 1.0;
    if (flags & LH_AREA_COSINE) {
        const double nn = (Ns[0] * Ns[0] + Ns[1] * Ns[1]) + Ns[2] * Ns[2];
        const double nd = (Ns[0] * dir[0] + Ns[1] * dir[1]) + Ns[2] * dir[2];
        const double c = nd / sqrt(nn * dd);
        w = c > 0.0 ? c : 0.0;
    }
    if (flags & LH_AREA_FACING) {
        const double cl = -((e->n[0] * dir[0] + e->n[1] * dir[1]) + e->n[2] * dir[2]) / sqrt(dd);
        w = w * (cl > 0.0 ? cl : 0.0);
    }
    if (flags & LH_AREA_INVSQ) w = w / dd;
    if (flags & LH_AREA_PDF) w = w * ((double)ntris * e->area);
    return w;
}

/* work item (hit, l, s) whole from its three uniforms: the ray, its weight, and (returned) the bound it is traced under -- `bound`, or 0.0: not traced,
 * it is not open whatever a walk would answer.  emitters: the table (the one dependent load of an item: record first_tri + j) */
LH_HD double lh_area_item(const double O[3], const double Ns[3], const lh_area_light_t *l, const lh_emitter_t *emitters, const double x[3], double bound,
                          double dir[3], double *w)
{
    const int32_t j = lh_area_pick(x[0], l->ntris);
    double pos[3];
    dir[0] = dir[1] = dir[2] = 0.0; *w = 0.0;
    if (j < 0) return 0.0;
    const lh_emitter_t *e = emitters + ((size_t)l->first_tri + (size_t)j);
    lh_area_point(e, x[1], x[2], pos);
    dir[0] = pos[0] - O[0]; dir[1] = pos[1] - O[1]; dir[2] = pos[2] - O[2];
    if (!(lh_area_fin(dir[0]) && lh_area_fin(dir[1]) && lh_area_fin(dir[2]))) return 0.0;
    if (dir[0] == 0.0 && dir[1] == 0.0 && dir[2] == 0.0) return 0.0;
    *w = lh_area_weight(Ns, dir, e, l->ntris, l->flags);
    return *w > 0.0 ? bound : 0.0;
}

/* the uniforms of item (l, s) of a hit: the slot's replayed ones (uni: its 3 L S doubles) or the built-in generator's */
LH_HD void lh_area_item_uniforms(const double *uni, unsigned long long key, unsigned long long seed, int L, int S, int l, int s, double x[3])
{
    if (uni) { const double *u = uni + 3 * ((size_t)l * (size_t)S + (size_t)s); x[0] = u[0]; x[1] = u[1]; x[2] = u[2]; }
    else lh_area_uniforms(key, seed, L, S, l, s, x);
}

/* the hit's mask and value from the any-hit bytes of its L S items (occ[l S + s] != 0: an occluder below the bound), in list and sample order;
 * *closed (or NULL): the items that are not open */
LH_HD uint32_t lh_area_value(const double O[3], const double Ns[3], const lh_area_light_t *lights, int L, int S, const lh_emitter_t *emitters, double bound,
                             const double *uni, unsigned long long key, unsigned long long seed, const uint8_t *occ, float value[3],
                             unsigned int *closed)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    uint32_t mask = 0u;
    unsigned int nopen = 0;
    int l, s;
    for (l = 0; l < L; l++)
        for (s = 0; s < S; s++) {
            double x[3], dir[3], w;
            lh_area_item_uniforms(uni, key, seed, L, S, l, s, x);
            const double tmax = lh_area_item(O, Ns, lights + l, emitters, x, bound, dir, &w);
            if (!(tmax > 0.0) || occ[(size_t)l * (size_t)S + (size_t)s]) continue;
            mask |= 1u << l;
            nopen++;
            s0 = s0 + w * lights[l].rgb[0]; s1 = s1 + w * lights[l].rgb[1]; s2 = s2 + w * lights[l].rgb[2];
        }
    value[0] = (float)(s0 / (double)S); value[1] = (float)(s1 / (double)S); value[2] = (float)(s2 / (double)S);
    if (closed) *closed = (unsigned int)(L * S) - nopen;
    return mask;
}

#endif
