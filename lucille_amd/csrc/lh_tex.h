/*
 * lh_tex.h -- the material texture of the occlusion transports, one statement of it for the resolve kernels (lh_render.hip), the
 * entry points (lh_tex.hip) and the test that checks it without a GPU (tests/test_tex_rule.py).
 *
 * Both transports the reference runs end the same way: where the hit's geometry has a material with a texture,
 *   ri_texture_fetch(texcol, texture, st[0], st[1]);  radiance[k] *= texcol[k]
 * (src/transport/ambientocclusion.c:393-401, src/transport/dirtmap.c:273-281).  The fetch is ri_texture_fetch (src/render/texture.c:
 * 86-235, the scanline branch): the fraction of (s, t), a bilinear filter over the four texels around it, a neighbour outside the
 * image counting as 0.  Texels are RGBA fp32, row 0 first (ri_texture_t.data, src/render/texture.h:21-29), no flip; everything else
 * is fp64 in the order written below.  The sums are sums of products: the files that include this header are compiled with
 * -ffp-contract=off (the reference is SSE2: no fused multiply-add).
 *
 * A non-finite s or t makes the reference's (int) cast undefined; here the result is unspecified but the texel index stays inside
 * the image: nothing outside the width x height texels is ever read.
 *
 * DESIGN.md 10.0c has the stage built on it; tests/test_gpu_tex.py pins the frames to it.
 */
#ifndef LH_TEX_H
#define LH_TEX_H

#include <math.h>
#include <stddef.h>

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

#define LH_TEX_MAX_SIZE 65536          /* RI_MAX_MIPMAP_SIZE 16 (texture.h:19): up to 65536 x 65536 */

/* what the kernels read of one mesh: texels NULL = the mesh has no texture */
typedef struct lh_tex_desc { const float *texels; int width, height; } lh_tex_desc_t;

/* texel (x, y), widened */
LH_HD void lh_tex_texel(const float *texels, int width, int x, int y, double e[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float *q = (const float *)__builtin_assume_aligned(texels, 16) + 4 * ((size_t)y * (size_t)width + (size_t)x);      /* the library's own block: one 16-byte load */
#else
    const float *q = texels + 4 * ((size_t)y * (size_t)width + (size_t)x);
#endif
    e[0] = (double)q[0]; e[1] = (double)q[1]; e[2] = (double)q[2]; e[3] = (double)q[3];
}

/* the fraction of a coordinate, clamped as texture.c:101-106 does */
LH_HD double lh_tex_wrap(double s)
{
    double u = s - floor(s);
    if (u < 0.0) u = 0.0;
    if (u >= 1.0) u = 1.0;
    return u;
}

/* the texel a pixel coordinate falls in: (int)p for every finite input (0 <= p <= n - 1 then); anything else -- a NaN from a
 * non-finite s -- goes to texel 0 */
LH_HD int lh_tex_cell(double p, int n) { return (p >= 0.0 && p <= (double)(n - 1)) ? (int)p : 0; }

/* ri_texture_fetch: out[4] = the filtered RGBA at (s, t); width, height >= 1 */
LH_HD void lh_tex_fetch(const float *texels, int width, int height, double s, double t, double out[4])
{
    const double u = lh_tex_wrap(s), v = lh_tex_wrap(t);
    const double px = u * (double)(width - 1), py = v * (double)(height - 1);
    const int x = lh_tex_cell(px, width), y = lh_tex_cell(py, height);
    const double dx = px - (double)x, dy = py - (double)y;
    const double w0 = (1.0 - dx) * (1.0 - dy), w1 = (1.0 - dx) * dy, w2 = dx * (1.0 - dy), w3 = dx * dy;
    const int right = x < width - 1, below = y < height - 1;
    double e0[4], e1[4] = {0.0, 0.0, 0.0, 0.0}, e2[4] = {0.0, 0.0, 0.0, 0.0}, e3[4] = {0.0, 0.0, 0.0, 0.0};
    int i;
    lh_tex_texel(texels, width, x, y, e0);
    if (below) lh_tex_texel(texels, width, x, y + 1, e1);
    if (right) lh_tex_texel(texels, width, x + 1, y, e2);
    if (right && below) lh_tex_texel(texels, width, x + 1, y + 1, e3);
    for (i = 0; i < 4; i++) out[i] = ((w0 * e0[i] + w1 * e1[i]) + w2 * e2[i]) + w3 * e3[i];
}

/* the coordinates of a hit: lerp_uv (intersection_state.c:58-76) over the primitive's six doubles (s0 t0 s1 t1 s2 t2), as
 * k_state_build writes doubles 18 and 19 of the hit epilogue */
LH_HD void lh_tex_st(const double *st6, double u, double v, double *s, double *t)
{
    const double w = 1.0 - u - v;
    *s = (w * st6[0] + u * st6[2]) + v * st6[4];
    *t = (w * st6[1] + u * st6[3]) + v * st6[5];
}

#endif
