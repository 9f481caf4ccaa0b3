/*
 * lh_shade.h -- device functions lh_render.hip and lh_whitted.hip share: the part of the hit epilogue a transport needs to send a ray
 * on (P, Ng, Ns, I of ri_intersection_state_build, src/render/intersection_state.c:99-248) and the environment as a kernel argument.
 * Device code only: included inside the including file's anonymous namespace, behind lh_pt.h (vnormalize, vcross, DevEnv, env_fetch)
 * and lh_internal.h (lh_env_src_t).
 */
#ifndef LH_SHADE_H
#define LH_SHADE_H

/* P, I (the normalised direction), Ns -- the interpolated vertex normals as they are, not normalised, where primitive p has them
 * (returns true), else the geometric normal -- and Ng of the hit (tt, uu, vv) of primitive p by the ray org / dir.  NG: Ng is wanted
 * whatever the mesh has (k_state_build); else it is computed, and the triangle's corners read, only for a flat-shaded hit */
template <bool NG>
__device__ __forceinline__ bool state_core(const void *tri64, const double *__restrict__ nrm9, uint32_t p, const double org[3], const double dir[3],
                                           double tt, double uu, double vv, double P[3], double Ng[3], double Ns[3], double I[3])
{
    LH_NC
    const double w = 1.0 - uu - vv;
    for (int k = 0; k < 3; k++) { P[k] = org[k] + dir[k] * tt; I[k] = dir[k]; }
    vnormalize(I);
    bool has_n = false;
    if (nrm9) { const double x = nrm9[9 * (size_t)p]; has_n = (x == x); }
    if (NG || !has_n) {
        const double *tv = (const double *)tri64 + 9 * (size_t)p;
        double v01[3], v02[3];
        for (int k = 0; k < 3; k++) { v01[k] = tv[3 + k] - tv[k]; v02[k] = tv[6 + k] - tv[k]; }
        vcross(Ng, v01, v02); vnormalize(Ng);
    }
    if (has_n) {
        const double *q = nrm9 + 9 * (size_t)p;
        for (int k = 0; k < 3; k++) { const double a = q[k] * w, b = q[3 + k] * uu, c = q[6 + k] * vv; Ns[k] = (a + b) + c; }
    } else for (int k = 0; k < 3; k++) Ns[k] = Ng[k];
    return has_n;
}

/* the accelerator's environment as a kernel argument */
__device__ __host__ inline DevEnv env_of(const lh_env_src_t &e)
{
    DevEnv d;
    d.rgb[0] = e.rgb[0]; d.rgb[1] = e.rgb[1]; d.rgb[2] = e.rgb[2];
    d.map = (const float4 *)e.map; d.w = e.w; d.h = e.h;
    return d;
}

/* env_fetch for a direction nobody checked: a component that is not finite would reach the texel index as a NaN; such a direction (its colour is
 * unspecified) is looked up as +z.  Every finite direction goes to env_fetch as it is: a zero vector or one whose norm under- or overflows
 * ends at u = v = 1/2 by env_fetch's own arithmetic */
__device__ __forceinline__ void env_lookup(const DevEnv &e, double dx, double dy, double dz, float out[3])
{
    if (!(isfinite(dx) && isfinite(dy) && isfinite(dz))) { dx = 0.0; dy = 0.0; dz = 1.0; }
    env_fetch(e, dx, dy, dz, out);
}

#endif
