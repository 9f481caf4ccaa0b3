/*
 * lh_whitted.h -- the rule of the refraction chain (trace_whitted, src/transport/whitted.c:32-86; ri_refract and ri_reflect,
 * src/render/reflection.c:26-128), one statement of it for the bounce kernel (lh_whitted.hip), the entry points' parameter check
 * and the test that checks it without a GPU (tests/test_whitted_rule.py).
 *
 * The transport has no random number in it: an eye hit sends ONE ray on, the refraction of the incoming direction I at the
 * interpolated normal Ns with the relative index eta (or its mirror image where the refraction does not exist), from P + eps R;
 * what that ray hits sends the next one, up to max_depth rays; the chain's value is the environment seen by the ray that leaves
 * the scene, or nothing if no ray does.  The reflection ray of a classic Whitted tracer is commented out in the reference and is
 * not part of this.
 *
 * One bounce, from the hit's state as lh_accel_state_build_device gives it (P: doubles 0-2; n = Ns: doubles 6-8, NOT normalised
 * when it is interpolated; I: doubles 20-22, the normalised ray direction) -- every step one fp64 operation in the order written,
 * nothing contracted:
 *   cos1 = (I0 n0 + I1 n1) + I2 n2
 *   cos1 < 0:  c = -cos1, e = 1 / eta, N = n;   else:  c = cos1, e = eta, N = -n           (entering / leaving by the sign alone)
 *   coeff = 1 - (e e) (1 - c c)
 *   coeff <= 0 (total internal reflection):  s = (double)(2.0f * (float)cos1) -- the reference keeps this dot product in a float and
 *       doubles it there --, R = I - n s with the normal as it came
 *   else:  q = e c - sqrt(coeff),  R = q N + e I
 *   n2 = (R0 R0 + R1 R1) + R2 R2;  n2 > (double)1.0e-17f:  R *= 1 / sqrt(n2);  else R stays as it is (a zero normal and a grazing ray)
 *   next ray:  org = P + eps R,  dir = R
 *
 * The chain of one eye hit (state 0), d = 1 .. max_depth: ray d is the bounce of state d - 1, traced as a closest-hit ray like any
 * other (no self-primitive skip: eps is far below the 1e-6 lh_ao.h's argument rests on).  A miss: the chain ESCAPES, bounces = d,
 * value = the environment in the direction of ray d.  A hit with d == max_depth: the chain is CUT, bounces = d | LH_WHITTED_CUT, value
 * 0 (whitted.c:48-50 returns with the radiance as it was initialised).  Any other hit: state d.  max_depth 0 cuts every eye hit.
 *
 * The environment is the accelerator's (lh_accel_set_environment; constant white if none was set).  The reference gives black
 * where the scene has no environment map: a caller who wants that sets a constant black environment.
 *
 * DESIGN.md 10.0e has the loop built on it; tests/test_gpu_whitted.py pins it to the oracle.
 */
#ifndef LH_WHITTED_H
#define LH_WHITTED_H

#include <math.h>
#include <stdint.h>

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

/* contraction off inside the functions below, whatever the including file is compiled with (host C: -ffp-contract=off does it) */
#ifndef LH_NC
#if defined(__clang__)
#define LH_NC _Pragma("clang fp contract(off)")
#else
#define LH_NC
#endif
#endif

#define LH_WHITTED_EPS_DEFAULT   1.0e-7      /* whitted.c:38 */
#define LH_WHITTED_ETA_DEFAULT   1.33        /* whitted.c:46 */
#define LH_WHITTED_DEPTH_DEFAULT 8           /* whitted.c:24 */
#define LH_WHITTED_DEPTH_MAX     64
#define LH_WHITTED_CUT_BIT       0x80000000u /* LH_WHITTED_CUT of lucille_hip.h */

/* accepted: eps finite and >= 0, eta finite and > 0, 0 <= max_depth <= 64, reserved 0.  Everything else (NaN included: every
 * comparison with it is false; x - x is 0 for finite x alone) is refused */
LH_HD int lh_whitted_params_ok(double eps, double eta, int max_depth, int reserved)
{
    if (!(eps >= 0.0 && eps - eps == 0.0)) return 0;
    if (!(eta > 0.0 && eta - eta == 0.0)) return 0;
    if (max_depth < 0 || max_depth > LH_WHITTED_DEPTH_MAX) return 0;
    return reserved == 0;
}

/* the direction the chain goes on in from a hit with incoming unit direction I and normal n; returns 1 for a total internal reflection */
LH_HD int lh_whitted_refract(const double I[3], const double n[3], double eta, double R[3])
{
    LH_NC
    const double cos1 = (I[0] * n[0] + I[1] * n[1]) + I[2] * n[2];
    const int entering = cos1 < 0.0;
    const double c = entering ? -cos1 : cos1;
    const double e = entering ? 1.0 / eta : eta;
    const double coeff = 1.0 - (e * e) * (1.0 - c * c);
    int tir = 0;
    if (coeff <= 0.0) {
        const double s = (double)(2.0f * (float)cos1);
        R[0] = I[0] - n[0] * s; R[1] = I[1] - n[1] * s; R[2] = I[2] - n[2] * s;
        tir = 1;
    } else {
        const double q = e * c - sqrt(coeff);
        const double N0 = entering ? n[0] : -n[0], N1 = entering ? n[1] : -n[1], N2 = entering ? n[2] : -n[2];
        R[0] = q * N0 + e * I[0]; R[1] = q * N1 + e * I[1]; R[2] = q * N2 + e * I[2];
    }
    {
        const double n2 = (R[0] * R[0] + R[1] * R[1]) + R[2] * R[2];
        if (n2 > (double)1.0e-17f) { const double r = 1.0 / sqrt(n2); R[0] *= r; R[1] *= r; R[2] *= r; }
    }
    return tir;
}

/* one bounce: the next ray of the chain from P, n = Ns and I of a hit's state */
LH_HD int lh_whitted_bounce(const double P[3], const double n[3], const double I[3], double eps, double eta, double org[3], double dir[3])
{
    LH_NC
    const int tir = lh_whitted_refract(I, n, eta, dir);
    org[0] = P[0] + eps * dir[0]; org[1] = P[1] + eps * dir[1]; org[2] = P[2] + eps * dir[2];
    return tir;
}

#endif
