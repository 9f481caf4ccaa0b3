/*
 * lh_sky.h -- the rule of the sun-and-sky light of the environment-lit gather (gather_sunsky with a sunsky light,
 * src/transport/ambientocclusion.c:206-324): the analytic Preetham sky (ri_sunsky_get_sky_rgb, src/render/sunsky.c:329-415) as the radiance of
 * a gather ray that is not occluded, and the sun's term of a hit's sum (contribution_from_sunlight, ambientocclusion.c:153-199,312-321).  One
 * statement of it for the resolve kernels (lh_render.hip), the entry points (lh_tile.hip, lh_sky.c) and the test that checks it without a
 * GPU (tests/test_sky_rule.py).  lh_env.h keeps the sum itself: lh_env_add, lh_env_finish.
 *
 * The sky of a direction, in the reference's types and order (float variables, fp64 libm calls on them, rounded to float where the
 * reference assigns to a float): swap y and z; below the horizon: zero; within 0.001 of it: pulled up to 0.001 and normalised; theta =
 * acos, phi = atan2 (0 where |theta| < 1e-6), gamma = angle_between(view, sun); three Perez functions give x, y, Y; M1, M2 from the
 * chromaticity.  From there the reference builds a 41-sample spectrum S0 + M1 S1 + M2 S2, scales it by Y / ly and sends it through
 * spectrum_to_xyz and xyz_to_rgb -- all linear in the spectrum, so
 *
 *     rgb_k = Y (C0_k + M1 C1_k + M2 C2_k) / (L0 + M1 L1 + M2 L2)
 *
 * with C_j = basis_rgb[j] the colour pipeline's rgb of basis spectrum S_j and L_j = basis_y[j] its CIE y: twelve floats the caller brings
 * (the daylight and colour-matching tables are not part of this project).  The collapsed sum is evaluated in fp64 and rounded once; it
 * rounds differently from the 41-sample one, so the sky is held to the reference by a measured bound (tests/test_sky_rule.py, DESIGN.md
 * 10.0f), not bit for bit.  A direction is taken as it is: one that is not of unit length gives an unspecified colour, NaN possibly.
 *
 * The sun's colour and direction are the caller's (light->col, light->direction): ri_sunsky_get_sunlight_rgb reads a turbidity that
 * ri_sunsky_init never stores.
 */
#ifndef LH_SKY_H
#define LH_SKY_H

#include <math.h>
#include <stdint.h>

#include "../../include/lucille_hip.h"

#ifndef LH_HD
#if defined(__HIPCC__)
#define LH_HD __host__ __device__ __forceinline__
#else
#define LH_HD static inline
#endif
#endif

#define LH_SKY_PI 3.14159265358979323846          /* M_PI */

/* finite: x - x is 0 for finite x alone (NaN: every comparison is false) */
LH_HD int lh_sky_fin(double x) { return x - x == 0.0; }

/* accepted: every field finite, flags within the defined bits */
LH_HD int lh_sky_ok(const lh_sky_t *s)
{
    int k, j, ok = lh_sky_fin(s->sun_theta) && lh_sky_fin(s->sun_phi) && lh_sky_fin(s->zenith_x) && lh_sky_fin(s->zenith_y) && lh_sky_fin(s->zenith_Y);
    for (k = 0; k < 5; k++) ok = ok && lh_sky_fin(s->perez_x[k]) && lh_sky_fin(s->perez_y[k]) && lh_sky_fin(s->perez_Y[k]);
    for (k = 0; k < 3; k++) {
        ok = ok && lh_sky_fin(s->basis_y[k]) && lh_sky_fin(s->sun_rgb[k]) && lh_sky_fin(s->sun_dir[k]);
        for (j = 0; j < 3; j++) ok = ok && lh_sky_fin(s->basis_rgb[k][j]);
    }
    return ok && (s->flags & ~(uint32_t)LH_SKY_FLAGS) == 0u;
}

/* PerezFunction's den (sunsky.c:148-150): of the sky alone */
LH_HD float lh_sky_perez_den(const float *lam, float sun_theta)
{
    const float ls = lam[3] * sun_theta;
    return (float)((1.0 + lam[0] * exp((double)lam[1])) *
                   (1.0 + lam[2] * exp((double)ls) + lam[4] * cos((double)sun_theta) * cos((double)sun_theta)));
}

/* the three denominators (x, y, Y), once per sky */
LH_HD void lh_sky_den(const lh_sky_t *s, float den[3])
{
    den[0] = lh_sky_perez_den(s->perez_x, s->sun_theta);
    den[1] = lh_sky_perez_den(s->perez_y, s->sun_theta);
    den[2] = lh_sky_perez_den(s->perez_Y, s->sun_theta);
}

/* PerezFunction's num and quotient (sunsky.c:152-156); ct = cos(theta), cg = cos(gamma) in fp64 */
LH_HD float lh_sky_perez(const float *lam, double ct, float gamma, double cg, float lvz, float den)
{
    const float lg = lam[3] * gamma;
    const float num = (float)((1.0 + lam[0] * exp(lam[1] / ct)) * (1.0 + lam[2] * exp((double)lg) + lam[4] * cg * cg));
    return lvz * num / den;
}

/* ri_sunsky_get_sky_rgb for the direction (dx, dy, dz), rounded to float first as gather_sunsky does into v[]; den: lh_sky_den of the sky */
LH_HD void lh_sky_rgb_den(const lh_sky_t *s, const float den[3], double dx, double dy, double dz, float rgb[3])
{
    float t0 = (float)dx, t1 = (float)dz, t2 = (float)dy;          /* t[1] = v[2], t[2] = v[1] */
    float theta, phi, gamma, cospi, x, y, Y, M1, M2, ly;
    double ct, cg, md, q;
    int k;
    if (t2 < 0.0f) { rgb[0] = 0.0f; rgb[1] = 0.0f; rgb[2] = 0.0f; return; }          /* under the horizon (-0.0 is not) */
    if ((double)t2 < 0.001) {
        float vlen;
        t2 = (float)0.001;
        vlen = (float)sqrt((double)(t0 * t0 + t1 * t1 + t2 * t2));
        t0 /= vlen; t1 /= vlen; t2 /= vlen;
    }
    theta = (float)acos((double)t2);
    if (fabs((double)theta) < 1.0e-6) phi = 0.0f;
    else phi = (float)atan2((double)t1, (double)t0);
    /* angle_between(theta, phi, sun_theta, sun_phi), sunsky.c:23-37 */
    {
        const float dphi = s->sun_phi - phi;
        cospi = (float)(sin((double)theta) * sin((double)s->sun_theta) * cos((double)dphi) + cos((double)theta) * cos((double)s->sun_theta));
        if ((double)cospi > 1.0) gamma = 0.0f;
        else if ((double)cospi < -1.0) gamma = (float)LH_SKY_PI;
        else gamma = (float)acos((double)cospi);
    }
    ct = cos((double)theta); cg = cos((double)gamma);
    x = lh_sky_perez(s->perez_x, ct, gamma, cg, s->zenith_x, den[0]);
    y = lh_sky_perez(s->perez_y, ct, gamma, cg, s->zenith_y, den[1]);
    Y = lh_sky_perez(s->perez_Y, ct, gamma, cg, s->zenith_Y, den[2]);
    /* chromaticity_to_spectrum's M1, M2 (sunsky.c:315-318) */
    md = 0.0241 + 0.2562 * x - 0.7341 * y;
    M1 = (float)((-1.3515 - 1.7703 * x + 5.9114 * y) / md);
    M2 = (float)((0.03 - 31.4424 * x + 30.0717 * y) / md);
    /* the spectrum, collapsed: its CIE y, then Y / ly times its rgb */
    ly = (float)((double)s->basis_y[0] + (double)M1 * (double)s->basis_y[1] + (double)M2 * (double)s->basis_y[2]);
    if (fabs((double)ly) < 1.0e-48) ly = 1.0f;
    q = (double)Y / (double)ly;
    for (k = 0; k < 3; k++)
        rgb[k] = (float)(q * ((double)s->basis_rgb[0][k] + (double)M1 * (double)s->basis_rgb[1][k] + (double)M2 * (double)s->basis_rgb[2][k]));
}

/* the same with the denominators made on the spot */
LH_HD void lh_sky_rgb(const lh_sky_t *s, double dx, double dy, double dz, float rgb[3])
{
    float den[3];
    lh_sky_den(s, den);
    lh_sky_rgb_den(s, den, dx, dy, dz, rgb);
}

/* the sun's term of a channel's sum: added after the N gather rays, before lh_env_finish, where the sun's ray is not occluded
 * (ambientocclusion.c:189-195,312-321) */
LH_HD double lh_sky_add_sun(double sum, int sun_occluded, float sun) { return sun_occluded ? sum : sum + (double)sun; }

#if !defined(__HIPCC__)
/* what ri_sunsky_init (sunsky.c:183-307) and init_sun_theta_phi (sunsky.c:39-75) leave in the struct without a table: the angles, the
 * fifteen Perez coefficients, the three zenith values, and sun_dir in the reference's light convention (y and z swapped,
 * src/ri/lightsource.c:156-158).  basis_*, sun_rgb and flags are left alone.  Host only */
static inline void lh_sky_site(lh_sky_t *s, float latitude, float longitude, float sm, int julian_day, float time_of_day, float turb)
{
#define LH_SKY_DEG2RAD(x) ((x) * LH_SKY_PI / 180.0)
    float solar_time, solar_declination, solar_altitude, solar_azimuth, opp, adj;
    float sun_theta, sun_phi, theta2, theta3, T, T2, chi, zenith_Y, zenith_x, zenith_y, sd[3];
    sm = sm * 15.0;
    solar_time = time_of_day
        + (0.170 * sin(4.0 * LH_SKY_PI * (julian_day - 80) / 373)
           - 0.129 * sin(2.0 * LH_SKY_PI * (julian_day - 8) / 355))
        + 12.0 * (LH_SKY_DEG2RAD(sm) - LH_SKY_DEG2RAD(longitude)) / LH_SKY_PI;
    solar_declination = (0.4093 * sin(2.0 * LH_SKY_PI * (julian_day - 81) / 368));
    solar_altitude = asin(sin(LH_SKY_DEG2RAD(latitude)) * sin(solar_declination) -
                          cos(LH_SKY_DEG2RAD(latitude)) * cos(solar_declination) * cos(LH_SKY_PI * solar_time / 12));
    opp = -cos(solar_declination) * sin(LH_SKY_PI * solar_time / 12);
    adj = -(cos(LH_SKY_DEG2RAD(latitude)) * sin(solar_declination) +
            sin(LH_SKY_DEG2RAD(latitude)) * cos(solar_declination) * cos(LH_SKY_PI * solar_time / 12));
    solar_azimuth = atan2(opp, adj);
    sun_phi = -solar_azimuth;
    sun_theta = LH_SKY_PI / 2.0 - solar_altitude;
    s->sun_theta = sun_theta; s->sun_phi = sun_phi;
    sd[0] = cos(sun_phi) * sin(sun_theta);
    sd[1] = sin(sun_phi) * sin(sun_theta);
    sd[2] = cos(sun_theta);
    s->sun_dir[0] = sd[0]; s->sun_dir[1] = sd[2]; s->sun_dir[2] = sd[1];          /* swap y and z */
    theta2 = sun_theta * sun_theta;
    theta3 = theta2 * sun_theta;
    T = turb;
    T2 = turb * turb;
    chi = (4.0 / 9.0 - T / 120.0) * (LH_SKY_PI - 2.0 * sun_theta);
    zenith_Y = (4.0453 * T - 4.9710) * tan(chi) - 0.2155 * T + 2.4192;
    zenith_Y *= 1000;
    zenith_x = (0.00165 * theta3 - 0.00374 * theta2 + 0.00208 * sun_theta + 0) * T2 +
               (-0.02902 * theta3 + 0.06377 * theta2 - 0.03202 * sun_theta + 0.00394) * T +
               (0.11693 * theta3 - 0.21196 * theta2 + 0.06052 * sun_theta + 0.25885);
    zenith_y = (0.00275 * theta3 - 0.00610 * theta2 + 0.00316 * sun_theta + 0) * T2 +
               (-0.04212 * theta3 + 0.08970 * theta2 - 0.04153 * sun_theta + 0.00515) * T +
               (0.15346 * theta3 - 0.26756 * theta2 + 0.06669 * sun_theta + 0.26688);
    s->perez_Y[0] = 0.17872 * T - 1.46303;
    s->perez_Y[1] = -0.35540 * T + 0.42749;
    s->perez_Y[2] = -0.02266 * T + 5.32505;
    s->perez_Y[3] = 0.12064 * T - 2.57705;
    s->perez_Y[4] = -0.06696 * T + 0.37027;
    s->perez_x[0] = -0.01925 * T - 0.25922;
    s->perez_x[1] = -0.06651 * T + 0.00081;
    s->perez_x[2] = -0.00041 * T + 0.21247;
    s->perez_x[3] = -0.06409 * T - 0.89887;
    s->perez_x[4] = -0.00325 * T + 0.04517;
    s->perez_y[0] = -0.01669 * T - 0.26078;
    s->perez_y[1] = -0.09495 * T + 0.00921;
    s->perez_y[2] = -0.00792 * T + 0.21023;
    s->perez_y[3] = -0.04405 * T - 1.65369;
    s->perez_y[4] = -0.01092 * T + 0.05291;
    s->zenith_x = zenith_x; s->zenith_y = zenith_y; s->zenith_Y = zenith_Y;
#undef LH_SKY_DEG2RAD
}
#endif

#endif
