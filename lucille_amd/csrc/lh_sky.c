/*
 * lh_sky.c -- lh_sky_from_site: the host-only part of the sun-and-sky light (lh_sky.h), plain C so that its float arithmetic is the
 * reference's (src/render/sunsky.c:39-75,183-307) as the C compiler evaluates it.
 */
#include "lh_sky.h"

int lh_sky_from_site(lh_sky_t *sky, float latitude, float longitude, float standard_meridian, int julian_day, float time_of_day, float turbidity)
{
    if (!sky) return -1;
    if (!(lh_sky_fin(latitude) && lh_sky_fin(longitude) && lh_sky_fin(standard_meridian) && lh_sky_fin(time_of_day) && lh_sky_fin(turbidity))) return -1;
    lh_sky_site(sky, latitude, longitude, standard_meridian, julian_day, time_of_day, turbidity);
    return 0;
}
