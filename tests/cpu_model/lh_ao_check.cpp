/* the built-in gather sampler (lucille_amd/csrc/lh_ao.h, included unchanged) as a stand-alone program: tests/test_ao_sampler_rule.py feeds it
 * (seed, key, grid, ray, hit record) rows and compares what it writes, bit for bit, with tests/ao_sampler.py.  lh_ao_check IN OUT
 * IN:  uint64 count; per case: case_t
 * OUT: per case: 6 doubles -- origin, direction
 * The device's sincospif is replaced by one that takes fp64 sin / cos of the reduced argument and rounds once: the argument 2 z1 lies in [0, 2] and is
 * exact, n = the nearest multiple of 1/2 and f = x - n / 2 are exact, and the multiples of 1/2 give exact 0 and +-1. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static inline void host_sincospif(float xf, float *s, float *c)
{
    double x = (double)xf;
    if (x >= 2.0) x -= 2.0;
    const double n = nearbyint(x * 2.0), f = x - n * 0.5;
    const double sn = sin(3.141592653589793 * f), cs = cos(3.141592653589793 * f);
    double so, co;
    switch ((long long)n & 3) {
    case 0: so = sn; co = cs; break;
    case 1: so = cs; co = -sn; break;
    case 2: so = -sn; co = -cs; break;
    default: so = -cs; co = sn; break;
    }
    *s = (float)so; *c = (float)co;
}

#define __device__
#define __forceinline__ inline
#define sincospif host_sincospif
#include "../../lucille_amd/csrc/lh_ao.h"

typedef struct { uint64_t seed, key; int32_t ntheta, nphi, r, pad; double h[LH_HITREC_DOUBLES]; } case_t;

static void die(const char *what) { fprintf(stderr, "lh_ao_check: %s\n", what); exit(2); }

int main(int argc, char **argv)
{
    uint64_t count;
    if (argc != 3) die("usage: lh_ao_check IN OUT");
    if (sizeof(case_t) != 128) die("struct sizes");
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) die("cannot open IN or OUT");
    if (fread(&count, sizeof(count), 1, f) != 1) die("short input");
    for (uint64_t k = 0; k < count; k++) {
        case_t c;
        double o[6];
        if (fread(&c, sizeof(c), 1, f) != 1) die("short input");
        if (c.ntheta < 1 || c.nphi < 1 || c.r < 0 || c.r >= c.ntheta * c.nphi) die("bad case");
        lh_ao_ray_builtin(c.h, c.key, c.seed, c.ntheta, c.nphi, c.r, o[0], o[1], o[2], o[3], o[4], o[5]);
        if (fwrite(o, sizeof(o), 1, g) != 1) die("short write");
    }
    if (fclose(g) != 0) die("short write");
    fclose(f);
    return 0;
}
