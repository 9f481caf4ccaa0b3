"""lucille_amd/csrc/lh_tmax.h -- the scalar pieces of the per-ray maximum distance that host C and the kernels share -- checked by a
small C program over 1.2 million seeded doubles and the edges (0, -0, denormals, the neighbours of powers of two, 1e38, 1e300, +inf,
NaN, negatives, floats widened):

  the fp32 bound, read as a real number, is >= tmax (>= 1e38f where tmax lies above that: the clamp) and <= 1e38f, and never a denormal;
  the certain-hit threshold is < tmax;
  dead bounds are exactly NaN and everything <= 0;
  the near-bound fragility test holds for every t in [tmax (1 - LH_FRAGILE_REL), tmax);
  best.t starts at min(tmax, 1e38); the final accept is t < tmax.

The same program is built once more with -fsanitize=undefined,address as a stand-alone executable and run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lucille_amd", "csrc")

PROGRAM = r'''
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "lh_reftrace.h"      /* LH_FRAGILE_REL */
#include "lh_tmax.h"

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static long nfail = 0, nchecked = 0;
#define CHECK(c, x) do { if (!(c)) { if (nfail++ < 20) printf("FAIL %s at tmax = %a (%g)\n", #c, (x), (x)); } } while (0)

static void check(double tmax)
{
    const float tb = lh_tmax_tb(tmax);
    const int dead = lh_tmax_dead(tmax);
    nchecked++;
    /* dead bounds are exactly NaN and <= 0 */
    CHECK(dead == (isnan(tmax) || tmax <= 0.0), tmax);
    if (dead) {
        CHECK(tb == -1.0f, tmax);
        CHECK(lh_tmax_sure_below(tb) < 0.0f, tmax);              /* no certain hit (t_hi >= 0) ends such a ray */
        CHECK(!lh_tmax_accept(0.0, tmax) && !lh_tmax_accept(DBL_TRUE_MIN, tmax) && !lh_tmax_accept(1.0, tmax), tmax);      /* no t >= 0 passes */
        return;
    }
    /* the fp32 bound: a normal float in [min(tmax, 1e38f), 1e38f] */
    CHECK(tb <= 1.0e38f, tmax);
    CHECK(tb >= FLT_MIN, tmax);
    CHECK((double)tb >= tmax || tb == 1.0e38f, tmax);
    if (tmax <= (double)1.0e38f) CHECK((double)tb >= tmax, tmax);
    /* ... and tight: at most one float above tmax, where it is not the clamp to the smallest normal */
    if (tmax >= (double)FLT_MIN && tmax <= (double)1.0e38f) CHECK((double)nextafterf(tb, 0.0f) < tmax, tmax);
    /* the certain-hit threshold is below tmax */
    CHECK((double)lh_tmax_sure_below(tb) < tmax, tmax);
    if (tb >= 1.0e-30f) CHECK(lh_tmax_sure_below(tb) > 0.999f * tb, tmax);     /* ... and not uselessly low */
    /* the start of best.t and the final accept */
    CHECK(lh_tmax_best0(tmax) == (tmax < 1.0e38 ? tmax : 1.0e38), tmax);
    CHECK(lh_tmax_accept(nextafter(tmax, 0.0), tmax) && !lh_tmax_accept(tmax, tmax) && !lh_tmax_accept(nextafter(tmax, INFINITY), tmax), tmax);
    /* near-bound fragility: every t in [tmax (1 - LH_FRAGILE_REL), tmax) is marked */
    if (!isinf(tmax)) {
        const long double lo = (long double)tmax * (1.0L - (long double)LH_FRAGILE_REL);
        double t = (double)lo; int k;
        if ((long double)t < lo) t = nextafter(t, INFINITY);                     /* the first double of the interval */
        for (k = 0; k < 4 && t < tmax; k++) { CHECK(lh_tmax_near(t, tmax), tmax); t = nextafter(t, INFINITY); }
        t = nextafter(tmax, 0.0);
        for (k = 0; k < 4 && (long double)t >= lo && t > 0.0; k++) { CHECK(lh_tmax_near(t, tmax), tmax); t = nextafter(t, 0.0); }
        for (k = 0; k < 4; k++) {
            const double f = (double)(rnd() >> 11) * (1.0 / 9007199254740992.0);
            t = (double)(lo + ((long double)tmax - lo) * (long double)f);
            if ((long double)t >= lo && t < tmax) CHECK(lh_tmax_near(t, tmax), tmax);
        }
        /* ... and the mark is not everywhere: far below the bound a hit keeps its flags */
        if (tmax >= DBL_MIN) CHECK(!lh_tmax_near(tmax * (1.0 - 1.0e-9), tmax), tmax);
    }
}

static void around(double x)
{
    double a = x, b = x; int k;
    check(x); check(-x);
    for (k = 0; k < 3; k++) { a = nextafter(a, INFINITY); b = nextafter(b, -INFINITY); check(a); check(b); }
}

int main(void)
{
    long i; int e;
    /* edges */
    around(0.0); check(-0.0); check(NAN); check(-NAN); check(INFINITY); check(-INFINITY);
    around(DBL_MIN); around(DBL_TRUE_MIN); around(DBL_MAX); around((double)FLT_MIN); around((double)FLT_TRUE_MIN); around((double)FLT_MAX);
    around(1.0e38); around((double)1.0e38f); around(1.0e300); around(1.0e-30); around((double)1.0e-30f); around(1.0); around(-1.0);
    for (e = -1074; e <= 1023; e++) around(ldexp(1.0, e));                       /* the neighbours of every power of two, denormals included */
    /* seeded doubles: every exponent (uniform bit patterns), and the range rays live in */
    for (i = 0; i < 600000; i++) { uint64_t w = rnd(); double x; memcpy(&x, &w, 8); check(x); }
    for (i = 0; i < 400000; i++) check(ldexp((double)(rnd() >> 11) * (1.0 / 9007199254740992.0) + 0.5, (int)(rnd() % 80) - 40));
    /* floats widened (the bounds of fp32 rays) */
    for (i = 0; i < 200000; i++) { uint32_t w = (uint32_t)rnd(); float f; memcpy(&f, &w, 4); check((double)f); }
    printf("%ld bounds checked, %ld failures\n", nchecked, nfail);
    return nfail ? 1 : 0;
}
'''


def _build(tmp_path, name, extra):
    src = tmp_path / "tmax_rule.c"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call(["cc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC] + extra + [str(src), "-o", str(exe), "-lm"])
    return str(exe)


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    n = int(p.stdout.strip().splitlines()[-1].split()[0])
    assert n >= 1000000, p.stdout
    return p.stdout


def test_the_rule_over_a_million_bounds_and_the_edges(tmp_path):
    out = _run(_build(tmp_path, "tmax_rule", []))
    assert "0 failures" in out


def test_the_same_program_under_the_sanitizers(tmp_path):
    """undefined behaviour (the float conversions, the bit increment of lh_tmax_tb) and addresses: a stand-alone executable"""
    try:
        exe = _build(tmp_path, "tmax_rule_san", ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("cc could not build the program with -fsanitize=undefined,address")
    out = _run(exe)
    assert "0 failures" in out and "runtime error" not in out
