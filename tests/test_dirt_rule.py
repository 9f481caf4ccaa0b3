"""lucille_amd/csrc/lh_dirt.h -- the rule of the dirtmap transport that the resolve kernels and host C share -- checked by a small C
program against a restatement written here, over the edges (t at 0, at the near clip, at the neighbours of both clips, at the far
clip, at 1e38; near = 0; far - near a denormal) and 400 000 seeded values:

  the weight c of a gather ray is in [0, 1], exactly 0 for t <= near, exactly 1 for a miss (t >= far: the bounded record's 1e38 included);
  c is monotone in t;  c equals the restatement bit for bit, and so does the value of a hit (sum in r order, / N) with its count;
  the parameter check accepts exactly: all finite, 0 <= near < far <= 1e38, eps >= 0 -- and refuses every NaN;
  the self-primitive skip is kept exactly from eps = 1e-6 on.

The same program is built once more with -fsanitize=address,undefined as a stand-alone executable and run."""
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
#include "lh_dirt.h"

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double unit(void) { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static long nfail = 0, nchecked = 0;
#define CHECK(c, t, n, f) do { if (!(c)) { if (nfail++ < 20) printf("FAIL %s at t = %a near = %a far = %a\n", #c, (t), (n), (f)); } } while (0)

/* the restatement: the issue's table, with volatile temporaries so that nothing is contracted or reordered */
static double restated(double t, double nearc, double farc)
{
    volatile double a, b, q, x, p, c;
    if (!(t < farc)) return 1.0;            /* a miss, or a hit at or beyond the far clip */
    if (t <= nearc) return 0.0;
    a = t - nearc; b = farc - nearc; q = a / b; x = 1.0 - q;
    p = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    c = 1.0 - p;
    return c;
}

static int same(double a, double b) { return memcmp(&a, &b, 8) == 0; }

static void check(double t, double nearc, double farc)
{
    const double c = lh_dirt_weight(t, nearc, farc);
    nchecked++;
    CHECK(c >= 0.0 && c <= 1.0, t, nearc, farc);
    CHECK(same(c, restated(t, nearc, farc)), t, nearc, farc);
    if (t <= nearc) CHECK(same(c, 0.0), t, nearc, farc);
    if (!(t < farc)) CHECK(same(c, 1.0), t, nearc, farc);
    CHECK(lh_dirt_hit(t, farc) == (t < farc), t, nearc, farc);
    /* monotone: the next doubles on either side */
    if (t > 0.0) CHECK(lh_dirt_weight(nextafter(t, 0.0), nearc, farc) <= c, t, nearc, farc);
    CHECK(lh_dirt_weight(nextafter(t, INFINITY), nearc, farc) >= c, t, nearc, farc);
}

static void clips(double nearc, double farc)
{
    double t; int k;
    if (!lh_dirt_params_ok(nearc, farc, 1.0e-5)) { printf("FAIL clips(%a, %a) refused\n", nearc, farc); nfail++; return; }
    check(0.0, nearc, farc); check(DBL_TRUE_MIN, nearc, farc); check(nearc, nearc, farc); check(farc, nearc, farc); check(1.0e38, nearc, farc);
    check(0.5 * (nearc + farc), nearc, farc);
    t = nearc; for (k = 0; k < 3; k++) { t = nextafter(t, INFINITY); check(t, nearc, farc); }
    t = nearc; for (k = 0; k < 3 && t > 0.0; k++) { t = nextafter(t, 0.0); check(t, nearc, farc); }
    t = farc; for (k = 0; k < 3; k++) { t = nextafter(t, INFINITY); check(t, nearc, farc); }
    t = farc; for (k = 0; k < 3; k++) { t = nextafter(t, 0.0); check(t, nearc, farc); }
    /* monotone over a sweep between the clips */
    { double prev = 0.0; for (k = 0; k <= 64; k++) { const double c = lh_dirt_weight(nearc + (farc - nearc) * (k / 64.0), nearc, farc); CHECK(c >= prev, (double)k, nearc, farc); prev = c; } }
}

static int ok_restated(double n, double f, double e)
{
    return isfinite(n) && isfinite(f) && isfinite(e) && 0.0 <= n && n < f && f <= 1.0e38 && e >= 0.0;
}

int main(void)
{
    long i; int k, j, l;
    const double specials[] = {0.0, -0.0, DBL_TRUE_MIN, DBL_MIN, 1.0e-6, 0.1, 0.5, 1.0, 1.0e38, nextafter(1.0e38, INFINITY), 1.0e39, DBL_MAX,
                               INFINITY, -INFINITY, NAN, -DBL_TRUE_MIN, -0.1, -1.0};
    const int ns = (int)(sizeof(specials) / sizeof(specials[0]));
    /* edges */
    clips(0.1, 0.5); clips(0.0, 0.5); clips(0.0, 1.0e38); clips(0.1, 1.0e38); clips(0.0, DBL_TRUE_MIN); clips(0.0, DBL_MIN);
    clips(1.0, nextafter(1.0, 2.0)); clips(0.25, nextafter(0.25, 1.0));
    clips(DBL_TRUE_MIN, 3 * DBL_TRUE_MIN);                 /* far - near a denormal */
    clips(DBL_MIN, DBL_MIN + 5 * DBL_TRUE_MIN);             /* ... between normals */
    clips(nextafter(1.0e38, 0.0), 1.0e38);
    /* seeded values: clips over forty binades, t below, between and beyond them */
    for (i = 0; i < 100000; i++) {
        const double farc = ldexp(unit() + 0.5, (int)(rnd() % 40) - 20), nearc = (rnd() & 7) ? farc * unit() : 0.0;
        if (!(nearc < farc)) continue;
        check(farc * 2.0 * unit(), nearc, farc);
        check(nearc + (farc - nearc) * unit(), nearc, farc);
        check(nearc * unit(), nearc, farc);
        check((rnd() & 1) ? 1.0e38 : farc * (1.0 + unit()), nearc, farc);
    }
    /* the value of a hit: the sum in r order, then / N, and the count of bounded hits */
    for (i = 0; i < 2000; i++) {
        double t[64]; volatile double sum = 0.0, val; uint32_t nh = 0, got = 77u; int N = (int)(rnd() % 8) + 1; N *= N;
        const double farc = 0.5 + unit(), nearc = 0.4 * unit();
        for (k = 0; k < N; k++) { const uint64_t w = rnd() % 4; t[k] = w == 0 ? 1.0e38 : (w == 1 ? nearc * unit() : 2.0 * unit()); }
        for (k = 0; k < N; k++) { if (t[k] < farc) nh++; sum = sum + restated(t[k], nearc, farc); }
        val = sum / (double)N;
        nchecked++;
        CHECK(same(lh_dirt_value(t, N, nearc, farc, &got), val) && got == nh, (double)N, nearc, farc);
    }
    /* the parameter check: every triple of the specials, and seeded triples */
    for (k = 0; k < ns; k++) for (j = 0; j < ns; j++) for (l = 0; l < ns; l++) {
        nchecked++;
        CHECK(lh_dirt_params_ok(specials[k], specials[j], specials[l]) == ok_restated(specials[k], specials[j], specials[l]), specials[l], specials[k], specials[j]);
    }
    for (i = 0; i < 100000; i++) {
        double n, f, e; uint64_t w;
        w = rnd(); memcpy(&n, &w, 8); w = rnd(); memcpy(&f, &w, 8); w = rnd(); memcpy(&e, &w, 8);
        if (rnd() & 1) { n = fabs(n); f = fabs(f); e = fabs(e); }
        nchecked++;
        CHECK(lh_dirt_params_ok(n, f, e) == ok_restated(n, f, e), e, n, f);
    }
    { const struct { double n, f, e; } d = {LH_DIRT_NEAR_DEFAULT, LH_DIRT_FAR_DEFAULT, LH_DIRT_EPS_DEFAULT};
      CHECK(d.n == 0.1 && d.f == 0.5 && d.e == 1.0e-5 && lh_dirt_params_ok(d.n, d.f, d.e), d.e, d.n, d.f); }
    /* the self-primitive skip: from AO's offset on */
    CHECK(lh_dirt_selfskip(1.0e-6) && lh_dirt_selfskip(1.0e-5) && !lh_dirt_selfskip(nextafter(1.0e-6, 0.0)) && !lh_dirt_selfskip(0.0), 0.0, 0.0, 0.0);
    printf("%ld values checked, %ld failures\n", nchecked, nfail);
    return nfail ? 1 : 0;
}
'''


def _build(tmp_path, name, extra):
    src = tmp_path / "dirt_rule.c"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call(["cc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC] + extra + [str(src), "-o", str(exe), "-lm"])
    return str(exe)


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    n = int(p.stdout.strip().splitlines()[-1].split()[0])
    assert n >= 400000, p.stdout
    return p.stdout


def test_the_rule_over_the_edges_and_seeded_values(tmp_path):
    out = _run(_build(tmp_path, "dirt_rule", []))
    assert "0 failures" in out


def test_the_same_program_under_the_sanitizers(tmp_path):
    """addresses (the N doubles of a hit) and undefined behaviour: a stand-alone executable"""
    try:
        exe = _build(tmp_path, "dirt_rule_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("cc could not build the program with -fsanitize=address,undefined")
    out = _run(exe)
    assert "0 failures" in out and "runtime error" not in out
