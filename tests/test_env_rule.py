"""lucille_amd/csrc/lh_env.h -- the rule of the environment-lit gather that the resolve kernels and host C share -- checked by a small C
program against a restatement written here (volatile temporaries: nothing contracted, nothing reordered):

  the value of a hit -- per channel the colours of the rays that are not occluded, added in r order in fp64, times scale, over N, stored
  as float -- and its count of occluded rays equal the restatement bit for bit over 2 000 seeded cases, N = 1 .. 100, channel values in
  [0, 1e4]; so do the cases all rays occluded (three zeros, count N), none occluded, and scale 0;
  the parameter check accepts exactly: both finite, eps >= 0, scale >= 0 -- over every pair of the specials of tests/test_dirt_rule.py
  and 100 000 seeded bit patterns -- and refuses every NaN;
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
#include <stdlib.h>
#include <string.h>
#include "lh_env.h"

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double unit(void) { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static long nfail = 0, nchecked = 0;
#define CHECK(c, a, b) do { if (!(c)) { if (nfail++ < 20) printf("FAIL %s at %a %a\n", #c, (double)(a), (double)(b)); } } while (0)

/* the restatement: the header's contract, channel by channel */
static float restated(const uint8_t *occ, const float *rad, int N, double scale, int k, uint32_t *count)
{
    volatile double sum = 0.0, m, q;
    volatile float f;
    uint32_t c = 0; int r;
    for (r = 0; r < N; r++) {
        if (occ[r]) { c++; continue; }
        sum = sum + (double)rad[3 * r + k];
    }
    m = scale * sum; q = m / (double)N; f = (float)q;
    *count = c;
    return f;
}

static int same(float a, float b) { return memcmp(&a, &b, 4) == 0; }

/* mode 0: seeded bytes; 1: all occluded; 2: none.  The arrays are allocated at their exact size: a read past N is the sanitizer's to see */
static void hit(int N, double scale, int mode)
{
    uint8_t *occ = (uint8_t *)malloc((size_t)N);
    float *rad = (float *)malloc(sizeof(float) * 3 * (size_t)N), got[3] = {-1.0f, -1.0f, -1.0f};
    uint32_t c = 77u, ce = 0; int k, r;
    for (r = 0; r < N; r++) {
        occ[r] = mode == 1 ? 1 : (mode == 2 ? 0 : (uint8_t)((rnd() % 16) < 9 ? ((rnd() & 1) ? 1 : 255) : 0));      /* any non-zero byte is "occluded" */
        for (k = 0; k < 3; k++) rad[3 * r + k] = (float)(1.0e4 * unit() * ((rnd() & 3) ? unit() : 1.0));
    }
    lh_env_value(occ, rad, N, scale, &c, got);
    nchecked++;
    for (k = 0; k < 3; k++) {
        const float e = restated(occ, rad, N, scale, k, &ce);
        CHECK(same(got[k], e) && c == ce, N, scale);
        if (mode == 1) CHECK(same(got[k], 0.0f) && c == (uint32_t)N, N, scale);
        if (mode == 2) CHECK(c == 0u, N, scale);
        if (scale == 0.0) CHECK(same(got[k], 0.0f), N, scale);
    }
    free(occ); free(rad);
}

static int ok_restated(double e, double m) { return isfinite(e) && isfinite(m) && e >= 0.0 && m >= 0.0; }

int main(void)
{
    long i; int k, j, N;
    const double specials[] = {0.0, -0.0, DBL_TRUE_MIN, DBL_MIN, 1.0e-6, 0.1, 0.5, 1.0, 1.0e38, nextafter(1.0e38, INFINITY), 1.0e39, DBL_MAX,
                               INFINITY, -INFINITY, NAN, -DBL_TRUE_MIN, -0.1, -1.0};
    const int ns = (int)(sizeof(specials) / sizeof(specials[0]));
    for (i = 0; i < 2000; i++) hit((int)(rnd() % 100) + 1, (rnd() & 1) ? 1.0 : ((rnd() & 1) ? 0.3183098861837907 : 4.0 * unit()), 0);
    for (N = 1; N <= 100; N++) { hit(N, 1.0, 1); hit(N, 0.3183098861837907, 2); hit(N, 0.0, 0); hit(N, 0.0, 2); }
    /* the pieces the kernels call: one add, one finish */
    { volatile double a = 0.1, b; volatile float f; b = a + (double)0.7f; CHECK(lh_env_add(0.1, 0.7f) == b, 0, 0);
      b = 0.3183098861837907 * 12.5; b = b / 16.0; f = (float)b; CHECK(same(lh_env_finish(0.3183098861837907, 12.5, 16), f), 0, 0); nchecked++; }
    /* the parameter check: every pair of the specials, and seeded bit patterns */
    for (k = 0; k < ns; k++) for (j = 0; j < ns; j++) {
        nchecked++;
        CHECK(lh_env_params_ok(specials[k], specials[j]) == ok_restated(specials[k], specials[j]), specials[k], specials[j]);
    }
    for (i = 0; i < 100000; i++) {
        double e, m; uint64_t w;
        w = rnd(); memcpy(&e, &w, 8); w = rnd(); memcpy(&m, &w, 8);
        if (rnd() & 1) { e = fabs(e); m = fabs(m); }
        nchecked++;
        CHECK(lh_env_params_ok(e, m) == ok_restated(e, m), e, m);
    }
    CHECK(LH_ENV_EPS_DEFAULT == 1.0e-5 && LH_ENV_SCALE_DEFAULT == 1.0 && lh_env_params_ok(LH_ENV_EPS_DEFAULT, LH_ENV_SCALE_DEFAULT), 0, 0);
    /* the self-primitive skip: from AO's offset on */
    CHECK(lh_env_selfskip(1.0e-6) && lh_env_selfskip(1.0e-5) && !lh_env_selfskip(nextafter(1.0e-6, 0.0)) && !lh_env_selfskip(0.0), 0, 0);
    printf("%ld cases checked, %ld failures\n", nchecked, nfail);
    return nfail ? 1 : 0;
}
'''


def _build(tmp_path, name, extra):
    src = tmp_path / "env_rule.c"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call(["cc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC] + extra + [str(src), "-o", str(exe), "-lm"])
    return str(exe)


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    n = int(p.stdout.strip().splitlines()[-1].split()[0])
    assert n >= 2000 + 400 + 18 * 18 + 100000, p.stdout
    return p.stdout


def test_the_rule_over_seeded_cases_and_its_edges(tmp_path):
    out = _run(_build(tmp_path, "env_rule", []))
    assert "0 failures" in out


def test_the_same_program_under_the_sanitizers(tmp_path):
    """addresses (the N bytes and 3 N floats of a hit, allocated at their exact size) and undefined behaviour: a stand-alone executable"""
    try:
        exe = _build(tmp_path, "env_rule_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("cc could not build the program with -fsanitize=address,undefined")
    out = _run(exe)
    assert "0 failures" in out and "runtime error" not in out
