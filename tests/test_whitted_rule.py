"""lucille_amd/csrc/lh_whitted.h -- the bounce of the refraction chain the device kernel and host C share -- checked without a GPU.

  1a. a small stand-alone C program runs lh_whitted_bounce over the cases below; its doubles equal a numpy restatement of the rule
      (tests/whitted_chain.py) bit for bit.  The same program is built once more with -fsanitize=address,undefined and run.
  1b. the same cases against tests/golden/whitted_bounce.npz: the direction and the total-reflection flag the COMPILED REFERENCE's
      ri_refract (src/render/reflection.c:69-128) returned for them (tests/golden/make_whitted_golden.py wrote it); where
      oracle/_ref/liblucille_ref.so is present the reference is also called live.

Cases (seeded), each with eta 1.33, 1.0 and 0.75: unit I with unit n; n of length 0.5 - 2; cos1 of both signs, exactly 0 and a few ulps
around it; angles within 1e-3 .. 1e-15 of the total-reflection limit on both sides (leaving with eta > 1, entering with eta < 1); coeff
exactly 0 (eta 1 at cos1 = 0); n = 0; I = 0 and a tiny I with n = 0, where the result is too short to be normalised."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import whitted_chain as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lucille_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "whitted_bounce.npz")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "liblucille_ref.so")
ETAS = (1.33, 1.0, 0.75)


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def cases():
    """(I [m, 3], n [m, 3], eta [m], P [m, 3], eps [m]) -- reproducible from the seed"""
    rng = np.random.default_rng(20251)
    I, N = [], []
    a = _unit(rng.standard_normal((600, 3))); b = _unit(rng.standard_normal((600, 3)))
    I.append(a); N.append(b)                                                          # unit I, unit n: both signs of cos1
    I.append(a); N.append(b * rng.uniform(0.5, 2.0, 600)[:, None])                     # n of length 0.5 - 2
    # cos1 exactly 0, and a few ulps either side of it
    ax = np.eye(3)
    for i in range(3):
        for j in range(3):
            if i != j:
                for ln in (1.0, 0.5, 2.0):
                    I.append(ax[i][None]); N.append(ln * ax[j][None])
                    for tiny in (5e-324, -5e-324, 1e-300, -1e-300, 2.0 ** -52, -2.0 ** -52):
                        v = ln * ax[j].copy(); v[i] = tiny
                        I.append(ax[i][None]); N.append(v[None])
    # angles around the total-reflection limit: sin(limit) = 1 / e for e > 1; I in the plane of n = +z and x, leaving (I.n > 0) and entering (I.n < 0)
    for e in (1.33, 1.0 / 0.75, 1.0 / 1.33, 0.75, 1.0):
        lim = np.arcsin(min(1.0, 1.0 / e)) if e >= 1.0 else np.arcsin(e)
        for d in (0.0, 1e-3, -1e-3, 1e-6, -1e-6, 1e-9, -1e-9, 1e-12, -1e-12, 1e-15, -1e-15):
            th = lim + d
            for sgn in (1.0, -1.0):
                for ln in (1.0, 0.7, 1.9):
                    I.append(np.array([[np.sin(th), 0.0, sgn * np.cos(th)]])); N.append(np.array([[0.0, 0.0, ln]]))
    I.append(_unit(rng.standard_normal((40, 3)))); N.append(np.zeros((40, 3)))          # n = 0
    I.append(np.zeros((4, 3))); N.append(np.concatenate([np.zeros((2, 3)), _unit(rng.standard_normal((2, 3)))]))      # I = 0: nothing to normalise
    I.append(1e-10 * _unit(rng.standard_normal((6, 3)))); N.append(np.zeros((6, 3)))   # a tiny I, n = 0: norm^2 = 1e-20 stays below the threshold
    I = np.concatenate(I); N = np.concatenate(N); m = I.shape[0]
    I = np.tile(I, (len(ETAS), 1)); N = np.tile(N, (len(ETAS), 1)); eta = np.repeat(np.array(ETAS), m)
    P = rng.uniform(-2.0, 2.0, I.shape)
    eps = np.where(np.arange(I.shape[0]) % 3 == 0, 1.0e-7, np.where(np.arange(I.shape[0]) % 3 == 1, 0.0, 1.0e-3))
    return tuple(np.ascontiguousarray(x, np.float64) for x in (I, N, eta, P, eps))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def restated(cs):
    I, N, eta, P, eps = cs
    R, tir = wc.refract_np(I, N, eta)
    return P + eps[:, None] * R, R, tir


def test_the_cases_cover_what_they_claim():
    I, N, eta, P, eps = cases()
    cos1 = (I[:, 0] * N[:, 0] + I[:, 1] * N[:, 1]) + I[:, 2] * N[:, 2]
    _, R, tir = restated((I, N, eta, P, eps))
    ent = cos1 < 0
    e = np.where(ent, 1.0 / eta, eta); c = np.abs(cos1)
    coeff = 1.0 - (e * e) * (1.0 - c * c)
    n2 = (R * R).sum(axis=1)
    for x in ETAS:
        k = eta == x
        assert (cos1[k] < 0).sum() > 100 and (cos1[k] > 0).sum() > 100 and (cos1[k] == 0).sum() >= 18
    assert (tir & ent).sum() > 20 and (tir & ~ent & (cos1 > 0)).sum() > 20 and (~tir).sum() > 1000
    assert (coeff == 0.0).sum() >= 18                       # coeff exactly 0: the <= of the rule
    assert ((coeff > 0) & (coeff < 1e-8)).sum() >= 4 and ((coeff < 0) & (coeff > -1e-8)).sum() >= 4          # both sides of the limit, closely
    assert (n2 <= wc.NORM_MIN).sum() >= 10                   # results that are not normalised
    assert ((N == 0).all(axis=1)).sum() >= 100
    ln = np.linalg.norm(N, axis=1)
    assert ((ln > 0.5) & (ln < 0.9)).sum() > 50 and (ln > 1.5).sum() > 50


# ---- 1a: the header, compiled ---------------------------------------------------------------------------------------------------
PROGRAM = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "lucille_hip.h"
#include "lh_whitted.h"

/* in: int32 m, then m records of 11 doubles (I, n, eta, P, eps).  out: m records of 7 doubles (org, dir, total-reflection flag) */
int main(int argc, char **argv)
{
    FILE *in, *out; int32_t m, i; double *rec;
    const lh_whitted_params_t def = LH_WHITTED_DEFAULTS;
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    if (fread(&m, 4, 1, in) != 1 || m < 0) return 2;
    rec = (double *)malloc(sizeof(double) * 11 * (size_t)m + 8);
    if (!rec || fread(rec, sizeof(double) * 11, (size_t)m, in) != (size_t)m) return 2;
    for (i = 0; i < m; i++) {
        const double *r = rec + 11 * (size_t)i;
        double res[7], again[3];
        res[6] = (double)lh_whitted_bounce(r + 7, r + 3, r, r[10], r[6], res, res + 3);
        if (lh_whitted_refract(r, r + 3, r[6], again) != (int)res[6]) return 3;          /* the direction alone: the same function */
        if (fwrite(res, sizeof(double), 7, out) != 7) return 2;
    }
    /* the parameter check: the defaults pass; what the entry points refuse does not */
    if (!lh_whitted_params_ok(def.eps, def.eta, def.max_depth, def.reserved)) return 4;
    if (!lh_whitted_params_ok(0.0, 1.0e-300, 0, 0) || !lh_whitted_params_ok(1.0, 1.0e300, 64, 0)) return 4;
    if (lh_whitted_params_ok(-1.0e-300, 1.33, 8, 0) || lh_whitted_params_ok(1.0e-7, 0.0, 8, 0) || lh_whitted_params_ok(1.0e-7, -1.0, 8, 0)) return 5;
    if (lh_whitted_params_ok(1.0e-7, 1.33, -1, 0) || lh_whitted_params_ok(1.0e-7, 1.33, 65, 0) || lh_whitted_params_ok(1.0e-7, 1.33, 8, 1)) return 5;
    { const double z = 0.0, nan = z / z, inf = 1.0 / z;
      if (lh_whitted_params_ok(nan, 1.33, 8, 0) || lh_whitted_params_ok(1.0e-7, nan, 8, 0) || lh_whitted_params_ok(inf, 1.33, 8, 0) ||
          lh_whitted_params_ok(1.0e-7, inf, 8, 0) || lh_whitted_params_ok(-inf, 1.33, 8, 0)) return 5; }
    free(rec); fclose(in); fclose(out);
    printf("%d bounces\n", (int)m);
    return 0;
}
'''


def _build(tmp_path, name, extra):
    src = tmp_path / "whitted_rule.c"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call(["cc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
                          + extra + [str(src), "-o", str(exe), "-lm"])
    return str(exe)


def _run(exe, tmp_path, cs):
    I, N, eta, P, eps = cs
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    rec = np.concatenate([I, N, eta[:, None], P, eps[:, None]], axis=1)
    with open(fin, "wb") as f:
        f.write(np.int32(rec.shape[0]).tobytes()); f.write(np.ascontiguousarray(rec, np.float64).tobytes())
    p = subprocess.run([exe, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stdout, (p.returncode, p.stdout[-4000:])
    got = np.fromfile(fout, np.float64).reshape(-1, 7)
    assert got.shape[0] == rec.shape[0]
    return got[:, 0:3], got[:, 3:6], got[:, 6] != 0.0


def _same(cs, got, exp, what):
    for name, g, e in zip(("org", "dir"), got[:2], exp[:2]):
        bad = np.nonzero((bits(g) != bits(e)).any(axis=1))[0]
        assert bad.size == 0, "%s: %s of %d of %d bounces differ, first: I %r n %r eta %r: %r vs %r" % (
            what, name, bad.size, g.shape[0], cs[0][bad[0]], cs[1][bad[0]], cs[2][bad[0]], g[bad[0]], e[bad[0]])
    assert np.array_equal(got[2], exp[2]), what


def test_the_header_equals_the_restatement(tmp_path):
    cs = cases()
    assert cs[0].shape[0] >= 4000
    _same(cs, _run(_build(tmp_path, "whitted_rule", []), tmp_path, cs), restated(cs), "lh_whitted.h")


def test_the_same_program_under_the_sanitizers(tmp_path):
    """addresses and undefined behaviour (the double -> float conversion of a huge dot product is not among the cases: the rule's inputs
    are unit directions and normals of moderate length): a stand-alone executable"""
    try:
        exe = _build(tmp_path, "whitted_rule_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("cc could not build the program with -fsanitize=address,undefined")
    cs = cases()
    _same(cs, _run(exe, tmp_path, cs), restated(cs), "lh_whitted.h under the sanitizers")


# ---- 1b: the compiled reference -------------------------------------------------------------------------------------------------
def reference_refract(lib, I, N, eta):
    """the compiled reference's int ri_refract(ri_vector_t out, const ri_vector_t in, const ri_vector_t n, ri_float_t eta), one call per
    case (ri_vector_t: four doubles)"""
    f = lib.ri_refract
    f.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double]; f.restype = C.c_int
    out = np.zeros((I.shape[0], 3)); tir = np.zeros(I.shape[0], bool)
    o = (C.c_double * 4)(); a = (C.c_double * 4)(); b = (C.c_double * 4)()
    for i in range(I.shape[0]):
        a[0:3] = I[i]; b[0:3] = N[i]; a[3] = 0.0; b[3] = 0.0
        o[0] = o[1] = o[2] = o[3] = 0.0
        tir[i] = f(o, a, b, float(eta[i])) != 0
        out[i] = o[0:3]
    return out, tir


def test_the_restatement_equals_the_compiled_reference_fixture():
    z = np.load(GOLDEN)
    cs = cases()
    # the fixture holds its own inputs: they are the cases of this file
    assert np.array_equal(bits(z["I"]), bits(cs[0])) and np.array_equal(bits(z["n"]), bits(cs[1])) and np.array_equal(bits(z["eta"]), bits(cs[2]))
    R, tir = wc.refract_np(cs[0], cs[1], cs[2])
    bad = np.nonzero((bits(R) != bits(z["R"])).any(axis=1))[0]
    assert bad.size == 0, "%d of %d differ from the reference, first: I %r n %r eta %r: %r vs %r" % (
        bad.size, R.shape[0], cs[0][bad[0]], cs[1][bad[0]], cs[2][bad[0]], R[bad[0]], z["R"][bad[0]])
    assert np.array_equal(tir, z["tir"])


def test_the_header_equals_the_compiled_reference_fixture(tmp_path):
    z = np.load(GOLDEN)
    cs = cases()
    org, R, tir = _run(_build(tmp_path, "whitted_rule", []), tmp_path, cs)
    assert np.array_equal(bits(R), bits(z["R"])) and np.array_equal(tir, z["tir"])
    assert np.array_equal(bits(org), bits(cs[3] + cs[4][:, None] * z["R"]))


@pytest.mark.skipif(not os.path.exists(REFLIB), reason="oracle/_ref/liblucille_ref.so is not built here")
def test_the_restatement_equals_the_compiled_reference_live():
    lib = C.CDLL(REFLIB)
    cs = cases()
    exp, etir = reference_refract(lib, cs[0], cs[1], cs[2])
    R, tir = wc.refract_np(cs[0], cs[1], cs[2])
    assert np.array_equal(bits(R), bits(exp)), int((bits(R) != bits(exp)).any(axis=1).sum())
    assert np.array_equal(tir, etir)
