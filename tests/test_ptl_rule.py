"""The rule of direct light at the path tracer's vertices (lucille_amd/csrc/lh_ptl.h: r = ((G kd) col) value in float32, and the vertex colour)
on the CPU: the header, compiled into the stand-alone program tests/cpu_model/lh_ptl_check.c with -fsanitize=address,undefined, against a
restatement in numpy, bit for bit, over random and edge inputs.

The restatement (direct, colour below) is what tests/test_gpu_pt_lit.py holds the device to."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_ptl_check.c")

CASE = np.dtype([("G", np.float32, (3,)), ("kd", np.float32, (3,)), ("col", np.float32, (3,)), ("value", np.float32, (3,)),
                 ("c", np.float64, (3, 3)), ("w", np.float64), ("u", np.float64), ("v", np.float64)])
OUT = np.dtype([("r", np.float32, (3,)), ("colour", np.float32, (3,))])


# ---- the rule, restated: every line one float32 operation per element, in the header's order -------------------------------------------------
def direct(G, kd, col, value):
    """r = ((G * kd) * col) * value: four float32 operands, three IEEE multiplies in this order"""
    G, kd, col, value = (np.asarray(x, np.float32) for x in (G, kd, col, value))
    with np.errstate(all="ignore"):
        a = G * kd
        b = a * col
        r = b * value
    assert r.dtype == np.float32
    return r


def colour(c0, c1, c2, u, v):
    """pt_scatter's three colour lines: w = 1 - u - v; (float)((c0 w + c1 u) + c2 v), in fp64; c0, c1, c2: [n, 3], u, v: [n]"""
    u = np.asarray(u, np.float64)[:, None]; v = np.asarray(v, np.float64)[:, None]
    with np.errstate(all="ignore"):
        w = 1.0 - u - v
        a = c0 * w
        b = c1 * u
        c = c2 * v
        return ((a + b) + c).astype(np.float32)


def _table():
    rng = np.random.default_rng(5)
    n = 6000
    t = np.zeros(n, CASE)
    # operands whose product depends on the association: mantissas spread over the whole range, magnitudes that over- and underflow in one order only
    for k in ("G", "kd", "col", "value"):
        t[k] = (rng.uniform(1.0, 2.0, (n, 3)) * 2.0 ** rng.integers(-6, 7, (n, 3))).astype(np.float32)
    t["col"][::3] *= rng.choice([-1.0, 1.0], (n // 3, 3)).astype(np.float32)                    # negative colours
    t["c"] = rng.uniform(-1.0, 2.0, (n, 3, 3))
    t["u"] = rng.uniform(0.0, 1.0, n); t["v"] = rng.uniform(0.0, 1.0, n) * (1.0 - t["u"])
    t["w"] = 1.0 - t["u"] - t["v"]
    e = 100
    t["G"][e:e + 50] = np.float32(1e30); t["kd"][e:e + 50] = np.float32(1e30); t["col"][e:e + 50] = np.float32(1e-30)     # (G kd) overflows, G (kd col) would not
    t["G"][e + 50:e + 100] = np.float32(1e-30); t["kd"][e + 50:e + 100] = np.float32(1e-30); t["col"][e + 50:e + 100] = np.float32(1e30)   # (G kd) underflows to 0
    t["value"][e + 100:e + 150, 0] = np.nan; t["value"][e + 150:e + 200, 1] = 0.0; t["value"][e + 200:e + 220, 2] = -0.0
    t["G"][e + 220:e + 240] = 1.0; t["G"][e + 240:e + 260, 1] = np.nan; t["kd"][e + 260:e + 280] = 0.0
    t["col"][e + 280:e + 300] = np.float32(-0.75); t["value"][e + 300:e + 320] = np.float32(np.inf)
    t["kd"][e + 300:e + 310] = 0.0                                                             # 0 x inf: NaN
    t["c"][e:e + 40] *= 1e300                                                                   # the sum overflows; the float conversion of a finite one too
    t["c"][e + 40:e + 80] *= 1e39
    t["c"][e + 80:e + 100, 1] = np.nan
    t["u"][e + 100:e + 120] = 1.0; t["v"][e + 100:e + 120] = 0.0; t["u"][e + 120:e + 140] = 0.0; t["v"][e + 120:e + 140] = 1.0
    t["w"] = 1.0 - t["u"] - t["v"]
    return t


def _build(tmp, src, name):
    exe = str(tmp / name)
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-sanitize=float-cast-overflow", src, "-o", exe, "-lm"])
    return exe


def _run(exe, tmp, table):
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint64(table.size).tobytes()); f.write(table.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    out = np.fromfile(fout, OUT)
    assert out.size == table.size
    return out


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    assert CASE.itemsize == 48 + 72 + 24 and OUT.itemsize == 24          # the C program's case_t and out_t
    d = tmp_path_factory.mktemp("ptl")
    t = _table()
    return t, _run(_build(d, SRC, "lh_ptl_check"), d, t)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_direct_bit_for_bit(rule):
    t, out = rule
    r = direct(t["G"], t["kd"], t["col"], t["value"])
    assert np.array_equal(bits(out["r"]), bits(r))
    # the association matters on these operands: the two other orders give other bits on many rows
    with np.errstate(all="ignore"):
        other1 = (t["G"] * (t["kd"] * t["col"])) * t["value"]
        other2 = (t["G"] * t["kd"]) * (t["col"] * t["value"])
        other3 = t["G"] * (t["kd"] * (t["col"] * t["value"]))
    for other in (other1, other2, other3):
        assert (bits(other) != bits(r)).any(axis=1).sum() >= 1000
    e = 100
    assert np.isinf(r[e:e + 50]).all() and np.isfinite(other1[e:e + 50]).all()              # (G kd) overflowed first
    assert (r[e + 50:e + 100] == 0.0).all() and (other1[e + 50:e + 100] != 0.0).all()      # ... or underflowed
    assert np.isnan(r[e + 100:e + 150, 0]).all() and (r[e + 150:e + 200, 1] == 0.0).all() and (r[e + 200:e + 220, 2] == 0.0).all()
    assert np.isnan(r[e + 240:e + 260, 1]).all() and (r[e + 260:e + 280] == 0.0).all()
    assert (r[e + 280:e + 300] < 0.0).all()                                                  # a negative colour gives a negative term: it is added as it is
    assert np.isnan(r[e + 300:e + 310]).all() and np.isinf(r[e + 310:e + 320]).all()


def test_colour_bit_for_bit(rule):
    t, out = rule
    col = colour(t["c"][:, 0], t["c"][:, 1], t["c"][:, 2], t["u"], t["v"])
    assert np.array_equal(bits(out["colour"]), bits(col))
    e = 100
    assert np.isinf(col[e + 40:e + 80]).any() and np.isnan(col[e + 80:e + 100]).any()
    # u = 1 / v = 1: the corner's own colour as a float
    assert np.array_equal(bits(col[e + 100:e + 120]), bits((t["c"][e + 100:e + 120, 0] * 0.0 + t["c"][e + 100:e + 120, 1] + t["c"][e + 100:e + 120, 2] * 0.0).astype(np.float32)))
