"""The rule of direct light (lucille_amd/csrc/lh_lights.h: the shadow ray of a hit to a light, its bound, its weight, a hit's mask and value) on the
CPU: the header, compiled into the stand-alone program tests/cpu_model/lh_lights_check.c with -fsanitize=address,undefined, against a restatement in
numpy, bit for bit, over random and edge inputs; and the light stage's plan (lh_gather.h, kind LH_GATHER_LIGHT) through tests/cpu_model/lh_gather_check.c.

The restatement (rays, weights, values below) is what tests/test_gpu_lights.py holds the device to."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_lights_check.c")
PLAN_SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_gather_check.c")

POINT, COSINE, INVSQ = 1, 2, 4
LMAX = 31
LIGHT = np.dtype([("v", np.float64, (3,)), ("rgb", np.float64, (3,)), ("flags", np.uint32), ("reserved", np.uint32)])
CASE = np.dtype([("P", np.float64, (3,)), ("Ns", np.float64, (3,)), ("eps", np.float64), ("L", np.uint32), ("pad", np.uint32), ("lights", LIGHT, (LMAX,)),
                 ("occ", np.uint8, (32,))])
OUT = np.dtype([("O", np.float64, (3,)), ("dir", np.float64, (LMAX, 3)), ("tmax_ray", np.float64, (LMAX,)), ("w", np.float64, (LMAX,)),
                ("tmax_item", np.float64, (LMAX,)), ("mask", np.uint32), ("ok", np.uint32), ("value", np.float32, (3,)), ("pad", np.uint32)])


# ---- the rule, restated: every line one fp64 operation per element, in the header's order ----------------------------------------------------
def origins(P, Ns, eps):
    """O[k] = P[k] + Ns[k] * eps"""
    with np.errstate(all="ignore"):
        return P + Ns * eps


def rays(O, v, flags):
    """the shadow ray of one light for every origin -> (dir [n, 3], tmax [n]: +inf directional, 1 point, 0 dark without a walk)"""
    n = O.shape[0]
    with np.errstate(all="ignore"):
        d = (np.asarray(v, np.float64)[None, :] - O) if flags & POINT else np.tile(np.asarray(v, np.float64), (n, 1))
    dark = ~np.isfinite(d).all(axis=1) | (d == 0.0).all(axis=1)
    return d, np.where(dark, 0.0, 1.0 if flags & POINT else np.inf)


def weights(Ns, d, flags):
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        w = np.ones(d.shape[0])
        if flags & COSINE:
            nn = (Ns[:, 0] * Ns[:, 0] + Ns[:, 1] * Ns[:, 1]) + Ns[:, 2] * Ns[:, 2]
            nd = (Ns[:, 0] * d[:, 0] + Ns[:, 1] * d[:, 1]) + Ns[:, 2] * d[:, 2]
            c = nd / np.sqrt(nn * dd)
            w = np.where(c > 0.0, c, 0.0)
        if flags & INVSQ:
            w = w / dd
    return w


def items(O, Ns, v, flags):
    """-> (dir, w, the bound the item is traced under: 0 where it is not traced -- dark, or !(w > 0))"""
    d, tmax = rays(O, v, flags)
    w = weights(Ns, d, flags)
    return d, w, np.where((tmax > 0.0) & (w > 0.0), tmax, 0.0)


def values(O, Ns, lights, occ):
    """lights: a sequence of (v, rgb, flags); occ [n, L]: the any-hit byte of every item -> (mask uint32 [n], value float32 [n, 3]): in list
    order, sum_k = sum_k + w * rgb_l[k] for the lights whose bit is set"""
    n = O.shape[0]
    s = np.zeros((n, 3)); mask = np.zeros(n, np.uint32)
    for l, (v, rgb, flags) in enumerate(lights):
        _, w, tm = items(O, Ns, v, int(flags))
        bit = (tm > 0.0) & (occ[:, l] == 0)
        mask |= np.where(bit, np.uint32(1 << l), np.uint32(0)).astype(np.uint32)
        with np.errstate(all="ignore"):
            s = np.where(bit[:, None], s + w[:, None] * np.asarray(rgb, np.float64)[None, :], s)
    with np.errstate(all="ignore"):
        return mask, s.astype(np.float32)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def _table():
    rng = np.random.default_rng(11)
    n = 4000
    t = np.zeros(n, CASE)
    t["P"] = rng.uniform(-2, 2, (n, 3)); t["Ns"] = rng.normal(size=(n, 3)) * rng.choice([1.0, 0.3, 7.0], (n, 1))
    t["eps"] = rng.choice([0.0, 1e-5, 1e-6, 0.25], n)
    t["L"] = rng.choice([1, 2, 5, 30, LMAX], n)
    t["L"][0], t["L"][1] = 1, LMAX
    t["lights"]["v"] = rng.uniform(-3, 3, (n, LMAX, 3)); t["lights"]["rgb"] = rng.uniform(0, 4, (n, LMAX, 3))
    t["lights"]["flags"] = rng.choice([0, COSINE, POINT, POINT | COSINE, POINT | INVSQ, POINT | COSINE | INVSQ], (n, LMAX))
    t["occ"] = rng.choice([0, 0, 1, 4], (n, 32))
    e = 100          # the edge rows, from here on
    O = origins(t["P"], t["Ns"], t["eps"][:, None])
    t["lights"]["v"][e:e + 40, 0] = O[e:e + 40]                      # a point light AT the origin: the zero direction (a directional light there: an ordinary ray)
    t["lights"]["flags"][e:e + 40, 0] = np.tile([POINT, POINT | COSINE, POINT | INVSQ, POINT | COSINE | INVSQ], 10)
    t["occ"][e:e + 40, 0] = 0
    t["L"][e + 40:e + 110] = 5
    t["Ns"][e + 40:e + 60] = 0.0                                      # Ns zero: the cosine is 0 / 0
    t["Ns"][e + 60:e + 80] = [1.0, 0.0, 0.0]                          # cosine exactly 0: Ns perpendicular to a directional light
    t["lights"]["v"][e + 60:e + 80, 0] = [0.0, 2.0, -1.0]; t["lights"]["flags"][e + 60:e + 80, 0] = COSINE; t["occ"][e + 60:e + 80, 0] = 0
    t["Ns"][e + 80:e + 100, 1] = np.nan                               # a NaN in Ns: O and every point light's direction with it
    t["P"][e + 100:e + 110, 2] = np.inf                               # a non-finite origin
    t["lights"]["v"][e + 110:e + 130] *= 1e200                        # dd overflows: w is 0 (cosine), 1 (none), 0 (inverse square)
    t["lights"]["v"][e + 130:e + 150] *= 1e-170                       # dd underflows to 0 or a denormal
    t["Ns"][e + 150:e + 170] *= -1e160
    t["occ"][e + 170:e + 200] = 0                                     # everything open: the mask's high bits
    t["L"][e + 170:e + 200] = LMAX
    t["lights"]["flags"][e + 170:e + 200] = 0
    return t


def _build(tmp, src, name):
    exe = str(tmp / name)
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe, "-lm"])
    return exe


def _run(exe, tmp, table, out_dtype):
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint64(table.size).tobytes()); f.write(table.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    out = np.fromfile(fout, out_dtype)
    assert out.size == table.size
    return out


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("lights")
    t = _table()
    return t, _run(_build(d, SRC, "lh_lights_check"), d, t, OUT)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_struct_sizes():
    assert LIGHT.itemsize == 56 and CASE.itemsize == 64 + 56 * LMAX + 32 and OUT.itemsize % 8 == 0


def test_ray_bound_and_weight_bit_for_bit(rule):
    t, out = rule
    O = origins(t["P"], t["Ns"], t["eps"][:, None])
    assert np.array_equal(bits(out["O"]), bits(O))
    seen = {"dark": 0, "w0": 0, "traced": 0}
    for l in range(LMAX):
        have = t["L"] > l
        for flags in np.unique(t["lights"]["flags"][:, l]):
            m = np.flatnonzero(have & (t["lights"]["flags"][:, l] == flags))
            if m.size == 0:
                continue
            # one light per call of the restatement: group the rows by their light's flags, the vector varies per row
            d = np.empty((m.size, 3)); tm = np.empty(m.size)
            with np.errstate(all="ignore"):
                d[:] = (t["lights"]["v"][m, l] - O[m]) if flags & POINT else t["lights"]["v"][m, l]
            dark = ~np.isfinite(d).all(axis=1) | (d == 0.0).all(axis=1)
            tm[:] = np.where(dark, 0.0, 1.0 if flags & POINT else np.inf)
            w = weights(t["Ns"][m], d, int(flags))
            ti = np.where((tm > 0.0) & (w > 0.0), tm, 0.0)
            assert np.array_equal(bits(out["dir"][m, l]), bits(d)), (l, flags)
            assert np.array_equal(bits(out["tmax_ray"][m, l]), bits(tm)), (l, flags)
            assert np.array_equal(bits(out["w"][m, l]), bits(w)), (l, flags)
            assert np.array_equal(bits(out["tmax_item"][m, l]), bits(ti)), (l, flags)
            seen["dark"] += int(dark.sum()); seen["w0"] += int(((tm > 0) & ~(w > 0)).sum()); seen["traced"] += int((ti > 0).sum())
    print(seen)
    assert seen["dark"] >= 40 and seen["w0"] >= 1000 and seen["traced"] >= 10000
    # the edges did what they were put there for
    e = 100
    assert (out["tmax_ray"][e:e + 40, 0] == 0.0).all() and (out["dir"][e:e + 40, 0] == 0.0).all()                   # the light at O
    assert (out["w"][e:e + 40:4, 0] == 1.0).all() and np.isinf(out["w"][e + 2:e + 40:4, 0]).all()                      # ... has a weight and still no bit
    assert (out["w"][e + 1:e + 40:4, 0] == 0.0).all()
    cos = (t["lights"]["flags"][e + 40:e + 60, :5] & COSINE) != 0
    assert (out["w"][e + 40:e + 60, :5][cos] == 0.0).all() and cos.any()                                                 # Ns zero: NaN -> 0
    assert (out["w"][e + 60:e + 80, 0] == 0.0).all() and (out["tmax_item"][e + 60:e + 80, 0] == 0.0).all() and np.isinf(out["tmax_ray"][e + 60:e + 80, 0]).all()
    pt = (t["lights"]["flags"][e + 80:e + 100, :5] & POINT) != 0
    assert (out["tmax_ray"][e + 80:e + 100, :5][pt] == 0.0).all() and np.isinf(out["tmax_ray"][e + 80:e + 100, :5][~pt]).all()


def test_mask_and_value_bit_for_bit(rule):
    """per row (every row has lights of its own): the list order, the float at the end, the bits"""
    t, out = rule
    O = origins(t["P"], t["Ns"], t["eps"][:, None])
    n = t.size
    s = np.zeros((n, 3)); mask = np.zeros(n, np.uint32)
    for l in range(LMAX):
        have = t["L"] > l
        bit = have & (out["tmax_item"][:, l] > 0.0) & (t["occ"][:, l] == 0)          # the items' bounds were checked above
        mask |= np.where(bit, np.uint32(1 << l), np.uint32(0)).astype(np.uint32)
        with np.errstate(all="ignore"):
            s = np.where(bit[:, None], s + out["w"][:, l, None] * t["lights"]["rgb"][:, l], s)
    with np.errstate(all="ignore"):
        val = s.astype(np.float32)
    assert np.array_equal(out["mask"], mask)
    assert np.array_equal(bits(out["value"]), bits(val))
    assert (mask[270:300] == (1 << LMAX) - 1).all()                      # 31 lights, all seen: bit 30 set, and the word is not 0xFFFFFFFF
    assert (mask != 0xFFFFFFFF).all() and (mask >> 30).any()
    assert ((mask == 0) & (val == 0.0).all(axis=1)).any() and np.isfinite(val[mask != 0]).any()
    # values() -- the form the GPU tests use, one list for all rows -- agrees on the rows of one list
    lights = [(t["lights"]["v"][7, l], t["lights"]["rgb"][7, l], int(t["lights"]["flags"][7, l])) for l in range(int(t["L"][7]))]
    m7, v7 = values(O[7:8], t["Ns"][7:8], lights, t["occ"][7:8])
    assert m7[0] == out["mask"][7] and np.array_equal(bits(v7[0]), bits(out["value"][7]))


def test_the_lists_the_rule_accepts(rule, tmp_path):
    t, out = rule
    fin = np.isfinite(t["eps"])
    assert (out["ok"][fin] == 1).all()          # every generated list is an accepted one: finite, flags in range, INVSQ with POINT, no zero direction
    bad = t[:16].copy()
    bad["L"] = 3
    bad["lights"]["flags"][:, :3] = 0
    bad["lights"]["flags"][0, 1] = INVSQ; bad["lights"]["flags"][1, 2] = 8; bad["lights"]["reserved"][2, 0] = 1
    bad["lights"]["v"][3, 1] = 0.0; bad["lights"]["v"][4, 2, 1] = np.nan; bad["lights"]["rgb"][5, 0, 2] = np.inf
    bad["eps"][6] = -1e-9; bad["eps"][7] = np.nan; bad["eps"][8] = np.inf
    bad["lights"]["flags"][9, 1] = POINT; bad["lights"]["v"][9, 1] = 0.0          # a point light at the world's origin: accepted
    bad["lights"]["flags"][10, 0] = POINT | COSINE | INVSQ
    got = _run(_build(tmp_path, SRC, "lh_lights_check"), tmp_path, bad, OUT)["ok"]
    assert list(got[:9]) == [0] * 9 and (got[9:] == 1).all()


def test_the_light_stages_plan(tmp_path):
    """kind 3 (LH_GATHER_LIGHT): fused on entries x L < 2^31 whoever asks, late up to 2^28 items, a tile's LH_AO_SYNC reads the count first; uniforms,
    the grouped order and the sun do not concern it"""
    case = np.dtype([(k, np.uint32) for k in ("kind", "where", "ao_fused", "uniforms", "ao_group", "sun", "sync", "pad")] + [("entries", np.uint64), ("N", np.uint64)])
    rows = []
    for where in (0, 1):
        for ao_fused in (0, 1):
            for sync in (0, 1):
                for grp in (0, 16):
                    for entries, N in ((1, 1), (2730, 31), ((1 << 28) // 16, 16), ((1 << 28) // 16 + 1, 16), (1 << 28, 1), ((1 << 28) + 1, 1),
                                       ((1 << 31) - 1, 1), (1 << 31, 1), ((1 << 31) // 31 + 1, 31), (1 << 26, 31)):
                        rows.append((3, where, ao_fused, 0, grp, grp != 0, sync, 0, entries, N))
    t = np.array(rows, case)
    out = _run(_build(tmp_path, PLAN_SRC, "lh_gather_check"), tmp_path, t, np.dtype([("fused", np.uint32), ("late", np.uint32)]))
    items_ = t["entries"] * t["N"]
    fused = (t["ao_fused"] != 0) & (items_ < (1 << 31))
    late = fused & (items_ <= (1 << 28)) & ~((t["where"] == 0) & (t["sync"] != 0))
    assert np.array_equal(out["fused"] != 0, fused) and np.array_equal(out["late"] != 0, late)
    assert fused.any() and (~fused & (t["ao_fused"] != 0)).any() and (fused & ~late).any() and late.any()
