"""The rule of area lights (lucille_amd/csrc/lh_area.h: the emitter record, the pick, the point, the ray, the weight, a hit's mask and value, the
built-in uniforms, what the entry points accept) on the CPU: the header, compiled into the stand-alone program tests/cpu_model/lh_area_check.c with
-fsanitize=address,undefined -ffp-contract=off, against a restatement in numpy, bit for bit, over random and edge inputs; against the compiled
reference's ri_light_sample_pos_and_normal through tests/golden/area_sample.npz (tests/golden/make_area_golden.py), bit for bit; and the stage's plan
(lh_gather.h, kind LH_GATHER_AREA) through tests/cpu_model/lh_gather_check.c.

The restatement (records, builtin_uniforms, items, values below) is what tests/test_gpu_area.py holds the device to."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_area_check.c")
PLAN_SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_gather_check.c")
GOLDEN = os.path.join(ROOT, "tests", "golden", "area_sample.npz")

COSINE, FACING, INVSQ, PDF = 1, 2, 4, 8
LMAX, SMAX = 31, 1024
KEY_MASK = (1 << 34) - 1
LIGHT = np.dtype([("first_tri", np.uint32), ("ntris", np.uint32), ("rgb", np.float64, (3,)), ("flags", np.uint32), ("reserved", np.uint32)])
HEAD = np.dtype([("P", np.float64, (3,)), ("Ns", np.float64, (3,)), ("eps", np.float64), ("bound", np.float64), ("L", np.uint32), ("S", np.uint32),
                 ("ntab", np.uint32), ("use_uni", np.uint32), ("key", np.uint64), ("seed", np.uint64), ("claim", np.uint64), ("mode", np.uint32),
                 ("reserved", np.uint32), ("lights", LIGHT, (LMAX,))])
TAIL = np.dtype([("O", np.float64, (3,)), ("mask", np.uint32), ("closed", np.uint32), ("ok", np.uint32), ("pad", np.uint32), ("value", np.float32, (3,)),
                 ("pick", np.int32)])
ITEM = np.dtype([("x", np.float64, (3,)), ("dir", np.float64, (3,)), ("w", np.float64), ("tmax", np.float64)])


# ---- the rule, restated: every line one fp64 operation per element, in the header's order ----------------------------------------------------
def records(tris):
    """triangles [n, 3, 3] -> the emitter records [n, 16]: v0 v1 v2 n area pad"""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        e1 = t[:, 1] - t[:, 0]; e2 = t[:, 2] - t[:, 0]
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        norm2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        ln = np.sqrt(norm2)
        r = 1.0 / ln
        n = np.where((norm2 > np.float64(np.float32(1.0e-17)))[:, None], c * r[:, None], c)
        area = 0.5 * ln
    out = np.zeros((t.shape[0], 16))
    out[:, 0:9] = t.reshape(-1, 9); out[:, 9:12] = n; out[:, 12] = area
    return out


def mix32(x):
    x = x.astype(np.uint64)
    x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xff51afd7ed558ccd); x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xc4ceb9fe1a85ec53)
    x = x ^ (x >> np.uint64(33))
    return ((x >> np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def builtin_uniforms(key, seed, L, S):
    """keys uint64 [n] -> the generator's uniforms [n, L, S, 3]"""
    key = np.atleast_1d(np.asarray(key, np.uint64))
    item = np.arange(L * S, dtype=np.uint64)
    c = ((key & np.uint64(KEY_MASK))[:, None] * np.uint64(L * S) + item[None, :]) * np.uint64(4)
    k = (np.array([seed], np.uint64) * np.uint64(0x9E3779B97F4A7C15))[0] ^ c
    x = np.stack([mix32(k + np.uint64(j)).astype(np.float64) * 2.0 ** -32 for j in range(3)], axis=-1)
    return x.reshape(key.shape[0], L, S, 3)


def pick(x0, ntris):
    """the offset of the sampled triangle in its run; -1: x0 is a NaN"""
    x0 = np.asarray(x0, np.float64)
    with np.errstate(all="ignore"):
        p = x0 * np.float64(ntris)
        j = np.where(~(p >= 1.0), 0.0, np.where(p >= np.float64(ntris), np.float64(ntris - 1), np.trunc(p)))
    return np.where(np.isnan(x0), -1, np.nan_to_num(j).astype(np.int64))


def points(rec, x1, x2):
    """the point drawn on records rec [n, 16]: the reference's expression, rounded to float"""
    with np.errstate(all="ignore"):
        s = np.sqrt(x1); t = x2
        a = 1.0 - s; b = s - t * s
        pos = (rec[:, 0:3] * a[:, None] + rec[:, 3:6] * b[:, None]) + (rec[:, 6:9] * s[:, None]) * t[:, None]
        return pos.astype(np.float32).astype(np.float64)


def weights(Ns, d, n, area, ntris, flags):
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        w = np.ones(d.shape[0])
        if flags & COSINE:
            nn = (Ns[:, 0] * Ns[:, 0] + Ns[:, 1] * Ns[:, 1]) + Ns[:, 2] * Ns[:, 2]
            nd = (Ns[:, 0] * d[:, 0] + Ns[:, 1] * d[:, 1]) + Ns[:, 2] * d[:, 2]
            c = nd / np.sqrt(nn * dd)
            w = np.where(c > 0.0, c, 0.0)
        if flags & FACING:
            cl = -((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) / np.sqrt(dd)
            w = w * np.where(cl > 0.0, cl, 0.0)
        if flags & INVSQ:
            w = w / dd
        if flags & PDF:
            w = w * (np.float64(ntris) * area)
    return w


def items(O, Ns, light, rec, x, bound):
    """one light (first_tri, ntris, rgb, flags) for rows of origins, normals and uniforms -> (dir [n, 3], w [n], the bound the item is traced under
    [n]: 0 where it is not -- a NaN x0, a zero or non-finite dir, !(w > 0))"""
    first, ntris, _, flags = light
    j = pick(x[:, 0], ntris)
    r = rec[first + np.maximum(j, 0)]
    pos = points(r, x[:, 1], x[:, 2])
    with np.errstate(all="ignore"):
        d = pos - O
    nan0 = j < 0
    d = np.where(nan0[:, None], 0.0, d)
    dark = nan0 | ~np.isfinite(d).all(axis=1) | (d == 0.0).all(axis=1)
    w = np.where(dark, 0.0, weights(Ns, d, r[:, 9:12], r[:, 12], ntris, int(flags)))
    return d, w, np.where(~dark & (w > 0.0), np.float64(bound), 0.0)


def values(O, Ns, lights, S, rec, X, bound, occ):
    """lights: a sequence of (first_tri, ntris, rgb, flags); X [n, L, S, 3]; occ [n, L, S]: the any-hit byte of every item -> (mask uint32 [n],
    value float32 [n, 3], the items that are not open [n]): in list and sample order sum_k = sum_k + w * rgb_l[k], value_k = (float)(sum_k / S)"""
    n = O.shape[0]
    s = np.zeros((n, 3)); mask = np.zeros(n, np.uint32); nopen = np.zeros(n, np.int64)
    for l, lt in enumerate(lights):
        for sm in range(S):
            _, w, tm = items(O, Ns, lt, rec, X[:, l, sm], bound)
            op = (tm > 0.0) & (occ[:, l, sm] == 0)
            mask |= np.where(op, np.uint32(1 << l), np.uint32(0)).astype(np.uint32)
            nopen += op
            with np.errstate(all="ignore"):
                s = np.where(op[:, None], s + w[:, None] * np.asarray(lt[2], np.float64)[None, :], s)
    with np.errstate(all="ignore"):
        return mask, (s / np.float64(S)).astype(np.float32), len(lights) * S - nopen


# ---- the program --------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, src, name):
    exe = str(tmp / name)
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe, "-lm"])
    return exe


def case(P, Ns, lights, tris, S, eps=1e-5, bound=1.0, key=0, seed=1, uni=None, occ=None, mode=0, claim=0, reserved=0):
    """one row of the program's input: lights a list of (first_tri, ntris, rgb, flags[, reserved])"""
    h = np.zeros((), HEAD)
    h["P"], h["Ns"], h["eps"], h["bound"] = P, Ns, eps, bound
    L = len(lights)
    h["L"], h["S"], h["key"], h["seed"], h["mode"], h["claim"], h["reserved"] = L, S, key, seed, mode, claim, reserved
    for l, lt in enumerate(lights[:LMAX]):
        h["lights"][l]["first_tri"], h["lights"][l]["ntris"], h["lights"][l]["rgb"], h["lights"][l]["flags"] = lt[:4]
        h["lights"][l]["reserved"] = lt[4] if len(lt) > 4 else 0
    tris = None if tris is None else np.asarray(tris, np.float64).reshape(-1, 3, 3)
    h["ntab"] = 0 if tris is None else tris.shape[0]
    h["use_uni"] = uni is not None
    if mode == 0 and occ is None:
        occ = np.zeros((L, S), np.uint8)
    return dict(h=h, tris=tris, uni=None if uni is None else np.asarray(uni, np.float64).reshape(L, S, 3), occ=occ, lights=lights)


def run(exe, tmp, cases):
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for c in cases:
            f.write(c["h"].tobytes())
            if int(c["h"]["mode"]) == 0:
                f.write(c["tris"].tobytes())
                if c["uni"] is not None:
                    f.write(c["uni"].tobytes())
                b = np.asarray(c["occ"], np.uint8).reshape(-1)
                f.write(b.tobytes() + bytes((-b.size) % 8))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    raw = open(fout, "rb").read()
    out, at = [], 0
    for c in cases:
        t = np.frombuffer(raw, TAIL, 1, at)[0]; at += TAIL.itemsize
        o = dict(t=t)
        if int(c["h"]["mode"]) == 0:
            nt, LS = int(c["h"]["ntab"]), int(c["h"]["L"]) * int(c["h"]["S"])
            o["rec"] = np.frombuffer(raw, np.float64, 16 * nt, at).reshape(nt, 16); at += 128 * nt
            o["it"] = np.frombuffer(raw, ITEM, LS, at).reshape(int(c["h"]["L"]), int(c["h"]["S"])); at += ITEM.itemsize * LS
        out.append(o)
    assert at == len(raw)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check(c, o):
    """a mode-0 case against the restatement, bit for bit; returns (dir, w, tmax) [L, S]"""
    h = c["h"]
    L, S = int(h["L"]), int(h["S"])
    with np.errstate(all="ignore"):
        O = (h["P"] + h["Ns"] * h["eps"])[None, :]
    Ns = h["Ns"][None, :]
    rec = records(c["tris"])
    assert np.array_equal(bits(o["rec"]), bits(rec))
    assert np.array_equal(bits(o["t"]["O"]), bits(O[0]))
    X = c["uni"][None] if c["uni"] is not None else builtin_uniforms([int(h["key"])], int(h["seed"]), L, S)
    assert np.array_equal(bits(o["it"]["x"]), bits(X[0]))
    W = np.zeros((L, S)); T = np.zeros((L, S)); D = np.zeros((L, S, 3))
    for l, lt in enumerate(c["lights"]):
        d, w, tm = items(np.repeat(O, S, 0), np.repeat(Ns, S, 0), lt[:4], rec, X[0, l], float(h["bound"]))
        D[l], W[l], T[l] = d, w, tm
    assert np.array_equal(bits(o["it"]["dir"]), bits(D))
    assert np.array_equal(bits(o["it"]["w"]), bits(W))
    assert np.array_equal(bits(o["it"]["tmax"]), bits(T))
    mask, val, closed = values(O, Ns, [lt[:4] for lt in c["lights"]], S, rec, X, float(h["bound"]), np.asarray(c["occ"]).reshape(1, L, S))
    assert int(o["t"]["mask"]) == int(mask[0]) and int(o["t"]["closed"]) == int(closed[0])
    assert np.array_equal(bits(o["t"]["value"]), bits(val[0]))
    return D, W, T


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("area"), SRC, "lh_area_check")


def _mesh(rng, n, centre=(0.0, 2.0, 0.0), size=0.5):
    return np.asarray(centre) + size * rng.standard_normal((n, 3, 3))


def test_struct_sizes():
    assert LIGHT.itemsize == 40 and HEAD.itemsize == 112 + 40 * LMAX and TAIL.itemsize == 56 and ITEM.itemsize == 64


def test_random_cases_bit_for_bit(exe, tmp_path):
    """every flag combination, replayed and built-in uniforms, L = 1 .. 31, S = 1 .. 1024"""
    rng = np.random.default_rng(5)
    cases = []
    shapes = [(1, 1), (1, SMAX), (LMAX, 1), (LMAX, 4), (3, 16), (2, 5)] + [(int(rng.integers(1, 6)), int(rng.integers(1, 9))) for _ in range(120)]
    for k, (L, S) in enumerate(shapes):
        nt = int(rng.integers(1, 26))
        tris = _mesh(rng, nt)
        if k % 7 == 3:
            tris[rng.integers(nt)] = np.repeat(rng.standard_normal((1, 3)), 3, 0)          # a triangle without area
        lights = []
        for l in range(L):
            first = int(rng.integers(nt)); n = int(rng.integers(1, nt - first + 1))
            lights.append((first, n, rng.uniform(0, 4, 3), (16 * k + l) % 16 if k < 40 else int(rng.integers(16))))
        uni = rng.random((L, S, 3)) if k % 2 else None
        occ = rng.choice([0, 0, 1, 4], (L, S)).astype(np.uint8)
        cases.append(case(rng.uniform(-2, 2, 3), rng.normal(size=3) * rng.choice([1.0, 0.3, 7.0]), lights, tris, S, eps=rng.choice([0.0, 1e-5, 0.25]),
                          bound=rng.choice([1.0, 1 - 1e-4, 0.5]), key=int(rng.integers(1 << 40)), seed=int(rng.integers(1 << 62)), uni=uni, occ=occ))
    # all 31 lights open: bit 30, and the word is not the mark of a miss
    tris = _mesh(rng, 31, centre=(0.0, 5.0, 0.0))
    cases.append(case((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), [(l, 1, (1.0, 0.5, 0.25), 0) for l in range(LMAX)], tris, 4, key=(1 << 34) - 1, seed=(1 << 64) - 1))
    out = run(exe, tmp_path, cases)
    seen = set()
    traced = dark = 0
    for c, o in zip(cases, out):
        _, W, T = check(c, o)
        assert int(o["t"]["ok"]) == 1
        traced += int((T > 0).sum()); dark += int((T == 0).sum())
        seen |= {int(lt[3]) for lt in c["lights"]}
    print(traced, dark)
    assert seen == set(range(16)) and traced > 500 and dark > 500          # both kinds of item in numbers
    assert int(out[-1]["t"]["mask"]) == (1 << LMAX) - 1 and int(out[-1]["t"]["closed"]) == 0


def test_the_pick_clamps(exe, tmp_path):
    """x0 at 0 and at 1 - 2^-53 with ntris 1, 3 and 2^20 (the product rounds up to ntris: the reference reads out of bounds there), NaN, out of range"""
    top = 1.0 - 2.0 ** -53
    rows = [(x0, n) for n in (1, 3, 1 << 20, (1 << 31) - 1) for x0 in (0.0, -0.0, top, 0.5, 1.0, 1.5, -0.25, -7.0, np.inf, -np.inf, np.nan, 1e300, 2.0 ** -60)]
    cases = [case((x0, 0, 0), (0, 0, 0), [], None, 1, mode=2, claim=n) for x0, n in rows]
    got = np.array([int(o["t"]["pick"]) for o in run(exe, tmp_path, cases)])
    want = np.array([int(pick(np.array([x0]), n)[0]) for x0, n in rows])
    assert np.array_equal(got, want)
    for (x0, n), j in zip(rows, got):
        assert (j == -1) == bool(np.isnan(x0)) and (np.isnan(x0) or 0 <= j <= n - 1)
        if x0 == top or x0 >= 1.0:
            assert j == n - 1          # the last triangle: the product of a number below 1 stays below ntris (n 2^-53 is at least half an ulp of n), at 1 and beyond the clamp holds it
        if x0 <= 0.0:
            assert j == 0
    assert top < 1.0 and top * 3.0 < 3.0 and top * float(1 << 20) < float(1 << 20)


# a triangle with float-exact vertices in the plane y = 2, its normal (0, -1, 0) or (0, 1, 0) by winding
FLAT = np.array([[[0.0, 2.0, 0.0], [0.0, 2.0, 1.0], [1.0, 2.0, 0.0]]])
DOWN = np.array([[[0.0, 2.0, 0.0], [1.0, 2.0, 0.0], [0.0, 2.0, 1.0]]])          # the same corner v0, the normal (0, -1, 0): it faces a hit below it
NOAREA = np.array([[[0.5, 3.0, 0.5], [0.5, 3.0, 0.5], [0.75, 3.25, 0.125]]])


def test_edges(exe, tmp_path):
    cases, name = [], []

    def add(n, *a, **kw):
        name.append(n); cases.append(case(*a, **kw))
    one = [[0.0, 0.0, 0.0]]
    for f in range(16):
        add("x1=0", (0.25, 0.0, 0.25), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], DOWN, 1, uni=[[0.3, 0.0, 0.7]])                    # the sample is v0
        add("at O", (0.0, 2.0, 0.0), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], FLAT, 1, eps=0.0, uni=[[0.3, 0.0, 0.7]])               # zero dir
        add("Ns=0", (0.25, 0.0, 0.25), (0.0, 0.0, 0.0), [(0, 1, (1, 1, 1), f)], DOWN, 1, uni=[[0.3, 0.5, 0.5]])
        add("cos0 surface", (0.25, 0.0, 0.25), (1.0, 0.0, 0.0), [(0, 1, (1, 1, 1), f)], DOWN, 1, eps=0.0, uni=[[0.0, 0.0, 0.0]])     # (a cosine below 0; the exact zero: below)
        add("cos0 emitter", (3.0, 2.0, 3.0), (-1.0, 5.0, -1.0), [(0, 1, (1, 1, 1), f)], FLAT, 1, eps=0.0, uni=[[0.3, 0.25, 0.5]])      # O in the emitter's plane
        add("cos0 emitter back", (3.0, 2.0, 3.0), (-1.0, 5.0, -1.0), [(0, 1, (1, 1, 1), f)], FLAT[:, ::-1], 1, eps=0.0, uni=[[0.3, 0.25, 0.5]])
        add("no area", (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], NOAREA, 1, uni=[[0.3, 0.25, 0.5]])
        add("dd over", (1e200, 0.0, 0.0), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], FLAT, 1, eps=0.0, uni=[[0.3, 0.25, 0.5]])
        add("dd under", (1e-170, 1e-170, 0.0), (0.0, -1.0, 0.0), [(0, 1, (1, 1, 1), f)], np.array([one * 3]) * 1.0 + [[[0, 0, 0], [0, 0, 1], [1, 0, 0]]], 1,
            eps=0.0, uni=[[0.3, 0.0, 0.5]])
        add("nan x0", (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], FLAT, 1, uni=[[np.nan, 0.25, 0.5]])
        add("x1<0", (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], FLAT, 1, uni=[[0.5, -0.25, 0.5]])                      # sqrt: NaN, dark
        add("x out of range", (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], FLAT, 1, uni=[[7.0, 4.0, -3.0]])              # the rule applied as it stands
        add("float overflow", (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), [(0, 1, (1, 1, 1), f)], FLAT * 1e60, 1, uni=[[0.5, 0.25, 0.5]])       # pos rounds to inf: dark
    # the surface cosine exactly 0: Ns = (1, 0, 0) and dir.x = 0
    for f in range(16):
        add("cos0 surface exact", (0.0, 0.0, 0.25), (1.0, 0.0, 0.0), [(0, 1, (1, 1, 1), f)], DOWN, 1, eps=0.0, uni=[[0.0, 0.0, 0.0]])
        add("cos0 surface exact back", (0.0, 0.0, 0.25), (-1.0, 0.0, 0.0), [(0, 1, (1, 1, 1), f)], DOWN, 1, eps=0.0, uni=[[0.0, 0.0, 0.0]])
    out = run(exe, tmp_path, cases)
    for n, c, o in zip(name, cases, out):
        D, W, T = check(c, o)
        f = int(c["lights"][0][3])
        d, w, t = D[0, 0], W[0, 0], T[0, 0]
        if n == "x1=0":
            assert np.array_equal(d, np.array([0.0, 2.0, 0.0]) - o["t"]["O"])
        if n in ("at O", "nan x0", "x1<0", "float overflow"):
            assert t == 0.0 and w == 0.0 and int(o["t"]["mask"]) == 0 and int(o["t"]["closed"]) == 1
            if n == "at O":
                assert (d == 0.0).all()
        if n == "Ns=0":
            assert (t == 0.0) == bool(f & COSINE)          # 0 / 0: the NaN gives 0
        if n.startswith("cos0 surface exact"):
            assert d[0] == 0.0 and (t == 0.0) == bool(f & COSINE)
        if n.startswith("cos0 emitter"):
            assert d[1] == 0.0 and (t == 0.0) == bool(f & FACING)
        if n == "no area":
            assert o["rec"][0, 12] == 0.0 and (o["rec"][0, 9:12] == 0.0).all()
            assert (t == 0.0) == bool(f & (PDF | FACING))          # the normal is the zero cross product: no facing cosine either
        if n == "dd over":
            assert (t == 0.0) == bool(f & (COSINE | FACING | INVSQ)) and (t == 0.0 or w == (0.5 if f & PDF else 1.0))
        if n == "dd under":
            assert np.isfinite(d).all() and (d != 0.0).any()
            if f == INVSQ:
                assert np.isinf(w) and t == 1.0
    assert len({n for n in name}) == 15


def test_the_golden_bit_for_bit(exe, tmp_path):
    """pos and n of the compiled reference's ri_light_sample_pos_and_normal for the uniforms its randomMT() drew"""
    z = np.load(GOLDEN)
    cases = []
    for k in range(4):
        tris, uni = z["tris%d" % k], z["uni%d" % k]
        nt, N = tris.shape[0], uni.shape[0]
        assert N >= 300 and (uni >= 0).all() and (uni < 1).all()
        # O = 0 (P = 0, Ns = 0): dir is pos
        cases.append(case((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), [(0, nt, (1, 1, 1), 0)], tris, N, uni=uni.reshape(1, N, 3)))
    out = run(exe, tmp_path, cases)
    for k, (c, o) in enumerate(zip(cases, out)):
        check(c, o)
        tris, uni, pos, nrm = z["tris%d" % k], z["uni%d" % k], z["pos%d" % k], z["nrm%d" % k]
        assert np.array_equal(bits(o["it"]["dir"][0]), bits(pos)), k
        j = pick(uni[:, 0], tris.shape[0])
        assert np.array_equal(bits(o["rec"][j, 9:12]), bits(nrm)), k
        assert len(set(j.tolist())) == tris.shape[0]          # every triangle was drawn
        assert np.array_equal(pos, pos.astype(np.float32).astype(np.float64))
    assert (z["nrm3"] == 0.0).all(axis=1).any()          # the triangle without area: the guard's else branch


def test_the_built_in_generator(exe, tmp_path):
    """keys beyond 34 bits are masked, the item index is l S + s, the stride is 4"""
    cases = [case((0, 0, 0), (0, 1, 0), [(0, 1, (1, 1, 1), 0)] * L, FLAT, S, key=key, seed=seed)
             for (L, S, key, seed) in ((1, 1, 0, 0), (3, 5, 12345, 1), (LMAX, 7, (1 << 34) + 5, 99), (2, SMAX, (1 << 34) - 1, (1 << 64) - 1), (3, 5, (7 << 34) | 12345, 1))]
    out = run(exe, tmp_path, cases)
    for c, o in zip(cases, out):
        check(c, o)
        x = o["it"]["x"]
        assert (x >= 0).all() and (x < 1).all() and np.array_equal(x * 2.0 ** 32, np.floor(x * 2.0 ** 32))
    assert np.array_equal(out[1]["it"]["x"], out[4]["it"]["x"])          # the key's high bits (the self primitive) do not reach the generator
    x = out[3]["it"]["x"].reshape(-1, 3)
    assert abs(x.mean() - 0.5) < 0.01 and len(np.unique(x)) > 0.99 * x.size


def test_what_the_entry_points_accept(exe, tmp_path):
    ok_light = (2, 3, (1.0, 2.0, 3.0), COSINE | FACING | INVSQ | PDF)
    rows = [  # (lights, S, eps, bound, claim, reserved, accepted)
        ([ok_light], 16, 1e-5, 1.0, 5, 0, 1), ([ok_light] * LMAX, 1, 0.0, 1e-300, 5, 0, 1), ([ok_light], SMAX, 1e-5, 1 - 1e-4, 1 << 31, 0, 1),
        ([], 16, 1e-5, 1.0, 5, 0, 0), ([ok_light] * (LMAX + 1), 16, 1e-5, 1.0, 5, 0, 0),
        ([ok_light], 0, 1e-5, 1.0, 5, 0, 0), ([ok_light], SMAX + 1, 1e-5, 1.0, 5, 0, 0),
        ([(0, 1, (np.nan, 0, 0), 0)], 1, 1e-5, 1.0, 5, 0, 0), ([(0, 1, (0, np.inf, 0), 0)], 1, 1e-5, 1.0, 5, 0, 0),
        ([(0, 1, (1, 1, 1), 16)], 1, 1e-5, 1.0, 5, 0, 0), ([(0, 1, (1, 1, 1), 0, 1)], 1, 1e-5, 1.0, 5, 0, 0),
        ([(0, 0, (1, 1, 1), 0)], 1, 1e-5, 1.0, 5, 0, 0), ([(2, 4, (1, 1, 1), 0)], 1, 1e-5, 1.0, 5, 0, 0), ([(5, 1, (1, 1, 1), 0)], 1, 1e-5, 1.0, 5, 0, 0),
        ([(0, 1, (1, 1, 1), 0)], 1, 1e-5, 1.0, 0, 0, 0),                                                       # no table
        ([(0xFFFFFFFF, 0xFFFFFFFF, (1, 1, 1), 0)], 1, 1e-5, 1.0, 5, 0, 0),                                    # the sum does not wrap
        ([(0xFFFFFFFF, 2, (1, 1, 1), 0)], 1, 1e-5, 1.0, 5, 0, 0),
        ([ok_light], 1, -1e-9, 1.0, 5, 0, 0), ([ok_light], 1, np.nan, 1.0, 5, 0, 0), ([ok_light], 1, np.inf, 1.0, 5, 0, 0),
        ([ok_light], 1, 1e-5, 0.0, 5, 0, 0), ([ok_light], 1, 1e-5, -1.0, 5, 0, 0), ([ok_light], 1, 1e-5, 1.0 + 2.0 ** -52, 5, 0, 0),
        ([ok_light], 1, 1e-5, np.nan, 5, 0, 0), ([ok_light], 1, 1e-5, np.inf, 5, 0, 0), ([ok_light], 1, 1e-5, 1.0, 5, 1, 0),
    ]
    cases = []
    for lights, S, eps, bound, claim, reserved, _ in rows:
        c = case((0, 0, 0), (0, 1, 0), lights[:LMAX], None, 1, eps=eps, bound=bound, mode=1, claim=claim, reserved=reserved)
        c["h"]["L"], c["h"]["S"] = len(lights), S
        cases.append(c)
    got = [int(o["t"]["ok"]) for o in run(exe, tmp_path, cases)]
    assert got == [r[-1] for r in rows]


def test_the_area_stages_plan(tmp_path):
    """kind 4 (LH_GATHER_AREA): the light stage's plan on entries x (L S), and replayed uniforms send it to the ray kernel"""
    case_t = np.dtype([(k, np.uint32) for k in ("kind", "where", "ao_fused", "uniforms", "ao_group", "sun", "sync", "pad")] + [("entries", np.uint64), ("N", np.uint64)])
    rows = []
    for where in (0, 1):
        for ao_fused in (0, 1):
            for uniforms in (0, 1):
                for sync in (0, 1):
                    for grp in (0, 16):
                        for entries, N in ((1, 1), (2730, 31 * 4), ((1 << 28) // 16, 16), ((1 << 28) // 16 + 1, 16), (1 << 28, 1), ((1 << 28) + 1, 1),
                                           ((1 << 31) - 1, 1), (1 << 31, 1), ((1 << 31) // (31 * 1024) + 1, 31 * 1024), (1 << 20, 31 * 1024)):
                            rows.append((4, where, ao_fused, uniforms, grp, grp != 0, sync, 0, entries, N))
    t = np.array(rows, case_t)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint64(t.size).tobytes()); f.write(t.tobytes())
    r = subprocess.run([_build(tmp_path, PLAN_SRC, "lh_gather_check"), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = np.fromfile(fout, np.dtype([("fused", np.uint32), ("late", np.uint32)]))
    n_items = t["entries"] * t["N"]
    fused = (t["ao_fused"] != 0) & (t["uniforms"] == 0) & (n_items < (1 << 31))
    late = fused & (n_items <= (1 << 28)) & ~((t["where"] == 0) & (t["sync"] != 0))
    assert np.array_equal(out["fused"] != 0, fused) and np.array_equal(out["late"] != 0, late)
    assert fused.any() and (~fused & (t["ao_fused"] != 0) & (t["uniforms"] == 0)).any() and (fused & ~late).any() and late.any()
    assert not (out["fused"][t["uniforms"] != 0]).any()
