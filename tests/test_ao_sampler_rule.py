"""The built-in gather sampler (lh_ao_ray_builtin, lucille_amd/csrc/lh_ao.h) on the CPU.

The header against the model: the header, included unchanged into the stand-alone program tests/cpu_model/lh_ao_check.cpp and compiled for the host with
-ffp-contract=off (and once more with -fsanitize=address,undefined), against tests/ao_sampler.py, bit for bit -- origins, directions through the axis
record (every component then is an exact float32 value) and through seeded general records.

The model's own properties, over 2^18 keys x N rays: strata, the unit vector, the cosine weighting, uniformity, independence, distinct counters.  They are
what makes the model worth holding the device to (tests/test_gpu_ao_sampler.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import ao_sampler as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_ao_check.cpp")
CASE = np.dtype([("seed", np.uint64), ("key", np.uint64), ("ntheta", np.int32), ("nphi", np.int32), ("r", np.int32), ("pad", np.int32), ("h", np.float64, (12,))])
AXIS = np.array([0.25, -3.0, 7.5, 0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0])          # origin, then ri_ortho_basis of Ns = (0, 0, 1)
SEEDS = (0, 5, 0x8000000000000005)
GRIDS = (1, 4, 16, 64, 289, 1024)
EDGE_GRIDS = (4, 16, 64)


def _build(tmp, sanitize):
    exe = str(tmp / ("lh_ao_check_san" if sanitize else "lh_ao_check"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=gnu++14", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"] + flags + [SRC, "-o", exe, "-lm"])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ao")
    return _build(tmp, False), _build(tmp, True)


def run(exe, tmp, rows):
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint64(rows.size).tobytes()); f.write(rows.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    return np.fromfile(fout, np.float64).reshape(rows.size, 6)


def rows_of(seed, keys, ns, h):
    """every ray of the keys: h one record for all or one per key"""
    ntheta, nphi, N = sm.grid(ns)
    keys = np.asarray(keys, np.uint64)
    t = np.zeros((keys.size, N), CASE)
    t["seed"], t["ntheta"], t["nphi"] = np.uint64(seed), ntheta, nphi
    t["key"] = keys[:, None]; t["r"] = np.arange(N)[None, :]
    t["h"] = np.broadcast_to(np.asarray(h, np.float64).reshape(-1, 1, 12), (keys.size, N, 12))
    return t.reshape(-1)


def key_sets(rng):
    top = 1 << 34
    parts = [np.arange(16), np.arange(top - 8, top), np.arange(top, top + 8), [top + (1 << 33), (1 << 64) - 1, (5 << 34) | 12345, 12345],
             rng.integers(0, 1 << 63, 4)]
    return np.concatenate([np.asarray(p, np.uint64) for p in parts])


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_struct_size():
    assert CASE.itemsize == 128


def test_the_header_equals_the_model_bit_for_bit(exes, tmp_path):
    rng = np.random.default_rng(17)
    keys = key_sets(rng)
    general = np.concatenate([rng.uniform(-5, 5, (keys.size, 3)), rng.standard_normal((keys.size, 9))], axis=1)
    jobs = [(seed, keys, ns, h) for seed in SEEDS for ns in GRIDS for h in (AXIS, general)]
    for ns in EDGE_GRIDS:
        found = sm.find_edge_keys(5, ns)
        assert all(found[e] is not None for e in sm.EDGES), (ns, found)
        ek = np.array([found[e][0] for e in sm.EDGES], np.uint64)
        jobs.append((5, ek, ns, AXIS)); jobs.append((5, ek | np.uint64(3 << 34), ns, general[:4]))
    rows = np.concatenate([rows_of(*j) for j in jobs])
    out = run(exes[0], tmp_path, rows)
    san = run(exes[1], tmp_path, rows)
    assert np.array_equal(u64(out), u64(san))
    at = 0
    for seed, ks, ns, h in jobs:
        N = sm.grid(ns)[2]
        L = sm.local(seed, ks, ns)
        got = out[at:at + ks.size * N].reshape(ks.size, N, 6); at += ks.size * N
        hh = np.broadcast_to(np.asarray(h, np.float64).reshape(-1, 12), (ks.size, 12))
        want = sm.world(hh, L["f32"])
        assert np.array_equal(u64(got[..., 0:3]), u64(np.broadcast_to(hh[:, None, 0:3], (ks.size, N, 3)))), (seed, ns)
        assert np.array_equal(u64(got[..., 3:6]), u64(want)), (seed, ns, int((u64(got[..., 3:6]) != u64(want)).any(axis=-1).sum()))
        if h is AXIS:          # dir = (d1, -d0, d2): exact float32 values, the local vector's own bits
            d = got[..., 3:6]
            assert np.array_equal(d, d.astype(np.float32).astype(np.float64))
            loc = np.stack([-d[..., 1], d[..., 0], d[..., 2]], axis=-1).astype(np.float32) + np.float32(0.0)
            assert np.array_equal(loc.view(np.uint32), (L["f32"] + np.float32(0.0)).view(np.uint32))
    assert at == rows.size
    # keys at or above 2^34 alias key & mask
    a = run(exes[0], tmp_path, rows_of(5, [3, (1 << 34) + 3, (9 << 34) | 3], 16, AXIS)).reshape(3, 16, 6)
    assert np.array_equal(u64(a[0]), u64(a[1])) and np.array_equal(u64(a[0]), u64(a[2]))
    b = run(exes[0], tmp_path, rows_of(5, [3, 4], 16, AXIS)).reshape(2, 16, 6)
    assert not np.array_equal(b[0], b[1])


@pytest.mark.parametrize("ns", EDGE_GRIDS)
def test_the_four_edges(exes, tmp_path, ns):
    """the keys the model finds, through the header: z0 == 1 gives st == 0 and a ray in the tangent plane; z1 == 1 gives phi = 2 pi, the ray of phi = 0;
    r1 == 0 at j = 0 gives (ct, 0, st); r0 == 0 at i = 0 gives Ns"""
    ntheta, nphi, N = sm.grid(ns)
    found = sm.find_edge_keys(5, ns)
    assert all(found[e] is not None and found[e][0] < sm.SEARCH_KEYS for e in sm.EDGES), found
    print(ns, found)
    ek = np.array([found[e][0] for e in sm.EDGES], np.uint64)
    L = sm.local(5, ek, ns)
    d = run(exes[0], tmp_path, rows_of(5, ek, ns, AXIS)).reshape(4, N, 6)[..., 3:6]
    loc = np.stack([-d[..., 1], d[..., 0], d[..., 2]], axis=-1)          # through the axis record: dir = (d1, -d0, d2)
    k, r = 0, found["z0_one"][1]
    assert r % ntheta == ntheta - 1 >= 1 and L["z0"][k, r] == 1.0 and L["st"][k, r] == 0.0 and L["ct"][k, r] == 1.0
    assert loc[k, r, 2] == 0.0 and abs(np.hypot(loc[k, r, 0], loc[k, r, 1]) - 1.0) < 2.0 ** -22
    k, r = 1, found["z1_one"][1]
    assert r // ntheta == nphi - 1 and L["z1"][k, r] == 1.0 and L["sphi"][k, r] == 0.0 and L["cphi"][k, r] == 1.0
    assert np.array_equal(loc[k, r], [L["ct"][k, r], 0.0, L["st"][k, r]])
    k, r = 2, found["phi_zero"][1]
    assert r // ntheta == 0 and L["r1"][k, r] == 0.0 and L["z1"][k, r] == 0.0
    assert np.array_equal(loc[k, r], [L["ct"][k, r], 0.0, L["st"][k, r]])
    k, r = 3, found["r0_zero"][1]
    assert r % ntheta == 0 and L["r0"][k, r] == 0.0 and L["ct"][k, r] == 0.0 and L["st"][k, r] == 1.0
    assert np.array_equal(loc[k, r], [0.0, 0.0, 1.0])


def test_the_exact_angles():
    """sinpi / cospi of the model at the multiples of 1/2 and next to them"""
    s, c = sm.sincospi(np.array([0.0, 0.5, 1.0, 1.5, 2.0]))
    assert np.array_equal(s, [0.0, 1.0, 0.0, -1.0, 0.0]) and np.array_equal(c, [1.0, 0.0, -1.0, 0.0, 1.0])
    x = np.float32(2.0) * np.random.default_rng(3).random(100000, dtype=np.float32)
    s, c = sm.sincospi(x)
    assert np.finfo(np.longdouble).nmant >= 63
    big = np.longdouble("3.14159265358979323846264338327950288") * x.astype(np.longdouble)          # x < 2: the product loses nothing that fp64 would show
    assert np.abs(s - np.sin(big).astype(np.float64)).max() < 2.0 ** -51 and np.abs(c - np.cos(big).astype(np.float64)).max() < 2.0 ** -51
    assert np.abs(s * s + c * c - 1.0).max() < 2.0 ** -51


def chi2_999(dof):
    try:
        from scipy import stats
        return float(stats.chi2.ppf(0.999, dof))
    except ImportError:
        assert dof == 255
        return 330.52          # the 99.9 % point of chi-square with 255 degrees of freedom


@pytest.mark.parametrize("ns", [16, 64])
def test_the_model_is_a_sampler(ns):
    """2^18 keys x N rays at seed 5"""
    ntheta, nphi, N = sm.grid(ns)
    nkeys, chunk = 1 << 18, 1 << 15
    fields = ("k", "r0", "r1", "z0", "z1", "ct", "st")
    parts = []
    for b in range(0, nkeys, chunk):          # of every chunk only the seven fields used below are kept
        p = sm.local(5, np.arange(b, b + chunk, dtype=np.uint64), ns)
        i, j = p["i"], p["j"]
        parts.append({f: p[f] for f in fields})
        del p
    L = {f: np.concatenate([p[f] for p in parts]) for f in fields}
    del parts
    n = nkeys * N
    # strata, the upper edge included: (i + r0) / ntheta may round up to it
    z0, z1 = L["z0"].astype(np.float64), L["z1"].astype(np.float64)
    lo0, hi0 = (i / ntheta)[None, :], ((i + 1) / ntheta)[None, :]
    lo1, hi1 = (j / nphi)[None, :], ((j + 1) / nphi)[None, :]
    assert ((lo0 <= z0) & (z0 <= hi0)).all() and ((lo1 <= z1) & (z1 <= hi1)).all()
    on_edge = int((z0 == hi0).sum()) + int((z1 == hi1).sum())
    print("rays on the upper edge of their stratum: %d of %d" % (on_edge, n))
    assert on_edge < 1e-5 * n
    # a unit vector
    ct, st = L["ct"].astype(np.float64), L["st"].astype(np.float64)
    assert (st >= 0.0).all() and (st <= 1.0).all()
    assert np.abs(ct * ct + st * st - 1.0).max() <= 3 * 2.0 ** -24
    # cosine-weighted: E sin(theta) = E sqrt(1 - z0) = 2 / 3
    se = st.std(ddof=1) / np.sqrt(n)
    print("mean of st %.7f, standard error %.2e" % (st.mean(), se))
    assert abs(st.mean() - 2.0 / 3.0) < 5 * se
    # uniform in the square
    r0, r1 = L["r0"].reshape(-1), L["r1"].reshape(-1)
    assert (r0 >= 0).all() and (r0 < 1).all() and (r1 >= 0).all() and (r1 < 1).all()
    hist = np.bincount((r0 * np.float32(16)).astype(np.int64) * 16 + (r1 * np.float32(16)).astype(np.int64), minlength=256)
    chi = float(((hist - n / 256.0) ** 2 / (n / 256.0)).sum())
    print("chi-square of the 16 x 16 histogram: %.1f (99.9 %% point %.1f)" % (chi, chi2_999(255)))
    assert hist.size == 256 and chi < chi2_999(255)
    # the jitter fills its stratum: both halves, to the last sixteenth
    assert hist.min() > 0
    # independent

    def corr(a, b):
        a = a.astype(np.float64) - a.mean(dtype=np.float64); b = b.astype(np.float64) - b.mean(dtype=np.float64)
        return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
    c01, c00 = corr(r0, r1), corr(r0[:-1], r0[1:])
    print("correlation r0 ~ r1 %.2e, r0 of rays r and r + 1 %.2e, bound %.2e" % (c01, c00, 5 / np.sqrt(n)))
    assert abs(c01) < 5 / np.sqrt(n) and abs(c00) < 5 / np.sqrt(n - 1)
    # no two (key, r) share a k or a k + 1
    k = L["k"].reshape(-1)
    with np.errstate(over="ignore"):
        both = np.concatenate([k, k + np.uint64(1)])
    assert np.unique(both).size == 2 * n
