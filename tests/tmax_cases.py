"""Per-ray maximum distance (lh_accel_intersect_device_tmax / _host_tmax): the scenes, the bounds and the expectation that the model
test (tests/test_tmax_model.py, no GPU) and the GPU test (tests/test_gpu_tmax.py) share, and the host library the model test walks.

The expectation is the contract itself: the oracle's unbounded record, kept where it is a hit with t < tmax (fp64, strict), else the
miss record (MISS, 1e38, 0, 0)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests.helpers import CSRC, MODEL_DIR, _fma_flag, chain_scene, load_golden, vertex_aimed_rays

_dp = C.POINTER(C.c_double)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)

NCLASSES = 13
# the bound classes, by number (t0: the oracle's t; for the oracle's misses a seeded value in (0, 2) stands in for it)
INF, T0, T0_UP, T0_DOWN, T0_ABOVE, T0_BELOW, HALF, TWICE, ZERO, NEGATIVE, NAN, E38, E300 = range(NCLASSES)


def sheets_scene():
    """eight copies of one triangle at z = 1 + k * 2e-11 (closer together than LH_FRAGILE_REL: every hit has partners within the
    fragility band), 5 000 rays from z = 0 straight at them: all hit prim 0 at t = 1.0"""
    tri = np.array([[-5.0, -5.0, 0.0], [5.0, -5.0, 0.0], [0.0, 7.0, 0.0]])
    P = np.concatenate([tri + [0.0, 0.0, 1.0 + k * 2e-11] for k in range(8)])
    rng = np.random.default_rng(7); n = 5000
    w = rng.random((n, 3)) + 0.05; w /= w.sum(1, keepdims=True)
    xy = (tri[None] * w[:, :, None]).sum(1)
    org = np.ascontiguousarray(np.stack([xy[:, 0], xy[:, 1], np.zeros(n)], 1))
    return P, np.arange(24, dtype=np.uint32), org, np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))


def _golden(name):
    z = load_golden(name)
    return z["P"], z["idx"], z["org"], z["dr"]


def _soup_3k_fat():
    g = load_golden("soup_3k_fat")
    return po.soup(int(g["ntri"]), int(g["nrays"]), float(g["half_extent"]), int(g["seed"]))


def _chain():
    P, idx = chain_scene(120)
    org, dr = vertex_aimed_rays(np.random.default_rng(5), P, idx, 20000)
    return P, idx, org, dr


# name -> (builder, rays, hits the oracle finds): the issue's table
SCENES = {
    "soup20k": (lambda: po.soup(20000, 60000, 0.01, 2027), 60000, 13568),
    "soup_3k_fat": (_soup_3k_fat, 10000, 5507),
    "fuzz_r06_f662_99": (lambda: _golden("fuzz_r06_f662_99"), 8000, 5688),
    "fuzz_r06_f661_359": (lambda: _golden("fuzz_r06_f661_359"), 4000, 3270),
    "chain120": (_chain, 20000, 4372),
    "sheets": (sheets_scene, 5000, 5000),
}


def bounds_for(exp, seed, classes=None, sheets=False):
    """one bound per ray, cycling through `classes` (default: all 13); sheets: the eight bounds between the sheets join the cycle"""
    prim, t = exp[0], exp[1]
    n = prim.shape[0]
    rng = np.random.default_rng(seed)
    t0 = np.where(prim != po.MISS, t, rng.uniform(1e-3, 2.0, n))
    classes = list(range(NCLASSES)) if classes is None else list(classes)
    table = {
        INF: np.full(n, np.inf), T0: t0, T0_UP: np.nextafter(t0, np.inf), T0_DOWN: np.nextafter(t0, 0.0),
        T0_ABOVE: t0 * (1.0 + 5e-11), T0_BELOW: t0 * (1.0 - 5e-11), HALF: 0.5 * t0, TWICE: 2.0 * t0, ZERO: np.zeros(n),
        NEGATIVE: np.full(n, -1.0), NAN: np.full(n, np.nan), E38: np.full(n, 1e38), E300: np.full(n, 1e300),
    }
    cols = [table[c] for c in classes]
    if sheets:
        cols += [np.full(n, 1.0 + (k + 0.5) * 2e-11) for k in range(8)]
    which = (np.arange(n) + seed) % len(cols)
    return np.ascontiguousarray(np.choose(which, cols)), which


def expected(exp, tmax):
    """the contract: the unbounded record where it is a hit with t < tmax, else the miss record -> ((prim, t, u, v), occluded)"""
    prim, t, u, v = exp
    with np.errstate(invalid="ignore"):
        keep = (prim != po.MISS) & (t < np.asarray(tmax, np.float64))
    return (np.where(keep, prim, np.uint32(po.MISS)).astype(np.uint32), np.where(keep, t, 1.0e38), np.where(keep, u, 0.0),
            np.where(keep, v, 0.0)), keep.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(P, idx, org, dr, exp): the scene, its rays and the oracle's unbounded records (computed once, shared, read-only)"""
    build, nrays, nhits = SCENES[name]
    P, idx, org, dr = build()
    org = np.ascontiguousarray(org, np.float64); dr = np.ascontiguousarray(dr, np.float64)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    exp = o.intersect(org, dr, nthreads=8)
    assert org.shape[0] == nrays and int((exp[0] != po.MISS).sum()) == nhits, (name, org.shape[0], int((exp[0] != po.MISS).sum()))
    for a in (org, dr) + tuple(exp):
        a.setflags(write=False)
    return dict(P=P, idx=idx, org=org, dr=dr, exp=exp)


# ---- the host library of the model test: tests/cpu_model/lh_tmax_model.c + lh_model.c + the product's sources ----
def build_tmax_model():
    so = os.path.join(MODEL_DIR, "liblh_tmax_model.so")
    srcs = [os.path.join(MODEL_DIR, "lh_tmax_model.c"), os.path.join(MODEL_DIR, "lh_model.c"), os.path.join(CSRC, "lh_bvh.c"),
            os.path.join(CSRC, "lh_refbvh.c"), os.path.join(CSRC, "lh_hostwalk.c")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("lh_bvh.h", "lh_filter.h", "lh_refbvh.h", "lh_reftrace.h", "lh_danger.h", "lh_tmax.h")]
    if (not os.path.exists(so)) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared"] + _fma_flag() + ["-I" + CSRC] + srcs +
                              ["-o", tmp, "-lm", "-lpthread"])
        os.replace(tmp, so)
    return so


class TmaxModel:
    """the product's bounded host walk (lh_hostwalk.c lh_host_walk_tmax) over the model's trees, lucille's own tree attached"""
    _L = None

    @classmethod
    def lib(cls):
        if cls._L is None:
            L = C.CDLL(build_tmax_model())
            L.lhm_build.restype = C.c_void_p; L.lhm_build.argtypes = [C.c_uint32, _dp, C.c_uint32, _u32p, C.c_int]
            L.lhm_free.argtypes = [C.c_void_p]
            L.lhm_ref_build.restype = C.c_void_p; L.lhm_ref_build.argtypes = [C.c_void_p, C.c_int]
            L.lhm_ref_free.argtypes = [C.c_void_p]
            L.lhtm_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, _dp, C.c_int, _u32p, _dp, _dp, _dp, _u8p]
            cls._L = L
        return cls._L

    def __init__(self, P, idx):
        L = self.lib()
        P = np.ascontiguousarray(P, np.float64).reshape(-1, 3); I = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        self.h = L.lhm_build(P.shape[0], P.ctypes.data_as(_dp), I.shape[0], I.ctypes.data_as(_u32p), 4)
        assert self.h
        self.ref = L.lhm_ref_build(self.h, 4)
        assert self.ref

    def close(self):
        if self.h:
            self.lib().lhm_ref_free(self.ref); self.lib().lhm_free(self.h); self.h = self.ref = None

    def walk(self, org, dr, tmax, anyhit):
        """-> (prim, t, u, v) or the occluded bytes; asserts the walk finished every ray"""
        org = np.ascontiguousarray(org, np.float64); dr = np.ascontiguousarray(dr, np.float64); tm = np.ascontiguousarray(tmax, np.float64)
        n = org.shape[0]
        prim = np.empty(n, np.uint32); t = np.empty(n); u = np.empty(n); v = np.empty(n); occ = np.full(n, 0x77, np.uint8)
        rc = self.lib().lhtm_walk(self.h, self.ref, n, org.ctypes.data_as(_dp), dr.ctypes.data_as(_dp), tm.ctypes.data_as(_dp), 1 if anyhit else 0,
                                  prim.ctypes.data_as(_u32p), t.ctypes.data_as(_dp), u.ctypes.data_as(_dp), v.ctypes.data_as(_dp),
                                  occ.ctypes.data_as(_u8p))
        assert rc == 0, rc
        return occ if anyhit else (prim, t, u, v)
