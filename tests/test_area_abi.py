"""The area-light stage's entry points (lh_accel_set_emitters, lh_accel_area_lights_device / _host, lh_accel_area_light_rays_device,
lh_render_area_lights_tile), lh_area_light_t and lh_area_params_t: the C ABI and the binding, without a GPU.  The rule itself is
tests/test_area_rule.py, the GPU side tests/test_gpu_area.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_set_emitters", "lh_accel_area_lights_device", "lh_accel_area_lights_host", "lh_accel_area_light_rays_device", "lh_render_area_lights_tile")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)
    assert la.AreaLight is binding.AreaLight and la.AreaParams is binding.AreaParams
    assert (la.AREA_COSINE, la.AREA_FACING, la.AREA_INVSQ, la.AREA_PDF, la.AREA_LIGHTS_MAX, la.AREA_SAMPLES_MAX) == (1, 2, 4, 8, 31, 1024)


def test_header_declares_them_and_the_layout_is_the_bindings(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the five functions to pointers of their declared types and prints the sizes, the
    offsets, the constants and the defaults: lh_area_light_t is 40 bytes, lh_area_params_t 24"""
    src = tmp_path / "area.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*e)(lh_accel_t *, const double *, size_t) = lh_accel_set_emitters;
    int (*a)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, const lh_area_light_t *, int,
             const lh_area_params_t *, uint64_t, const void *, const void *, const void *, size_t, const void *, void *, void *, void *) = lh_accel_area_lights_device;
    int (*b)(lh_accel_t *, size_t, const double *, const double *, const uint32_t *, const double *, const double *, const double *, const lh_area_light_t *, int,
             const lh_area_params_t *, uint64_t, const uint64_t *, const double *, size_t, uint32_t *, float *) = lh_accel_area_lights_host;
    int (*c)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, const lh_area_light_t *, int,
             const lh_area_params_t *, uint64_t, const void *, const void *, void *, void *, void *, void *, void *, void *, size_t, void *) = lh_accel_area_light_rays_device;
    int (*d)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, const lh_area_light_t *, int, const lh_area_params_t *, uint64_t, void *,
             lh_tile_stats_t *, void *) = lh_render_area_lights_tile;
    const lh_area_params_t def = LH_AREA_DEFAULTS;
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u %d %d %d %d %d %u %.17g %.17g\n", sizeof(lh_area_light_t), _Alignof(lh_area_light_t),
           offsetof(lh_area_light_t, first_tri), offsetof(lh_area_light_t, ntris), offsetof(lh_area_light_t, rgb), offsetof(lh_area_light_t, flags),
           offsetof(lh_area_light_t, reserved), sizeof(lh_area_params_t), offsetof(lh_area_params_t, eps), offsetof(lh_area_params_t, bound),
           offsetof(lh_area_params_t, nsamples), offsetof(lh_area_params_t, reserved), LH_AREA_COSINE, LH_AREA_FACING, LH_AREA_INVSQ, LH_AREA_PDF,
           LH_AREA_LIGHTS_MAX, LH_AREA_SAMPLES_MAX, ((1u << LH_AREA_LIGHTS_MAX) - 1u) != LH_AO_NO_HIT,
           e != NULL && a != NULL && b != NULL && c != NULL && d != NULL, (int)def.nsamples, def.reserved, def.eps, def.bound);
    return 0;
}
''')
    exe = tmp_path / "area"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in got[:22]] == [40, 8, 0, 4, 8, 32, 36, 24, 0, 8, 16, 20, 1, 2, 4, 8, 31, 1024, 1, 1, 16, 0]
    assert float(got[22]) == 1.0e-5 and float(got[23]) == 1.0
    assert C.sizeof(binding.AreaLight) == 40 and C.alignment(binding.AreaLight) == 8 and C.sizeof(binding.AreaParams) == 24
    assert [(n, getattr(binding.AreaLight, n).offset) for n, _ in binding.AreaLight._fields_] == [("first_tri", 0), ("ntris", 4), ("rgb", 8), ("flags", 32), ("reserved", 36)]
    assert [(n, getattr(binding.AreaParams, n).offset) for n, _ in binding.AreaParams._fields_] == [("eps", 0), ("bound", 8), ("nsamples", 16), ("reserved", 20)]
    p = la.AreaParams()
    assert (p.eps, p.bound, p.nsamples, p.reserved) == (1.0e-5, 1.0, 16, 0)


def test_binding_prototypes_and_signatures():
    L = binding.lib()
    assert [len(getattr(L, n).argtypes) for n in NEW] == [3, 20, 17, 22, 14]
    assert list(inspect.signature(la.HipAccel.set_emitters).parameters) == ["self", "tris"]
    assert list(inspect.signature(la.HipAccel.area_lights_device).parameters) == ["self", "org", "dr", "records", "lights", "params", "seed", "key", "uniforms",
                                                                                  "index", "count", "out", "stream"]
    assert list(inspect.signature(la.HipAccel.area_lights_host).parameters) == ["self", "org", "dr", "records", "lights", "params", "seed", "key", "uniforms"]
    assert list(inspect.signature(la.HipAccel.area_light_rays_device).parameters) == ["self", "org", "dr", "records", "lights", "params", "seed", "key", "uniforms",
                                                                                      "out", "stream"]
    assert list(inspect.signature(la.HipAccel.render_area_lights_tile).parameters) == ["self", "cam", "x0", "y0", "w", "h", "pixel_samples", "lights", "params",
                                                                                       "seed", "out", "stream"]
    l = la.AreaLight(3, 7, (4, 5, 6), la.AREA_FACING | la.AREA_PDF)
    assert (l.first_tri, l.ntris, list(l.rgb), l.flags, l.reserved) == (3, 7, [4.0, 5.0, 6.0], 10, 0)
    with pytest.raises(ValueError):
        binding._area_array("x", [la.AreaLight(), "not a light"])


def test_set_emitters_refusals_need_no_device():
    """the array is looked at first: a vertex that is not finite, 2^31 triangles, a count without an array; a good table on no accelerator is the
    accelerator's refusal"""
    L = binding.lib()
    tri = np.array([[0.0, 2.0, 0.0, 1.0, 2.0, 0.0, 0.0, 2.0, 1.0]] * 4)

    def call(a, n):
        rc = L.lh_accel_set_emitters(None, None if a is None else a.ctypes.data, n)
        return rc, L.lh_last_error().decode()

    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 17, 35):
            t = tri.copy(); t.reshape(-1)[at] = bad
            rc, err = call(t, 4)
            assert rc == -1 and "bad emitters" in err and "lh_accel_set_emitters" in err and "triangle %d" % (at // 9) in err, err
    rc, err = call(tri, 1 << 31); assert rc == -1 and "bad emitters" in err and "2^31" in err, err          # refused before a vertex is read
    rc, err = call(None, 4); assert rc == -1 and "bad emitters" in err, err
    rc, err = call(tri, 0); assert rc == -1 and "bad emitters" in err, err
    rc, err = call(tri, 4); assert rc == -1 and "not committed" in err, err
    rc, err = call(None, 0); assert rc == -1 and "not committed" in err, err          # removing needs an accelerator too


def _calls(L, lights, nl, params, n=8):
    """the four entry points on a NULL accelerator with host arrays standing in for every array: each refusal below comes before any of them is read"""
    o = np.zeros((n, 3)); p = np.zeros(n, np.uint32); t = np.zeros(n)
    vis, rgb = np.full(n, 7, np.uint32), np.full((n, 3), 7.0, np.float32)
    big = np.zeros((n * 64, 3)); tm = np.zeros(n * 64); cam = la.Camera.make(8, 8, 1.0, np.eye(4))
    pp = None if params is None else C.byref(params)
    return vis, rgb, [
        ("lh_accel_area_lights_device", lambda: L.lh_accel_area_lights_device(None, n, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data, t.ctypes.data,
                                                                              t.ctypes.data, lights, nl, pp, 1, None, None, None, 0, None, vis.ctypes.data,
                                                                              rgb.ctypes.data, None)),
        ("lh_accel_area_lights_host", lambda: L.lh_accel_area_lights_host(None, n, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data, t.ctypes.data,
                                                                          t.ctypes.data, lights, nl, pp, 1, None, None, 0, vis.ctypes.data, rgb.ctypes.data)),
        ("lh_accel_area_light_rays_device", lambda: L.lh_accel_area_light_rays_device(None, n, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data,
                                                                                      t.ctypes.data, t.ctypes.data, lights, nl, pp, 1, None, None, vis.ctypes.data,
                                                                                      vis.ctypes.data, big.ctypes.data, big.ctypes.data, tm.ctypes.data,
                                                                                      tm.ctypes.data, n * 64, None)),
        ("lh_render_area_lights_tile", lambda: L.lh_render_area_lights_tile(None, C.byref(cam), 0, 0, 8, 8, 1, lights, nl, pp, 1, rgb.ctypes.data, None, None))]


def test_refusals_need_no_device():
    """a bad list or bad parameters are refused ("bad area lights") before the accelerator is looked at, by every entry point, and nothing is written.
    Without an accelerator there is no emitter table, so every run leaves it: the best list is refused on that ground, with the table's size in the
    message"""
    L = binding.lib()
    good = [la.AreaLight(0, 1, (1, 1, 1)), la.AreaLight(1, 2, (2, 0, 1), la.AREA_FACING | la.AREA_INVSQ | la.AREA_PDF), la.AreaLight(3, 20, (1, 2, 3), 15)]

    def arr(ls):
        return (la.AreaLight * len(ls))(*ls)

    def refused(lights, nl, params, *msgs):
        vis, rgb, calls = _calls(L, lights, nl, params)
        for name, call in calls:
            rc = call()
            err = L.lh_last_error().decode()
            assert rc == -1 and name in err and all(m in err for m in msgs), (name, err)
        assert (vis == 7).all() and (rgb == 7.0).all()

    refused(arr(good), 3, None, "bad area lights", "within the 0 triangles")          # a light whose run leaves the table: there is none
    refused(arr([la.AreaLight(0xFFFFFFFF, 0xFFFFFFFF)]), 1, None, "bad area lights")
    refused(None, 3, None, "bad area lights")
    refused(arr(good), 0, None, "bad area lights")
    refused(arr(good), -1, None, "bad area lights")
    refused(arr([la.AreaLight()] * 32), 32, None, "bad area lights")
    for eps in (-1e-9, float("nan"), float("inf"), float("-inf")):
        refused(arr(good), 3, la.AreaParams(eps=eps), "bad area lights", "eps")
    for bound in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        refused(arr(good), 3, la.AreaParams(bound=bound), "bad area lights", "bound")
    for ns in (0, -1, 1025, 1 << 30):
        refused(arr(good), 3, la.AreaParams(nsamples=ns), "bad area lights", "nsamples")
    refused(arr(good), 3, la.AreaParams(reserved=1), "bad area lights")
    for bad in (float("nan"), float("inf")):
        ls = [la.AreaLight(x.first_tri, x.ntris, tuple(x.rgb), x.flags) for x in good]; ls[1].rgb[2] = bad
        refused(arr(ls), 3, None, "bad area lights")
    for flags in (16, 1 << 31, 0x10F):
        refused(arr([la.AreaLight(0, 1, (1, 1, 1), flags)]), 1, None, "bad area lights")
    refused(arr([la.AreaLight(0, 1, (1, 1, 1), 0, 1)]), 1, None, "bad area lights")
    refused(arr([la.AreaLight(0, 0)]), 1, None, "bad area lights")
