"""The light stage's entry points (lh_accel_lights_device / _host, lh_accel_light_rays_device, lh_render_lights_tile), lh_light_t and
lh_lights_params_t: the C ABI and the binding, without a GPU.  The rule itself is tests/test_lights_rule.py, the GPU side
tests/test_gpu_lights.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_lights_device", "lh_accel_lights_host", "lh_accel_light_rays_device", "lh_render_lights_tile")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)
    assert la.Light is binding.Light and la.LightsParams is binding.LightsParams
    assert (la.LIGHT_POINT, la.LIGHT_COSINE, la.LIGHT_INVSQ, la.LIGHTS_MAX) == (1, 2, 4, 31)


def test_header_declares_them_and_the_layout_is_the_bindings(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the four functions to pointers of their declared types and prints the sizes,
    the offsets and the constants: lh_light_t is 56 bytes, and a full mask of LH_LIGHTS_MAX lights is not the mark of a miss"""
    src = tmp_path / "lights.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*a)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, const lh_light_t *, int,
             const lh_lights_params_t *, const void *, size_t, const void *, void *, void *, void *) = lh_accel_lights_device;
    int (*b)(lh_accel_t *, size_t, const double *, const double *, const uint32_t *, const double *, const double *, const double *, const lh_light_t *, int,
             const lh_lights_params_t *, uint32_t *, float *) = lh_accel_lights_host;
    int (*c)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, const lh_light_t *, int,
             const lh_lights_params_t *, void *, void *, void *, void *, void *, size_t, void *) = lh_accel_light_rays_device;
    int (*d)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, const lh_light_t *, int, const lh_lights_params_t *, void *, lh_tile_stats_t *,
             void *) = lh_render_lights_tile;
    const lh_lights_params_t def = LH_LIGHTS_DEFAULTS;
    printf("%zu %zu %zu %zu %zu %zu %zu %u %u %u %d %d %d %.17g\n", sizeof(lh_light_t), _Alignof(lh_light_t), offsetof(lh_light_t, v), offsetof(lh_light_t, rgb),
           offsetof(lh_light_t, flags), offsetof(lh_light_t, reserved), sizeof(lh_lights_params_t), LH_LIGHT_POINT, LH_LIGHT_COSINE, LH_LIGHT_INVSQ, LH_LIGHTS_MAX,
           ((LH_LIGHTS_MAX == 32 ? 0xFFFFFFFFu : (1u << (LH_LIGHTS_MAX & 31)) - 1u) != LH_AO_NO_HIT), a != NULL && b != NULL && c != NULL && d != NULL, def.eps);
    return 0;
}
''')
    exe = tmp_path / "lights"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in got[:13]] == [56, 8, 0, 24, 48, 52, 8, 1, 2, 4, 31, 1, 1] and float(got[13]) == 1.0e-5
    assert C.sizeof(binding.Light) == 56 and C.alignment(binding.Light) == 8 and C.sizeof(binding.LightsParams) == 8
    assert [(n, getattr(binding.Light, n).offset) for n, _ in binding.Light._fields_] == [("v", 0), ("rgb", 24), ("flags", 48), ("reserved", 52)]
    assert la.LightsParams().eps == 1.0e-5


def test_binding_prototypes_and_signatures():
    L = binding.lib()
    assert [len(getattr(L, n).argtypes) for n in NEW] == [17, 13, 18, 13]
    assert list(inspect.signature(la.HipAccel.lights_device).parameters) == ["self", "org", "dr", "records", "lights", "params", "index", "count", "out", "stream"]
    assert list(inspect.signature(la.HipAccel.lights_host).parameters) == ["self", "org", "dr", "records", "lights", "params"]
    assert list(inspect.signature(la.HipAccel.light_rays_device).parameters) == ["self", "org", "dr", "records", "lights", "params", "out", "stream"]
    assert list(inspect.signature(la.HipAccel.render_lights_tile).parameters) == ["self", "cam", "x0", "y0", "w", "h", "pixel_samples", "lights", "params", "out", "stream"]
    l = la.Light((1, 2, 3), (4, 5, 6), la.LIGHT_POINT | la.LIGHT_INVSQ)
    assert list(l.v) == [1.0, 2.0, 3.0] and list(l.rgb) == [4.0, 5.0, 6.0] and l.flags == 5 and l.reserved == 0


def _calls(L, lights, nl, params, n=8, outs=None):
    """the four entry points on a NULL accelerator with host arrays standing in for every array: each refusal below comes before any of them is read"""
    o = np.zeros((n, 3)); p = np.zeros(n, np.uint32); t = np.zeros(n)
    vis, rgb = outs if outs is not None else (np.full(n, 7, np.uint32), np.full((n, 3), 7.0, np.float32))
    big = np.zeros((n * 32, 3)); tm = np.zeros(n * 32); cam = la.Camera.make(8, 8, 1.0, np.eye(4))
    ptr = None if lights is None else lights
    pp = None if params is None else C.byref(params)
    return vis, rgb, [
        ("lh_accel_lights_device", lambda: L.lh_accel_lights_device(None, n, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data, t.ctypes.data, t.ctypes.data,
                                                                    ptr, nl, pp, None, 0, None, vis.ctypes.data, rgb.ctypes.data, None)),
        ("lh_accel_lights_host", lambda: L.lh_accel_lights_host(None, n, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data, t.ctypes.data, t.ctypes.data,
                                                                ptr, nl, pp, vis.ctypes.data, rgb.ctypes.data)),
        ("lh_accel_light_rays_device", lambda: L.lh_accel_light_rays_device(None, n, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data, t.ctypes.data,
                                                                            t.ctypes.data, ptr, nl, pp, vis.ctypes.data, vis.ctypes.data, big.ctypes.data,
                                                                            big.ctypes.data, tm.ctypes.data, n * 32, None)),
        ("lh_render_lights_tile", lambda: L.lh_render_lights_tile(None, C.byref(cam), 0, 0, 8, 8, 1, ptr, nl, pp, rgb.ctypes.data, None, None))]


def test_refusals_need_no_device():
    """a bad list or a bad eps is refused ("bad lights") before the accelerator is looked at, by every entry point; a good one on an accelerator that
    is not committed, by the accelerator; nothing is written"""
    L = binding.lib()
    good = [la.Light((0.3, 0.9, 0.2), (1, 1, 1)), la.Light((1, 2, 3), (2, 0, 1), la.LIGHT_POINT | la.LIGHT_COSINE | la.LIGHT_INVSQ), la.Light((0, -1, 0), (1, 2, 3), la.LIGHT_COSINE)]

    def arr(ls):
        return (la.Light * len(ls))(*ls)

    def refused(lights, nl, params, msg):
        vis, rgb, calls = _calls(L, lights, nl, params)
        for name, call in calls:
            rc = call()
            err = L.lh_last_error().decode()
            assert rc == -1 and msg in err and name in err, (name, err)
        assert (vis == 7).all() and (rgb == 7.0).all()

    refused(arr(good), 3, None, "not committed")
    refused(arr(good), 3, la.LightsParams(0.0), "not committed")
    refused(arr([la.Light((0, 1, 0), (1, 1, 1))] * 31), 31, None, "not committed")
    refused(arr([la.Light((0, 0, 0), (1, 1, 1), la.LIGHT_POINT)]), 1, None, "not committed")          # a point light may sit anywhere
    # the list
    refused(None, 3, None, "bad lights")
    refused(arr(good), 0, None, "bad lights")
    refused(arr(good), -1, None, "bad lights")
    refused(arr([la.Light((0, 1, 0), (1, 1, 1))] * 32), 32, None, "bad lights")          # LH_LIGHTS_MAX is 31: a mask of 32 bits would be the mark of a miss
    # eps
    for eps in (-1e-9, float("nan"), float("inf"), float("-inf")):
        refused(arr(good), 3, la.LightsParams(eps), "bad lights")
    # one light of the list
    def one(k, **kw):
        ls = [la.Light(tuple(x.v), tuple(x.rgb), x.flags, x.reserved) for x in good]
        for name, val in kw.items():
            if name in ("v", "rgb"):
                getattr(ls[k], name)[val[0]] = val[1]
            else:
                setattr(ls[k], name, val)
        return arr(ls)

    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(3):
            refused(one(k, v=(k, bad)), 3, None, "bad lights")
            refused(one(k, rgb=(2 - k, bad)), 3, None, "bad lights")
    z = one(0, v=(0, 0.0)); z[0].v[1] = 0.0; z[0].v[2] = 0.0
    refused(z, 3, None, "bad lights")                                           # a directional light without a direction
    for flags in (8, 16, 1 << 31, 0x107):
        refused(one(1, flags=flags), 3, None, "bad lights")
    refused(one(0, flags=la.LIGHT_INVSQ), 3, None, "bad lights")                # the inverse square needs a position
    refused(one(2, flags=la.LIGHT_INVSQ | la.LIGHT_COSINE), 3, None, "bad lights")
    refused(one(2, reserved=1), 3, None, "bad lights")


def test_the_other_refusals_come_after_the_lights():
    """with a good list: sizes and alignments as lh_accel_env_device refuses them, before the accelerator"""
    L = binding.lib()
    good = (la.Light * 2)(la.Light((0.3, 0.9, 0.2), (1, 1, 1)), la.Light((1, 2, 3), (2, 0, 1), la.LIGHT_POINT))
    o = np.zeros((8, 3)); p = np.zeros(8, np.uint32); t = np.zeros(8); vis = np.zeros(9, np.uint32); rgb = np.zeros((9, 3), np.float32)

    def dev(n=8, index=None, n_index=0, count=None, v=vis.ctypes.data, r=rgb.ctypes.data):
        rc = L.lh_accel_lights_device(None, n, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data, t.ctypes.data, t.ctypes.data, good, 2, None,
                                      index, n_index, count, v, r, None)
        return rc, L.lh_last_error().decode()

    rc, err = dev(n=1 << 31); assert rc == -1 and "2^31 - 1 rays" in err, err
    rc, err = dev(index=vis.ctypes.data, n_index=(1 << 30) + 1); assert rc == -1 and "2^30 entries" in err, err
    rc, err = dev(index=vis.ctypes.data + 2, n_index=4); assert rc == -1 and "not 4-byte aligned" in err, err
    rc, err = dev(v=vis.ctypes.data + 1); assert rc == -1 and "not 4-byte aligned" in err, err
    rc, err = dev(r=rgb.ctypes.data + 2); assert rc == -1 and "not 4-byte aligned" in err, err
    rc, err = dev(); assert rc == -1 and "not committed" in err, err
    big = np.zeros((64, 3)); tm = np.zeros(65)
    rc = L.lh_accel_light_rays_device(None, 8, o.ctypes.data, o.ctypes.data, p.ctypes.data, t.ctypes.data, t.ctypes.data, t.ctypes.data, good, 2, None,
                                      vis.ctypes.data, vis.ctypes.data, big.ctypes.data, big.ctypes.data, tm.ctypes.data + 4, 64, None)
    assert rc == -1 and "not 8-byte aligned" in L.lh_last_error().decode()
    with pytest.raises(ValueError):
        binding._light_array("x", [la.Light(), "not a light"])
