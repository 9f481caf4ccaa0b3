"""The refraction chain's entry points (lh_accel_whitted_rays_device / lh_accel_whitted_device / lh_accel_whitted_host /
lh_render_whitted_tile): the C ABI and the binding, without a GPU.  The rule itself is tests/test_whitted_rule.py, the GPU side
tests/test_gpu_whitted.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_whitted_rays_device", "lh_accel_whitted_device", "lh_accel_whitted_host", "lh_render_whitted_tile")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_header_declares_them_the_struct_and_the_defaults(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the four functions to pointers of their declared types and prints the
    size and offsets of lh_whitted_params_t, LH_WHITTED_DEFAULTS and LH_WHITTED_CUT: they are the binding's"""
    src = tmp_path / "whitted.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*r)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *,
             const lh_whitted_params_t *, const void *, size_t, const void *, void *, void *, void *) = lh_accel_whitted_rays_device;
    int (*f)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *,
             const lh_whitted_params_t *, const void *, size_t, const void *, void *, void *, void *, void *, void *) = lh_accel_whitted_device;
    int (*g)(lh_accel_t *, size_t, const double *, const double *, const uint32_t *, const double *, const double *, const double *,
             const lh_whitted_params_t *, uint32_t *, double *, double *, float *) = lh_accel_whitted_host;
    int (*h)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, const lh_whitted_params_t *, void *, lh_pt_stats_t *, void *) = lh_render_whitted_tile;
    const lh_whitted_params_t d = LH_WHITTED_DEFAULTS;
    printf("%zu %zu %zu %zu %zu %d %u %d %d %.17g %.17g\n", sizeof(lh_whitted_params_t), offsetof(lh_whitted_params_t, eps),
           offsetof(lh_whitted_params_t, eta), offsetof(lh_whitted_params_t, max_depth), offsetof(lh_whitted_params_t, reserved),
           r != NULL && f != NULL && g != NULL && h != NULL, LH_WHITTED_CUT, d.max_depth, d.reserved, d.eps, d.eta);
    return 0;
}
''')
    exe = tmp_path / "whitted"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in got[:9]] == [24, 0, 8, 16, 20, 1, 0x80000000, 8, 0]
    assert [float(x) for x in got[9:]] == [1.0e-7, 1.33]
    assert C.sizeof(binding.WhittedParams) == 24
    assert [(n, getattr(binding.WhittedParams, n).offset) for n, _ in binding.WhittedParams._fields_] == [("eps", 0), ("eta", 8), ("max_depth", 16), ("reserved", 20)]
    d = la.WhittedParams()
    assert (d.eps, d.eta, d.max_depth, d.reserved) == (1.0e-7, 1.33, 8, 0)
    assert la.WHITTED_CUT == 0x80000000


def test_binding_prototypes_and_signatures():
    """one argtype per parameter of the header's prototypes (the C program above holds the prototypes to the library)"""
    L = binding.lib()
    assert len(L.lh_accel_whitted_rays_device.argtypes) == 15
    assert len(L.lh_accel_whitted_device.argtypes) == 17
    assert len(L.lh_accel_whitted_host.argtypes) == 13
    assert len(L.lh_render_whitted_tile.argtypes) == 11
    # argument order and defaults mirror the dirt methods, minus the gather's sample count, seed, keys and uniforms
    gone = ("gather_nsamples", "seed", "key", "uniforms")
    for wh, dirt in (("whitted_device", "dirt_device"), ("whitted_rays_device", "dirt_device"), ("whitted_host", "dirt_host"), ("render_whitted_tile", "render_dirt_tile")):
        pw = inspect.signature(getattr(la.HipAccel, wh)).parameters
        pd = {k: v for k, v in inspect.signature(getattr(la.HipAccel, dirt)).parameters.items() if k not in gone}
        assert list(pw) == list(pd) and [pw[k].default for k in pw] == [pd[k].default for k in pd], wh


BAD_PARAMS = [(float("nan"), 1.33, 8, 0), (1e-7, float("nan"), 8, 0), (-1e-12, 1.33, 8, 0), (float("inf"), 1.33, 8, 0), (float("-inf"), 1.33, 8, 0),
              (1e-7, 0.0, 8, 0), (1e-7, -1.33, 8, 0), (1e-7, float("inf"), 8, 0), (1e-7, 1.33, -1, 0), (1e-7, 1.33, 65, 0), (1e-7, 1.33, 8, 1), (1e-7, 1.33, 8, -1)]


def test_argument_refusals_need_no_device():
    """the parameter and argument checks come before the accelerator is looked at; the last cases are the accelerator's own"""
    L = binding.lib()
    o = np.zeros((9, 3)); t = np.zeros(9); prim = np.zeros(9, np.uint32)
    idx = np.zeros(8, np.uint32); b = np.full(9, 0x77777777, np.uint32); rgb = np.full((9, 3), 7.0, np.float32)
    eo = np.full((9, 3), 7.0); ed = np.full((9, 3), 7.0)
    O, T, P, I, B, R, EO, ED = (x.ctypes.data for x in (o, t, prim, idx, b, rgb, eo, ed))
    cam = la.Camera(); st = binding.PtStats()
    tile = np.full((4, 4, 3), 7.0, np.float32)
    calls = lambda d: (          # noqa: E731
        ("lh_accel_whitted_rays_device", lambda: L.lh_accel_whitted_rays_device(None, 8, O, O, P, T, T, T, d, None, 0, None, EO, ED, None)),
        ("lh_accel_whitted_device", lambda: L.lh_accel_whitted_device(None, 8, O, O, P, T, T, T, d, None, 0, None, B, EO, ED, R, None)),
        ("lh_accel_whitted_host", lambda: L.lh_accel_whitted_host(None, 8, O, O, P, T, T, T, d, B, EO, ED, R)),
        ("lh_render_whitted_tile", lambda: L.lh_render_whitted_tile(None, C.byref(cam), 0, 0, 4, 4, 1, d, tile.ctypes.data, C.byref(st), None)))
    for bad in BAD_PARAMS:
        d = la.WhittedParams(*bad)
        for name, call in calls(C.byref(d)):
            rc = call()
            err = L.lh_last_error().decode()
            assert rc == -1 and "bad refraction parameters" in err and name in err, (bad, name, err)
    good = la.WhittedParams(0.0, 1e-300, 0, 0); top = la.WhittedParams(1.0, 1e300, 64, 0)
    tail = (B, EO, ED, R, None)
    cases = [
        ((1 << 31, O, O, P, T, T, T, None, None, 0, None) + tail, "2^31"),
        ((8, O, O, P, T, T, T, None, None, (1 << 30) + 1, None) + tail, "2^30"),
        ((8, O, O, P, T, T, T, None, I + 2, 4, None) + tail, "4-byte aligned"),
        ((8, O, O, P, T, T, T, None, I, 8, I + 1) + tail, "4-byte aligned"),
        ((8, O + 4, O, P, T, T, T, None, None, 0, None) + tail, "8-byte aligned"),
        ((8, O, O, P, T, T + 4, T, None, None, 0, None) + tail, "8-byte aligned"),
        ((8, O, O, P + 2, T, T, T, None, None, 0, None) + tail, "4-byte"),
        ((8, O, O, P, T, T, T, None, None, 0, None, B + 2, EO, ED, R, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, None, None, 0, None, B, EO + 4, ED, R, None), "8-byte aligned"),
        ((8, O, O, P, T, T, T, None, None, 0, None, B, EO, ED + 4, R, None), "8-byte aligned"),
        ((8, O, O, P, T, T, T, None, None, 0, None, B, EO, ED, R + 1, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, None, None, 0, None) + tail, "not committed"),                  # NULL parameters: the defaults
        ((8, None, O, P, T, T, T, None, None, 0, None) + tail, "not committed"),               # a NULL array: asked after the accelerator
        ((8, O, O, P, T, T, T, C.byref(good), None, 0, None) + tail, "not committed"),         # the smallest accepted values
        ((8, O, O, P, T, T, T, C.byref(top), None, 0, None) + tail, "not committed"),          # the largest
        ((0, None, None, None, None, None, None, None, None, 0, None, None, None, None, None, None), "not committed"),
    ]
    for args, msg in cases:
        rc = L.lh_accel_whitted_device(None, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_whitted_device" in err, (args, err)
    rcases = [
        ((1 << 31, O, O, P, T, T, T, None, None, 0, None, EO, ED, None), "2^31"),
        ((8, O, O, P, T, T, T, None, None, (1 << 30) + 1, None, EO, ED, None), "2^30"),
        ((8, O, O, P, T, T, T, None, I + 1, 4, None, EO, ED, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, None, None, 0, None, EO + 4, ED, None), "8-byte aligned"),
        ((8, O, O, P, T, T, T, None, None, 0, None, EO, ED + 2, None), "8-byte aligned"),
        ((8, O, O, P, T, T, T, None, None, 0, None, EO, ED, None), "not committed"),
    ]
    for args, msg in rcases:
        rc = L.lh_accel_whitted_rays_device(None, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_whitted_rays_device" in err, (args, err)
    for name, call in calls(None)[2:]:
        rc = call()
        err = L.lh_last_error().decode()
        assert rc == -1 and name in err and "not committed" in err, (name, err)
    rc = L.lh_accel_whitted_host(None, 1 << 31, O, O, P, T, T, T, None, B, EO, ED, R)
    assert rc == -1 and "2^31" in L.lh_last_error().decode()
    assert (b == 0x77777777).all() and (rgb == 7.0).all() and (eo == 7.0).all() and (ed == 7.0).all() and (tile == 7.0).all()
