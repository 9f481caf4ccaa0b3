"""The environment-lit gather's entry points (lh_accel_env_device / lh_accel_env_host / lh_render_env_tile / lh_accel_environment_device /
lh_accel_environment_host): the C ABI and the binding, without a GPU.  The rule itself is tests/test_env_rule.py, the GPU side
tests/test_gpu_envgather.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_env_device", "lh_accel_env_host", "lh_render_env_tile", "lh_accel_environment_device", "lh_accel_environment_host")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_header_declares_them_the_struct_and_the_defaults(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the five functions to pointers of their declared types and prints
    the size of lh_env_params_t and LH_ENV_DEFAULTS: they are the binding's"""
    src = tmp_path / "env.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*f)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, int,
             const lh_env_params_t *, uint64_t, const void *, const void *, const void *, size_t, const void *, void *, void *, void *) = lh_accel_env_device;
    int (*g)(lh_accel_t *, size_t, const double *, const double *, const uint32_t *, const double *, const double *, const double *,
             int, const lh_env_params_t *, uint64_t, const uint64_t *, const double *, size_t, uint32_t *, float *) = lh_accel_env_host;
    int (*h)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, int, const lh_env_params_t *, uint64_t, const void *, void *,
             lh_tile_stats_t *, void *) = lh_render_env_tile;
    int (*p)(lh_accel_t *, size_t, const void *, void *, void *) = lh_accel_environment_device;
    int (*q)(lh_accel_t *, size_t, const double *, float *) = lh_accel_environment_host;
    const lh_env_params_t d = LH_ENV_DEFAULTS;
    printf("%zu %zu %zu %d %.17g %.17g\n", sizeof(lh_env_params_t), offsetof(lh_env_params_t, eps), offsetof(lh_env_params_t, scale),
           f != NULL && g != NULL && h != NULL && p != NULL && q != NULL, d.eps, d.scale);
    return 0;
}
''')
    exe = tmp_path / "env"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in got[:4]] == [16, 0, 8, 1]
    assert [float(x) for x in got[4:]] == [1.0e-5, 1.0]
    assert C.sizeof(binding.EnvParams) == 16
    assert [(n, getattr(binding.EnvParams, n).offset) for n, _ in binding.EnvParams._fields_] == [("eps", 0), ("scale", 8)]
    d = la.EnvParams()
    assert (d.eps, d.scale) == (1.0e-5, 1.0)


def test_binding_prototypes_and_signatures():
    """one argtype per parameter of the header's prototypes (the C program above holds the prototypes to the library)"""
    L = binding.lib()
    assert len(L.lh_accel_env_device.argtypes) == 19
    assert len(L.lh_accel_env_host.argtypes) == 16
    assert len(L.lh_render_env_tile.argtypes) == 14
    assert len(L.lh_accel_environment_device.argtypes) == 5
    assert len(L.lh_accel_environment_host.argtypes) == 4
    # argument order and defaults mirror the dirt methods
    for env, dirt in (("env_device", "dirt_device"), ("env_host", "dirt_host"), ("render_env_tile", "render_dirt_tile")):
        pe = inspect.signature(getattr(la.HipAccel, env)).parameters
        pd = inspect.signature(getattr(la.HipAccel, dirt)).parameters
        assert list(pe) == list(pd) and [pe[k].default for k in pe] == [pd[k].default for k in pd], env
    assert list(inspect.signature(la.HipAccel.environment_device).parameters) == ["self", "dirs", "out", "stream"]
    assert list(inspect.signature(la.HipAccel.environment_host).parameters) == ["self", "dirs"]


BAD_PARAMS = [(float("nan"), 1.0), (1e-5, float("nan")), (-1e-9, 1.0), (1e-5, -0.5), (float("inf"), 1.0), (1e-5, float("inf")), (float("-inf"), 1.0)]


def test_argument_refusals_need_no_device():
    """the parameter and argument checks come before the accelerator is looked at; the last cases are the accelerator's own"""
    L = binding.lib()
    o = np.zeros((8, 3)); t = np.zeros(8); prim = np.zeros(8, np.uint32); key = np.zeros(9, np.uint64)
    idx = np.zeros(8, np.uint32); cnt = np.full(8, 0x77777777, np.uint32); val = np.full((8, 3), 7.0, np.float32)
    O, T, P = o.ctypes.data, t.ctypes.data, prim.ctypes.data
    K, I, CN, R = key.ctypes.data, idx.ctypes.data, cnt.ctypes.data, val.ctypes.data
    cam = la.Camera(); st = binding.TileStats()
    rgb = np.full((4, 4, 3), 7.0, np.float32)
    for bad in BAD_PARAMS:
        d = la.EnvParams(*bad)
        for name, call in (("lh_accel_env_device", lambda: L.lh_accel_env_device(None, 8, O, O, P, T, T, T, 16, C.byref(d), 1, None, None, None, 0, None, CN, R, None)),
                           ("lh_accel_env_host", lambda: L.lh_accel_env_host(None, 8, O, O, P, T, T, T, 16, C.byref(d), 1, None, None, 0, CN, R)),
                           ("lh_render_env_tile", lambda: L.lh_render_env_tile(None, C.byref(cam), 0, 0, 4, 4, 1, 16, C.byref(d), 1, None, rgb.ctypes.data, C.byref(st), None))):
            rc = call()
            err = L.lh_last_error().decode()
            assert rc == -1 and "bad environment-gather parameters" in err and name in err, (bad, name, err)
    good = la.EnvParams(0.0, 0.0)
    cases = [
        ((8, O, O, P, T, T, T, 0, None, 1, None, None, None, 0, None, CN, R, None), "gather_nsamples"),
        ((1 << 31, O, O, P, T, T, T, 16, None, 1, None, None, None, 0, None, CN, R, None), "2^31"),
        ((8, O, O, P, T, T, T, 16, None, 1, None, None, None, (1 << 30) + 1, None, CN, R, None), "2^30"),
        ((8, O, O, P, T, T, T, 16, None, 1, None, None, I + 2, 4, None, CN, R, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, None, 1, None, None, I, 8, I + 1, CN, R, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, None, 1, K + 4, None, None, 0, None, CN, R, None), "8-byte aligned"),
        ((8, O, O, P, T, T, T, 16, None, 1, None, None, None, 0, None, CN + 2, R, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, None, 1, None, None, None, 0, None, CN, R + 1, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, None, 1, None, None, None, 0, None, CN, R, None), "not committed"),          # NULL parameters: the defaults
        ((8, O, O, P, T, T, T, 16, C.byref(good), 1, None, None, None, 0, None, CN, R, None), "not committed"),  # the smallest accepted pair
    ]
    for args, msg in cases:
        rc = L.lh_accel_env_device(None, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_env_device" in err, (args, err)
    for name, call in (("lh_accel_env_host", lambda: L.lh_accel_env_host(None, 8, O, O, P, T, T, T, 16, None, 1, None, None, 0, CN, R)),
                       ("lh_render_env_tile", lambda: L.lh_render_env_tile(None, C.byref(cam), 0, 0, 4, 4, 1, 16, None, 1, None, rgb.ctypes.data, C.byref(st), None)),
                       ("lh_accel_environment_device", lambda: L.lh_accel_environment_device(None, 8, O, R, None)),
                       ("lh_accel_environment_host", lambda: L.lh_accel_environment_host(None, 8, O, R))):
        rc = call()
        err = L.lh_last_error().decode()
        assert rc == -1 and name in err and "not committed" in err, (name, err)
    assert (cnt == 0x77777777).all() and (val == 7.0).all() and (rgb == 7.0).all()
