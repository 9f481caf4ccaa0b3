"""The dirtmap transport's entry points (lh_accel_dirt_device / lh_accel_dirt_host / lh_render_dirt_tile): the C ABI and the binding,
without a GPU.  The rule itself is tests/test_dirt_rule.py, the GPU side tests/test_gpu_dirt.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_dirt_device", "lh_accel_dirt_host", "lh_render_dirt_tile")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_header_declares_them_the_struct_and_the_defaults(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the three functions to pointers of their declared types and prints
    the size of lh_dirt_params_t and LH_DIRT_DEFAULTS: they are the binding's"""
    src = tmp_path / "dirt.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*f)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, int,
             const lh_dirt_params_t *, uint64_t, const void *, const void *, const void *, size_t, const void *, void *, void *, void *) = lh_accel_dirt_device;
    int (*g)(lh_accel_t *, size_t, const double *, const double *, const uint32_t *, const double *, const double *, const double *,
             int, const lh_dirt_params_t *, uint64_t, const uint64_t *, const double *, size_t, uint32_t *, float *) = lh_accel_dirt_host;
    int (*h)(lh_accel_t *, const lh_camera_t *, int, int, int, int, int, int, const lh_dirt_params_t *, uint64_t, const void *, void *,
             lh_tile_stats_t *, void *) = lh_render_dirt_tile;
    const lh_dirt_params_t d = LH_DIRT_DEFAULTS;
    printf("%zu %zu %zu %zu %d %.17g %.17g %.17g\n", sizeof(lh_dirt_params_t), offsetof(lh_dirt_params_t, near_clip), offsetof(lh_dirt_params_t, far_clip),
           offsetof(lh_dirt_params_t, eps), f != NULL && g != NULL && h != NULL, d.near_clip, d.far_clip, d.eps);
    return 0;
}
''')
    exe = tmp_path / "dirt"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in got[:5]] == [24, 0, 8, 16, 1]
    assert [float(x) for x in got[5:]] == [0.1, 0.5, 1.0e-5]
    assert C.sizeof(binding.DirtParams) == 24
    assert [(n, getattr(binding.DirtParams, n).offset) for n, _ in binding.DirtParams._fields_] == [("near_clip", 0), ("far_clip", 8), ("eps", 16)]
    d = la.DirtParams()
    assert (d.near_clip, d.far_clip, d.eps) == (0.1, 0.5, 1.0e-5)


def test_binding_prototypes_and_signatures():
    """one argtype per parameter of the header's prototypes (the C program above holds the prototypes to the library)"""
    L = binding.lib()
    assert len(L.lh_accel_dirt_device.argtypes) == 19
    assert len(L.lh_accel_dirt_host.argtypes) == 16
    assert len(L.lh_render_dirt_tile.argtypes) == 14
    p = inspect.signature(la.HipAccel.dirt_device).parameters
    assert list(p) == ["self", "org", "dr", "records", "gather_nsamples", "params", "seed", "key", "uniforms", "index", "count", "out", "stream"]
    assert p["seed"].default == 1 and all(p[k].default is None for k in ("params", "key", "uniforms", "index", "count", "out", "stream"))
    p = inspect.signature(la.HipAccel.dirt_host).parameters
    assert list(p) == ["self", "org", "dr", "records", "gather_nsamples", "params", "seed", "key", "uniforms"]
    p = inspect.signature(la.HipAccel.render_dirt_tile).parameters
    assert list(p) == ["self", "cam", "x0", "y0", "w", "h", "pixel_samples", "gather_nsamples", "params", "seed", "uniforms", "out", "stream"]
    # the AO twins keep their signatures
    p = inspect.signature(la.HipAccel.ao_device).parameters
    assert list(p) == ["self", "org", "dr", "records", "gather_nsamples", "seed", "key", "uniforms", "index", "count", "out", "stream"]


BAD_PARAMS = [(float("nan"), 0.5, 1e-5), (0.1, float("nan"), 1e-5), (0.1, 0.5, float("nan")), (-0.1, 0.5, 1e-5), (0.5, 0.5, 1e-5), (0.6, 0.5, 1e-5),
              (0.1, float("inf"), 1e-5), (0.1, 1.1e38, 1e-5), (0.1, 0.5, -1e-9), (0.1, 0.5, float("inf")), (float("-inf"), 0.5, 0.0)]


def test_argument_refusals_need_no_device():
    """the argument checks come before the accelerator is looked at; the last cases are the accelerator's own"""
    L = binding.lib()
    o = np.zeros((8, 3)); t = np.zeros(8); prim = np.zeros(8, np.uint32); key = np.zeros(9, np.uint64)
    idx = np.zeros(8, np.uint32); cnt = np.full(8, 0x77777777, np.uint32); val = np.full(8, 7.0, np.float32)
    O, T, P = o.ctypes.data, t.ctypes.data, prim.ctypes.data
    K, I, CN, R = key.ctypes.data, idx.ctypes.data, cnt.ctypes.data, val.ctypes.data
    cam = la.Camera(); st = binding.TileStats()
    rgb = np.full((4, 4, 3), 7.0, np.float32)
    for bad in BAD_PARAMS:
        d = la.DirtParams(*bad)
        for name, call in (("lh_accel_dirt_device", lambda: L.lh_accel_dirt_device(None, 8, O, O, P, T, T, T, 16, C.byref(d), 1, None, None, None, 0, None, CN, R, None)),
                           ("lh_accel_dirt_host", lambda: L.lh_accel_dirt_host(None, 8, O, O, P, T, T, T, 16, C.byref(d), 1, None, None, 0, CN, R)),
                           ("lh_render_dirt_tile", lambda: L.lh_render_dirt_tile(None, C.byref(cam), 0, 0, 4, 4, 1, 16, C.byref(d), 1, None, rgb.ctypes.data, C.byref(st), None))):
            rc = call()
            err = L.lh_last_error().decode()
            assert rc == -1 and "bad dirt parameters" in err and name in err, (bad, name, err)
    good = la.DirtParams(0.0, 1.0e38, 0.0)
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
        ((8, O, O, P, T, T, T, 16, C.byref(good), 1, None, None, None, 0, None, CN, R, None), "not committed"),  # the widest accepted clips
    ]
    for args, msg in cases:
        rc = L.lh_accel_dirt_device(None, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_dirt_device" in err, (args, err)
    rc = L.lh_accel_dirt_host(None, 8, O, O, P, T, T, T, 16, None, 1, None, None, 0, CN, R)
    assert rc == -1 and "lh_accel_dirt_host" in L.lh_last_error().decode() and "not committed" in L.lh_last_error().decode()
    rc = L.lh_render_dirt_tile(None, C.byref(cam), 0, 0, 4, 4, 1, 16, None, 1, None, rgb.ctypes.data, C.byref(st), None)
    assert rc == -1 and "lh_render_dirt_tile" in L.lh_last_error().decode() and "not committed" in L.lh_last_error().decode()
    assert (cnt == 0x77777777).all() and (val == 7.0).all() and (rgb == 7.0).all()
