"""The sun-and-sky light's entry points (lh_sky_from_site / lh_accel_set_sky / lh_accel_sky_device / lh_accel_sky_host) and lh_sky_t: the C
ABI and the binding, without a GPU.  The rule itself is tests/test_sky_rule.py, the GPU side tests/test_gpu_sky.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_sky_from_site", "lh_accel_set_sky", "lh_accel_sky_device", "lh_accel_sky_host")
LAYOUT = [("sun_theta", 0), ("sun_phi", 4), ("perez_x", 8), ("perez_y", 28), ("perez_Y", 48), ("zenith_x", 68), ("zenith_y", 72), ("zenith_Y", 76),
          ("basis_rgb", 80), ("basis_y", 116), ("sun_rgb", 128), ("flags", 140), ("sun_dir", 144)]


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)
    assert la.Sky is binding.Sky and la.SKY_SUN == 1


def test_header_declares_them_and_the_layout_is_the_bindings(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the four functions to pointers of their declared types and prints the size,
    the alignment and every offset of lh_sky_t and the flag: they are the documented ones and the binding's; lh_env_params_t stays 16 bytes"""
    src = tmp_path / "sky.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
#define O(f) printf(" %zu", offsetof(lh_sky_t, f))
int main(void)
{
    int (*f)(lh_sky_t *, float, float, float, int, float, float) = lh_sky_from_site;
    int (*g)(lh_accel_t *, const lh_sky_t *) = lh_accel_set_sky;
    int (*p)(lh_accel_t *, size_t, const void *, void *, void *) = lh_accel_sky_device;
    int (*q)(lh_accel_t *, size_t, const double *, float *) = lh_accel_sky_host;
    printf("%zu %zu %zu %u %u %d", sizeof(lh_sky_t), _Alignof(lh_sky_t), sizeof(lh_env_params_t), LH_SKY_SUN, LH_SKY_FLAGS, f != NULL && g != NULL && p != NULL && q != NULL);
    O(sun_theta); O(sun_phi); O(perez_x); O(perez_y); O(perez_Y); O(zenith_x); O(zenith_y); O(zenith_Y); O(basis_rgb); O(basis_y); O(sun_rgb); O(flags); O(sun_dir);
    printf(" %zu %zu\n", sizeof(((lh_sky_t *)0)->basis_rgb), sizeof(((lh_sky_t *)0)->sun_dir));
    return 0;
}
''')
    exe = tmp_path / "sky"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got[:6] == [168, 8, 16, 1, 1, 1]
    assert got[6:19] == [o for _, o in LAYOUT] and got[19:] == [36, 24]
    assert C.sizeof(binding.Sky) == 168 and C.alignment(binding.Sky) == 8
    assert [(n, getattr(binding.Sky, n).offset) for n, _ in binding.Sky._fields_] == LAYOUT
    assert C.sizeof(binding.EnvParams) == 16


def test_binding_prototypes_and_signatures():
    L = binding.lib()
    assert len(L.lh_sky_from_site.argtypes) == 7 and len(L.lh_accel_set_sky.argtypes) == 2
    assert len(L.lh_accel_sky_device.argtypes) == 5 and len(L.lh_accel_sky_host.argtypes) == 4
    assert list(inspect.signature(la.HipAccel.sky_device).parameters) == list(inspect.signature(la.HipAccel.environment_device).parameters)
    assert list(inspect.signature(la.HipAccel.sky_host).parameters) == list(inspect.signature(la.HipAccel.environment_host).parameters)
    assert list(inspect.signature(la.HipAccel.set_sky).parameters) == ["self", "sky"]
    assert list(inspect.signature(la.HipAccel.reset_sky).parameters) == ["self"]


def test_from_site_needs_no_device_and_leaves_the_callers_fields_alone():
    L = binding.lib()
    s = la.Sky()
    s.basis_y[:] = [1.0, 2.0, 3.0]; s.sun_rgb[:] = [4.0, 5.0, 6.0]; s.flags = 1; s.basis_rgb[2][1] = 7.0
    assert L.lh_sky_from_site(C.byref(s), 35.39, 139.44, 9.0, 20, 10.5, 2.0) == 0
    assert list(s.basis_y) == [1.0, 2.0, 3.0] and list(s.sun_rgb) == [4.0, 5.0, 6.0] and s.flags == 1 and s.basis_rgb[2][1] == 7.0
    assert 0.0 < s.sun_theta < np.pi / 2 and abs(np.linalg.norm(list(s.sun_dir)) - 1.0) < 1e-6 and s.sun_dir[1] > 0.0          # a morning sun, above the horizon (y is up)
    assert s.sun_dir[1] == float(np.float32(np.cos(np.float64(s.sun_theta))))                                                 # y and z swapped: the zenith angle's cosine is y
    assert s.zenith_Y > 0.0 and s.perez_Y[0] == np.float32(0.17872 * np.float64(np.float32(2.0)) - 1.46303)
    assert L.lh_sky_from_site(None, 35.39, 139.44, 9.0, 20, 10.5, 2.0) == -1
    for bad in (float("nan"), float("inf")):
        for k in (0, 1, 2, 4, 5):
            a = [35.39, 139.44, 9.0, 20, 10.5, 2.0]; a[k] = bad
            assert L.lh_sky_from_site(C.byref(s), *a) == -1, (k, bad)
    t = la.Sky.from_site(35.39, 139.44, 9.0, 20, 10.5, 2.0, basis_rgb=np.arange(9.0).reshape(3, 3), basis_y=[1, 2, 3], sun_rgb=(4, 5, 6), flags=la.SKY_SUN)
    assert t.sun_theta == s.sun_theta and [list(r) for r in t.basis_rgb] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]] and t.flags == 1
    with pytest.raises(ValueError):
        la.Sky.from_site(float("nan"), 139.44, 9.0, 20, 10.5, 2.0)


def test_refusals_need_no_device():
    """a bad struct is refused before the accelerator is looked at; a good one on an accelerator that is not committed, by the accelerator"""
    L = binding.lib()
    good = la.Sky.from_site(35.39, 139.44, 9.0, 20, 10.5, 2.0, basis_rgb=np.ones((3, 3)), basis_y=np.ones(3), sun_rgb=(1, 1, 1), flags=la.SKY_SUN)

    def refused(sky, msg):
        rc = L.lh_accel_set_sky(None, C.byref(sky) if sky is not None else None)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_set_sky" in err, err

    refused(good, "not committed")
    refused(None, "not committed")
    for name, _ in binding.Sky._fields_:
        for bad in (float("nan"), float("inf"), float("-inf")):
            s = la.Sky.from_buffer_copy(good)
            f = getattr(s, name)
            if name == "flags":
                continue
            if name == "basis_rgb":
                f[1][2] = bad
            elif hasattr(f, "__len__"):
                f[len(f) - 1] = bad
            else:
                setattr(s, name, bad)
            refused(s, "bad sky parameters")
    for flags in (2, 3, 1 << 31, 0x100):
        s = la.Sky.from_buffer_copy(good); s.flags = flags
        refused(s, "bad sky parameters")
    o = np.zeros((8, 3)); r = np.full((8, 3), 7.0, np.float32)
    for name, call in (("lh_accel_sky_device", lambda: L.lh_accel_sky_device(None, 8, o.ctypes.data, r.ctypes.data, None)),
                       ("lh_accel_sky_host", lambda: L.lh_accel_sky_host(None, 8, o.ctypes.data, r.ctypes.data))):
        rc = call()
        err = L.lh_last_error().decode()
        assert rc == -1 and name in err and "not committed" in err, (name, err)
    assert (r == 7.0).all()
