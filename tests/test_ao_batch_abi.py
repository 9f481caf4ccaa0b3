"""The AO stage for a caller's batch of hit records (lh_accel_ao_device / lh_accel_ao_host / lh_accel_ao_rays_device): the C ABI and
the binding, without a GPU.  The GPU side is tests/test_gpu_ao_batch.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_ao_device", "lh_accel_ao_host", "lh_accel_ao_rays_device")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_header_declares_them_and_the_no_hit_constant(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the three functions to pointers of their declared types and prints
    LH_AO_NO_HIT: it is the binding's"""
    src = tmp_path / "ao_batch.c"
    src.write_text(r'''
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*f)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, int, uint64_t,
             const void *, const void *, const void *, size_t, const void *, void *, void *, void *) = lh_accel_ao_device;
    int (*g)(lh_accel_t *, size_t, const double *, const double *, const uint32_t *, const double *, const double *, const double *,
             int, uint64_t, const uint64_t *, const double *, size_t, uint32_t *, float *) = lh_accel_ao_host;
    int (*h)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, const void *, const void *, int, uint64_t,
             const void *, const void *, void *, void *, void *, void *, size_t, void *) = lh_accel_ao_rays_device;
    printf("%u %d\n", LH_AO_NO_HIT, f != NULL && g != NULL && h != NULL);
    return 0;
}
''')
    exe = tmp_path / "ao_batch"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [binding.AO_NO_HIT, 1]
    assert la.AO_NO_HIT == 0xFFFFFFFF == la.MISS


def test_binding_prototypes_and_signatures():
    """one argtype per parameter of the header's prototypes: 18 for lh_accel_ao_device, 15 for lh_accel_ao_host, and 18 for
    lh_accel_ao_rays_device (its prototype has 18 parameters; the C program above holds the binding to it)"""
    L = binding.lib()
    assert len(L.lh_accel_ao_device.argtypes) == 18
    assert len(L.lh_accel_ao_host.argtypes) == 15
    assert len(L.lh_accel_ao_rays_device.argtypes) == 18
    p = inspect.signature(la.HipAccel.ao_device).parameters
    assert list(p) == ["self", "org", "dr", "records", "gather_nsamples", "seed", "key", "uniforms", "index", "count", "out", "stream"]
    assert p["seed"].default == 1 and all(p[k].default is None for k in ("key", "uniforms", "index", "count", "out", "stream"))
    assert p["gather_nsamples"].default is inspect.Parameter.empty
    p = inspect.signature(la.HipAccel.ao_rays_device).parameters
    assert list(p) == ["self", "org", "dr", "records", "gather_nsamples", "seed", "key", "uniforms", "out", "stream"]
    assert p["seed"].default == 1 and all(p[k].default is None for k in ("key", "uniforms", "out", "stream"))
    p = inspect.signature(la.HipAccel.ao_host).parameters
    assert list(p) == ["self", "org", "dr", "records", "gather_nsamples", "seed", "key", "uniforms"]
    assert p["seed"].default == 1 and p["key"].default is None and p["uniforms"].default is None
    assert "UNSPECIFIED" in la.HipAccel.ao_device.__doc__


def test_argument_refusals_need_no_device():
    """the argument checks come before the accelerator is looked at; the last case is the accelerator's own"""
    L = binding.lib()
    o = np.zeros((8, 3)); t = np.zeros(8); prim = np.zeros(8, np.uint32); key = np.zeros(9, np.uint64)
    idx = np.zeros(8, np.uint32); cnt = np.full(8, 0x77777777, np.uint32); rad = np.full(8, 7.0, np.float32)
    O, T, P = o.ctypes.data, t.ctypes.data, prim.ctypes.data
    K, I, CN, R = key.ctypes.data, idx.ctypes.data, cnt.ctypes.data, rad.ctypes.data
    cases = [
        ((8, O, O, P, T, T, T, 0, 1, None, None, None, 0, None, CN, R, None), "gather_nsamples"),
        ((1 << 31, O, O, P, T, T, T, 16, 1, None, None, None, 0, None, CN, R, None), "2^31"),
        ((8, O, O, P, T, T, T, 16, 1, None, None, None, (1 << 30) + 1, None, CN, R, None), "2^30"),
        ((8, O, O, P, T, T, T, 16, 1, None, None, I + 2, 4, None, CN, R, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, 1, None, None, I, 8, I + 1, CN, R, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, 1, K + 4, None, None, 0, None, CN, R, None), "8-byte aligned"),
        ((8, O, O, P, T, T, T, 16, 1, None, None, None, 0, None, CN + 2, R, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, 1, None, None, None, 0, None, CN, R + 1, None), "4-byte aligned"),
        ((8, O, O, P, T, T, T, 16, 1, None, None, None, 0, None, CN, R, None), "not committed"),
    ]
    for args, msg in cases:
        rc = L.lh_accel_ao_device(None, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_ao_device" in err, (args, err)
    rc = L.lh_accel_ao_rays_device(None, 8, O, O, P, T, T, T, 0, 1, None, None, CN, CN, O, O, 128, None)
    assert rc == -1 and "lh_accel_ao_rays_device" in L.lh_last_error().decode()
    rc = L.lh_accel_ao_host(None, 8, O, O, P, T, T, T, 16, 1, None, None, 0, CN, R)
    assert rc == -1 and "lh_accel_ao_host" in L.lh_last_error().decode() and "not committed" in L.lh_last_error().decode()
    assert (cnt == 0x77777777).all() and (rad == 7.0).all()
