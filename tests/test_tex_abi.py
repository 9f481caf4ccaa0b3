"""Material textures (lh_accel_set_texture / _set_texture_device, lh_accel_texture_device / _host, lh_multi_set_texture): the C ABI and
the binding, without a GPU.  The rule itself is tests/test_tex_rule.py, the GPU side tests/test_gpu_tex.py.

The refusals that look at the arguments alone are checked here on any machine; the ones that need an accelerator (mesh out of range,
not a device pointer) and set / replace / remove on an uncommitted accelerator need a visible device to create one -- the library has
no CPU fallback -- and are checked here where there is one, and again in tests/test_gpu_tex.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_set_texture", "lh_accel_set_texture_device", "lh_accel_texture_device", "lh_accel_texture_host", "lh_multi_set_texture")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_header_declares_them(tmp_path):
    """a C program compiled against include/lucille_hip.h assigns the functions to pointers of their declared types"""
    src = tmp_path / "tex.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*a)(lh_accel_t *, uint32_t, const float *, int, int) = lh_accel_set_texture;
    int (*b)(lh_accel_t *, uint32_t, const void *, int, int, void *) = lh_accel_set_texture_device;
    int (*c)(lh_accel_t *, size_t, const void *, const void *, const void *, const void *, size_t, const void *, void *, void *) = lh_accel_texture_device;
    int (*d)(lh_accel_t *, size_t, const uint32_t *, const double *, const double *, double *) = lh_accel_texture_host;
    int (*e)(lh_multi_t *, uint32_t, const float *, int, int) = lh_multi_set_texture;
    printf("%d %u\n", a != NULL && b != NULL && c != NULL && d != NULL && e != NULL, LH_ALL_MESHES);
    return 0;
}
''')
    exe = tmp_path / "tex"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    assert subprocess.check_output([str(exe)]).decode().split() == ["1", str(0xFFFFFFFF)]


def test_binding_prototypes_and_signatures():
    L = binding.lib()
    assert len(L.lh_accel_set_texture.argtypes) == 5
    assert len(L.lh_accel_set_texture_device.argtypes) == 6
    assert len(L.lh_accel_texture_device.argtypes) == 10
    assert len(L.lh_accel_texture_host.argtypes) == 6
    assert len(L.lh_multi_set_texture.argtypes) == 5
    p = inspect.signature(la.HipAccel.set_texture).parameters
    assert list(p) == ["self", "mesh", "texels", "stream"] and p["stream"].default is None
    p = inspect.signature(la.HipAccel.texture_device).parameters
    assert list(p) == ["self", "records", "index", "count", "out", "stream"]
    assert list(inspect.signature(la.HipAccel.texture_host).parameters) == ["self", "prim", "u", "v"]
    assert list(inspect.signature(la.HipMulti.set_texture).parameters) == ["self", "mesh", "texels"]


def test_argument_refusals_need_no_device():
    """the checks of the array and its size come before the accelerator is looked at; then the accelerator's own"""
    L = binding.lib()
    tex = np.full((2, 3, 4), 0.5, np.float32); T = tex.ctypes.data
    setters = (("lh_accel_set_texture", lambda *a: L.lh_accel_set_texture(None, 0, *a)),
               ("lh_accel_set_texture_device", lambda *a: L.lh_accel_set_texture_device(None, 0, *a, None)))
    for name, call in setters:
        for args, msg in (((T, 0, 2), "bad texture size"), ((T, 3, 0), "bad texture size"), ((T, -1, 2), "bad texture size"),
                          ((T, 65537, 2), "bad texture size"), ((T, 3, 65537), "bad texture size"), ((None, 3, 0), "bad texture size"),
                          ((None, 3, 2), "NULL array"), ((T + 2, 3, 1), "not 4-byte aligned"),
                          ((T, 3, 2), "accel is NULL"), ((T, 65536, 65536), "accel is NULL"), ((None, 0, 0), "accel is NULL")):
            rc = call(*args)
            err = L.lh_last_error().decode()
            assert rc == -1 and msg in err and name in err, (name, args, err)
    rc = L.lh_multi_set_texture(None, 0, T, 3, 2)
    assert rc == -1 and "lh_multi_set_texture" in L.lh_last_error().decode() and "not committed" in L.lh_last_error().decode()
    # the batch fetch
    prim = np.zeros(8, np.uint32); u = np.zeros(9); out = np.full((8, 4), 7.0); idx = np.zeros(8, np.uint32)
    P, U, O, I = prim.ctypes.data, u.ctypes.data, out.ctypes.data, idx.ctypes.data
    for args, msg in (((1 << 31, P, U, U, None, 0, None, O, None), "2^31"),
                      ((8, P, U, U, None, (1 << 30) + 1, None, O, None), "2^30"),
                      ((8, P, U, U, I + 2, 4, None, O, None), "4-byte aligned"),
                      ((8, P, U, U, I, 8, I + 1, O, None), "4-byte aligned"),
                      ((8, P + 2, U, U, None, 0, None, O, None), "4-byte aligned"),
                      ((8, P, U + 4, U, None, 0, None, O, None), "8-byte aligned"),
                      ((8, P, U, U + 4, None, 0, None, O, None), "8-byte aligned"),
                      ((8, P, U, U, None, 0, None, O + 4, None), "8-byte aligned"),
                      ((8, P, U, U, None, 0, None, O, None), "not committed")):
        rc = L.lh_accel_texture_device(None, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_texture_device" in err, (args, err)
    rc = L.lh_accel_texture_host(None, 8, P, U, U, O)
    assert rc == -1 and "lh_accel_texture_host" in L.lh_last_error().decode() and "not committed" in L.lh_last_error().decode()
    assert (out == 7.0).all()


def uncommitted_set_replace_remove():
    """set, replace and remove on an accelerator that is not committed (host meshes: no device memory is touched); the refusals that
    need an accelerator.  Shared with tests/test_gpu_tex.py"""
    L = binding.lib()
    acc = la.HipAccel(0)
    try:
        P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]); idx = np.array([0, 1, 2], np.uint32)
        a = np.full((2, 3, 4), 0.5, np.float32); b = np.full((5, 1, 4), 2.0, np.float32)
        # no mesh yet: every ordinal is out of range, "all meshes" is nobody
        assert L.lh_accel_set_texture(acc.h, 0, a.ctypes.data, 3, 2) == -1 and "mesh 0 out of range" in L.lh_last_error().decode()
        acc.set_texture(la.ALL_MESHES, a)
        acc.add_mesh(P, idx); acc.add_mesh(P + 2.0, idx)
        assert L.lh_accel_set_texture(acc.h, 2, a.ctypes.data, 3, 2) == -1 and "mesh 2 out of range" in L.lh_last_error().decode()
        assert L.lh_accel_set_texture(acc.h, 2, None, 0, 0) == -1 and "mesh 2 out of range" in L.lh_last_error().decode()
        acc.set_texture(0, a)                  # set
        acc.set_texture(0, b)                  # replace
        acc.set_texture(1, a)
        acc.set_texture(la.ALL_MESHES, b)      # replace both with one shared block
        acc.set_texture(1, None)               # remove
        acc.set_texture(1, None)               # ... twice
        acc.set_texture(la.ALL_MESHES, None)
        acc.set_texture(0, a)                  # left set: lh_accel_destroy frees it
        # a refusal changes nothing: the call after it still works
        assert L.lh_accel_set_texture(acc.h, 0, a.ctypes.data, 0, 2) == -1 and "bad texture size" in L.lh_last_error().decode()
        assert L.lh_accel_set_texture_device(acc.h, 0, a.ctypes.data, 3, 2, None) == -1
        assert "not a device pointer" in L.lh_last_error().decode() and "lh_accel_set_texture_device" in L.lh_last_error().decode()
        acc.set_texture(0, b)
    finally:
        acc.close()


def test_set_replace_remove_on_an_uncommitted_accelerator():
    if la.device_count() == 0:
        pytest.skip("creating an accelerator needs a visible device (there is no CPU fallback); tests/test_gpu_tex.py runs this on the GPU")
    uncommitted_set_replace_remove()
