"""Per-vertex normals and attributes of device meshes (lh_accel_set_normals_device, lh_accel_set_attribute_device): header, library
and binding agree, without a GPU.  The GPU side is tests/test_gpu_device_attr.py."""
import ctypes as C
import inspect
import os
import subprocess

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_set_normals_device", "lh_accel_set_attribute_device")


def test_library_exports_both_entry_points():
    L = C.CDLL(la.build_library())
    for name in NEW:
        assert hasattr(L, name), name
        assert name in binding.ABI_SYMBOLS


def test_header_declares_them(tmp_path):
    """a C program compiled against include/lucille_hip.h takes both addresses with their declared types"""
    src = tmp_path / "device_attr.c"
    src.write_text(r'''
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*n)(lh_accel_t *, uint32_t, uint32_t, const void *, int, size_t, int, void *) = lh_accel_set_normals_device;
    int (*a)(lh_accel_t *, uint32_t, int, uint32_t, const void *, int, size_t, void *) = lh_accel_set_attribute_device;
    printf("%d %d %d %d\n", n != NULL, a != NULL, LH_ATTR_COLOR, LH_ATTR_TEXCOORD_UNSHARED);
    return 0;
}
''')
    exe = tmp_path / "device_attr"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [1, 1, la.ATTR_COLOR, la.ATTR_TEXCOORD_UNSHARED]


def test_binding_prototypes_and_methods():
    L = binding.lib()
    assert len(L.lh_accel_set_normals_device.argtypes) == 8 and len(L.lh_accel_set_attribute_device.argtypes) == 8
    sig = inspect.signature(la.HipAccel.set_normals_device).parameters
    assert list(sig) == ["self", "mesh", "normals", "two_side", "stream"] and sig["two_side"].default == 0 and sig["stream"].default is None
    sig = inspect.signature(la.HipAccel.set_attribute_device).parameters
    assert list(sig) == ["self", "mesh", "kind", "data", "stream"] and sig["stream"].default is None


def test_null_accelerator_is_refused_before_anything_else():
    L = binding.lib()
    assert L.lh_accel_set_normals_device(None, 0, 0, None, binding.POS_F64, 24, 0, None) == -1
    assert "accel is NULL" in L.lh_last_error().decode() and "lh_accel_set_normals_device" in L.lh_last_error().decode()
    assert L.lh_accel_set_attribute_device(None, 0, la.ATTR_COLOR, 0, None, binding.POS_F64, 24, None) == -1
    assert "accel is NULL" in L.lh_last_error().decode() and "lh_accel_set_attribute_device" in L.lh_last_error().decode()


def test_existing_signatures_are_unchanged():
    """what tests/test_device_mesh_abi.py pins, and the host-pointer setters"""
    assert list(inspect.signature(la.HipAccel.add_mesh_device).parameters) == ["self", "positions", "indices", "stream"]
    assert list(inspect.signature(la.HipAccel.commit).parameters) == ["self", "build_threads", "on_device", "build"]
    assert list(inspect.signature(la.HipAccel.set_normals).parameters) == ["self", "mesh", "normals", "two_side"]
    assert list(inspect.signature(la.HipAccel.set_attribute).parameters) == ["self", "mesh", "kind", "data"]
    L = binding.lib()
    assert len(L.lh_accel_add_mesh_device.argtypes) == 8 and len(L.lh_accel_set_normals.argtypes) == 5
    assert len(L.lh_accel_set_attribute.argtypes) == 6
