"""Updatable device meshes (lh_accel_update_mesh_device, lh_accel_recommit): header, library and binding agree, without a GPU.  The GPU side is
tests/test_gpu_recommit.py, the plan of a re-commit tests/test_recommit_plan.py."""
import ctypes as C
import inspect
import os
import subprocess

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_both_entry_points():
    L = C.CDLL(la.build_library())
    for name in ("lh_accel_update_mesh_device", "lh_accel_recommit", "lh_accel_danger_list"):
        assert hasattr(L, name), name
        assert name in binding.ABI_SYMBOLS


def test_header_declares_them_and_the_info_struct(tmp_path):
    """a C program compiled against include/lucille_hip.h takes both addresses with the declared types and prints the size and the offsets of
    lh_recommit_info_t: they are the binding's structure's"""
    src = tmp_path / "recommit.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*u)(lh_accel_t *, uint32_t, uint32_t, const void *, int, size_t, void *) = lh_accel_update_mesh_device;
    int (*r)(lh_accel_t *, lh_recommit_info_t *) = lh_accel_recommit;
    int (*d)(const lh_accel_t *, uint32_t *, uint32_t *, uint32_t *, double *) = lh_accel_danger_list;
    printf("%zu %zu %zu %zu %zu %d\n", sizeof(lh_recommit_info_t), offsetof(lh_recommit_info_t, flattened), offsetof(lh_recommit_info_t, rebuilt_trees),
           offsetof(lh_recommit_info_t, regathered), offsetof(lh_recommit_info_t, seconds), u != NULL && r != NULL && d != NULL);
    return 0;
}
''')
    exe = tmp_path / "recommit"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    R = binding.RecommitInfo
    assert got == [C.sizeof(R), R.flattened.offset, R.rebuilt_trees.offset, R.regathered.offset, R.seconds.offset, 1]
    assert C.sizeof(R) == 24 and R.seconds.offset == 16


def test_binding_prototypes_and_methods():
    L = binding.lib()
    vp, u32 = C.c_void_p, C.c_uint32
    assert L.lh_accel_update_mesh_device.argtypes == [vp, u32, u32, vp, C.c_int, C.c_size_t, vp]
    assert L.lh_accel_recommit.argtypes == [vp, C.POINTER(binding.RecommitInfo)]
    sig = inspect.signature(la.HipAccel.update_mesh_device)
    assert list(sig.parameters) == ["self", "mesh", "positions", "stream"] and sig.parameters["stream"].default is None
    assert list(inspect.signature(la.HipAccel.recommit).parameters) == ["self"]
    # unchanged for callers
    assert list(inspect.signature(la.HipAccel.set_normals_device).parameters) == ["self", "mesh", "normals", "two_side", "stream"]
    assert list(inspect.signature(la.HipAccel.set_attribute_device).parameters) == ["self", "mesh", "kind", "data", "stream"]


def test_a_null_accelerator_is_refused_before_anything_is_looked_at():
    L = binding.lib()
    assert L.lh_accel_update_mesh_device(None, 0, 0, None, 7, 1, None) == -1          # the format and the stride are bad too: not reached
    assert "lh_accel_update_mesh_device: accel is NULL" in L.lh_last_error().decode()
    info = binding.RecommitInfo(1, 1, 1, 1.0)
    assert L.lh_accel_recommit(None, C.byref(info)) == -1
    assert "lh_accel_recommit: accel is NULL" in L.lh_last_error().decode()
    assert L.lh_accel_recommit(None, None) == -1
    assert L.lh_accel_danger_list(None, None, None, None, None) == -1 and "not committed" in L.lh_last_error().decode()
