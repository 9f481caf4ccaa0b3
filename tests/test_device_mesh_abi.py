"""Device-resident meshes (lh_accel_add_mesh_device): header, library and binding agree, without a GPU.  The GPU side is
tests/test_gpu_device_mesh.py."""
import ctypes as C
import inspect
import os
import subprocess

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_point():
    L = C.CDLL(la.build_library())
    assert hasattr(L, "lh_accel_add_mesh_device")
    assert "lh_accel_add_mesh_device" in binding.ABI_SYMBOLS


def test_header_declares_it_and_the_position_formats(tmp_path):
    """a C program compiled against include/lucille_hip.h takes the function's address with its declared type and prints the
    constants: they are the binding's"""
    src = tmp_path / "device_mesh.c"
    src.write_text(r'''
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*f)(lh_accel_t *, uint32_t, const void *, int, size_t, uint32_t, const void *, void *) = lh_accel_add_mesh_device;
    printf("%d %d %d\n", LH_POS_F64, LH_POS_F32, f != NULL);
    return 0;
}
''')
    exe = tmp_path / "device_mesh"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [binding.POS_F64, binding.POS_F32, 1]
    assert (la.POS_F64, la.POS_F32) == (0, 1)


def test_binding_prototype_and_method():
    L = binding.lib()
    assert len(L.lh_accel_add_mesh_device.argtypes) == 8
    p = list(inspect.signature(la.HipAccel.add_mesh_device).parameters)
    assert p == ["self", "positions", "indices", "stream"]
    assert inspect.signature(la.HipAccel.add_mesh_device).parameters["stream"].default is None
    assert list(inspect.signature(la.HipAccel.commit).parameters) == ["self", "build_threads", "on_device", "build"]      # unchanged for callers


def test_argument_refusals_need_no_device():
    """a NULL accelerator is refused before anything else is looked at"""
    L = binding.lib()
    assert L.lh_accel_add_mesh_device(None, 0, None, binding.POS_F64, 24, 0, None, None) == -1
    assert "accel is NULL" in L.lh_last_error().decode()
