"""Indexed ray batches and hit compaction (lh_accel_intersect_device_indexed / lh_accel_compact_device): the C ABI and the
binding, without a GPU.  The GPU side is tests/test_gpu_indexed.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_intersect_device_indexed", "lh_accel_compact_device")


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_header_declares_them_and_the_select_constants(tmp_path):
    """a C program compiled against include/lucille_hip.h takes the address of both functions with their declared types and
    prints the constants: they are the binding's"""
    src = tmp_path / "indexed.c"
    src.write_text(r'''
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*f)(lh_accel_t *, size_t, const void *, const void *, int, int, void *, void *, void *, void *, void *, int,
             const void *, size_t, const void *, void *) = lh_accel_intersect_device_indexed;
    int (*g)(size_t, int, const void *, const void *, int, const void *, size_t, const void *, void *, void *, void *) =
        lh_accel_compact_device;
    printf("%d %d %d %d %d\n", LH_SELECT_HIT, LH_SELECT_MISS, LH_SELECT_OCCLUDED, LH_SELECT_UNOCCLUDED, f != NULL && g != NULL);
    return 0;
}
''')
    exe = tmp_path / "indexed"
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [binding.SELECT_HIT, binding.SELECT_MISS, binding.SELECT_OCCLUDED, binding.SELECT_UNOCCLUDED, 1]
    assert (la.SELECT_HIT, la.SELECT_MISS, la.SELECT_OCCLUDED, la.SELECT_UNOCCLUDED) == (0, 1, 2, 3)


def test_binding_prototypes_and_signatures():
    L = binding.lib()
    assert len(L.lh_accel_intersect_device_indexed.argtypes) == 16
    assert len(L.lh_accel_compact_device.argtypes) == 11
    p = inspect.signature(la.HipAccel.intersect_device).parameters
    assert p["index"].default is None and p["count"].default is None
    assert "UNSPECIFIED" in la.HipAccel.intersect_device.__doc__ and "UNSPECIFIED" in la.HipAccel.intersect_device_indexed.__doc__
    assert list(inspect.signature(binding.compact).parameters)[:5] == ["records_or_occluded", "select", "index", "count", "out"]
    assert la.compact is binding.compact


def test_indexed_refusals_need_no_device():
    """the argument checks come before the accelerator is looked at: every refusal of lh_accel_intersect_device_ex, and the list's own"""
    L = binding.lib()
    rec = binding._rec16_host(8)
    o = np.zeros((8, 3), np.float32)
    t = np.zeros(8)
    idx = np.zeros(8, np.uint32)
    cases = [
        (2, binding.REC_F64, rec.ctypes.data, None, la.MODE_CLOSEST, idx.ctypes.data, 8, None, "ray format"),
        (binding.RAYS_F32, 5, rec.ctypes.data, None, la.MODE_CLOSEST, idx.ctypes.data, 8, None, "record format"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, 7, idx.ctypes.data, 8, None, "mode"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, la.MODE_ANY, idx.ctypes.data, 8, None, "any-hit"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, t.ctypes.data, la.MODE_CLOSEST, idx.ctypes.data, 8, None, "must be NULL"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data + 4, None, la.MODE_CLOSEST, idx.ctypes.data, 8, None, "aligned"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, la.MODE_CLOSEST, None, (1 << 30) + 1, None, "2^30"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, la.MODE_CLOSEST, idx.ctypes.data + 2, 4, None, "4-byte aligned"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, la.MODE_CLOSEST, idx.ctypes.data, 8, idx.ctypes.data + 1, "4-byte aligned"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, la.MODE_CLOSEST, idx.ctypes.data, 8, None, "not committed"),
    ]
    for rf, cf, r, tp, mode, ip, ni, cp, msg in cases:
        rc = L.lh_accel_intersect_device_indexed(None, 8, o.ctypes.data, o.ctypes.data, rf, cf, r, tp, None, None, None, mode, ip, ni, cp, None)
        assert rc == -1 and msg in L.lh_last_error().decode(), (rf, cf, mode, ni, L.lh_last_error())


def test_compact_refusals_need_no_device():
    L = binding.lib()
    rec = binding._rec16_host(8)
    occ = np.zeros(8, np.uint8)
    out = np.zeros(8, np.uint32)
    cnt = np.zeros(1, np.uint32); cnt2 = np.zeros(1, np.uint32); idx2 = np.zeros(8, np.uint32)
    R, O, X, N = rec.ctypes.data, occ.ctypes.data, out.ctypes.data, cnt.ctypes.data
    cases = [
        ((8, binding.REC16, R, None, 9, None, 0, None, X, N, None), "select"),
        ((8, 3, R, None, binding.SELECT_HIT, None, 0, None, X, N, None), "record format"),
        ((8, binding.REC16, None, O, binding.SELECT_MISS, None, 0, None, X, N, None), "prim_or_rec16 is NULL"),
        ((8, binding.REC16, R + 4, None, binding.SELECT_HIT, None, 0, None, X, N, None), "aligned"),
        ((8, binding.REC_F64, R, None, binding.SELECT_OCCLUDED, None, 0, None, X, N, None), "occluded is NULL"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, None, 0, None, None, N, None), "output list"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, None, 0, None, X, None, None), "output list"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, X + 2, 4, None, X, N, None), "4-byte aligned"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, None, (1 << 30) + 1, None, X, N, None), "2^30"),
        ((1 << 33, binding.REC_F64, R, None, binding.SELECT_HIT, None, 0, None, X, N, None), "32 bits"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, X, 8, N, X, cnt2.ctypes.data, None), "overlap"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, X, 4, N, X + 8, cnt2.ctypes.data, None), "overlap"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, idx2.ctypes.data, 8, N, X, N, None), "alias"),
        ((8, binding.REC_F64, R, None, binding.SELECT_HIT, idx2.ctypes.data, 8, N, X, X + 4, None), "inside a list"),
    ]
    for args, msg in cases:
        rc = L.lh_accel_compact_device(*args)
        assert rc == -1 and msg in L.lh_last_error().decode(), (args, L.lh_last_error())
    assert not out.any() and not cnt.any()
