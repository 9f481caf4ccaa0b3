"""Per-ray maximum distance (lh_accel_intersect_device_tmax / lh_accel_intersect_host_tmax): the C ABI and the binding, without a GPU.
The rule is tests/test_tmax_rule.py and tests/test_tmax_model.py, the GPU side tests/test_gpu_tmax.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_intersect_device_tmax", "lh_accel_intersect_host_tmax")

USE = r'''
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    int (*f)(lh_accel_t *, size_t, const void *, const void *, const void *, int, int, void *, void *, void *, void *, void *, int,
             const void *, size_t, const void *, void *) = lh_accel_intersect_device_tmax;
    int (*g)(lh_accel_t *, size_t, const void *, const void *, const void *, int, int, void *, double *, double *, double *, uint8_t *,
             int) = lh_accel_intersect_host_tmax;
    printf("%d\n", f != NULL && g != NULL);
    return 0;
}
'''


def test_library_exports_the_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_prototypes_have_17_and_13_arguments():
    L = binding.lib()
    assert len(L.lh_accel_intersect_device_tmax.argtypes) == 17
    assert len(L.lh_accel_intersect_host_tmax.argtypes) == 13
    for name in ("intersect_device", "intersect_device_indexed", "intersect_host"):
        p = inspect.signature(getattr(la.HipAccel, name)).parameters
        assert p["tmax"].default is None, name
        assert "tmax" in getattr(la.HipAccel, name).__doc__
    assert list(inspect.signature(la.HipAccel.intersect_host_tmax).parameters)[:4] == ["self", "org", "dr", "tmax"]


@pytest.mark.parametrize("cc,std,ext", [("cc", "-std=c11", "c"), ("c++", "-std=c++17", "cpp")])
def test_header_compiles_as_c11_and_cxx17(tmp_path, cc, std, ext):
    """a program that takes the address of both functions with their declared types, compiled against include/lucille_hip.h"""
    src = tmp_path / ("tmax." + ext)
    src.write_text(USE)
    exe = tmp_path / ("tmax_" + ext)
    lib_dir = os.path.join(ROOT, "lucille_amd", "csrc")
    la.build_library()
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-llucille_hip", "-Wl,-rpath," + lib_dir])
    assert subprocess.check_output([str(exe)]).decode().split() == ["1"]


def test_device_refusals_need_no_device():
    """the argument checks come before the accelerator is looked at: every refusal of lh_accel_intersect_device_ex / _indexed, a
    misaligned bound array, more than 2^30 rays"""
    L = binding.lib()
    rec = binding._rec16_host(8); rec[:] = 0
    o = np.zeros((8, 3), np.float32)
    t = np.zeros(8)
    tm = np.zeros(16, np.float32)
    idx = np.zeros(8, np.uint32)
    F32, F64, R16, R64 = binding.RAYS_F32, binding.RAYS_F64, binding.REC16, binding.REC_F64
    TM, R, I = tm.ctypes.data, rec.ctypes.data, idx.ctypes.data
    # (n_rays, tmax, ray format, record format, records, t, mode, index, n_index, count, message)
    cases = [
        (8, TM, 2, R64, R, None, la.MODE_CLOSEST, I, 8, None, "ray format"),
        (8, TM, F32, 5, R, None, la.MODE_CLOSEST, I, 8, None, "record format"),
        (8, TM, F32, R16, R, None, 7, I, 8, None, "mode"),
        (8, TM, F32, R16, R, None, la.MODE_ANY, I, 8, None, "any-hit"),
        (8, TM, F32, R16, R, t.ctypes.data, la.MODE_CLOSEST, I, 8, None, "must be NULL"),
        (8, TM, F32, R16, R + 4, None, la.MODE_CLOSEST, I, 8, None, "aligned"),
        (8, TM, F32, R16, R, None, la.MODE_CLOSEST, None, (1 << 30) + 1, None, "2^30"),
        (8, TM, F32, R16, R, None, la.MODE_CLOSEST, I + 2, 4, None, "4-byte aligned"),
        (8, TM, F32, R16, R, None, la.MODE_CLOSEST, I, 8, I + 1, "4-byte aligned"),
        (8, TM + 2, F32, R16, R, None, la.MODE_CLOSEST, None, 0, None, "tmax not aligned"),
        (8, TM + 4, F64, R64, R, None, la.MODE_CLOSEST, None, 0, None, "tmax not aligned"),        # doubles: 8-byte elements
        (8, TM + 2, F32, R16, R, None, la.MODE_CLOSEST, I, 8, None, "tmax not aligned"),
        ((1 << 30) + 1, TM, F32, R16, R, None, la.MODE_CLOSEST, None, 0, None, "2^30 rays"),
        ((1 << 30) + 1, TM, F32, R16, R, None, la.MODE_CLOSEST, I, 8, None, "2^30 rays"),
        (8, TM, F32, R16, R, None, la.MODE_CLOSEST, None, 0, None, "not committed"),
        (8, TM, F32, R16, R, None, la.MODE_CLOSEST, I, 8, None, "not committed"),
    ]
    for n, tp, rf, cf, r, tt, mode, ip, ni, cp, msg in cases:
        rc = L.lh_accel_intersect_device_tmax(None, n, o.ctypes.data, o.ctypes.data, tp, rf, cf, r, tt, None, None, None, mode, ip, ni, cp, None)
        assert rc == -1 and msg in L.lh_last_error().decode(), (n, rf, cf, mode, ni, msg, L.lh_last_error())
    assert not rec.any()


def test_a_null_bound_is_the_unbounded_entry_point():
    """d_tmax == NULL forwards: the refusal carries the name of the entry point it went to"""
    L = binding.lib()
    rec = binding._rec16_host(8); o = np.zeros((8, 3), np.float32); idx = np.zeros(8, np.uint32)
    rc = L.lh_accel_intersect_device_tmax(None, 8, o.ctypes.data, o.ctypes.data, None, 2, binding.REC16, rec.ctypes.data, None, None, None,
                                          None, la.MODE_CLOSEST, None, 0, None, None)
    assert rc == -1 and "lh_accel_intersect_device_ex" in L.lh_last_error().decode()
    rc = L.lh_accel_intersect_device_tmax(None, 8, o.ctypes.data, o.ctypes.data, None, 2, binding.REC16, rec.ctypes.data, None, None, None,
                                          None, la.MODE_CLOSEST, idx.ctypes.data, 8, None, None)
    assert rc == -1 and "lh_accel_intersect_device_indexed" in L.lh_last_error().decode()
    rc = L.lh_accel_intersect_host_tmax(None, 8, o.ctypes.data, o.ctypes.data, None, 2, binding.REC16, rec.ctypes.data, None, None, None, None,
                                        la.MODE_CLOSEST)
    assert rc == -1 and "lh_accel_intersect_host_ex" in L.lh_last_error().decode()


def test_host_refusals_need_no_device():
    L = binding.lib()
    rec = binding._rec16_host(8); rec[:] = 0
    o = np.zeros((8, 3)); t = np.zeros(8); tm = np.zeros(16)
    F64, R16, R64 = binding.RAYS_F64, binding.REC16, binding.REC_F64
    cases = [
        (tm.ctypes.data, 3, R64, rec.ctypes.data, None, la.MODE_CLOSEST, "ray format"),
        (tm.ctypes.data, F64, 4, rec.ctypes.data, None, la.MODE_CLOSEST, "record format"),
        (tm.ctypes.data, F64, R16, rec.ctypes.data, None, la.MODE_ANY, "any-hit"),
        (tm.ctypes.data, F64, R16, rec.ctypes.data, t.ctypes.data, la.MODE_CLOSEST, "must be NULL"),
        (tm.ctypes.data, F64, R16, rec.ctypes.data + 8, None, la.MODE_CLOSEST, "aligned"),
        (tm.ctypes.data + 4, F64, R16, rec.ctypes.data, None, la.MODE_CLOSEST, "tmax not aligned"),
        (tm.ctypes.data, F64, R16, rec.ctypes.data, None, la.MODE_CLOSEST, "not committed"),
    ]
    for tp, rf, cf, r, tt, mode, msg in cases:
        rc = L.lh_accel_intersect_host_tmax(None, 8, o.ctypes.data, o.ctypes.data, tp, rf, cf, r, tt, None, None, None, mode)
        assert rc == -1 and msg in L.lh_last_error().decode(), (rf, cf, mode, msg, L.lh_last_error())
    assert not rec.any()


class _FakeTensor:
    """enough of a device tensor for the binding's argument checks, which come before anything touches a device"""
    is_cuda = True

    def __init__(self, dtype, shape, device="cuda:0", contiguous=True):
        self.dtype, self.shape, self.device, self._c = dtype, shape, device, contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c


def test_binding_argument_checks():
    torch = pytest.importorskip("torch")
    acc = la.HipAccel.__new__(la.HipAccel)           # no device: the checks below raise before the handle is used
    org = _FakeTensor(torch.float64, (8, 3))
    good = _FakeTensor(torch.float64, (8,))
    with pytest.raises(ValueError, match="default variant"):
        la.HipAccel.intersect_device(acc, org, org, tmax=good, variant=la.VARIANT_DIRECT)
    with pytest.raises(ValueError, match="default variant"):
        la.HipAccel.intersect_device(acc, org, org, tmax=good, counters=True)
    for bad in (_FakeTensor(torch.float32, (8,)), _FakeTensor(torch.float64, (7,)), _FakeTensor(torch.float64, (8, 1)),
                _FakeTensor(torch.float64, (8,), contiguous=False), _FakeTensor(torch.float64, (8,), device="cuda:1"), np.zeros(8)):
        with pytest.raises(ValueError, match="tmax must be"):
            binding._tmax_device(bad, org, "intersect_device")
    assert binding._tmax_device(good, org, "intersect_device") is good
