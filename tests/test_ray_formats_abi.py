"""fp32 ray batches and 16-byte hit records (lh_accel_intersect_host_ex / _device_ex): the C ABI and the binding, without a GPU.
The GPU side is tests/test_gpu_ray_formats.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lh_accel_intersect_host_ex", "lh_accel_intersect_device_ex")


def test_library_exports_the_format_entry_points():
    L = C.CDLL(la.build_library())
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert all(n in binding.ABI_SYMBOLS for n in NEW)


def test_header_record_layout_and_constants(tmp_path):
    """a C program compiled against include/lucille_hip.h: lh_rec16_t is 16 bytes {prim, t, u, v}, the format constants as the
    binding has them"""
    src = tmp_path / "rec16.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "lucille_hip.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %d %d %d %d\n", sizeof(lh_rec16_t), offsetof(lh_rec16_t, prim), offsetof(lh_rec16_t, t),
           offsetof(lh_rec16_t, u), offsetof(lh_rec16_t, v), LH_RAYS_F64, LH_RAYS_F32, LH_REC_F64, LH_REC16);
    return 0;
}
''')
    exe = tmp_path / "rec16"
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in got] == [16, 0, 4, 8, 12, binding.RAYS_F64, binding.RAYS_F32, binding.REC_F64, binding.REC16]
    assert (binding.RAYS_F64, binding.RAYS_F32, binding.REC_F64, binding.REC16) == (0, 1, 0, 1)


def test_header_compiles_as_cxx(tmp_path):
    src = tmp_path / "rec16.cpp"
    src.write_text('#include "lucille_hip.h"\nstatic_assert(sizeof(lh_rec16_t) == 16, "");\nint main() { return 0; }\n')
    subprocess.check_call(["c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_binding_prototypes():
    L = binding.lib()
    assert len(L.lh_accel_intersect_host_ex.argtypes) == 12
    assert len(L.lh_accel_intersect_device_ex.argtypes) == 13


@pytest.mark.parametrize("n", [0, 1, 3, 1000])
def test_host_record_array_is_16_byte_aligned(n):
    for _ in range(8):
        r = binding._rec16_host(n)
        assert r.shape == (n, 4) and r.dtype == np.uint32 and r.flags.c_contiguous
        assert r.ctypes.data % 16 == 0


def test_records_keyword_is_checked():
    assert binding._records_format("f64") == binding.REC_F64
    assert binding._records_format("rec16") == binding.REC16
    with pytest.raises(ValueError):
        binding._records_format("f32")


def test_dtype_selects_the_ray_format():
    assert binding._is_f32(np.zeros((2, 3), np.float32))
    assert not binding._is_f32(np.zeros((2, 3), np.float64))
    assert not binding._is_f32([[0.0, 0.0, 0.0]])
    torch = pytest.importorskip("torch")
    assert binding._is_f32(torch.zeros((2, 3), dtype=torch.float32))
    assert not binding._is_f32(torch.zeros((2, 3), dtype=torch.float64))


def test_refusals_need_no_device():
    """the format checks come first: an unknown format / mode, LH_REC16 in any-hit mode, t/u/v beside LH_REC16 and a misaligned
    record pointer are refused with a message before the accelerator is looked at"""
    L = binding.lib()
    rec = binding._rec16_host(8)
    o = np.zeros((8, 3), np.float32)
    t = np.zeros(8)
    cases = [
        (2, binding.REC_F64, rec.ctypes.data, None, la.MODE_CLOSEST, "ray format"),
        (binding.RAYS_F32, 5, rec.ctypes.data, None, la.MODE_CLOSEST, "record format"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, 7, "mode"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, la.MODE_ANY, "any-hit"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, t.ctypes.data, la.MODE_CLOSEST, "must be NULL"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data + 4, None, la.MODE_CLOSEST, "aligned"),
    ]
    for rf, cf, r, tp, mode, msg in cases:
        rc = L.lh_accel_intersect_host_ex(None, 8, o.ctypes.data, o.ctypes.data, rf, cf, r, tp, None, None, None, mode)
        assert rc == -1 and msg in L.lh_last_error().decode(), (rf, cf, mode, L.lh_last_error())
        rc = L.lh_accel_intersect_device_ex(None, 8, o.ctypes.data, o.ctypes.data, rf, cf, r, tp, None, None, None, mode, None)
        assert rc == -1 and msg in L.lh_last_error().decode(), (rf, cf, mode, L.lh_last_error())
