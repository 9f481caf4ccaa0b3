"""fp32 ray batches and 16-byte hit records on the device and host paths (lh_accel_intersect_host_ex / _device_ex).

Every answer of the new formats is an identity with the fp64 entry points, checked bit for bit:
  _ex(fp32 rays, LH_REC16)  == pack16(fp64 entry point(the widened rays))   closest hit
  _ex(fp32 rays, any hit)   == fp64 any hit(the widened rays)
where pack16 is lh_dist_pack_records16 (prim, then (float) t, u, v).  LH_POISON_OUTPUTS=1 (tests/conftest.py): every record
slot starts as 0x77 bytes, so a record no kernel wrote cannot pass."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32_rays(org, dr):
    """the fp32 rays and the fp64 rays they stand for"""
    o32 = np.ascontiguousarray(org, np.float32); d32 = np.ascontiguousarray(dr, np.float32)
    return o32, d32, o32.astype(np.float64), d32.astype(np.float64)


def pack16_np(prim, t, u, v):
    rec = np.empty((prim.shape[0], 4), np.uint32)
    rec[:, 0] = np.asarray(prim).view(np.uint32) if np.asarray(prim).dtype == np.int32 else prim
    for k, a in ((1, t), (2, u), (3, v)):
        rec[:, k] = np.asarray(a, np.float64).astype(np.float32).view(np.uint32)
    return rec


def expected16(acc, o64, d64):
    """pack16 of the fp64 device entry point's records for the fp64 rays o64 / d64 (host arrays), on the device"""
    import torch
    n = o64.shape[0]
    out = acc.intersect_device(torch.from_numpy(o64).cuda(), torch.from_numpy(d64).cuda())
    rec = torch.empty(16 * n, dtype=torch.uint8, device="cuda")
    binding.pack_records16(out[0], out[1], out[2], out[3], rec)
    torch.cuda.synchronize()
    return rec.view(torch.int32).reshape(n, 4).cpu().numpy().view(np.uint32), tuple(x.cpu().numpy() for x in out)


def expected_any(acc, o64, d64):
    import torch
    occ = acc.intersect_device(torch.from_numpy(o64).cuda(), torch.from_numpy(d64).cuda(), mode=la.MODE_ANY)[0]
    torch.cuda.synchronize()
    return occ.cpu().numpy()


def host_ex(acc, org, dr, ray_format, record_format, mode=la.MODE_CLOSEST):
    """lh_accel_intersect_host_ex through ctypes: rec16 -> (n, 4) u32; SoA -> (prim, t, u, v); any hit -> occluded bytes"""
    org = np.ascontiguousarray(org); dr = np.ascontiguousarray(dr)
    n = org.shape[0]
    L = acc.L
    if mode == la.MODE_ANY:
        occ = np.full(n, 0x55, np.uint8)
        rc = L.lh_accel_intersect_host_ex(acc.h, n, org.ctypes.data, dr.ctypes.data, ray_format, record_format, None, None, None, None,
                                          occ.ctypes.data, mode)
        assert rc == 0, L.lh_last_error()
        return occ
    if record_format == binding.REC16:
        rec = binding._rec16_host(n)
        rc = L.lh_accel_intersect_host_ex(acc.h, n, org.ctypes.data, dr.ctypes.data, ray_format, record_format, rec.ctypes.data,
                                          None, None, None, None, mode)
        assert rc == 0, L.lh_last_error()
        return rec
    prim = np.empty(n, np.uint32); t = np.empty(n); u = np.empty(n); v = np.empty(n)
    rc = L.lh_accel_intersect_host_ex(acc.h, n, org.ctypes.data, dr.ctypes.data, ray_format, record_format, prim.ctypes.data,
                                      t.ctypes.data, u.ctypes.data, v.ctypes.data, None, mode)
    assert rc == 0, L.lh_last_error()
    return prim, t, u, v


def dev_rec16(acc, org, dr):
    import torch
    rec = acc.intersect_device(torch.from_numpy(np.ascontiguousarray(org)).cuda(), torch.from_numpy(np.ascontiguousarray(dr)).cuda(),
                               records="rec16")[0]
    torch.cuda.synchronize()
    assert rec.shape == (org.shape[0], 4) and rec.dtype == torch.int32
    return rec.cpu().numpy().view(np.uint32)


def dev_any(acc, org, dr):
    import torch
    occ = acc.intersect_device(torch.from_numpy(np.ascontiguousarray(org)).cuda(), torch.from_numpy(np.ascontiguousarray(dr)).cuda(),
                               mode=la.MODE_ANY)[0]
    torch.cuda.synchronize()
    return occ.cpu().numpy()


def assert_rec_equal(got, exp, what):
    bad = np.nonzero((got != exp).any(1))[0]
    assert bad.size == 0, "%s: %d of %d records differ, first %s: got %r expected %r" % (what, bad.size, got.shape[0], bad[:4],
                                                                                       got[bad[:4]], exp[bad[:4]])


def scene(name):
    if name.startswith("fuzz_"):
        z = load_golden(name)
        return z["P"], z["idx"], z["org"], z["dr"]
    if name.startswith("soup_"):
        g = load_golden(name)
        return po.soup(int(g["ntri"]), int(g["nrays"]), float(g["half_extent"]), int(g["seed"]))
    return po.soup(50000, 100000, 0.005, 41)          # seeded soup


def check_identities(acc, org, dr, what):
    o32, d32, o64, d64 = f32_rays(org, dr)
    exp16, exp = expected16(acc, o64, d64)
    exp16_f64rays, _ = expected16(acc, np.ascontiguousarray(org, np.float64), np.ascontiguousarray(dr, np.float64))
    occ = expected_any(acc, o64, d64)
    assert_rec_equal(dev_rec16(acc, o32, d32), exp16, what + ": device, fp32 rays, rec16")
    assert_rec_equal(dev_rec16(acc, np.ascontiguousarray(org, np.float64), np.ascontiguousarray(dr, np.float64)), exp16_f64rays,
                     what + ": device, fp64 rays, rec16")
    assert np.array_equal(dev_any(acc, o32, d32), occ), what + ": device, fp32 rays, any hit"
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp16, what + ": host, fp32 rays, rec16")
    got = host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC_F64)
    for k in range(4):
        assert np.array_equal(np.asarray(got[k]).view(np.uint64 if k else np.uint32), np.asarray(exp[k]).view(np.uint64 if k else np.uint32)), \
            what + ": host, fp32 rays, fp64 records"
    assert np.array_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC_F64, la.MODE_ANY), occ), what + ": host, fp32 rays, any hit"
    return exp16


@pytest.mark.parametrize("wide8", [0, 1])
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("name", ["seeded", "soup_20k", "soup_3k_fat", "fuzz_r06_f662_99", "fuzz_r06_f661_359"])
def test_fp32_rays_and_rec16_are_the_fp64_path(name, build, wide8):
    P, idx, org, dr = scene(name)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(build=build); acc.wait_exact()
    acc.set_param("wide8", wide8)
    check_identities(acc, org, dr, "%s, %s tree, wide8 %d" % (name, build, wide8))
    acc.close()


def test_rec16_against_the_oracle():
    """one seeded scene against the oracle directly: fp64 on the widened rays, records rounded to fp32"""
    P, idx, org, dr = po.soup(20000, 60000, 0.01, 2027)
    o32, d32, o64, d64 = f32_rays(org, dr)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    exp = pack16_np(*o.intersect(o64, d64, nthreads=8))
    assert (exp[:, 0] != po.MISS).sum() > 1000
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    assert_rec_equal(dev_rec16(acc, o32, d32), exp, "device vs oracle")
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp, "host vs oracle")
    miss = exp[:, 0] == po.MISS
    assert np.all(exp[miss, 1] == np.float32(1e38).view(np.uint32))
    acc.close()


def retraced(acc):
    return int(acc.L.lh_accel_last_retraced(acc.h))


@pytest.mark.parametrize("nrays", [100000, 30000])
def test_rec16_through_the_fixup_paths(nrays):
    """a stack capped at 8 rows (4-wide nodes: wide8 0, where the cap holds) and a small visit budget.  100 000 rays: the rays
    over budget or rows go through the fix-up queue to the cooperative walk; 30 000 rays (below 65 536: no queue): they stay
    flagged in the prim word of their record for k_fixups' sequential walk.  Either writes whole rec16 records; the counted host
    launch (trace_statistics) shows that rays were finished there and counts like the fp64 one"""
    P, idx, org, dr = po.soup(200000, nrays, 0.005, 43)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    acc.set_param("wide8", 0); acc.set_param("stack_cap", 8); acc.set_param("ray_budget", 16)
    o32, d32, o64, d64 = f32_rays(org, dr)
    exp16, _ = expected16(acc, o64, d64)
    assert_rec_equal(dev_rec16(acc, o32, d32), exp16, "capped stack, device")
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp16, "capped stack, host")
    acc.trace_statistics(True)
    acc.statistics(clear=True)
    acc.intersect_host(o64, d64)
    s64 = acc.statistics(clear=True); r64 = retraced(acc)
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp16, "capped stack, counted host")
    s16 = acc.statistics(clear=True); r16 = retraced(acc)
    acc.trace_statistics(False)
    assert r16 > 0 and r64 > 0, (r16, r64)
    assert s16["rays"] == s64["rays"] == org.shape[0] and s16["hits"] == s64["hits"] == int((exp16[:, 0] != po.MISS).sum())
    assert s16["nodes"] > 0 and s16["tris"] > 0
    acc.close()


@pytest.mark.parametrize("n", [1, 17, 64])
def test_rec16_small_batches(n):
    """batches of at most 64 rays take k_trace_small"""
    P, idx, org, dr = po.soup(20000, 5000, 0.01, 44)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    o32, d32, o64, d64 = f32_rays(org[:n], dr[:n])
    exp16, _ = expected16(acc, o64, d64)
    assert_rec_equal(dev_rec16(acc, o32, d32), exp16, "%d rays, device" % n)
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp16, "%d rays, host" % n)
    assert np.array_equal(dev_any(acc, o32, d32), expected_any(acc, o64, d64))
    acc.close()


def test_empty_scene_rec16():
    acc = la.HipAccel(0); acc.commit()
    o32 = np.zeros((100, 3), np.float32); d32 = np.ones((100, 3), np.float32)
    exp = pack16_np(np.full(100, po.MISS, np.uint32), np.full(100, 1e38), np.zeros(100), np.zeros(100))
    assert_rec_equal(dev_rec16(acc, o32, d32), exp, "empty scene, device")
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp, "empty scene, host")
    acc.close()


def test_empty_scene_rec16_fills_every_slot():
    """300 records that held something else (more than one 256-thread block, not a multiple of it): all of them become the miss record"""
    import torch
    n = 300
    acc = la.HipAccel(0); acc.commit()
    o = torch.zeros((n, 3), dtype=torch.float64, device="cuda"); d = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    rec = torch.full((n, 4), 0x3F000007, dtype=torch.int32, device="cuda")
    got = acc.intersect_device(o, d, out=(rec,), records="rec16")
    torch.cuda.synchronize()
    assert got[0] is rec
    exp = pack16_np(np.full(n, po.MISS, np.uint32), np.full(n, 1e38), np.zeros(n), np.zeros(n))
    assert_rec_equal(rec.cpu().numpy().view(np.uint32), exp, "empty scene, pre-filled records")
    acc.close()


def big_batch(n, seed=45):
    P, idx, _, _ = po.soup(20000, 10, 0.01, seed)
    rng = np.random.default_rng(seed)
    org = rng.uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
    dr = rng.normal(size=(n, 3)).astype(np.float32)
    return P, idx, org, dr


def test_host_pipeline_ragged_and_below_pipe_min():
    """5 Mi + 12 345 rays: pipelined, the last chunk ragged; 1 Mi rays: the plain path below LH_PIPE_MIN"""
    P, idx, o32, d32 = big_batch(5 * 2 ** 20 + 12345)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    o64 = o32.astype(np.float64); d64 = d32.astype(np.float64)
    exp16, _ = expected16(acc, o64, d64)
    occ = expected_any(acc, o64, d64)
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp16, "pipelined, fp32 rays, rec16")
    assert np.array_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC_F64, la.MODE_ANY), occ), "pipelined, any hit"
    assert_rec_equal(host_ex(acc, o64, d64, binding.RAYS_F64, binding.REC16), exp16, "pipelined, fp64 rays, rec16")
    m = 2 ** 20
    assert_rec_equal(host_ex(acc, o32[:m], d32[:m], binding.RAYS_F32, binding.REC16), exp16[:m], "plain path, rec16")
    acc.close()


def test_host_pipeline_small_chunk_ring(monkeypatch):
    """LH_PIPE_CHUNK / LH_PIPE_DEPTH are latched per accelerator: a fresh one with a ring of two 64 Ki-ray blocks"""
    P, idx, o32, d32 = big_batch(2 ** 21 + 777, seed=46)
    monkeypatch.setenv("LH_PIPE_CHUNK", str(1 << 16)); monkeypatch.setenv("LH_PIPE_DEPTH", "2")
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    o64 = o32.astype(np.float64); d64 = d32.astype(np.float64)
    exp16, _ = expected16(acc, o64, d64)
    assert_rec_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp16, "small-chunk ring, rec16")
    assert np.array_equal(host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC_F64, la.MODE_ANY), expected_any(acc, o64, d64))
    acc.close()


CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from tests import test_gpu_ray_formats as T
from lucille_amd import binding
import lucille_amd as la
P, idx, o32, d32 = T.big_batch(300001, seed=47)
acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
exp16, _ = T.expected16(acc, o32.astype(np.float64), d32.astype(np.float64))
T.assert_rec_equal(T.host_ex(acc, o32, d32, binding.RAYS_F32, binding.REC16), exp16, "LH_PIPE_MIN=100000")
acc.close()
print("CHILD_OK")
'''


def test_host_pipeline_lowered_pipe_min():
    """LH_PIPE_MIN is latched once per process: a child process pipelines 300 001 rays (fewer than four blocks: cut in four)"""
    env = dict(os.environ, LH_PIPE_MIN="100000", LH_POISON_OUTPUTS="1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_refusals_write_nothing():
    """each refusal of the contract returns -1 with a message and leaves the caller's outputs as they were"""
    import torch
    P, idx, org, dr = po.soup(2000, 1000, 0.01, 48)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    o32, d32, _, _ = f32_rays(org, dr)
    n = o32.shape[0]
    L = acc.L
    rec = binding._rec16_host(n); rec[:] = 0x5A5A5A5A
    t = np.full(n, 0.25)
    occ = np.full(n, 0x33, np.uint8)
    cases = [
        (2, binding.REC_F64, rec.ctypes.data, None, None, la.MODE_CLOSEST, "ray format"),
        (binding.RAYS_F32, 2, rec.ctypes.data, None, None, la.MODE_CLOSEST, "record format"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, None, 3, "mode"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, None, occ.ctypes.data, la.MODE_ANY, "any-hit"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data, t.ctypes.data, None, la.MODE_CLOSEST, "must be NULL"),
        (binding.RAYS_F32, binding.REC16, rec.ctypes.data + 8, None, None, la.MODE_CLOSEST, "aligned"),
    ]
    for rf, cf, r, tp, op, mode, msg in cases:
        rc = L.lh_accel_intersect_host_ex(acc.h, n, o32.ctypes.data, d32.ctypes.data, rf, cf, r, tp, None, None, op, mode)
        assert rc == -1 and msg in L.lh_last_error().decode(), (msg, L.lh_last_error())
    assert np.all(rec == 0x5A5A5A5A) and np.all(t == 0.25) and np.all(occ == 0x33)
    d_o = torch.from_numpy(o32).cuda(); d_d = torch.from_numpy(d32).cuda()
    d_rec = torch.full((n + 1, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_t = torch.full((n,), 0.25, dtype=torch.float64, device="cuda")
    d_occ = torch.full((n,), 0x33, dtype=torch.uint8, device="cuda")
    base = d_rec.data_ptr()
    dcases = [
        (2, binding.REC_F64, base, None, None, la.MODE_CLOSEST, "ray format"),
        (binding.RAYS_F32, 2, base, None, None, la.MODE_CLOSEST, "record format"),
        (binding.RAYS_F32, binding.REC16, base, None, None, 3, "mode"),
        (binding.RAYS_F32, binding.REC16, base, None, d_occ.data_ptr(), la.MODE_ANY, "any-hit"),
        (binding.RAYS_F32, binding.REC16, base, d_t.data_ptr(), None, la.MODE_CLOSEST, "must be NULL"),
        (binding.RAYS_F32, binding.REC16, base + 4, None, None, la.MODE_CLOSEST, "aligned"),
    ]
    s = torch.cuda.current_stream().cuda_stream
    for rf, cf, r, tp, op, mode, msg in dcases:
        rc = L.lh_accel_intersect_device_ex(acc.h, n, d_o.data_ptr(), d_d.data_ptr(), rf, cf, C.c_void_p(r), C.c_void_p(tp) if tp else None,
                                            None, None, C.c_void_p(op) if op else None, mode, C.c_void_p(s))
        assert rc == -1 and msg in L.lh_last_error().decode(), (msg, L.lh_last_error())
    torch.cuda.synchronize()
    assert bool((d_rec == 0x5A5A5A5A).all()) and bool((d_t == 0.25).all()) and bool((d_occ == 0x33).all())
    # n == 0 is no work and no error, whatever the record pointer (an empty tensor's may be NULL)
    for r in (rec.ctypes.data, None):
        assert L.lh_accel_intersect_host_ex(acc.h, 0, o32.ctypes.data, d32.ctypes.data, binding.RAYS_F32, binding.REC16, r,
                                            None, None, None, None, la.MODE_CLOSEST) == 0
        assert L.lh_accel_intersect_device_ex(acc.h, 0, d_o.data_ptr(), d_d.data_ptr(), binding.RAYS_F32, binding.REC16,
                                              C.c_void_p(base) if r else None, None, None, None, None, la.MODE_CLOSEST, C.c_void_p(s)) == 0
    acc.close()


def test_binding_float32_inputs():
    """the binding: float32 tensors / arrays select the fp32 ray format; records="rec16" gives (n, 4) records; fp64 callers see
    what they saw before"""
    import torch
    P, idx, org, dr = po.soup(20000, 30000, 0.01, 49)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    o32, d32, o64, d64 = f32_rays(org, dr)
    exp16, exp = expected16(acc, o64, d64)
    got = acc.intersect_host(o32, d32)                       # float32 arrays: fp32 rays, fp64 records
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float64
    for k in range(4):
        assert np.array_equal(np.asarray(got[k]).view(np.uint64 if k else np.uint32), np.asarray(exp[k]).view(np.uint64 if k else np.uint32))
    out = acc.intersect_device(torch.from_numpy(o32).cuda(), torch.from_numpy(d32).cuda())
    torch.cuda.synchronize()
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.float64
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), exp[0].view(np.uint32)) and np.array_equal(out[1].cpu().numpy(), exp[1])
    rec = acc.intersect_device(torch.from_numpy(o64).cuda(), torch.from_numpy(d64).cuda(), records="rec16")[0]
    torch.cuda.synchronize()
    assert_rec_equal(rec.cpu().numpy().view(np.uint32), exp16, "binding, fp64 tensors, rec16")
    with pytest.raises(ValueError):
        acc.intersect_device(torch.from_numpy(o32).cuda(), torch.from_numpy(d32).cuda(), variant=la.VARIANT_DIRECT)
    acc.close()
