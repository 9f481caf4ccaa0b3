"""Meshes handed over as device arrays (lh_accel_add_mesh_device; lh_flatten.hip: one kernel flattens every mesh into the fp64
triangle records, then the device builders): everything is compared bit for bit with (a) the oracle and (b) an accelerator the
existing path built from the same values in host arrays with commit(on_device=True), after wait_exact()."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding, scenes
from oracle import pyoracle as po
from tests.helpers import assert_hits_equal, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_KEYS = ("ntriangles", "ntriangles_in_tree", "nnodes_traversal")


def dev_idx(I):
    import torch
    return torch.from_numpy(np.ascontiguousarray(I, np.uint32).view(np.int32)).cuda()


def dev_pos(P):
    import torch
    return torch.from_numpy(np.ascontiguousarray(P)).cuda()


def device_mesh_accel(meshes, stream=None):
    """meshes: (positions tensor, indices tensor) pairs, added in order"""
    acc = la.HipAccel(0)
    for P, I in meshes:
        acc.add_mesh_device(P, I, stream=stream)
    info = acc.commit()
    return acc, info


def host_array_accel(meshes):
    """(b): the existing path, from host arrays holding the same fp64 values"""
    acc = la.HipAccel(0)
    for P, I in meshes:
        acc.add_mesh(P, I)
    info = acc.commit(on_device=True)
    acc.wait_exact()
    return acc, info


def oracle_of(meshes):
    o = po.Oracle()
    for P, I in meshes:
        I = np.asarray(I, np.uint32)
        if I.shape[0] >= 3:
            o.add_mesh(P[:, :3], I[:I.shape[0] - I.shape[0] % 3])        # primitive ids do not see empty meshes or trailing indices
    o.build()
    return o


def device_records(acc, org, dr, mode=la.MODE_CLOSEST):
    import torch
    out = acc.intersect_device(torch.from_numpy(org).cuda(), torch.from_numpy(dr).cuda(), mode=mode)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().view(np.uint32) if x.dtype == torch.int32 else x.cpu().numpy() for x in out)


def check_records(acc, ref, exp, org, dr, what):
    """closest-hit records of both batch paths against the oracle (a) and the host-array accelerator (b); any-hit = prim != MISS"""
    got = acc.intersect_host(org, dr)
    assert_hits_equal(got, exp, what + ": host batch against the oracle")
    assert_hits_equal(got, ref.intersect_host(org, dr), what + ": host batch against the host-array build")
    gd = device_records(acc, org, dr)
    assert_hits_equal(gd, exp, what + ": device batch against the oracle")
    assert_hits_equal(gd, device_records(ref, org, dr), what + ": device batch against the host-array build")
    hit = exp[0] != po.MISS
    assert np.array_equal(acc.intersect_host(org, dr, mode=la.MODE_ANY).astype(bool), hit)
    assert np.array_equal(device_records(acc, org, dr, la.MODE_ANY)[0].astype(bool), hit)


@pytest.mark.parametrize("fmt", ["f64", "f32"])
@pytest.mark.parametrize("ntri,he,seed", [(1, 0.2, 1), (3, 0.2, 2), (4, 0.2, 3), (5, 0.2, 4), (37, 0.1, 5), (3000, 0.05, 6), (200000, 0.008, 7)])
def test_parity(ntri, he, seed, fmt):
    P, idx, org, dr = po.soup(ntri, 60000, he, 1000 + seed)
    if fmt == "f32":
        P32 = P.astype(np.float32); P = P32.astype(np.float64)          # the oracle and (b) get the widened values
        acc, info = device_mesh_accel([(dev_pos(P32), dev_idx(idx))])
    else:
        acc, info = device_mesh_accel([(dev_pos(P), dev_idx(idx))])
    ref, rinfo = host_array_accel([(P, idx)])
    exp = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
    check_records(acc, ref, exp, org, dr, "%d triangles, %s" % (ntri, fmt))
    ai, bi = acc.info(), ref.info()
    assert ai["ntriangles"] == ntri and all(ai[k] == bi[k] for k in INFO_KEYS), (ai, bi)
    an, ap = acc.ref_tree(); bn, bp = ref.ref_tree()
    assert an.tobytes() == bn.tobytes() and np.array_equal(ap, bp)
    acc.close(); ref.close()


def test_several_meshes_formats_and_strides():
    import torch
    S = [po.soup(n, 40000, 0.05, 3000 + k) for k, n in enumerate((700, 301, 257, 130))]
    org, dr = S[0][2], S[0][3]
    P0, I0 = S[0][0], S[0][1]
    P1 = np.zeros((S[1][0].shape[0], 4)); P1[:, :3] = S[1][0]; P1[:, 3] = 7.0; I1 = S[1][1]          # ri_vector_t: stride 32
    P2 = np.full((S[2][0].shape[0], 4), 9.0, np.float32); P2[:, :3] = S[2][0].astype(np.float32); I2 = S[2][1]      # f32 at stride 16
    P3 = np.zeros((0, 3)); I3 = np.zeros(0, np.uint32)                                                  # empty
    P4 = S[3][0]; I4 = np.concatenate([S[3][1], np.array([5, 4], np.uint32)])                           # 2 trailing indices
    rng = np.random.default_rng(5)
    I5 = np.ascontiguousarray(I0.reshape(-1, 3)[rng.permutation(I0.shape[0] // 3)[:200]][:, ::-1]).reshape(-1)      # shares P0, other triangles
    d0 = dev_pos(P0)
    dmeshes = [(d0, dev_idx(I0)), (dev_pos(P1), dev_idx(I1)), (dev_pos(P2), dev_idx(I2)), (torch.zeros((0, 3), dtype=torch.float64, device="cuda"), dev_idx(I3)),
               (dev_pos(P4), dev_idx(I4)), (d0, dev_idx(I5))]
    hmeshes = [(P0, I0), (P1, I1), (P2[:, :3].astype(np.float64), I2), (P3, I3), (P4, I4), (P0, I5)]
    assert dmeshes[1][0].stride(0) * 8 == 32 and dmeshes[2][0].stride(0) * 4 == 16
    acc, info = device_mesh_accel(dmeshes)
    ref, _ = host_array_accel(hmeshes)
    ntri = sum(m[1].shape[0] // 3 for m in hmeshes)
    assert info["ntriangles"] == ntri == ref.info()["ntriangles"]
    for p in range(ntri):
        assert acc.prim_lookup(p) == ref.prim_lookup(p), p
    exp = oracle_of(hmeshes).intersect(org, dr, nthreads=8)
    assert (exp[0] != po.MISS).sum() > 100
    check_records(acc, ref, exp, org, dr, "six meshes")
    # a strided VIEW (every other row of a wider tensor) takes its stride from the tensor
    wide = torch.zeros((2 * P0.shape[0], 5), dtype=torch.float64, device="cuda"); wide[::2, :3] = d0
    acc2, _ = device_mesh_accel([(wide[::2, :4], dev_idx(I0))])
    assert_hits_equal(acc2.intersect_host(org, dr), oracle_of([(P0, I0)]).intersect(org, dr, nthreads=8), "strided view")
    acc.close(); ref.close(); acc2.close()


def test_exact_t_ties_and_vertex_rays():
    g = load_golden("ao_c1")
    P, I = scenes.tessellate(g["pos0"], g["idx0"], 3)
    acc, _ = device_mesh_accel([(dev_pos(P), dev_idx(I))])
    o = po.Oracle(); o.add_mesh(P, I); o.build()
    rng = np.random.default_rng(4)
    T = P[I.astype(np.int64)].reshape(-1, 3, 3)
    pick = rng.integers(0, T.shape[0], 20000)
    tgt = T[pick, rng.integers(0, 3, 20000)].copy()                         # exactly a vertex
    tgt[::2] = 0.5 * (T[pick[::2], 0] + T[pick[::2], 1])                    # exactly an edge midpoint
    org = tgt + rng.normal(size=tgt.shape) * 3.0
    dr = tgt - org
    ok = np.abs(dr[:, 1]) > 1e-14
    org, dr = np.ascontiguousarray(org[ok]), np.ascontiguousarray(dr[ok])
    exp = o.intersect(org, dr, nthreads=8)
    assert_hits_equal(acc.intersect_host(org, dr), exp, "device meshes, ties")
    assert_hits_equal(device_records(acc, org, dr), exp, "device meshes, ties, device batch")
    assert o.count_equal_t(org[:4000], dr[:4000], exp[1][:4000]).max() >= 2       # ties really occur
    acc.close()


def degenerate_cases():
    rng = np.random.default_rng(9)
    # zero-area triangles (two equal vertices), exactly collinear ones, duplicates of one triangle, among ordinary ones
    P, idx, org, dr = po.soup(2000, 30000, 0.05, 4100)
    T = P.reshape(-1, 3, 3).copy()
    T[0:200:4, 1] = T[0:200:4, 0]; T[1:200:4, 2] = T[1:200:4, 0]; T[2:200:4, 2] = T[2:200:4, 1]
    T[200:300, 2] = T[200:300, 0] + 2.0 * (T[200:300, 1] - T[200:300, 0])
    T[300:340] = T[1000]
    yield "zero-area, collinear, duplicates", np.ascontiguousarray(T.reshape(-1, 3)), idx, org, dr, False
    n = 3000
    tri = np.zeros((n, 1, 3)) + 0.5 + rng.uniform(-0.3, 0.3, (n, 3, 3)); tri -= tri.mean(axis=1, keepdims=True) - 0.5      # every centroid = (0.5, 0.5, 0.5)
    org = rng.uniform(-1, 2, (20000, 3)); dr = rng.uniform(0, 1, (20000, 3)) - org
    yield "equal centroids", tri.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32), org, dr, False
    m = 60
    x = 2.0 ** -np.arange(m)
    tri = np.stack([np.stack([x, np.zeros(m), np.zeros(m)], 1), np.stack([x * 1.0001, np.full(m, 1e-3), np.zeros(m)], 1),
                    np.stack([x, np.zeros(m), np.full(m, 1e-3)], 1)], 1)
    tri = np.concatenate([tri, tri + np.array([0, 2e-3, 0]), tri + np.array([0, 4e-3, 0]), tri + np.array([0, 6e-3, 0]), tri + np.array([0, 8e-3, 0])])
    P = tri.reshape(-1, 3)
    org = rng.uniform(-0.5, 1.5, (20000, 3)); tgt = P[rng.integers(0, P.shape[0], 20000)] + rng.normal(scale=1e-4, size=(20000, 3))
    yield "exponential line", P, np.arange(P.shape[0], dtype=np.uint32), org, tgt - org, True


def test_degenerate_input_and_the_deep_tree():
    """the last case is an LBVH deeper than the walks' stacks: the one scene whose flattened triangles are copied to the host, where
    both trees are built -- it must commit and answer like the host-array build, which falls back the same way"""
    for what, P, idx, org, dr, deep in degenerate_cases():
        P = np.ascontiguousarray(P); org = np.ascontiguousarray(org); dr = np.ascontiguousarray(dr)
        acc, info = device_mesh_accel([(dev_pos(P), dev_idx(idx))])
        ref, rinfo = host_array_accel([(P, idx)])
        exp = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
        check_records(acc, ref, exp, org, dr, what)
        assert acc.info()["ntriangles_in_tree"] == ref.info()["ntriangles_in_tree"], what
        assert acc.info()["ntriangles"] == idx.shape[0] // 3
        if deep:
            assert info["nnodes"] == rinfo["nnodes"] and info["max_depth"] == rinfo["max_depth"]      # the host builders' tree, both times
        acc.close(); ref.close()


def test_sources_may_be_overwritten_in_stream_order():
    import torch
    P, idx, org, dr = po.soup(50000, 40000, 0.01, 5100)
    exp = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
    s = torch.cuda.Stream()
    dP = dev_pos(P); dI = dev_idx(idx)
    torch.cuda.synchronize()
    acc = la.HipAccel(0)
    with torch.cuda.stream(s):
        acc.add_mesh_device(dP, dI, stream=s)
        dP.fill_(123.0); dI.zero_()                   # same stream, behind the library's copies
    acc.commit()
    assert_hits_equal(acc.intersect_host(org, dr), exp, "sources overwritten after the add")
    torch.cuda.synchronize()
    assert float(dP[0, 0]) == 123.0
    acc.close()


def test_frames_and_the_hit_epilogue():
    import torch
    g = load_golden("ao_c1")
    meshes = [(np.ascontiguousarray(g["pos%d" % k]), np.ascontiguousarray(g["idx%d" % k])) for k in range(int(g["ngeoms"]))]
    acc, _ = device_mesh_accel([(dev_pos(P), dev_idx(I)) for P, I in meshes])
    ref, _ = host_array_accel(meshes)
    c = g["camera"]
    cam = la.Camera.make(64, 64, c[16], c[:16], int(c[19]))
    a, sa = acc.render_ao_tile(cam, 0, 0, 64, 64, 2, 16, seed=11)
    b, sb = ref.render_ao_tile(cam, 0, 0, 64, 64, 2, 16, seed=11)
    torch.cuda.synchronize()
    assert sa == sb and sa["primary_hits"] > 1000 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    cam2 = la.Camera.make(32, 32, c[16], c[:16], int(c[19]))
    a, sa = acc.render_pt_tile2(cam2, 0, 0, 32, 32, 0, 4, 4, seed=12)
    b, sb = ref.render_pt_tile2(cam2, 0, 0, 32, 32, 0, 4, 4, seed=12)
    torch.cuda.synchronize()
    assert sa == sb and sa["rays"] > 4 * 32 * 32 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    d_org, d_dir = acc.primary_rays(cam, 0, 0, 64, 64, 1)
    torch.cuda.synchronize()
    org = d_org.cpu().numpy().reshape(-1, 3); dr = d_dir.cpu().numpy().reshape(-1, 3)
    rec = acc.intersect_host(org, dr)
    assert_hits_equal(rec, ref.intersect_host(org, dr), "camera rays")
    assert (rec[0] != po.MISS).sum() > 100
    sta = acc.state_build(org, dr, *rec); stb = ref.state_build(org, dr, *rec)
    assert sta.tobytes() == stb.tobytes() and np.abs(sta).sum() > 0
    acc.close(); ref.close()


def _raw_add(acc, npos, pos, fmt, stride, nidx, idx):
    L = binding.lib()
    rc = L.lh_accel_add_mesh_device(acc.h, npos, pos, fmt, stride, nidx, idx, None)
    return rc, L.lh_last_error().decode()


def test_refusals_leave_the_accelerator_usable():
    import torch
    P, idx, org, dr = po.soup(500, 20000, 0.08, 6100)
    exp = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
    dP = dev_pos(P); dI = dev_idx(idx); dP32 = dev_pos(P.astype(np.float32))
    n, ni = P.shape[0], idx.shape[0]
    acc = la.HipAccel(0)
    p, i, p32 = dP.data_ptr(), dI.data_ptr(), dP32.data_ptr()
    hostP = np.ascontiguousarray(P); hostI = np.ascontiguousarray(idx)
    cases = [
        ((n, p, 2, 24, ni, i), "unknown position format"),
        ((n, p, binding.POS_F64, 16, ni, i), "bad stride"),
        ((n, p, binding.POS_F64, 28, ni, i), "bad stride"),
        ((n, p32, binding.POS_F32, 8, ni, i), "bad stride"),
        ((n, p32, binding.POS_F32, 14, ni, i), "bad stride"),
        ((n - 1, p + 4, binding.POS_F64, 24, ni, i), "positions not aligned"),
        ((n - 1, p32 + 2, binding.POS_F32, 12, ni, i), "positions not aligned"),
        ((n, p, binding.POS_F64, 24, ni - 3, i + 2), "indices not 4-byte aligned"),
        ((n, None, binding.POS_F64, 24, ni, i), "NULL array"),
        ((n, p, binding.POS_F64, 24, ni, None), "NULL array"),
        ((n, hostP.ctypes.data, binding.POS_F64, 24, ni, i), "not a device pointer"),
        ((n, p, binding.POS_F64, 24, ni, hostI.ctypes.data), "not a device pointer"),
        ((n, p, binding.POS_F64, 24, 3 << 29, i), "2^29 triangles"),          # refused by its count: the array is never looked at
    ]
    for args, msg in cases:
        rc, err = _raw_add(acc, *args)
        assert rc == -1 and msg in err, (args, err)
    # Python refuses what the C call cannot take before calling it
    for bad in (lambda: acc.add_mesh_device(P, idx), lambda: acc.add_mesh_device(dP, dI.to(torch.int64)), lambda: acc.add_mesh_device(dP.to(torch.float16), dI),
                lambda: acc.add_mesh_device(dP.t(), dI), lambda: acc.add_mesh_device(dP[:, :2], dI)):
        with pytest.raises(ValueError):
            bad()
    # nothing changed: the same accelerator takes the mesh, refuses to mix, to take normals / attributes, and to build on the host
    acc.add_mesh_device(dP, dI)
    with pytest.raises(la.LucilleHipError, match="cannot be mixed"):
        acc.add_mesh(P, idx)
    nrm = np.zeros((n, 3))
    assert binding.lib().lh_accel_set_normals(acc.h, 0, nrm.ctypes.data, 24, 0) == -1 and "device meshes" in binding.lib().lh_last_error().decode()
    with pytest.raises(la.LucilleHipError, match="device meshes"):
        acc.set_attribute(0, la.ATTR_COLOR, np.zeros((n, 3)))
    for kw in ({"build": "host"}, {"build_threads": 4}):
        with pytest.raises(la.LucilleHipError, match="device meshes"):
            acc.commit(**kw)
    acc.commit()
    assert_hits_equal(acc.intersect_host(org, dr), exp, "after the refusals")
    with pytest.raises(la.LucilleHipError, match="already committed"):
        acc.add_mesh_device(dP, dI)
    with pytest.raises(la.LucilleHipError, match="device meshes"):
        acc.export()
    fresh = la.HipAccel(0)
    assert binding.lib().lh_accel_commit_replica(C.c_void_p(fresh.h.value), C.c_void_p(acc.h.value)) == -1
    assert "device meshes" in binding.lib().lh_last_error().decode()
    fresh.close()
    d = la.HipDist(0, 1, 0, unique_id=la.HipDist.unique_id(), transport=la.DIST_RCCL)
    with pytest.raises(la.LucilleHipError, match="device meshes"):
        d.broadcast_scene(acc)
    d.close()
    assert_hits_equal(acc.intersect_host(org, dr), exp, "after the refused replica / broadcast")
    acc.close()
    # host meshes first: the device mesh is refused, the accelerator commits as it was
    mixed = la.HipAccel(0); mixed.add_mesh(P, idx)
    with pytest.raises(la.LucilleHipError, match="cannot be mixed"):
        mixed.add_mesh_device(dP, dI)
    mixed.commit()
    assert_hits_equal(mixed.intersect_host(org, dr), exp, "host mesh after a refused device mesh")
    mixed.close()
    # lh_multi_* replicates host meshes only
    m = la.HipMulti(devices=[0])
    m.accel(0).add_mesh_device(dP, dI)
    with pytest.raises(la.LucilleHipError, match="device meshes"):
        m.commit()
    m.close()


def test_empty_scenes_always_miss():
    import torch
    org = np.random.default_rng(1).uniform(-1, 1, (1000, 3)); dr = -org
    acc = la.HipAccel(0)
    acc.add_mesh_device(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    acc.add_mesh_device(torch.zeros((5, 3), dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))      # 2 indices: no triangle
    info = acc.commit()
    assert info["ntriangles"] == 0
    rec = acc.intersect_host(org, dr)
    assert (rec[0] == po.MISS).all() and (rec[1] == 1.0e38).all() and not acc.intersect_host(org, dr, mode=la.MODE_ANY).any()
    acc.close()


@pytest.mark.parametrize("bad_index", [None, 0xFFFFFFFF])
def test_errors_found_on_the_device(bad_index):
    """an index >= npositions is met by the flatten kernel before it addresses anything: the commit fails naming it, nothing faults,
    and the same process goes on to build and query a good accelerator"""
    P, idx, org, dr = po.soup(3000, 20000, 0.05, 7100)
    npos = P.shape[0]
    bad = idx.copy(); bad[4567] = npos if bad_index is None else bad_index
    acc = la.HipAccel(0); acc.add_mesh_device(dev_pos(P), dev_idx(bad))
    with pytest.raises(la.LucilleHipError, match=r"index %d out of range \(npositions %d\)" % (int(bad[4567]), npos)):
        acc.commit()
    with pytest.raises(la.LucilleHipError, match="earlier commit"):          # the existing failed-commit state
        acc.commit()
    acc.close()
    # a NaN in a referenced vertex fails with the existing message; in an unreferenced one it does not, as on the host path
    Pn = np.concatenate([P, np.full((1, 3), np.nan)])
    good, _ = device_mesh_accel([(dev_pos(Pn), dev_idx(idx))])
    exp = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
    assert_hits_equal(good.intersect_host(org, dr), exp, "after a failed commit, NaN in an unreferenced vertex")
    assert_hits_equal(device_records(good, org, dr), exp, "after a failed commit, device batch")
    good.close()
    Pn = P.copy(); Pn[idx[999], 1] = np.nan
    acc = la.HipAccel(0); acc.add_mesh_device(dev_pos(Pn), dev_idx(idx))
    with pytest.raises(la.LucilleHipError, match="NaN, infinite or beyond 1e30"):
        acc.commit()
    acc.close()


def test_device_mesh_commits_do_not_leak_device_memory():
    import torch
    P, idx, org, dr = po.soup(200000, 1000, 0.006, 77)
    dP = dev_pos(P); dI = dev_idx(idx)

    def once():
        acc, _ = device_mesh_accel([(dP, dI)])
        acc.intersect_host(org, dr)
        acc.close()
    once(); once()                                    # allocator pools, code objects
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        once()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    # the margin of test_device_commit_does_not_leak_device_memory: one commit's temporaries and copies are > 30 MB here
    assert free0 - free1 < 16 << 20, "device memory shrank by %.1f MB over twenty device-mesh commits" % ((free0 - free1) / 1e6)


CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, torch
import lucille_amd as la
from oracle import pyoracle as po
P, idx, org, dr = po.soup(200000, 1000, 0.006, 78)
dP = torch.from_numpy(P).cuda(); dI = torch.from_numpy(idx.view(np.int32)).cuda()
torch.cuda.synchronize()
sys.stderr.write("=== device meshes\n"); sys.stderr.flush()
a = la.HipAccel(0); a.add_mesh_device(dP, dI); a.commit()
sys.stderr.write("=== host arrays\n"); sys.stderr.flush()
b = la.HipAccel(0); b.add_mesh(P, idx); b.commit(on_device=True); b.wait_exact()
ra = a.intersect_host(org, dr); rb = b.intersect_host(org, dr)
assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
a.close(); b.close()
sys.stderr.write("=== done\n")
"""


def test_no_host_flatten_and_no_upload():
    """LH_BUILD_TIMING=1 in a fresh child: the device-mesh commit prints neither the host flatten nor the tri64 upload line, the
    host-array device build in the same child prints both"""
    env = dict(os.environ, LH_BUILD_TIMING="1")
    env.pop("LH_BUILD", None); env.pop("LH_REF_BUILD", None)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    head, rest = err.split("=== device meshes\n")[1].split("=== host arrays\n")
    host = rest.split("=== done\n")[0]
    assert "device flatten" in head and "host flatten" not in head and "tri64 upload" not in head, head
    assert "device build:" in head                      # the device builders ran behind it
    assert "host flatten" in host and "tri64 upload" in host and "device flatten" not in host, host
