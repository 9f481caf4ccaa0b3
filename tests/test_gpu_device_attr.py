"""Per-vertex normals and attributes of device meshes (lh_accel_set_normals_device / lh_accel_set_attribute_device; lh_flatten.hip:
k_gather_attributes fills the per-primitive arrays behind the flatten).  Everything is compared bit for bit with the compiled
reference's records (tests/golden/state_attr.npz), the oracle, and an accelerator the host-array path built from the same values
with commit(on_device=True), after wait_exact()."""
import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
from tests.golden.make_golden import apply_state_scene, state_scene
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

KINDS = ((la.ATTR_COLOR, "C"), (la.ATTR_TANGENT, "T"), (la.ATTR_BINORMAL, "B"), (la.ATTR_TEXCOORD, "ST"), (la.ATTR_TEXCOORD_UNSHARED, "STU"))


def dev_idx(I):
    import torch
    return torch.from_numpy(np.ascontiguousarray(I, np.uint32).view(np.int32)).cuda()


def dev_pos(P):
    import torch
    P = np.ascontiguousarray(P)
    if P.size == 0:                                   # an empty mesh: a fresh tensor has the strides of its shape
        return torch.zeros(P.shape, dtype=torch.float64 if P.dtype == np.float64 else torch.float32, device="cuda")
    return torch.from_numpy(P).cuda()


def dev_strided(A):
    """rows one element wider than the data (3 -> 4: ri_vector_t; st 2 -> 3), the data a view of them"""
    import torch
    wide = torch.full((A.shape[0], A.shape[1] + 1), 7.0, dtype=torch.float64, device="cuda")
    wide[:, :A.shape[1]] = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    return wide[:, :A.shape[1]]


def dev_f32(A):
    return dev_pos(np.asarray(A).astype(np.float32))


class DeviceScene:
    """adapter: a scene description (apply_state_scene's calls) onto a HipAccel of device meshes"""

    def __init__(self, attr=dev_pos, stream=None):
        self.acc = la.HipAccel(0)
        self.attr, self.stream = attr, stream

    def add_mesh(self, P, idx):
        self.acc.add_mesh_device(dev_pos(P), dev_idx(idx), stream=self.stream)

    def set_normals(self, k, N, two_side):
        self.acc.set_normals_device(k, self.attr(N) if N is not None else None, two_side, stream=self.stream)

    def set_attribute(self, k, kind, data):
        self.acc.set_attribute_device(k, kind, self.attr(data), stream=self.stream)


class HostScene:
    """the same calls onto the host-array path"""

    def __init__(self):
        self.acc = la.HipAccel(0)

    def add_mesh(self, P, idx):
        self.acc.add_mesh(P, idx)

    def set_normals(self, k, N, two_side):
        self.acc.set_normals(k, N, two_side)

    def set_attribute(self, k, kind, data):
        self.acc.set_attribute(k, kind, data)


def device_accel(meshes, attr=dev_pos, stream=None):
    s = DeviceScene(attr, stream); apply_state_scene(s, meshes, False)
    return s.acc, s.acc.commit()


def host_accel(meshes):
    s = HostScene(); apply_state_scene(s, meshes, False)
    info = s.acc.commit(on_device=True); s.acc.wait_exact()
    return s.acc, info


def oracle_of(meshes):
    """the oracle numbers only the meshes that have triangles"""
    o = po.Oracle(); k = 0
    for m in meshes:
        if m["idx"].shape[0] < 3:
            continue
        o.add_mesh(m["P"], m["idx"])
        if "N" in m or m["two_side"]:
            o.set_normals(k, m.get("N"), m["two_side"])
        for kind, key in KINDS:
            if key in m:
                o.set_attribute(k, kind, m[key])
        k += 1
    o.build()
    return o


def records(acc, org, dr):
    """(prim, state records) of the host batch path"""
    prim, t, u, v = acc.intersect_host(org, dr)
    return prim, acc.state_build(org, dr, prim, t, u, v)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


# ---- 1. the reference's own records ------------------------------------------------------------------------------------
def test_state_records_equal_the_reference():
    g = load_golden("state_attr")
    meshes, org, dr = state_scene(int(g["seed"]))
    acc, _ = device_accel(meshes)
    prim, st = records(acc, org, dr)
    assert np.array_equal(prim, g["prim"]) and (prim != po.MISS).sum() > 1000
    assert np.array_equal(st, g["state"])
    acc.close()
    meshes, org, dr = state_scene(5)
    acc, _ = device_accel(meshes)
    o = po.Oracle(); apply_state_scene(o, meshes, False); o.build()
    op, ost = o.state_batch(org, dr)
    prim, st = records(acc, org, dr)
    assert np.array_equal(prim, op) and np.array_equal(st, ost)
    acc.close()


# ---- 2. formats and strides ---------------------------------------------------------------------------------------------
def test_formats_and_strides():
    meshes, org, dr = state_scene(2024)
    packed, _ = device_accel(meshes, dev_pos)
    strided, _ = device_accel(meshes, dev_strided)
    assert dev_strided(meshes[0]["N"]).stride(0) == 4 and dev_strided(meshes[0]["ST"]).stride(0) == 3
    pp, ps = records(packed, org, dr)
    sp, ss = records(strided, org, dr)
    assert same(pp, sp) and same(ps, ss) and np.array_equal(ps, load_golden("state_attr")["state"])
    packed.close(); strided.close()
    # fp32: the value IS its widening -- the host-array accelerator holds the widened values
    wide = [dict(m, **{k: m[k].astype(np.float32).astype(np.float64) for k in ("N", "C", "T", "B", "ST", "STU") if k in m}) for m in meshes]
    assert not np.array_equal(wide[0]["N"], meshes[0]["N"])
    f32, _ = device_accel(meshes, dev_f32)
    ref, _ = host_accel(wide)
    fp, fs = records(f32, org, dr)
    rp, rs = records(ref, org, dr)
    assert same(fp, rp) and same(fs, rs) and not same(fs, ps)
    f32.close(); ref.close()


# ---- 3. mesh boundaries inside a workgroup ------------------------------------------------------------------------------
def boundary_scene():
    """six meshes of 1, 3, 0, 85, 86 and 200 triangles: the first workgroup's 256 corners end inside primitive 85 (mesh 3), so mesh
    boundaries fall inside workgroups and between them; presence of every attribute alternates"""
    rng = np.random.default_rng(31)
    meshes = []
    for k, ntri in enumerate((1, 3, 0, 85, 86, 200)):
        own = ntri // 2 if k == 5 else ntri                       # the two_side mesh: its second half = the first, reversed
        c = rng.uniform(-0.5, 0.5, (own, 1, 3)) + np.array([0.3 * k - 0.7, 0.0, 0.0])
        tri = c + rng.uniform(-0.15, 0.15, (own, 3, 3))
        npos = 3 * own if own <= 3 else 3 * own // 2              # the larger meshes share vertices: indices point into a smaller pool
        P = tri.reshape(-1, 3)[:npos].copy()
        idx = (np.arange(3 * own) if own <= 3 else np.concatenate([rng.permutation(npos)[:3] for _ in range(own)])).astype(np.uint32)
        m = {"P": P, "idx": idx, "two_side": 0}
        if k == 5:
            m["idx"] = np.concatenate([idx, idx[::-1]]).astype(np.uint32); m["two_side"] = 1
            assert m["idx"].shape[0] == 600 and m["idx"].shape[0] % 6 == 0
        if k in (0, 3, 5):
            m["N"] = unit(rng.normal(size=(npos, 3)))
        if k == 4:
            m["C"] = rng.uniform(0, 1, (npos, 3)); m["B"] = unit(rng.normal(size=(npos, 3)))
        if k == 0:
            m["T"] = unit(rng.normal(size=(npos, 3)))
        if k == 1:                                                # both: the shared ones win
            m["ST"] = rng.uniform(0, 4, (npos, 2)); m["STU"] = rng.uniform(-1, 1, (m["idx"].shape[0], 2))
        if k == 3:
            m["STU"] = rng.uniform(-1, 1, (m["idx"].shape[0], 2))
        assert m["idx"].shape[0] % 3 == 0
        meshes.append(m)
    T = np.concatenate([m["P"][m["idx"].astype(np.int64)].reshape(-1, 3, 3) for m in meshes if m["idx"].shape[0]])
    assert T.shape[0] == 375
    n = 4000
    pick = np.concatenate([np.arange(375), rng.integers(0, 375, n - 375)])          # every triangle is aimed at
    w = rng.dirichlet((2.0, 2.0, 2.0), n)
    tgt = (T[pick] * w[:, :, None]).sum(axis=1)
    org = tgt + unit(rng.normal(size=(n, 3))) * rng.uniform(1.0, 3.0, (n, 1))
    return meshes, np.ascontiguousarray(org), np.ascontiguousarray(tgt - org)


def test_mesh_boundaries_inside_a_workgroup():
    meshes, org, dr = boundary_scene()
    acc, info = device_accel(meshes)
    ref, rinfo = host_accel(meshes)
    assert info["ntriangles"] == 375 == rinfo["ntriangles"]
    ap, ast = records(acc, org, dr)
    rp, rst = records(ref, org, dr)
    op, ost = oracle_of(meshes).state_batch(org, dr)
    hits = int((ap != po.MISS).sum())
    first = np.cumsum([0] + [m["idx"].shape[0] // 3 for m in meshes])
    seen = {int(np.searchsorted(first, q, side="right")) - 1 for q in np.unique(ap[ap != po.MISS])}
    print("hits", hits, "of", org.shape[0], "meshes hit", sorted(seen))
    assert hits > org.shape[0] - org.shape[0] // 20               # fewer than one ray in twenty may miss
    assert same(ap, rp) and same(ast, rst)
    assert np.array_equal(ap, op) and np.array_equal(ast, ost)
    assert seen == {0, 1, 3, 4, 5}                                # both sides of every boundary are looked at
    acc.close(); ref.close()


# ---- 4. frames use the attributes ---------------------------------------------------------------------------------------
def test_frames_use_the_attributes():
    import torch
    g = load_golden("ao_c1")
    rng = np.random.default_rng(41)
    meshes = []
    for k in range(int(g["ngeoms"])):
        P = np.ascontiguousarray(g["pos%d" % k]); I = np.ascontiguousarray(g["idx%d" % k])
        N = np.ascontiguousarray(g["nrm%d" % k]) if ("nrm%d" % k) in g.files else unit(rng.normal(size=P.shape))
        m = {"P": P, "idx": I, "two_side": int(g["two_side%d" % k]), "N": N}
        if k == 1:
            m["C"] = rng.uniform(0, 1, P.shape)
        meshes.append(m)
    acc, _ = device_accel(meshes)
    ref, _ = host_accel(meshes)
    flat, _ = device_accel([{"P": m["P"], "idx": m["idx"], "two_side": m["two_side"]} for m in meshes])
    c = g["camera"]
    cam = la.Camera.make(64, 64, c[16], c[:16], int(c[19]))
    a, sa = acc.render_ao_tile(cam, 0, 0, 64, 64, 2, 16, seed=11)
    b, sb = ref.render_ao_tile(cam, 0, 0, 64, 64, 2, 16, seed=11)
    f, sf = flat.render_ao_tile(cam, 0, 0, 64, 64, 2, 16, seed=11)
    torch.cuda.synchronize()
    a, b, f = a.cpu().numpy(), b.cpu().numpy(), f.cpu().numpy()
    assert sa == sb and sa["primary_hits"] > 1000 and a.tobytes() == b.tobytes()
    assert sf["primary_hits"] == sa["primary_hits"] and a.tobytes() != f.tobytes()       # the normals are read
    cam2 = la.Camera.make(32, 32, c[16], c[:16], int(c[19]))
    a, sa = acc.render_pt_tile2(cam2, 0, 0, 32, 32, 0, 4, 4, seed=12)
    b, sb = ref.render_pt_tile2(cam2, 0, 0, 32, 32, 0, 4, 4, seed=12)
    torch.cuda.synchronize()
    assert sa == sb and sa["rays"] > 4 * 32 * 32 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # the AO stage for a caller's batch: the 64 x 64 primary rays and their records
    out = []
    for x in (acc, ref):
        d_org, d_dir = x.primary_rays(cam, 0, 0, 64, 64, 1)
        rec = x.intersect_device(d_org, d_dir)
        cnt, rad = x.ao_device(d_org, d_dir, rec, 16, seed=13)
        torch.cuda.synchronize()
        out.append((rec[0].cpu().numpy(), cnt.cpu().numpy(), rad.cpu().numpy()))
    for x, y in zip(*out):
        assert same(x, y)
    assert (out[0][0].view(np.uint32) != po.MISS).sum() > 500
    acc.close(); ref.close(); flat.close()


# ---- 5. the deep tree ---------------------------------------------------------------------------------------------------
def test_the_deep_tree_keeps_its_attributes():
    """the "exponential line" of tests/test_gpu_device_mesh.py: an LBVH deeper than the walks' stacks, built on the host after all"""
    rng = np.random.default_rng(9)
    m = 60
    x = 2.0 ** -np.arange(m)
    tri = np.stack([np.stack([x, np.zeros(m), np.zeros(m)], 1), np.stack([x * 1.0001, np.full(m, 1e-3), np.zeros(m)], 1),
                    np.stack([x, np.zeros(m), np.full(m, 1e-3)], 1)], 1)
    tri = np.concatenate([tri, tri + np.array([0, 2e-3, 0]), tri + np.array([0, 4e-3, 0]), tri + np.array([0, 6e-3, 0]), tri + np.array([0, 8e-3, 0])])
    P = np.ascontiguousarray(tri.reshape(-1, 3))
    assert P.shape[0] == 900
    org = rng.uniform(-0.5, 1.5, (20000, 3)); tgt = P[rng.integers(0, P.shape[0], 20000)] + rng.normal(scale=1e-4, size=(20000, 3))
    dr = np.ascontiguousarray(tgt - org)
    meshes = [{"P": P, "idx": np.arange(900, dtype=np.uint32), "two_side": 0, "N": unit(rng.normal(size=P.shape)), "C": rng.uniform(0, 1, P.shape)}]
    acc, info = device_accel(meshes)
    ref, rinfo = host_accel(meshes)
    assert info["nnodes"] == rinfo["nnodes"] and info["max_depth"] == rinfo["max_depth"]      # the host builders' tree, both times
    ap, ast = records(acc, org, dr)
    rp, rst = records(ref, org, dr)
    assert same(ap, rp) and same(ast, rst) and (ap != po.MISS).sum() > 100
    hit = ap != po.MISS
    assert not same(ast[hit][:, 6:9], ast[hit][:, 3:6]) and np.abs(ast[hit][:, 15:18]).sum() > 0      # Ns is not Ng, the colour is there
    acc.close(); ref.close()


# ---- 6. stream order ----------------------------------------------------------------------------------------------------
def test_sources_may_be_overwritten_in_stream_order():
    import torch
    P, idx, org, dr = po.soup(20000, 20000, 0.02, 5200)
    N = unit(np.random.default_rng(6).normal(size=P.shape))
    ref, _ = host_accel([{"P": P, "idx": idx, "two_side": 0, "N": N}])
    s = torch.cuda.Stream()
    dP, dI, dN = dev_pos(P), dev_idx(idx), dev_pos(N)
    torch.cuda.synchronize()
    acc = la.HipAccel(0)
    with torch.cuda.stream(s):
        acc.add_mesh_device(dP, dI, stream=s)
        acc.set_normals_device(0, dN, stream=s)
        dN.fill_(123.0)                               # same stream, behind the library's copy
    acc.commit()
    ap, ast = records(acc, org, dr)
    rp, rst = records(ref, org, dr)
    assert same(ap, rp) and same(ast, rst) and (ap != po.MISS).sum() > 100
    torch.cuda.synchronize()
    assert float(dN[0, 0]) == 123.0 and float(dN[-1, 2]) == 123.0
    acc.close(); ref.close()


# ---- 7. refusals leave the accelerator usable ---------------------------------------------------------------------------
def test_refusals_leave_the_accelerator_usable():
    import torch
    g = load_golden("state_attr")
    meshes, org, dr = state_scene(int(g["seed"]))
    L = binding.lib()
    F64, F32 = binding.POS_F64, binding.POS_F32
    s = DeviceScene()
    for m in meshes:
        s.add_mesh(m["P"], m["idx"])
    acc = s.acc
    n, ni = meshes[0]["P"].shape[0], meshes[0]["idx"].shape[0]
    dN = dev_pos(meshes[0]["N"]); dN32 = dev_f32(meshes[0]["N"]); dST = dev_pos(meshes[0]["ST"])
    dSTU = dev_pos(np.zeros((ni, 2)))
    p, p32, st, stu = dN.data_ptr(), dN32.data_ptr(), dST.data_ptr(), dSTU.data_ptr()
    hostN = np.ascontiguousarray(meshes[0]["N"])                  # host memory: asked about, never read
    C_, ST_, STU_ = la.ATTR_COLOR, la.ATTR_TEXCOORD, la.ATTR_TEXCOORD_UNSHARED

    def normals(h, mesh, count, ptr, fmt, stride):
        return L.lh_accel_set_normals_device(h, mesh, count, ptr, fmt, stride, 0, None), L.lh_last_error().decode()

    def attribute(h, mesh, kind, count, ptr, fmt, stride):
        return L.lh_accel_set_attribute_device(h, mesh, kind, count, ptr, fmt, stride, None), L.lh_last_error().decode()

    ncases = [((3, n, p, F64, 24), "mesh 3 out of range"), ((0, n, p, 2, 24), "unknown format"), ((0, n, p, F64, 16), "bad stride"),
              ((0, n, p, F64, 28), "bad stride"), ((0, n, p32, F32, 8), "bad stride"), ((0, n, p32, F32, 14), "bad stride"),
              ((0, n - 1, p + 4, F64, 24), "not aligned"), ((0, n - 1, p32 + 2, F32, 12), "not aligned"), ((0, n, None, F64, 24), "NULL array"),
              ((0, n, hostN.ctypes.data, F64, 24), "not a device pointer"), ((0, n - 1, p, F64, 1 << 30), "extends past its allocation"),      # (a wrong count too: refused either way)
              ((0, n - 1, p, F64, 24), "%d values given, the mesh needs %d" % (n - 1, n)), ((0, 0, p, F64, 24), "0 values given, the mesh needs %d" % n)]
    for args, msg in ncases:
        rc, err = normals(acc.h, *args)
        assert rc == -1 and msg in err and "lh_accel_set_normals_device" in err, (args, err)
    acases = [((3, C_, n, p, F64, 24), "mesh 3 out of range"), ((0, -1, n, p, F64, 24), "unknown attribute kind"), ((0, 5, n, p, F64, 24), "unknown attribute kind"),
              ((0, C_, n, p, 7, 24), "unknown format"), ((0, C_, n, p, F64, 20), "bad stride"), ((0, ST_, n, st, F64, 8), "bad stride"),
              ((0, ST_, n, p32, F32, 4), "bad stride"), ((0, C_, n - 1, p + 4, F64, 24), "not aligned"), ((0, C_, n, None, F64, 24), "NULL array"),
              ((0, C_, n, hostN.ctypes.data, F64, 24), "not a device pointer"), ((0, C_, n + 1, p, F64, 1 << 30), "extends past its allocation"),
              ((0, C_, n + 1, p, F64, 24), "%d values given, the mesh needs %d (one per vertex)" % (n + 1, n)),
              ((0, ST_, ni, stu, F64, 16), "%d values given, the mesh needs %d (one per vertex)" % (ni, n)),
              ((0, STU_, n, st, F64, 16), "%d values given, the mesh needs %d (one per index)" % (n, ni))]
    for args, msg in acases:
        rc, err = attribute(acc.h, *args)
        assert rc == -1 and msg in err and "lh_accel_set_attribute_device" in err, (args, err)
    # Python refuses what the C call cannot take before calling it
    for bad in (lambda: acc.set_normals_device(0, meshes[0]["N"]), lambda: acc.set_normals_device(0, dN.to(torch.float16)), lambda: acc.set_normals_device(0, dN.t()),
                lambda: acc.set_normals_device(0, dN[:, :2]), lambda: acc.set_normals_device(0, dN.reshape(-1)), lambda: acc.set_attribute_device(0, C_, meshes[0]["C"]),
                lambda: acc.set_attribute_device(0, ST_, dST[:, :1]), lambda: acc.set_attribute_device(0, C_, dN.to(torch.int64)), lambda: acc.set_attribute_device(0, C_, dN.cpu())):
        with pytest.raises(ValueError):
            bad()
    # the host-pointer forms stay refused, by name
    assert L.lh_accel_set_normals(acc.h, 0, hostN.ctypes.data, 24, 0) == -1 and "device meshes" in L.lh_last_error().decode()
    with pytest.raises(la.LucilleHipError, match="device meshes"):
        acc.set_attribute(0, C_, meshes[0]["C"])
    # nothing changed: the same accelerator takes the right calls -- a wrong array first, replaced, and one set and removed again
    acc.set_normals_device(0, dev_pos(meshes[0]["N"][::-1].copy()), 0)
    acc.set_attribute_device(2, la.ATTR_TANGENT, dev_pos(meshes[2]["C"]))
    acc.set_attribute_device(2, la.ATTR_TANGENT, None)
    for k, m in enumerate(meshes):
        if "N" in m or m["two_side"]:
            s.set_normals(k, m.get("N"), m["two_side"])
        for kind, key in KINDS:
            if key in m:
                s.set_attribute(k, kind, m[key])
    acc.commit()
    prim, stt = records(acc, org, dr)
    assert np.array_equal(prim, g["prim"]) and np.array_equal(stt, g["state"])
    rc, err = normals(acc.h, 0, n, p, F64, 24)
    assert rc == -1 and "already committed" in err
    rc, err = attribute(acc.h, 0, C_, n, p, F64, 24)
    assert rc == -1 and "already committed" in err
    acc.close()
    # an accelerator with host meshes, and one with none: the calls are for device meshes and name the host form
    h = HostScene(); apply_state_scene(h, meshes, False)
    empty = la.HipAccel(0)
    for x in (h.acc, empty):
        rc, err = normals(x.h, 0, n, p, F64, 24)
        assert rc == -1 and "device meshes" in err and "lh_accel_set_normals" in err.split(";")[-1], err
        rc, err = attribute(x.h, 0, C_, n, p, F64, 24)
        assert rc == -1 and "device meshes" in err and "lh_accel_set_attribute" in err.split(";")[-1], err
    with pytest.raises(la.LucilleHipError, match="device meshes"):
        h.acc.set_normals_device(0, dN)
    h.acc.commit()
    prim, stt = records(h.acc, org, dr)
    assert np.array_equal(prim, g["prim"]) and np.array_equal(stt, g["state"])
    h.acc.close(); empty.close()


# ---- 8. no leak ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_index", [False, True])
def test_commits_with_attributes_do_not_leak_device_memory(bad_index):
    import torch
    P, idx, org, dr = po.soup(200000, 1000, 0.006, 79)
    rng = np.random.default_rng(8)
    if bad_index:
        idx = idx.copy(); idx[4567] = P.shape[0]
    dP, dI = dev_pos(P), dev_idx(idx)
    dN = dev_pos(unit(rng.normal(size=P.shape))); dC = dev_pos(rng.uniform(0, 1, P.shape)); dS = dev_pos(rng.uniform(0, 1, (P.shape[0], 2)))
    dU = dev_pos(rng.uniform(0, 1, (idx.shape[0], 2)))

    def once():
        acc = la.HipAccel(0)
        acc.add_mesh_device(dP, dI)
        acc.set_normals_device(0, dN, 1)
        for kind, d in ((la.ATTR_COLOR, dC), (la.ATTR_TANGENT, dN), (la.ATTR_BINORMAL, dC), (la.ATTR_TEXCOORD, dS), (la.ATTR_TEXCOORD_UNSHARED, dU)):
            acc.set_attribute_device(0, kind, d)
        if bad_index:
            with pytest.raises(la.LucilleHipError, match="out of range"):
                acc.commit()
        else:
            acc.commit()
            acc.intersect_host(org, dr)
        acc.close()
    once(); once()                                    # allocator pools, code objects
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(8):
        once()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    # the margin of test_device_mesh_commits_do_not_leak_device_memory: one cycle's attribute copies and arrays are > 100 MB here
    assert free0 - free1 < 16 << 20, "device memory shrank by %.1f MB over eight commits with attributes" % ((free0 - free1) / 1e6)
