"""Updatable device meshes (set_param("updatable", 1); lh_accel_update_mesh_device; lh_accel_recommit): after every re-commit the accelerator must be
the one a caller gets by creating a new one from the new positions.  The expected answer comes from two independent sources each time -- oracle.pyoracle
on the new positions, and a fresh (not updatable) accelerator built from them -- and both the host batch and the device batch are compared with them,
closest hit and any hit, bit for bit.  The helpers follow tests/test_gpu_device_mesh.py."""
import os

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding, scenes
from oracle import pyoracle as po
from tests.helpers import assert_hits_equal, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_KEYS = ("ntriangles", "ntriangles_in_tree", "nnodes_traversal", "nnodes", "max_depth", "nleaves")


def dev_idx(I):
    import torch
    return torch.from_numpy(np.ascontiguousarray(I, np.uint32).view(np.int32)).cuda()


def dev_pos(P):
    import torch
    return torch.from_numpy(np.ascontiguousarray(P)).cuda()


def device_mesh_accel(meshes, updatable=False, before_commit=None):
    """meshes: (positions tensor, indices tensor) pairs, added in order"""
    acc = la.HipAccel(0)
    if updatable:
        acc.set_param("updatable", 1)
    for P, I in meshes:
        acc.add_mesh_device(P, I)
    if before_commit:
        before_commit(acc)
    info = acc.commit()
    return acc, info


def oracle_of(meshes):
    o = po.Oracle()
    for P, I in meshes:
        I = np.asarray(I, np.uint32)
        if I.shape[0] >= 3:
            o.add_mesh(np.asarray(P, np.float64)[:, :3], I[:I.shape[0] - I.shape[0] % 3])        # primitive ids do not see empty meshes or trailing indices
    o.build()
    return o


def device_records(acc, org, dr, mode=la.MODE_CLOSEST):
    import torch
    out = acc.intersect_device(torch.from_numpy(org).cuda(), torch.from_numpy(dr).cuda(), mode=mode)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().view(np.uint32) if x.dtype == torch.int32 else x.cpu().numpy() for x in out)


def check_records(acc, ref, exp, org, dr, what):
    """closest-hit records of both batch paths against the oracle (a) and the fresh accelerator (b); any-hit = prim != MISS"""
    got = acc.intersect_host(org, dr)
    assert_hits_equal(got, exp, what + ": host batch against the oracle")
    gd = device_records(acc, org, dr)
    assert_hits_equal(gd, exp, what + ": device batch against the oracle")
    if ref is not None:
        assert_hits_equal(got, ref.intersect_host(org, dr), what + ": host batch against the fresh accelerator")
        assert_hits_equal(gd, device_records(ref, org, dr), what + ": device batch against the fresh accelerator")
    hit = exp[0] != po.MISS
    assert np.array_equal(acc.intersect_host(org, dr, mode=la.MODE_ANY).astype(bool), hit), what + ": any hit, host batch"
    assert np.array_equal(device_records(acc, org, dr, la.MODE_ANY)[0].astype(bool), hit), what + ": any hit, device batch"


def check_like_fresh(acc, ref, what):
    ai, bi = acc.info(), ref.info()
    assert all(ai[k] == bi[k] for k in INFO_KEYS), (what, ai, bi)
    an, ap = acc.ref_tree(); bn, bp = ref.ref_tree()
    assert an.tobytes() == bn.tobytes() and np.array_equal(ap, bp), what + ": lucille's own tree"


# ---- 1. parity over sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f64", "f32"])
@pytest.mark.parametrize("ntri,he,seed", [(1, 0.2, 1), (3, 0.2, 2), (4, 0.2, 3), (5, 0.2, 4), (37, 0.1, 5), (3000, 0.05, 6), (200000, 0.008, 7)])
def test_parity(ntri, he, seed, fmt):
    P0, idx, o3, d3 = po.soup(ntri, 20000, he, 1000 + seed)
    dt = np.float32 if fmt == "f32" else np.float64
    shift = np.array([3.0, -2.0, 5.0])
    rng = np.random.default_rng(seed)
    # the placements, in the vertices' own format (the oracle and the fresh accelerator get the widened values)
    Q = [P0.astype(dt)]
    Q.append((Q[0] + shift.astype(dt)).astype(dt))                                  # the bounds and the grid move
    Q.append((Q[1] * dt(1000.0)).astype(dt))                                          # the grid step changes
    Q.append((Q[2] + (rng.uniform(-1, 1, P0.shape) * 0.2 * he * 1000.0).astype(dt)).astype(dt))      # the topology changes
    # 60 000 rays, drawn once: a third through each distinct placement (the jitter stays inside the scaled one)
    org = np.ascontiguousarray(np.concatenate([o3, o3 + shift, 1000.0 * (o3 + shift)]))
    dr = np.ascontiguousarray(np.concatenate([d3, d3, 1000.0 * d3]))
    assert org.shape[0] == 60000
    dI = dev_idx(idx)
    acc, info0 = device_mesh_accel([(dev_pos(Q[0]), dI)], updatable=True)
    exp0 = oracle_of([(Q[0], idx)]).intersect(org, dr, nthreads=8)
    check_records(acc, None, exp0, org, dr, "first commit")
    first = acc.intersect_host(org, dr)
    bytes0 = acc.info()["device_bytes"]
    hits = [(exp0[0] != po.MISS).sum()]
    for k in (1, 2, 3):
        what = "%d triangles, %s, update %d" % (ntri, fmt, k)
        acc.update_mesh_device(0, dev_pos(Q[k]))
        r = acc.recommit()
        assert (r["flattened"], r["rebuilt_trees"], r["regathered"]) == (1, 1, 1) and r["ntriangles"] == ntri, (what, r)
        ref, _ = device_mesh_accel([(dev_pos(Q[k]), dI)])
        exp = oracle_of([(Q[k], idx)]).intersect(org, dr, nthreads=8)
        hits.append((exp[0] != po.MISS).sum())
        check_records(acc, ref, exp, org, dr, what)
        check_like_fresh(acc, ref, what)
        ref.close()
    assert min(hits) > 0 and (ntri < 3000 or min(hits) > 1000), hits          # the rays cross every placement
    # back to the first positions: the first commit's records, its bytes
    acc.update_mesh_device(0, dev_pos(Q[0]))
    r = acc.recommit()
    assert_hits_equal(acc.intersect_host(org, dr), first, "back to the first positions")
    assert_hits_equal(device_records(acc, org, dr), exp0, "back to the first positions, device batch")
    assert r["device_bytes"] == bytes0 and all(r[k] == info0[k] for k in INFO_KEYS), (r, info0, bytes0)
    acc.close()


# ---- 2. several meshes ----------------------------------------------------------------------------------------------------------------------
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
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    dmeshes = [(d0, dev_idx(I0)), (dev_pos(P1), dev_idx(I1)), (dev_pos(P2), dev_idx(I2)), (empty, dev_idx(I3)), (dev_pos(P4), dev_idx(I4)), (d0, dev_idx(I5))]
    assert dmeshes[1][0].stride(0) * 8 == 32 and dmeshes[2][0].stride(0) * 4 == 16
    acc, info = device_mesh_accel(dmeshes, updatable=True)
    # only mesh 1 moves, handed over as fp32 at stride 12 although it was added as fp64 at stride 32; the empty mesh takes an update and does nothing
    N1 = (S[1][0] * 0.7 + np.array([0.2, 0.1, -0.1])).astype(np.float32)
    assert dev_pos(N1).stride(0) * 4 == 12
    acc.update_mesh_device(1, dev_pos(N1))
    acc.update_mesh_device(3, empty)
    r = acc.recommit()
    assert (r["flattened"], r["rebuilt_trees"]) == (1, 1)
    hmeshes = [(P0, I0), (N1.astype(np.float64), I1), (P2[:, :3].astype(np.float64), I2), (P3, I3), (P4, I4), (P0, I5)]
    fresh = [dmeshes[0], (dev_pos(N1), dmeshes[1][1])] + dmeshes[2:]
    ref, _ = device_mesh_accel(fresh)
    ntri = sum(m[1].shape[0] // 3 for m in hmeshes)
    assert r["ntriangles"] == ntri == ref.info()["ntriangles"]
    for p in range(ntri):
        assert acc.prim_lookup(p) == ref.prim_lookup(p), p
    exp = oracle_of(hmeshes).intersect(org, dr, nthreads=8)
    assert (exp[0] != po.MISS).sum() > 100
    check_records(acc, ref, exp, org, dr, "six meshes, mesh 1 updated")
    check_like_fresh(acc, ref, "six meshes")
    acc.close(); ref.close()


# ---- 3. slivers come and go ------------------------------------------------------------------------------------------------------------------
def sliver_soup():
    """the 2 000-triangle soup of tests/test_gpu_device_mesh.py degenerate_cases, and its "zero-area, collinear, duplicates" form"""
    P, idx, org, dr = po.soup(2000, 30000, 0.05, 4100)
    T = P.reshape(-1, 3, 3).copy()
    T[0:200:4, 1] = T[0:200:4, 0]; T[1:200:4, 2] = T[1:200:4, 0]; T[2:200:4, 2] = T[2:200:4, 1]
    T[200:300, 2] = T[200:300, 0] + 2.0 * (T[200:300, 1] - T[200:300, 0])
    T[300:340] = T[1000]
    return np.ascontiguousarray(P), np.ascontiguousarray(T.reshape(-1, 3)), idx, np.ascontiguousarray(org), np.ascontiguousarray(dr)


def same_danger(acc, ref):
    """the danger list of both sides (lh_accel_danger_list): a stale one only routes other rays to the reference's walk, no record shows it"""
    a, b = acc.danger_list(), ref.danger_list()
    return a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()


def test_slivers_come_and_go():
    P, D, idx, org, dr = sliver_soup()
    dI = dev_idx(idx)
    acc, info0 = device_mesh_accel([(dev_pos(P), dI)], updatable=True)
    first = acc.intersect_host(org, dr)
    assert info0["ntriangles_in_tree"] == 2000
    ref0, _ = device_mesh_accel([(dev_pos(P), dI)])
    # into the degenerate form: triangles leave the traversal tree, the collinear ones that stay cap the directions
    acc.update_mesh_device(0, dev_pos(D)); r = acc.recommit()
    ref, _ = device_mesh_accel([(dev_pos(D), dI)])
    assert r["ntriangles_in_tree"] < 2000 and r["ntriangles_in_tree"] == ref.info()["ntriangles_in_tree"]
    check_records(acc, ref, oracle_of([(D, idx)]).intersect(org, dr, nthreads=8), org, dr, "degenerate form")
    check_like_fresh(acc, ref, "degenerate form")
    # this form holds a hundred collinear triangles, more than a list takes (LH_DANGER_MAX = 16): every ray beyond the cap is routed, here as on the
    # fresh accelerator; the scene without slivers has no list either (and no cap)
    assert ref0.danger_list()[0] == 0 and ref0.danger_list()[2].shape[0] == 0
    assert same_danger(acc, ref), (acc.danger_list(), ref.danger_list())
    ref.close()
    # the slivers move to other triangles: a list of the OLD boxes that stayed would route other rays; the oracle cannot see that, the list itself can
    listed = None
    for lo in (1200, 1500):                               # ten slivers (a list holds them), then ten others
        T2 = P.reshape(-1, 3, 3).copy()
        T2[lo:lo + 10, 2] = T2[lo:lo + 10, 0] + 2.0 * (T2[lo:lo + 10, 1] - T2[lo:lo + 10, 0])
        D2 = np.ascontiguousarray(T2.reshape(-1, 3))
        acc.update_mesh_device(0, dev_pos(D2)); r = acc.recommit()
        ref, rinfo = device_mesh_accel([(dev_pos(D2), dI)])
        assert all(r[k] == rinfo[k] for k in INFO_KEYS), (r, rinfo)
        check_records(acc, ref, oracle_of([(D2, idx)]).intersect(org, dr, nthreads=8), org, dr, "slivers at %d" % lo)
        now = acc.danger_list()
        assert now[2].shape[0] > 0 and same_danger(acc, ref), (now, ref.danger_list())          # a danger list appears: the fresh accelerator's
        assert listed is None or now[2].tobytes() != listed[2].tobytes()                        # ... and not the one of the slivers that left
        listed = now
        ref.close()
    # and back: no sliver, no list -- info and the count must be the fresh accelerator's
    acc.update_mesh_device(0, dev_pos(P)); r = acc.recommit()
    ref, rinfo = device_mesh_accel([(dev_pos(P), dI)])
    assert r["ntriangles_in_tree"] == 2000
    assert all(r[k] == rinfo[k] for k in INFO_KEYS) and r["device_bytes"] == rinfo["device_bytes"] == info0["device_bytes"], (r, rinfo)
    assert_hits_equal(acc.intersect_host(org, dr), first, "back from the degenerate form")
    check_records(acc, ref, first, org, dr, "back from the degenerate form")
    assert acc.danger_list()[0] == 0 and same_danger(acc, ref) and same_danger(acc, ref0), acc.danger_list()
    ref.close(); ref0.close()
    # every triangle collapsed to a point: every ray misses
    Z = np.repeat(P.reshape(-1, 3, 3)[:, :1], 3, axis=1).reshape(-1, 3)
    acc.update_mesh_device(0, dev_pos(np.ascontiguousarray(Z))); r = acc.recommit()
    ref, rinfo = device_mesh_accel([(dev_pos(np.ascontiguousarray(Z)), dI)])
    assert r["ntriangles"] == 2000 and all(r[k] == rinfo[k] for k in INFO_KEYS), (r, rinfo)          # (a scene of nothing else is built as it was handed over)
    check_like_fresh(acc, ref, "points")
    ref.close()
    rec = acc.intersect_host(org, dr)
    assert (rec[0] == po.MISS).all() and not acc.intersect_host(org, dr, mode=la.MODE_ANY).any()
    assert (device_records(acc, org, dr)[0] == po.MISS).all() and not device_records(acc, org, dr, la.MODE_ANY)[0].any()
    acc.close()


# ---- 4. exact-t ties ---------------------------------------------------------------------------------------------------------------------------
def test_exact_t_ties_after_a_translation():
    g = load_golden("ao_c1")
    P, I = scenes.tessellate(g["pos0"], g["idx0"], 3)
    shift = np.array([2.0, 4.0, -8.0])
    Pn = P + shift
    assert np.array_equal(Pn - shift, P)                    # exact in fp64 for these coordinates: the moved scene has the ties of the first
    acc, _ = device_mesh_accel([(dev_pos(P), dev_idx(I))], updatable=True)
    acc.update_mesh_device(0, dev_pos(Pn)); acc.recommit()
    ref, _ = device_mesh_accel([(dev_pos(Pn), dev_idx(I))])
    o = po.Oracle(); o.add_mesh(Pn, I); o.build()
    rng = np.random.default_rng(4)
    T = Pn[I.astype(np.int64)].reshape(-1, 3, 3)
    pick = rng.integers(0, T.shape[0], 20000)
    tgt = T[pick, rng.integers(0, 3, 20000)].copy()                         # exactly a vertex
    tgt[::2] = 0.5 * (T[pick[::2], 0] + T[pick[::2], 1])                    # exactly an edge midpoint
    org = tgt + rng.normal(size=tgt.shape) * 3.0
    dr = tgt - org
    ok = np.abs(dr[:, 1]) > 1e-14
    org, dr = np.ascontiguousarray(org[ok]), np.ascontiguousarray(dr[ok])
    exp = o.intersect(org, dr, nthreads=8)
    check_records(acc, ref, exp, org, dr, "moved scene, ties")
    check_like_fresh(acc, ref, "moved scene")
    assert o.count_equal_t(org[:4000], dr[:4000], exp[1][:4000]).max() >= 2       # ties really occur
    acc.close(); ref.close()


# ---- 5. old geometry until the re-commit; stream order; launches in flight ----------------------------------------------------------------------
def test_old_geometry_until_the_recommit():
    import torch
    P, idx, org, dr = po.soup(50000, 40000, 0.01, 5100)
    Pn = np.ascontiguousarray(P[::-1] * 0.9 + 0.05)
    old = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
    new = oracle_of([(Pn, idx)]).intersect(org, dr, nthreads=8)
    assert not np.array_equal(old[0], new[0])
    acc, _ = device_mesh_accel([(dev_pos(P), dev_idx(idx))], updatable=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    src = dev_pos(Pn); d_org = torch.from_numpy(org).cuda(); d_dir = torch.from_numpy(dr).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        acc.update_mesh_device(0, src, stream=s1)
        src.fill_(123.0)                                  # same stream, behind the library's copy
    with torch.cuda.stream(s2):
        inflight = acc.intersect_device(d_org, d_dir, stream=s2.cuda_stream)          # enqueued before the re-commit: the old scene, whenever it runs
    assert_hits_equal(acc.intersect_host(org, dr), old, "staged, not re-committed: host batch")
    acc.recommit()
    s2.synchronize()
    got = tuple(x.cpu().numpy().view(np.uint32) if x.dtype == torch.int32 else x.cpu().numpy() for x in inflight)
    assert_hits_equal(got, old, "the batch enqueued before the re-commit")
    check_records(acc, None, new, org, dr, "after the re-commit")
    torch.cuda.synchronize()
    assert float(src[0, 0]) == 123.0
    acc.close()


# ---- 6. everything else survives ---------------------------------------------------------------------------------------------------------------
def test_everything_else_survives():
    import torch
    g = load_golden("ao_c1")
    meshes = [(np.ascontiguousarray(g["pos%d" % k]), np.ascontiguousarray(g["idx%d" % k])) for k in range(int(g["ngeoms"]))]
    rng = np.random.default_rng(21)
    nrm = [rng.normal(size=P.shape) for P, _ in meshes]
    nrm = [np.ascontiguousarray(n / np.linalg.norm(n, axis=1, keepdims=True)) for n in nrm]
    a = 0.3                                                  # a rotation about z: the normals must turn with the vertices
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rot = lambda X: np.ascontiguousarray(X @ R.T)
    tex = rng.uniform(0.2, 1.5, (5, 7, 4)).astype(np.float32)
    envmap = rng.uniform(0.0, 2.0, (4, 8, 4)).astype(np.float32)
    sg = np.load(os.path.join(ROOT, "tests", "golden", "sky_reference.npz"))
    s = sg["site0"]
    sky = la.Sky.from_site(s[0], s[1], s[2], int(s[3]), s[4], s[5], basis_rgb=sg["basis_rgb"], basis_y=sg["basis_y"], sun_rgb=sg["sun_rgb0"], flags=la.SKY_SUN)
    st = [rng.uniform(0, 1, (P.shape[0], 2)) for P, _ in meshes]

    def build(pos, normals, updatable):
        def before(acc):
            acc.set_param("wide8", 1)
            for k in range(len(meshes)):
                acc.set_normals_device(k, dev_pos(normals[k]))
                acc.set_attribute_device(k, la.ATTR_TEXCOORD, dev_pos(st[k]))
        acc, _ = device_mesh_accel([(dev_pos(P), dev_idx(I)) for P, (_, I) in zip(pos, meshes)], updatable=updatable, before_commit=before)
        acc.set_texture(0, tex)
        acc.set_material(1, la.Material.make(kd=(0.3, 0.6, 0.9), ks=(0.2, 0.2, 0.2)))
        acc.set_environment((1.0, 0.5, 2.0), envmap)
        return acc

    c = g["camera"]
    cam = la.Camera.make(64, 64, c[16], c[:16], int(c[19])); cam2 = la.Camera.make(32, 32, c[16], c[:16], int(c[19]))

    def frames(acc):
        out = []
        acc.reset_sky()
        for f in (lambda: acc.render_ao_tile(cam, 0, 0, 64, 64, 2, 16, seed=11), lambda: acc.render_env_tile(cam, 0, 0, 64, 64, 2, 16, seed=11),
                  lambda: acc.render_dirt_tile(cam, 0, 0, 64, 64, 2, 16, seed=11), lambda: acc.render_pt_tile2(cam2, 0, 0, 32, 32, 0, 4, 4, seed=12)):
            rgb, stats = f(); torch.cuda.synchronize()
            out.append((rgb.cpu().numpy().tobytes(), stats))
        acc.set_sky(sky)
        rgb, stats = acc.render_env_tile(cam, 0, 0, 64, 64, 2, 16, seed=11); torch.cuda.synchronize()
        out.append((rgb.cpu().numpy().tobytes(), stats))
        d_org, d_dir = acc.primary_rays(cam, 0, 0, 64, 64, 1); torch.cuda.synchronize()
        org = d_org.cpu().numpy().reshape(-1, 3); dr = d_dir.cpu().numpy().reshape(-1, 3)
        rec = acc.intersect_host(org, dr)
        out.append((acc.state_build(org, dr, *rec).tobytes(), int((rec[0] != po.MISS).sum())))
        return out

    acc = build([P for P, _ in meshes], nrm, True)
    acc.set_sky(sky)
    assert acc.dump_node_bytes() == 128
    before = frames(acc)
    newP = [rot(P) for P, _ in meshes]; newN = [rot(n) for n in nrm]
    for k in range(len(meshes)):
        acc.update_mesh_device(k, dev_pos(newP[k]))
        acc.set_normals_device(k, dev_pos(newN[k]))
    r = acc.recommit()
    assert (r["flattened"], r["rebuilt_trees"], r["regathered"]) == (1, 1, 1)
    assert acc.dump_node_bytes() == 128
    ref = build(newP, newN, False)
    got, want = frames(acc), frames(ref)
    names = ("ao tile", "env tile", "dirt tile", "pt tile", "env tile under the sky", "state records of the camera rays")
    for name, x, y, z in zip(names, got, want, before):
        assert x[1] == y[1], (name, x[1], y[1])
        assert x[0] == y[0], name + ": bytes differ from the fresh accelerator's"
        assert x[0] != z[0], name + ": the frame did not change with the scene"
    assert got[0][1]["primary_hits"] > 1000 and got[5][1] > 100
    check_like_fresh(acc, ref, "rotated scene")
    # a 60 000-ray dump over the 8-wide nodes against the oracle
    allP = np.concatenate(newP)
    lo, hi = allP.min(axis=0), allP.max(axis=0)
    org = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (60000, 3))
    dr = np.ascontiguousarray(allP[rng.integers(0, allP.shape[0], 60000)] + rng.normal(scale=0.05, size=(60000, 3)) - org)
    exp = oracle_of([(P, I) for P, (_, I) in zip(newP, meshes)]).intersect(org, dr, nthreads=8)
    assert (exp[0] != po.MISS).sum() > 10000
    check_records(acc, ref, exp, org, dr, "dump over the 8-wide nodes")
    acc.close(); ref.close()


# ---- 7. what was redone ------------------------------------------------------------------------------------------------------------------------
def test_what_was_redone():
    P, idx, org, dr = po.soup(3000, 20000, 0.05, 8100)
    rng = np.random.default_rng(3)
    col = rng.uniform(0, 1, P.shape); col2 = rng.uniform(0, 1, P.shape)
    dI = dev_idx(idx)
    acc, _ = device_mesh_accel([(dev_pos(P), dI)], updatable=True, before_commit=lambda a: a.set_attribute_device(0, la.ATTR_COLOR, dev_pos(col)))
    r = acc.recommit()
    assert (r["flattened"], r["rebuilt_trees"], r["regathered"]) == (0, 0, 0)          # nothing staged
    tree = acc.ref_tree()
    rec = acc.intersect_host(org, dr)
    assert (rec[0] != po.MISS).sum() > 1000
    st0 = acc.state_build(org, dr, *rec)
    # the same positions again: flattened, compared, the trees stand
    acc.update_mesh_device(0, dev_pos(P))
    r = acc.recommit()
    assert (r["flattened"], r["rebuilt_trees"]) == (1, 0)
    t2 = acc.ref_tree()
    assert tree[0].tobytes() == t2[0].tobytes() and np.array_equal(tree[1], t2[1])
    assert_hits_equal(acc.intersect_host(org, dr), rec, "unchanged positions")
    assert acc.state_build(org, dr, *rec).tobytes() == st0.tobytes()
    # a colour alone: gathered again, no tree built
    acc.set_attribute_device(0, la.ATTR_COLOR, dev_pos(col2))
    assert acc.state_build(org, dr, *rec).tobytes() == st0.tobytes()                   # staged only
    r = acc.recommit()
    assert (r["flattened"], r["rebuilt_trees"], r["regathered"]) == (0, 0, 1)
    t3 = acc.ref_tree()
    assert tree[0].tobytes() == t3[0].tobytes() and np.array_equal(tree[1], t3[1])
    st1 = acc.state_build(org, dr, *rec)
    hit = rec[0] != po.MISS
    assert not np.array_equal(st1[hit][:, 15:18], st0[hit][:, 15:18])                   # P Ng Ns tangent binormal COLOR st I inside
    keep = np.r_[0:15, 18:24]
    assert st1[:, keep].tobytes() == st0[:, keep].tobytes()
    ref, _ = device_mesh_accel([(dev_pos(P), dI)], before_commit=lambda a: a.set_attribute_device(0, la.ATTR_COLOR, dev_pos(col2)))
    assert ref.state_build(org, dr, *rec).tobytes() == st1.tobytes()
    assert_hits_equal(acc.intersect_host(org, dr), rec, "after the attribute-only re-commit")
    acc.close(); ref.close()


# ---- 8. refusals and failures leave a working accelerator ---------------------------------------------------------------------------------------
def _raw_update(acc, mesh, npos, pos, fmt, stride):
    L = binding.lib()
    rc = L.lh_accel_update_mesh_device(acc.h, mesh, npos, pos, fmt, stride, None)
    return rc, L.lh_last_error().decode()


def test_refusals_and_failures_leave_a_working_accelerator():
    P, idx, org, dr = po.soup(500, 20000, 0.08, 6100)
    old = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
    dP = dev_pos(P); dI = dev_idx(idx); dP32 = dev_pos(P.astype(np.float32))
    n = P.shape[0]
    p, p32 = dP.data_ptr(), dP32.data_ptr()
    hostP = np.ascontiguousarray(P)
    F64, F32 = binding.POS_F64, binding.POS_F32
    acc = la.HipAccel(0); acc.set_param("updatable", 1)
    with pytest.raises(la.LucilleHipError, match="cannot be mixed"):
        acc.add_mesh(P, idx)
    acc.add_mesh_device(dP, dI)
    rc, err = _raw_update(acc, 0, n, p, F64, 24)
    assert rc == -1 and "not committed" in err
    with pytest.raises(la.LucilleHipError, match="not committed"):
        acc.recommit()
    acc.commit()
    with pytest.raises(la.LucilleHipError, match="before the commit"):
        acc.set_param("updatable", 0)
    cases = [
        ((1, n, p, F64, 24), "mesh 1 out of range"),
        ((0, n - 1, p, F64, 24), "%d positions given, the mesh has %d" % (n - 1, n)),
        ((0, n, p, 2, 24), "unknown position format"),
        ((0, n, p, F64, 16), "bad stride"),
        ((0, n, p, F64, 28), "bad stride"),
        ((0, n, p32, F32, 8), "bad stride"),
        ((0, n, p32, F32, 14), "bad stride"),
        ((0, n, p + 4, F64, 24), "positions not aligned"),
        ((0, n, p32 + 2, F32, 12), "positions not aligned"),
        ((0, n, None, F64, 24), "NULL array"),
        ((0, n, hostP.ctypes.data, F64, 24), "not a device pointer"),
        ((0, n, p, F64, 1 << 30), "extends past its allocation"),
    ]
    for args, msg in cases:
        rc, err = _raw_update(acc, *args)
        assert rc == -1 and msg in err and "lh_accel_update_mesh_device" in err, (args, err)
    r = acc.recommit()
    assert (r["flattened"], r["rebuilt_trees"], r["regathered"]) == (0, 0, 0)          # nothing was staged by any of them
    check_records(acc, None, old, org, dr, "after the refusals")
    # a referenced vertex set to NaN: the commit's message, the old scene, the staged mesh still staged; a repaired one goes through
    Pn = np.ascontiguousarray(P * 0.8 + 0.1)
    bad = Pn.copy(); bad[idx[99], 1] = np.nan
    acc.update_mesh_device(0, dev_pos(bad))
    for _ in range(2):
        with pytest.raises(la.LucilleHipError, match="lh_accel_recommit: a vertex coordinate is NaN, infinite or beyond 1e30"):
            acc.recommit()
        check_records(acc, None, old, org, dr, "after the failed re-commit")
    acc.update_mesh_device(0, dev_pos(Pn))
    r = acc.recommit()
    assert r["rebuilt_trees"] == 1
    check_records(acc, None, oracle_of([(Pn, idx)]).intersect(org, dr, nthreads=8), org, dr, "after the repaired re-commit")
    acc.close()
    # an accelerator that never set "updatable": every call of today answers as today, the new ones are refused
    plain, _ = device_mesh_accel([(dP, dI)])
    rc, err = _raw_update(plain, 0, n, p, F64, 24)
    assert rc == -1 and "not updatable" in err and "\"updatable\"" in err
    with pytest.raises(la.LucilleHipError, match="not updatable"):
        plain.recommit()
    with pytest.raises(la.LucilleHipError, match="already committed"):
        plain.set_normals_device(0, dP)
    with pytest.raises(la.LucilleHipError, match="already committed"):
        plain.set_attribute_device(0, la.ATTR_COLOR, dP)
    check_records(plain, None, old, org, dr, "not updatable")
    plain.close()
    # host meshes: the parameter is refused
    host = la.HipAccel(0); host.add_mesh(P, idx)
    with pytest.raises(la.LucilleHipError, match="cannot be mixed"):
        host.set_param("updatable", 1)
    host.close()


def exponential_line():
    """the "exponential line" of tests/test_gpu_device_mesh.py degenerate_cases, as it stands there (300 triangles: five strips of 60).  The device
    builders make its trees nowadays -- a Morton code bounds the radix tree's depth -- so the tests below lower "build_depth_cap", the depth beyond
    which the device builders are given up, to the depth of an ordinary soup: this scene, several levels deeper, then takes the paths it is named for"""
    rng = np.random.default_rng(9)
    m = 60
    x = 2.0 ** -np.arange(m)
    tri = np.stack([np.stack([x, np.zeros(m), np.zeros(m)], 1), np.stack([x * 1.0001, np.full(m, 1e-3), np.zeros(m)], 1),
                    np.stack([x, np.zeros(m), np.full(m, 1e-3)], 1)], 1)
    tri = np.concatenate([tri, tri + np.array([0, 2e-3, 0]), tri + np.array([0, 4e-3, 0]), tri + np.array([0, 6e-3, 0]), tri + np.array([0, 8e-3, 0])])
    P = np.ascontiguousarray(tri.reshape(-1, 3))
    org = rng.uniform(-0.5, 1.5, (20000, 3)); tgt = P[rng.integers(0, P.shape[0], 20000)] + rng.normal(scale=1e-4, size=(20000, 3))
    return P, np.arange(P.shape[0], dtype=np.uint32), np.ascontiguousarray(org), np.ascontiguousarray(tgt - org)


def line_and_soup():
    """the exponential line, a soup of as many triangles, and the levels of their device-built trees (the line's is the deeper one)"""
    E, idx, eorg, edr = exponential_line()
    P, sidx, org, dr = po.soup(idx.shape[0] // 3, 20000, 0.08, 6200)
    assert P.shape == E.shape and np.array_equal(sidx, idx)
    depth = []
    for X in (E, P):
        a, info = device_mesh_accel([(dev_pos(X), dev_idx(idx))])
        depth.append(info["max_depth"]); a.close()
    assert depth[0] > depth[1] >= 1, depth
    return E, eorg, edr, P, org, dr, idx, depth[1]


def test_a_commit_that_fell_back_is_not_updatable():
    E, org, dr, _, _, _, idx, cap = line_and_soup()
    host = la.HipAccel(0); host.add_mesh(E, idx); hinfo = host.commit(build="host")
    acc, info = device_mesh_accel([(dev_pos(E), dev_idx(idx))], updatable=True, before_commit=lambda a: a.set_param("build_depth_cap", cap))
    assert info["nnodes"] == hinfo["nnodes"] and info["max_depth"] == hinfo["max_depth"]          # the host builders' tree: the commit fell back
    exp = oracle_of([(E, idx)]).intersect(org, dr, nthreads=8)
    rc, err = _raw_update(acc, 0, E.shape[0], dev_pos(E).data_ptr(), binding.POS_F64, 24)
    assert rc == -1 and "not updatable" in err and "host builders" in err, err
    with pytest.raises(la.LucilleHipError, match="not updatable"):
        acc.recommit()
    with pytest.raises(la.LucilleHipError, match="already committed"):
        acc.set_normals_device(0, dev_pos(E))
    check_records(acc, host, exp, org, dr, "after the refused update")
    acc.close(); host.close()


def test_an_update_the_device_builders_cannot_build():
    E, _, _, P, org, dr, idx, cap = line_and_soup()
    old = oracle_of([(P, idx)]).intersect(org, dr, nthreads=8)
    assert (old[0] != po.MISS).sum() > 100
    acc, info0 = device_mesh_accel([(dev_pos(P), dev_idx(idx))], updatable=True, before_commit=lambda a: a.set_param("build_depth_cap", cap))
    assert info0["max_depth"] == cap                      # the soup's own tree passes
    tree = acc.ref_tree()
    acc.update_mesh_device(0, dev_pos(E))
    for _ in range(2):                                    # what was staged stays staged: the second call fails the same way
        with pytest.raises(la.LucilleHipError, match=r"cannot build the updated scene \(.*\): it needs a new accelerator"):
            acc.recommit()
        check_records(acc, None, old, org, dr, "after the re-commit that could not build")
        i = acc.info()
        assert all(i[k] == info0[k] for k in INFO_KEYS) and i["device_bytes"] == info0["device_bytes"]
        t = acc.ref_tree()
        assert t[0].tobytes() == tree[0].tobytes() and np.array_equal(t[1], tree[1])
    with pytest.raises(la.LucilleHipError, match="already committed"):          # not the failed-commit state
        acc.commit()
    # a mesh the builders can build (the soup, shrunk): the same accelerator goes on
    Pn = np.ascontiguousarray(P * 0.5 + 0.25)
    acc.set_param("build_depth_cap", 86)                  # (rounding may cost the shrunk soup's tree a level)
    acc.update_mesh_device(0, dev_pos(Pn))
    r = acc.recommit()
    assert r["rebuilt_trees"] == 1
    ref, _ = device_mesh_accel([(dev_pos(Pn), dev_idx(idx))])
    check_records(acc, ref, oracle_of([(Pn, idx)]).intersect(org, dr, nthreads=8), org, dr, "after the next update")
    check_like_fresh(acc, ref, "after the next update")
    acc.close(); ref.close()
