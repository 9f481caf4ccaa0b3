"""The routing decision around zero-area triangles that stay in the traversal tree, at its edges, on the device and on every
path beside it (tests/test_danger_routing_model.py states the mechanism and pins its arithmetic on the CPU; tests/danger_scenes.py
builds the scenes and rays).  The expectation is always the oracle's records, bit for bit."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests import danger_scenes as ds
from tests.helpers import Model, assert_hits_equal

pytestmark = pytest.mark.gpu

BUILDS = ["host", "device"]


def _pack16(prim, t, u, v):
    """lh_rec16_t records of fp64 records: {prim, t, u, v rounded to float32}"""
    rec = np.empty((prim.shape[0], 4), np.uint32)
    rec[:, 0] = prim
    for k, a in ((1, t), (2, u), (3, v)):
        rec[:, k] = np.asarray(a, np.float64).astype(np.float32).view(np.uint32)
    return rec


def _commit(P, idx, build):
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(build=build); acc.wait_exact()
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    return acc, o


def _device(acc, org, dr, **kw):
    import torch
    out = acc.intersect_device(torch.from_numpy(org).cuda(), torch.from_numpy(dr).cuda(), **kw)
    cnt = None
    if kw.get("counters"):
        out, cnt = out
    torch.cuda.synchronize()
    out = tuple(x.cpu().numpy() for x in out)
    return (out, cnt) if cnt is not None else out


def check_all_paths(acc, o, org, dr, zprim, what):
    """every path that answers a ray, against the oracle: the device batch (closest hit with counters, any hit, the textbook walk,
    8-wide nodes, a small batch), the host batch, one ray at a time, and the fp32 twins of the rays with 16-byte records.
    -> (oracle records, counters of the closest-hit device batch)"""
    n = org.shape[0]
    exp = o.intersect(org, dr, nthreads=8)
    out, cnt = _device(acc, org, dr, counters=True)
    assert_hits_equal(out, exp, what + ": device batch")
    nz = int((exp[0] == zprim).sum())
    assert cnt["retraced"] >= nz, "%s: %d rays through the reference walk, the oracle reports the collinear triangle on %d" % (what, cnt["retraced"], nz)
    occ = _device(acc, org, dr, mode=la.MODE_ANY)[0]
    assert np.array_equal(occ.astype(bool), exp[0] != po.MISS), what + ": any hit"
    assert_hits_equal(_device(acc, org, dr, variant=la.VARIANT_DIRECT), exp, what + ": textbook walk")
    acc.set_param("wide8", 1)
    try:
        assert_hits_equal(_device(acc, org, dr), exp, what + ": 8-wide nodes")
    finally:
        acc.set_param("wide8", 0)
    assert_hits_equal(_device(acc, np.ascontiguousarray(org[:40]), np.ascontiguousarray(dr[:40])), tuple(x[:40] for x in exp), what + ": 40 rays")
    m = min(n, 3000)
    assert_hits_equal(acc.intersect_host(org[:m], dr[:m]), tuple(x[:m] for x in exp), what + ": host batch")
    for k in range(0, min(n, 700), 7):
        hit, p_, t_, u_, v_ = acc.intersect1(org[k], dr[k])
        assert p_ == int(exp[0][k]) and (p_ == po.MISS or (t_, u_, v_) == (exp[1][k], exp[2][k], exp[3][k])), "%s: ray %d alone" % (what, k)
    o32 = np.ascontiguousarray(org, np.float32); d32 = np.ascontiguousarray(dr, np.float32)
    exp16 = _pack16(*o.intersect(o32.astype(np.float64), d32.astype(np.float64), nthreads=8))
    rec = _device(acc, o32, d32, records="rec16")[0].view(np.uint32)
    bad = np.nonzero((rec != exp16).any(1))[0]
    assert bad.size == 0, "%s: fp32 rays, 16-byte records: %d differ, first %s" % (what, bad.size, bad[:5])
    return exp, cnt


# ---- 1. the strip, one leaf --------------------------------------------------------------------------------------
@pytest.mark.parametrize("high", [False, True], ids=["low", "high"])
@pytest.mark.parametrize("build", BUILDS)
def test_strip_one_leaf(build, high):
    """12 triangles, one leaf in lucille's tree; the dead triangle half a cell outside the live bounds takes the leaf's box out of
    the scene's grid.  100 000 rays through the strip in between, through the collinear triangle's extended line: the oracle reports
    the triangle on 1 516 of them (high side: 740) and on none once the dead triangle is gone.  With the box clamped to the grid the
    device batch on the host-built tree answered a miss on every one of them (1 516 / 740 records differed on an MI355X); the
    device-built tree passed."""
    P, idx, info = ds.one_leaf_scene(high)
    acc, o = _commit(P, idx, build)
    assert acc.info()["ntriangles"] == 12 and acc.info()["ntriangles_in_tree"] == 11
    org, dr = ds.strip_rays(100000, info, high)
    exp, cnt = check_all_paths(acc, o, org, dr, info["zprim"], "strip, %s side, %s tree" % ("high" if high else "low", build))
    assert (exp[0] == info["zprim"]).sum() >= 500
    acc.close()


# ---- 2. the strip, many leaves -----------------------------------------------------------------------------------
def _leaf_box(acc, prim):
    """from the accelerator's copy of lucille's tree: the box of `prim`'s leaf as its parent holds it -> (lo, hi)"""
    nodes, prims = acc.ref_tree()
    pos = int(np.nonzero(prims == prim)[0][0])
    leaf = [i for i in range(nodes.shape[0]) if nodes["is_leaf"][i] and nodes["first"][i] <= pos < nodes["first"][i] + nodes["count"][i]]
    assert len(leaf) == 1
    parent = int(nodes["parent"][leaf[0]]); assert parent >= 0
    box = nodes["box"][parent][0 if int(nodes["child"][parent][0]) == leaf[0] else 1]
    return box[:3].copy(), box[3:].copy()


@pytest.mark.parametrize("build", BUILDS)
def test_strip_many_leaves(build):
    """404 triangles, 36 leaves: the collinear triangle near the x = 0 face shares its leaf with the dead triangle half a cell outside.
    The rule that replaced the clamp sends every ray beyond the cap through the reference walk on such a scene; that the box path is
    still what the ordinary scene gets shows on the same scene without the dead triangle: rays beyond the cap that pass 0.3 scene
    extents away from the leaf's box walk the traversal tree.  (With the clamped box: 373 records differed on the host-built tree.)"""
    P, idx, info = ds.many_leaf_scene()
    glo, step = Model(P, idx).grid()
    acc, o = _commit(P, idx, build)
    lo, hi = _leaf_box(acc, info["zprim"])
    assert 0.3 * step[0] < glo[0] - lo[0] < 0.9 * step[0]
    org, dr = ds.strip_rays(100000, info)
    exp, cnt = check_all_paths(acc, o, org, dr, info["zprim"], "strip, many leaves, %s tree" % build)
    assert (exp[0] == info["zprim"]).sum() >= 150            # 373 with these seeds
    acc.close()
    # the control: no dead triangle, the leaf's box inside the grid
    P0, idx0, info0 = ds.many_leaf_scene(dead=False)
    acc0, o0 = _commit(P0, idx0, build)
    lo0, hi0 = _leaf_box(acc0, info0["zprim"])
    assert np.all(lo0 >= glo) and np.all(hi0 <= glo + 65535.0 * step)
    rng = np.random.default_rng(17); n = 20000
    corg = rng.uniform(0.0, 1.0, (n, 3)); corg[:, 0] = hi0[0] + 0.3 + rng.uniform(0.0, 0.2, n)
    cdr = rng.normal(size=(n, 3)); cdr[:, 0] = np.abs(cdr[:, 0]); cdr[:, 1] = np.where(np.abs(cdr[:, 1]) < 0.05, 0.05, cdr[:, 1])
    cdr *= rng.uniform(100.0, 600.0, (n, 1)) / np.abs(cdr).max(1, keepdims=True)
    assert np.all(corg[:, 0] - hi0[0] >= 0.3) and np.all(cdr[:, 0] >= 0.0)          # every point of every ray: 0.3 extents from the box or more
    assert np.all(np.abs(cdr).max(1) > 7.0)                                          # beyond the cap of 6.4
    cexp = o0.intersect(corg, cdr, nthreads=8)
    cout, ccnt = _device(acc0, corg, cdr, counters=True)
    assert_hits_equal(cout, cexp, "control, %s tree" % build)
    assert ccnt["retraced"] <= n // 20, "control: %d of %d rays through the reference walk" % (ccnt["retraced"], n)
    acc0.close()


# ---- 3. the cap's boundary ---------------------------------------------------------------------------------------
def _cap_scene(k):
    """50 live triangles in [-1, 3]^3 and the exactly collinear, dyadic triangle v0 = (1/4, 1/4, 1/4), e1 = (1/2, 1/4, 1/4), e2 = k e1:
    |e1|_1 |e2|_1 = k exactly, a computed normal of exactly zero"""
    rng = np.random.default_rng(31)
    corners = np.array([[[-1.0, -1.0, -1.0], [-0.7, -0.9, -0.9], [-0.9, -0.7, -0.9]], [[3.0, 3.0, 3.0], [2.7, 2.9, 2.9], [2.9, 2.7, 2.9]]])
    # 14 around each corner triangle (leaves of their own in lucille's tree: the collinear triangle's leaf stays inside the grid), 20 around it
    c = np.concatenate([rng.uniform(-0.85, -0.4, (14, 1, 3)), rng.uniform(2.4, 2.85, (14, 1, 3)), rng.uniform(-0.1, 2.2, (20, 1, 3))])
    live = np.concatenate([corners, c + rng.uniform(-0.15, 0.15, (48, 3, 3))])
    v0 = np.array([0.25, 0.25, 0.25]); e1 = np.array([0.5, 0.25, 0.25])
    Z = np.stack([v0, v0 + e1, v0 + k * e1])[None]
    assert np.array_equal(Z[0, 2] - v0, k * e1)
    P = np.concatenate([live, Z]).reshape(-1, 3).copy()
    return P, np.arange(P.shape[0], dtype=np.uint32), 50


def _rays_at(rng, n, centre, D, unit_y=False):
    """n rays aimed through `centre` whose largest direction component is EXACTLY D (unit_y: that component is dir.y = +-D)"""
    w = rng.normal(size=(n, 3))
    if unit_y:
        w = rng.uniform(-1.0, 1.0, (n, 3)); w[:, 1] = rng.choice([-1.0, 1.0], n)
    w[:, 1] = np.where(np.abs(w[:, 1]) < 0.05 * np.abs(w).max(1), 0.05 * np.abs(w).max(1), w[:, 1])
    dr = w / np.abs(w).max(1, keepdims=True) * D
    assert np.all(np.abs(dr).max(1) == D)
    org = centre[None] - dr / np.linalg.norm(dr, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, (n, 1))
    return np.ascontiguousarray(org), np.ascontiguousarray(dr)


@pytest.mark.parametrize("build", BUILDS)
def test_cap_boundary(build):
    """s2 = 3: the cap is the double 1 / 3 = 0.33333333333333331; rounded to nearest float it was 0.3333333432674408, and rays with D in
    between were routed by the host walk and not by the device.  D == cap is not beyond it; the next double, cap + 1e-9 and the old
    float itself are, and every such ray aimed into the leaf's box takes the reference walk.
    s2 = 1 + 2^-30: the cap 0.99999999906867743 rounds to 1.0f, which unit-length directions along an axis (D == 1.0) never exceed.
    (With the cap rounded to nearest, on both builders: 0 of the 2 000 rays at the next double took the reference walk; the records
    were equal all the same -- at D s2 = 1 the reference's noise is far below its 1e-14.)"""
    third = 1.0 / 3.0
    for k, batches in ((3.0, [(third, False), (float(np.nextafter(third, 1.0)), True), (third + 1e-9, True), (float(np.float32(third)), True)]),
                       (1.0 + 2.0 ** -30, [(1.0, True)])):
        P, idx, zprim = _cap_scene(k)
        assert Model(P, idx).deg_dcap() == 1.0 / k                 # the host builder's; the device builder rounds s2 up to a float first
        acc, o = _commit(P, idx, build)
        assert acc.info()["ntriangles_in_tree"] == 51
        lo, hi = _leaf_box(acc, zprim)
        rng = np.random.default_rng(3)
        for D, routed in batches:
            org, dr = _rays_at(rng, 2000, 0.5 * (lo + hi), D, unit_y=(k != 3.0))
            exp = o.intersect(org, dr, nthreads=8)
            what = "s2 = %r, D = %r, %s tree" % (k, D, build)
            out, cnt = _device(acc, org, dr, counters=True)
            assert_hits_equal(out, exp, what + ": device batch")
            assert_hits_equal(acc.intersect_host(org, dr), exp, what + ": host batch")
            for j in range(0, 140, 7):
                hit, p_, t_, u_, v_ = acc.intersect1(org[j], dr[j])
                assert p_ == int(exp[0][j]) and (p_ == po.MISS or (t_, u_, v_) == (exp[1][j], exp[2][j], exp[3][j])), "%s: ray %d alone" % (what, j)
            if routed:
                assert cnt["retraced"] == 2000, "%s: %d of 2000 rays through the reference walk" % (what, cnt["retraced"])
        acc.close()


# ---- 4. axis-parallel rays ---------------------------------------------------------------------------------------
def _axis_batches(info, family, box):
    """the family through the triangle itself, then with the origins' zero-direction coordinate on a face of the danger leaf's box and
    one double inside and outside of it (both faces of one such axis; for rays along y: x on a face, then z on a face)"""
    yield "through the triangle", ds.axis_rays(20000, info, family)
    for axis in {"dx0": (0,), "dz0": (2,), "dx0dz0": (0, 2)}[family]:
        for side in (0, 1):
            for ulps in (0, 1, -1):
                yield "axis %d, side %d, %+d ulp" % (axis, side, ulps), ds.axis_rays(3000, info, family, seed=7 + ulps, face=(axis, side, ulps), box=box)


@pytest.mark.parametrize("family", ds.AXIS_FAMILIES)
@pytest.mark.parametrize("build", BUILDS)
def test_axis_parallel_one_leaf(build, family):
    """direction components that are exactly 0, beyond the cap, at a danger leaf: the reference multiplies by +-DBL_MAX there, the host
    test skips the axis, the device relies on lh_safe_dir and slab_w's slack.  The one-leaf scene without the dead triangle."""
    P, idx, info = ds.one_leaf_scene(dead=False)
    m = Model(P, idx); m.ref_build()
    box = m.ref_bbox()                       # one leaf: the danger box is the scene box of lucille's tree
    acc, o = _commit(P, idx, build)
    for name, (org, dr) in _axis_batches(info, family, box):
        exp, cnt = check_all_paths(acc, o, org, dr, info["zprim"], "%s, %s, %s tree" % (family, name, build))
        if name == "through the triangle":
            assert (exp[0] == info["zprim"]).sum() >= 600           # 20 000 of the model test's 100 000 rays, its floor of 3 000
    acc.close()


@pytest.mark.parametrize("dead", [False, True], ids=["box", "every-ray"])
@pytest.mark.parametrize("family", ds.AXIS_FAMILIES)
@pytest.mark.parametrize("build", BUILDS)
def test_axis_parallel_many_leaves(build, family, dead):
    """the same on the many-leaf scene.  Without the dead triangle its danger leaf lies inside the grid: the device asks the packed box
    through slab_w.  With it every ray beyond the cap takes the reference walk."""
    P, idx, info = ds.many_leaf_scene(dead=dead)
    acc, o = _commit(P, idx, build)
    box = _leaf_box(acc, info["zprim"])
    for name, (org, dr) in _axis_batches(info, family, box):
        exp, cnt = check_all_paths(acc, o, org, dr, info["zprim"], "many leaves, %s, %s, %s tree" % (family, name, build))
        if name == "through the triangle":
            assert (exp[0] == info["zprim"]).sum() >= 100           # 280 and more with these seeds
    acc.close()
