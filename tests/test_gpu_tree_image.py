"""The traversal trees the device holds, read back (lh_accel_tree_image) and checked node by node with tests/tree_check.py -- the checker that
tests/test_tree_check.py proves on the CPU.  Hit records of random rays (tests/test_gpu_devbuild.py) hardly see a child box one grid code too
tight (the slab test's own slack hides the grazing rays), a stack count one row short (the lost entry reads back as node 0, the ray restarts
and still gets its answer) or a triangle under two leaves (counts and speed only); here every box is decoded in fp64 and compared with the fp64
vertices below it at zero tolerance, every leaf range and every reference is accounted for, and the stack figures are recomputed from the nodes.

No rays are traced, except the 256 that make an accelerator build its 8-wide nodes on first use.  Every case: one commit, one read-back, the
checker on the 4-wide tree and -- where resident -- on the 8-wide tree; what it measured is kept (CASES / measured) so that the tests of the
stack figures further down read the same images.

Depths: q4_depth and q8_depth are the builders' own level counters.  lh_build.hip's collapse loops write one level of records per iteration
and count that level's inner children; the iteration that writes the deepest level counts none and is the last, so the counter ends at the
number of levels exactly (what "adds nothing" there is the list of level starts, which lh_device_build trims itself).  lh_bvh.c declares the
same (tests/test_bvh_builder.py: md == d4).  The checker asks for declared >= measured; this file asserts that they are equal.

A scene image received through lh_dist_broadcast_scene is not covered: tests/test_gpu_dist.py receives one only in a second process."""
import os

import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests import tree_check as tc

pytestmark = pytest.mark.gpu

SIZES = {1: 0.2, 4: 0.2, 5: 0.2, 37: 0.1, 513: 0.05, 3000: 0.05, 70000: 0.01}      # triangles -> half edge of the unit soup


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def soup(n, seed=0, nrays=1):
    return po.soup(n, nrays, SIZES.get(n, 0.05), 31000 + n + seed)


def mesh_of(tris):
    P = np.ascontiguousarray(np.asarray(tris, np.float64).reshape(-1, 3))
    return P, np.arange(P.shape[0], dtype=np.uint32)


def equal_centroids():
    rng = np.random.default_rng(9); n = 3000
    tri = 0.5 + rng.uniform(-0.3, 0.3, (n, 3, 3)); tri -= tri.mean(axis=1, keepdims=True) - 0.5
    return mesh_of(tri)


def exponential_line():
    m = 60; x = 2.0 ** -np.arange(m); z = np.zeros(m)
    tri = np.stack([np.stack([x, z, z], 1), np.stack([x * 1.0001, z + 1e-3, z], 1), np.stack([x, z, z + 1e-3], 1)], 1)
    return mesh_of(np.concatenate([tri + np.array([0, k * 2e-3, 0]) for k in range(5)]))


def planar(zvalue):
    P, idx, _, _ = soup(3000, seed=1)
    P = P.copy(); P[:, 2] = zvalue
    return P, idx


def placed(scale, offset):
    P, idx, _, _ = soup(3000, seed=2)
    return P * scale + np.asarray(offset, np.float64), idx


def with_degenerates():
    """3 000 live triangles and 300 with two equal vertices: v0 == v1, v0 == v2, and v1 == v2 -- short (dead: out of the tree) and long (they stay)"""
    P, idx, _, _ = soup(3000, seed=3)
    live = P[idx].reshape(-1, 3, 3)
    rng = np.random.default_rng(12)
    d = live[rng.integers(0, 3000, 300)].copy()
    d[0:100, 1] = d[0:100, 0]; d[100:200, 2] = d[100:200, 0]; d[200:300, 2] = d[200:300, 1]
    d[250:300, 0] += 0.5                                                   # |v1 - v0|_1 beyond 0.0988: not provably missed, kept in the tree
    tris = np.concatenate([live, d])[rng.permutation(3300)]
    return mesh_of(tris)


def few_live_among_dead():
    P, idx, _, _ = soup(5, seed=4)
    live = P[idx].reshape(-1, 3, 3)[:3]
    rng = np.random.default_rng(13)
    d = rng.uniform(0, 1, (50, 3, 3)); d[:25, 1] = d[:25, 0]; d[25:, 2] = d[25:, 0]
    return mesh_of(np.concatenate([d[:20], live, d[20:]]))


def only_dead():
    rng = np.random.default_rng(14)
    d = rng.uniform(0, 1, (40, 3, 3)); d[:20, 1] = d[:20, 0]; d[20:, 2] = d[20:, 0]
    return mesh_of(d)


def tris_of(P, idx):
    return np.asarray(P, np.float64)[np.asarray(idx).astype(np.int64)].reshape(-1, 3, 3)


def dev_pos(P):
    import torch
    return torch.from_numpy(np.ascontiguousarray(P)).cuda()


def dev_idx(I):
    import torch
    return torch.from_numpy(np.ascontiguousarray(I, np.uint32).view(np.int32)).cuda()


def first_dump(acc, P):
    """256 rays through the scene's box: the dump that makes an accelerator with wide8 = 1 bring its 8-wide nodes"""
    rng = np.random.default_rng(1)
    lo, hi = P.min(0), P.max(0)
    org = rng.uniform(lo - 1.0, hi + 1.0, (256, 3)); dr = rng.uniform(lo, hi, (256, 3)) - org
    acc.intersect_host(np.ascontiguousarray(org), np.ascontiguousarray(dr))


# ---- one image, checked ----------------------------------------------------------------------------------------------------------------------
def check_image(img, tris, what, device_built=None, want_q8=None):
    """the whole checker on one image -> what it measured, beside the declared figures"""
    n = tris.shape[0]
    assert img["ntris"] == n and img["q4nodes"].shape[0] == img["nq4"] >= 1 and img["q8nodes"].shape[0] == img["nq8"], what
    assert img["tri32"].shape[0] == n and img["tri64"].shape == (n, 3, 3), what
    if device_built is not None:
        assert img["device_built"] == int(device_built), what
    if want_q8 is not None:
        assert (img["nq8"] > 0) == bool(want_q8), (what, img["nq8"])
    assert (img["nq8"] == 0) == (img["q8_depth"] == 0) and (img["nq8"] == 0 or img["nq4"] > 1), what
    built = bool(img["device_built"])
    try:
        tc.check_records(img["tri32"], img["tri64"], tris, img["nlive"], img["bmin"], img["bmax"], img["scene_r"])
        r4 = tc.check_tree(img["q4nodes"], 4, img["tri32"], tris, img["grid_lo"], img["grid_step"], img["nlive"], img["q4_depth"],
                           stack=img["q4_stack"], device_built=built, pairs=os.environ.get("LH_Q4_PAIRS", "1") != "0")
        r8 = None
        if img["nq8"]:
            r8 = tc.check_tree(img["q8nodes"], 8, img["tri32"], tris, img["grid_lo"], img["grid_step"], img["nlive"], img["q8_depth"])
    except tc.TreeError as e:
        raise AssertionError("%s (%s-built, %d triangles, %d live): %s" % (what, "device" if built else "host", n, img["nlive"], e)) from e
    print("%s: %s-built, %d / %d triangles, 4-wide %d nodes %d levels (declared %d) need %d + 5 (declared %d)%s"
          % (what, "device" if built else "host", img["nlive"], n, img["nq4"], r4["levels"], img["q4_depth"], r4["need"], img["q4_stack"],
             "" if r8 is None else ", 8-wide %d nodes %d levels (declared %d) need %d" % (img["nq8"], r8["levels"], img["q8_depth"], r8["need"])))
    assert img["q4_depth"] == r4["levels"], (what, img["q4_depth"], r4)            # the module's docstring: the counters are exact
    if built:
        assert img["q4_stack"] == (r4["need"] + 5 if img["nq4"] > 1 else 0), (what, img["q4_stack"], r4)
    if r8 is not None:
        assert img["q8_depth"] == r8["levels"], (what, img["q8_depth"], r8)
        assert r8["nleaves"] == r4["nleaves"] and r8["npad"] == 0, (what, r4, r8)          # the same leaves; no padding among the 8-wide nodes
    return {"q4_stack": img["q4_stack"], "q4_depth": img["q4_depth"], "q8_depth": img["q8_depth"], "nq8": img["nq8"],
            "need4": r4["need"], "need8": None if r8 is None else r8["need"]}


def device_commit(P, idx, wide8=None):
    acc = la.HipAccel(0); acc.add_mesh(P, idx)
    if wide8 is not None:
        acc.set_param("wide8", wide8)
    acc.commit(on_device=True)
    return acc


# ---- the cases: name -> a function that commits, reads back, checks and returns what check_image returns ---------------------------------
CASES = {}
_measured = {}


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def measured(name):
    if name not in _measured:
        _measured[name] = CASES[name]()
    return _measured[name]


def _size_case(n, wide8):
    def run():
        P, idx, _, _ = soup(n)
        acc = device_commit(P, idx, wide8)
        try:
            # without the knob the builder makes no 8-wide nodes, and a tree of one node has no 8-wide form (five triangles may be such a tree)
            want_q8 = False if (not wide8 or n <= 4) else (None if n == 5 else True)
            return check_image(acc.tree_image(), tris_of(P, idx), "soup %d, wide8 = %d" % (n, wide8), device_built=True, want_q8=want_q8)
        finally:
            acc.close()
    return run


for _n in SIZES:
    for _w in (0, 1):
        CASES["soup-%d%s" % (_n, "-wide8" if _w else "")] = _size_case(_n, _w)


def _distribution_case(what, make, device_built=True):
    def run():
        P, idx = make()
        acc = device_commit(P, idx, 1)
        try:
            return check_image(acc.tree_image(), tris_of(P, idx), what, device_built=device_built)
        finally:
            acc.close()
    return run


CASES["equal-centroids"] = _distribution_case("equal centroids", equal_centroids)
CASES["exponential-line"] = _distribution_case("exponential line", exponential_line, device_built=None)      # (the commit may fall back to the host builder)
CASES["planar-z-exact"] = _distribution_case("every z = 0.25: an axis of no extent, grid_step 1e-30", lambda: planar(0.25))
CASES["planar-z-one-ulp"] = _distribution_case("every z = 0.1, no float: an axis one ulp wide", lambda: planar(0.1))
CASES["scaled-1e3-moved"] = _distribution_case("soup x 1e3 + (-800, 400, -200)", lambda: placed(1e3, (-800.0, 400.0, -200.0)))
CASES["scaled-1e-3"] = _distribution_case("soup x 1e-3", lambda: placed(1e-3, (0.0, 0.0, 0.0)))
CASES["degenerates-among-live"] = _distribution_case("3 000 live + 300 with two equal vertices", with_degenerates)
CASES["few-live-among-dead"] = _distribution_case("3 live + 50 dead: one leaf after the sort", few_live_among_dead)
CASES["only-dead"] = _distribution_case("40 dead triangles: the drop is given up", only_dead)


@case("host-commit")
def _host_commit():
    """the upload of the host builder's trees; then wide8 = 1 after the commit: lh_ensure_formats builds and uploads the 8-wide nodes on first use"""
    P, idx, _, _ = soup(3000, seed=5)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(build="host")
    try:
        check_image(acc.tree_image(), tris_of(P, idx), "host commit", device_built=False, want_q8=False)
        acc.set_param("wide8", 1)
        first_dump(acc, P)
        return check_image(acc.tree_image(), tris_of(P, idx), "host commit, 8-wide nodes on first use", device_built=False, want_q8=True)
    finally:
        acc.close()


@case("device-commit-wide8-later")
def _device_commit_wide8_later():
    """the 8-wide nodes of a device-built scene asked for after the commit: a second run of the builder on first use"""
    P, idx, _, _ = soup(3000, seed=6)
    acc = device_commit(P, idx, 0)
    try:
        before = acc.tree_image()
        check_image(before, tris_of(P, idx), "device commit, wide8 = 0", device_built=True, want_q8=False)
        acc.set_param("wide8", 1)
        first_dump(acc, P)
        after = acc.tree_image()
        got = check_image(after, tris_of(P, idx), "device commit, 8-wide nodes on first use", device_built=True, want_q8=True)
        for k in ("q4nodes", "tri32", "tri64"):                             # the second run leaves what is resident as it is
            assert after[k].tobytes() == before[k].tobytes(), k
        return got
    finally:
        acc.close()


def _device_mesh_case(dt):
    def run():
        P, idx, _, _ = soup(3000, seed=7)
        Q = np.ascontiguousarray(P.astype(dt))
        acc = la.HipAccel(0); acc.set_param("wide8", 1); acc.add_mesh_device(dev_pos(Q), dev_idx(idx)); acc.commit()
        try:
            return check_image(acc.tree_image(), tris_of(Q, idx), "device mesh, %s positions" % np.dtype(dt).name, device_built=True, want_q8=True)
        finally:
            acc.close()
    return run


CASES["device-mesh-f64"] = _device_mesh_case(np.float64)
CASES["device-mesh-f32"] = _device_mesh_case(np.float32)


@case("device-mesh-recommit")
def _device_mesh_recommit():
    """an updatable device mesh, new vertices, a re-commit: the boxes contain the NEW vertices, tri64 is the new input"""
    P, idx, _, _ = soup(3000, seed=8)
    rng = np.random.default_rng(15)
    N = P * np.array([1.5, 0.75, 1.0]) + np.array([3.0, -2.0, 5.0]) + rng.uniform(-0.02, 0.02, P.shape)
    acc = la.HipAccel(0); acc.set_param("updatable", 1); acc.set_param("wide8", 1); acc.add_mesh_device(dev_pos(P), dev_idx(idx)); acc.commit()
    try:
        check_image(acc.tree_image(), tris_of(P, idx), "updatable device mesh, first commit", device_built=True)
        acc.update_mesh_device(0, dev_pos(N))
        r = acc.recommit()
        assert (r["flattened"], r["rebuilt_trees"]) == (1, 1), r
        img = acc.tree_image()
        with pytest.raises(AssertionError):                                 # ... and not the old ones
            check_image(img, tris_of(P, idx), "the re-committed image against the OLD vertices")
        return check_image(img, tris_of(N, idx), "updatable device mesh, re-committed", device_built=True)
    finally:
        acc.close()


@case("multi-replica-1")
def _multi_replica():
    """replica 1 of an lh_multi commit: on the second device where two are visible, else -- as tests/test_gpu_multi.py does -- on the same device
    once more (the same replica path: a device-built scene is built again for the replica, a host-built one uploaded again)"""
    import torch
    second = 1 if torch.cuda.device_count() >= 2 else 0
    P, idx, _, _ = soup(3000, seed=9)
    out = None
    for code, built in ((-2, True), (0, False)):
        m = la.HipMulti([0, second]); m.add_mesh(P, idx); m.commit(code)
        try:
            for k in (0, 1):
                got = check_image(m.accel(k).tree_image(), tris_of(P, idx), "lh_multi replica %d, %s commit" % (k, "device" if built else "host"), device_built=built)
                out = out or (got if k == 1 else None)
        finally:
            m.close()
    return out


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_resident_trees_hold_every_invariant(name):
    measured(name)


@pytest.mark.parametrize("name", list(CASES))
def test_unchecked_rows_cover_the_four_wide_need(name):
    """q4_stack (or, where it is 0, 3 x q4_depth + 5) is what lh_plan_rows4 sizes the LDS columns with.  A batch under 65 536 rays walks them
    UNCHECKED while they are 64 or fewer (`guard` 0), a larger one while they are 34 or fewer: the rows of such a launch must cover the need
    recomputed from the read-back nodes -- the entries a ray holds when it steps at its deepest node + 5 (the sentinel and the step's own writes)"""
    f = measured(name)
    for dense in (False, True):
        rows, guard = tc.plan_rows4(f["q4_stack"], f["q4_depth"], dense)
        assert rows % 2 == 0 and rows <= tc.ROWS_UNCHECKED
        if not guard:
            assert rows >= f["need4"] + 5, (name, dense, rows, f)
    if name.startswith("soup-"):          # no soup here is deep enough for the checked walk: the bound above was exercised
        assert not tc.plan_rows4(f["q4_stack"], f["q4_depth"], False)[1], (name, f)


@pytest.mark.parametrize("name", list(CASES))
def test_unchecked_rows_cover_the_eight_wide_need(name):
    """q8_depth sizes the 8-wide walk's columns: 7 x q8_depth + 10 rows, unchecked up to 48.  Recomputed: the entries a ray holds when it steps at
    its deepest 8-wide node (children - 1 per ancestor) + 10, the plan's own constant for the step's seven pushes, the sentinel and the
    scratch row"""
    f = measured(name)
    if not f["nq8"]:
        assert f["q8_depth"] == 0 and f["need8"] is None                    # nothing resident, nothing declared
        return
    rows, guard = tc.plan_rows8(f["q8_depth"])
    assert rows % 2 == 0 and rows <= tc.ROWS8_CAP
    if not guard:
        assert rows >= f["need8"] + 10, (name, rows, f)


def test_an_accelerator_that_is_not_committed_is_refused():
    P, idx, _, _ = soup(37)
    acc = la.HipAccel(0); acc.add_mesh(P, idx)
    with pytest.raises(la.LucilleHipError, match="lh_accel_tree_image: accel not committed"):
        acc.tree_image()
    acc.commit(on_device=True)
    assert acc.tree_image()["ntris"] == 37
    acc.close()


def test_every_pointer_may_be_null_and_the_call_changes_nothing():
    """the figures alone, one array alone; two read-backs are the same bytes, and so are the hit records before and after"""
    import ctypes as C
    from lucille_amd import binding
    P, idx, org, dr = soup(513, nrays=2000)
    acc = device_commit(P, idx, 1)
    before = acc.intersect_host(org, dr)
    a = acc.tree_image()
    info = binding.TreeImage()
    assert acc.L.lh_accel_tree_image(acc.h, C.byref(info), None, None, None, None) == 0 and info.nq4 == a["nq4"] and info.nq8 == a["nq8"] > 0
    assert acc.L.lh_accel_tree_image(acc.h, None, None, None, None, None) == 0
    q8 = np.zeros(a["nq8"], la.HipAccel.Q8_NODE)
    assert acc.L.lh_accel_tree_image(acc.h, None, None, q8.ctypes.data_as(C.c_void_p), None, None) == 0
    assert q8.tobytes() == a["q8nodes"].tobytes()
    b = acc.tree_image()
    for k in ("q4nodes", "q8nodes", "tri32", "tri64"):
        assert a[k].tobytes() == b[k].tobytes(), k
    after = acc.intersect_host(org, dr)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    acc.close()
