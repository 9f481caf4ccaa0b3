"""The 4-wide node step (node_step4, lh_kernels.hip) reads a node either from the workgroup's LDS copy of the top of the tree or
from the scene's array, through two different instructions, and writes the four children's references to rank-derived stack rows.
Neither the boundary between the two fetches ("top_nodes" 0 / 16 / the default: nodes 15 and 16 sit on the two sides of it) nor
the form of the push may change a bit or a visit: records equal the textbook walk's and the oracle's, and the counting launch's
node and triangle totals are the same for every setting -- also with the stack capped at 8 rows, where the checked step and the
cooperative walk's ring form of it finish the rays.

What the totals are compared under.  An any-hit ray's walk is its own: its culling bound never moves.  A closest-hit ray's is not at
the default "tri_batch": the triangle pass waits until that many lanes of the wave hold a parked leaf, a lane that waits goes on
descending under its old bound, and which rays share a wave depends on the order the waves' atomics reach the cursors -- the
closest-hit totals of two launches with the SAME settings differ in the fourth digit (figures: profiles/node_step_trim.md).  With
"tri_batch" 1 a parked leaf is taken in the iteration it was parked in, every ray's walk is its own again, and the totals are
exact: that is where the closest-hit totals are compared (the any-hit totals: at the default as well)."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NRAYS = 65536          # a dense launch: the checked rows, the fix-up queue
TOPS = (0, 16, -1)     # no copy; a boundary inside the tree; the default (what the CU's LDS leaves over)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _records(acc, d_o, d_d, variant=la.VARIANT_DEFAULT):
    import torch
    out = acc.intersect_device(d_o, d_d, variant=variant)
    occ = acc.intersect_device(d_o, d_d, mode=la.MODE_ANY, variant=variant)[0]
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out] + [occ.cpu().numpy().astype(bool)]


def _check(acc, d_o, d_d, exp, what, direct=None):
    """records at the defaults for every top_nodes; then the totals: (any-hit nodes, tris at the defaults; closest-hit nodes, tris and
    any-hit nodes, tris with every ray's walk its own).  The knob goes last: an accelerator whose "tri_batch" was set keeps the
    caller's knobs for good (ray dumps no longer pick their own)"""
    counts = [[], [], []]
    for k, top in enumerate(TOPS):
        acc.set_param("top_nodes", top)
        got = _records(acc, d_o, d_d)
        _assert_records(got, exp, "%s, top_nodes %d" % (what, top))
        if direct is not None:
            assert all(np.array_equal(a, b) for a, b in zip(got, direct)), (what, top)
        a0 = acc.intersect_device(d_o, d_d, mode=la.MODE_ANY, counters=True)[1]
        c0 = acc.intersect_device(d_o, d_d, counters=True)[1]
        counts[k] += [a0["nodes"], a0["tris"]]
        print("    %s, top_nodes %d: closest-hit totals at the default tri_batch (not compared): %d nodes, %d tris" % (what, top, c0["nodes"], c0["tris"]))
    acc.set_param("tri_batch", 1)
    for k, top in enumerate(TOPS):
        acc.set_param("top_nodes", top)
        c = acc.intersect_device(d_o, d_d, counters=True)[1]
        a = acc.intersect_device(d_o, d_d, mode=la.MODE_ANY, counters=True)[1]
        counts[k] += [c["nodes"], c["tris"], a["nodes"], a["tris"]]
    print("%s: totals per top_nodes %s: %s" % (what, TOPS, counts))
    assert counts[0] == counts[1] == counts[2], (what, counts)
    assert min(counts[0]) > 0, (what, counts)


def _assert_records(got, exp, what):
    assert np.array_equal(got[0].view(np.uint32), exp[0]), what + ": prim"
    for k in (1, 2, 3):
        assert np.array_equal(got[k], exp[k]), what + ": " + "tuv"[k - 1]
    assert np.array_equal(got[4], exp[0] != po.MISS), what + ": any-hit"


@pytest.fixture(scope="module")
def soup():
    P, idx, org, dr = po.soup(2000, NRAYS, 0.03, 20261)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    exp = o.intersect(org, dr, nthreads=16)
    assert int((exp[0] != po.MISS).sum()) > NRAYS // 50
    return P, idx, _dev(org), _dev(dr), exp


@pytest.mark.parametrize("cap", [0, 8])
def test_records_and_visits_do_not_depend_on_the_lds_boundary(soup, cap):
    P, idx, d_o, d_d, exp = soup
    acc = la.HipAccel(0); acc.add_mesh(P, idx); info = acc.commit(); acc.set_param("wide8", 0)
    assert info["nnodes_traversal"] > 16
    direct = _records(acc, d_o, d_d, la.VARIANT_DIRECT)
    _assert_records(direct, exp, "textbook walk")
    acc.set_param("stack_cap", cap)
    _check(acc, d_o, d_d, exp, "soup, stack_cap %d" % cap, direct)
    acc.close()


def _slab_scene(ntri, rng):
    """ntri triangles that all span z = 1 .. 1.25 exactly and overlap around the z axis: every box of the tree has the same near
    and far z plane, so a ray going up the axis enters all children of a node at the bit-equal distance (the slot number in the
    key's low bits alone orders them), and a tree of 1 .. 16 such triangles has a root with one, two, three or four children
    (leaves hold up to four triangles): the empty slots of the step"""
    P = np.empty((ntri, 3, 3))
    for k in range(ntri):
        a = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
        r = rng.uniform(0.5, 1.0, 3)
        P[k, :, 0] = r * np.cos(a) + rng.uniform(-0.1, 0.1); P[k, :, 1] = r * np.sin(a) + rng.uniform(-0.1, 0.1)
        P[k, :, 2] = (1.0, 1.25, 1.0 if k % 2 else 1.25)
    return P.reshape(-1, 3), np.arange(3 * ntri, dtype=np.uint32)


@pytest.mark.parametrize("ntri", [1, 2, 3, 5, 7, 9, 11, 16])
def test_equal_entry_distances_and_empty_slots(ntri):
    rng = np.random.default_rng(100 + ntri)
    P, idx = _slab_scene(ntri, rng)
    org = np.zeros((NRAYS, 3)); org[:, :2] = rng.uniform(-0.3, 0.3, (NRAYS, 2)); org[:, 2] = rng.uniform(-1.0, 0.5, NRAYS)
    dr = np.zeros((NRAYS, 3)); dr[:, :2] = rng.uniform(-0.05, 0.05, (NRAYS, 2)); dr[:, 2] = 1.0
    dr[::7, :2] = 0.0                                                   # straight up: the z planes decide every entry distance
    dr[::5, 2] = -1.0                                                   # away from the slab: every child missed
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    exp = o.intersect(org, dr, nthreads=16)
    assert int((exp[0] != po.MISS).sum()) > NRAYS // 4
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.set_param("wide8", 0)
    d_o, d_d = _dev(org), _dev(dr)
    _assert_records(_records(acc, d_o, d_d, la.VARIANT_DIRECT), exp, "%d triangles, textbook walk" % ntri)
    _check(acc, d_o, d_d, exp, "%d triangles" % ntri)
    acc.close()
