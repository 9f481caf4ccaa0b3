"""The routing decision around zero-area triangles that stay in the traversal tree, at its edges, on the CPU (no device).

A ray whose largest direction component D exceeds the cap 1 / s2 AND that hits the box of a "danger" leaf (a leaf of lucille's
own tree that holds such a triangle) takes the reference's own walk; every other ray is answered by the traversal tree alone.
The records equal the reference's only if the routed rays are a SUPERSET of the rays on which the reference reports such a
triangle (from the rounding noise of its determinant, on any ray that reaches the leaf and passes through the triangle's line).
The pure parts of the decision are lh_danger.h (the box on the 16-bit grid, the device's float cap, the ray sources that take
the test), lh_filter.h (the device's box test) and lh_hostwalk.c lh_danger_hit (the host's); tests/cpu_model links them as they are.

Three edges:
 * the box was accepted up to a cell outside the grid and CLAMPED to it -- the grid covers the traversal tree's triangles, the
   box those of lucille's tree, which keeps the dead ones (two equal vertices): a dead triangle half a cell outside left a strip
   the reference's box covers and the device's did not;
 * the device compared D with the cap rounded to NEAREST float, above the double the host walk compares with for half of all
   caps, and a cap in [1 - 2^-25, 1) switched the test off for unit-vector sources;
 * axis-parallel rays: the host test skips axes with |d| <= 1e-14, the device relies on lh_safe_dir and slab_w's slack."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import danger_scenes as ds
from tests.helpers import Model

N = 100000


# ---- packing -----------------------------------------------------------------------------------------------------
def _pack_cases():
    """(grid_lo f32 [3], grid_step f32 [3], box_lo [3], box_hi [3]) for a few thousand seeded boxes: every face inside the grid,
    touching its end, or up to three cells outside.  Two grids: the unit cube's, and that of a scene far from the origin"""
    rng = np.random.default_rng(1234)
    out = []
    for g0, ext in ((np.zeros(3), np.ones(3)), (np.array([9600.0, -12345.678, 4.0e6]), np.array([7.5, 300.0, 2000.0]))):
        glo = g0.astype(np.float32)
        step = (ext / 65535.0 * (1.0 + 1e-6)).astype(np.float32); step = np.where(step.astype(np.float64) < ext / 65535.0 * (1.0 + 1e-6),
                                                                                     np.nextafter(step, np.float32(np.inf)), step)
        g = glo.astype(np.float64); st = step.astype(np.float64); top = g + 65535.0 * st
        for _ in range(1500):
            lo = np.empty(3); hi = np.empty(3)
            for k in range(3):
                kind_lo, kind_hi = rng.integers(0, 4, 2)
                # low face: well inside / within a cell inside the low end / exactly on it / up to three cells outside
                lo[k] = (g[k] + rng.uniform(0.0, 0.6) * 65535.0 * st[k], g[k] + rng.uniform(0.0, 1.0) * st[k], g[k],
                         g[k] - rng.uniform(0.0, 3.0) * st[k])[kind_lo]
                hi[k] = (top[k] - rng.uniform(0.0, 0.39) * 65535.0 * st[k], top[k] - rng.uniform(0.0, 1.0) * st[k], top[k],
                         top[k] + rng.uniform(0.0, 3.0) * st[k])[kind_hi]
            out.append((glo, step, lo, hi))
        # the ends themselves and their neighbours in double
        for k in range(3):
            for lo_k in (g[k], np.nextafter(g[k], -np.inf), np.nextafter(g[k], np.inf)):
                for hi_k in (top[k], np.nextafter(top[k], -np.inf), np.nextafter(top[k], np.inf)):
                    lo = g + 0.25 * 65535.0 * st; hi = g + 0.5 * 65535.0 * st; lo[k] = lo_k; hi[k] = hi_k
                    out.append((glo, step, lo, hi))
    return out


def test_packed_box_contains_the_union_box_or_every_ray_is_routed():
    """Whenever lh_danger_pack returns words, the box they name on the grid contains the box it was given, in fp64 on every axis;
    otherwise it says "every ray" -- and it does return words for boxes inside the grid, so the ordinary case keeps its box.
    (The clamp this replaces returned words for 1 046 of these 3 054 cases, and 479 of them cut the box.)"""
    cases = _pack_cases()
    nwords = nall = 0; bad = []
    for i, (glo, step, lo, hi) in enumerate(cases):
        w = Model.danger_pack(lo, hi, glo, step)
        g = glo.astype(np.float64); st = step.astype(np.float64)
        inside = bool(np.all(lo >= g) and np.all(hi <= g + 65535.0 * st))
        if w is None:
            nall += 1
            assert not inside, "case %d: a box inside the grid fell back to every ray: %r %r" % (i, lo, hi)
            continue
        nwords += 1
        qlo = (w & 0xFFFF).astype(np.float64); qhi = (w >> 16).astype(np.float64)
        if not (np.all(g + qlo * st <= lo) and np.all(g + qhi * st >= hi)):
            bad.append(i)
    assert nwords > 100 and nall > 1000, (nwords, nall)
    assert not bad, "%d of %d packed boxes do not contain their box, first cases %s" % (len(bad), nwords, bad[:5])


# ---- cap ---------------------------------------------------------------------------------------------------------
def _caps():
    rng = np.random.default_rng(99)
    s2 = np.exp(rng.uniform(np.log(1e-3), np.log(1e6), 1000))
    return [1.0 / 3.0, 1.0 - 2.0 ** -30, 1.0, 1.0 + 2.0 ** -52, 1024.0, np.inf] + list(1.0 / s2)


def test_device_cap_is_never_above_the_double_cap():
    """the host walk routes D > cap (double); the device routes D > (double)(float cap): the float must not be above the double.
    (Rounded to nearest: above it for 518 of these 1 006 caps, 1 / 3 among them.)"""
    above = []
    for cap in _caps():
        f = Model.dcap_device(cap)
        assert f == float(np.float32(f))
        if np.isinf(cap):
            assert np.isinf(f) and f > 0
            continue
        assert np.isfinite(f) and f >= 0.0
        if f > cap:
            above.append(cap)
        # ... and not lower than it has to be: the next float up is above the cap
        assert float(np.nextafter(np.float32(f), np.float32(np.inf))) > cap
    assert not above, "%d caps rounded up, first %r" % (len(above), above[:4])


def test_unit_vector_sources_take_the_test_whenever_a_unit_vector_can_exceed_the_cap():
    """cap_srcs bit 0: the cap is finite; bits 1 and 2 (AO rays, camera rays): set whenever the double cap is below 1 + 4 x 2^-52"""
    for cap in _caps():
        srcs = Model.dcap_srcs(cap)
        assert (srcs & 1) == (1 if np.isfinite(cap) else 0), cap
        if cap < 1.0 + 4.0 * 2.0 ** -52:
            assert srcs & 6 == 6, "cap %r: the unit-vector sources skip the test" % cap
        if cap >= 1.0 + 2.0 ** -40:
            assert srcs & 6 == 0, "cap %r: every AO and camera ray would take the test" % cap


# ---- superset, per ray -------------------------------------------------------------------------------------------
class _Scene:
    """one scene: the model (grid, lucille's tree, the cap), the oracle, the ONE danger box (the collinear triangle's leaf; one leaf:
    the scene box of lucille's tree, Model.ref_bbox())"""

    def __init__(self, high, dead, many=False):
        P, idx, self.info = (ds.many_leaf_scene if many else ds.one_leaf_scene)(high, dead)
        self.m = Model(P, idx)
        assert (self.m.ref_build()["nleaf"] == 1) == (not many)
        self.o = po.Oracle(); self.o.add_mesh(P, idx); self.o.build()
        self.lo, self.hi = self.m.ref_leaf_box(self.info["zprim"])
        if not many:
            assert all(np.array_equal(x, y) for x, y in zip((self.lo, self.hi), self.m.ref_bbox()))
        self.glo, self.step = self.m.grid()
        self.cap = self.m.deg_dcap()

    def routed_on_device(self, org, dr):
        w = Model.danger_pack(self.lo, self.hi, self.glo, self.step)
        return np.ones(org.shape[0], bool) if w is None else self.m.device_box_test(org, dr, w)

    def check_superset(self, org, dr, floor, what):
        D = np.abs(dr).max(1)
        assert np.all(D > self.cap) and np.all(D > Model.dcap_device(self.cap)) and np.all(D < 1024.0)
        assert np.all(np.abs(dr[:, 1]) > 1e-3 * np.linalg.norm(dr, axis=1))
        exp = self.o.intersect(org, dr, nthreads=8)
        hit = exp[0] == self.info["zprim"]
        assert hit.sum() >= floor, "%s: the oracle reports the collinear triangle on %d rays only" % (what, hit.sum())
        host = Model.danger_hit(org[hit], dr[hit], np.concatenate([self.lo, self.hi])[None])
        dev = self.routed_on_device(org[hit], dr[hit])
        assert host.all(), "%s: the host test misses %d of the %d rays the reference reports" % (what, (~host).sum(), hit.sum())
        assert dev.all(), "%s: the device decision misses %d of the %d rays the reference reports" % (what, (~dev).sum(), hit.sum())


class _Case:
    """a strip scene (low or high side) and the same scene without its dead triangle"""

    def __init__(self, high):
        self.high = high
        self.full = _Scene(high, True); self.bare = _Scene(high, False)
        self.info = self.full.info
        for k in ("lo", "hi", "glo", "step", "cap"):
            setattr(self, k, getattr(self.full, k))


@pytest.fixture(scope="module", params=[False, True], ids=["low", "high"])
def case(request):
    return _Case(request.param)


def test_scene_is_what_the_tests_assume(case):
    """live bounds exactly [0, 1]^3, the dead triangle half a cell outside them in lucille's box, a cap of 2.13"""
    assert np.array_equal(case.glo, np.zeros(3)) and abs(case.step[0] / ds.CELL - 1.0) < 2e-6
    assert 2.1 < case.cap < 2.2
    out = (case.hi[0] - 1.0) if case.high else -case.lo[0]
    assert 0.49 * case.step[0] < out < 0.51 * case.step[0]
    assert np.all(case.lo[1:] > -1e-13) and np.all(case.hi[1:] < 1.0 + 1e-13)
    assert np.array_equal(case.bare.glo, case.glo) and np.array_equal(case.bare.step, case.step) and case.bare.cap == case.cap
    assert np.all(case.bare.lo > -1e-13) and np.all(case.bare.hi < 1.0 + 1e-13)


def test_strip_rays_the_reference_reports_are_routed(case):
    """rays through the strip between the live bounds and the dead triangle, through the collinear triangle's extended line.
    (With the clamped box the device decision missed all 1 516 rays of the low side and all 740 of the high side.)"""
    org, dr = ds.strip_rays(N, case.info, case.high)
    assert np.all(np.linalg.norm(org - 0.5, axis=1) < 1.5) and np.all(dr[:, 0] != 0.0)
    # fp64: while a ray is within lucille's box (its y and z slabs; x follows), it stays inside (-0.5 cell, -0.2 cell) in x --
    # the high side: the same distances beyond x = 1
    xmin, xmax = ds.strip_x_range(org, dr, case.lo, case.hi)
    assert not np.isnan(xmin).any()
    c = case.step[0]
    if case.high:
        assert np.all(xmin > 1.0 + 0.2 * c) and np.all(xmax < 1.0 + 0.5 * c)
    else:
        assert np.all(xmin > -0.5 * c) and np.all(xmax < -0.2 * c)
    case.full.check_superset(org, dr, 500, "strip")
    exp0 = case.bare.o.intersect(org, dr, nthreads=8)               # without the dead triangle lucille's box ends at the live bounds
    assert (exp0[0] != po.MISS).sum() == 0


@pytest.mark.parametrize("family", ds.AXIS_FAMILIES)
def test_axis_parallel_rays_the_reference_reports_are_routed(case, family):
    """direction components that are exactly 0, through the triangle's line inside the box, with and without the dead triangle"""
    org, dr = ds.axis_rays(N, case.info, family)
    zero = {"dx0": [0], "dz0": [2], "dx0dz0": [0, 2]}[family]
    assert np.all(dr[:, zero] == 0.0) and np.all(np.linalg.norm(org - 0.5, axis=1) < 1.5)
    case.bare.check_superset(org, dr, 3000, family + ", without the dead triangle")
    case.full.check_superset(org, dr, 3000, family)


@pytest.mark.parametrize("high", [False, True], ids=["low", "high"])
def test_axis_parallel_rays_against_a_box_inside_the_grid(high):
    """the one-leaf scenes' box is lucille's scene box, which leaves the grid by its margin of 1e-14: the decision there is "every
    ray".  Here the collinear triangle's leaf lies inside the grid (404 triangles, 36 leaves, no dead triangle), the packing returns
    words, and the device's answer is lh_slab_w's: zero direction components go through lh_safe_dir and the per-ray slack.
    Floors: under half of the 1 400 and more hits per batch seen with these seeds"""
    sc = _Scene(high, False, many=True)
    assert Model.danger_pack(sc.lo, sc.hi, sc.glo, sc.step) is not None
    for family in ds.AXIS_FAMILIES:
        org, dr = ds.axis_rays(N, sc.info, family)
        sc.check_superset(org, dr, 500, "many leaves, " + family)
    # ... and the box is a box: rays far from it are not routed (the decision is not "every ray" in disguise)
    rng = np.random.default_rng(8)
    org = rng.uniform(0.0, 1.0, (2000, 3)); org[:, 0] = 0.8 if not high else 0.2
    dr = np.zeros((2000, 3)); dr[:, 1] = rng.choice([-500.0, 500.0], 2000)
    assert not sc.routed_on_device(org, dr).any()
