"""The built-in gather sampler on the device (lh_ao_ray_builtin, lucille_amd/csrc/lh_ao.h) against the model of tests/ao_sampler.py -- an independent
statement of the rule, held to the host-compiled header and to its own statistics in tests/test_ao_sampler_rule.py:

  (a) one-triangle scenes whose hit record holds only 0 and +-1, through ao_rays_device: every component of a direction is then a float32 value of the
      local vector, which is compared with the model component by component;
  (b) general bases and the frame key, through the tile pipeline's scratch;
  (c) the generator's edges (z0 == 1: a ray in the tangent plane; z1 == 1; phi = 0; the ray Ns) through the stages, against the oracle.

K, the tolerance of the two trigonometric components (cospi(2 z1) ct and sinpi(2 z1) ct as float32 products of the device's sincospif) against the model's
fp64 products, in units of the last place of float32: the largest error measured over all cases of (a) is K_MEASURED; the tests assert that figure rounded up
to a whole ulp plus one (another ROCm's polynomial may round the last place the other way), and never more than 4, OpenCL's bound for sinpi / cospi."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests import ao_sampler as sm
from tests.helpers import load_golden
from tests.test_gpu_ao_batch import NO_HIT, ao, ao_rays, dev, expected, host
from tests.test_gpu_dirt import dirt, same_bits
from tests.test_gpu_envgather import RGB, env, sky

pytestmark = pytest.mark.gpu

K_MEASURED = 1.8232          # ulp32, the largest error of a trigonometric component over the cases of (a)
K = min(int(np.ceil(K_MEASURED)) + 1, 4)
SEEDS = (0, 5, 0x8000000000000005)
GRIDS = (1, 2, 3, 4, 9, 16, 17, 64, 289)
EDGE_GRIDS = (4, 16, 64)


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ulp32(x):
    """the unit in the last place of float32 at the fp64 value x"""
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def edge_keys(ns):
    found = sm.find_edge_keys(5, ns)
    assert all(found[e] is not None for e in sm.EDGES), (ns, found)
    return found


def oracle_records(o, org, dr, rec):
    """the 12-double AO records of the hits, from the oracle: lo_state_build, then lo_ortho_basis of Ns -> [nhits, 12] in ray order"""
    L = po.lib()
    L.lo_ortho_basis.argtypes = [po._dp, po._dp]
    prim, t, u, v = rec
    out = []
    for i in np.nonzero(prim != po.MISS)[0]:
        P = np.empty(3); Ng = np.empty(3); Ns = np.empty(3); B = np.empty((3, 3))
        L.lo_state_build(o.h, int(prim[i]), float(t[i]), float(u[i]), float(v[i]), org[i].ctypes.data_as(po._dp), dr[i].ctypes.data_as(po._dp),
                         P.ctypes.data_as(po._dp), Ng.ctypes.data_as(po._dp), Ns.ctypes.data_as(po._dp), None)
        L.lo_ortho_basis(B.ctypes.data_as(po._dp), Ns.ctypes.data_as(po._dp))
        out.append(np.concatenate([P + Ns * 1.0e-6, B[0], B[1], Ns]))
    return np.array(out)


# ---- (a) axis scenes ------------------------------------------------------------------------------------------------------------------------
def axis_scene(axis, sign):
    """the triangle (0,0,0) (4,0,0) (0,4,0) turned so that its normal is sign * e_axis (its area 8 makes the normal exact), 64 rays straight down onto
    points of it whose coordinates are sixteenths, and 3 rays that miss"""
    eu, ev, en = np.eye(3)[(axis + 1) % 3], np.eye(3)[(axis + 2) % 3], np.eye(3)[axis] * sign
    V = np.array([0 * eu, 4 * eu, 4 * ev] if sign > 0 else [0 * eu, 4 * ev, 4 * eu])
    rng = np.random.default_rng(10 + 2 * axis + (sign > 0))
    st = rng.integers(1, 31, (67, 2)) / 16.0
    org = st[:, :1] * eu + st[:, 1:] * ev + en
    dr = np.tile(-en, (67, 1))          # (with sign +1 the two zeros of the direction are -0.0: tests/test_gpu_signed_zero.py)
    for m in (5, 20, 66):
        dr[m] = en
    return V, np.arange(3, dtype=np.uint32), org, dr


@pytest.fixture(scope="module")
def worst():
    """the largest errors of (a), gathered over its cases"""
    return {"trig": 0.0}


@pytest.mark.parametrize("axis,sign", [(a, s) for a in range(3) for s in (1, -1)])
def test_axis_scenes_against_the_model(axis, sign, worst):
    """every local component on every world axis with either sign: origins bit for bit, every direction component an exact float32 value, st bit for bit
    (0 at the z0 == 1 key), the trigonometric components within K ulp32 of the model's fp64 products, all three bit for bit at the phi = 0 keys.
    Measured on an MI355X: the largest error of a trigonometric component over the six scenes is 1.8232 ulp32 (K_MEASURED), so K = 3 is asserted."""
    import torch
    V, idx, org, dr = axis_scene(axis, sign)
    acc = la.HipAccel(0); acc.add_mesh(V, idx); acc.commit(); acc.wait_exact()
    o = po.Oracle(); o.add_mesh(V, idx); o.build()
    try:
        to, td = dev(org), dev(dr)
        rec = acc.intersect_device(to, td); torch.cuda.synchronize()
        hrec = (host(rec[0], np.uint32).copy(), host(rec[1]).copy(), host(rec[2]).copy(), host(rec[3]).copy())
        h = oracle_records(o, org, dr, hrec)
        ids = np.nonzero(hrec[0] != po.MISS)[0]
        n = org.shape[0]
        assert ids.size == 64 == h.shape[0] and set(np.nonzero(hrec[0] == po.MISS)[0]) == {5, 20, 66}
        # the record holds 0 and +-1 alone: tangent, binormal, Ns are signed unit vectors, one on every axis
        B = h[:, 3:12].reshape(-1, 3, 3)
        assert np.isin(B, (0.0, 1.0, -1.0)).all() and (np.abs(B).sum(axis=2) == 1).all() and (np.abs(B).sum(axis=1) == 1).all()
        assert (B[:, 2] == np.eye(3)[axis] * sign).all() and (B == B[0]).all()
        scan = np.full(n, NO_HIT, np.uint32); scan[ids] = np.arange(ids.size, dtype=np.uint32)
        rng = np.random.default_rng(100 + 2 * axis + (sign > 0))
        big = 0.0
        for seed in SEEDS:
            for ns in GRIDS:
                N = sm.grid(ns)[2]
                low = rng.integers(0, 1 << 34, n).astype(np.uint64)
                sets = [("random", low), ("high bits", low ^ (rng.integers(1, 1 << 30, n).astype(np.uint64) << np.uint64(34))), ("identity", None)]
                found = None
                if seed == 5 and ns in EDGE_GRIDS:
                    found = edge_keys(ns)
                    sets.append(("edges", np.resize(np.array([found[e][0] for e in sm.EDGES], np.uint64), n)))
                for name, key in sets:
                    slot, nslots, aorg, adir = ao_rays(acc, to, td, rec, ns, seed=seed, key=None if key is None else dev(key))
                    what = (name, seed, ns)
                    assert np.array_equal(slot, scan) and nslots == ids.size, what
                    assert np.array_equal(u64(aorg), u64(np.repeat(h[:, 0:3], N, axis=0))), what
                    kk = (np.arange(n, dtype=np.uint64) if key is None else key)[ids]
                    L = sm.local(seed, kk, ns)
                    adir = adir.reshape(ids.size, N, 3)
                    assert np.array_equal(adir, adir.astype(np.float32).astype(np.float64)), what
                    loc = np.stack([(adir * B[:, None, k, :]).sum(axis=2) for k in range(3)], axis=-1)          # exact: one term is +-d, two are 0
                    assert np.array_equal((loc[..., 2].astype(np.float32) + np.float32(0)).view(np.uint32), L["st"].view(np.uint32)), what
                    err = np.abs(loc[..., 0:2] - L["ref"][..., 0:2]) / ulp32(L["ref"][..., 0:2])
                    big = max(big, float(err.max()))
                    assert err.max() <= K, (what, float(err.max()))
                    exact = (L["r1"] == 0.0) & (L["j"] == 0)[None, :]          # phi = 0: the device's sincospif(0) is (0, 1) like any
                    assert np.array_equal(u64(adir[exact]), u64(sm.world(h, L["f32"])[exact])), what
                    if found is not None and name == "edges":
                        e_of = {e: np.nonzero(kk == np.uint64(found[e][0]))[0] for e in sm.EDGES}
                        assert all(v.size >= 8 for v in e_of.values())
                        r = found["z0_one"][1]
                        assert (L["z0"][e_of["z0_one"], r] == 1.0).all() and (loc[e_of["z0_one"], r, 2] == 0.0).all(), what
                        r = found["phi_zero"][1]
                        assert exact[e_of["phi_zero"], r].all() and (loc[e_of["phi_zero"], r, 1] == 0.0).all(), what
                        r = found["r0_zero"][1]
                        assert np.array_equal(adir[e_of["r0_zero"], r], B[e_of["r0_zero"], 2]), what          # d = Ns
                        r = found["z1_one"][1]
                        assert (L["z1"][e_of["z1_one"], r] == 1.0).all(), what
        worst["trig"] = max(worst["trig"], big)
        print("axis %d sign %+d: largest error of a trigonometric component %.4f ulp32 (so far %.4f); asserted K = %d" % (axis, sign, big, worst["trig"], K))
    finally:
        acc.close()


# ---- (b) general bases and the frame key ----------------------------------------------------------------------------------------------------
def load_scene(name):
    g = load_golden(name)
    acc = la.HipAccel(0)
    for k in range(int(g["ngeoms"])):
        acc.add_mesh(g["pos%d" % k], g["idx%d" % k])
        if ("nrm%d" % k) in g.files:
            acc.set_normals(k, g["nrm%d" % k], int(g["two_side%d" % k]))
    acc.commit()
    ocam = po.Camera.from_ref(g["camera"])
    return {"acc": acc, "cam": la.Camera.make(ocam.width, ocam.height, ocam.flength, list(ocam.cam2world), ocam.rh)}


@pytest.fixture(scope="module")
def scenes():
    s = {"ao_c1": load_scene("ao_c1"), "ao_ps": load_scene("ao_ps")}
    yield s
    for v in s.values():
        v["acc"].close()


TILES = {"tile (4, 8, 24, 16)": (4, 8, 24, 16), "tile (37, 101, 50, 23)": (37, 101, 50, 23), "tile (37, 41, 50, 23)": (37, 41, 50, 23)}
REGIONS = tuple(TILES) + ("frame", "bands")


@pytest.mark.parametrize("ns", [9, 16])
@pytest.mark.parametrize("pxs", [1, 2])
@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("which", ["ao_c1", "ao_ps"])
def test_frame_keys_and_general_bases(scenes, which, region, pxs, ns):
    """The tile pipeline with "ao_fused" 0 shows its rays in scratch 0 .. 10.  The hit slots are the hits in sample order; the key of a slot is
    tests.ao_sampler.frame_key of the pixel and sub-sample of its sample index (lines below ao_ps's 96 -- all of tile (37, 101, 50, 23) there -- are
    outside the frame and hit nothing; tile (37, 41, 50, 23) is that tile inside ao_ps's frame); scratch 8 is the record's origin, bit for bit; and
    scratch 9 is within
        (K + 2) 2^-23 (|d0 h[3+k]| + |d1 h[6+k]|) + 4 * 2^-52 (|d0 h[3+k]| + |d1 h[6+k]| + |d2 h[9+k]|)
    of the model's fp64 direction through the record of scratch 7, component k by component.  The device's d0, d1 are float32 values within K ulp32 of
    the model's fp64 products d0, d1, and an ulp32 of x is at most 2^-23 |x|: the two products d0 h[3+k], d1 h[6+k] move by at most
    K 2^-23 (|d0 h[3+k]| + |d1 h[6+k]|); d2 is the model's bit for bit.  Either side then rounds three products, each by at most 2^-53 of its own
    term -- together at most 2^-53 M, M = |d0 h[3+k]| + |d1 h[6+k]| + |d2 h[9+k]| -- and two sums, each by at most 2^-53 of a partial sum that is at most
    M: 3 * 2^-53 M a side, 3 * 2^-52 M for both.  The fourth 2^-52 M and the 2 added to K cover the second-order terms (M is K 2^-23 larger on the
    device's side, the partial sums carry the products' roundings).
    The key of a slot is checked through the directions it generates, that is its low 34 bits; the self-primitive bits above them (the primitive, or
    LH_SLOT_NOSELF under interpolated normals) are not in the scratch and are not looked at here -- the occluded counts of
    test_edges_through_the_stages and of tests/test_gpu_ao_batch.py depend on them.
    render_ao_bands (two full-width bands of 16 lines from lines 8 and 40, one device batch) goes through the same stage and shows the same scratch: it is
    held to the same check."""
    acc, cam = scenes[which]["acc"], scenes[which]["cam"]
    W, H = cam.width, cam.height
    N = sm.grid(ns)[2]
    acc.set_param("ao_fused", 0)
    try:
        if region == "bands":
            x0, w, lines = 0, W, np.concatenate([np.arange(8, 24), np.arange(40, 56)])
            _, st = acc.render_ao_bands(cam, [8, 40], 16, pxs, ns, seed=5)
        else:
            x0, y0, w, hh = (0, 0, W, H) if region == "frame" else TILES[region]
            lines = np.arange(y0, y0 + hh)
            _, st = acc.render_ao_tile(cam, x0, y0, w, hh, pxs, ns, seed=5)
        s = {k: acc.scratch(k, dt, wd) for k, dt, wd in ((2, np.uint32, 1), (6, np.uint32, 1), (7, np.float64, 12), (8, np.float64, 3), (9, np.float64, 3))}
    finally:
        acc.set_param("ao_fused", 1)
    nsamp = w * lines.size * pxs * pxs
    assert s[2].shape[0] == s[6].shape[0] == nsamp
    hit = s[2] != po.MISS
    nslots = int(hit.sum())
    assert st["primary_hits"] == nslots == s[7].shape[0] and s[8].shape[0] == s[9].shape[0] == nslots * N
    assert not hit[np.repeat(lines >= H, w * pxs * pxs)].any()
    if region == "tile (37, 101, 50, 23)" and which == "ao_ps":
        assert nslots == 0
    if region == "frame":
        assert nslots > 1000
    scan = np.full(nsamp, NO_HIT, np.uint32); scan[hit] = np.arange(nslots, dtype=np.uint32)
    assert np.array_equal(s[6], scan)
    keys = sm.region_keys(x0, w, lines, pxs, W)[hit]
    assert np.array_equal(u64(s[8]), u64(np.repeat(s[7][:, 0:3], N, axis=0)))
    got = s[9].reshape(nslots, N, 3)
    worst_ratio = 0.0
    for b in range(0, nslots, 1 << 15):
        e = min(b + (1 << 15), nslots)
        L = sm.local(5, keys[b:e], ns)
        h = s[7][b:e]
        want = sm.world(h, L["ref"])
        d = np.abs(L["ref"])
        trig = np.stack([d[..., 0] * np.abs(h[:, None, 3 + k]) + d[..., 1] * np.abs(h[:, None, 6 + k]) for k in range(3)], axis=-1)
        full = trig + np.stack([d[..., 2] * np.abs(h[:, None, 9 + k]) for k in range(3)], axis=-1)
        bound = (K + 2) * 2.0 ** -23 * trig + 4 * 2.0 ** -52 * full
        err = np.abs(got[b:e] - want)
        assert (err <= bound).all(), (which, region, pxs, ns, int((err > bound).any(axis=(1, 2)).sum()), e - b)
        worst_ratio = max(worst_ratio, float((err / np.maximum(bound, 1e-300)).max()))
    print("%s %s ps %d ns %d: %d slots, largest error / bound %.3f" % (which, region, pxs, ns, nslots, worst_ratio))


# ---- (c) the edges through the stages -------------------------------------------------------------------------------------------------------
def edge_scene():
    """a floor of two triangles, 2000 a side, tilted off every axis (the determinant `a` of triangle_isect for a ray in the floor's plane is rounding noise,
    not an exact 0), a seeded soup of 300 blockers above its middle, and 320 rays down onto the floor from below the blockers"""
    rng = np.random.default_rng(2026)
    nrm = np.array([0.3, 0.5, 0.81]); nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    c = np.array([1.7, -2.3, 0.9])
    q = [c + 1000.0 * (a * e1 + b * e2) for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    floor = np.array([q[0], q[1], q[2], q[0], q[2], q[3]])
    if np.dot(np.cross(floor[1] - floor[0], floor[2] - floor[0]), nrm) < 0:
        floor = floor[[0, 2, 1, 3, 5, 4]]
    nb = 300
    ctr = c + rng.uniform(-9, 9, (nb, 1)) * e1 + rng.uniform(-9, 9, (nb, 1)) * e2 + rng.uniform(0.3, 3.0, (nb, 1)) * nrm
    soup = (ctr[:, None, :] + 0.8 * rng.standard_normal((nb, 3, 3))).reshape(-1, 3)
    soup = soup + np.maximum(0.05 - (soup - c) @ nrm, 0.0)[:, None] * nrm          # every blocker vertex at least 0.05 above the floor
    n = 320
    p = c + rng.uniform(-5, 5, (n, 1)) * e1 + rng.uniform(-5, 5, (n, 1)) * e2
    org = p + 0.02 * nrm
    dr = np.tile(-nrm, (n, 1))
    return floor, soup, org, dr


@pytest.fixture(scope="module")
def edges():
    import torch
    floor, soup, org, dr = edge_scene()
    P = np.concatenate([floor, soup]); idx = np.arange(P.shape[0], dtype=np.uint32)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    acc.set_environment(RGB, sky())
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    alone = po.Oracle(); alone.add_mesh(floor, np.arange(6, dtype=np.uint32)); alone.build()          # the floor without its blockers
    to, td = dev(org), dev(dr)
    rec = acc.intersect_device(to, td); torch.cuda.synchronize()
    prim = host(rec[0], np.uint32).copy()
    assert np.isin(prim, (0, 1)).all() and (prim == 0).sum() > 50 and (prim == 1).sum() > 50          # every ray lands on the floor, on both triangles
    # the keys: each edge key of each grid on 8 hits, the rest random
    rng = np.random.default_rng(77)
    key = rng.integers(0, 1 << 34, org.shape[0]).astype(np.uint64)
    at = 0
    for ns in EDGE_GRIDS:
        found = edge_keys(ns)
        for e in sm.EDGES:
            key[at:at + 8] = found[e][0]; at += 8
    key = key[rng.permutation(key.size)]
    yield {"acc": acc, "oracle": o, "alone": alone, "org": to, "dr": td, "rec": rec, "prim": prim, "key": key, "dkey": dev(key)}
    acc.close()


@pytest.mark.parametrize("ns", EDGE_GRIDS)
def test_edges_through_the_stages(edges, ns):
    """ao_device, fused and materialised, gives the oracle's any-hit counts over the rays ao_rays_device shows for the batch, bit for bit -- the batch
    holds every edge key of every grid on 8 hits; 20 % to 80 % of the gather rays are occluded in the oracle's answer; dirt_device and env_device answer
    fused as materialised.
    The rays with st == 0 start 1e-6 above a flat-shaded triangle and run parallel to it: the self-primitive skip (lh_ao.h) rests on the oracle not
    hitting that triangle, which is asserted on the floor without its blockers."""
    acc, o = edges["acc"], edges["oracle"]
    org, dr, rec, key = edges["org"], edges["dr"], edges["rec"], edges["key"]
    N = sm.grid(ns)[2]
    n = key.size
    slot, nslots, aorg, adir = ao_rays(acc, org, dr, rec, ns, seed=5, key=edges["dkey"])
    assert nslots == n and np.array_equal(slot, np.arange(n, dtype=np.uint32))
    L = sm.local(5, key, ns)
    found = edge_keys(ns)
    flat = L["st"] == 0.0
    assert flat.sum() == 8 and (flat == ((key == np.uint64(found["z0_one"][0]))[:, None] & (np.arange(N) == found["z0_one"][1])[None, :])).all()
    occ = o.intersect(aorg, adir, nthreads=8)[0] != po.MISS
    share = occ.mean()
    print("ns %d: %d of %d gather rays occluded (%.1f %%); of the %d rays with st == 0: %d" % (ns, int(occ.sum()), occ.size, 100 * share, int(flat.sum()),
                                                                                           int(occ.reshape(n, N)[flat].sum())))
    assert 0.2 <= share <= 0.8
    ecnt, erad = expected(slot, occ, N)
    for fused in (1, 0):
        cnt, rad = ao(acc, org, dr, rec, ns, fused, seed=5, key=edges["dkey"])
        assert np.array_equal(cnt, ecnt), (fused, np.nonzero(cnt != ecnt)[0][:8], key[cnt != ecnt][:8])
        assert same_bits(rad, erad), fused
    # the rays in the tangent plane: d . Ns == 0 as far as the basis is orthogonal, and the floor is not hit -- neither the triangle the ray starts on,
    # nor its neighbour in the same plane
    fo, fd = aorg.reshape(n, N, 3)[flat], adir.reshape(n, N, 3)[flat]
    assert set(edges["prim"][np.nonzero(flat)[0]]) == {0, 1}          # on both triangles of the floor
    nrm = np.array([0.3, 0.5, 0.81]); nrm /= np.linalg.norm(nrm)
    assert (np.abs(fd @ nrm) < 1e-14).all()
    assert (edges["alone"].intersect(fo, fd)[0] == po.MISS).all()
    # and every ray of the batch: the floor alone occludes nothing (the hemisphere is above it)
    assert (edges["alone"].intersect(aorg, adir, nthreads=8)[0] == po.MISS).all()
    dc = {f: dirt(acc, org, dr, rec, ns, la.DirtParams(0.1, 2.0, 1e-5), f, seed=5, key=edges["dkey"]) for f in (1, 0)}
    assert np.array_equal(dc[1][0], dc[0][0]) and same_bits(dc[1][1], dc[0][1])
    assert (dc[1][0] != NO_HIT).all() and 0 < int(dc[1][0].sum()) < n * N
    ec = {f: env(acc, org, dr, rec, ns, la.EnvParams(1e-5, 1.0), f, seed=5, key=edges["dkey"]) for f in (1, 0)}
    assert np.array_equal(ec[1][0], ec[0][0]) and same_bits(ec[1][1], ec[0][1])
    assert 0 < int(ec[1][0].sum()) < n * N and (ec[1][1] > 0).any()
