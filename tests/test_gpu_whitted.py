"""The refraction chain on the device (lh_accel_whitted_rays_device / lh_accel_whitted_device / lh_accel_whitted_host /
lh_render_whitted_tile) against the oracle: closest hits and states from po.Oracle.state_batch, the bounce restated in numpy
(tests/whitted_chain.py, pinned to the compiled reference by tests/test_whitted_rule.py and tests/test_whitted_chain.py).  Geometry --
bounces, end rays, next rays -- is compared as bits; rgb as bits against environment_device on the end directions (that fetch is
pinned by tests/test_gpu_envgather.py)."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests import whitted_chain as wc
from tests.helpers import load_golden
from tests.test_oracle_ao import oracle_from_fixture

pytestmark = pytest.mark.gpu

NO_HIT = la.AO_NO_HIT
CUT = la.WHITTED_CUT
POISON32, POISONF, POISOND = 0x5A5A5A5A, -12345.678, -98765.4321
RGB = (1.0, 0.5, 2.0)
CONST = (0.25, 3.0, 0.5)


def sky():
    """the seeded 32 x 48 light probe of tests/test_gpu_envgather.py"""
    return np.random.default_rng(3).uniform(0.1, 2.0, (32, 48, 4)).astype(np.float32)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def poison(n):
    import torch
    return (torch.full((n,), POISON32, dtype=torch.int32, device="cuda"), torch.full((n, 3), POISOND, dtype=torch.float64, device="cuda"),
            torch.full((n, 3), POISOND, dtype=torch.float64, device="cuda"), torch.full((n, 3), POISONF, dtype=torch.float32, device="cuda"))


def make_scene(P, idx, org, dr, normals=None, env=None, device_mesh=False):
    """an accelerator and the oracle over one mesh, the rays on the device with their closest-hit records, the oracle's records and states"""
    import torch
    acc = la.HipAccel(0)
    if device_mesh:
        acc.add_mesh_device(dev(P), dev(idx))
    else:
        acc.add_mesh(P, idx)
        if normals is not None:
            acc.set_normals(0, normals, 0)
    acc.commit(); acc.wait_exact()
    if env is not None:
        acc.set_environment(*env)
    o = po.Oracle(); o.add_mesh(P, idx)
    if normals is not None:
        o.set_normals(0, normals, 0)
    o.build()
    to, td = dev(org), dev(dr)
    rec = acc.intersect_device(to, td); torch.cuda.synchronize()
    prim0, st0 = o.state_batch(org, dr)
    assert np.array_equal(host(rec[0], np.uint32), prim0)
    return {"acc": acc, "oracle": o, "org": to, "dr": td, "rec": rec, "prim0": prim0, "st0": st0, "n": org.shape[0], "chains": {}, "P": P, "idx": idx,
            "horg": org, "hdr": dr}


def helper_chain(sc, eps, eta, depth):
    """the helper's chain of the scene's rays, computed once per parameter set and left unchanged"""
    k = (eps, eta, depth)
    if k not in sc["chains"]:
        b, eo, ed, info = wc.run_chain(sc["oracle"].state_batch, sc["prim0"], sc["st0"], eps, eta, depth)
        for a in (b, eo, ed):
            a.setflags(write=False)
        sc["chains"][k] = (b, eo, ed, info)
    return sc["chains"][k]


def colours(acc, d):
    import torch
    if d.shape[0] == 0:
        return np.zeros((0, 3), np.float32)
    c = acc.environment_device(dev(d)); torch.cuda.synchronize()
    return host(c).copy()


def expected_outputs(acc, b, eo, ed, ids=None):
    """(bounces, end_org, end_dir, rgb) a call over the rays `ids` (None: all) leaves in poisoned outputs"""
    n = b.shape[0]
    listed = np.zeros(n, bool); listed[np.arange(n) if ids is None else ids] = True
    traced = listed & ~np.isnan(eo[:, 0])
    xb = np.where(listed, b, np.uint32(POISON32)).astype(np.uint32)
    xo = np.where(traced[:, None], eo, POISOND); xd = np.where(traced[:, None], ed, POISOND)
    esc = listed & (b != NO_HIT) & ((b & CUT) == 0)
    rgb = np.full((n, 3), np.float32(POISONF), np.float32)
    rgb[listed] = 0.0
    rgb[esc] = colours(acc, ed[esc])
    return xb, xo, xd, rgb


def run_device(sc, params, **kw):
    out = sc["acc"].whitted_device(sc["org"], sc["dr"], sc["rec"], params, out=poison(sc["n"]), **kw)
    return host(out[0], np.uint32).copy(), host(out[1]).copy(), host(out[2]).copy(), host(out[3]).copy()


def assert_outputs(got, exp, what=""):
    assert np.array_equal(got[0], exp[0]), (what, "bounces", int((got[0] != exp[0]).sum()))
    for k, name in ((1, "end_org"), (2, "end_dir"), (3, "rgb")):
        assert same(got[k], exp[k]), (what, name, int((bits(got[k]) != bits(exp[k])).any(axis=1).sum()))


@pytest.fixture(scope="module")
def big():
    """po.soup(3000, 5000, 0.05, 7) under the seeded sky"""
    sc = make_scene(*po.soup(3000, 5000, 0.05, 7), env=(RGB, sky()))
    yield sc
    sc["acc"].close()


@pytest.fixture(scope="module")
def small():
    """po.soup(300, 2000, 0.2, 5) under a constant environment"""
    sc = make_scene(*po.soup(300, 2000, 0.2, 5), env=(CONST,))
    yield sc
    sc["acc"].close()


# ---- 4. the bounce alone --------------------------------------------------------------------------------------------------------
def test_the_bounce_alone(big):
    import torch
    sc = big; n = sc["n"]; acc = sc["acc"]
    hit = sc["prim0"] != po.MISS
    assert 500 < int(hit.sum()) < n
    for eta in (1.33, 0.75):
        p = la.WhittedParams(1e-7, eta, 8)
        eo, ed, tir = wc.bounce_np(sc["st0"][hit, 0:3], sc["st0"][hit, 6:9], sc["st0"][hit, 20:23], p.eps, p.eta)
        assert 0 < int(tir.sum()) < int(hit.sum())
        xo = np.full((n, 3), POISOND); xd = np.full((n, 3), POISOND); xo[hit] = eo; xd[hit] = ed
        out = acc.whitted_rays_device(sc["org"], sc["dr"], sc["rec"], p, out=poison(n)[1:3]); torch.cuda.synchronize()
        assert same(host(out[0]), xo) and same(host(out[1]), xd)          # misses keep their poison
        # a list with a count below its length: the slots of rays that are not listed keep their poison too
        ids = np.random.default_rng(5).permutation(n)[:1500].astype(np.uint32); cnt = 1111
        out = acc.whitted_rays_device(sc["org"], sc["dr"], sc["rec"], p, index=dev(ids), count=dev(np.array([cnt], np.uint32)), out=poison(n)[1:3])
        torch.cuda.synchronize()
        listed = np.zeros(n, bool); listed[ids[:cnt]] = True
        assert same(host(out[0]), np.where(listed[:, None], xo, POISOND)) and same(host(out[1]), np.where(listed[:, None], xd, POISOND))


# ---- 5. the chain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [1.33, 1.0])
@pytest.mark.parametrize("depth", [8, 3, 1, 0])
@pytest.mark.parametrize("which", ["big", "small"])
def test_the_chain_equals_the_helper(request, which, depth, eta):
    sc = request.getfixturevalue(which)
    p = la.WhittedParams(1e-7, eta, depth)
    b, eo, ed, info = helper_chain(sc, p.eps, p.eta, depth)
    assert info["grazing"] == 0 and info["selfhit"] == 0
    got = run_device(sc, p)
    assert_outputs(got, expected_outputs(sc["acc"], b, eo, ed), (which, depth, eta))
    hit = sc["prim0"] != po.MISS
    cut = hit & ((b & CUT) != 0)
    assert (got[3][cut] == 0.0).all() and (got[3][~hit] == 0.0).all() and (got[0][~hit] == NO_HIT).all()          # exact zeros
    if depth == 0:
        assert (got[0][hit] == CUT).all() and (got[1] == POISOND).all() and (got[2] == POISOND).all()
    if eta == 1.33:          # what the scenes were chosen for
        if which == "big":
            assert (depth != 8 or int(cut.sum()) == 0) and (depth != 3 or int(cut.sum()) > 100)
        elif depth == 8:
            assert int(cut.sum()) >= 1 and info["tir"] >= 100 and all(r > 0 for r in info["rays"][1:])
    if depth >= 1:
        esc = hit & ~cut
        assert esc.any() and (got[3][esc] > 0.0).all()
        if which == "big":
            assert (got[3][esc][:, 0] != got[3][esc][:, 1]).any()          # the map, not a constant


def test_a_device_mesh_accelerator_gives_the_same(small):
    sc = make_scene(small["P"], small["idx"], small["horg"], small["hdr"], env=(RGB, sky()), device_mesh=True)
    try:
        p = la.WhittedParams()
        b, eo, ed, _ = helper_chain(small, p.eps, p.eta, p.max_depth)
        assert_outputs(run_device(sc, p), expected_outputs(sc["acc"], b, eo, ed), "device mesh")
    finally:
        sc["acc"].close()


def test_the_empty_scene_starts_no_chain(small):
    """a record whose primitive the scene does not have counts as a miss: in an empty scene every record does"""
    empty = la.HipAccel(0); empty.commit()
    try:
        out = empty.whitted_device(small["org"], small["dr"], small["rec"], out=poison(small["n"]))
        assert (host(out[0], np.uint32) == NO_HIT).all() and (host(out[3]) == 0.0).all() and (host(out[1]) == POISOND).all() and (host(out[2]) == POISOND).all()
    finally:
        empty.close()


# ---- 6. non-unit interpolated normals -------------------------------------------------------------------------------------------
def test_interpolated_normals_are_taken_as_they_are():
    P, idx, org, dr, N = wc.soup_with_normals(po)
    ln = np.linalg.norm(N, axis=1)
    assert ln.min() >= 0.5 and ln.max() <= 2.0 and (ln < 0.8).any() and (ln > 1.5).any()
    sc = make_scene(P, idx, org, dr, normals=N, env=(RGB, sky()))
    try:
        p = la.WhittedParams()
        b, eo, ed, info = helper_chain(sc, p.eps, p.eta, p.max_depth)
        nl = np.linalg.norm(sc["st0"][sc["prim0"] != po.MISS, 6:9], axis=1)
        assert (np.abs(nl - 1.0) > 0.05).mean() > 0.5          # most hits have an Ns that is far from unit length: it is taken as it is
        assert info["cut"] >= 1 and info["tir"] >= 100 and info["grazing"] == 0
        assert_outputs(run_device(sc, p), expected_outputs(sc["acc"], b, eo, ed), "normals")
    finally:
        sc["acc"].close()


# ---- 7. lists -------------------------------------------------------------------------------------------------------------------
def test_lists_counts_null_outputs_and_the_host_form(small):
    import torch
    sc = small; n = sc["n"]; acc = sc["acc"]
    p = la.WhittedParams(1e-7, 1.33, 5)
    b, eo, ed, _ = helper_chain(sc, p.eps, p.eta, 5)
    rng = np.random.default_rng(9)
    ids = rng.permutation(n)[:700].astype(np.uint32)
    ids = np.concatenate([ids, ids[:40], np.array([n, n + 7, 0xFFFFFFFF], np.uint32)])          # duplicates; ids beyond the rays are skipped
    rng.shuffle(ids)
    for cnt in (None, 333, 100000):
        m = ids.shape[0] if cnt is None else min(cnt, ids.shape[0])
        use = ids[:m]; use = use[use < n]
        got = run_device(sc, p, index=dev(ids), count=None if cnt is None else dev(np.array([cnt], np.uint32)))
        assert_outputs(got, expected_outputs(acc, b, eo, ed, use), ("list", cnt))
    # the identity list under a count
    got = run_device(sc, p, count=dev(np.array([257], np.uint32)))
    assert_outputs(got, expected_outputs(acc, b, eo, ed, np.arange(257)), "count alone")
    # any output may be missing: the others are as before
    full = expected_outputs(acc, b, eo, ed)
    for k in range(4):
        out = list(poison(n)); out[k] = None
        acc.whitted_device(sc["org"], sc["dr"], sc["rec"], p, out=tuple(out))
        for j in range(4):
            if j != k:
                g = host(out[j], np.uint32) if j == 0 else host(out[j])
                assert (np.array_equal(g, full[j]) if j == 0 else same(g, full[j])), (k, j)
    acc.whitted_device(sc["org"], sc["dr"], sc["rec"], p, out=(None, None, None, None))
    # the host form: untraced end rays are the zeros the binding starts from
    hb, ho, hd, hrgb = acc.whitted_host(sc["horg"], sc["hdr"], tuple(host(x, np.uint32) if i == 0 else host(x) for i, x in enumerate(sc["rec"])), p)
    traced = ~np.isnan(eo[:, 0])
    assert np.array_equal(hb, full[0]) and same(hrgb, full[3])
    assert same(ho, np.where(traced[:, None], eo, 0.0)) and same(hd, np.where(traced[:, None], ed, 0.0))
    torch.cuda.synchronize()


def test_statistics_count_the_chain_rays(small):
    sc = small; acc = sc["acc"]
    p = la.WhittedParams()
    _, _, _, info = helper_chain(sc, p.eps, p.eta, p.max_depth)
    acc.trace_statistics(True)
    try:
        acc.statistics(clear=True)
        run_device(sc, p)
        st = acc.statistics(clear=True)
        assert st["rays"] == sum(info["rays"]) > 0 and st["nodes"] > 0
    finally:
        acc.trace_statistics(False)


# ---- 8. the tile ----------------------------------------------------------------------------------------------------------------
def load_frame(name, env):
    g = load_golden(name)
    o = oracle_from_fixture(g)
    acc = la.HipAccel(0)
    for k in range(int(g["ngeoms"])):
        acc.add_mesh(g["pos%d" % k], g["idx%d" % k])
        if ("nrm%d" % k) in g.files:
            acc.set_normals(k, g["nrm%d" % k], int(g["two_side%d" % k]))
    acc.commit(); acc.wait_exact()
    acc.set_environment(*env)
    ocam = po.Camera.from_ref(g["camera"])
    cam = la.Camera.make(ocam.width, ocam.height, ocam.flength, list(ocam.cam2world), ocam.rh)
    return acc, o, cam


def tile_expected(acc, o, cam, x0, y0, w, h, ps, p):
    """primary_rays -> the helper's chain -> environment_device -> the accumulation of env_resolve restated: (rgb [h, w, 3], info, misses)"""
    import torch
    org, dr = acc.primary_rays(cam, x0, y0, w, h, ps); torch.cuda.synchronize()
    horg, hdr = host(org).copy(), host(dr).copy()
    prim0, st0 = o.state_batch(horg, hdr)
    b, eo, ed, info = wc.run_chain(o.state_batch, prim0, st0, p.eps, p.eta, p.max_depth)
    miss = prim0 == po.MISS
    esc = ~miss & ((b & CUT) == 0)
    per = np.zeros((prim0.shape[0], 3), np.float32)
    per[miss] = colours(acc, hdr[miss]); per[esc] = colours(acc, ed[esc])
    spp = ps * ps
    per = per.astype(np.float64).reshape(w * h, spp, 3)
    accum = np.zeros((w * h, 3))
    for s in range(spp):
        accum = accum + per[:, s, :]
    rgb = np.maximum((accum * (1.0 / spp)).astype(np.float32), np.float32(0.0)).reshape(h, w, 3)[::-1]
    return np.ascontiguousarray(rgb), info, int(miss.sum())


@pytest.mark.parametrize("name,x0,y0,ps,env", [("ao_ps", 24, 32, 2, "map"), ("ao_c1", 104, 112, 1, "const")])
def test_tile_equals_the_composition_and_does_not_depend_on_tiling(name, x0, y0, ps, env):
    acc, o, cam = load_frame(name, (RGB, sky()) if env == "map" else (CONST,))
    try:
        W, H = 48, 32
        p = la.WhittedParams()
        exp, info, misses = tile_expected(acc, o, cam, x0, y0, W, H, ps, p)
        S = W * H * ps * ps
        assert info["cut"] >= 1 and info["grazing"] == 0 and (name != "ao_ps" or misses > 100) and (name != "ao_c1" or misses == 0)
        acc.trace_statistics(True); acc.statistics(clear=True)
        rgb, st = acc.render_whitted_tile(cam, x0, y0, W, H, ps, p)
        stat = acc.statistics(clear=True); acc.trace_statistics(False)
        rgb = host(rgb).copy()
        assert same(rgb, exp), int((bits(rgb) != bits(exp)).sum())
        deepest = max(d for d, r in enumerate(info["rays"]) if r > 0)
        assert st == {"paths": S, "rays": S + sum(info["rays"]), "max_depth_reached": deepest}
        assert stat["rays"] == st["rays"]
        assert (rgb > 0.0).any() and (ps != 1 or (rgb == 0.0).all(axis=2).any())          # a cut chain is a black sample
        tot = 0
        for ty in (0, 1):
            for tx in (0, 1):
                q, sq = acc.render_whitted_tile(cam, x0 + 24 * tx, y0 + 16 * ty, 24, 16, ps, p)
                # image orientation: the tile at frame lines y0 + 16 ty .. is rows H - 16 (ty + 1) .. of the flipped window
                assert same(host(q), np.ascontiguousarray(rgb[H - 16 * (ty + 1):H - 16 * ty, 24 * tx:24 * (tx + 1)])), (tx, ty)
                tot += sq["rays"]
        assert tot == st["rays"]
        # depth 0: every hit is a black sample, every miss the environment
        exp0, info0, _ = tile_expected(acc, o, cam, x0, y0, W, H, ps, la.WhittedParams(1e-7, 1.33, 0))
        rgb0, st0 = acc.render_whitted_tile(cam, x0, y0, W, H, ps, la.WhittedParams(1e-7, 1.33, 0))
        assert same(host(rgb0), exp0) and st0 == {"paths": S, "rays": S, "max_depth_reached": 0}
    finally:
        acc.close()


def test_the_empty_scene_renders_the_environment():
    import torch
    empty = la.HipAccel(0); empty.commit()
    try:
        empty.set_environment(RGB, sky())
        cam = la.Camera.make(40, 24, 1.0, [1.0 if k % 5 == 0 else 0.0 for k in range(16)], 1)
        rgb, st = empty.render_whitted_tile(cam, 3, 2, 33, 17, 2)
        org, dr = empty.primary_rays(cam, 3, 2, 33, 17, 2); torch.cuda.synchronize()
        per = colours(empty, host(dr).copy()).astype(np.float64).reshape(33 * 17, 4, 3)
        accum = np.zeros((33 * 17, 3))
        for s in range(4):
            accum = accum + per[:, s, :]
        exp = np.ascontiguousarray((accum * 0.25).astype(np.float32).reshape(17, 33, 3)[::-1])
        assert same(host(rgb), exp) and st == {"paths": 33 * 17 * 4, "rays": 33 * 17 * 4, "max_depth_reached": 0}
        assert (exp[:, :, 0] != exp[:, :, 1]).any()
    finally:
        empty.close()
