"""The sun-and-sky light of the environment-lit gather on the device (lh_accel_set_sky; lh_accel_sky_device / _host; lh_accel_env_device /
_host and lh_render_env_tile while a sky is set): the Preetham sky as the radiance of an open gather ray, the sun's shadow ray per hit.

The scene is tests/test_gpu_envgather.py's: po.soup(3000, 5000, 0.05, 7), its 2 730 hits, seed 3.  The skies are the four of
tests/golden/sky_reference.npz (what the compiled reference answered), built here by Sky.from_site with the fixture's basis floats and
sun colours; the gather runs under the first, the reference's default site, whose sun lights about a fifth of the hits and stands
behind about half of them.

Pinned to the oracle: the gather rays' occlusion is the oracle's any-hit answer, the sun's is the oracle's plain any-hit answer from the
same origin along sun_dir, the colours are lh_accel_sky_device's on the gather directions (itself held to the reference within the bound
of tests/test_sky_rule.py), and a hit's value is lh_env_value plus the sun's term restated in numpy: fp64, r order, the sun last,
np.float32 at the end.  Counts are compared as integers, colours as uint32 views of the floats."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests.test_gpu_ao import load_case
from tests.test_gpu_ao_batch import NO_HIT, POISON32, POISONF, dev, host
from tests.test_gpu_dirt import gather_rays, oracle_t, same_bits
from tests.test_gpu_envgather import INV_PI, RGB, env, poison, scatter, sky as probe
from tests.test_sky_rule import BOUND, GOLDEN, NSKY, sky_error

pytestmark = pytest.mark.gpu

EPS = 1e-5


def make_sky(g, k, flags):
    s = g["site%d" % k]
    return la.Sky.from_site(s[0], s[1], s[2], int(s[3]), s[4], s[5], basis_rgb=g["basis_rgb"], basis_y=g["basis_y"], sun_rgb=g["sun_rgb%d" % k], flags=flags)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def values(occ, rad, N, scale, sun_occ=None, sun_rgb=None):
    """per hit slot: (count uint32, value float32 [3]) -- sum_k = sum_k + rad_r[k] over the rays that are not occluded, r ascending; then,
    with a sun, sum_k = sum_k + sun_rgb[k] where its ray is not occluded; then (scale * sum_k) / N in fp64, stored as float"""
    occ = occ.reshape(-1, N).astype(bool); rad = rad.reshape(-1, N, 3).astype(np.float64)
    s = np.zeros((occ.shape[0], 3))
    for r in range(N):
        s = np.where(occ[:, r, None], s, s + rad[:, r, :])
    if sun_occ is not None:
        s = np.where(sun_occ.astype(bool)[:, None], s, s + np.asarray(sun_rgb, np.float32).astype(np.float64)[None, :])
    return occ.sum(axis=1).astype(np.uint32), ((scale * s) / float(N)).astype(np.float32)


@pytest.fixture(scope="module")
def sk():
    """the soup, committed, with the closest-hit records of its rays, the seeded light probe as its environment, and -- before any sky was
    ever set -- the environment gather's answers, fused and materialised"""
    import torch
    n = 5000
    P, idx, org, dr = po.soup(3000, n, 0.05, 7)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    acc.set_environment(RGB, probe())
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    to, td = dev(org), dev(dr)
    rec = acc.intersect_device(to, td); torch.cuda.synchronize()
    before = [env(acc, to, td, rec, 16, la.EnvParams(EPS, INV_PI), fused, seed=3) for fused in (1, 0)]
    g = np.load(GOLDEN)
    d = {"acc": acc, "oracle": o, "P": P, "idx": idx, "org": to, "dr": td, "rec": rec, "prim": host(rec[0], np.uint32).copy(), "n": n,
         "before": before, "g": g, "gather": {}}
    yield d
    acc.close()


def sun_answers(sk, sun_dir):
    """by the oracle alone, per hit slot: (the sun's ray from P + eps Ns is occluded, it is blocked by the hit's own primitive, Ns . sun_dir)"""
    if "sun" not in sk:
        acc = sk["acc"]
        st = acc.state_build(host(sk["org"]), host(sk["dr"]), *(host(sk["rec"][0], np.uint32), host(sk["rec"][1]), host(sk["rec"][2]), host(sk["rec"][3])))
        ids = np.nonzero(sk["prim"] != po.MISS)[0]
        org = st[ids, 0:3] + st[ids, 6:9] * EPS
        prim = sk["oracle"].intersect(org, np.tile(np.asarray(sun_dir, np.float64), (ids.shape[0], 1)), nthreads=8)[0]
        sk["sun"] = (prim != po.MISS, prim == sk["prim"][ids], st[ids, 6:9] @ np.asarray(sun_dir, np.float64))
    return sk["sun"]


def sky_gather(sk, ns):
    """the gather rays of the whole batch, the oracle's any-hit answers and (the sky of site 0 being set) sky_device's colours for them"""
    import torch
    if ns not in sk["gather"]:
        acc = sk["acc"]
        slot, nslots, go, gd = gather_rays(acc, sk["org"], sk["dr"], sk["rec"], ns, EPS, seed=3)
        _, occ = oracle_t(sk["oracle"], go, gd)
        rad = host(acc.sky_device(dev(gd))).copy(); torch.cuda.synchronize()
        sk["gather"][ns] = (slot, nslots, occ, rad, gd)
    return sk["gather"][ns]


# ---- 1. the fetch alone -------------------------------------------------------------------------------------------------------
def test_the_fetch_alone(sk):
    """sky_device on the fixture's directions: within the CPU test's bound of the reference's rgb, exactly 0 below the horizon; sky_host
    bit for bit; odd directions return; no sky: refused"""
    import torch
    acc, g = sk["acc"], sk["g"]
    try:
        for k in range(NSKY):
            acc.set_sky(make_sky(g, k, 0))
            d = g["dirs%d" % k].astype(np.float64)
            out = acc.sky_device(dev(d)); torch.cuda.synchronize()
            got = host(out).copy()
            e, dark_ok = sky_error(got, g["rgb%d" % k])
            print("sky %d: largest e on the device %.3g (bound %.3g), %d of %d bit-equal to the reference" % (k, e, BOUND, int((got == g["rgb%d" % k]).sum()), got.size))
            assert dark_ok and e <= BOUND, (k, e)
            assert same_bits(acc.sky_host(d), got), k
        odd = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, np.nan, 0.0], [np.inf, 1.0, 0.0], [0.0, np.inf, 0.0], [0.0, -np.inf, 0.0],
                        [1e308, 1e308, 1e308], [-1e308, 1e308, 0.0], [1e-320, 1e-320, 0.0]])
        out = acc.sky_device(dev(odd)); torch.cuda.synchronize()
        assert host(out).shape == (odd.shape[0], 3)
        assert (host(out)[5] == 0.0).all()                  # below the horizon, whatever its length
        assert acc.sky_host(np.zeros((0, 3))).shape == (0, 3)
    finally:
        acc.reset_sky()
    for call in (lambda: acc.sky_device(dev(np.ones((4, 3)))), lambda: acc.sky_host(np.ones((4, 3)))):
        with pytest.raises(la.LucilleHipError, match="no sky is set"):
            call()
    with pytest.raises(ValueError):
        acc.set_sky(g["sky0"])
    bad = make_sky(g, 0, 2)
    with pytest.raises(la.LucilleHipError, match="bad sky parameters"):
        acc.set_sky(bad)
    bad = make_sky(g, 0, 1); bad.perez_Y[3] = float("nan")
    with pytest.raises(la.LucilleHipError, match="bad sky parameters"):
        acc.set_sky(bad)


# ---- 2. the scene exercises the sun ---------------------------------------------------------------------------------------------
def test_the_scene_exercises_the_sun(sk):
    """by the oracle alone: the sun lights between a tenth and nine tenths of the 2 730 hits, and at least 50 hits with the sun behind them
    (Ns . sun_dir < 0) have their sun ray blocked by their own primitive -- a self-primitive skip on the sun's ray would change those"""
    s = make_sky(sk["g"], 0, la.SKY_SUN)
    occ, own, ndots = sun_answers(sk, list(s.sun_dir))
    lit = 1.0 - float(occ.mean()); behind_own = int(((ndots < 0) & own).sum())
    print("sun-lit share %.3f of %d slots; %d slots with the sun behind them blocked by their own primitive" % (lit, occ.shape[0], behind_own))
    assert occ.shape[0] == 2730 and 0.1 <= lit <= 0.9 and behind_own >= 50
    assert (own <= occ).all()


# ---- 3. oracle pin of the gather ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun", [0, 1])
@pytest.mark.parametrize("ns", [1, 16, 64])
def test_oracle_pin_of_the_gather(sk, ns, sun):
    acc, g = sk["acc"], sk["g"]; N = int(np.sqrt(ns)) ** 2
    s = make_sky(g, 0, la.SKY_SUN if sun else 0)
    acc.set_sky(s)
    try:
        slot, nslots, occ, rad, _ = sky_gather(sk, ns)
        socc, own, ndots = sun_answers(sk, list(s.sun_dir))
        lit = 1.0 - float(socc.mean())
        assert nslots == 2730 and 0.1 <= lit <= 0.9 and int(((ndots < 0) & own).sum()) >= 50
        assert (rad[occ == 0] >= 0).all() and (rad > 0).any()
        miss = sk["prim"] == po.MISS
        for scale in (1.0, INV_PI):
            cnt, val = values(occ, rad, N, scale, socc if sun else None, list(s.sun_rgb))
            ecnt, eval_ = scatter(slot, cnt, val)
            if sun:                                          # the sun's term shows: without it the values differ
                assert not same_bits(eval_, scatter(slot, *values(occ, rad, N, scale))[1])
            for fused in (1, 0):
                c, v = env(acc, sk["org"], sk["dr"], sk["rec"], ns, la.EnvParams(EPS, scale), fused, seed=3)
                print("N %d sun %d scale %g fused %d: counts differ at %d, colours at %d of %d" % (N, sun, scale, fused, int((c != ecnt).sum()), int((v.view(np.uint32) != eval_.view(np.uint32)).sum()), v.size))
                assert np.array_equal(c, ecnt), (scale, fused, int((c != ecnt).sum()))
                assert same_bits(v, eval_), (scale, fused)
                assert (c[miss] == NO_HIT).all() and (v[miss] == 0.0).all()
        # the host form: the same bytes
        hrec = (host(sk["rec"][0], np.uint32), host(sk["rec"][1]), host(sk["rec"][2]), host(sk["rec"][3]))
        hc, hv = acc.env_host(host(sk["org"]), host(sk["dr"]), hrec, ns, la.EnvParams(EPS, INV_PI), seed=3)
        assert np.array_equal(hc, ecnt) and same_bits(hv, eval_)
    finally:
        acc.reset_sky()


def test_statistics_stay_those_of_the_gather_rays(sk):
    """with trace statistics on, `rays` advances by hits x N and `hits` by the occluded gather rays: the sun's rays are not counted"""
    acc = sk["acc"]; ns = N = 16
    acc.set_sky(make_sky(sk["g"], 0, la.SKY_SUN))
    try:
        slot, nslots, occ, _, _ = sky_gather(sk, ns)
        acc.trace_statistics(True)
        for fused in (1, 0):
            acc.statistics(clear=True)
            env(acc, sk["org"], sk["dr"], sk["rec"], ns, la.EnvParams(EPS, 1.0), fused, seed=3)
            st = acc.statistics(clear=True)
            assert st["rays"] == nslots * N and st["hits"] == int(occ.sum()), (fused, st)
    finally:
        acc.trace_statistics(False)
        acc.reset_sky()


# ---- 4. lists -------------------------------------------------------------------------------------------------------------------
def test_lists_write_the_listed_slots_alone(sk):
    import torch
    acc = sk["acc"]; n = sk["n"]; NS = 16
    org, dr, rec = sk["org"], sk["dr"], sk["rec"]
    p = la.EnvParams(EPS, INV_PI)
    acc.set_sky(make_sky(sk["g"], 0, la.SKY_SUN))
    try:
        full_c, full_v = env(acc, org, dr, rec, NS, p, 1, seed=3)

        def check(index, count, listed, fused):
            out = poison(n)
            cnt, v = env(acc, org, dr, rec, NS, p, fused, seed=3, index=index, count=count, out=out)
            assert np.array_equal(cnt[listed], full_c[listed]) and same_bits(v[listed], full_v[listed])
            assert (cnt[~listed] == POISON32).all() and (v[~listed] == np.float32(POISONF)).all()

        rng = np.random.default_rng(5)
        lst = rng.permutation(n)[:1500].astype(np.uint32)
        lst[7] = lst[3]; lst[11] = n + 9                                  # an id twice, an id >= n
        listed = np.zeros(n, bool); listed[lst[lst < n]] = True
        for fused in (1, 0):
            check(dev(lst), None, listed, fused)
        part = np.zeros(n, bool); part[lst[:100][lst[:100] < n]] = True   # a device count cuts the list
        for fused in (1, 0):
            check(dev(lst), torch.tensor([100], dtype=torch.int32, device="cuda"), part, fused)
        idx, cnt = la.compact(rec[0], la.SELECT_HIT)                      # the hits, count on the device
        check(idx, cnt, sk["prim"] != po.MISS, 1)
        check(dev(lst), torch.zeros(1, dtype=torch.int32, device="cuda"), np.zeros(n, bool), 1)
    finally:
        acc.reset_sky()


# ---- 5. the tile ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1():
    return load_case("ao_c1")


@pytest.mark.parametrize("pxs", [1, 2])
def test_tile_equals_the_batch_values_and_does_not_depend_on_tiling_or_texture(c1, sk, pxs):
    """lh_render_env_tile under a sky == lh_render_primary_rays -> lh_accel_intersect_device -> lh_accel_env_device with key = absolute
    sample position -> per sample the hit's three floats, accumulated over the pixel's sub-samples and written as k_ao_resolve does; no
    texture multiply: with a texture on the mesh the tile is the same"""
    import torch
    acc, cam = c1["acc"], c1["cam"]
    p = la.EnvParams(EPS, INV_PI)
    T, NS, N = 64, 16, 16
    x0, y0 = (cam.width - T) // 2, (cam.height - T) // 2
    spp = pxs * pxs
    s = make_sky(sk["g"], 0, la.SKY_SUN)
    try:
        org, dr = acc.primary_rays(cam, x0, y0, T, T, pxs)
        rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
        i = np.arange(T * T * spp, dtype=np.int64)
        ipix = i // spp
        key = dev(((y0 + ipix // T) * cam.width + (x0 + ipix % T)) * spp + (i - ipix * spp))
        s.flags = 0; acc.set_sky(s)
        cnt, v_nosun = env(acc, org, dr, rec, NS, p, 1, seed=5, key=key)
        hit = cnt != NO_HIT
        nslots = int(hit.sum())
        s.flags = la.SKY_SUN
        for cand in ([0.3, 0.9, 0.316227766], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [-0.6, 0.0, -0.8], [0.8, 0.6, 0.0], [-0.8, 0.6, 0.0]):
            s.sun_dir[:] = cand                                # the first of these suns that lights some of the tile's hits and not others
            acc.set_sky(s)
            c2, v = env(acc, org, dr, rec, NS, p, 1, seed=5, key=key)
            sunlit = (v[hit] != v_nosun[hit]).any(axis=1)
            print("tile: sun %s: %d hits, the sun's term shows at %d" % (cand, nslots, int(sunlit.sum())))
            assert np.array_equal(c2, cnt)
            if 0 < int(sunlit.sum()) < nslots:
                break
        assert 0 < int(sunlit.sum()) < nslots                 # lit and shadowed hits both
        per = v.astype(np.float64).reshape(T * T, spp, 3)
        accum = np.zeros((T * T, 3))
        for q in range(spp):
            accum = accum + per[:, q, :]
        exp = np.maximum((accum * (1.0 / spp)).astype(np.float32), np.float32(0.0)).reshape(T, T, 3)[::-1]
        for fused in (1, 0):
            acc.set_param("ao_fused", fused)
            rgb, st = acc.render_env_tile(cam, x0, y0, T, T, pxs, NS, p, seed=5)
            rgb = host(rgb).copy()
            acc.set_param("ao_fused", 1)
            assert 0 < nslots == st["primary_hits"] and st["primary_rays"] == T * T * spp and st["ao_rays"] == nslots * N
            assert st["ao_occluded"] == int(cnt[hit].sum()) > 0
            assert same_bits(rgb, exp), (fused, int((rgb != exp).sum()))
        assert (rgb > 0.0).any() and (rgb[:, :, 0] != rgb[:, :, 2]).any()
        tot = {k: 0 for k in st}
        for ty in (0, 1):
            for tx in (0, 1):
                q, sq = acc.render_env_tile(cam, x0 + 32 * tx, y0 + 32 * ty, 32, 32, pxs, NS, p, seed=5)
                assert same_bits(host(q), rgb[T - 32 * (ty + 1):T - 32 * ty, 32 * tx:32 * (tx + 1)]), (tx, ty)
                for k in tot:
                    tot[k] += sq[k]
        assert tot == st
        acc.set_texture(0, np.random.default_rng(8).uniform(0.2, 1.5, (5, 7, 4)).astype(np.float32))
        try:
            assert ((host(acc.texture_device(rec))[:, :3][hit] != 1.0).any(axis=1)).any()
            for fused in (1, 0):
                acc.set_param("ao_fused", fused)
                q, sq = acc.render_env_tile(cam, x0, y0, T, T, pxs, NS, p, seed=5)
                assert same_bits(host(q), rgb) and sq == st, fused
        finally:
            acc.set_param("ao_fused", 1)
            acc.set_texture(0, None)
    finally:
        acc.set_param("ao_fused", 1)
        acc.reset_sky()


# ---- 6. no sky ------------------------------------------------------------------------------------------------------------------
def test_removing_the_sky_restores_the_environment_gather(sk):
    """with no sky set the environment gather answers what it answered before set_sky / reset_sky were ever called, bit for bit"""
    acc = sk["acc"]
    p = la.EnvParams(EPS, INV_PI)
    acc.set_sky(make_sky(sk["g"], 0, la.SKY_SUN))
    under = env(acc, sk["org"], sk["dr"], sk["rec"], 16, p, 1, seed=3)
    acc.reset_sky()
    assert np.array_equal(under[0], sk["before"][0][0]) and not same_bits(under[1], sk["before"][0][1])
    for k, fused in enumerate((1, 0)):
        c, v = env(acc, sk["org"], sk["dr"], sk["rec"], 16, p, fused, seed=3)
        assert np.array_equal(c, sk["before"][k][0]) and same_bits(v, sk["before"][k][1]), fused
    assert same_bits(sk["before"][0][1], sk["before"][1][1])
