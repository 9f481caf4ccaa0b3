"""The environment-lit gather on the device (lh_accel_env_device / lh_accel_env_host / lh_render_env_tile, and the fetch alone,
lh_accel_environment_device / _host): sky light through the AO stage.

Pinned to the oracle: the gather rays are the AO stage's directions (lh_accel_ao_rays_device: the same by construction) from the origins
P + Ns * eps (tests.test_gpu_dirt.gather_rays), their occlusion is the oracle's any-hit answer (prim != MISS), their colours are
lh_accel_environment_device's on the same directions (itself checked against the numpy restatement of ri_texture_ibl_fetch), and the
value of a hit is lh_env_value restated in numpy: fp64, r order, np.float32 at the end.  Counts are compared as integers, colours as
uint32 views of the floats."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
from tests.test_gpu_ao import load_case
from tests.test_gpu_ao_batch import NO_HIT, POISON32, POISONF, ao, dev, host
from tests.test_gpu_dirt import gather_rays, oracle_t, same_bits
from tests.test_gpu_pt import ibl_fetch_numpy

pytestmark = pytest.mark.gpu

INV_PI = 0.3183098861837907
RGB = (1.0, 0.5, 2.0)


def sky():
    """the seeded 32 x 48 light probe of tests/test_gpu_pt.py::test_ibl_lookup_on_a_miss"""
    return np.random.default_rng(3).uniform(0.1, 2.0, (32, 48, 4)).astype(np.float32)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def values(occ, rad, N, scale):
    """per hit slot: (count uint32, value float32 [3]) -- sum_k = sum_k + rad_r[k] over the rays that are not occluded, r ascending,
    then (scale * sum_k) / N in fp64, stored as float"""
    occ = occ.reshape(-1, N).astype(bool); rad = rad.reshape(-1, N, 3).astype(np.float64)
    s = np.zeros((occ.shape[0], 3))
    for r in range(N):
        s = np.where(occ[:, r, None], s, s + rad[:, r, :])
    return occ.sum(axis=1).astype(np.uint32), ((scale * s) / float(N)).astype(np.float32)


def scatter(slot_of_ray, cnt, val):
    """per-slot answers -> the per-ray outputs (a miss: NO_HIT, three 0.0f)"""
    n = slot_of_ray.shape[0]
    hit = slot_of_ray != NO_HIT
    c = np.full(n, NO_HIT, np.uint32); c[hit] = cnt[slot_of_ray[hit]]
    out = np.zeros((n, 3), np.float32); out[hit] = val[slot_of_ray[hit]]
    return c, out


def poison(n):
    import torch
    return (torch.full((n,), POISON32, dtype=torch.int32, device="cuda"), torch.full((n, 3), POISONF, dtype=torch.float32, device="cuda"))


def env(acc, o, d, rec, ns, params, fused=1, **kw):
    """env_device with "ao_fused" set for the call -> (count uint32 [n], rgb float32 [n, 3]) on the host"""
    acc.set_param("ao_fused", fused)
    try:
        c, v = acc.env_device(o, d, rec, ns, params, **kw)
    finally:
        acc.set_param("ao_fused", 1)
    return host(c, np.uint32).copy(), host(v).copy()


def colours(acc, gd):
    """environment_device on the gather rays' directions, on the host"""
    import torch
    if gd.shape[0] == 0:
        return np.zeros((0, 3), np.float32)
    c = acc.environment_device(dev(gd)); torch.cuda.synchronize()
    return host(c).copy()


@pytest.fixture(scope="module")
def soup():
    """po.soup(3000, 5000, 0.05, 7), committed, with the closest-hit records of its rays and the seeded sky as its environment"""
    import torch
    n = 5000
    P, idx, org, dr = po.soup(3000, n, 0.05, 7)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    acc.set_environment(RGB, sky())
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    to, td = dev(org), dev(dr)
    rec = acc.intersect_device(to, td); torch.cuda.synchronize()
    return {"acc": acc, "oracle": o, "P": P, "idx": idx, "org": to, "dr": td, "rec": rec, "prim": host(rec[0], np.uint32).copy(), "n": n, "gather": {}}


def soup_gather(soup, ns, eps):
    """the gather rays of the whole soup batch, the oracle's any-hit answers and the sky's colours for them, computed once per (ns, eps)"""
    k = (ns, eps)
    if k not in soup["gather"]:
        slot, nslots, go, gd = gather_rays(soup["acc"], soup["org"], soup["dr"], soup["rec"], ns, eps, seed=3)
        _, occ = oracle_t(soup["oracle"], go, gd)
        rad = colours(soup["acc"], gd)
        occ.setflags(write=False); rad.setflags(write=False); gd.setflags(write=False)
        soup["gather"][k] = (slot, nslots, occ, rad, gd)
    return soup["gather"][k]


# ---- 1. the fetch alone -------------------------------------------------------------------------------------------------------
def test_the_fetch_alone(soup):
    """Constant environment: rgb exactly.  The seeded map: ri_texture_ibl_fetch restated in numpy, times rgb.  Device and host libm
    differ by a few ulp in acos and the normalisation; the bilinear fetch is Lipschitz in (u, v) with constant (W - 1) + (H - 1) times the
    largest neighbour difference (1.9): (47 + 31) * 1.9 ~ 150, and away from the poles (|dz| <= 0.999) u and v move by less than 1e-12,
    so the doubles differ by less than 1.5e-10; the two float roundings (the sum, the product with rgb) add 2^-23 relative.  Hence
    |got - exp| <= 2^-22 |exp| + 1e-9"""
    import torch
    rng = np.random.default_rng(11)
    d = rng.normal(size=(40000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.ascontiguousarray(d[np.abs(d[:, 2]) <= 0.999][:20000])
    assert d.shape[0] == 20000
    d *= rng.uniform(0.5, 3.0, (20000, 1))                  # the direction need not be a unit vector
    acc = la.HipAccel(0); acc.add_mesh(soup["P"], soup["idx"]); acc.commit()
    try:
        got = host(acc.environment_device(dev(d)))          # none set: constant white
        assert (got == 1.0).all()
        acc.set_environment((0.25, 3.0, 0.0))
        got = host(acc.environment_device(dev(d)))
        assert np.array_equal(got, np.tile(np.float32([0.25, 3.0, 0.0]), (20000, 1)))
        m = sky()
        acc.set_environment(RGB, m)
        out = acc.environment_device(dev(d)); torch.cuda.synchronize()
        got = host(out).copy()
        exp = ibl_fetch_numpy(m.astype(np.float64), d).astype(np.float32) * np.float32(RGB)
        err = np.abs(got.astype(np.float64) - exp.astype(np.float64))
        bound = 2.0 ** -22 * np.abs(exp.astype(np.float64)) + 1e-9
        print("fetch: largest |got - exp| %.3g, largest excess over the bound %.3g, %d of %d bit-equal" % (err.max(), (err - bound).max(), int((got == exp).sum()), got.size))
        assert (err <= bound).all(), float((err - bound).max())
        assert same_bits(acc.environment_host(d), got)
        # a zero or non-finite direction: an unspecified colour, a finite one (every texel is), nothing faults
        odd = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [np.inf, 1.0, 0.0], [0.0, -np.inf, 0.0], [1e-320, 0.0, 0.0], [1e308, 1e308, 1e308]])
        g = host(acc.environment_device(dev(odd)))
        assert np.isfinite(g).all() and (g >= 0.0).all() and (g <= 4.0).all()
    finally:
        acc.close()


# ---- 2. oracle pin on the soup ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("ns", [1, 5, 16, 25, 100])
def test_oracle_pin_on_the_soup(soup, ns, eps):
    acc = soup["acc"]; N = int(np.sqrt(ns)) ** 2
    slot, nslots, occ, rad, _ = soup_gather(soup, ns, eps)
    share = float(occ.mean()); per = occ.reshape(-1, N).sum(axis=1)
    print("N %d eps %g: %d hits, occluded share %.3f, slots fully occluded %d, fully open %d" % (N, eps, nslots, share, int((per == N).sum()), int((per == 0).sum())))
    assert nslots == 2730 and 0.2 <= share <= 0.8
    if N <= 16:                                           # (of 100 rays some are nearly always open and some occluded)
        assert (per == N).any() and (per == 0).any()      # the occluded-all and open-all paths
    miss = soup["prim"] == po.MISS
    for scale in (1.0, INV_PI):
        cnt, val = values(occ, rad, N, scale)
        ecnt, eval_ = scatter(slot, cnt, val)
        for fused in (1, 0):
            c, v = env(acc, soup["org"], soup["dr"], soup["rec"], ns, la.EnvParams(eps, scale), fused, seed=3)
            print("scale %g fused %d: counts differ at %d, colours at %d of %d" % (scale, fused, int((c != ecnt).sum()), int((v.view(np.uint32) != eval_.view(np.uint32)).sum()), v.size))
            assert np.array_equal(c, ecnt), (scale, fused, int((c != ecnt).sum()))
            assert same_bits(v, eval_), (scale, fused)
            assert (c[miss] == NO_HIT).all() and (v[miss] == 0.0).all()


# ---- 3. the AO stage when the sky is white ------------------------------------------------------------------------------------
def test_it_is_the_ao_stage_when_the_sky_is_white(soup):
    acc = soup["acc"]; ns = N = 16
    occ, radiance = ao(acc, soup["org"], soup["dr"], soup["rec"], ns, 1, seed=3)
    acc.reset_environment()
    try:
        for fused in (1, 0):
            c, v = env(acc, soup["org"], soup["dr"], soup["rec"], ns, la.EnvParams(1e-6, 1.0), fused, seed=3)
            assert np.array_equal(c, occ), fused
            for k in range(3):
                assert same_bits(v[:, k], radiance), (fused, k)
            hit = c != NO_HIT
            assert same_bits(v[hit, 0], ((1.0 * (N - c[hit].astype(np.float64))) / N).astype(np.float32))
    finally:
        acc.set_environment(RGB, sky())


# ---- 4. compaction and lane boundaries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_compaction_and_lane_boundaries(soup, n):
    """the first n rays of the soup (the first gather rays of its hits are the batch's: slots number the hits in ray order)"""
    acc = soup["acc"]; ns = N = 16; eps = 1e-5
    slot, _, occ, rad, _ = soup_gather(soup, ns, eps)
    m = int((slot[:n] != NO_HIT).sum())
    cnt, val = values(occ[:m * N], rad[:m * N], N, INV_PI)
    ecnt, eval_ = scatter(slot[:n], cnt, val)
    org, dr = soup["org"][:n].contiguous(), soup["dr"][:n].contiguous()
    rec = tuple(x[:n].contiguous() for x in soup["rec"])
    cf, vf = env(acc, org, dr, rec, ns, la.EnvParams(eps, INV_PI), 1, seed=3)
    cm, vm = env(acc, org, dr, rec, ns, la.EnvParams(eps, INV_PI), 0, seed=3)
    assert np.array_equal(cf, cm) and same_bits(vf, vm)
    assert np.array_equal(cf, ecnt) and same_bits(vf, eval_)


# ---- 5. lists -------------------------------------------------------------------------------------------------------------------
def test_lists_write_the_listed_slots_alone(soup):
    import torch
    acc = soup["acc"]; n = soup["n"]; NS = 16
    org, dr, rec = soup["org"], soup["dr"], soup["rec"]
    hit = soup["prim"] != po.MISS
    p = la.EnvParams(1e-5, 1.0)
    full_c, full_v = env(acc, org, dr, rec, NS, p, 1, seed=3)

    def check(index, count, listed, fused):
        out = poison(n)
        cnt, v = env(acc, org, dr, rec, NS, p, fused, seed=3, index=index, count=count, out=out)
        assert np.array_equal(cnt[listed], full_c[listed]) and same_bits(v[listed], full_v[listed])
        assert (cnt[~listed] == POISON32).all() and (v[~listed] == np.float32(POISONF)).all()          # 12 bytes per ray of d_rgb

    idx, cnt = la.compact(rec[0], la.SELECT_HIT)                      # the hits, count on the device
    for fused in (1, 0):
        check(idx, cnt, hit, fused)
    rng = np.random.default_rng(5)
    lst = rng.permutation(n)[:1500].astype(np.uint32)
    lst[7] = lst[3]; lst[11] = n + 9; lst[12] = 0xFFFFFFF0            # a duplicate id, two ids >= n
    listed = np.zeros(n, bool); listed[lst[lst < n]] = True
    for fused in (1, 0):
        check(dev(lst), None, listed, fused)
    part = np.zeros(n, bool); part[lst[:100][lst[:100] < n]] = True   # the count cuts the list
    check(dev(lst), torch.tensor([100], dtype=torch.int32, device="cuda"), part, 1)
    check(None, torch.tensor([77], dtype=torch.int32, device="cuda"), np.arange(n) < 77, 1)      # identity list with a count
    for fused in (1, 0):                                              # count = 0 on the device: nothing is written
        check(dev(lst), torch.zeros(1, dtype=torch.int32, device="cuda"), np.zeros(n, bool), fused)


# ---- 6. rays that the persistent walk does not finish ---------------------------------------------------------------------------
def test_small_visit_budgets_go_through_the_cooperative_walk(soup):
    """tiny "ray_budget"s send most gather rays through the fix-up queue to the cooperative walk, which stores the same byte: the answer
    does not depend on the budget, and with statistics on the queue's traffic shows (lh_accel_last_retraced)"""
    acc = soup["acc"]; ns = N = 16; eps = 1e-5
    slot, nslots, occ, rad, _ = soup_gather(soup, ns, eps)
    cnt, val = values(occ, rad, N, 1.0)
    ecnt, eval_ = scatter(slot, cnt, val)
    p = la.EnvParams(eps, 1.0)
    try:
        for budget in (2, 9, 40):
            acc.set_param("ray_budget", budget)
            c, v = env(acc, soup["org"], soup["dr"], soup["rec"], ns, p, 1, seed=3)
            assert np.array_equal(c, ecnt) and same_bits(v, eval_), budget
        acc.set_param("ray_budget", 2)
        acc.trace_statistics(True)
        acc.statistics(clear=True)
        c, v = env(acc, soup["org"], soup["dr"], soup["rec"], ns, p, 1, seed=3)
        s = acc.statistics(clear=True)
        queued = int(acc.L.lh_accel_last_retraced(acc.h))
        print("budget 2: %d of %d gather rays through the queue" % (queued, s["rays"]))
        assert np.array_equal(c, ecnt) and same_bits(v, eval_)
        assert s["rays"] == nslots * N and 0 < queued <= s["rays"]
        assert s["hits"] == int(ecnt[ecnt != NO_HIT].sum())          # counters[4]: the occluded rays
    finally:
        acc.trace_statistics(False)
        acc.set_param("ray_budget", 128)


def test_queue_overflow_answers_as_the_materialised_stage():
    """the frame whose fused AO stage overflows its fix-up queue at "ray_budget" 1 (tests.helpers.ao_overflow_case): the gather answers
    at budget 1 as at budget 256 and as the materialised stage, bit for bit"""
    from tests.helpers import ao_overflow_case
    import torch
    acc, cam = ao_overflow_case()
    acc.set_environment(RGB, sky())
    p = la.EnvParams(1e-5, INV_PI)
    W, H, NS, N = cam.width, cam.height, 16, 16
    try:
        org, dr = acc.primary_rays(cam, 0, 0, W, H, 2)
        rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
        n = org.shape[0]
        miss = host(rec[0], np.uint32) == po.MISS
        assert n == W * H * 4 and 0 < int(miss.sum()) < n
        acc.set_param("ray_budget", 256)
        ref_c, ref_v = env(acc, org, dr, rec, NS, p, 1, seed=5, out=poison(n))
        assert (ref_c[miss] == NO_HIT).all() and (ref_v[miss] == 0.0).all() and (ref_c[~miss] <= N).all()
        assert 0 < int(ref_c[~miss].sum()) < int((~miss).sum()) * N and (ref_v[~miss] > 0.0).any()
        acc.set_param("ray_budget", 1)
        for fused in (1, 0):
            cnt, v = env(acc, org, dr, rec, NS, p, fused, seed=5, out=poison(n))
            assert np.array_equal(cnt, ref_c), (fused, int((cnt != ref_c).sum()))
            assert same_bits(v, ref_v), fused
    finally:
        acc.set_param("ray_budget", 128); acc.set_param("ao_fused", 1)
        acc.close()


# ---- 7. replay with caller uniforms ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1():
    case = load_case("ao_c1")
    case["acc"].set_environment(RGB, sky())
    return case


def test_replay_with_caller_uniforms(c1):
    import torch
    acc, cam, o = c1["acc"], c1["cam"], c1["oracle"]
    W = H = 256; N = NS = 16
    p = la.EnvParams(1e-5, INV_PI)
    order = np.zeros(2 * 64, np.uint32)
    nb = po.lib().lo_bucket_order(W, H, 32, order.ctypes.data_as(po.C.POINTER(po.C.c_uint)))
    mt = np.empty(2 * N * 1024 + 64); po.lib().lo_mt_stream(4357, mt.size, mt.ctypes.data_as(po._dp))
    uni_h = mt[:2 * N * 1024].copy(); uni = dev(uni_h)
    org = dr = rec = None
    for b in range(nb):                                   # the first 32 x 32 bucket of the reference's order that hits anything
        bx, by = int(order[2 * b]) * 32, int(order[2 * b + 1]) * 32
        org, dr = acc.primary_rays(cam, bx, by, 32, 32, 1)
        rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
        if (host(rec[0], np.uint32) != po.MISS).any():
            break
    slot, nslots, go, gd = gather_rays(acc, org, dr, rec, NS, p.eps, uniforms=uni)
    assert nslots > 0
    _, occ = oracle_t(o, go, gd)
    cnt, val = values(occ, colours(acc, gd), N, p.scale)
    ecnt, eval_ = scatter(slot, cnt, val)
    assert 0 < int(cnt.sum()) < nslots * N and (val > 0.0).any()
    c, v = env(acc, org, dr, rec, NS, p, 1, uniforms=uni)
    assert np.array_equal(c, ecnt) and same_bits(v, eval_)
    used = uni.clone(); used[2 * N * nslots:] = 0.5       # 2 * N * hits uniforms are consumed: the rest does not matter
    c, v = env(acc, org, dr, rec, NS, p, 1, uniforms=used)
    assert np.array_equal(c, ecnt) and same_bits(v, eval_)
    hrec = (host(rec[0], np.uint32), host(rec[1]), host(rec[2]), host(rec[3]))
    hc, hv = acc.env_host(host(org), host(dr), hrec, NS, p, uniforms=uni_h)
    assert np.array_equal(hc, ecnt) and same_bits(hv, eval_)
    hc, hv = acc.env_host(host(org), host(dr), hrec, NS, p, seed=9)          # and the built-in generator through the host form
    dc, dv = env(acc, org, dr, rec, NS, p, 1, seed=9)
    assert np.array_equal(hc, dc) and same_bits(hv, dv)


# ---- 8. the tile ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("textured", [False, True])
@pytest.mark.parametrize("pxs", [1, 2])
def test_tile_equals_the_composition_and_does_not_depend_on_tiling(c1, pxs, textured):
    """lh_render_env_tile == lh_render_primary_rays -> lh_accel_intersect_device -> lh_accel_env_device with key = absolute sample
    position -> per sample the hit's three floats, times the texture of its mesh where it has one, accumulated over the pixel's
    sub-samples and written as k_ao_resolve does"""
    import torch
    acc, cam = c1["acc"], c1["cam"]
    p = la.EnvParams(1e-5, INV_PI)
    T, NS, N = 64, 16, 16
    x0, y0 = (cam.width - T) // 2, (cam.height - T) // 2
    spp = pxs * pxs
    if textured:
        acc.set_texture(0, np.random.default_rng(8).uniform(0.2, 1.5, (5, 7, 4)).astype(np.float32))
    try:
        for fused in (1, 0):
            acc.set_param("ao_fused", fused)
            rgb, st = acc.render_env_tile(cam, x0, y0, T, T, pxs, NS, p, seed=5)
            rgb = host(rgb).copy()
            acc.set_param("ao_fused", 1)
            org, dr = acc.primary_rays(cam, x0, y0, T, T, pxs)
            rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
            i = np.arange(T * T * spp, dtype=np.int64)
            ipix = i // spp
            key = dev(((y0 + ipix // T) * cam.width + (x0 + ipix % T)) * spp + (i - ipix * spp))
            cnt, v = env(acc, org, dr, rec, NS, p, 1, seed=5, key=key)
            hit = cnt != NO_HIT
            nslots = int(hit.sum())
            assert 0 < nslots == st["primary_hits"] and st["primary_rays"] == T * T * spp and st["ao_rays"] == nslots * N
            assert st["ao_occluded"] == int(cnt[hit].sum()) > 0
            per = v.astype(np.float64)
            tex = host(acc.texture_device(rec))[:, :3]
            assert ((tex[hit] != 1.0).any(axis=1)).any() == textured
            per = np.where(hit[:, None], per * tex, 0.0) if textured else per
            per = per.reshape(T * T, spp, 3)
            accum = np.zeros((T * T, 3))
            for s in range(spp):
                accum = accum + per[:, s, :]
            exp = np.maximum((accum * (1.0 / spp)).astype(np.float32), np.float32(0.0)).reshape(T, T, 3)[::-1]
            assert same_bits(rgb, exp), (fused, int((rgb != exp).sum()))
            assert (rgb > 0.0).any() and (rgb[:, :, 0] != rgb[:, :, 1]).any()
        # the same frame region as four 32 x 32 tiles
        tot = {k: 0 for k in st}
        for ty in (0, 1):
            for tx in (0, 1):
                q, sq = acc.render_env_tile(cam, x0 + 32 * tx, y0 + 32 * ty, 32, 32, pxs, NS, p, seed=5)
                # image orientation: the tile at frame lines y0 + 32 ty .. is rows T - 32 (ty + 1) .. of the flipped 64-line tile
                assert same_bits(host(q), rgb[T - 32 * (ty + 1):T - 32 * ty, 32 * tx:32 * (tx + 1)]), (tx, ty)
                for k in tot:
                    tot[k] += sq[k]
        assert tot == st
    finally:
        acc.set_param("ao_fused", 1)
        if textured:
            acc.set_texture(0, None)


def test_tile_leaves_the_ao_tile_scratch_alone(c1):
    from tests.helpers import scratch_count
    acc, cam = c1["acc"], c1["cam"]
    x0, y0 = (cam.width - 64) // 2, (cam.height - 64) // 2
    acc.set_param("ao_fused", 0)
    try:
        _, st = acc.render_ao_tile(cam, x0, y0, 64, 64, 1, 16, seed=5)
        before = [acc.scratch(k, dt, w) for k, dt, w in ((0, np.float64, 3), (6, np.uint32, 1), (8, np.float64, 3), (10, np.uint8, 1))]
        acc.render_env_tile(cam, 0, 0, 48, 40, 2, 4, la.EnvParams(), seed=9)          # materialised: the AO stage's path, scratch of its own
        acc.set_param("ao_fused", 1)
        acc.render_env_tile(cam, 0, 0, 48, 40, 2, 4, la.EnvParams(), seed=9)
    finally:
        acc.set_param("ao_fused", 1)
    after = [acc.scratch(k, dt, w) for k, dt, w in ((0, np.float64, 3), (6, np.uint32, 1), (8, np.float64, 3), (10, np.uint8, 1))]
    assert scratch_count(acc, 8) == st["primary_hits"] * 16 > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- 9. edges -------------------------------------------------------------------------------------------------------------------
def test_device_mesh_accelerator_empty_scene_and_a_changed_environment(soup):
    import torch
    n = 4000; NS = N = 16
    p = la.EnvParams(1e-5, 1.0)
    org, dr = soup["org"][:n].contiguous(), soup["dr"][:n].contiguous()
    rec = tuple(x[:n].contiguous() for x in soup["rec"])
    ref_c, ref_v = env(soup["acc"], org, dr, rec, NS, p, 1, seed=3)
    assert ((ref_c != NO_HIT) & (ref_c > 0)).any()
    dm = la.HipAccel(0)
    dm.add_mesh_device(dev(soup["P"]), dev(soup["idx"])); dm.commit(); dm.wait_exact()
    dm.set_environment(RGB, sky())
    rec_d = dm.intersect_device(org, dr); torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(rec_d, rec))
    for fused in (1, 0):
        c, v = env(dm, org, dr, rec_d, NS, p, fused, seed=3)
        assert np.array_equal(c, ref_c) and same_bits(v, ref_v)
    # set_environment between two calls changes the second call only
    slot, _, occ, _, gd = soup_gather(soup, NS, 1e-5)
    m = int((slot[:n] != NO_HIT).sum())
    other = np.random.default_rng(21).uniform(0.0, 3.0, (9, 17, 4)).astype(np.float32)
    dm.set_environment((2.0, 1.0, 0.5), other)
    first_c, first_v = c.copy(), v.copy()
    c2, v2 = env(dm, org, dr, rec_d, NS, p, 1, seed=3)
    cnt, val = values(occ[:m * N], colours(dm, gd[:m * N].copy()), N, 1.0)
    e2 = scatter(slot[:n], cnt, val)
    assert np.array_equal(c2, e2[0]) and same_bits(v2, e2[1]) and not same_bits(v2, ref_v)
    assert np.array_equal(first_c, ref_c) and same_bits(first_v, ref_v)
    dm.close()
    empty = la.HipAccel(0); empty.commit()
    c, v = env(empty, org, dr, rec, NS, p, 1, out=poison(n))          # whatever the records say: nothing is there to hit
    assert (c == NO_HIT).all() and (v == 0.0).all()
    cam = la.Camera.make(32, 32, 1.0, [1.0 if k % 5 == 0 else 0.0 for k in range(16)], 1)
    rgb, st = empty.render_env_tile(cam, 0, 0, 32, 32, 1, NS, p)
    assert (host(rgb) == 0.0).all() and st["primary_hits"] == 0 and st["ao_rays"] == 0 and st["ao_occluded"] == 0
    empty.close()


def test_refusals_leave_the_outputs_untouched(soup):
    import torch
    acc, L = soup["acc"], binding.lib()
    n = 64
    org, dr = soup["org"][:n].contiguous(), soup["dr"][:n].contiguous()
    prim, t, u, v = (x[:n].contiguous() for x in soup["rec"])
    cnt, val = poison(n)
    key = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    O, D, P, T, U, V = (x.data_ptr() for x in (org, dr, prim, t, u, v))
    CN, R, K, I = cnt.data_ptr(), val.data_ptr(), key.data_ptr(), idx.data_ptr()
    raw = la.HipAccel(0)                                                # never committed
    bad = [la.EnvParams(float("nan"), 1.0), la.EnvParams(1e-5, float("nan")), la.EnvParams(-1e-300, 1.0), la.EnvParams(1e-5, -1.0),
           la.EnvParams(float("inf"), 1.0), la.EnvParams(1e-5, float("inf"))]
    cases = [(acc.h, (n, O, D, P, T, U, V, 16, C.byref(b), 1, None, None, None, 0, None, CN, R, None), "bad environment-gather parameters") for b in bad] + [
        (raw.h, (n, O, D, P, T, U, V, 16, None, 1, None, None, None, 0, None, CN, R, None), "not committed"),
        (acc.h, (n, None, D, P, T, U, V, 16, None, 1, None, None, None, 0, None, CN, R, None), "NULL"),
        (acc.h, (n, O, D, P, None, U, V, 16, None, 1, None, None, None, 0, None, CN, R, None), "NULL"),
        (acc.h, (n, O, D, P, T, U, V, 0, None, 1, None, None, None, 0, None, CN, R, None), "gather_nsamples"),
        (acc.h, (1 << 31, O, D, P, T, U, V, 16, None, 1, None, None, None, 0, None, CN, R, None), "2^31"),
        (acc.h, (n, O, D, P, T, U, V, 16, None, 1, None, None, None, (1 << 30) + 1, None, CN, R, None), "2^30"),
        (acc.h, (n, O, D, P, T, U, V, 16, None, 1, None, None, I + 2, 8, None, CN, R, None), "4-byte aligned"),
        (acc.h, (n, O, D, P, T, U, V, 16, None, 1, None, None, I, 8, I + 1, CN, R, None), "4-byte aligned"),
        (acc.h, (n, O, D, P, T, U, V, 16, None, 1, K + 4, None, None, 0, None, CN, R, None), "8-byte aligned"),
        (acc.h, (n, O, D, P, T, U, V, 16, None, 1, None, None, None, 0, None, CN + 2, R, None), "4-byte aligned"),
        (acc.h, (n, O, D, P, T, U, V, 16, None, 1, None, None, None, 0, None, CN, R + 2, None), "4-byte aligned"),
        (acc.h, (n, O, D, P, T, U, V, 16, None, 1, None, None, None, 0, None, None, None, None), "both outputs"),
    ]
    for h, args, msg in cases:
        rc = L.lh_accel_env_device(h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_env_device" in err, (args, err)
    hc = np.full(n, POISON32, np.uint32); hv = np.full((n, 3), POISONF, np.float32); z = np.zeros((n, 3)); zp = np.zeros(n, np.uint32); zt = np.zeros(n)
    Z, ZP, ZT = z.ctypes.data, zp.ctypes.data, zt.ctypes.data
    for h, args, msg in [
            (raw.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, None, 1, None, None, 0, hc.ctypes.data, hv.ctypes.data), "not committed"),
            (acc.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, C.byref(bad[0]), 1, None, None, 0, hc.ctypes.data, hv.ctypes.data), "bad environment-gather parameters"),
            (acc.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, None, 1, None, ZT, n, hc.ctypes.data, hv.ctypes.data), "uniforms"),
            (acc.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, None, 1, None, None, 0, None, None), "both outputs")]:
        rc = L.lh_accel_env_host(h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_env_host" in err, (args, err)
    cam = la.Camera.make(32, 32, 1.0, [1.0 if k % 5 == 0 else 0.0 for k in range(16)], 1)
    rgb = torch.full((8, 8, 3), POISONF, dtype=torch.float32, device="cuda"); st = binding.TileStats()
    for h, args, msg in [
            (raw.h, (C.byref(cam), 0, 0, 8, 8, 1, 16, None, 1, None, rgb.data_ptr(), C.byref(st), None), "not committed"),
            (acc.h, (C.byref(cam), 0, 0, 8, 8, 1, 16, C.byref(bad[1]), 1, None, rgb.data_ptr(), C.byref(st), None), "bad environment-gather parameters"),
            (acc.h, (C.byref(cam), 0, 0, 8, 8, 1, 16, None, 1, None, None, C.byref(st), None), "NULL"),
            (acc.h, (C.byref(cam), 0, 0, 0, 8, 1, 16, None, 1, None, rgb.data_ptr(), C.byref(st), None), "bad tile"),
            (acc.h, (C.byref(cam), 0, 0, 8, 8, 1, 0, None, 1, None, rgb.data_ptr(), C.byref(st), None), "bad tile")]:
        rc = L.lh_render_env_tile(h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_render_env_tile" in err, (args, err)
    for h, args, msg in [(raw.h, (n, D, R, None), "not committed"), (acc.h, (n, None, R, None), "NULL"), (acc.h, (n, D, None, None), "NULL"),
                         (acc.h, (n, D + 4, R, None), "8-byte aligned"), (acc.h, (n, D, R + 2, None), "4-byte aligned")]:
        rc = L.lh_accel_environment_device(h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_environment_device" in err, (args, err)
    torch.cuda.synchronize()
    assert (host(cnt) == POISON32).all() and (host(val) == np.float32(POISONF)).all() and (host(rgb) == np.float32(POISONF)).all()
    assert (hc == POISON32).all() and (hv == np.float32(POISONF)).all()
    # zero rays / directions: 0, no array looked at
    assert L.lh_accel_env_device(acc.h, 0, None, None, None, None, None, None, 16, None, 1, None, None, None, 0, None, None, None, None) == 0
    assert L.lh_accel_environment_device(acc.h, 0, None, None, None) == 0 and L.lh_accel_environment_host(acc.h, 0, None, None) == 0
    # the binding refuses what is not an EnvParams, and wrong dtypes and shapes, before it calls C
    rec = (prim, t, u, v)
    for wrong in (lambda: acc.env_device(org, dr, rec, 16, (1e-5, 1.0)), lambda: acc.env_device(org.float(), dr, rec, 16),
                  lambda: acc.env_device(org, dr, rec, 16, out=(cnt, val[:, 0].contiguous())), lambda: acc.env_host(z, z, (zp, zt, zt, zt), 16, 0.5),
                  lambda: acc.environment_device(org.float())):
        with pytest.raises(ValueError):
            wrong()
    raw.close()
