"""The dirtmap transport on the device (lh_accel_dirt_device / lh_accel_dirt_host / lh_render_dirt_tile): range-limited,
distance-weighted occlusion.

Pinned to the oracle: the gather rays are the AO stage's directions (lh_accel_ao_rays_device: the same by construction) from the
origins P + Ns * eps (lh_accel_state_build_*: doubles 0..2 and 6..8), the oracle's closest-hit t of those rays goes through the rule of
lh_dirt.h restated in numpy, summed in r order.  Counts are compared as integers, values as uint32 views of the floats."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
from tests.test_gpu_ao import load_case
from tests.test_gpu_ao_batch import NO_HIT, POISON32, POISONF, ao, ao_rays, dev, host, poison

pytestmark = pytest.mark.gpu


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def weights(t, hit, near, far):
    """c of every gather ray from the oracle's unbounded closest-hit record (hit, t) -> (bounded hit, c)"""
    bh = hit & (t < far)
    with np.errstate(invalid="ignore", over="ignore"):
        a = t - near; b = far - near; q = a / b; x = 1.0 - q
        p = np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))
        c = 1.0 - p
    c = np.where(t <= near, 0.0, c)
    return bh, np.where(bh, c, 1.0)


def values(t, hit, N, near, far):
    """per hit slot: (near_hits uint32, value float64) -- sum = sum + c_r for r = 0 .. N - 1, then / N"""
    bh, c = weights(t, hit, near, far)
    bh = bh.reshape(-1, N); c = c.reshape(-1, N)
    s = np.zeros(c.shape[0])
    for r in range(N):
        s = s + c[:, r]
    return bh.sum(axis=1).astype(np.uint32), s / float(N)


def scatter(slot_of_ray, nh, val):
    """per-slot answers -> the per-ray outputs (a miss: NO_HIT, 0.0f)"""
    n = slot_of_ray.shape[0]
    hit = slot_of_ray != NO_HIT
    cnt = np.full(n, NO_HIT, np.uint32); cnt[hit] = nh[slot_of_ray[hit]]
    out = np.zeros(n, np.float32); out[hit] = val[slot_of_ray[hit]].astype(np.float32)
    return cnt, out


def dirt(acc, o, d, rec, ns, params, fused=1, **kw):
    """dirt_device with "ao_fused" set for the call -> (near_hits uint32, value float32) on the host"""
    acc.set_param("ao_fused", fused)
    try:
        c, v = acc.dirt_device(o, d, rec, ns, params, **kw)
    finally:
        acc.set_param("ao_fused", 1)
    return host(c, np.uint32).copy(), host(v).copy()


def gather_rays(acc, org, dr, rec, ns, eps, **kw):
    """the dirt stage's gather rays, built outside it: (slot_of_ray, nslots, origins [nslots * N, 3], directions)"""
    slot, nslots, _, adir = ao_rays(acc, org, dr, rec, ns, **kw)
    N = int(np.sqrt(ns)) ** 2
    st = acc.state_build(host(org), host(dr), host(rec[0], np.uint32), host(rec[1]), host(rec[2]), host(rec[3]))
    ids = np.nonzero(slot != NO_HIT)[0]
    assert np.array_equal(slot[ids], np.arange(nslots, dtype=np.uint32))          # hit slots in ray order
    o = st[ids, 0:3] + st[ids, 6:9] * eps
    return slot, nslots, np.repeat(o, N, axis=0), adir


def oracle_t(o, org, dr):
    if org.shape[0] == 0:
        return np.zeros(0), np.zeros(0, bool)
    prim, t, _, _ = o.intersect(org, dr, nthreads=8)
    return t, prim != po.MISS


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def soup():
    """po.soup(3000, 5000, 0.05, 7), committed, with the closest-hit records of its rays"""
    import torch
    n = 5000
    P, idx, org, dr = po.soup(3000, n, 0.05, 7)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    to, td = dev(org), dev(dr)
    rec = acc.intersect_device(to, td); torch.cuda.synchronize()
    return {"acc": acc, "oracle": o, "P": P, "idx": idx, "org": to, "dr": td, "rec": rec, "prim": host(rec[0], np.uint32).copy(), "n": n, "gather": {}}


def soup_gather(soup, ns, eps):
    """the gather rays of the whole soup batch and the oracle's answers for them, computed once per (ns, eps)"""
    k = (ns, eps)
    if k not in soup["gather"]:
        slot, nslots, go, gd = gather_rays(soup["acc"], soup["org"], soup["dr"], soup["rec"], ns, eps, seed=3)
        t, hit = oracle_t(soup["oracle"], go, gd)
        t.setflags(write=False); hit.setflags(write=False)
        soup["gather"][k] = (slot, nslots, t, hit)
    return soup["gather"][k]


# ---- 1. oracle pin on the soup ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("ns", [4, 16])
def test_oracle_pin_on_the_soup(soup, ns, eps):
    acc = soup["acc"]; N = int(np.sqrt(ns)) ** 2
    slot, nslots, t, hit = soup_gather(soup, ns, eps)
    th = t[hit]
    assert th.size >= 1000, th.size
    near, far = float(np.percentile(th, 25)), float(np.percentile(th, 75))
    shares = [float((th <= near).mean()), float(((th > near) & (th < far)).mean()), float((th >= far).mean())]
    print("gather rays that hit: %d of %d; near %.17g far %.17g; shares %s" % (th.size, t.size, near, far, shares))
    assert min(shares) >= 0.10, shares
    nh, val = values(t, hit, N, near, far)
    ecnt, eval_ = scatter(slot, nh, val)
    p = la.DirtParams(near, far, eps)
    for fused in (1, 0):
        cnt, v = dirt(acc, soup["org"], soup["dr"], soup["rec"], ns, p, fused, seed=3)
        print("fused %d: counts differ at %d, values at %d of %d" % (fused, int((cnt != ecnt).sum()), int((v.view(np.uint32) != eval_.view(np.uint32)).sum()), cnt.size))
        assert np.array_equal(cnt, ecnt), (fused, int((cnt != ecnt).sum()))
        assert same_bits(v, eval_), fused
        miss = soup["prim"] == po.MISS
        assert (cnt[miss] == NO_HIT).all() and (v[miss] == 0.0).all()


# ---- 2. edges of the clips ----------------------------------------------------------------------------------------------------
def test_clips_at_the_exact_t_of_two_gather_rays(soup):
    acc = soup["acc"]; ns = N = 16; eps = 1e-5
    slot, nslots, t, hit = soup_gather(soup, ns, eps)
    order = np.argsort(np.where(hit, t, np.inf))
    k = int(hit.sum())
    i_near, i_far = int(order[k // 4]), int(order[(3 * k) // 4])
    near, far = float(t[i_near]), float(t[i_far])
    assert 0.0 < near < far
    bh, c = weights(t, hit, near, far)
    assert c[i_near] == 0.0 and bh[i_near]            # at the near clip: weight 0, still a bounded hit
    assert c[i_far] == 1.0 and not bh[i_far]          # at the far clip: a miss
    nh, val = values(t, hit, N, near, far)
    ecnt, eval_ = scatter(slot, nh, val)
    for fused in (1, 0):
        cnt, v = dirt(acc, soup["org"], soup["dr"], soup["rec"], ns, la.DirtParams(near, far, eps), fused, seed=3)
        assert np.array_equal(cnt, ecnt) and same_bits(v, eval_), fused
    # the ray at the far clip is not counted: with the next double above it as the far clip it is
    far2 = float(np.nextafter(far, np.inf))
    nh2, val2 = values(t, hit, N, near, far2)
    assert nh2[i_far // N] == nh[i_far // N] + 1
    cnt2, v2 = dirt(acc, soup["org"], soup["dr"], soup["rec"], ns, la.DirtParams(near, far2, eps), 1, seed=3)
    e2 = scatter(slot, nh2, val2)
    assert np.array_equal(cnt2, e2[0]) and same_bits(v2, e2[1])


def test_unbounded_clips_count_what_the_ao_stage_counts(soup):
    """far_clip = 1e38, near_clip = 0, eps = 1e-6: the rays are the AO stage's, every hit is a bounded hit"""
    acc = soup["acc"]; ns = N = 16
    slot, nslots, t, hit = soup_gather(soup, ns, 1e-6)
    occ, _ = ao(acc, soup["org"], soup["dr"], soup["rec"], ns, 1, seed=3)
    nh, val = values(t, hit, N, 0.0, 1.0e38)
    ecnt, eval_ = scatter(slot, nh, val)
    for fused in (1, 0):
        cnt, v = dirt(acc, soup["org"], soup["dr"], soup["rec"], ns, la.DirtParams(0.0, 1.0e38, 1e-6), fused, seed=3)
        assert np.array_equal(cnt, occ), fused
        assert np.array_equal(cnt, ecnt) and same_bits(v, eval_)


# ---- 3. compaction and lane boundaries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_compaction_and_lane_boundaries(soup, n):
    """the first n rays of the soup (the first n * N' gather rays of its hits are the batch's: slots number the hits in ray order)"""
    acc = soup["acc"]; ns = N = 16; eps = 1e-5
    slot, _, t, hit = soup_gather(soup, ns, eps)
    m = int((slot[:n] != NO_HIT).sum())
    th = t[hit]
    near, far = float(np.percentile(th, 25)), float(np.percentile(th, 75))
    nh, val = values(t[:m * N], hit[:m * N], N, near, far)
    ecnt, eval_ = scatter(slot[:n], nh, val)
    org, dr = soup["org"][:n].contiguous(), soup["dr"][:n].contiguous()
    rec = tuple(x[:n].contiguous() for x in soup["rec"])
    cf, vf = dirt(acc, org, dr, rec, ns, la.DirtParams(near, far, eps), 1, seed=3)
    cm, vm = dirt(acc, org, dr, rec, ns, la.DirtParams(near, far, eps), 0, seed=3)
    assert np.array_equal(cf, cm) and same_bits(vf, vm)
    assert np.array_equal(cf, ecnt) and same_bits(vf, eval_)


def test_lists_write_the_listed_slots_alone(soup):
    import torch
    acc = soup["acc"]; n = soup["n"]; NS = 16
    org, dr, rec = soup["org"], soup["dr"], soup["rec"]
    hit = soup["prim"] != po.MISS
    p = la.DirtParams(0.02, 0.3, 1e-5)
    full_c, full_v = dirt(acc, org, dr, rec, NS, p, 1, seed=3)

    def check(index, count, listed, fused):
        out = poison(n)
        cnt, v = dirt(acc, org, dr, rec, NS, p, fused, seed=3, index=index, count=count, out=out)
        assert np.array_equal(cnt[listed], full_c[listed]) and same_bits(v[listed], full_v[listed])
        assert (cnt[~listed] == POISON32).all() and (v[~listed] == np.float32(POISONF)).all()

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


# ---- 3b. rays that the persistent walk does not finish --------------------------------------------------------------------------
def test_small_visit_budgets_go_through_the_cooperative_walk(soup):
    """tiny "ray_budget"s send most gather rays through the fix-up queue to the cooperative walk, which stores the same word: the answer
    does not depend on the budget, and with statistics on the queue's traffic shows (lh_accel_last_retraced)"""
    acc = soup["acc"]; ns = N = 16; eps = 1e-5
    slot, nslots, t, hit = soup_gather(soup, ns, eps)
    th = t[hit]
    near, far = float(np.percentile(th, 25)), float(np.percentile(th, 75))
    nh, val = values(t, hit, N, near, far)
    ecnt, eval_ = scatter(slot, nh, val)
    p = la.DirtParams(near, far, eps)
    try:
        for budget in (2, 9, 40):
            acc.set_param("ray_budget", budget)
            cnt, v = dirt(acc, soup["org"], soup["dr"], soup["rec"], ns, p, 1, seed=3)
            assert np.array_equal(cnt, ecnt) and same_bits(v, eval_), budget
        acc.set_param("ray_budget", 2)
        acc.trace_statistics(True)
        acc.statistics(clear=True)
        cnt, v = dirt(acc, soup["org"], soup["dr"], soup["rec"], ns, p, 1, seed=3)
        s = acc.statistics(clear=True)
        queued = int(acc.L.lh_accel_last_retraced(acc.h))
        print("budget 2: %d of %d gather rays through the queue" % (queued, s["rays"]))
        assert np.array_equal(cnt, ecnt) and same_bits(v, eval_)
        assert s["rays"] == nslots * N and 0 < queued <= s["rays"]
    finally:
        acc.trace_statistics(False)
        acc.set_param("ray_budget", 128)


# ---- 4. queue overflow --------------------------------------------------------------------------------------------------------
def test_queue_overflow_answers_as_the_materialised_stage():
    """the frame whose fused AO stage overflows its fix-up queue at "ray_budget" 1 (tests.helpers.ao_overflow_case): the dirt stage
    answers at budget 1 as at budget 256 and as the materialised stage, bit for bit"""
    from tests.helpers import ao_overflow_case, load_golden
    acc, cam = ao_overflow_case()
    g = load_golden("ao_c1")
    pts = np.concatenate([g["pos%d" % k].reshape(-1, 3) for k in range(int(g["ngeoms"]))])
    diag = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    p = la.DirtParams(0.02 * diag, 0.2 * diag, 1e-5)
    W, H, NS, N = cam.width, cam.height, 16, 16
    import torch
    try:
        org, dr = acc.primary_rays(cam, 0, 0, W, H, 2)
        rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
        n = org.shape[0]
        miss = host(rec[0], np.uint32) == po.MISS
        assert n == W * H * 4 and 0 < int(miss.sum()) < n
        acc.set_param("ray_budget", 256)
        ref_c, ref_v = dirt(acc, org, dr, rec, NS, p, 1, seed=5, out=poison(n))
        assert (ref_c[miss] == NO_HIT).all() and (ref_v[miss] == 0.0).all() and (ref_c[~miss] <= N).all()
        assert 0 < int(ref_c[~miss].sum()) < int((~miss).sum()) * N and (ref_v[~miss] <= 1.0).all() and (ref_v[~miss] > 0.0).any()
        acc.set_param("ray_budget", 1)
        for fused in (1, 0):
            cnt, v = dirt(acc, org, dr, rec, NS, p, fused, seed=5, out=poison(n))
            assert np.array_equal(cnt, ref_c), (fused, int((cnt != ref_c).sum()))
            assert same_bits(v, ref_v), fused
    finally:
        acc.set_param("ray_budget", 128); acc.set_param("ao_fused", 1)
        acc.close()


# ---- 5. replay with caller uniforms ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1():
    return load_case("ao_c1")


@pytest.fixture(scope="module")
def ps():
    return load_case("ao_ps")


def scene_clips(case, eps=1e-5):
    g = case["g"]
    pts = np.concatenate([g["pos%d" % k].reshape(-1, 3) for k in range(int(g["ngeoms"]))])
    diag = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    return la.DirtParams(0.01 * diag, 0.25 * diag, eps)


def test_replay_with_caller_uniforms(c1):
    acc, cam, o = c1["acc"], c1["cam"], c1["oracle"]
    W = H = 256; N = NS = 16
    p = scene_clips(c1)
    order = np.zeros(2 * 64, np.uint32)
    nb = po.lib().lo_bucket_order(W, H, 32, order.ctypes.data_as(po.C.POINTER(po.C.c_uint)))
    mt = np.empty(2 * N * 1024 + 64); po.lib().lo_mt_stream(4357, mt.size, mt.ctypes.data_as(po._dp))
    uni_h = mt[:2 * N * 1024].copy(); uni = dev(uni_h)
    import torch
    org = dr = rec = None
    for b in range(nb):                                   # the first 32 x 32 bucket of the reference's order that hits anything
        bx, by = int(order[2 * b]) * 32, int(order[2 * b + 1]) * 32
        org, dr = acc.primary_rays(cam, bx, by, 32, 32, 1)
        rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
        if (host(rec[0], np.uint32) != po.MISS).any():
            break
    slot, nslots, go, gd = gather_rays(acc, org, dr, rec, NS, p.eps, uniforms=uni)
    assert nslots > 0
    t, hit = oracle_t(o, go, gd)
    nh, val = values(t, hit, N, p.near_clip, p.far_clip)
    ecnt, eval_ = scatter(slot, nh, val)
    assert 0 < int(nh.sum()) and (val > 0.0).any()
    cnt, v = dirt(acc, org, dr, rec, NS, p, 1, uniforms=uni)
    assert np.array_equal(cnt, ecnt) and same_bits(v, eval_)
    hrec = (host(rec[0], np.uint32), host(rec[1]), host(rec[2]), host(rec[3]))
    hc, hv = acc.dirt_host(host(org), host(dr), hrec, NS, p, uniforms=uni_h)
    assert np.array_equal(hc, ecnt) and same_bits(hv, eval_)
    hc, hv = acc.dirt_host(host(org), host(dr), hrec, NS, p, seed=9)          # and the built-in generator through the host form
    dc, dv = dirt(acc, org, dr, rec, NS, p, 1, seed=9)
    assert np.array_equal(hc, dc) and same_bits(hv, dv)


# ---- 6. the tile ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,pxs", [("c1", 1), ("c1", 2), ("ps", 1), ("ps", 2)])
def test_tile_equals_the_composition_and_does_not_depend_on_tiling(c1, ps, which, pxs):
    """lh_render_dirt_tile == lh_render_primary_rays -> lh_accel_intersect_device -> the dirt stage with key = absolute sample
    position, resolved as k_ao_resolve does.  The stage's per-hit value is a double inside the tile and a float at lh_accel_dirt_device's
    output, so the composition is checked twice: the oracle's doubles (rounded) are lh_accel_dirt_device's floats, and the same doubles
    accumulated per pixel are the tile"""
    import torch
    case = c1 if which == "c1" else ps
    acc, cam, o = case["acc"], case["cam"], case["oracle"]
    p = scene_clips(case)
    T, NS, N = 64, 16, 16
    x0, y0 = (cam.width - T) // 2, (cam.height - T) // 2
    spp = pxs * pxs
    rgb, st = acc.render_dirt_tile(cam, x0, y0, T, T, pxs, NS, p, seed=5)
    rgb = host(rgb).copy()
    org, dr = acc.primary_rays(cam, x0, y0, T, T, pxs)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    i = np.arange(T * T * spp, dtype=np.int64)
    ipix = i // spp
    key_h = ((y0 + ipix // T) * cam.width + (x0 + ipix % T)) * spp + (i - ipix * spp)
    key = dev(key_h)
    slot, nslots, go, gd = gather_rays(acc, org, dr, rec, NS, p.eps, seed=5, key=key)
    assert 0 < nslots == st["primary_hits"] and st["primary_rays"] == T * T * spp and st["ao_rays"] == nslots * N
    t, hit = oracle_t(o, go, gd)
    nh, val = values(t, hit, N, p.near_clip, p.far_clip)
    assert st["ao_occluded"] == int(nh.sum()) > 0
    ecnt, eval_ = scatter(slot, nh, val)
    cnt, v = dirt(acc, org, dr, rec, NS, p, 1, seed=5, key=key)
    assert np.array_equal(cnt, ecnt) and same_bits(v, eval_)
    # k_ao_resolve: accum = accum + value over the pixel's sub-samples, (float)(accum * (1.0 / (xs * ys))), clamped at 0, y flipped
    per = np.zeros(T * T * spp); h = slot != NO_HIT; per[h] = val[slot[h]]
    per = per.reshape(T * T, spp)
    accum = np.zeros(T * T)
    for s in range(spp):
        accum = accum + per[:, s]
    f = np.maximum((accum * (1.0 / spp)).astype(np.float32), np.float32(0.0)).reshape(T, T)[::-1]
    exp = np.repeat(f[:, :, None], 3, axis=2)
    assert same_bits(rgb, exp), int((rgb != exp).sum())
    assert (rgb > 0.0).any() and (rgb < 1.0).any()
    # the same frame region as four 32 x 32 tiles
    tot = {k: 0 for k in st}
    for ty in (0, 1):
        for tx in (0, 1):
            q, sq = acc.render_dirt_tile(cam, x0 + 32 * tx, y0 + 32 * ty, 32, 32, pxs, NS, p, seed=5)
            # image orientation: the tile at frame lines y0 + 32 ty .. is rows T - 32 (ty + 1) .. of the flipped 64-line tile
            assert same_bits(host(q), rgb[T - 32 * (ty + 1):T - 32 * ty, 32 * tx:32 * (tx + 1)]), (tx, ty)
            for k in tot:
                tot[k] += sq[k]
    assert tot == st


def test_tile_leaves_the_ao_tile_scratch_alone(c1):
    from tests.helpers import scratch_count
    acc, cam = c1["acc"], c1["cam"]
    x0, y0 = (cam.width - 64) // 2, (cam.height - 64) // 2
    acc.set_param("ao_fused", 0)
    try:
        _, st = acc.render_ao_tile(cam, x0, y0, 64, 64, 1, 16, seed=5)
    finally:
        acc.set_param("ao_fused", 1)
    before = [acc.scratch(k, dt, w) for k, dt, w in ((0, np.float64, 3), (6, np.uint32, 1), (8, np.float64, 3), (10, np.uint8, 1))]
    acc.render_dirt_tile(cam, 0, 0, 48, 40, 2, 4, scene_clips(c1), seed=9)
    after = [acc.scratch(k, dt, w) for k, dt, w in ((0, np.float64, 3), (6, np.uint32, 1), (8, np.float64, 3), (10, np.uint8, 1))]
    assert scratch_count(acc, 8) == st["primary_hits"] * 16 > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- 7. other scenes, refusals, statistics ----------------------------------------------------------------------------------------
def test_device_mesh_accelerator_and_empty_scene(soup):
    import torch
    n = 4000; NS = 16
    p = la.DirtParams(0.02, 0.3, 1e-5)
    org, dr = soup["org"][:n].contiguous(), soup["dr"][:n].contiguous()
    rec = tuple(x[:n].contiguous() for x in soup["rec"])
    ref_c, ref_v = dirt(soup["acc"], org, dr, rec, NS, p, 1, seed=3)
    assert ((ref_c != NO_HIT) & (ref_c > 0)).any()
    dm = la.HipAccel(0)
    dm.add_mesh_device(dev(soup["P"]), dev(soup["idx"])); dm.commit(); dm.wait_exact()
    rec_d = dm.intersect_device(org, dr); torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(rec_d, rec))
    for fused in (1, 0):
        c, v = dirt(dm, org, dr, rec_d, NS, p, fused, seed=3)
        assert np.array_equal(c, ref_c) and same_bits(v, ref_v)
    dm.close()
    empty = la.HipAccel(0); empty.commit()
    c, v = dirt(empty, org, dr, rec, NS, p, 1)                        # whatever the records say: nothing is there to hit
    assert (c == NO_HIT).all() and (v == 0.0).all()
    cam = la.Camera.make(32, 32, 1.0, [1.0 if k % 5 == 0 else 0.0 for k in range(16)], 1)
    rgb, st = empty.render_dirt_tile(cam, 0, 0, 32, 32, 1, NS, p)
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
    bad = [la.DirtParams(float("nan"), 0.5, 1e-5), la.DirtParams(0.5, 0.5, 1e-5), la.DirtParams(0.1, 2e38, 1e-5), la.DirtParams(-0.0 - 1e-300, 0.5, 1e-5),
           la.DirtParams(0.1, 0.5, -1.0), la.DirtParams(0.1, 0.5, float("inf"))]
    cases = [(acc.h, (n, O, D, P, T, U, V, 16, C.byref(b), 1, None, None, None, 0, None, CN, R, None), "bad dirt parameters") for b in bad] + [
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
        rc = L.lh_accel_dirt_device(h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_dirt_device" in err, (args, err)
    hc = np.full(n, POISON32, np.uint32); hv = np.full(n, POISONF, np.float32); z = np.zeros((n, 3)); zp = np.zeros(n, np.uint32); zt = np.zeros(n)
    Z, ZP, ZT = z.ctypes.data, zp.ctypes.data, zt.ctypes.data
    for h, args, msg in [
            (raw.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, None, 1, None, None, 0, hc.ctypes.data, hv.ctypes.data), "not committed"),
            (acc.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, C.byref(bad[0]), 1, None, None, 0, hc.ctypes.data, hv.ctypes.data), "bad dirt parameters"),
            (acc.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, None, 1, None, ZT, n, hc.ctypes.data, hv.ctypes.data), "uniforms"),
            (acc.h, (n, Z, Z, ZP, ZT, ZT, ZT, 16, None, 1, None, None, 0, None, None), "both outputs")]:
        rc = L.lh_accel_dirt_host(h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_dirt_host" in err, (args, err)
    cam = la.Camera.make(32, 32, 1.0, [1.0 if k % 5 == 0 else 0.0 for k in range(16)], 1)
    rgb = torch.full((8, 8, 3), POISONF, dtype=torch.float32, device="cuda"); st = binding.TileStats()
    for h, args, msg in [
            (raw.h, (C.byref(cam), 0, 0, 8, 8, 1, 16, None, 1, None, rgb.data_ptr(), C.byref(st), None), "not committed"),
            (acc.h, (C.byref(cam), 0, 0, 8, 8, 1, 16, C.byref(bad[1]), 1, None, rgb.data_ptr(), C.byref(st), None), "bad dirt parameters"),
            (acc.h, (C.byref(cam), 0, 0, 8, 8, 1, 16, None, 1, None, None, C.byref(st), None), "NULL"),
            (acc.h, (C.byref(cam), 0, 0, 0, 8, 1, 16, None, 1, None, rgb.data_ptr(), C.byref(st), None), "bad tile"),
            (acc.h, (C.byref(cam), 0, 0, 8, 8, 1, 0, None, 1, None, rgb.data_ptr(), C.byref(st), None), "bad tile")]:
        rc = L.lh_render_dirt_tile(h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_render_dirt_tile" in err, (args, err)
    torch.cuda.synchronize()
    assert (host(cnt) == POISON32).all() and (host(val) == np.float32(POISONF)).all() and (host(rgb) == np.float32(POISONF)).all()
    assert (hc == POISON32).all() and (hv == np.float32(POISONF)).all()
    # zero rays: 0, no array looked at
    assert L.lh_accel_dirt_device(acc.h, 0, None, None, None, None, None, None, 16, None, 1, None, None, None, 0, None, None, None, None) == 0
    # the binding refuses what is not a DirtParams, and wrong dtypes, before it calls C
    rec = (prim, t, u, v)
    for wrong in (lambda: acc.dirt_device(org, dr, rec, 16, (0.1, 0.5, 1e-5)), lambda: acc.dirt_device(org.float(), dr, rec, 16),
                  lambda: acc.dirt_device(org, dr, rec, 16, out=(cnt.float(), val)), lambda: acc.dirt_host(z, z, (zp, zt, zt, zt), 16, 0.5)):
        with pytest.raises(ValueError):
            wrong()
    raw.close()


def test_statistics_count_hits_times_n(soup):
    acc = soup["acc"]; n = 3000; NS = 16; N = 16
    p = la.DirtParams(0.02, 0.3, 1e-5)
    org, dr = soup["org"][:n].contiguous(), soup["dr"][:n].contiguous()
    rec = tuple(x[:n].contiguous() for x in soup["rec"])
    nslots = int((soup["prim"][:n] != po.MISS).sum())
    ref = {f: dirt(acc, org, dr, rec, NS, p, f, seed=3) for f in (1, 0)}
    acc.trace_statistics(True)
    try:
        for fused in (1, 0):
            acc.statistics(clear=True)
            cnt, v = dirt(acc, org, dr, rec, NS, p, fused, seed=3)
            s = acc.statistics(clear=True)
            assert np.array_equal(cnt, ref[fused][0]) and same_bits(v, ref[fused][1])
            assert s["rays"] == nslots * N and s["hits"] == int(cnt[cnt != NO_HIT].sum()) > 0 and s["nodes"] > 0
    finally:
        acc.trace_statistics(False)
