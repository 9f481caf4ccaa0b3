"""Direct light on the device (lh_accel_lights_device / _host, lh_accel_light_rays_device, lh_render_lights_tile; the rule:
lucille_amd/csrc/lh_lights.h): one shadow ray per hit and light, which lights each hit sees and what they add.

The scene is the environment tests' soup: po.soup(3000, 5000, 0.05, 7), its 2 730 hits (no multiple of 64); the tile runs on the ao_c1 golden scene.

Pinned to the oracle: the origins are restated from state_build (P + eps Ns), every shadow ray is the restatement's of tests/test_lights_rule.py, its
answer is oracle.intersect on (O, dir) filtered by t < tmax, and masks and values are that file's values() -- compared as integers and as uint32 views
of the floats.  A pair whose shadow ray has |dir.y| <= 1e-14 is outside the contract (reference UB) and is left out; at most 1 pair in 10 000 may be.

The light sets: the reference's sun (L = 1, directional, no flags); five lights -- a directional one from below with the cosine, a point light inside
the soup, one far outside it with the cosine, and the two inverse-square forms: with the first set, every combination of flags the rule accepts; and
LIGHTS_MAX = 31 lights cycling through all six, bit 30 exercised (the header says why the list ends at 31)."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests.test_gpu_ao import load_case
from tests.test_gpu_ao_batch import NO_HIT, POISON32, POISONF, dev, host
from tests.test_gpu_dirt import same_bits
from tests.test_lights_rule import COSINE, INVSQ, POINT, items, values

pytestmark = pytest.mark.gpu

EPS = 1e-5
SUN = [((0.3, 0.9, 0.316227766), (1.0, 0.9, 0.8), 0)]
FIVE = [((0.1, -1.0, 0.2), (0.5, 0.25, 1.0), COSINE),                    # from below
        ((0.45, 0.52, 0.48), (1.0, 2.0, 3.0), POINT),                     # inside the soup (the unit cube)
        ((40.0, 75.0, -30.0), (3.0, 1.0, 0.5), POINT | COSINE),           # far outside
        ((0.9, 1.3, 0.4), (0.25, 0.5, 0.125), POINT | INVSQ),
        ((-1.2, 0.8, -0.7), (2.0, 2.0, 1.0), POINT | COSINE | INVSQ)]


def _many():
    rng = np.random.default_rng(31)
    combos = [0, COSINE, POINT, POINT | COSINE, POINT | INVSQ, POINT | COSINE | INVSQ]
    out = []
    for l in range(la.LIGHTS_MAX):
        f = combos[l % 6]
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * (rng.uniform(1.5, 4.0) if f & POINT else 1.0)
        if abs(v[1]) < 0.05:
            v[1] = 0.05
        out.append((tuple(float(x) for x in v), tuple(float(x) for x in rng.uniform(0.1, 2.0, 3)), f))
    out[30] = ((0.2, 1.0, 0.1), (1.0, 1.0, 1.0), 0)          # the last light, bit 30: a plain directional one many hits see
    return out


SETS = {"sun": SUN, "five": FIVE, "many": _many()}


def mk(lights):
    return [la.Light(v, rgb, flags) for v, rgb, flags in lights]


def lights(acc, o, d, rec, ls, params=None, fused=1, **kw):
    """lights_device with "ao_fused" set for the call -> (visible uint32, rgb float32 [n, 3]) on the host"""
    acc.set_param("ao_fused", fused)
    try:
        v, c = acc.lights_device(o, d, rec, mk(ls), params, **kw)
    finally:
        acc.set_param("ao_fused", 1)
    return host(v, np.uint32).copy(), host(c).copy()


def poison(n):
    import torch
    return (torch.full((n,), POISON32, dtype=torch.int32, device="cuda"), torch.full((n, 3), POISONF, dtype=torch.float32, device="cuda"))


@pytest.fixture(scope="module")
def ls():
    """the soup, committed, with the closest-hit records of its rays, the hits' origins and normals restated from state_build, and per light set the
    oracle's answers -- computed once, never changed"""
    import torch
    n = 5000
    P, idx, org, dr = po.soup(3000, n, 0.05, 7)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    to, td = dev(org), dev(dr)
    rec = acc.intersect_device(to, td); torch.cuda.synchronize()
    prim = host(rec[0], np.uint32).copy()
    st = acc.state_build(org, dr, prim, host(rec[1]), host(rec[2]), host(rec[3]))
    ids = np.nonzero(prim != po.MISS)[0]
    O = st[ids, 0:3] + st[ids, 6:9] * EPS
    Ns = st[ids, 6:9].copy()
    O.setflags(write=False); Ns.setflags(write=False)
    d = {"acc": acc, "oracle": o, "P": P, "idx": idx, "org": to, "dr": td, "rec": rec, "prim": prim, "n": n, "ids": ids, "O": O, "Ns": Ns, "exp": {}}
    yield d
    acc.close()


def expected(ls, name):
    """-> (occ [nslots, L]: the oracle's bounded any-hit answer of every item that is traced, 0 elsewhere; out [nslots, L]: the pairs outside the
    contract; mask, value per slot; tmax [nslots, L])"""
    if name not in ls["exp"]:
        O, Ns, L = ls["O"], ls["Ns"], len(SETS[name])
        occ = np.zeros((O.shape[0], L), np.uint8); out = np.zeros((O.shape[0], L), bool); tms = np.zeros((O.shape[0], L))
        for l, (v, rgb, flags) in enumerate(SETS[name]):
            d, w, tm = items(O, Ns, v, flags)
            go = tm > 0.0
            out[:, l] = go & (np.abs(d[:, 1]) <= 1e-14)
            prim, t, _, _ = ls["oracle"].intersect(O[go], d[go], nthreads=8)
            occ[go, l] = (prim != po.MISS) & (t < tm[go])
            tms[:, l] = tm
        mask, val = values(O, Ns, SETS[name], occ)
        for a in (occ, out, mask, val, tms):
            a.setflags(write=False)
        ls["exp"][name] = (occ, out, mask, val, tms)
    return ls["exp"][name]


def scatter(ls, mask, val):
    n = ls["n"]
    m = np.full(n, NO_HIT, np.uint32); m[ls["ids"]] = mask
    v = np.zeros((n, 3), np.float32); v[ls["ids"]] = val
    return m, v


def compare(ls, name, got_mask, got_val):
    """masks as integers, values as bits, the pairs outside the contract left out (their bit in either mask, their hit's value)"""
    occ, out, mask, val, _ = expected(ls, name)
    emask, eval_ = scatter(ls, mask, val)
    skip_bits = np.zeros(ls["n"], np.uint32)
    skip_bits[ls["ids"]] = (out.astype(np.uint32) << np.arange(out.shape[1], dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
    hit = emask != NO_HIT
    assert (got_mask[~hit] == NO_HIT).all() and (got_val[~hit] == 0.0).all()
    keep = ~skip_bits[hit]
    assert np.array_equal(got_mask[hit] & keep, emask[hit] & keep), (name, int(((got_mask[hit] & keep) != (emask[hit] & keep)).sum()))
    whole = hit & (skip_bits == 0)
    assert same_bits(got_val[whole], eval_[whole]), (name, int((got_val[whole].view(np.uint32) != eval_[whole].view(np.uint32)).any(axis=1).sum()))


# ---- 1. the sets exercise the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sun", "five", "many"])
def test_the_sets_exercise_the_rule(ls, name):
    """by the oracle and the restatement alone: lit and shadowed pairs for every light, culled pairs where a cosine says so, and at most 1 pair in
    10 000 outside the contract"""
    occ, out, mask, val, tms = expected(ls, name)
    L = len(SETS[name]); nslots = occ.shape[0]
    assert nslots == 2730 and nslots % 64 != 0
    print("%s: %d pairs, %d outside the contract, %d not traced, %d closed, %d lit" % (name, occ.size, int(out.sum()), int((tms == 0).sum()), int(occ.sum()),
                                                                                       int(sum(bin(int(m)).count("1") for m in mask))))
    assert out.sum() * 10000 <= occ.size
    for l in range(L):
        bit = (mask >> np.uint32(l)) & 1
        assert 0 < int(bit.sum()) < nslots, l                                   # every light is seen by some hits and not by others
        if SETS[name][l][2] & COSINE:
            assert (tms[:, l] == 0).any() and (tms[:, l] > 0).any(), l          # the cosine culls the hits that face away
        else:
            assert (tms[:, l] > 0).all() and occ[:, l].any(), l                 # every pair is traced, some are closed
    if name == "many":
        assert L == 31 and ((mask >> np.uint32(30)) & 1).any() and (mask != NO_HIT).all()
    if name == "sun":
        assert np.array_equal(val[mask == 1], np.tile(np.asarray(SUN[0][1], np.float32), (int((mask == 1).sum()), 1)))          # Lo += light->col
    assert (val[mask == 0] == 0.0).all() and (val[mask != 0] > 0.0).any()


# ---- 2. the oracle pin, fused and materialised ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sun", "five", "many"])
def test_oracle_pin_fused_and_materialised(ls, name):
    acc = ls["acc"]
    got = {}
    for fused in (1, 0):
        m, v = lights(acc, ls["org"], ls["dr"], ls["rec"], SETS[name], la.LightsParams(EPS), fused)
        compare(ls, name, m, v)
        got[fused] = (m, v)
    assert np.array_equal(got[1][0], got[0][0]) and same_bits(got[1][1], got[0][1])          # both paths: the same bytes
    m, v = lights(acc, ls["org"], ls["dr"], ls["rec"], SETS[name], None, 1)                   # NULL parameters: eps 1e-5
    assert np.array_equal(m, got[1][0]) and same_bits(v, got[1][1])


def test_another_eps_moves_the_origins(ls):
    acc = ls["acc"]
    m0, v0 = lights(acc, ls["org"], ls["dr"], ls["rec"], FIVE, la.LightsParams(EPS), 1)
    for fused in (1, 0):
        m, v = lights(acc, ls["org"], ls["dr"], ls["rec"], FIVE, la.LightsParams(0.25), fused)
        assert not same_bits(v, v0) and (m != m0).any()


# ---- 3. the rays alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["five", "many"])
def test_the_rays_alone_and_a_bounded_any_hit_launch_reproduce_the_bits(ls, name):
    import torch
    acc = ls["acc"]; L = len(SETS[name]); n = ls["n"]
    so, ns, ro, rd, rt = acc.light_rays_device(ls["org"], ls["dr"], ls["rec"], mk(SETS[name]), la.LightsParams(EPS))
    torch.cuda.synchronize()
    nslots = int(host(ns, np.uint32)[0])
    assert nslots == ls["ids"].shape[0]
    slot = host(so, np.uint32)
    escan = np.full(n, NO_HIT, np.uint32); escan[ls["ids"]] = np.arange(nslots, dtype=np.uint32)
    assert np.array_equal(slot, escan)
    m = nslots * L
    go, gd, gt = host(ro)[:m].reshape(nslots, L, 3), host(rd)[:m].reshape(nslots, L, 3), host(rt)[:m].reshape(nslots, L)
    for l, (v, rgb, flags) in enumerate(SETS[name]):
        d, w, tm = items(ls["O"], ls["Ns"], v, flags)
        assert np.array_equal(go[:, l].view(np.uint64), ls["O"].view(np.uint64)), l
        assert np.array_equal(gd[:, l].view(np.uint64), d.view(np.uint64)), l
        assert np.array_equal(gt[:, l].view(np.uint64), tm.view(np.uint64)), l
    occ = acc.intersect_device(ro[:m].contiguous(), rd[:m].contiguous(), mode=la.MODE_ANY, tmax=rt[:m].contiguous())[0]
    torch.cuda.synchronize()
    occ = host(occ).reshape(nslots, L)
    bits = (gt > 0.0) & (occ == 0)
    by_hand = (bits.astype(np.uint32) << np.arange(L, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
    stage, _ = lights(acc, ls["org"], ls["dr"], ls["rec"], SETS[name], la.LightsParams(EPS), 1)
    assert np.array_equal(by_hand, stage[ls["ids"]])
    assert (occ[gt == 0.0] == 0).all()          # a dead bound: the launch answers 0, the byte the stage leaves for an item it does not trace
    with pytest.raises(la.LucilleHipError, match="capacity_rays"):
        acc.light_rays_device(ls["org"], ls["dr"], ls["rec"], mk(SETS[name]), None, out=(so, ns, ro[:m - 1], rd, rt))


# ---- 4. lists ---------------------------------------------------------------------------------------------------------------------------------
def test_lists_write_the_listed_slots_alone(ls):
    import torch
    acc = ls["acc"]; n = ls["n"]
    org, dr, rec = ls["org"], ls["dr"], ls["rec"]
    full_m, full_v = lights(acc, org, dr, rec, FIVE, None, 1)

    def check(index, count, listed, fused):
        out = poison(n)
        m, v = lights(acc, org, dr, rec, FIVE, None, fused, index=index, count=count, out=out)
        assert np.array_equal(m[listed], full_m[listed]) and same_bits(v[listed], full_v[listed])
        assert (m[~listed] == POISON32).all() and (v[~listed] == np.float32(POISONF)).all()

    rng = np.random.default_rng(5)
    lst = rng.permutation(n)[:1500].astype(np.uint32)
    lst[7] = lst[3]; lst[11] = n + 9                                  # an id twice, an id >= n
    listed = np.zeros(n, bool); listed[lst[lst < n]] = True
    part = np.zeros(n, bool); part[lst[:100][lst[:100] < n]] = True   # a device count cuts the list
    for fused in (1, 0):
        check(dev(lst), None, listed, fused)
        check(dev(lst), torch.tensor([100], dtype=torch.int32, device="cuda"), part, fused)
        check(dev(lst), torch.zeros(1, dtype=torch.int32, device="cuda"), np.zeros(n, bool), fused)
    idx, cnt = la.compact(rec[0], la.SELECT_HIT)                      # the hits, count on the device
    check(idx, cnt, ls["prim"] != po.MISS, 1)
    # one output alone
    vis = torch.full((n,), POISON32, dtype=torch.int32, device="cuda")
    acc.lights_device(org, dr, rec, mk(FIVE), None, out=(vis, None))
    assert np.array_equal(host(vis, np.uint32), full_m)
    rgb = torch.full((n, 3), POISONF, dtype=torch.float32, device="cuda")
    acc.lights_device(org, dr, rec, mk(FIVE), None, out=(None, rgb))
    assert same_bits(host(rgb), full_v)
    with pytest.raises(ValueError):
        acc.lights_device(org, dr, rec, mk(FIVE), None, out=(None, None))


# ---- 5. small and empty -------------------------------------------------------------------------------------------------------------------------
def test_one_ray(ls):
    """n_rays = 1: a hit and a miss, every set, both paths"""
    acc = ls["acc"]
    full = {name: lights(acc, ls["org"], ls["dr"], ls["rec"], SETS[name], None, 1) for name in SETS}
    hit_id = int(ls["ids"][0]); miss_id = int(np.nonzero(ls["prim"] == po.MISS)[0][0])
    for i in (hit_id, miss_id):
        o, d = ls["org"][i:i + 1].contiguous(), ls["dr"][i:i + 1].contiguous()
        rec = tuple(x[i:i + 1].contiguous() for x in ls["rec"])
        for name in SETS:
            for fused in (1, 0):
                m, v = lights(acc, o, d, rec, SETS[name], None, fused)
                assert m[0] == full[name][0][i] and same_bits(v[0], full[name][1][i]), (i, name, fused)
    assert full["five"][0][miss_id] == NO_HIT and full["five"][0][hit_id] != NO_HIT


def test_empty_scene_and_no_rays(ls):
    import torch
    e = la.HipAccel(0); e.commit()
    try:
        n = 100
        org, dr = ls["org"][:n].contiguous(), ls["dr"][:n].contiguous()
        rec = tuple(x[:n].contiguous() for x in ls["rec"])          # records of another scene: an empty scene reads none of them
        out = poison(n)
        m, v = lights(e, org, dr, rec, FIVE, None, 1, out=out)
        assert (m == NO_HIT).all() and (v == 0.0).all()
        lst = np.array([5, 5, 99, 100, 7], np.uint32)
        out = poison(n)
        m, v = lights(e, org, dr, rec, FIVE, None, 1, index=dev(lst), out=out)
        listed = np.zeros(n, bool); listed[[5, 99, 7]] = True
        assert (m[listed] == NO_HIT).all() and (m[~listed] == POISON32).all() and (v[~listed] == np.float32(POISONF)).all()
        so, ns, _, _, _ = e.light_rays_device(org, dr, rec, mk(FIVE)); torch.cuda.synchronize()
        assert int(host(ns)[0]) == 0 and (host(so, np.uint32) == NO_HIT).all()
        hv, hr = e.lights_host(host(org), host(dr), tuple(host(x) for x in rec), mk(FIVE))
        assert (hv == NO_HIT).all() and (hr == 0.0).all()
    finally:
        e.close()
    z = ls["org"][:0].contiguous()
    m, v = ls["acc"].lights_device(z, z, tuple(x[:0].contiguous() for x in ls["rec"]), mk(SUN))
    assert m.shape[0] == 0 and tuple(v.shape) == (0, 3)


def test_host_form_equals_the_device_form(ls):
    acc = ls["acc"]
    hrec = (host(ls["rec"][0], np.uint32), host(ls["rec"][1]), host(ls["rec"][2]), host(ls["rec"][3]))
    for name in ("five", "many"):
        m, v = lights(acc, ls["org"], ls["dr"], ls["rec"], SETS[name], la.LightsParams(EPS), 1)
        hm, hv = acc.lights_host(host(ls["org"]), host(ls["dr"]), hrec, mk(SETS[name]), la.LightsParams(EPS))
        assert np.array_equal(hm, m) and same_bits(hv, v), name


# ---- 6. rays that the persistent walk does not finish -------------------------------------------------------------------------------------------
def test_short_stacks_and_a_small_budget_go_through_the_cooperative_walk(ls):
    """an accelerator of its own on the same soup with "stack_cap" 8 and "ao_budget" 4: a large share of the shadow rays leaves the persistent walk for
    the fix-up queue and the cooperative walk, which makes the ray again from the item index and stores the same byte"""
    acc = la.HipAccel(0); acc.add_mesh(ls["P"], ls["idx"]); acc.commit(); acc.wait_exact()
    try:
        acc.set_param("stack_cap", 8); acc.set_param("ao_budget", 4)
        acc.trace_statistics(True)
        for name in ("five", "many"):
            acc.statistics(clear=True)
            m, v = lights(acc, ls["org"], ls["dr"], ls["rec"], SETS[name], la.LightsParams(EPS), 1)
            s = acc.statistics(clear=True)
            queued = int(acc.L.lh_accel_last_retraced(acc.h))
            occ, out, mask, val, tms = expected(ls, name)
            print("%s: %d of %d items through the queue (%d traced)" % (name, queued, s["rays"], int((tms > 0).sum())))
            assert 0 < queued <= int((tms > 0).sum())
            compare(ls, name, m, v)
            ref = lights(ls["acc"], ls["org"], ls["dr"], ls["rec"], SETS[name], la.LightsParams(EPS), 1)
            assert np.array_equal(m, ref[0]) and same_bits(v, ref[1])
    finally:
        acc.close()


# ---- 7. statistics ------------------------------------------------------------------------------------------------------------------------------
def test_statistics_count_the_work_items(ls):
    """with trace statistics on, `rays` advances by hits x L -- work items, traced or culled -- and `hits` (counters[4]) by the items whose bit is clear"""
    acc = ls["acc"]
    acc.trace_statistics(True)
    try:
        for name in ("sun", "five"):
            L = len(SETS[name]); nslots = ls["ids"].shape[0]
            for fused in (1, 0):
                acc.statistics(clear=True)
                m, _ = lights(acc, ls["org"], ls["dr"], ls["rec"], SETS[name], None, fused)
                st = acc.statistics(clear=True)
                set_bits = int(sum(bin(int(x)).count("1") for x in m[m != NO_HIT]))
                assert st["rays"] == nslots * L and st["hits"] == nslots * L - set_bits, (name, fused, st)
    finally:
        acc.trace_statistics(False)


# ---- 8. the tile ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1():
    return load_case("ao_c1")


@pytest.mark.parametrize("pxs", [1, 2])
def test_tile_equals_the_batch_values_and_does_not_depend_on_tiling(c1, pxs):
    """lh_render_lights_tile == lh_render_primary_rays -> lh_accel_intersect_device -> lh_accel_lights_device -> per sample the hit's three floats,
    widened, added over the pixel's sub-samples in sample order, scaled, converted, clamped and written as the environment tile's"""
    import torch
    acc, cam = c1["acc"], c1["cam"]
    T = 64
    x0, y0 = (cam.width - T) // 2, (cam.height - T) // 2
    spp = pxs * pxs
    org, dr = acc.primary_rays(cam, x0, y0, T, T, pxs)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    # lights around the camera's scene, whatever its scale: placed from the hits' own bounding box
    prim = host(rec[0], np.uint32); hit = prim != po.MISS
    Pn = (host(org) + host(dr) * host(rec[1])[:, None])[hit]
    lo, hi = Pn.min(axis=0), Pn.max(axis=0); c = 0.5 * (lo + hi); r = float(np.linalg.norm(hi - lo))
    sets = [((0.3, 0.9, 0.316227766), (1.0, 0.9, 0.8), 0), ((-0.5, 0.7, 0.4), (0.2, 0.4, 0.9), COSINE),
            (tuple(c + np.array([0.3, 0.8, 0.2]) * r), (3.0, 2.0, 1.0), POINT | COSINE),
            (tuple(c + np.array([-0.6, 0.5, -0.4]) * r), (0.5, 1.0, 2.0) , POINT | COSINE | INVSQ)]
    m, v = lights(acc, org, dr, rec, sets, None, 1)
    nslots = int(hit.sum())
    set_bits = int(sum(bin(int(x)).count("1") for x in m[hit]))
    assert 0 < set_bits < nslots * len(sets) and (v[hit] > 0).any()
    per = v.astype(np.float64).reshape(T * T, spp, 3)
    accum = np.zeros((T * T, 3))
    for q in range(spp):
        accum = accum + per[:, q, :]
    exp = np.maximum((accum * (1.0 / spp)).astype(np.float32), np.float32(0.0)).reshape(T, T, 3)[::-1]
    for fused in (1, 0):
        acc.set_param("ao_fused", fused)
        try:
            rgb, st = acc.render_lights_tile(cam, x0, y0, T, T, pxs, mk(sets))
        finally:
            acc.set_param("ao_fused", 1)
        rgb = host(rgb).copy()
        assert 0 < nslots == st["primary_hits"] and st["primary_rays"] == T * T * spp and st["ao_rays"] == nslots * len(sets)
        assert st["ao_occluded"] == nslots * len(sets) - set_bits
        assert same_bits(rgb, exp), (fused, int((rgb != exp).sum()))
    assert (rgb[:, :, 0] != rgb[:, :, 2]).any()
    tot = {k: 0 for k in st}
    for ty in (0, 1):
        for tx in (0, 1):
            q, sq = acc.render_lights_tile(cam, x0 + 32 * tx, y0 + 32 * ty, 32, 32, pxs, mk(sets))
            assert same_bits(host(q), rgb[T - 32 * (ty + 1):T - 32 * ty, 32 * tx:32 * (tx + 1)]), (tx, ty)
            for k in tot:
                tot[k] += sq[k]
    assert tot == st
    q, sq = acc.render_lights_tile(cam, x0, y0 + 3, T, 17, pxs, mk(sets))          # an odd tiling of the same frame
    assert same_bits(host(q), rgb[T - 20:T - 3])
