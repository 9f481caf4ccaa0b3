"""Area lights on the device (lh_accel_set_emitters, lh_accel_area_lights_device / _host, lh_accel_area_light_rays_device,
lh_render_area_lights_tile; the rule: lucille_amd/csrc/lh_area.h): S rays per hit and light to points drawn on the light's emitter triangles, which
lights each hit sees and the mean of what the samples add.

The scene is the lights tests' soup: po.soup(3000, 5000, 0.05, 7), its 2 730 hits (no multiple of 64); the tile runs on the ao_c1 golden scene.

Pinned to the oracle: the origins are restated from state_build (P + eps Ns), every item's uniforms, ray, bound and weight are the restatement's of
tests/test_area_rule.py, its answer is oracle.intersect on (O, dir) filtered by t < bound, and masks and values are that file's values() -- compared as
integers and as uint32 views of the floats.  An item whose ray has |dir.y| <= 1e-14 is outside the contract; the emitters chosen here leave out none
(positions are floats against double origins), which test_the_sets_exercise_the_rule checks with the oracle and the restatement alone.

The emitter table holds four emitters one after the other: a triangle above the soup, a quad inside it, a mesh of twenty triangles outside, and three
triangles of which the middle one has no area."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests.test_area_rule import COSINE, FACING, INVSQ, PDF, builtin_uniforms, items, records, values
from tests.test_gpu_ao import load_case
from tests.test_gpu_ao_batch import NO_HIT, POISON32, POISONF, dev, host
from tests.test_gpu_dirt import same_bits

pytestmark = pytest.mark.gpu

EPS = 1e-5
SEED = 7


def _table():
    rng = np.random.default_rng(20240)
    one = np.array([[[0.2, 2.13, 0.25], [0.85, 2.21, 0.3], [0.5, 2.05, 0.9]]])          # above the unit cube, its normal points down
    quad = np.array([[[0.3, 0.45, 0.3], [0.55, 0.47, 0.32], [0.53, 0.44, 0.57]], [[0.3, 0.45, 0.3], [0.53, 0.44, 0.57], [0.28, 0.42, 0.55]]])
    mesh = np.array([1.7, 1.3, -1.9]) + 0.3 * rng.standard_normal((20, 3, 3))
    flat = np.array([[[0.0, 3.0, 0.0], [0.0, 3.2, 1.0], [1.0, 3.1, 0.0]],
                     [[0.5, 3.0, 0.5], [0.5, 3.0, 0.5], [0.9, 3.3, 0.1]],               # no area
                     [[1.0, 3.0, 1.0], [1.0, 3.1, 2.0], [2.0, 3.3, 1.0]]])
    return np.concatenate([one, quad, mesh, flat])


TABLE = _table()
ONE, QUAD, MESH, FLAT = (0, 1), (1, 2), (3, 20), (23, 3)


def _many():
    rng = np.random.default_rng(31)
    out = []
    for l in range(la.AREA_LIGHTS_MAX):
        first = int(rng.integers(TABLE.shape[0])); n = int(rng.integers(1, min(4, TABLE.shape[0] - first) + 1))
        out.append((first, n, tuple(float(x) for x in rng.uniform(0.1, 2.0, 3)), l % 16))
    out[30] = (ONE[0], ONE[1], (1.0, 1.0, 1.0), 0)          # the last light, bit 30: the plain triangle above the soup
    return out


# name -> (lights, S)
SETS = {"one1": ([(ONE[0], ONE[1], (1.0, 0.9, 0.8), 0)], 1),
        "one16": ([(ONE[0], ONE[1], (1.0, 0.9, 0.8), 0)], 16),
        "three": ([(ONE[0], ONE[1], (1.0, 0.9, 0.8), 0), (QUAD[0], QUAD[1], (3.0, 2.0, 1.0), FACING | INVSQ | PDF),
                   (MESH[0], MESH[1], (0.5, 1.0, 2.0), COSINE | FACING | INVSQ | PDF)], 4),
        "many": (_many(), 4),
        "flat": ([(FLAT[0], FLAT[1], (1.0, 2.0, 3.0), PDF), (FLAT[0], FLAT[1], (0.25, 0.5, 1.0), 0)], 4)}


def mk(lights):
    return [la.AreaLight(f, n, rgb, flags) for f, n, rgb, flags in lights]


def prm(S, bound=1.0, eps=EPS):
    return la.AreaParams(eps, bound, S)


def area(acc, o, d, rec, name, fused=1, bound=1.0, eps=EPS, seed=SEED, **kw):
    """area_lights_device with "ao_fused" set for the call -> (visible uint32, rgb float32 [n, 3]) on the host"""
    lights, S = SETS[name] if isinstance(name, str) else name
    acc.set_param("ao_fused", fused)
    try:
        v, c = acc.area_lights_device(o, d, rec, mk(lights), prm(S, bound, eps), seed, **kw)
    finally:
        acc.set_param("ao_fused", 1)
    return host(v, np.uint32).copy(), host(c).copy()


def poison(n):
    import torch
    return (torch.full((n,), POISON32, dtype=torch.int32, device="cuda"), torch.full((n, 3), POISONF, dtype=torch.float32, device="cuda"))


def hits_of(acc, org, dr, eps=EPS):
    """closest-hit records of a batch and the hits' origins and normals restated from state_build"""
    import torch
    to, td = dev(org), dev(dr)
    rec = acc.intersect_device(to, td); torch.cuda.synchronize()
    prim = host(rec[0], np.uint32).copy()
    st = acc.state_build(org, dr, prim, host(rec[1]), host(rec[2]), host(rec[3]))
    ids = np.nonzero(prim != po.MISS)[0]
    O = st[ids, 0:3] + st[ids, 6:9] * eps
    Ns = st[ids, 6:9].copy()
    O.setflags(write=False); Ns.setflags(write=False)
    return {"org": to, "dr": td, "rec": rec, "prim": prim, "ids": ids, "O": O, "Ns": Ns, "n": org.shape[0]}


@pytest.fixture(scope="module")
def ls():
    """the soup, committed, with the emitter table set, the closest-hit records of its rays and the restated hits -- computed once, never changed"""
    n = 5000
    P, idx, org, dr = po.soup(3000, n, 0.05, 7)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    acc.set_emitters(TABLE)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    d = hits_of(acc, org, dr)
    d.update({"acc": acc, "oracle": o, "P": P, "idx": idx, "horg": org, "hdr": dr, "exp": {}})
    yield d
    acc.close()


def pin(oracle, O, Ns, keys, lights, S, table=TABLE, bound=1.0, seed=SEED, X=None):
    """the restatement and the oracle -> (X [nslots, L, S, 3], D, W, T [nslots, L, S(, 3)], occ [nslots, L, S], outside [nslots, L, S], mask, value,
    closed per slot)"""
    rec = records(table)
    L, ns = len(lights), O.shape[0]
    if X is None:
        X = builtin_uniforms(keys, seed, L, S)
    D = np.zeros((ns, L, S, 3)); W = np.zeros((ns, L, S)); T = np.zeros((ns, L, S))
    for l, lt in enumerate(lights):
        for s in range(S):
            D[:, l, s], W[:, l, s], T[:, l, s] = items(O, Ns, lt, rec, X[:, l, s], bound)
    go = T > 0.0
    Ob = np.broadcast_to(O[:, None, None, :], D.shape)
    prim, t, _, _ = oracle.intersect(np.ascontiguousarray(Ob[go]), np.ascontiguousarray(D[go]), nthreads=8)
    occ = np.zeros((ns, L, S), np.uint8)
    occ[go] = (prim != po.MISS) & (t < T[go])
    outside = go & (np.abs(D[..., 1]) <= 1e-14)
    mask, val, closed = values(O, Ns, lights, S, rec, X, bound, occ)
    r = dict(X=X, D=D, W=W, T=T, occ=occ, outside=outside, mask=mask, val=val, closed=closed, prim=prim, t=t, go=go)
    for a in r.values():
        a.setflags(write=False)
    return r


def expected(ls, name):
    if name not in ls["exp"]:
        lights, S = SETS[name]
        ls["exp"][name] = pin(ls["oracle"], ls["O"], ls["Ns"], ls["ids"].astype(np.uint64), lights, S)
    return ls["exp"][name]


def scatter(h, mask, val):
    n = h["n"]
    m = np.full(n, NO_HIT, np.uint32); m[h["ids"]] = mask
    v = np.zeros((n, 3), np.float32); v[h["ids"]] = val
    return m, v


def compare(h, e, got_mask, got_val, what=""):
    """masks as integers, values as bits (no item is outside the contract: checked where the expectation is made)"""
    assert not e["outside"].any()
    emask, eval_ = scatter(h, e["mask"], e["val"])
    assert np.array_equal(got_mask, emask), (what, int((got_mask != emask).sum()))
    assert same_bits(got_val, eval_), (what, int((got_val.view(np.uint32) != eval_.view(np.uint32)).any(axis=1).sum()))


# ---- 1. the sets exercise the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_the_sets_exercise_the_rule(ls, name):
    """by the oracle and the restatement alone: open and closed items for every light, culled items where a flag says so, partly lit lights (the soft
    edge), and no item outside the contract"""
    e = expected(ls, name)
    lights, S = SETS[name]
    L, nslots = len(lights), e["T"].shape[0]
    assert nslots == 2730 and nslots % 64 != 0
    open_ = (e["T"] > 0) & (e["occ"] == 0)
    per_light = open_.sum(axis=2)
    print("%s: %d items, %d outside the contract, %d not traced, %d closed, %d open, %d (hit, light) pairs partly lit" % (
        name, e["T"].size, int(e["outside"].sum()), int((e["T"] == 0).sum()), int(e["occ"].sum()), int(open_.sum()), int(((per_light > 0) & (per_light < S)).sum())))
    assert not e["outside"].any()
    assert open_.any() and e["occ"].any()
    if S > 1:
        assert ((per_light > 0) & (per_light < S)).any()          # a penumbra: some samples of a light open, some not
    for l, lt in enumerate(lights):
        if name != "many":
            assert 0 < int(open_[:, l].any(axis=1).sum()) < nslots, l
            if lt[3] & (COSINE | FACING):
                assert (e["T"][:, l] == 0).any(), l          # a cosine culls the hits that face away
    if name == "many":
        assert L == 31 and ((e["mask"] >> np.uint32(30)) & 1).any() and (e["mask"] != NO_HIT).all()
        assert {lt[3] for lt in lights} == set(range(16))
    if name == "flat":
        j = np.floor(e["X"][:, :, :, 0] * 3).astype(int)
        assert (e["T"][:, 0][j[:, 0] == 1] == 0).all() and (e["T"][:, 1][j[:, 1] == 1] > 0).any()          # no area: weightless with the pdf, traced without
    if name == "one1":
        lit = e["mask"] == 1
        assert np.array_equal(e["val"][lit], np.tile(np.asarray(lights[0][2], np.float32), (int(lit.sum()), 1)))
    assert (e["val"][e["mask"] == 0] == 0.0).all() and (e["val"][e["mask"] != 0] > 0.0).any()


# ---- 2. the oracle pin: fused, materialised, replayed ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_oracle_pin_fused_materialised_and_replayed(ls, name):
    acc = ls["acc"]
    e = expected(ls, name)
    got = {}
    for fused in (1, 0):
        m, v = area(acc, ls["org"], ls["dr"], ls["rec"], name, fused)
        compare(ls, e, m, v, (name, fused))
        got[fused] = (m, v)
    assert np.array_equal(got[1][0], got[0][0]) and same_bits(got[1][1], got[0][1])          # both paths: the same bytes
    # the built-in generator computed here and fed through the replay path: one sampling rule
    uni = dev(np.ascontiguousarray(e["X"]).reshape(-1))
    m, v = area(acc, ls["org"], ls["dr"], ls["rec"], name, 1, uniforms=uni, seed=12345)
    assert np.array_equal(m, got[1][0]) and same_bits(v, got[1][1])


def test_defaults_seed_eps_and_other_uniforms(ls):
    acc = ls["acc"]
    lights, S = SETS["three"]
    base = area(acc, ls["org"], ls["dr"], ls["rec"], "three")
    v, c = acc.area_lights_device(ls["org"], ls["dr"], ls["rec"], mk(lights), None, SEED)          # NULL parameters: eps 1e-5, bound 1, 16 samples
    e16 = pin(ls["oracle"], ls["O"], ls["Ns"], ls["ids"].astype(np.uint64), lights, 16)
    compare(ls, e16, host(v, np.uint32), host(c), "defaults")
    for kw in (dict(seed=SEED + 1), dict(eps=0.25)):
        for fused in (1, 0):
            m, v = area(acc, ls["org"], ls["dr"], ls["rec"], "three", fused, **kw)
            assert not same_bits(v, base[1]) and (m != base[0]).any(), kw
    # uniforms of the caller's own: the expectation follows them
    rng = np.random.default_rng(3)
    X = rng.random((ls["ids"].shape[0], len(lights), S, 3))
    e = pin(ls["oracle"], ls["O"], ls["Ns"], None, lights, S, X=X)
    m, v = area(acc, ls["org"], ls["dr"], ls["rec"], "three", 1, uniforms=dev(X.reshape(-1)))
    compare(ls, e, m, v, "own uniforms")
    # keys of the caller's own
    keys = (np.arange(ls["n"], dtype=np.uint64) * np.uint64(977) + np.uint64(5)) | (np.uint64(9) << np.uint64(34))
    e = pin(ls["oracle"], ls["O"], ls["Ns"], keys[ls["ids"]], lights, S)
    for fused in (1, 0):
        m, v = area(acc, ls["org"], ls["dr"], ls["rec"], "three", fused, key=dev(keys))
        compare(ls, e, m, v, ("keys", fused))


# ---- 3. the rays alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "many"])
def test_the_rays_alone_and_a_bounded_any_hit_launch_reproduce_the_bits(ls, name):
    import torch
    acc = ls["acc"]; n = ls["n"]
    lights, S = SETS[name]; L = len(lights)
    e = expected(ls, name)
    so, ns, ro, rd, rt, rw = acc.area_light_rays_device(ls["org"], ls["dr"], ls["rec"], mk(lights), prm(S), SEED)
    torch.cuda.synchronize()
    nslots = int(host(ns, np.uint32)[0])
    assert nslots == ls["ids"].shape[0]
    escan = np.full(n, NO_HIT, np.uint32); escan[ls["ids"]] = np.arange(nslots, dtype=np.uint32)
    assert np.array_equal(host(so, np.uint32), escan)
    m = nslots * L * S
    go, gd = host(ro)[:m].reshape(nslots, L, S, 3), host(rd)[:m].reshape(nslots, L, S, 3)
    gt, gw = host(rt)[:m].reshape(nslots, L, S), host(rw)[:m].reshape(nslots, L, S)
    assert np.array_equal(go.view(np.uint64), np.ascontiguousarray(np.broadcast_to(ls["O"][:, None, None, :], go.shape)).view(np.uint64))
    assert np.array_equal(gd.view(np.uint64), np.ascontiguousarray(e["D"]).view(np.uint64))
    assert np.array_equal(gt.view(np.uint64), np.ascontiguousarray(e["T"]).view(np.uint64))
    assert np.array_equal(gw.view(np.uint64), np.ascontiguousarray(e["W"]).view(np.uint64))
    occ = acc.intersect_device(ro[:m].contiguous(), rd[:m].contiguous(), mode=la.MODE_ANY, tmax=rt[:m].contiguous())[0]
    torch.cuda.synchronize()
    occ = host(occ).reshape(nslots, L, S)
    assert np.array_equal(occ != 0, e["occ"] != 0)
    assert (occ[gt == 0.0] == 0).all()          # a dead bound: the launch answers 0, the byte the stage leaves for an item it does not trace
    # the weighted mean by hand gives the stage's mask
    open_ = (gt > 0.0) & (occ == 0)
    by_hand = (open_.any(axis=2).astype(np.uint32) << np.arange(L, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
    stage, _ = area(acc, ls["org"], ls["dr"], ls["rec"], name, 1)
    assert np.array_equal(by_hand, stage[ls["ids"]])
    with pytest.raises(la.LucilleHipError, match="capacity_rays"):
        acc.area_light_rays_device(ls["org"], ls["dr"], ls["rec"], mk(lights), prm(S), SEED, out=(so, ns, ro[:m - 1], rd, rt, rw))
    # replayed uniforms and no weights
    uni = dev(np.ascontiguousarray(e["X"]).reshape(-1))
    out = acc.area_light_rays_device(ls["org"], ls["dr"], ls["rec"], mk(lights), prm(S), 99, uniforms=uni, out=(so, ns, ro, torch.zeros_like(rd), rt, None))
    torch.cuda.synchronize()
    assert np.array_equal(host(out[3])[:m].view(np.uint64), gd.reshape(m, 3).view(np.uint64))


# ---- 4. lists ---------------------------------------------------------------------------------------------------------------------------------
def test_lists_write_the_listed_slots_alone(ls):
    import torch
    acc = ls["acc"]; n = ls["n"]
    org, dr, rec = ls["org"], ls["dr"], ls["rec"]
    full_m, full_v = area(acc, org, dr, rec, "three")

    def check(index, count, listed, fused):
        out = poison(n)
        m, v = area(acc, org, dr, rec, "three", fused, index=index, count=count, out=out)
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
    lights, S = SETS["three"]
    vis = torch.full((n,), POISON32, dtype=torch.int32, device="cuda")
    acc.area_lights_device(org, dr, rec, mk(lights), prm(S), SEED, out=(vis, None))
    assert np.array_equal(host(vis, np.uint32), full_m)
    rgb = torch.full((n, 3), POISONF, dtype=torch.float32, device="cuda")
    acc.area_lights_device(org, dr, rec, mk(lights), prm(S), SEED, out=(None, rgb))
    assert same_bits(host(rgb), full_v)
    with pytest.raises(ValueError):
        acc.area_lights_device(org, dr, rec, mk(lights), prm(S), SEED, out=(None, None))


# ---- 5. small and empty -------------------------------------------------------------------------------------------------------------------------
def test_one_ray(ls):
    """n_rays = 1: a hit and a miss, both paths; the key is the ray's own (its id in the big batch)"""
    acc = ls["acc"]
    hit_id = int(ls["ids"][0]); miss_id = int(np.nonzero(ls["prim"] == po.MISS)[0][0])
    for name in ("one16", "three"):
        full = area(acc, ls["org"], ls["dr"], ls["rec"], name)
        for i in (hit_id, miss_id):
            o, d = ls["org"][i:i + 1].contiguous(), ls["dr"][i:i + 1].contiguous()
            rec = tuple(x[i:i + 1].contiguous() for x in ls["rec"])
            for fused in (1, 0):
                m, v = area(acc, o, d, rec, name, fused, key=dev(np.array([i], np.uint64)))
                assert m[0] == full[0][i] and same_bits(v[0], full[1][i]), (i, name, fused)
        assert full[0][miss_id] == NO_HIT and full[0][hit_id] != NO_HIT


def test_empty_scene_and_no_rays(ls):
    import torch
    e = la.HipAccel(0); e.commit()
    try:
        e.set_emitters(TABLE)
        lights, S = SETS["three"]
        n = 100
        org, dr = ls["org"][:n].contiguous(), ls["dr"][:n].contiguous()
        rec = tuple(x[:n].contiguous() for x in ls["rec"])          # records of another scene: an empty scene reads none of them
        out = poison(n)
        m, v = area(e, org, dr, rec, "three", 1, out=out)
        assert (m == NO_HIT).all() and (v == 0.0).all()
        lst = np.array([5, 5, 99, 100, 7], np.uint32)
        out = poison(n)
        m, v = area(e, org, dr, rec, "three", 1, index=dev(lst), out=out)
        listed = np.zeros(n, bool); listed[[5, 99, 7]] = True
        assert (m[listed] == NO_HIT).all() and (m[~listed] == POISON32).all() and (v[~listed] == np.float32(POISONF)).all()
        so, ns = e.area_light_rays_device(org, dr, rec, mk(lights), prm(S))[:2]; torch.cuda.synchronize()
        assert int(host(ns)[0]) == 0 and (host(so, np.uint32) == NO_HIT).all()
        hv, hr = e.area_lights_host(host(org), host(dr), tuple(host(x) for x in rec), mk(lights), prm(S))
        assert (hv == NO_HIT).all() and (hr == 0.0).all()
    finally:
        e.close()
    z = ls["org"][:0].contiguous()
    m, v = ls["acc"].area_lights_device(z, z, tuple(x[:0].contiguous() for x in ls["rec"]), mk(SETS["one1"][0]), prm(1))
    assert m.shape[0] == 0 and tuple(v.shape) == (0, 3)


def test_host_form_equals_the_device_form(ls):
    acc = ls["acc"]
    hrec = (host(ls["rec"][0], np.uint32), host(ls["rec"][1]), host(ls["rec"][2]), host(ls["rec"][3]))
    for name in ("three", "many"):
        lights, S = SETS[name]
        m, v = area(acc, ls["org"], ls["dr"], ls["rec"], name)
        hm, hv = acc.area_lights_host(ls["horg"], ls["hdr"], hrec, mk(lights), prm(S), SEED)
        assert np.array_equal(hm, m) and same_bits(hv, v), name
        e = expected(ls, name)
        uni = np.zeros(3 * len(lights) * S * ls["n"])          # the host form asks for the worst case: every ray hits
        uni[:e["X"].size] = np.ascontiguousarray(e["X"]).reshape(-1)
        hm, hv = acc.area_lights_host(ls["horg"], ls["hdr"], hrec, mk(lights), prm(S), 4242, uniforms=uni)
        assert np.array_equal(hm, m) and same_bits(hv, v), name
    with pytest.raises(la.LucilleHipError, match="uniforms given"):
        acc.area_lights_host(ls["horg"], ls["hdr"], hrec, mk(SETS["three"][0]), prm(4), SEED, uniforms=np.zeros(3 * 3 * 4 * ls["n"] - 1))


# ---- 6. emitters that are scene geometry too ------------------------------------------------------------------------------------------------
def test_an_emitter_in_the_scene_does_not_shadow_itself_under_a_bound_below_one(ls):
    """the quad added to the scene as a mesh.  At bound 1 the emitter closes about half of the rays that reach it (pos, rounded to float, lies on
    either side of its plane); under bound = 1 - 1e-4 those rays end in front of it and are open -- all but the rays that START on the emitter and run
    in its plane, whose t is not near 1.  The oracle says which; the device must say the same, either way"""
    quad = TABLE[QUAD[0]:QUAD[0] + QUAD[1]]
    qP = quad.reshape(-1, 3); qI = np.arange(qP.shape[0], dtype=np.uint32)
    acc = la.HipAccel(0); acc.add_mesh(ls["P"], ls["idx"]); acc.add_mesh(qP, qI); acc.commit(); acc.wait_exact()
    try:
        acc.set_emitters(TABLE)
        o = po.Oracle(); o.add_mesh(ls["P"], ls["idx"]); o.add_mesh(qP, qI); o.build()
        h = hits_of(acc, ls["horg"], ls["hdr"])
        nsoup = ls["idx"].shape[0] // 3
        lights, S = [(QUAD[0], QUAD[1], (3.0, 2.0, 1.0), INVSQ | PDF)], 4
        closed = {}
        for bound in (1.0, 1.0 - 1e-4):
            e = pin(o, h["O"], h["Ns"], h["ids"].astype(np.uint64), lights, S, bound=bound)
            own = (e["prim"] >= nsoup) & (e["prim"] != po.MISS)          # the ray's first hit is the emitter
            c = e["occ"][e["go"]][own] != 0
            on_emitter = h["prim"][h["ids"]][np.nonzero(e["go"])[0][own]] >= nsoup
            closed[bound] = int(c.sum())
            print("bound %.17g: %d rays reach the emitter first, it closes %d of them (%d of those start on it)" % (bound, int(own.sum()), closed[bound], int(c[on_emitter].sum())))
            assert own.sum() > 1000
            if bound < 1.0:
                assert not c[~on_emitter].any()
            for fused in (1, 0):
                m, v = area(acc, h["org"], h["dr"], h["rec"], (lights, S), fused, bound=bound)
                compare(h, e, m, v, (bound, fused))
        assert closed[1.0] > 10 * closed[1.0 - 1e-4]
    finally:
        acc.close()


# ---- 7. rays that the persistent walk does not finish -------------------------------------------------------------------------------------------
def test_short_stacks_and_a_small_budget_go_through_the_cooperative_walk(ls):
    """an accelerator of its own on the same soup with "stack_cap" 8 and "ao_budget" 4: most traced items leave the persistent walk for the fix-up queue
    and the cooperative walk, which makes ray and bound again from the item index and stores the same byte"""
    acc = la.HipAccel(0); acc.add_mesh(ls["P"], ls["idx"]); acc.commit(); acc.wait_exact()
    try:
        acc.set_emitters(TABLE)
        acc.set_param("stack_cap", 8); acc.set_param("ao_budget", 4)
        acc.trace_statistics(True)
        for name in ("three", "many"):
            acc.statistics(clear=True)
            m, v = area(acc, ls["org"], ls["dr"], ls["rec"], name)
            s = acc.statistics(clear=True)
            queued = int(acc.L.lh_accel_last_retraced(acc.h))
            e = expected(ls, name)
            print("%s: %d of %d items through the queue (%d traced)" % (name, queued, s["rays"], int((e["T"] > 0).sum())))
            assert 0 < queued <= int((e["T"] > 0).sum())
            compare(ls, e, m, v, name)
    finally:
        acc.close()


# ---- 8. statistics ------------------------------------------------------------------------------------------------------------------------------
def test_statistics_count_the_work_items(ls):
    """with trace statistics on, `rays` advances by hits x L x S -- work items, traced or not -- and `hits` (counters[4]) by the items that are not open"""
    acc = ls["acc"]
    acc.trace_statistics(True)
    try:
        for name in ("one16", "three"):
            lights, S = SETS[name]; nslots = ls["ids"].shape[0]
            e = expected(ls, name)
            for fused in (1, 0):
                acc.statistics(clear=True)
                area(acc, ls["org"], ls["dr"], ls["rec"], name, fused)
                st = acc.statistics(clear=True)
                assert st["rays"] == nslots * len(lights) * S and st["hits"] == int(e["closed"].sum()), (name, fused, st)
    finally:
        acc.trace_statistics(False)


# ---- 9. the table: replaced, removed, kept across a re-commit -----------------------------------------------------------------------------------
def test_replacing_and_removing_the_table_between_calls(ls):
    acc = la.HipAccel(0); acc.add_mesh(ls["P"], ls["idx"]); acc.commit(); acc.wait_exact()
    try:
        lights, S = SETS["one16"]
        with pytest.raises(la.LucilleHipError, match="bad area lights"):          # no table yet: every run leaves it
            area(acc, ls["org"], ls["dr"], ls["rec"], "one16")
        acc.set_emitters(TABLE)
        a = area(acc, ls["org"], ls["dr"], ls["rec"], "one16")
        compare(ls, expected(ls, "one16"), *a)
        moved = TABLE[:1] + np.array([0.7, 0.4, -0.6])
        acc.set_emitters(moved)                                                    # replaced by a table of one triangle elsewhere
        e = pin(ls["oracle"], ls["O"], ls["Ns"], ls["ids"].astype(np.uint64), lights, S, table=moved)
        for fused in (1, 0):
            b = area(acc, ls["org"], ls["dr"], ls["rec"], "one16", fused)
            compare(ls, e, *b)
        assert not same_bits(a[1], b[1])
        with pytest.raises(la.LucilleHipError, match="bad area lights"):          # "three" reaches beyond the one triangle
            area(acc, ls["org"], ls["dr"], ls["rec"], "three")
        acc.set_emitters(None)
        with pytest.raises(la.LucilleHipError, match="bad area lights"):
            area(acc, ls["org"], ls["dr"], ls["rec"], "one16")
        acc.set_emitters(TABLE.reshape(-1, 9))
        c = area(acc, ls["org"], ls["dr"], ls["rec"], "one16")
        assert np.array_equal(a[0], c[0]) and same_bits(a[1], c[1])
        bad = TABLE.copy(); bad[5, 1, 2] = np.nan
        with pytest.raises(la.LucilleHipError, match="bad emitters"):
            acc.set_emitters(bad)
        c = area(acc, ls["org"], ls["dr"], ls["rec"], "one16")                     # a refused table leaves the old one
        assert np.array_equal(a[0], c[0]) and same_bits(a[1], c[1])
    finally:
        acc.close()


def test_the_table_is_kept_across_a_recommit(ls):
    import torch
    P = torch.from_numpy(np.ascontiguousarray(ls["P"])).cuda()
    I = torch.from_numpy(np.ascontiguousarray(ls["idx"], np.uint32).view(np.int32)).cuda()
    acc = la.HipAccel(0)
    try:
        acc.set_param("updatable", 1)
        acc.add_mesh_device(P, I)
        acc.commit()
        acc.set_emitters(TABLE)
        ref = area(ls["acc"], ls["org"], ls["dr"], ls["rec"], "three")
        a = area(acc, ls["org"], ls["dr"], ls["rec"], "three")
        assert np.array_equal(a[0], ref[0]) and same_bits(a[1], ref[1])
        acc.update_mesh_device(0, P)
        acc.recommit()
        for fused in (1, 0):
            b = area(acc, ls["org"], ls["dr"], ls["rec"], "three", fused)
            assert np.array_equal(b[0], ref[0]) and same_bits(b[1], ref[1])
    finally:
        acc.close()


# ---- 10. the tile ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1():
    return load_case("ao_c1")


@pytest.mark.parametrize("pxs", [1, 2])
def test_tile_equals_the_batch_values_and_does_not_depend_on_tiling(c1, pxs):
    """lh_render_area_lights_tile == lh_render_primary_rays -> lh_accel_intersect_device -> lh_accel_area_lights_device with key = absolute sample
    position -> per sample the hit's three floats, widened, added over the pixel's sub-samples in sample order, scaled, converted, clamped and written
    as the light tile's"""
    import torch
    acc, cam = c1["acc"], c1["cam"]
    T, S = 64, 4
    x0, y0 = (cam.width - T) // 2, (cam.height - T) // 2
    spp = pxs * pxs
    org, dr = acc.primary_rays(cam, x0, y0, T, T, pxs)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    # emitters around the camera's scene, whatever its scale: placed from the hits' own bounding box
    prim = host(rec[0], np.uint32); hit = prim != po.MISS
    Pn = (host(org) + host(dr) * host(rec[1])[:, None])[hit]
    lo, hi = Pn.min(axis=0), Pn.max(axis=0); c = 0.5 * (lo + hi); r = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(9)
    table = np.concatenate([c + np.array([0.3, 0.8, 0.2]) * r + 0.15 * r * rng.standard_normal((2, 3, 3)),
                            c + np.array([-0.6, 0.5, -0.4]) * r + 0.1 * r * rng.standard_normal((5, 3, 3))])
    acc.set_emitters(table)
    try:
        sets = ([(0, 2, (3.0, 2.0, 1.0), COSINE), (2, 5, (0.5, 1.0, 2.0), COSINE | INVSQ | PDF), (0, 7, (0.2, 0.4, 0.9), 0)], S)
        i = np.arange(T * T * spp, dtype=np.int64)
        ipix = i // spp
        key = dev(((y0 + ipix // T) * cam.width + (x0 + ipix % T)) * spp + (i - ipix * spp))
        m, v = area(acc, org, dr, rec, sets, 1, seed=5, key=key)
        nslots = int(hit.sum())
        acc.trace_statistics(True)
        try:
            acc.statistics(clear=True)
            area(acc, org, dr, rec, sets, 1, seed=5, key=key)
            closed = acc.statistics(clear=True)["hits"]
        finally:
            acc.trace_statistics(False)
        assert 0 < closed < nslots * 3 * S and (v[hit] > 0).any()
        per = v.astype(np.float64).reshape(T * T, spp, 3)
        accum = np.zeros((T * T, 3))
        for q in range(spp):
            accum = accum + per[:, q, :]
        exp = np.maximum((accum * (1.0 / spp)).astype(np.float32), np.float32(0.0)).reshape(T, T, 3)[::-1]
        for fused in (1, 0):
            acc.set_param("ao_fused", fused)
            try:
                rgb, st = acc.render_area_lights_tile(cam, x0, y0, T, T, pxs, mk(sets[0]), prm(S), 5)
            finally:
                acc.set_param("ao_fused", 1)
            rgb = host(rgb).copy()
            assert 0 < nslots == st["primary_hits"] and st["primary_rays"] == T * T * spp and st["ao_rays"] == nslots * 3 * S
            assert st["ao_occluded"] == closed
            assert same_bits(rgb, exp), (fused, int((rgb != exp).sum()))
        assert (rgb[:, :, 0] != rgb[:, :, 2]).any()
        tot = {k: 0 for k in st}
        for ty in (0, 1):
            for tx in (0, 1):
                q, sq = acc.render_area_lights_tile(cam, x0 + 32 * tx, y0 + 32 * ty, 32, 32, pxs, mk(sets[0]), prm(S), 5)
                assert same_bits(host(q), rgb[T - 32 * (ty + 1):T - 32 * ty, 32 * tx:32 * (tx + 1)]), (tx, ty)
                for k in tot:
                    tot[k] += sq[k]
        assert tot == st
        q, sq = acc.render_area_lights_tile(cam, x0, y0 + 3, T, 17, pxs, mk(sets[0]), prm(S), 5)          # an odd tiling of the same frame
        assert same_bits(host(q), rgb[T - 20:T - 3])
    finally:
        acc.set_emitters(None)
