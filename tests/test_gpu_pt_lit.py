"""The path tracer with direct light from a light list and a path-vertex sink (lh_render_pt_tile_lit / lh_render_pt_bands_lit; the rule:
lucille_amd/csrc/lh_ptl.h, restated in tests/test_ptl_rule.py) on the device.

The oracle's path tracer knows no lights.  What ties the lit frame down is COMPOSITION: the sink hands out every entry of every bounce; the
sink is tied to the oracle (records per path, counts per bounce, the radiance of every path that ends in a miss, every record retraced by
lh_accel_intersect_device); the oracle-pinned lh_accel_lights_device on the sink's hit records gives `value`; the rule in numpy float32 gives
every hit's r; and the frame is the integer sum of pt_fix_np over the miss records' environment terms and the hit records' direct terms,
converted as pixel_from_paths converts -- all bit for bit: the pixel sums are integers, no order of additions needs stating.

The hand-derivable frame's light shines straight along +z: a shadow ray with dir.y = 0, which the reference leaves undefined; the device gives
that axis the value the other axes get (lh_reftrace.h), and the answers the test asks for (open above the lone plane, shut below it by the
plane itself) are the only ones any walk can give there."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from tests import pt_cases as pc
from tests.test_lights_rule import items, origins
from tests.test_ptl_rule import colour, direct

pytestmark = pytest.mark.gpu

REACH_BAR = pc.REACH_BAR
ENV = (0.9, 0.8, 0.7)
MISS = 0xFFFFFFFF

# the light lists.  The plane of ao_ps lies at z = -0.586 (normal +z), the sphere (radius 1.59) around (2.69, -2.03, 1.74), the camera looks
# down on both from (7.5, -6.5, 5.3): a light towards (-0.5, 0.6, 1) throws the sphere's shadow onto the plane between sphere and camera
SLANTED = la.Light((-0.5, 0.6, 1.0), (1.5, 1.0, 0.5), la.LIGHT_COSINE)
POINT = la.Light((5.5, -5.0, 4.0), (40.0, 30.0, 20.0), la.LIGHT_POINT | la.LIGHT_COSINE | la.LIGHT_INVSQ)


def _many():
    rng = np.random.default_rng(31)
    out = [SLANTED, POINT]
    for k in range(29):
        rgb = rng.uniform(0.02, 0.3, 3)
        if k % 3 == 0:
            pos = np.array([rng.uniform(-5, 6), rng.uniform(-6, 5), rng.uniform(0.5, 6.0)])
            out.append(la.Light(pos, rgb * 20.0, la.LIGHT_POINT | (la.LIGHT_COSINE if k % 2 else 0) | (la.LIGHT_INVSQ if k % 4 == 0 else 0)))
        else:
            out.append(la.Light((rng.uniform(-1, 1), rng.uniform(0.1, 1) * rng.choice([-1, 1]), rng.uniform(0.2, 1.5)), rgb, la.LIGHT_COSINE if k % 2 else 0))
    assert len(out) == 31
    return out


LISTS = {"L1": [SLANTED], "L2": [POINT, SLANTED], "L31": _many()}


def lit_case(w, h, spp, max_vertices, tile=None, seed=21):
    """ao_ps with GLASS on the sphere and diffuse on the coloured plane"""
    c = dict(pc.sum_case(w, h, spp))
    c.update(name="lit %d x %d x %d, %d vertices" % (w, h, spp, max_vertices), mats=[list(pc.GLASS), list(pc.mat(kd=pc.DIFFUSE))],
             max_vertices=max_vertices, seed=seed, tile=tile or (0, 0, w, h))
    return c


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(meshes):
        if id(meshes) not in made:
            made[id(meshes)] = (pc.accel_of(meshes), pc.oracle_of(meshes))
        return made[id(meshes)]
    yield get
    for acc, _ in made.values():
        acc.close()


def setup(acc, case, env_rgb=ENV, env_map=None):
    for k, m in enumerate(case["mats"]):
        acc.set_material(k, pc.la_material(m))
    acc.set_environment(env_rgb, env_map)


def total_records(o, case, env_rgb=ENV, env_map=None):
    return int(pc.render_oracle(o, case, 0, env_rgb, env_map)[1]["rays"])


def lit(acc, case, lights=(), sink=None, params=None, tile=None, flags=0):
    x0, y0, w, h = tile or case["tile"]
    img, st = acc.render_pt_tile_lit(pc.cameras(case["cam"])[0], x0, y0, w, h, 0, case["spp"], case["spp"], max_vertices=case["max_vertices"], flags=flags,
                                     lights=lights, params=params, sink=sink, seed=case["seed"])
    return img.cpu().numpy(), st


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b, what):
    bad = np.argwhere(bits(a) != bits(b))
    assert bad.shape[0] == 0, "%s: %d of %d words differ, first at %s: %r / %r" % (what, bad.shape[0], a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


# ---- the composition ---------------------------------------------------------------------------------------------------------------------
def frame_from_terms(pix, terms, w, h, spp_total):
    """pixel_from_paths for terms that come several to a path: the int64 sum of pt_fix_np per pixel and channel over the terms that are neither
    NaN nor 0, converted once; [h, w, 3], top line first"""
    terms = np.asarray(terms, np.float32)
    valid = (terms == terms) & (terms != 0.0)
    with np.errstate(invalid="ignore"):
        fix = np.where(valid, pc.pt_fix_np(np.where(valid, terms, np.float32(0.0))), np.int64(0))
    acc = np.zeros((w * h, 3), np.int64)
    np.add.at(acc, pix, fix)
    s = (acc.astype(np.float64) * 2.3283064365386963e-10).astype(np.float32)
    inv = np.float32(1.0) / np.float32(spp_total)
    return np.ascontiguousarray((np.float32(0.0) + s * inv).reshape(h, w, 3)[::-1])


def materials_of(acc, case, prim):
    """-> (kd float32 [n, 3], mesh [n], triangle of the mesh [n]) of hit records; misses get mesh 0"""
    mesh = np.zeros(prim.shape[0], np.int64); tri = np.zeros(prim.shape[0], np.int64)
    for p in np.unique(prim[prim != MISS]):
        m, i = acc.prim_lookup(int(p))          # i: the triangle's place in the mesh's index list, 3 x its number
        mesh[prim == p] = m; tri[prim == p] = i // 3
    kd = np.array([m[0:3] for m in case["mats"]], np.float32)[mesh]
    return kd, mesh, tri


def colours_of(case, mesh, tri, u, v):
    """the three colour lines of pt_scatter for every record: 1 where the mesh has no colours"""
    col = np.ones((mesh.shape[0], 3), np.float32)
    for k, m in enumerate(case["meshes"]):
        if "C" not in m:
            continue
        sel = np.flatnonzero(mesh == k)
        ix = m["idx"].reshape(-1, 3)[tri[sel]]
        col[sel] = colour(m["C"][ix[:, 0]], m["C"][ix[:, 1]], m["C"][ix[:, 2]], u[sel], v[sel])
    return col


def expected(acc, case, sink, lights, params, env_rgb=ENV):
    """the sink's records -> (records, hit mask, value, visible, expected direct per record, expected frame)"""
    rec = sink.records()
    n = rec["prim"].shape[0]
    assert sink.total() == n <= sink.capacity
    hit = rec["prim"] != MISS
    val = np.zeros((n, 3), np.float32); vis = np.zeros(n, np.uint32)
    if lights:
        gv, gr = acc.lights_device(sink.org[:n], sink.dir[:n], (sink.prim[:n], sink.t[:n], sink.u[:n], sink.v[:n]), lights, params)
        vis, val = gv.cpu().numpy().view(np.uint32), gr.cpu().numpy()
    kd, mesh, tri = materials_of(acc, case, rec["prim"])
    col = colours_of(case, mesh, tri, rec["u"], rec["v"])
    r = np.where(hit[:, None], direct(rec["thr"], kd, col, val), np.float32(0.0)).astype(np.float32)
    with np.errstate(all="ignore"):
        env = rec["thr"] * np.asarray(env_rgb, np.float32)[None, :]
    terms = np.where(hit[:, None], r, env)
    _, _, w, h = case["tile"]
    frame = frame_from_terms(rec["path"].astype(np.int64) // case["spp"], terms, w, h, case["spp"])
    return rec, hit, val, vis, r, frame


# ---- 1. unlit equality -----------------------------------------------------------------------------------------------------------------
def test_without_lights_or_sink_the_frame_is_the_unlit_one(scenes):
    s2 = pc.branch_cases()[2]
    assert s2["name"] == "S2 glass sphere"
    for case in (s2, pc.sum_case(23, 17, 65)):
        acc, _ = scenes(case["meshes"])
        setup(acc, case)
        x0, y0, w, h = case["tile"]
        cam = pc.cameras(case["cam"])[0]
        ref, rst = acc.render_pt_tile2(cam, x0, y0, w, h, 0, case["spp"], case["spp"], max_vertices=case["max_vertices"], seed=case["seed"])
        got, st = lit(acc, case)
        assert st == rst
        same(got, ref.cpu().numpy(), case["name"])
        # the bands three ranks would own, three lines each
        H, rows = cam.height, 3
        nb = H // rows
        for r in range(3):
            mine = len(range(r, nb, 3))
            a, sa = acc.render_pt_bands(cam, rows * r, rows, 3 * rows, mine, 0, case["spp"], case["spp"], max_vertices=case["max_vertices"], seed=case["seed"])
            b, sb = acc.render_pt_bands_lit(cam, rows * r, rows, 3 * rows, mine, 0, case["spp"], case["spp"], max_vertices=case["max_vertices"], seed=case["seed"])
            assert sa == sb
            same(b.cpu().numpy(), a.cpu().numpy(), "%s, bands of rank %d" % (case["name"], r))


# ---- 2. the sink against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", (False, True), ids=("constant", "probe"))
def test_the_sink_against_the_oracle(scenes, probe):
    """chain structure (records per path, counts per bounce), directions and throughputs (the radiance of every path that ends in a miss) and
    the records themselves (retraced), over all records of the S2 case"""
    import torch
    case = pc.branch_cases()[2]
    acc, o = scenes(case["meshes"])
    env_rgb, env_map = (pc.PROBE_RGB, pc.random_probe()) if probe else (ENV, None)
    _, est, per, rad, _ = pc.render_oracle(o, case, 0, env_rgb, env_map)
    setup(acc, case, env_rgb, env_map)
    sink = la.PtSink(est["rays"], case["max_vertices"])
    got, st = lit(acc, case, sink=sink)
    assert st == est
    rec = sink.records()
    n = rec["prim"].shape[0]
    assert n == est["rays"] == sink.total()
    per = per.reshape(-1).astype(np.int64); rad = rad.reshape(-1, 3)
    # records per path, counts per bounce, depths in blocks
    assert np.array_equal(np.bincount(rec["path"], minlength=per.shape[0]), per)
    counts = np.array([(per > d).sum() for d in range(case["max_vertices"])], np.uint32)
    assert np.array_equal(rec["counts"], counts) and counts[-1] == 0
    assert np.array_equal(rec["depth"], np.repeat(np.arange(case["max_vertices"], dtype=np.uint32), counts))
    assert (rec["direct"] == 0.0).all()
    # every path's records are its bounces 0 .. rays - 1, once each
    order = np.lexsort((rec["depth"], rec["path"]))
    first = np.concatenate([[0], np.cumsum(per)[:-1]])
    assert np.array_equal(rec["depth"][order], np.arange(n) - np.repeat(first, per))
    # a path that ends in a miss: thr x env of its last record is the oracle's radiance
    last = order[np.cumsum(per) - 1]
    ends = rec["prim"][last] == MISS
    assert ends.sum() >= REACH_BAR and (rec["depth"][last][ends] > 0).sum() >= REACH_BAR
    if probe:
        env = acc.environment_device(sink.dir[:n].contiguous()).cpu().numpy()[last]
    else:
        env = np.tile(np.asarray(env_rgb, np.float32), (last.shape[0], 1))
    with np.errstate(all="ignore"):
        lrad = rec["thr"][last] * env
    lrad = np.where((rec["depth"][last] == 0)[:, None], env, lrad)          # camera rays carry no throughput: the environment itself
    paths = rec["path"][last]
    nan = np.isnan(rad[paths][ends]) & np.isnan(lrad[ends])
    bad = (bits(lrad[ends]) != bits(rad[paths][ends])) & ~nan
    print("paths that end in a miss: %d, radiance words that differ: %d" % (int(ends.sum()), int(bad.sum())))
    assert not bad.any()
    assert (rad[paths][~ends] == 0.0).all()
    # the records, retraced
    p2, t2, u2, v2 = acc.intersect_device(sink.org[:n].contiguous(), sink.dir[:n].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(p2.cpu().numpy().view(np.uint32), rec["prim"])
    for name, x in (("t", t2), ("u", u2), ("v", v2)):
        same(x.cpu().numpy(), rec[name], "retraced " + name)
    # and the unlit frame is the composition of the miss records alone
    if not probe:
        same(got, expected(acc, case, sink, (), None, env_rgb)[5], "composition, no lights")


# ---- 3. the lit frame by composition -------------------------------------------------------------------------------------------------------
LIT = [("L1", 23, 17, 3, 2), ("L1", 23, 17, 3, 12), ("L2", 23, 17, 3, 2), ("L2", 23, 17, 3, 12), ("L31", 23, 17, 3, 2), ("L31", 23, 17, 3, 12),
       ("L2", 7, 5, 65, 12), ("L1", 7, 5, 1, 3)]


def check_lit(scenes, case, lights, params=None, bars=True):
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    sink = la.PtSink(total_records(o, case), case["max_vertices"])
    got, st = lit(acc, case, lights=lights, sink=sink, params=params)
    rec, hit, val, vis, r, frame = expected(acc, case, sink, lights, params)
    assert st["rays"] == rec["prim"].shape[0]
    same(rec["direct"], r, case["name"] + ": direct")
    same(got, frame, case["name"] + ": frame")
    if not bars:
        return rec, hit, r
    # non-vacuity: conditions, not measurements
    lit0 = int((hit & (rec["depth"] == 0) & (r != 0.0).any(axis=1)).sum()); lit1 = int((hit & (rec["depth"] >= 1) & (r != 0.0).any(axis=1)).sum())
    h = np.flatnonzero(hit)
    st24 = acc.state_build(rec["org"][h], rec["dir"][h], rec["prim"][h], rec["t"][h], rec["u"][h], rec["v"][h])
    eps = 1.0e-5 if params is None else params.eps
    O = origins(st24[:, 0:3], st24[:, 6:9], eps)
    shadow = np.zeros(h.shape[0], bool)
    for l, light in enumerate(lights):
        _, wl, tm = items(O, st24[:, 6:9], tuple(light.v), int(light.flags))
        shadow |= (tm > 0.0) & (wl > 0.0) & (((vis[h] >> l) & 1) == 0)
    glass = int((materials_of(acc, case, rec["prim"])[1][h] == 0).sum())
    print("%s, %d lights: lit hits at bounce 0: %d, later: %d; real shadows: %d; hits on the glass sphere: %d" % (case["name"], len(lights), lit0, lit1, int(shadow.sum()), glass))
    assert lit0 >= REACH_BAR and int(shadow.sum()) >= REACH_BAR and glass >= REACH_BAR
    if case["max_vertices"] > 2:          # two vertices: one bounce
        assert lit1 >= REACH_BAR
    return rec, hit, r


@pytest.mark.parametrize("name, w, h, spp, mv", LIT, ids=["%s %dx%dx%d v%d" % c for c in LIT])
def test_the_lit_frame_is_the_composition(scenes, name, w, h, spp, mv):
    """d_direct == the rule on lh_accel_lights_device's values, and the frame == the integer sums of the environment and direct terms, bit for
    bit; the light lists reach lit hits at the first and at later bounces, real shadows and the glass sphere.  spp 65: a pixel's run of paths
    straddles a wave in pt_accumulate; 7 x 5 x 1: fewer paths than a wave (no bars: 35 paths)"""
    check_lit(scenes, lit_case(w, h, spp, mv), LISTS[name], bars=w * h * spp >= 1000)


# ---- 4. invariances ------------------------------------------------------------------------------------------------------------------------
def test_invariances_of_the_lit_frame(scenes):
    import torch
    case = lit_case(23, 17, 3, 12)
    lights = LISTS["L2"]
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    cam = pc.cameras(case["cam"])[0]
    whole, st = lit(acc, case, lights=lights)
    # one tile == the same region as two tiles; a tile off the origin == its region of the frame
    left, sl = lit(acc, case, lights=lights, tile=(0, 0, 11, 17)); right, sr = lit(acc, case, lights=lights, tile=(11, 0, 12, 17))
    same(np.concatenate([left, right], axis=1), whole, "two tiles")
    assert sl["rays"] + sr["rays"] == st["rays"]
    x0, y0, w, h = 5, 3, 13, 9
    part, _ = lit(acc, case, lights=lights, tile=(x0, y0, w, h))
    same(part, whole[17 - y0 - h:17 - y0, x0:x0 + w], "the tile (5, 3, 13, 9)")
    # bands of 1 and 3 lines, stride 3 x rows: the lines three ranks would own
    for rows in (1, 3):
        nb = 17 // rows
        img = torch.zeros((nb, rows, 23, 3), dtype=torch.float32, device="cuda")
        for r in range(3):
            mine = len(range(r, nb, 3))
            out, _ = acc.render_pt_bands_lit(cam, rows * r, rows, 3 * rows, mine, 0, case["spp"], case["spp"], max_vertices=case["max_vertices"], lights=lights,
                                             seed=case["seed"])
            img[r::3] = out
        torch.cuda.synchronize()
        same(img.flip(0).reshape(nb * rows, 23, 3).cpu().numpy(), whole[17 - nb * rows:], "bands of %d" % rows)
    # materialised shadow rays == fused
    acc.set_param("ao_fused", 0)
    try:
        mat, sm = lit(acc, case, lights=lights)
    finally:
        acc.set_param("ao_fused", 1)
    same(mat, whole, "ao_fused 0")
    # a sink present == a sink absent, whichever arrays it has
    for fields in (None, ("prim",), ()):
        sink = la.PtSink(total_records(o, case), case["max_vertices"], fields=fields)
        with_sink, ss = lit(acc, case, lights=lights, sink=sink)
        same(with_sink, whole, "with a sink %s" % (fields,))
        assert ss == st and sink.total() == st["rays"]


# ---- 5. a hand-derivable frame ---------------------------------------------------------------------------------------------------------------
def test_a_frame_derived_by_hand(scenes):
    """the lone plane, a black environment, two vertices, one sample, one light without flags straight along the plane's normal: value = c, so a
    pixel that hits is pt_fix(kd x 1 x c), converted; a pixel that misses is 0.  From below with the light below, every pixel is 0: the origin
    lies eps above the plane and the hit's own triangle shadows it"""
    kd, c = (0.7, 0.6, 0.5), (1.25, 0.5, 3.0)
    meshes = pc.plane_meshes()
    acc, o = scenes(meshes)
    for eye_z, rh, toward in ((5.0, 1, 1.0), (-5.0, 0, -1.0)):
        case = pc._case("hand", meshes, [pc.mat(kd=kd)], pc.camera(24, 16, 0.08, pc.eye_matrix((0.0, 0.0, eye_z)), rh), 1, 3, (), max_vertices=2)
        setup(acc, case, (0.0, 0.0, 0.0))
        sink = la.PtSink(24 * 16, 2)
        got, st = lit(acc, case, lights=[la.Light((0.0, 0.0, toward), c)], sink=sink)
        rec = sink.records()
        assert rec["prim"].shape[0] == 24 * 16 and np.array_equal(rec["path"], np.arange(24 * 16))
        hit = rec["prim"] != MISS
        assert hit.sum() >= REACH_BAR and (~hit).sum() >= REACH_BAR
        r = (np.asarray(kd, np.float32) * np.float32(1.0)) * np.asarray(c, np.float32)
        model = np.where(hit[:, None], r[None, :], np.float32(0.0)).astype(np.float32) if toward > 0 else np.zeros((24 * 16, 3), np.float32)
        same(got, pc.frame_from_paths(model[:, None, :], 24, 16, 1), "light towards %+g" % toward)
        same(rec["direct"], model, "direct, light towards %+g" % toward)
        assert (got != 0.0).any() == (toward > 0)


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------------
def test_a_chain_with_empty_bounces(scenes):
    """chain plane 400, lit: every path has ended long before the limit -- bounces with count 0 go through the light stage's empty list, the
    read-back after the 8th bounce ends the chain, the sink's counts are written all the same"""
    case = [c for c in pc.chain_cases() if c["name"] == "chain plane 400"][0]
    acc, o = scenes(case["meshes"])
    _, est, per, _, _ = pc.render_oracle(o, case, 0, ENV, None)
    rec, hit, r = check_lit(scenes, case, [la.Light((0.3, 0.4, 1.0), (0.5, 0.25, 1.0), la.LIGHT_COSINE)], bars=False)
    per = per.reshape(-1).astype(np.int64)
    counts = np.array([(per > d).sum() for d in range(400)], np.uint32)
    assert np.array_equal(rec["counts"], counts) and (counts[:8] == 0).any() and rec["prim"].shape[0] == est["rays"]
    assert (hit & (r != 0.0).any(axis=1)).sum() >= REACH_BAR


@pytest.mark.parametrize("name", ("chain 10", "chain 18"))
def test_long_chains_between_two_planes(scenes, name):
    """slab_meshes(): reflectance 1 between two facing planes, most paths alive up to the vertex limit -- full bounces either side of pt_tile's count
    read-backs after bounces 7 and 15, the ray, path-word and throughput sets swapped many times while the counts stay high, hits that end at the
    vertex limit far from the camera.  One point light between the planes: both normals point up, so the lower plane (the even bounces) is lit and
    the upper one shadows itself"""
    case = [c for c in pc.chain_cases() if c["name"] == name][0]
    light = la.Light((3.0, 2.0, 10.0), (50.0, 25.0, 100.0), la.LIGHT_POINT | la.LIGHT_COSINE | la.LIGHT_INVSQ)
    rec, hit, r = check_lit(scenes, case, [light], bars=False)
    nz = hit & (r != 0.0).any(axis=1)
    late = int((nz & (rec["depth"] >= 8)).sum()); at_limit = int((nz & (rec["depth"] == case["max_vertices"] - 2)).sum())
    dark = int((hit & ~nz & (rec["depth"] >= 8)).sum())
    print("%s: lit hits at bounce >= 8: %d, of them at the last bounce: %d; unlit hits at bounce >= 8: %d; entries per bounce %s" % (
        name, late, at_limit, dark, [int(x) for x in rec["counts"][:case["max_vertices"] - 1]]))
    assert late >= REACH_BAR and rec["counts"][8] >= 256          # behind the first read-back the chain is still more than four waves wide
    if case["max_vertices"] == 10:
        assert at_limit >= REACH_BAR                               # bounce 8 is the last: lit hits whose paths end at the vertex limit
    else:
        # bounces 9 .. 16: the upper plane's hits stay dark, the lower plane's are lit up to and beyond the second read-back (26 entries are left there)
        assert dark >= REACH_BAR and (nz & (rec["depth"] >= 10)).sum() >= REACH_BAR and at_limit >= 1


def test_a_sink_smaller_than_the_pass(scenes):
    """the counts are true, nothing at or behind the capacity is written, the records below it are the pass's"""
    import torch
    case = lit_case(23, 17, 3, 12)
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    total = total_records(o, case)
    full = la.PtSink(total, case["max_vertices"])
    ref, _ = lit(acc, case, lights=LISTS["L1"], sink=full)
    small = la.PtSink(total, case["max_vertices"])
    for k in small.FIELDS:
        getattr(small, k).view(torch.uint8).fill_(0x77)
    cap = total // 2 + 1
    s = small.struct(); s.capacity = cap
    got, st = lit(acc, case, lights=LISTS["L1"], sink=s)
    same(got, ref, "frame")
    assert small.total() == total == st["rays"] and np.array_equal(small.counts.cpu().numpy(), full.counts.cpu().numpy())
    for k in small.FIELDS:
        a = getattr(small, k).cpu().numpy()
        assert (a[cap:].view(np.uint8) == 0x77).all(), k
        assert not (a[:cap].reshape(cap, -1).view(np.uint8) == 0x77).all(axis=1).any(), k
    # bounce 0 is in path order: those records are the full sink's; all of them retrace
    n0 = min(cap, 23 * 17 * 3)
    for k in small.FIELDS:
        same(getattr(small, k)[:n0].cpu().numpy(), getattr(full, k)[:n0].cpu().numpy(), k)
    p2, t2, u2, v2 = acc.intersect_device(small.org[:cap].contiguous(), small.dir[:cap].contiguous())
    assert np.array_equal(p2.cpu().numpy(), small.prim[:cap].cpu().numpy())
    for name, x in (("t", t2), ("u", u2), ("v", v2)):
        same(x.cpu().numpy(), getattr(small, name)[:cap].cpu().numpy(), "retraced " + name)


def test_refusals_enqueue_nothing(scenes):
    import torch
    case = lit_case(7, 5, 1, 3)
    acc, _ = scenes(case["meshes"])
    setup(acc, case)
    cam = pc.cameras(case["cam"])[0]
    out = torch.full((5, 7, 3), 7.0, dtype=torch.float32, device="cuda")
    bout = torch.full((5, 1, 7, 3), 7.0, dtype=torch.float32, device="cuda")
    sink = la.PtSink(64, 3)

    def refused(msg, lights=(), sink=None):
        for call in (lambda: acc.render_pt_tile_lit(cam, 0, 0, 7, 5, 0, 1, 1, max_vertices=3, lights=lights, sink=sink, out=out),
                     lambda: acc.render_pt_bands_lit(cam, 0, 1, 1, 5, 0, 1, 1, max_vertices=3, lights=lights, sink=sink, out=bout)):
            with pytest.raises(la.LucilleHipError) as e:
                call()
            assert all(m in str(e.value) for m in msg), str(e.value)

    refused(("bad lights",), [la.Light((0, 1, 1), (1, 1, 1))] * 32)
    refused(("bad lights",), [la.Light((0, 1, 1), (1, float("nan"), 1))])
    refused(("bad lights",), [la.Light((0, 1, 1), (1, 1, 1), la.LIGHT_INVSQ)])
    for field, msg in (("d_org", "not 8-byte aligned"), ("d_prim", "not 4-byte aligned")):
        s = sink.struct(); setattr(s, field, getattr(s, field) + 2)
        refused(("sink", msg), [SLANTED], s)
    rc = acc.L.lh_render_pt_tile_lit(acc.h, C.byref(cam), 0, 0, 7, 5, 0, 1, 1, 3, 0, None, 2, None, None, 1, C.c_void_p(out.data_ptr()), None, None)
    assert rc == -1 and "bad lights" in acc.L.lh_last_error().decode()
    # with lights every entry of every bounce may add a term to its pixel's sums: 11 samples x 399 bounces are more than the 4096 they hold
    with pytest.raises(la.LucilleHipError) as e:
        acc.render_pt_tile_lit(cam, 0, 0, 7, 5, 0, 11, 11, max_vertices=400, lights=[SLANTED], out=out)
    assert "4096" in str(e.value) and "lh_render_pt_tile_lit" in str(e.value)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (bout == 7.0).all() and sink.total() == 0
    unlit, _ = acc.render_pt_tile_lit(cam, 0, 0, 7, 5, 0, 11, 11, max_vertices=400)          # ... without lights the pass is the unlit one's
    assert (unlit.cpu().numpy() != 0.0).any()
    # and the same arguments, made good, render
    got, _ = acc.render_pt_tile_lit(cam, 0, 0, 7, 5, 0, 1, 1, max_vertices=3, lights=[SLANTED], sink=sink)
    assert sink.total() > 0 and (got.cpu().numpy() != 0.0).any()


def test_statistics_count_the_stage_on_top_of_the_closest_hits(scenes):
    """with lh_accel_trace_statistics on: rays = the pass's closest-hit rays + hits x nlights, as lh_accel_lights_device counts its items"""
    case = lit_case(23, 17, 3, 12)
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    sink = la.PtSink(total_records(o, case), case["max_vertices"], fields=("prim",))
    acc.trace_statistics(True)
    try:
        acc.statistics(clear=True)
        _, st = lit(acc, case, lights=LISTS["L2"], sink=sink)
        s = acc.statistics(clear=True)
    finally:
        acc.trace_statistics(False)
    hits = int((sink.records()["prim"] != MISS).sum())
    assert s["rays"] == st["rays"] + 2 * hits
