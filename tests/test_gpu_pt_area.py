"""The path tracer with area lights at every path vertex (lh_render_pt_tile_lights / lh_render_pt_bands_lights; the rule: lucille_amd/csrc/lh_ptl.h,
restated in tests/test_pta_rule.py and tests/test_ptl_rule.py) on the device.

As in tests/test_gpu_pt_lit.py the frame is tied down by COMPOSITION: the sink hands out every entry of every bounce; per bounce d the keys are
computed here from the records' path ids, the tile and the camera, the seed is lh_ptl_area_seed(seed, d), and the oracle-pinned
lh_accel_area_lights_device on the bounce's records gives the area value (for the smallest case the oracle itself does, through
tests.test_gpu_area.pin); lh_accel_lights_device gives the delta value; the rule in numpy float32 gives every hit's r; the frame is the integer sum
of pt_fix_np over the miss records' environment terms and the hit records' r.  All bit for bit."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from tests import pt_cases as pc
from tests.test_area_rule import COSINE, FACING, INVSQ, PDF
from tests.test_gpu_area import pin
from tests.test_gpu_pt_lit import ENV, LISTS, MISS, bits, colours_of, frame_from_terms, lit_case, materials_of, same, setup, total_records
from tests.test_pta_rule import area_seed, path_keys, value_add
from tests.test_ptl_rule import direct

pytestmark = pytest.mark.gpu

REACH_BAR = pc.REACH_BAR
EPS = 1e-5


# the emitter table: a quad above and beside the sphere whose normals point down, then a strip of seven unequal triangles on the other side of the
# scene (the plane of ao_ps lies at z = -0.586, the sphere of radius 1.59 around (2.69, -2.03, 1.74), the camera looks down from (7.5, -6.5, 5.3))
def _table():
    quad = np.array([[[1.7, -3.0, 6.5], [1.7, -1.0, 6.5], [3.7, -1.0, 6.5]], [[1.7, -3.0, 6.5], [3.7, -1.0, 6.5], [3.7, -3.0, 6.5]]])
    xs = np.array([-2.0, -1.7, -1.1, -0.8, -0.1, 0.2, 0.7, 1.1, 1.5])
    ys = np.array([1.0, 1.3, 1.05, 1.25, 1.1, 1.3, 1.0, 1.2, 1.15])
    zs = np.array([3.0, 4.2, 3.1, 4.0, 3.0, 4.2, 3.3, 4.1, 3.0])
    v = np.stack([xs, ys, zs], axis=1)
    strip = np.stack([v[k:k + 3] for k in range(7)])
    return np.concatenate([quad, strip])


TABLE = _table()
QUAD = (0, 2, (3.0, 2.5, 2.0), COSINE | FACING)
STRIP = (2, 7, (4.0, 6.0, 8.0), COSINE | INVSQ | PDF)


def _many():
    rng = np.random.default_rng(77)
    out = []
    for l in range(la.AREA_LIGHTS_MAX):
        first = int(rng.integers(TABLE.shape[0])); n = int(rng.integers(1, min(4, TABLE.shape[0] - first) + 1))
        out.append((first, n, tuple(float(x) for x in rng.uniform(0.1, 2.0, 3)), l % 16))
    return out


# name -> (area lights as (first_tri, ntris, rgb, flags), S)
AREAS = {"quad16": ([QUAD], 16), "two4": ([QUAD, STRIP], 4), "many1": (_many(), 1), "quad1024": ([QUAD], 1024)}


def mk(lights):
    return [la.AreaLight(f, n, rgb, flags) for f, n, rgb, flags in lights]


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(meshes):
        if id(meshes) not in made:
            acc = pc.accel_of(meshes)
            acc.set_emitters(TABLE)
            made[id(meshes)] = (acc, pc.oracle_of(meshes))
        return made[id(meshes)]
    yield get
    for acc, _ in made.values():
        acc.close()


def run(acc, case, lights=(), area=(), S=16, sink=None, tile=None, spp=None, flags=0, lit=False, out=None):
    """render_pt_tile_lights (lit: render_pt_tile_lit) of a case -> (frame on the host, stats); spp: (begin, count, total), default the whole case"""
    x0, y0, w, h = tile or case["tile"]
    b, c, t = spp or (0, case["spp"], case["spp"])
    cam = pc.cameras(case["cam"])[0]
    if lit:
        img, st = acc.render_pt_tile_lit(cam, x0, y0, w, h, b, c, t, max_vertices=case["max_vertices"], flags=flags, lights=lights, sink=sink,
                                         seed=case["seed"], out=out)
    else:
        img, st = acc.render_pt_tile_lights(cam, x0, y0, w, h, b, c, t, max_vertices=case["max_vertices"], flags=flags, lights=lights, area=mk(area),
                                            area_params=la.AreaParams(EPS, 1.0, S), sink=sink, seed=case["seed"], out=out)
    return img.cpu().numpy(), st


def bounce_blocks(rec):
    """the sink's records come out per bounce: (d, first, last) of every bounce that has entries"""
    first = np.concatenate([[0], np.cumsum(rec["counts"].astype(np.int64))])
    n = rec["prim"].shape[0]
    return [(d, int(first[d]), int(min(first[d + 1], n))) for d in range(rec["counts"].shape[0]) if first[d] < min(first[d + 1], n)]


def by_path(rec):
    """a sink's records in (path, bounce) order: from bounce 1 on the slot order of a bounce depends on scheduling, the set of records does not"""
    o = np.lexsort((rec["depth"], rec["path"]))
    return {k: (v if k == "counts" else v[o]) for k, v in rec.items()}


def keys_of(case, rec, tile=None, spp=None):
    x0, y0, w, h = tile or case["tile"]
    b, c, t = spp or (0, case["spp"], case["spp"])
    return path_keys(rec["path"], c, b, t, case["cam"]["w"], x0, y0, w, h)


def area_values(acc, case, sink, rec, keys, area, S):
    """lh_accel_area_lights_device on every bounce's records with its keys and its seed -> (mask uint32 [n], value float32 [n, 3])"""
    import torch
    n = rec["prim"].shape[0]
    mask = np.zeros(n, np.uint32); val = np.zeros((n, 3), np.float32)
    for d, a, b in bounce_blocks(rec):
        assert (rec["depth"][a:b] == d).all()
        key = torch.from_numpy(np.ascontiguousarray(keys[a:b]).view(np.int64)).cuda()
        gv, gr = acc.area_lights_device(sink.org[a:b].contiguous(), sink.dir[a:b].contiguous(),
                                        (sink.prim[a:b].contiguous(), sink.t[a:b].contiguous(), sink.u[a:b].contiguous(), sink.v[a:b].contiguous()),
                                        mk(area), la.AreaParams(EPS, 1.0, S), area_seed(case["seed"], d), key=key)
        mask[a:b] = gv.cpu().numpy().view(np.uint32); val[a:b] = gr.cpu().numpy()
    return mask, val


def open_counts(acc, case, sink, rec, keys, area, S):
    """per hit record and light: the samples traced and the samples open, from the rays alone and a bounded any-hit launch; and the traced items'
    smallest |dir.y| -> (traced [n, L], open [n, L], min |dir.y|)"""
    import torch
    n, L = rec["prim"].shape[0], len(area)
    traced = np.zeros((n, L), np.int64); open_ = np.zeros((n, L), np.int64); ymin = np.inf
    for d, a, b in bounce_blocks(rec):
        key = torch.from_numpy(np.ascontiguousarray(keys[a:b]).view(np.int64)).cuda()
        so, ns, ro, rd, rt, _ = acc.area_light_rays_device(sink.org[a:b].contiguous(), sink.dir[a:b].contiguous(),
                                                           (sink.prim[a:b].contiguous(), sink.t[a:b].contiguous(), sink.u[a:b].contiguous(),
                                                            sink.v[a:b].contiguous()), mk(area), la.AreaParams(EPS, 1.0, S), area_seed(case["seed"], d), key=key)
        torch.cuda.synchronize()
        nslots = int(ns.cpu().numpy().view(np.uint32)[0])
        m = nslots * L * S
        if m == 0:
            continue
        occ = acc.intersect_device(ro[:m].contiguous(), rd[:m].contiguous(), mode=la.MODE_ANY, tmax=rt[:m].contiguous())[0]
        torch.cuda.synchronize()
        occ = occ.cpu().numpy().reshape(nslots, L, S); tm = rt[:m].cpu().numpy().reshape(nslots, L, S); dy = np.abs(rd[:m].cpu().numpy()[:, 1]).reshape(nslots, L, S)
        ids = a + np.flatnonzero(so.cpu().numpy().view(np.uint32) != 0xFFFFFFFF)
        assert ids.shape[0] == nslots and (rec["prim"][ids] != MISS).all()
        traced[ids] = (tm > 0.0).sum(axis=2); open_[ids] = ((tm > 0.0) & (occ == 0)).sum(axis=2)
        if (tm > 0.0).any():
            ymin = min(ymin, float(dy[tm > 0.0].min()))
    return traced, open_, ymin


def expected(acc, case, sink, lights, area, S, tile=None, spp=None, env_rgb=ENV, area_val=None):
    """the sink's records -> (records, hit mask, keys, expected r per record, expected frame)"""
    rec = sink.records()
    n = rec["prim"].shape[0]
    assert sink.total() == n <= sink.capacity
    hit = rec["prim"] != MISS
    keys = keys_of(case, rec, tile, spp)
    delta = None
    if lights:
        _, gr = acc.lights_device(sink.org[:n], sink.dir[:n], (sink.prim[:n], sink.t[:n], sink.u[:n], sink.v[:n]), lights, None)
        delta = gr.cpu().numpy()
    if area and area_val is None:
        area_val = area_values(acc, case, sink, rec, keys, area, S)[1]
    if lights and area:
        val = value_add(delta, area_val)
    else:
        val = delta if lights else (area_val if area else np.zeros((n, 3), np.float32))
    kd, mesh, tri = materials_of(acc, case, rec["prim"])
    col = colours_of(case, mesh, tri, rec["u"], rec["v"])
    r = np.where(hit[:, None], direct(rec["thr"], kd, col, val), np.float32(0.0)).astype(np.float32)
    with np.errstate(all="ignore"):
        env = rec["thr"] * np.asarray(env_rgb, np.float32)[None, :]
    terms = np.where(hit[:, None], r, env)
    _, _, w, h = tile or case["tile"]
    b, c, t = spp or (0, case["spp"], case["spp"])
    frame = frame_from_terms(rec["path"].astype(np.int64) // c, terms, w, h, t)
    return rec, hit, keys, r, frame


# ---- 1. equalities -------------------------------------------------------------------------------------------------------------------------------
def test_without_area_lights_the_calls_are_the_lit_ones(scenes):
    """narea == 0: frame, statistics and every sink array are the _lit forms' for 0, 1 and 2 delta lights; with nothing at all the unlit forms' frames"""
    case = lit_case(23, 17, 3, 12)
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    cam = pc.cameras(case["cam"])[0]
    total = total_records(o, case)
    for lights in ([], LISTS["L1"], LISTS["L2"]):
        sa, sb = la.PtSink(total, 12), la.PtSink(total, 12)
        ref, rst = run(acc, case, lights=lights, sink=sa, lit=True)
        got, st = run(acc, case, lights=lights, sink=sb)
        assert st == rst
        same(got, ref, "%d delta lights" % len(lights))
        ra, rb = by_path(sa.records()), by_path(sb.records())
        for k in ra:
            same(rb[k], ra[k], "%d delta lights, sink %s" % (len(lights), k))
    ref, rst = acc.render_pt_tile2(cam, 0, 0, 23, 17, 0, 3, 3, max_vertices=12, seed=case["seed"])
    got, st = run(acc, case)
    assert st == rst
    same(got, ref.cpu().numpy(), "nothing: the unlit tile")
    rows, nb = 3, 17 // 3
    for r in range(3):
        mine = len(range(r, nb, 3))
        a, sa = acc.render_pt_bands(cam, rows * r, rows, 3 * rows, mine, 0, 3, 3, max_vertices=12, seed=case["seed"])
        b, sb = acc.render_pt_bands_lights(cam, rows * r, rows, 3 * rows, mine, 0, 3, 3, max_vertices=12, seed=case["seed"])
        c, sc = acc.render_pt_bands_lit(cam, rows * r, rows, 3 * rows, mine, 0, 3, 3, max_vertices=12, lights=LISTS["L2"], seed=case["seed"])
        d, sd = acc.render_pt_bands_lights(cam, rows * r, rows, 3 * rows, mine, 0, 3, 3, max_vertices=12, lights=LISTS["L2"], seed=case["seed"])
        assert sa == sb and sc == sd
        same(b.cpu().numpy(), a.cpu().numpy(), "nothing: bands of rank %d" % r)
        same(d.cpu().numpy(), c.cpu().numpy(), "two delta lights: bands of rank %d" % r)


# ---- 2. composition ------------------------------------------------------------------------------------------------------------------------------
def check(scenes, case, name, lights=(), bars=False, oracle_pin=False):
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    area, S = AREAS[name]
    sink = la.PtSink(total_records(o, case), case["max_vertices"])
    got, st = run(acc, case, lights=lights, area=area, S=S, sink=sink)
    rec, hit, keys, r, frame = expected(acc, case, sink, lights, area, S)
    assert st["rays"] == rec["prim"].shape[0]
    same(rec["direct"], r, case["name"] + ": direct")
    same(got, frame, case["name"] + ": frame")
    if oracle_pin:
        # the area value once more, straight from the oracle: the restated rule and oracle.intersect on every hit record, bounce by bounce
        h = np.flatnonzero(hit)
        st24 = acc.state_build(rec["org"][h], rec["dir"][h], rec["prim"][h], rec["t"][h], rec["u"][h], rec["v"][h])
        O = st24[:, 0:3] + st24[:, 6:9] * EPS; Ns = st24[:, 6:9]
        val = np.zeros((rec["prim"].shape[0], 3), np.float32)
        for d in np.unique(rec["depth"][h]):
            sel = rec["depth"][h] == d
            e = pin(o, np.ascontiguousarray(O[sel]), np.ascontiguousarray(Ns[sel]), keys[h][sel], area, S, table=TABLE, seed=area_seed(case["seed"], int(d)))
            assert not e["outside"].any()
            val[h[sel]] = e["val"]
        rec2, _, _, r2, frame2 = expected(acc, case, sink, lights, area, S, area_val=val)
        same(r2, r, case["name"] + ": direct from the oracle's values")
        same(frame2, frame, case["name"] + ": frame from the oracle's values")
    if bars:
        # non-vacuity: conditions on the inputs, separately for the camera rays' hits and for the later bounces'
        traced, open_, ymin = open_counts(acc, case, sink, rec, keys, area, S)
        assert ymin > 1e-14
        lit_later = int((hit & (rec["depth"] >= 1) & (r != 0.0).any(axis=1)).sum())
        for what, sel in (("bounce 0", hit & (rec["depth"] == 0)), ("bounces >= 1", hit & (rec["depth"] >= 1))):
            t, op = traced[sel, 0], open_[sel, 0]
            partly = int(((op > 0) & (op < S)).sum()); full = int((op == S).sum()); shut = int(((t > 0) & (op == 0)).sum())
            print("%s, %s: %d hits, light 0: partly open %d, fully open %d, traced but shut %d, not traced %d; lit hits at bounces >= 1: %d" % (
                case["name"], what, int(sel.sum()), partly, full, shut, int((t == 0).sum()), lit_later))
            assert partly >= REACH_BAR and full >= REACH_BAR and shut >= REACH_BAR
        assert lit_later >= REACH_BAR
    return rec, hit, r


def test_one_area_light_and_the_bars(scenes):
    """the quad, 16 samples: at the camera rays' hits and at the later bounces' alike, hits that see all of it, part of it (the penumbra) and none of
    it though their samples were traced; lit hits at bounces >= 1; no traced item outside the shadow rays' contract.  41 x 31 x 3: at 23 x 17 x 3
    the later bounces have 10 hits whose traced samples are all shut, fewer than the bar asks for"""
    check(scenes, lit_case(41, 31, 3, 12), "quad16", bars=True)


def test_two_area_and_two_delta_lights(scenes):
    """both stages: value = delta + area, one float32 add -- and the add matters: many hits have both terms non-zero"""
    case = lit_case(23, 17, 3, 12)
    rec, hit, r = check(scenes, case, "two4", lights=LISTS["L2"])
    acc, _ = scenes(case["meshes"])
    sink = la.PtSink(rec["prim"].shape[0], 12)
    r = r[np.lexsort((rec["depth"], rec["path"]))]
    run(acc, case, lights=LISTS["L2"], sink=sink); rd = by_path(sink.records())["direct"]
    run(acc, case, area=AREAS["two4"][0], S=4, sink=sink); ra = by_path(sink.records())["direct"]
    both = (rd != 0.0).any(axis=1) & (ra != 0.0).any(axis=1)
    differs = (bits(r[both]) != bits(rd[both])).any(axis=1) & (bits(r[both]) != bits(ra[both])).any(axis=1)
    print("hits with a delta and an area term: %d, of them with an r that is neither term's alone: %d" % (int(both.sum()), int(differs.sum())))
    assert differs.sum() >= REACH_BAR


CASES = [("many1", 23, 17, 3, 12, False), ("quad1024", 7, 5, 1, 3, True), ("quad16", 23, 17, 3, 2, False), ("two4", 23, 17, 1, 12, False),
         ("two4", 23, 17, 65, 3, False)]


@pytest.mark.parametrize("name, w, h, spp, mv, oracle_pin", CASES, ids=["%s %dx%dx%d v%d" % c[:5] for c in CASES])
def test_the_frame_is_the_composition(scenes, name, w, h, spp, mv, oracle_pin):
    """31 lights of one sample; one light of 1 024 samples on fewer paths than a wave -- pinned to the oracle itself; two vertices: one bounce; one
    sample a pixel; 65: a pixel's run of paths straddles a wave in pt_accumulate"""
    check(scenes, lit_case(w, h, spp, mv), name, lights=LISTS["L1"] if name == "many1" else (), oracle_pin=oracle_pin)


def test_materialised_shadow_rays_give_the_same_bytes(scenes):
    case = lit_case(23, 17, 3, 12)
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    area, S = AREAS["two4"]
    total = total_records(o, case)
    sa, sb = la.PtSink(total, 12), la.PtSink(total, 12)
    whole, st = run(acc, case, lights=LISTS["L2"], area=area, S=S, sink=sa)
    acc.set_param("ao_fused", 0)
    try:
        mat, sm = run(acc, case, lights=LISTS["L2"], area=area, S=S, sink=sb)
    finally:
        acc.set_param("ao_fused", 1)
    assert sm == st
    same(mat, whole, "ao_fused 0")
    ra, rb = by_path(sa.records()), by_path(sb.records())
    for k in ra:
        same(rb[k], ra[k], "ao_fused 0: sink " + k)


# ---- 4. tiling -----------------------------------------------------------------------------------------------------------------------------------
def test_tiles_bands_and_passes_over_the_samples(scenes):
    import torch
    case = lit_case(23, 17, 3, 12)
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    cam = pc.cameras(case["cam"])[0]
    area, S = AREAS["two4"]
    lights = LISTS["L1"]
    total = total_records(o, case)
    full = la.PtSink(total, 12)
    whole, st = run(acc, case, lights=lights, area=area, S=S, sink=full)
    # four unequal tiles
    frame = np.zeros_like(whole); rays = 0
    for x0, y0, w, h in ((0, 0, 11, 7), (11, 0, 12, 7), (0, 7, 5, 10), (5, 7, 18, 10)):
        part, sp = run(acc, case, lights=lights, area=area, S=S, tile=(x0, y0, w, h))
        frame[17 - y0 - h:17 - y0, x0:x0 + w] = part; rays += sp["rays"]
    same(frame, whole, "four tiles")
    assert rays == st["rays"]
    # the bands three ranks would own, of 1 and 3 lines
    for rows in (1, 3):
        nb = 17 // rows
        img = torch.zeros((nb, rows, 23, 3), dtype=torch.float32, device="cuda")
        for r in range(3):
            mine = len(range(r, nb, 3))
            out, _ = acc.render_pt_bands_lights(cam, rows * r, rows, 3 * rows, mine, 0, 3, 3, max_vertices=12, lights=lights, area=mk(area),
                                                area_params=la.AreaParams(EPS, 1.0, S), seed=case["seed"])
            img[r::3] = out
        torch.cuda.synchronize()
        same(img.flip(0).reshape(nb * rows, 23, 3).cpu().numpy(), whole[17 - nb * rows:], "bands of %d" % rows)
    # sample 2 of 3 as a pass of its own: path for path the records and the direct light of sample 2 of the whole pass
    one = la.PtSink(total, 12)
    run(acc, case, lights=lights, area=area, S=S, sink=one, spp=(2, 1, 3))
    ra, rb = full.records(), one.records()
    pick = np.flatnonzero(ra["path"] % 3 == 2)
    oa = pick[np.lexsort((ra["depth"][pick], ra["path"][pick] // 3))]
    ob = np.lexsort((rb["depth"], rb["path"]))
    assert oa.shape[0] == ob.shape[0] >= 23 * 17 and np.array_equal(ra["path"][oa] // 3, rb["path"][ob]) and np.array_equal(ra["depth"][oa], rb["depth"][ob])
    for k in ("org", "dir", "prim", "t", "u", "v", "thr", "direct"):
        same(rb[k][ob], ra[k][oa], "sample 2 alone: " + k)
    assert (ra["direct"][oa] != 0.0).any(axis=1).sum() >= REACH_BAR
    assert np.array_equal(keys_of(case, {"path": rb["path"][ob]}, spp=(2, 1, 3)), keys_of(case, {"path": ra["path"][oa]}))


# ---- 5. a hand-derivable frame ---------------------------------------------------------------------------------------------------------------------
def test_a_frame_derived_by_hand():
    """the lone plane, a black environment, two vertices, one emitter triangle without flags, four samples: every item weighs 1 and is open, value =
    (float)(4 rgb / 4) = rgb, so a pixel that hits is pt_fix(kd x 1 x rgb) per sample, converted; with the emitter below the plane every shadow
    ray starts eps above it and meets the hit's own triangle: every pixel is 0"""
    kd, c = (0.7, 0.6, 0.5), (1.25, 0.5, 3.0)
    meshes = pc.plane_meshes()
    acc = pc.accel_of(meshes)
    try:
        case = pc._case("hand", meshes, [pc.mat(kd=kd)], pc.camera(24, 16, 0.08, pc.eye_matrix((0.0, 0.0, 5.0)), 1), 2, 3, (), max_vertices=2)
        setup(acc, case, (0.0, 0.0, 0.0))
        cam = pc.cameras(case["cam"])[0]
        for z in (40.0, -40.0):
            acc.set_emitters(np.array([[[-1.0, -1.25, z], [2.0, -0.5, z], [0.25, 1.5, z + 1.0]]]))
            sink = la.PtSink(24 * 16 * 2, 2)
            got, st = acc.render_pt_tile_lights(cam, 0, 0, 24, 16, 0, 2, 2, max_vertices=2, area=[la.AreaLight(0, 1, c, 0)],
                                                area_params=la.AreaParams(EPS, 1.0, 4), sink=sink, seed=3)
            got = got.cpu().numpy()
            rec = sink.records()
            assert rec["prim"].shape[0] == 24 * 16 * 2 and np.array_equal(rec["path"], np.arange(24 * 16 * 2))
            hit = rec["prim"] != MISS
            assert hit.sum() >= REACH_BAR and (~hit).sum() >= REACH_BAR
            r = (np.asarray(kd, np.float32) * np.float32(1.0)) * np.asarray(c, np.float32)
            model = np.where(hit[:, None], r[None, :], np.float32(0.0)).astype(np.float32) if z > 0 else np.zeros((24 * 16 * 2, 3), np.float32)
            same(got, pc.frame_from_paths(model.reshape(24 * 16, 2, 3), 24, 16, 2), "emitter at z = %+g" % z)
            same(rec["direct"], model, "direct, emitter at z = %+g" % z)
            assert (got != 0.0).any() == (z > 0)
    finally:
        acc.close()


# ---- 6. refusals and statistics ----------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(scenes):
    import torch
    case = lit_case(7, 5, 1, 3)
    acc, _ = scenes(case["meshes"])
    setup(acc, case)
    cam = pc.cameras(case["cam"])[0]
    out = torch.full((5, 7, 3), 7.0, dtype=torch.float32, device="cuda")
    bout = torch.full((5, 1, 7, 3), 7.0, dtype=torch.float32, device="cuda")
    sink = la.PtSink(64, 3)
    for k in sink.FIELDS + ("counts",):
        getattr(sink, k).view(torch.uint8).fill_(0x77)
    quad = mk([QUAD])

    def refused(msg, cam=cam, spp=(0, 1, 1), mv=3, tile=(0, 0, 7, 5), bands=True, sink=sink, **kw):
        calls = [lambda: acc.render_pt_tile_lights(cam, *tile, *spp, max_vertices=mv, sink=sink, out=out, **kw)]
        if bands:
            calls.append(lambda: acc.render_pt_bands_lights(cam, 0, 1, 1, 5, *spp, max_vertices=mv, sink=sink, out=bout, **kw))
        for call in calls:
            with pytest.raises(la.LucilleHipError) as e:
                call()
            assert all(m in str(e.value) for m in msg), str(e.value)

    refused(("bad lights",), lights=[la.Light((0, 1, 1), (1, 1, 1))] * 32, area=quad)
    refused(("bad area lights",), area=quad * 32)
    refused(("bad area lights",), area=[la.AreaLight(8, 2, (1, 1, 1))])                                    # a run beyond the table's 9 triangles
    refused(("bad area lights",), area=[la.AreaLight(0, 1, (1, float("inf"), 1))])
    refused(("bad area lights",), area=quad, area_params=la.AreaParams(EPS, 1.0, 1025))
    refused(("bad area lights",), area=quad, area_params=la.AreaParams(EPS, 0.0, 4))
    refused(("bad area lights",), area=quad, area_params=la.AreaParams(EPS, 1.0, 4, reserved=1))
    s = sink.struct(); s.d_org = s.d_org + 4
    refused(("sink", "not 8-byte aligned"), sink=s, area=quad)
    # the reserved words of the structure itself
    arr = (la.AreaLight * 1)(*quad)
    for field in ("reserved0", "reserved1"):
        pl = la.PtLights(); pl.area = arr; pl.narea = 1; setattr(pl, field, 1)
        sk = sink.struct()
        rc = acc.L.lh_render_pt_tile_lights(acc.h, C.byref(cam), 0, 0, 7, 5, 0, 1, 1, 3, 0, C.byref(pl), C.byref(sk), 1, C.c_void_p(out.data_ptr()), None, None)
        assert rc == -1 and "reserved" in acc.L.lh_last_error().decode()
    # no emitter table
    acc.set_emitters(None)
    try:
        refused(("bad area lights",), area=quad)
    finally:
        acc.set_emitters(TABLE)
    # the keys' 34 bits: a frame of 2^17 x 2^17 pixels and two samples, of which a 1 x 1 tile is asked for; 2^34 keys exactly are fine
    big = la.Camera.make(1 << 17, 1 << 17, 1.0, np.eye(4))
    one = torch.full((1, 1, 3), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(la.LucilleHipError) as e:
        acc.render_pt_tile_lights(big, 5, 5, 1, 1, 0, 1, 2, max_vertices=3, area=quad, sink=sink, out=one)
    assert "2^34" in str(e.value) and "lh_render_pt_tile_lights" in str(e.value)
    # one term per entry of every bounce: 11 samples x 399 bounces are more than the 4096 a pixel's sums hold, with area lights alone too
    refused(("4096",), spp=(0, 11, 11), mv=400, area=quad)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (bout == 7.0).all() and (one == 7.0).all()
    for k in sink.FIELDS + ("counts",):
        assert (getattr(sink, k).view(torch.uint8) == 0x77).all(), k
    # the same frame at one sample holds 2^34 keys exactly: rendered
    acc.render_pt_tile_lights(big, 5, 5, 1, 1, 0, 1, 1, max_vertices=3, area=quad, out=one)
    torch.cuda.synchronize()
    assert not (one == 7.0).all()
    # and the same arguments, made good, render
    got, _ = acc.render_pt_tile_lights(cam, 0, 0, 7, 5, 0, 1, 1, max_vertices=3, area=quad, sink=sink)
    assert sink.total() > 0 and (got.cpu().numpy() != 0.0).any()


def test_statistics_count_both_stages_on_top_of_the_closest_hits(scenes):
    """with lh_accel_trace_statistics on: rays = the pass's closest-hit rays + hits x nlights + hits x narea x S"""
    case = lit_case(23, 17, 3, 12)
    acc, o = scenes(case["meshes"])
    setup(acc, case)
    area, S = AREAS["two4"]
    for lights in (LISTS["L2"], []):
        sink = la.PtSink(total_records(o, case), case["max_vertices"], fields=("prim",))
        acc.trace_statistics(True)
        try:
            acc.statistics(clear=True)
            _, st = run(acc, case, lights=lights, area=area, S=S, sink=sink)
            s = acc.statistics(clear=True)
        finally:
            acc.trace_statistics(False)
        hits = int((sink.records()["prim"] != MISS).sum())
        assert hits >= REACH_BAR and s["rays"] == st["rays"] + len(lights) * hits + len(area) * S * hits
