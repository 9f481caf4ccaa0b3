"""Material textures on the device (lh_accel_set_texture / _set_texture_device, the textured AO and dirt tiles, lh_accel_texture_device /
_host, lh_multi_set_texture): radiance[k] *= texcol[k] where the hit's mesh has a texture (ambientocclusion.c:393-401, dirtmap.c:273-281).

The expected frame is built in numpy from the tile's own scratch (lh_render_scratch: primary rays and records, slot_of_sample, the
materialised AO rays' occluded bytes), the st of lh_accel_state_build_host (pinned to the reference by tests/test_gpu_state.py) and the
fetch restated in tests/test_tex_rule.py (pinned to the compiled reference there); frames are compared as uint32 views of the floats.

Scenes (frames of 80 x 80, tiles of 40 x 40, pixel_samples 1 and 2, gather_nsamples 4):
  c1    the ao_c1 golden (322 triangles, four meshes) with synthetic per-vertex texture coordinates: the floor (64x64) and mesh 0 (7x3)
        textured, mesh 1 textured (1x5) WITHOUT coordinates (s = t = 0), mesh 2 with coordinates but no texture;
  soup  a two-mesh soup of 400 triangles, only the first mesh (267 triangles, 5x1 texels) textured.
Coverage of the tile, from the oracle's records of its camera samples (printed): at least 30 % hit a textured mesh, at least 10 % hit an
untextured one or miss, and the coordinates of the textured hits span more than one period of s and of t."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
from tests.helpers import load_golden
from tests.test_gpu_dirt import gather_rays, oracle_t, values
from tests.test_tex_abi import uncommitted_set_replace_remove
from tests.test_tex_rule import fetch_np

pytestmark = pytest.mark.gpu

W = H = 80
T = 40
NS, N = 4, 4
TILE = {"c1": (20, 20), "soup": (20, 20)}          # x0, y0 of the 40 x 40 tile
MISS = np.uint32(0xFFFFFFFF)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def host(x):
    return x.detach().cpu().numpy()


def make_textures(rng):
    return {(w, h): (rng.uniform(0.05, 1.6, (h, w, 4))).astype(np.float32) for w, h in ((64, 64), (7, 3), (1, 5), (5, 1))}


class Case:
    """meshes (positions, indices), per-mesh texture coordinates (or None) and textures (or None), the oracle, the 80 x 80 camera"""

    def __init__(self, name, meshes, st, tex, cam20):
        self.name, self.meshes, self.st, self.tex = name, meshes, st, dict(tex)
        self.first = np.cumsum([0] + [m[1].shape[0] // 3 for m in meshes])
        self.oracle = po.Oracle()
        for P, idx in meshes:
            self.oracle.add_mesh(P, idx)
        self.oracle.build()
        self.ocam = po.Camera.from_ref(cam20, W, H)
        self.cam = la.Camera.make(W, H, self.ocam.flength, list(self.ocam.cam2world), self.ocam.rh)
        self.acc = self.accel()
        self.memo = {}

    def accel(self, textures=True, device=False):
        import torch
        acc = la.HipAccel(0)
        for k, (P, idx) in enumerate(self.meshes):
            if device:
                acc.add_mesh_device(torch.from_numpy(P).cuda(), torch.from_numpy(idx.astype(np.int32)).cuda())
                if self.st[k] is not None:
                    acc.set_attribute_device(k, la.ATTR_TEXCOORD, torch.from_numpy(self.st[k]).cuda())
            else:
                acc.add_mesh(P, idx)
                if self.st[k] is not None:
                    acc.set_attribute(k, la.ATTR_TEXCOORD, self.st[k])
        if textures:          # before commit: trees do not depend on them
            for k, t in self.tex.items():
                acc.set_texture(k, t)
        acc.commit(); acc.wait_exact()
        return acc

    def mesh_of(self, prim):
        return np.searchsorted(self.first, prim, side="right") - 1

    def close(self):
        self.acc.close()


def c1_case():
    g = load_golden("ao_c1")
    meshes = [(np.ascontiguousarray(g["pos%d" % k], np.float64), np.ascontiguousarray(g["idx%d" % k], np.uint32)) for k in range(int(g["ngeoms"]))]

    def st_of(P):
        return np.ascontiguousarray(np.stack([0.9 * P[:, 0] + 0.35 * P[:, 2] + 0.1, 0.8 * P[:, 1] - 0.45 * P[:, 2] + 0.3 * P[:, 0]], -1))
    tx = make_textures(np.random.default_rng(5))
    st = [st_of(meshes[0][0]), None, st_of(meshes[2][0]), st_of(meshes[3][0])]
    return Case("c1", meshes, st, {0: tx[(7, 3)], 1: tx[(1, 5)], 3: tx[(64, 64)]}, g["camera"])


def soup_case():
    P, idx, _, _ = po.soup(400, 10, 0.1, 11)
    nA = 267
    A = (np.ascontiguousarray(P[:3 * nA]), np.arange(3 * nA, dtype=np.uint32))
    B = (np.ascontiguousarray(P[3 * nA:]), np.arange(3 * (400 - nA), dtype=np.uint32))
    assert np.array_equal(idx, np.arange(1200, dtype=np.uint32))          # the soup's triangles are unshared, in order

    def st_of(Q):
        return np.ascontiguousarray(np.stack([2.2 * Q[:, 0] + 0.3 * Q[:, 1] - 0.4, 1.9 * Q[:, 1] - 0.4 * Q[:, 2] + 0.25], -1))
    c2w = np.eye(4); c2w[3, :3] = (0.5, 0.5, -1.5)
    cam20 = np.concatenate([c2w.ravel(), [2.0, W, H, 0]])
    tx = make_textures(np.random.default_rng(6))
    return Case("soup", [A, B], [st_of(A[0]), st_of(B[0])], {0: tx[(5, 1)]}, cam20)


@pytest.fixture(scope="module")
def cases():
    cs = {"c1": c1_case(), "soup": soup_case()}
    yield cs
    for c in cs.values():
        c.close()


# ---- the expectation ----------------------------------------------------------------------------------------------------------------
def compose(case, tex, prim, st, slot, value_of_slot, w, h, ps):
    """k_ao_resolve with the multiply: per camera sample rad (0 for a miss), rad_k = rad * texcol[k] where the hit's mesh has a texture,
    accum_k = accum_k + rad_k over the sub-samples, (float)(accum_k * (1.0 / (xs * ys))), negatives to 0, lines flipped"""
    S = ps * ps; n = w * h * S
    hit = slot != MISS
    rad = np.zeros(n); rad[hit] = value_of_slot[slot[hit]]
    col = np.repeat(rad[:, None], 3, axis=1)
    mesh = np.full(n, -1); mesh[hit] = case.mesh_of(prim[hit])
    for m, t in tex.items():
        sel = mesh == m
        if sel.any():
            col[sel] = rad[sel, None] * fetch_np(t, st[sel, 0], st[sel, 1])[:, :3]
    col = col.reshape(w * h, S, 3)
    accum = np.zeros((w * h, 3))
    for s in range(S):
        accum = accum + col[:, s]
    f = (accum * (1.0 / S)).astype(np.float32)
    f = np.where(f < 0.0, np.float32(0.0), f)
    return f.reshape(h, w, 3)[::-1]


def records(acc):
    """the last AO tile's camera rays, records and slots, and the st of the hit epilogue"""
    org = acc.scratch(0, np.float64, 3); dr = acc.scratch(1, np.float64, 3)
    prim = acc.scratch(2, np.uint32, 1); t = acc.scratch(3, np.float64, 1); u = acc.scratch(4, np.float64, 1); v = acc.scratch(5, np.float64, 1)
    slot = acc.scratch(6, np.uint32, 1)
    st = acc.state_build(org, dr, prim, t, u, v)[:, 18:20]
    return {"org": org, "dr": dr, "prim": prim, "t": t, "u": u, "v": v, "slot": slot, "st": st}


def materialised_tile(acc, cam, x0, y0, w, h, ps, seed, uniforms=None):
    """the tile with its AO rays in HBM -> (frame, stats, records, radiance per hit slot from the occluded bytes)"""
    acc.set_param("ao_fused", 0)
    try:
        rgb, st = acc.render_ao_tile(cam, x0, y0, w, h, ps, NS, seed=seed, uniforms=uniforms)
        rgb = host(rgb).copy()
        r = records(acc)
        occ = acc.scratch(10, np.uint8, 1).reshape(-1, N)
    finally:
        acc.set_param("ao_fused", 1)
    cnt = (occ != 0).sum(axis=1).astype(np.float64)
    assert occ.shape[0] == st["primary_hits"] and int(cnt.sum()) == st["ao_occluded"]
    ns = float(N)
    return rgb, st, r, 1.0 * (ns - cnt) / ns


def coverage(case, r, tex):
    """the issue's conditions, from the oracle's records of the tile's camera samples"""
    prim, _, u, v = case.oracle.intersect(r["org"], r["dr"], nthreads=8)
    assert np.array_equal(prim, r["prim"])
    hit = prim != po.MISS
    mesh = np.full(prim.shape[0], -1); mesh[hit] = case.mesh_of(prim[hit])
    textured = np.isin(mesh, list(tex))
    with_st = np.isin(mesh, [m for m in tex if case.st[m] is not None])
    s, t = r["st"][with_st, 0], r["st"][with_st, 1]
    f_tex, f_rest = float(textured.mean()), float((~textured).mean())
    print("%s: %d samples, textured %.3f, untextured or miss %.3f (miss %.3f), s in [%.3f, %.3f], t in [%.3f, %.3f]" % (
        case.name, prim.shape[0], f_tex, f_rest, float((~hit).mean()), s.min(), s.max(), t.min(), t.max()))
    assert f_tex >= 0.30 and f_rest >= 0.10, (f_tex, f_rest)
    assert s.max() - s.min() > 1.0 and t.max() - t.min() > 1.0


def reference_tile(case, ps, seed=5):
    """the 40 x 40 tile of a case, materialised once per (ps, seed): its frame, stats, records, expectation"""
    k = (ps, seed)
    if k not in case.memo:
        x0, y0 = TILE[case.name]
        rgb, st, r, rad = materialised_tile(case.acc, case.cam, x0, y0, T, T, ps, seed)
        exp = compose(case, case.tex, r["prim"], r["st"], r["slot"], rad, T, T, ps)
        for a in (rgb, exp, rad):
            a.setflags(write=False)
        case.memo[k] = (rgb, st, r, rad, exp)
    return case.memo[k]


# ---- 1. the AO tile ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [1, 2])
@pytest.mark.parametrize("name", ["c1", "soup"])
def test_ao_tile_fused_materialised_and_host(cases, name, ps):
    case = cases[name]; acc, cam = case.acc, case.cam
    x0, y0 = TILE[name]
    rgb_m, st_m, r, rad, exp = reference_tile(case, ps)
    coverage(case, r, case.tex)
    print("materialised: %d of %d values differ" % (int((bits(rgb_m) != bits(exp)).sum()), exp.size))
    assert same(rgb_m, exp)
    assert (exp[..., 0] != exp[..., 1]).any() and (exp[..., 1] != exp[..., 2]).any()          # colour, not grey
    rgb_f, st_f = acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)
    assert st_f == st_m and same(host(rgb_f), exp)
    # the plain-C host form
    L = binding.lib()
    L.lh_render_ao_tile_host.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    out = np.full((T, T, 3), 7.0, np.float32); st = binding.TileStats()
    assert L.lh_render_ao_tile_host(acc.h, C.byref(cam), x0, y0, T, T, ps, NS, 5, None, 0, out.ctypes.data, C.byref(st)) == 0, L.lh_last_error()
    assert same(out, exp) and st.primary_hits == st_m["primary_hits"] and st.ao_occluded == st_m["ao_occluded"]
    # statistics do not change with textures
    plain = case.accel(textures=False)
    _, st_p = plain.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)
    plain.close()
    assert st_p == st_m


@pytest.mark.parametrize("name", ["c1", "soup"])
def test_ao_tile_with_replayed_uniforms(cases, name):
    import torch
    case = cases[name]; acc, cam = case.acc, case.cam
    x0, y0 = TILE[name]; ps = 2
    uni = torch.from_numpy(np.random.default_rng(3).random(2 * N * T * T * ps * ps)).cuda()
    rgb, st, r, rad = materialised_tile(acc, cam, x0, y0, T, T, ps, 1, uniforms=uni)
    exp = compose(case, case.tex, r["prim"], r["st"], r["slot"], rad, T, T, ps)
    assert st["primary_hits"] > 0 and same(rgb, exp)
    acc2, _ = acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, uniforms=uni)          # "ao_fused" 1: uniforms materialise all the same
    assert same(host(acc2), exp)
    assert not same(exp, reference_tile(case, ps)[4])                               # other samples than the built-in generator's


def test_negative_products_are_clamped(cases):
    case = cases["c1"]; cam = case.cam
    x0, y0 = TILE["c1"]
    tex = dict(case.tex)
    neg = tex[3].copy(); neg[..., 0] = -neg[..., 0]; neg[::2, :, 1] *= -1.0; tex[3] = neg
    acc = case.accel(textures=False)
    for k, t in tex.items():          # after commit this time
        acc.set_texture(k, t)
    for ps in (1, 2):
        rgb, st, r, rad = materialised_tile(acc, cam, x0, y0, T, T, ps, 5)
        exp = compose(case, tex, r["prim"], r["st"], r["slot"], rad, T, T, ps)
        unclamped = compose(case, {k: np.abs(t) for k, t in tex.items()}, r["prim"], r["st"], r["slot"], rad, T, T, ps)
        assert same(rgb, exp) and (exp >= 0.0).all()
        zeroed = (exp[..., 0] == 0.0) & (unclamped[..., 0] > 0.0)
        print("ps %d: %d pixels clamped in channel 0" % (ps, int(zeroed.sum())))
        assert zeroed.sum() > 100 and ((exp[..., 1] == 0.0) & (unclamped[..., 1] > 0.0)).any() and (exp[..., 1] > 0.0).any()
        assert same(host(acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)[0]), exp)
    acc.close()


# ---- 2. all ones, set and remove, the device setter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "soup"])
def test_ones_and_removal_give_the_untextured_frame(cases, name):
    import torch
    case = cases[name]; cam = case.cam
    x0, y0 = TILE[name]
    acc = case.accel(textures=False)
    ref = {}
    for ps in (1, 2):
        rgb, st = acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)
        ref[ps] = (host(rgb).copy(), st)
        rgb_m, st_m, r, rad = materialised_tile(acc, cam, x0, y0, T, T, ps, 5)
        assert same(rgb_m, ref[ps][0]) and same(ref[ps][0], compose(case, {}, r["prim"], r["st"], r["slot"], rad, T, T, ps))
    acc.set_texture(la.ALL_MESHES, np.ones((3, 7, 4), np.float32))
    for ps in (1, 2):
        rgb, st = acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)
        assert st == ref[ps][1] and host(rgb).tobytes() == ref[ps][0].tobytes()
    # replace by the case's textures: through the host setter and through the device setter
    for k, t in case.tex.items():
        acc.set_texture(k, t)
    for k in range(len(case.meshes)):
        if k not in case.tex:
            acc.set_texture(k, None)
    host_frames = {ps: host(acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)[0]).copy() for ps in (1, 2)}
    assert same(host_frames[2], reference_tile(case, 2)[4])
    side = torch.cuda.Stream()
    for k, t in case.tex.items():
        d = torch.from_numpy(t).cuda(); torch.cuda.synchronize()
        acc.set_texture(k, d, stream=side)          # read by a copy on `side`; the tile below runs on torch's current stream
        d.record_stream(side)
        del d
    for ps in (1, 2):
        assert host(acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)[0]).tobytes() == host_frames[ps].tobytes()
    acc.set_texture(la.ALL_MESHES, None)
    for ps in (1, 2):
        rgb, st = acc.render_ao_tile(cam, x0, y0, T, T, ps, NS, seed=5)
        assert st == ref[ps][1] and host(rgb).tobytes() == ref[ps][0].tobytes()
    acc.close()


# ---- 3. bands, frames, tilings, replicas -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "soup"])
def test_bands_frame_host_tilings_and_two_replicas(cases, name):
    case = cases[name]; acc, cam = case.acc, case.cam
    ps = 2
    # the frame as one tile: the expectation from its own scratch
    rgb1, st1, r, rad = materialised_tile(acc, cam, 0, 0, W, H, ps, 7)
    exp = compose(case, case.tex, r["prim"], r["st"], r["slot"], rad, W, H, ps)
    assert same(rgb1, exp)
    one, s_one = acc.render_ao_frame_host(cam, ps, NS, seed=7, tile=W)
    four, s_four = acc.render_ao_frame_host(cam, ps, NS, seed=7, tile=T)
    assert same(one, exp) and same(four, exp) and s_one == s_four == st1
    # bands: lines 8..27 and 50..69 as one batch, every band in image orientation
    y0s = [8, 50]; rows = 20
    b, sb = acc.render_ao_bands(cam, y0s, rows, ps, NS, seed=7)
    b = host(b)
    for k, y0 in enumerate(y0s):
        assert same(b[k], exp[H - (y0 + rows):H - y0]), k
    # two replicas of one GPU
    m = la.HipMulti([0, 0])
    for k, (P, idx) in enumerate(case.meshes):
        m.add_mesh(P, idx)
        if case.st[k] is not None:
            m.accel(0).set_attribute(k, la.ATTR_TEXCOORD, case.st[k])
    m.commit()
    for k, t in case.tex.items():
        m.set_texture(k, t)
    frame, sm, _ = m.render_ao_frame(cam, ps, NS, seed=7, tile=T)
    assert same(frame, exp) and sm == st1
    m.set_texture(la.ALL_MESHES, None)
    plain, _, _ = m.render_ao_frame(cam, ps, NS, seed=7, tile=T)
    assert same(plain, compose(case, {}, r["prim"], r["st"], r["slot"], rad, W, H, ps))
    m.close()


def test_device_meshes_with_device_coordinates(cases):
    for name in ("c1", "soup"):
        case = cases[name]; x0, y0 = TILE[name]
        dm = case.accel(device=True)
        for ps in (1, 2):
            rgb, st = dm.render_ao_tile(case.cam, x0, y0, T, T, ps, NS, seed=5)
            assert st == reference_tile(case, ps)[1] and same(host(rgb), reference_tile(case, ps)[4]), (name, ps)
        dm.close()


# ---- 4. the dirt tile ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [1, 2])
@pytest.mark.parametrize("name", ["c1", "soup"])
def test_dirt_tile(cases, name, ps):
    """the composition tests/test_gpu_dirt.py pins the untextured tile with -- the gather rays of the stage, the oracle's closest hits, the
    rule of lh_dirt.h restated -- times the texture"""
    import torch
    case = cases[name]; acc, cam, o = case.acc, case.cam, case.oracle
    x0, y0 = TILE[name]; spp = ps * ps
    ext = float(np.linalg.norm(np.ptp(np.concatenate([m[0] for m in case.meshes]), axis=0)))
    p = la.DirtParams(0.01 * ext, 0.25 * ext, 1e-5)
    org, dr = acc.primary_rays(cam, x0, y0, T, T, ps)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    i = np.arange(T * T * spp, dtype=np.int64); ipix = i // spp
    key = torch.from_numpy(((y0 + ipix // T) * cam.width + (x0 + ipix % T)) * spp + (i - ipix * spp)).cuda()
    slot, nslots, go, gd = gather_rays(acc, org, dr, rec, NS, p.eps, seed=5, key=key)
    t, hit = oracle_t(o, go, gd)
    nh, val = values(t, hit, N, p.near_clip, p.far_clip)
    prim = host(rec[0]).view(np.uint32)
    st = acc.state_build(host(org), host(dr), prim, host(rec[1]), host(rec[2]), host(rec[3]))[:, 18:20]
    exp = compose(case, case.tex, prim, st, slot, val, T, T, ps)
    for fused in (1, 0):
        acc.set_param("ao_fused", fused)
        try:
            rgb, stt = acc.render_dirt_tile(cam, x0, y0, T, T, ps, NS, p, seed=5)
        finally:
            acc.set_param("ao_fused", 1)
        print("%s ps %d fused %d: %d of %d values differ" % (name, ps, fused, int((bits(host(rgb)) != bits(exp)).sum()), exp.size))
        assert same(host(rgb), exp), fused
        assert stt["primary_hits"] == nslots and stt["ao_occluded"] == int(nh.sum()) > 0
    assert (exp[..., 0] != exp[..., 1]).any() and 0.0 < float(val.mean()) < 1.0
    plain = case.accel(textures=False)
    rgb, stp = plain.render_dirt_tile(cam, x0, y0, T, T, ps, NS, p, seed=5)
    assert stp == stt and same(host(rgb), compose(case, {}, prim, st, slot, val, T, T, ps))
    plain.close()


# ---- 5. the fetch alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "soup"])
def test_texture_device_and_host(cases, name):
    import torch
    case = cases[name]; acc = case.acc
    _, _, r, _, _ = reference_tile(case, 2)
    n = r["prim"].shape[0]
    prim, u, v, st = r["prim"], r["u"], r["v"], r["st"]
    hit = prim != MISS
    mesh = np.full(n, -1); mesh[hit] = case.mesh_of(prim[hit])
    exp = np.zeros((n, 4)); exp[hit] = 1.0
    for m, t in case.tex.items():
        sel = mesh == m
        exp[sel] = fetch_np(t, st[sel, 0], st[sel, 1])
    untextured = hit & ~np.isin(mesh, list(case.tex))
    assert untextured.sum() > 100 and (~hit).sum() > 100 and (hit & ~untextured).sum() > 1000
    d_rec = (torch.from_numpy(prim.view(np.int32)).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda"), torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda())
    got = host(acc.texture_device(d_rec)); torch.cuda.synchronize()
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    assert (got[untextured] == 1.0).all() and (got[~hit] == 0.0).all()
    assert np.array_equal(acc.texture_host(prim, u, v).view(np.uint64), exp.view(np.uint64))
    # a list with duplicates and out-of-range ids, a count on the device; the slots of rays that are not traced keep their poison
    rng = np.random.default_rng(9)
    ids = rng.integers(0, n, 500).astype(np.uint32); ids[10:20] = ids[0:10]; ids[30:40] = np.uint32(n) + np.arange(10, dtype=np.uint32); ids[45] = MISS
    cnt = 400
    index = torch.from_numpy(ids.view(np.int32)).cuda(); count = torch.tensor([cnt], dtype=torch.int32, device="cuda")
    poison = np.full((n, 4), np.float64(-7.25))
    out = torch.from_numpy(poison.copy()).cuda()
    acc.texture_device(d_rec, index=index, count=count, out=out); torch.cuda.synchronize()
    e = poison.copy(); listed = ids[:cnt]; listed = listed[listed < n]; e[listed] = exp[listed]
    assert np.array_equal(host(out).view(np.uint64), e.view(np.uint64))
    out = torch.from_numpy(poison.copy()).cuda()
    acc.texture_device(d_rec, count=torch.tensor([n + 5], dtype=torch.int32, device="cuda"), out=out); torch.cuda.synchronize()      # the identity list, clamped
    assert np.array_equal(host(out).view(np.uint64), exp.view(np.uint64))
    # no texture at all: ones for hits, zeros for misses; an empty scene: zeros
    plain = case.accel(textures=False)
    got = host(plain.texture_device(d_rec)); torch.cuda.synchronize()
    assert (got[hit] == 1.0).all() and (got[~hit] == 0.0).all()
    plain.close()
    empty = la.HipAccel(0); empty.commit()
    got = host(empty.texture_device(d_rec)); torch.cuda.synchronize()
    assert (got == 0.0).all()
    empty.close()


def test_refusals_that_need_an_accelerator(cases):
    import torch
    uncommitted_set_replace_remove()
    acc, L = cases["soup"].acc, binding.lib()
    d = torch.zeros((2, 3, 4), dtype=torch.float32, device="cuda")
    for args, msg in (((5, d.data_ptr(), 3, 2, None), "mesh 5 out of range"), ((0, d.data_ptr() + 2, 3, 1, None), "not 4-byte aligned"), ((0, None, 3, 2, None), "NULL array"), ((0, d.data_ptr(), 0, 2, None), "bad texture size")):
        rc = L.lh_accel_set_texture_device(acc.h, *args)
        err = L.lh_last_error().decode()
        assert rc == -1 and msg in err and "lh_accel_set_texture_device" in err, (args, err)
    # nothing changed: the frame is still the case's
    case = cases["soup"]; x0, y0 = TILE["soup"]
    assert same(host(acc.render_ao_tile(case.cam, x0, y0, T, T, 1, NS, seed=5)[0]), reference_tile(case, 1)[4])
