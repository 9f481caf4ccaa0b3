"""The entry points that take HOST arrays, through their one staging block (lh_stage.h; lh_stage_up / lh_stage_down): one accelerator over a
200-triangle scene, every host form in turn at batch sizes 1, 257, 3, 1025, 2 -- the block grows, is reused while it holds a larger layout another entry
point left, and grows again -- and every answer compared bit for bit with the matching device form's on tensors of the same bytes (the same kernel on the
same inputs: there is no tolerance).  The optional arrays are present and NULL; a beam beside the scene box keeps the plane it was given and a chain that
ends at depth 0 keeps its end-ray slots; a refused call between good ones changes nothing."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from tests.helpers import beam_set_np, raster_case

gpu = pytest.mark.gpu

SIZES = (1, 257, 3, 1025, 2)
NS = 4                        # gather rays per hit (a 2 x 2 grid)
WIN = 8                       # the raster window, and the AO tile
MISS = 0xFFFFFFFF


class In:
    """an input array (None: NULL in either form)"""
    def __init__(self, a): self.a = a


class Out:
    """an output array as the caller hands it over (None: NULL in either form)"""
    def __init__(self, a): self.a = a


class Host:
    """an argument of the host form alone"""
    def __init__(self, v): self.v = v


class Dev:
    """arguments of the device form alone"""
    def __init__(self, *v): self.v = v


def call_both(L, host_name, dev_name, spec):
    """-> (rc of the host form, rc of the device form, the host form's outputs, the device form's outputs): spec lists the host form's arguments behind
    the accelerator, with the device form's own (list, stream) where they stand"""
    import torch
    hargs, dargs, houts, douts, keep = [], [], [], [], []
    for s in spec:
        if isinstance(s, (In, Out)):
            if s.a is None:
                hargs.append(None); dargs.append(None)
                if isinstance(s, Out):
                    houts.append(None); douts.append(None)
                continue
            h = np.ascontiguousarray(s.a).copy()
            d = torch.from_numpy(h.copy().view(np.uint8).reshape(-1)).cuda()
            keep += [h, d]
            hargs.append(h.ctypes.data); dargs.append(d.data_ptr())
            if isinstance(s, Out):
                houts.append(h); douts.append(d)
        elif isinstance(s, Host):
            hargs.append(s.v)
        elif isinstance(s, Dev):
            dargs.extend(s.v)
        else:
            hargs.append(s); dargs.append(s)
    rc_h = getattr(L, host_name)(*hargs)
    rc_d = getattr(L, dev_name)(*dargs)
    torch.cuda.synchronize()
    return rc_h, rc_d, houts, [None if d is None else d.cpu().numpy() for d in douts]


def same_outputs(what, r):
    rc_h, rc_d, houts, douts = r
    assert rc_h == 0 and rc_d == 0, (what, rc_h, rc_d, binding.lib().lh_last_error())
    assert len(houts) == len(douts) and any(h is not None for h in houts)
    for k, (h, d) in enumerate(zip(houts, douts)):
        assert (h is None) == (d is None)
        if h is not None:
            assert h.view(np.uint8).reshape(-1).tobytes() == d.tobytes(), "%s: output %d differs between the host and the device form" % (what, k)
    return houts


class Fixture:
    def __init__(self):
        c = raster_case(seed=31, ntri=200, width=WIN, height=WIN, nbeams=1)
        self.P, self.idx = c["P"], c["idx"]
        acc = la.HipAccel(0)
        acc.add_mesh(self.P, self.idx)
        acc.set_attribute(0, la.ATTR_TEXCOORD, np.ascontiguousarray(0.3 * self.P[:, :2] + 0.1 * self.P[:, 2:3]))
        acc.set_texture(0, np.random.default_rng(5).uniform(0.05, 1.6, (3, 7, 4)).astype(np.float32))
        acc.commit(); acc.wait_exact()
        acc.set_environment((0.9, 0.6, 0.3))
        acc.set_sky(la.Sky.from_site(35.0, 139.0, 9.0, 180, 14.0, 3.0, basis_rgb=np.eye(3), basis_y=(1.0, 0.5, 0.25), sun_rgb=(2.0, 1.5, 1.0), flags=la.SKY_SUN))
        acc.set_emitters(np.array([[[-1.0, -1.0, 1.0], [1.0, -1.0, 1.0], [0.0, 1.0, 1.0]], [[-2.0, 0.0, 2.0], [2.0, 0.0, 2.0], [0.0, 2.0, 3.0]]]))
        self.acc, self.L = acc, acc.L
        L = self.L
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        L.lh_render_ao_tile_host.argtypes = [vp, vp] + [i32] * 6 + [C.c_uint64, vp, sz, vp, vp]
        L.lh_accel_beam_visibility_set_host.argtypes = [vp, sz, vp, vp]
        L.lh_accel_beam_raster_set_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
        self.cam = la.Camera.make(WIN, WIN, 2.0, np.eye(4), rh=0)          # at the origin, looking down +z at the scene: its edge pixels see past it
        self.lights = (la.Light * 2)(la.Light((0.0, 0.0, -1.0), (1.0, 0.5, 0.25)), la.Light((0.0, 0.0, 0.0), (0.5, 1.0, 2.0), la.LIGHT_POINT | la.LIGHT_COSINE))
        self.area = (la.AreaLight * 2)(la.AreaLight(0, 1, (1.0, 0.5, 0.25), la.AREA_COSINE), la.AreaLight(1, 1, (0.5, 1.0, 2.0), la.AREA_COSINE | la.AREA_PDF))
        self.memo = {}

    def batch(self, n):
        """n rays towards the scene and their closest-hit records, n directions, n beams in either form, n raster beams: made once per size"""
        if n not in self.memo:
            rng = np.random.default_rng(1000 + n)
            org = np.ascontiguousarray(np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2.5, 2.5, n), np.zeros(n)], 1))
            dr = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), np.ones(n)], 1)
            dr = np.ascontiguousarray(dr / np.linalg.norm(dr, axis=1, keepdims=True))
            prim, t, u, v = self.acc.intersect_host(org, dr)
            dirs = rng.normal(size=(n, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            # beams from around the origin aimed into the scene's box (tests.helpers.random_beams aims into the unit cube)
            borg = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 0, n)], 1)
            c = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 8, n)], 1) - borg
            c /= np.linalg.norm(c, axis=1, keepdims=True)
            a = np.cross(c, rng.normal(size=(n, 3))); a /= np.linalg.norm(a, axis=1, keepdims=True)
            s = 0.02; bb = np.cross(c, a)
            bdirs = np.ascontiguousarray(np.stack([c - s * a - s * bb, c + s * a - s * bb, c + s * a + s * bb, c - s * a + s * bb], 1))
            c = raster_case(seed=31, ntri=200, width=WIN, height=WIN, nbeams=n)
            rorg = c["org"].copy(); rorg[1::3, 0] += 100.0                                         # every third beam starts far to the side: it misses the scene box
            self.memo[n] = dict(org=org, dr=dr, prim=prim.astype(np.uint32), t=t, u=u, v=v, dirs=np.ascontiguousarray(dirs), key=rng.integers(0, 1 << 34, n).astype(np.uint64),
                                uni=rng.uniform(0.0, 1.0, 3 * 2 * 16 * n), borg=borg, bdirs=bdirs, rorg=rorg, rdirs=c["dirs"], rcorners=c["corners"],
                                plane=binding.RasterPlane(WIN, WIN, (C.c_double * 9)(*c["frame"].reshape(-1)), (C.c_double * 3)(*c["eye"]), float(c["fov"])))
        return self.memo[n]

    def close(self):
        self.acc.close()


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    yield f
    f.close()


def records(b):
    return [In(b["org"]), In(b["dr"]), In(b["prim"]), In(b["t"]), In(b["u"]), In(b["v"])]


# the gather forms: (host, device, what stands between the records and the seed, radiance floats per ray, uniforms per gather ray x gather rays per hit)
def gather_rows(fx):
    dp, ep, lp, ap = la.DirtParams(), la.EnvParams(), la.LightsParams(), la.AreaParams(nsamples=4, bound=0.999)
    fx.params = (dp, ep, lp, ap)
    return [("lh_accel_ao_host", "lh_accel_ao_device", [NS], 1, 2 * NS, True),
            ("lh_accel_dirt_host", "lh_accel_dirt_device", [NS, C.byref(dp)], 1, 2 * NS, True),
            ("lh_accel_env_host", "lh_accel_env_device", [NS, C.byref(ep)], 3, 2 * NS, True),
            ("lh_accel_lights_host", "lh_accel_lights_device", [fx.lights, 2, C.byref(lp)], 3, 0, False),
            ("lh_accel_area_lights_host", "lh_accel_area_lights_device", [fx.area, 2, C.byref(ap)], 3, 3 * 2 * 4, True)]


def gather_spec(fx, row, b, n, key, uni, counts, rad, seed=9):
    host, dev, mid, rf, upr, seeded = row
    spec = [fx.acc.h, n] + records(b) + list(mid)
    if seeded:
        nuni = upr * n
        spec += [seed, In(b["key"] if key else None), In(b["uni"][:nuni] if uni else None), Host(nuni if uni else 0)]
    spec += [Dev(None, 0, None), Out(np.full(n, 0x55555555, np.uint32) if counts else None), Out(np.full(rf * n, 7.0, np.float32) if rad else None), Dev(None)]
    return host, dev, spec


def every_row(fx, n, optional):
    """every host form once at n; optional: the optional arrays are given (else NULL, as far as a call still has an output)"""
    L, acc, b = fx.L, fx.acc, fx.batch(n)
    hits = b["prim"] != MISS
    # -- beam visibility, from corner directions and preset
    r = same_outputs("beam_visibility", call_both(L, "lh_accel_beam_visibility_host", "lh_accel_beam_visibility_device",
                                                  [acc.h, n, In(b["borg"]), In(b["bdirs"]), Out(np.full(n, 77, np.int32)), Dev(None)]))
    vis = r[0]
    assert set(vis.tolist()) <= {-1, 0, 1, 2} and (n < 257 or len(set(vis.tolist())) > 1)
    sets, refused = beam_set_np(b["borg"], b["bdirs"])
    got = np.full(n, 77, np.int32)
    assert L.lh_accel_beam_visibility_set_host(acc.h, n, sets.ctypes.data, got.ctypes.data) == 0, L.lh_last_error()
    assert np.array_equal(got[~refused], vis[~refused])                    # (no device form takes preset beams: against the beams they were set from)
    # -- beam raster, with and without the flags; the planes start as 7.0
    t0 = np.full((n, WIN, WIN), 7.0)
    spec = [acc.h, n, In(b["rorg"]), In(b["rdirs"]), In(b["rcorners"]), C.addressof(b["plane"]), Out(t0), Out(np.full(n, 77, np.int32)),
            Out(np.full((n, 4), 0x55, np.uint64) if optional else None), Dev(None)]
    t, st = same_outputs("beam_raster", call_both(L, "lh_accel_beam_raster_host", "lh_accel_beam_raster_device", spec))[:2]
    aside = np.zeros(n, bool); aside[1::3] = True
    assert (st[aside] == 1).all() and (t[aside] == 7.0).all()              # beside the scene box: the plane stays as it was given
    assert (t[st == 0] != 7.0).all() and (n < 3 or (st == 0).any())
    rsets, rref = beam_set_np(b["rorg"], b["rdirs"])
    assert not rref.any()
    t2 = np.full((n, WIN, WIN), 7.0); st2 = np.full(n, 77, np.int32); fl2 = np.zeros((n, 4), np.uint64)
    assert L.lh_accel_beam_raster_set_host(acc.h, n, rsets.ctypes.data, b["rcorners"].ctypes.data, C.addressof(b["plane"]), t2.ctypes.data, st2.ctypes.data,
                                           fl2.ctypes.data if optional else None) == 0, L.lh_last_error()
    assert np.array_equal(st2, st) and t2.tobytes() == t.tobytes()
    # -- the five gather forms
    for row in gather_rows(fx):
        variants = [(1, 1, 1, 1)] if optional else [(0, 0, 1, 0), (0, 0, 0, 1)]
        for key, uni, counts, rad in variants:
            host, dev, spec = gather_spec(fx, row, b, n, key, uni, counts, rad)
            outs = same_outputs(host, call_both(L, host, dev, spec))
            if counts:
                assert np.array_equal(outs[0] == MISS, ~hits), host
    # -- the environment and the sky seen in n directions
    for host, dev in (("lh_accel_environment_host", "lh_accel_environment_device"), ("lh_accel_sky_host", "lh_accel_sky_device")):
        same_outputs(host, call_both(L, host, dev, [acc.h, n, In(b["dirs"]), Out(np.full(3 * n, 7.0, np.float32)), Dev(None)]))
    # -- the hit epilogue: the host form zeroes what the device form leaves alone (a miss's state), so the device form starts from zeros
    same_outputs("state_build", call_both(L, "lh_accel_state_build_host", "lh_accel_state_build_device",
                                          [acc.h, n] + records(b) + [Out(np.zeros((n, la.STATE_DOUBLES))), Dev(None)]))
    # -- the texture fetch
    rgba = same_outputs("texture", call_both(L, "lh_accel_texture_host", "lh_accel_texture_device",
                                             [acc.h, n, In(b["prim"]), In(b["u"]), In(b["v"]), Dev(None, 0, None), Out(np.full((n, 4), 7.0)), Dev(None)]))[0]
    assert (rgba[~hits] == 0.0).all() and (rgba[hits] != 7.0).all()
    # -- the refraction chain: the end rays start as 7.0
    wp = la.WhittedParams()
    for bn, eo, ed, rgb in ([(1, 1, 1, 1)] if optional else [(0, 0, 0, 1), (1, 1, 0, 0)]):
        spec = [acc.h, n] + records(b) + [C.byref(wp), Dev(None, 0, None), Out(np.full(n, 0x55555555, np.uint32) if bn else None), Out(np.full((n, 3), 7.0) if eo else None),
                                          Out(np.full((n, 3), 7.0) if ed else None), Out(np.full((n, 3), 7.0, np.float32) if rgb else None), Dev(None)]
        outs = same_outputs("whitted", call_both(L, "lh_accel_whitted_host", "lh_accel_whitted_device", spec))
        if bn and eo:
            assert np.array_equal(outs[0] == MISS, ~hits)
            assert (outs[1][~hits] == 7.0).all() and (outs[1][hits] != 7.0).any(axis=1).all()          # a chain that ends at depth 0 keeps its end-ray slots
    return hits


def tile(fx, uniforms):
    """lh_render_ao_tile_host against lh_render_ao_tile into a tensor (no `n`: the tile is the window)"""
    import torch
    L, acc = fx.L, fx.acc
    uni = np.random.default_rng(3).uniform(0.0, 1.0, 2 * NS * WIN * WIN) if uniforms else None
    out = np.full((WIN, WIN, 3), 7.0, np.float32); st = binding.TileStats(); st_d = binding.TileStats()
    assert L.lh_render_ao_tile_host(acc.h, C.byref(fx.cam), 0, 0, WIN, WIN, 1, NS, 5, None if uni is None else uni.ctypes.data, 0 if uni is None else uni.size,
                                    out.ctypes.data, C.byref(st)) == 0, L.lh_last_error()
    d_uni = None if uni is None else torch.from_numpy(uni).cuda()
    d_out = torch.full((WIN, WIN, 3), 7.0, dtype=torch.float32, device="cuda")
    assert L.lh_render_ao_tile(acc.h, C.byref(fx.cam), 0, 0, WIN, WIN, 1, NS, 5, None if uni is None else d_uni.data_ptr(), d_out.data_ptr(), C.byref(st_d), None) == 0
    torch.cuda.synchronize()
    assert out.tobytes() == d_out.cpu().numpy().tobytes()
    assert 0 < st.primary_hits < st.primary_rays == WIN * WIN and (st.primary_hits, st.ao_rays, st.ao_occluded) == (st_d.primary_hits, st_d.ao_rays, st_d.ao_occluded)
    return out


@gpu
def test_every_host_form_through_one_block_that_grows_and_is_reused(fx):
    seen_hits = seen_misses = 0
    for k, n in enumerate(SIZES):
        hits = every_row(fx, n, optional=(k % 2 == 0))
        seen_hits += int(hits.sum()); seen_misses += int((~hits).sum())
        if n >= 257:
            assert hits.any() and (~hits).any()
        tile(fx, uniforms=(k % 2 == 0))
    assert seen_hits > 100 and seen_misses > 100
    # the sizes again with the optional arrays the other way round: the block is as large as it gets, every layout is a stale one's successor
    for k, n in enumerate(SIZES):
        every_row(fx, n, optional=(k % 2 == 1))
        tile(fx, uniforms=(k % 2 == 1))
    # the whole frame through the same block, tile by tile, is the frame of one tile
    whole, st = fx.acc.render_ao_frame_host(fx.cam, 1, NS, seed=5, tile=WIN)
    tiled, st4 = fx.acc.render_ao_frame_host(fx.cam, 1, NS, seed=5, tile=3)
    assert whole.tobytes() == tiled.tobytes() and st == st4 and whole.tobytes() == tile(fx, False).tobytes()


@gpu
def test_a_refused_call_between_two_good_ones(fx):
    L, acc = fx.L, fx.acc
    b = fx.batch(257)
    row = gather_rows(fx)[0]
    host, dev, spec = gather_spec(fx, row, b, 257, 1, 1, 1, 1)
    first = same_outputs(host, call_both(L, host, dev, spec))
    # both outputs NULL: refused before anything is staged
    n = 257
    assert L.lh_accel_ao_host(acc.h, n, b["org"].ctypes.data, b["dr"].ctypes.data, b["prim"].ctypes.data, b["t"].ctypes.data, b["u"].ctypes.data, b["v"].ctypes.data,
                              NS, 9, None, None, 0, None, None) == -1
    assert L.lh_last_error().decode() == "lh_accel_ao_host: both outputs are NULL"
    # too few uniforms: refused too
    assert L.lh_accel_ao_host(acc.h, n, b["org"].ctypes.data, b["dr"].ctypes.data, b["prim"].ctypes.data, b["t"].ctypes.data, b["u"].ctypes.data, b["v"].ctypes.data,
                              NS, 9, None, b["uni"].ctypes.data, 2 * NS * n - 1, first[0].ctypes.data, None) == -1
    assert L.lh_last_error().decode() == "lh_accel_ao_host: %d uniforms given, the batch may consume %d" % (2 * NS * n - 1, 2 * NS * n)
    # a raster window of no pixels, behind the arguments' own checks
    plane = binding.RasterPlane(0, WIN, b["plane"].frame, b["plane"].eye, b["plane"].fov)
    t = np.full((n, WIN, WIN), 7.0); st = np.full(n, 77, np.int32)
    assert L.lh_accel_beam_raster_host(acc.h, n, b["rorg"].ctypes.data, b["rdirs"].ctypes.data, b["rcorners"].ctypes.data, C.addressof(plane), t.ctypes.data,
                                       st.ctypes.data, None) == -1
    assert L.lh_last_error().decode() == "beam_raster: the raster window is 0 x %d" % WIN and (t == 7.0).all() and (st == 77).all()
    again = same_outputs(host, call_both(L, host, dev, spec))
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()
    # and another entry point's layout over the same block
    every_row(fx, 3, optional=True)
