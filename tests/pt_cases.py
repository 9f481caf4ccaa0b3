"""The path tracer's edge cases (lh_pt.h, lh_render.hip k_pt_decide / k_pt_scatter / pt_fix / pt_accumulate, lh_tile.hip pt_tile): the scenes,
materials, cameras, environments, frame sizes and seeds that tests/test_pt_cases.py (no GPU: do the inputs reach the branches they are for?
-- asked of the oracle's counters alone) and tests/test_gpu_pt_edges.py (the device against the oracle) share, and the three restatements
the expectations are made of:

  pt_fix_np         lh_render.hip's pt_fix in numpy float32, one IEEE operation per line
  lh_div_make_py    lh_pt.h's lh_div_make / lh_div in Python integers
  pixel_from_paths  a pixel of a pass from the oracle's per-path radiances: the integer sum of pt_fix over the paths that carry light,
                    converted once -- what k_pt_resolve writes into a zeroed frame, to the bit

A case is a dict: meshes (the dict format of tests/state_edges.py), mats (ten floats per mesh: kd, ks, kt, ior), cam (the 16 + 4 numbers both
camera structures are built from), tile (x0, y0, w, h), spp, seed, max_vertices, flags (the weightings to run) and reach: the oracle counters
(oracle.pyoracle.PT_COUNTERS) the case is there for, each of which its inputs must reach REACH_BAR times.  Test infrastructure."""
import functools

import numpy as np

import lucille_amd as la
from oracle import pyoracle as po
from tests import state_edges as se
from tests.golden.make_golden import apply_state_scene
from tests.helpers import load_golden

REACH_BAR = 16
DIFFUSE = (0.7, 0.6, 0.5)
PROBE_RGB = (1.0, 0.5, 2.0)


# ---- materials, cameras, environments --------------------------------------------------------------------------------------------
def mat(kd=0.0, ks=0.0, kt=0.0, ior=1.0):
    """ten floats: kd, ks, kt (a number or three), ior"""
    three = lambda x: [float(c) for c in x] if np.ndim(x) else [float(x)] * 3
    return three(kd) + three(ks) + three(kt) + [float(ior)]


def la_material(m10):
    return la.Material.make(kd=m10[0:3], ks=m10[3:6], kt=m10[6:9], ior=m10[9])


def camera(w, h, flength, c2w, rh=1, ortho=0):
    """the numbers of one camera: width, height, flength, cam2world [16] (row vectors: world = camera @ M), rh, ortho"""
    return {"w": int(w), "h": int(h), "flength": float(flength), "c2w": [float(x) for x in np.asarray(c2w, np.float64).reshape(16)],
            "rh": int(rh), "ortho": int(ortho)}


def cameras(cam):
    """-> (la.Camera, po.Camera) from the same 16 + 4 numbers"""
    out = []
    for cls in (la.Camera, po.Camera):
        c = cls(); c.width, c.height, c.rh, c.ortho, c.flength = cam["w"], cam["h"], cam["rh"], cam["ortho"], cam["flength"]
        for i in range(16):
            c.cam2world[i] = cam["c2w"][i]
        out.append(c)
    return tuple(out)


def eye_matrix(eye, rot=None, scale=(1.0, 1.0, 1.0)):
    """cam2world = diag(scale) x rot x translation to `eye` (row vectors: a camera-space vector is scaled, turned, then moved)"""
    m = np.eye(4)
    m[:3, :3] = np.diag(scale) @ (np.eye(3) if rot is None else np.asarray(rot, np.float64))
    m[3, :3] = eye
    return m


def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`, as the matrix row vectors are multiplied with"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return (np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)).T


def aimed(target, distance, rot, rh, scale=(1.0, 1.0, 1.0)):
    """cam2world of a camera turned by `rot` that looks at `target` from `distance` away: the view direction is -z of the camera for rh = 1,
    +z for rh = 0 (camera.c:248-318)"""
    look = np.array([0.0, 0.0, -1.0 if rh else 1.0]) @ np.asarray(rot, np.float64)
    return eye_matrix(np.asarray(target, np.float64) - distance * look, rot, scale)


def random_probe():
    """the light probe tests/test_gpu_pt_oracle.py draws"""
    return np.random.default_rng(11).uniform(0.1, 2.0, (32, 48, 4)).astype(np.float32)


def flat_probe(c=0.3):
    """every texel the float c: a fetch is float(c x (w0 + w1 + w2 + w3)) = c whatever acos returned"""
    return np.full((8, 12, 4), np.float32(c), np.float32)


# constant environments of the exact pixel sums: (name, rgb)
CONSTANT_ENVS = (("positive", (0.9, 0.8, 0.7)),
                 ("negative, carry and NaN", (-0.75, -1.0e-10, float("nan"))),
                 ("clamped", (1.0e9, -1.0e9, 0.5)))


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _mesh(P, idx, two_side=0, **attr):
    m = {"P": np.ascontiguousarray(P, np.float64), "idx": np.ascontiguousarray(idx, np.uint32), "two_side": int(two_side)}
    m.update({k: np.ascontiguousarray(a, np.float64) for k, a in attr.items()})
    return m


@functools.lru_cache(maxsize=None)
def plane_meshes():
    """the 100 x 100 square at z = 0 of tests/test_oracle_ptref.py"""
    P = np.array([[-50.0, -50.0, 0.0], [50.0, -50.0, 0.0], [50.0, 50.0, 0.0], [-50.0, 50.0, 0.0]])
    return (_mesh(P, [0, 1, 2, 0, 2, 3]),)


@functools.lru_cache(maxsize=None)
def ps_meshes(colours=True):
    """tests/golden/ao_ps.npz: mesh 0 the sphere (1 984 triangles, normals), mesh 1 the two-triangle plane -- here with vertex colours"""
    g = load_golden("ao_ps")
    out = []
    for k in range(int(g["ngeoms"])):
        attr = {"N": g["nrm%d" % k]} if ("nrm%d" % k) in g.files else {}
        if colours and k == 1:
            attr["C"] = np.array([[1.0, 0.5, 0.25], [0.5, 1.0, 0.75], [0.75, 0.25, 1.0], [0.25, 0.75, 0.5]])
        out.append(_mesh(g["pos%d" % k], g["idx%d" % k], int(g["two_side%d" % k]), **attr))
    assert out[0]["idx"].shape[0] == 3 * 1984 and out[1]["idx"].shape[0] == 6
    return tuple(out)


def ps_camera(w=96, h=96):
    c = load_golden("ao_ps")["camera"]
    return camera(w, h, c[16], c[:16], int(c[19]))


@functools.lru_cache(maxsize=None)
def edge_meshes():
    return tuple(se.edge_scene(7)[0])


def oracle_of(meshes):
    o = po.Oracle(); apply_state_scene(o, meshes, False); o.build()
    return o


def accel_of(meshes):
    """a committed la.HipAccel of the meshes (GPU)"""
    acc = la.HipAccel(0); apply_state_scene(acc, meshes, False); acc.commit()
    return acc


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _case(name, meshes, mats, cam, spp, seed, reach, tile=None, max_vertices=8, flags=(0,)):
    assert len(mats) == len(meshes)
    return {"name": name, "meshes": meshes, "mats": [list(m) for m in mats], "cam": cam, "tile": tile or (0, 0, cam["w"], cam["h"]),
            "spp": spp, "seed": seed, "max_vertices": max_vertices, "flags": tuple(flags), "reach": tuple(reach)}


BOTH = (0, la.PT_REFERENCE_WEIGHTS)
GLASS = mat(kd=0.2, ks=0.1, kt=0.7, ior=1.5)
E1_CENTRE = (26.0, 12.0, 0.0)
TURN = rotation((1.0, 2.0, 3.0), 0.4)                 # not about an axis


def _tiny_view(k, rotated):
    """a 16 x 16 frame, flength 2000, from 0.1 above the centroid of E0's k-th tiny triangle (tests/state_edges.py TINY_LEGS), looking
    along its normal: the window is 1e-4 wide"""
    m = edge_meshes()[se.FAMILIES.index("E0")]
    tri = m["P"][3 * (k + (len(se.TINY_LEGS) if rotated else 0)):][:3]
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    x = e1 / np.linalg.norm(e1); z = np.cross(e1, e2); z = z / np.linalg.norm(z)
    rot = np.stack([x, np.cross(z, x), z])              # rows: the camera's axes in the world
    return camera(16, 16, 2000.0, eye_matrix(tri.mean(axis=0) + 0.1 * z, rot), 1)


@functools.lru_cache(maxsize=None)
def branch_cases():
    """S1 - S4: every branch of the vertex arithmetic"""
    plane, ps, edge = plane_meshes(), ps_meshes(), edge_meshes()
    down = camera(24, 16, 1.0, eye_matrix((0.0, 0.0, 5.0)), 1)
    nedge = len(edge)
    out = [
        # S1: a lone plane of glass whose relative index 1 / 0.6 turns most refractions into reflections
        _case("S1 glass plane", plane, [mat(kt=1.0, ior=0.6)], down, 4, 3, ("tir", "refracted", "miss_later"), flags=BOTH),
        _case("S1 mixed plane", plane, [mat(kd=0.3, ks=0.3, kt=0.3, ior=0.6)], down, 4, 3,
              ("tir", "refracted", "diffuse", "mirror", "roulette", "axis0"), flags=BOTH),
        # S2: the sphere of glass over the coloured plane
        _case("S2 glass sphere", ps, [GLASS, mat(kd=DIFFUSE)], ps_camera(48, 48), 4, 5,
              ("tir", "interior", "refracted", "mirror", "diffuse", "back", "normals", "colours", "roulette", "limit", "miss_first", "miss_later"),
              max_vertices=12, flags=BOTH),
        # S3: E1's normals on the +-0.6 thresholds from above, and mirrored (left-handed, from below)
        _case("S3 thresholds rh", edge, [mat(kd=DIFFUSE)] * nedge, camera(48, 32, 0.5, eye_matrix((26.0, 12.0, 15.0)), 1), 16, 7,
              ("axis0", "axis1", "axis2", "back", "diffuse")),
        _case("S3 thresholds lh", edge, [mat(kd=DIFFUSE)] * nedge, camera(48, 32, 0.5, eye_matrix((26.0, 12.0, -15.0)), 0), 16, 7,
              ("axis0", "axis1", "axis2", "diffuse")),
    ]
    # S4: the two smallest E0 triangles (legs 5e-5 and 3e-5), in the axis plane and rotated: Ng stays unnormalised
    for rotated in (False, True):
        for k in (3, 4):
            out.append(_case("S4 tiny %g%s" % (se.TINY_LEGS[k], " rotated" if rotated else ""), edge, [mat(kd=DIFFUSE)] * nedge,
                             _tiny_view(k, rotated), 4, 9, ("flat_unnormalised", "diffuse")))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def camera_cases():
    """S5: the cameras pt_primary_ray has no other test of -- orthographic, both handednesses, a cam2world that is a rotation not about an
    axis times a non-uniform scale, width != height, tiles off the origin that are narrower than the frame"""
    ps, edge = ps_meshes(), edge_meshes()
    nedge = len(edge)
    out = []
    for rh in (1, 0):
        # orthographic: the window is cam2world's scale, 56 x 34 around E1, seen at a slant so that the upright triangles show
        out.append(_case("S5 ortho rh=%d" % rh, edge, [mat(kd=DIFFUSE)] * nedge,
                         camera(48, 32, 0.5, aimed(E1_CENTRE, 40.0, TURN, rh, (28.0, 17.0, 1.0)), rh, 1), 16, 13,
                         ("diffuse", "miss_first"), tile=(5, 3, 41, 27)))
        # perspective through the same turned and scaled matrix
        out.append(_case("S5 turned rh=%d" % rh, edge, [mat(kd=DIFFUSE)] * nedge,
                         camera(48, 32, 1.0, aimed(E1_CENTRE, 30.0, TURN, rh, (1.3, 0.8, 1.0)), rh, 0), 16, 13,
                         ("diffuse", "miss_first"), tile=(3, 2, 43, 29)))
    c = ps_camera(40, 24)
    m = np.array(c["c2w"]).reshape(4, 4)
    m = eye_matrix((0.0, 0.0, 0.0), rotation((3.0, 1.0, 2.0), 0.1), (1.3, 0.8, 1.0)) @ m
    out.append(_case("S5 glass sphere, scaled and turned", ps, [GLASS, mat(kd=DIFFUSE)], camera(40, 24, c["flength"], m, c["rh"]), 4, 5,
                     ("tir", "interior", "diffuse", "miss_first", "colours", "normals"), tile=(7, 5, 23, 13), max_vertices=12))
    out.append(_case("S5 glass sphere, orthographic", ps, [GLASS, mat(kd=DIFFUSE)],
                     camera(40, 24, c["flength"], eye_matrix((0.0, 0.0, 0.0), None, (5.0, 3.0, 1.0)) @ np.array(c["c2w"]).reshape(4, 4), c["rh"], 1),
                     4, 5, ("tir", "interior", "diffuse", "miss_first"), tile=(1, 2, 37, 21), max_vertices=12))
    return tuple(out)


SUM_FRAMES = ((23, 17), (7, 5))
SUM_SPP = (1, 2, 3, 63, 64, 65, 100, 257)      # runs of one lane, runs that straddle a wave, runs longer than a wave


def sum_case(w, h, spp):
    """the exact pixel sums: ao_ps all diffuse, a frame that is no power of two.  23 x 17 x 65 is more than three decide spans of 8 192 paths"""
    big = w * h * spp >= 500
    return _case("sums %d x %d x %d" % (w, h, spp), ps_meshes(), [mat(kd=DIFFUSE)] * 2, ps_camera(w, h), spp, 21,
                 ("miss_first", "miss_later") if big else ())


def sum_cases():
    return tuple(sum_case(w, h, spp) for (w, h) in SUM_FRAMES for spp in SUM_SPP)


CHAIN_VERTICES = (2, 3, 9, 10, 17, 18)          # pt_tile reads a count back after bounces 7 and 15: chains that end either side of each


@functools.lru_cache(maxsize=None)
def slab_meshes():
    """the square twice, 20 apart: between the two a path of reflectance 1 goes on for dozens of vertices, and some leave at every bounce"""
    P = plane_meshes()[0]["P"]
    return (_mesh(P, [0, 1, 2, 0, 2, 3]), _mesh(P + np.array([0.0, 0.0, 20.0]), [0, 1, 2, 0, 2, 3]))


def chain_cases():
    """reflectance 1 between two planes, seen from between them: most paths live until the vertex limit (in ao_ps a handful of
    samples that bounce into the closed sphere do); and the lone plane under a limit of 400, where every path has ended long before the
    first read-back"""
    between = camera(24, 16, 1.0, eye_matrix((0.0, 0.0, 10.0)), 1)
    out = [_case("chain %d" % mv, slab_meshes(), [mat(kd=1.0)] * 2, between, 4, 17, ("limit",), max_vertices=mv) for mv in CHAIN_VERTICES]
    out.append(_case("chain plane 400", plane_meshes(), [mat(kd=1.0)], camera(24, 16, 1.0, eye_matrix((0.0, 0.0, 5.0)), 1), 4, 3,
                     ("diffuse", "miss_later"), max_vertices=400))
    return tuple(out)


DIV_W = (1, 3, 23, 41)
DIV_SPP = (1, 3, 7, 100)
DIV_BAND_ROWS = (1, 3, 5)                        # band_stride = 3 x band_rows: the bands three ranks would own


def division_tile_cases():
    """tiles whose width and sample count are odd and not one less than a power of two (and 1, lh_div's `one`), off the frame's origin"""
    return tuple(_case("div tile w %d spp %d" % (w, spp), ps_meshes(), [mat(kd=DIFFUSE)] * 2, ps_camera(96, 96), spp, 23, (), tile=(37, 20, w, 5))
                 for w in DIV_W for spp in DIV_SPP)


def division_band_case(spp):
    """a 41 x 45 frame for render_pt_bands: 45 lines are whole bands of 1, 3 and 5 lines for three ranks"""
    return _case("div bands spp %d" % spp, ps_meshes(), [mat(kd=DIFFUSE)] * 2, ps_camera(41, 45), spp, 29, ("diffuse", "miss_first", "miss_later"))


def all_cases():
    return (branch_cases() + camera_cases() + sum_cases() + chain_cases() + division_tile_cases() + tuple(division_band_case(s) for s in (3, 7)))


def render_oracle(o, case, flags=0, env_rgb=(1.0, 1.0, 1.0), env_map=None, **over):
    """Oracle.render_pt(detail=True) of a case -> (frame, stats, rays per path, radiance per path, counters)"""
    c = dict(case); c.update(over)
    x0, y0, w, h = c["tile"]
    return o.render_pt(cameras(c["cam"])[1], x0, y0, w, h, 0, c["spp"], c["spp"], max_vertices=c["max_vertices"], materials=c["mats"],
                       env_rgb=env_rgb, env_map=env_map, ref_weights=flags, seed=c["seed"], detail=True)


# ---- restatements ----------------------------------------------------------------------------------------------------------------
FIX_CLAMP = np.float32(262144.0)


def pt_fix_np(r):
    """lh_render.hip pt_fix, line by line in float32 -> the 64-bit fixed-point word (32 fraction bits) as int64 (two's complement)"""
    r = np.asarray(r, np.float32)
    r = np.minimum(np.maximum(r, -FIX_CLAMP), FIX_CLAMP)                # fminf(fmaxf(r, -clamp), clamp)
    fl = np.floor(r)                                                      # floorf
    fr = r - fl
    carry = fr >= np.float32(1.0)
    fr = np.where(carry, np.float32(0.0), fr)
    fl = np.where(carry, fl + np.float32(1.0), fl)
    lo = fr * np.float32(4294967296.0)
    assert lo.dtype == np.float32 and fl.dtype == np.float32
    lo = lo.astype(np.uint64).astype(np.int64)                            # (uint32_t): in range after the carry
    assert (lo < (1 << 32)).all()
    return (fl.astype(np.int32).astype(np.int64) << 32) | lo


def pixel_from_paths(rad, spp_total):
    """rad: float32 [pixels, samples of the pass, 3] -> float32 [pixels, 3]: what one pass adds to a zeroed pixel.  pt_accumulate /
    pt_accumulate_uniform: the integer sum of pt_fix(r) over the paths whose r is neither NaN nor 0; k_pt_resolve: that sum as a double
    x 2^-32, rounded to float once, x (1.0f / spp_total), + 0"""
    rad = np.asarray(rad, np.float32)
    valid = (rad == rad) & (rad != 0.0)
    with np.errstate(invalid="ignore"):
        fix = np.where(valid, pt_fix_np(np.where(valid, rad, np.float32(0.0))), np.int64(0))
    v = fix.sum(axis=1, dtype=np.int64)
    s = (v.astype(np.float64) * 2.3283064365386963e-10).astype(np.float32)
    inv = np.float32(1.0) / np.float32(spp_total)
    return np.float32(0.0) + s * inv


def frame_from_paths(rad, w, h, spp_total):
    """pixel_from_paths in the frame's orientation: [h, w, 3], top line first (the oracle's pixels come bottom line first)"""
    return np.ascontiguousarray(pixel_from_paths(rad, spp_total).reshape(h, w, 3)[::-1])


def lh_div_make_py(d, plus_one=1):
    """lh_pt.h lh_div_make -> (m, sh, one)"""
    if d <= 1:
        return 0, 0, 1
    l = 0
    while (1 << l) < d:
        l += 1
    k = max(30 + l, 32)
    return (1 << k) // d + plus_one, k - 32, 0


def lh_div_py(n, dv):
    """lh_pt.h lh_div: __umulhi(n, m) >> sh"""
    m, sh, one = dv
    return n if one else ((n * m) >> 32) >> sh
