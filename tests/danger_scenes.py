"""Scenes and rays for the edges of the routing decision around zero-area triangles that stay in the traversal tree
(lh_danger.h, lh_walk.h ray_needs_ref_walk, lh_hostwalk.c lh_danger_hit): shared by tests/test_danger_routing_model.py (CPU model)
and tests/test_gpu_danger_routing.py (device).  Test infrastructure.

The live triangles span exactly [0, 1]^3, so the scene's 16-bit grid starts at 0 and one cell is (1 / 65535) (1 + 1e-6) rounded
up to float32 (lh_bvh.c setup_grid).  CELL is the nominal 1 / 65535: the scenes are placed with it, the tests that need the exact
step read it from the built scene."""
import numpy as np

CELL = 1.0 / 65535.0
LINE_A = np.array([0.07, 0.4, 0.4])
LINE_U = np.array([0.6, 0.1, 0.79]) / np.linalg.norm([0.6, 0.1, 0.79])
CORNERS = np.array([[[0.0, 0.0, 0.0], [0.2, 0.05, 0.1], [0.05, 0.2, 0.1]],
                    [[1.0, 1.0, 1.0], [0.8, 0.95, 0.9], [0.95, 0.8, 0.9]]])          # they pin the live bounds to [0, 1]^3


def _line(high, a=LINE_A):
    """the collinear triangle's line (a, u); high: the scene mirrored in x about 0.5"""
    a = a.copy(); u = LINE_U.copy()
    if high:
        a[0] = 1.0 - a[0]; u[0] = -u[0]
    return a, u


def _mirror(T, high):
    if high:
        T = T.copy(); T[..., 0] = 1.0 - T[..., 0]
    return T


def _dead(high, y, z, v2=None):
    """a dead triangle (v0 == v1: the traversal tree drops it, lucille's own tree keeps it) half a cell outside the live bounds in x;
    v2: its third vertex (default: half a cell outside as well)"""
    x = 1.0 + 0.5 * CELL if high else -0.5 * CELL
    v2 = [x, y + 0.01, z + 0.02] if v2 is None else [1.0 - v2[0] if high else v2[0], v2[1], v2[2]]
    return np.array([[[x, y, z], [x, y, z], v2]])


def one_leaf_scene(high=False, dead=True):
    """12 triangles (11 without the dead one), one leaf in lucille's own tree: 10 live ones with bounds exactly [0, 1]^3, one
    collinear triangle on LINE_A + s LINE_U (s = 0, 0.35, 0.6: |e1|_1 |e2|_1 = 0.469, a cap of 2.13), one dead triangle half a cell
    below x = 0 (high: the mirror image, half a cell above x = 1).  -> P, idx, dict(a, u, zprim)"""
    rng = np.random.default_rng(21)
    c = rng.uniform(0.15, 0.85, (8, 1, 3)); live = np.concatenate([CORNERS, c + rng.uniform(-0.1, 0.1, (8, 3, 3))])
    a, u = _line(high)
    Z = np.stack([a, a + 0.35 * u, a + 0.6 * u])[None]
    parts = [_mirror(live, high), Z] + ([_dead(high, 0.4, 0.3)] if dead else [])
    P = np.concatenate(parts).reshape(-1, 3).copy()
    return P, np.arange(P.shape[0], dtype=np.uint32), dict(a=a, u=u, zprim=10, smax=0.6)


def many_leaf_scene(high=False, dead=True):
    """402 live triangles in [0, 1]^3 (two of them the corner triangles), a collinear triangle that starts 0.0005 from the x = 0
    face (s = 0, 0.2, 0.35 on its line: a cap of 6.4) and the dead triangle beside it, half a cell outside.
    -> P, idx, dict(a, u, zprim)"""
    rng = np.random.default_rng(22)
    c = rng.uniform(0.03, 0.97, (400, 1, 3)); live = np.concatenate([CORNERS, c + rng.uniform(-0.03, 0.03, (400, 3, 3))])
    a, u = _line(high, np.array([0.0005, 0.4, 0.4]))
    Z = np.stack([a, a + 0.2 * u, a + 0.35 * u])[None]
    # the dead triangle's third vertex puts its centroid on the collinear triangle's: the builder bins them together
    parts = [_mirror(live, high), Z] + ([_dead(high, 0.41, 0.45, (0.33, 0.44, 0.73))] if dead else [])
    P = np.concatenate(parts).reshape(-1, 3).copy()
    return P, np.arange(P.shape[0], dtype=np.uint32), dict(a=a, u=u, zprim=402, smax=0.35)


def _scaled(rng, org, w):
    """directions w (unit length, at most one component that is not in the plane: largest component >= 0.7) scaled by 100-1000: every
    largest component beyond the scenes' caps and below 1024"""
    dr = w * rng.uniform(100.0, 1000.0, (w.shape[0], 1))
    return np.ascontiguousarray(org), np.ascontiguousarray(dr)


def _yz_unit(rng, n):
    """unit vectors (0, wy, wz) with |wy| > 2e-3: the reference leaves its y reciprocal unset below 1e-14 |dir| (bvh.c:483-487) and the
    contract starts at 1e-3"""
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    ang = np.where(np.abs(np.sin(ang)) > 2e-3, ang, ang + 0.01)
    return np.stack([np.zeros(n), np.sin(ang), np.cos(ang)], 1)


def strip_rays(n, info, high=False, seed=5):
    """rays that run through the strip between the live bounds and the dead triangle: each passes through the point where the
    collinear triangle's EXTENDED line crosses x = xc, xc in (-0.42, -0.23) cell (high: mirrored beyond x = 1), almost inside the
    plane x = xc (|dir.x| <= 1e-7 |dir|, never 0), from an origin less than one scene extent away"""
    rng = np.random.default_rng(seed)
    a, u = info["a"], info["u"]
    off = rng.uniform(0.23, 0.42, n) * CELL
    xc = 1.0 + off if high else -off
    p = a[None] + ((xc - a[0]) / u[0])[:, None] * u[None]; p[:, 0] = xc
    w = _yz_unit(rng, n)
    w[:, 0] = rng.uniform(1e-9, 1e-7, n) * rng.choice([-1.0, 1.0], n)
    org = p - rng.uniform(0.05, 0.9, (n, 1)) * w
    return _scaled(rng, org, w)


def strip_x_range(org, dr, box_lo, box_hi):
    """fp64: the x range of each ray while it is inside the box's y and z slabs (t >= 0) -> (xmin, xmax), NaN where it never is"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = np.zeros(org.shape[0]); t1 = np.full(org.shape[0], np.inf)
        for k in (1, 2):
            ta = (box_lo[k] - org[:, k]) / dr[:, k]; tb = (box_hi[k] - org[:, k]) / dr[:, k]
            t0 = np.maximum(t0, np.minimum(ta, tb)); t1 = np.minimum(t1, np.maximum(ta, tb))
        xa = org[:, 0] + t0 * dr[:, 0]; xb = org[:, 0] + t1 * dr[:, 0]
    ok = t0 <= t1
    return np.where(ok, np.minimum(xa, xb), np.nan), np.where(ok, np.maximum(xa, xb), np.nan)


AXIS_FAMILIES = ("dx0", "dz0", "dx0dz0")


def axis_rays(n, info, family, seed=5, face=None, box=None):
    """axis-parallel rays through the collinear triangle's line: family "dx0" (dir.x == 0 exactly), "dz0", "dx0dz0" (along +-y).
    face=None: through points of the triangle itself (s in 0 .. 0.6 of its line; the many-leaf scene: 0 .. 0.35).  face=(axis, side, ulps) with a box (lo, hi): the origins' coordinate on
    `axis` -- one with a zero direction component -- lies on that face of the box (side 0 low, 1 high), `ulps` doubles inside (+)
    or outside (-) of it, and the ray passes through the point where the triangle's EXTENDED line crosses that plane."""
    rng = np.random.default_rng(seed)
    a, u = info["a"], info["u"]
    if face is None:
        s = rng.uniform(0.0, info["smax"], (n, 1))
    else:
        axis, side, ulps = face
        c = float(box[side][axis])
        for _ in range(abs(ulps)):
            c = float(np.nextafter(c, (np.inf if (side == 0) == (ulps > 0) else -np.inf)))
        s = np.full((n, 1), (c - a[axis]) / u[axis])
    p = a[None] + s * u[None]
    if face is not None:
        p[:, axis] = c
    if family == "dx0":
        w = _yz_unit(rng, n)
    elif family == "dz0":
        w = _yz_unit(rng, n)[:, [2, 1, 0]]
    else:
        w = np.zeros((n, 3)); w[:, 1] = rng.choice([-1.0, 1.0], n)
    org = p - rng.uniform(0.05, 0.9, (n, 1)) * w
    if face is not None:
        org[:, axis] = c
    # the LARGEST component D = 1000 sqrt(U(0.01, 1)): 100-1000 like the strip rays', with a density that rises with D -- the noise
    # of the reference's determinant grows with D, and it reports the triangle on 6 % of such rays at D = 900 and on none at D = 100
    dr = w / np.abs(w).max(1, keepdims=True) * (1000.0 * np.sqrt(rng.uniform(0.01, 1.0, (n, 1))))
    return np.ascontiguousarray(org), np.ascontiguousarray(dr)
