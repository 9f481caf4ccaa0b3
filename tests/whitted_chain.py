"""The refraction chain (lucille_amd/csrc/lh_whitted.h) restated in numpy, for the tests: the bounce, and the chain of every eye hit as a
loop over a tracer that returns closest hits with their ri_intersection_state_build records (po.Oracle.state_batch, or the compiled
reference's).  A helper, not a test module."""
import numpy as np

MISS = 0xFFFFFFFF          # the miss primitive id; LH_AO_NO_HIT in `bounces`
CUT = 0x80000000           # LH_WHITTED_CUT
NORM_MIN = float(np.float32(1.0e-17))          # ri_vector_normalize's float literal, widened
DEFAULTS = (1.0e-7, 1.33, 8)                   # eps, eta, max_depth (whitted.c:38,46,24)


def refract_np(I, n, eta):
    """the direction a hit sends the chain on in: (R [m, 3], total-reflection flags [m]).  Every step one IEEE fp64 operation in the
    rule's order; eta a scalar or an array [m]"""
    I = np.asarray(I, np.float64).reshape(-1, 3); n = np.asarray(n, np.float64).reshape(-1, 3)
    eta = np.broadcast_to(np.asarray(eta, np.float64), (I.shape[0],))
    with np.errstate(all="ignore"):
        cos1 = (I[:, 0] * n[:, 0] + I[:, 1] * n[:, 1]) + I[:, 2] * n[:, 2]
        ent = cos1 < 0.0
        c = np.where(ent, -cos1, cos1)
        e = np.where(ent, 1.0 / eta, eta)
        N = np.where(ent[:, None], n, -n)
        coeff = 1.0 - (e * e) * (1.0 - c * c)
        tir = coeff <= 0.0
        s = (np.float32(2.0) * cos1.astype(np.float32)).astype(np.float64)          # the reference's float dot product, doubled as a float
        Rt = I - n * s[:, None]
        q = e * c - np.sqrt(np.where(tir, 0.0, coeff))
        Rr = q[:, None] * N + e[:, None] * I
        R = np.where(tir[:, None], Rt, Rr)
        n2 = (R[:, 0] * R[:, 0] + R[:, 1] * R[:, 1]) + R[:, 2] * R[:, 2]
        big = n2 > NORM_MIN
        r = 1.0 / np.sqrt(np.where(big, n2, 1.0))
        R = np.where(big[:, None], R * r[:, None], R)
    return R, tir


def bounce_np(P, n, I, eps, eta, refract=refract_np):
    """the next ray of the chain from P, n = Ns and I of a hit's state: (org, dir, total-reflection flags)"""
    R, tir = refract(I, n, eta)
    return np.asarray(P, np.float64).reshape(-1, 3) + eps * R, R, tir


def run_chain(tracer, prim0, st0, eps=DEFAULTS[0], eta=DEFAULTS[1], max_depth=DEFAULTS[2], refract=refract_np):
    """the chain of every record of (prim0 [n], st0 [n, 24]) -- the eye rays' closest hits and states -- over tracer(org, dir) ->
    (prim, state).  Returns (bounces uint32 [n]: MISS for a miss record, d for a chain whose ray d escaped, d | CUT for a chain cut at
    the limit; end_org, end_dir [n, 3]: the last ray traced for the record, NaN where there is none; info: rays per depth (index d),
    total reflections, cut chains, chain rays with |dir.y| <= 1e-14 (the reference's undefined case) and chain rays that hit the
    primitive they left)"""
    prim0 = np.asarray(prim0, np.uint32); n = prim0.shape[0]
    bounces = np.full(n, MISS, np.uint32)
    end_org = np.full((n, 3), np.nan); end_dir = np.full((n, 3), np.nan)
    alive = np.nonzero(prim0 != MISS)[0]
    st = np.asarray(st0, np.float64)[alive]; left = prim0[alive]
    info = {"rays": [0] * (max_depth + 1), "tir": 0, "cut": 0, "grazing": 0, "selfhit": 0, "hits": int(alive.size)}
    if max_depth == 0:
        bounces[alive] = CUT; info["cut"] = int(alive.size)
    for d in range(1, max_depth + 1):
        if alive.size == 0:
            break
        o, r, tir = bounce_np(st[:, 0:3], st[:, 6:9], st[:, 20:23], eps, eta, refract)
        info["rays"][d] = int(alive.size); info["tir"] += int(tir.sum()); info["grazing"] += int((np.abs(r[:, 1]) <= 1e-14).sum())
        p, s2 = tracer(o, r)
        end_org[alive] = o; end_dir[alive] = r
        miss = p == MISS
        info["selfhit"] += int(((p == left) & ~miss).sum())
        bounces[alive[miss]] = d
        if d == max_depth:
            bounces[alive[~miss]] = np.uint32(d | CUT); info["cut"] = int((~miss).sum())
            break
        alive = alive[~miss]; st = s2[~miss]; left = p[~miss]
    return bounces, end_org, end_dir, info


def soup_with_normals(po, seed=11):
    """the 300-triangle soup with seeded per-vertex normals of length 0.5 - 2: (positions, indices, org, dir, normals)"""
    P, idx, org, dr = po.soup(300, 2000, 0.2, 5)
    rng = np.random.default_rng(seed)
    N = rng.standard_normal((P.shape[0], 3))
    N *= (rng.uniform(0.5, 2.0, P.shape[0]) / np.linalg.norm(N, axis=1))[:, None]
    return P, idx, org, dr, np.ascontiguousarray(N)
