"""One edge scene for the hit epilogue (ri_intersection_state_build, intersection_state.c:99-248) and every copy of it the product
holds: k_state_build / state_core (lh_shade.h), ao_hit_epilogue (lh_render.hip), pt_scatter (lh_pt.h), the host mirror (lh_host.c),
and the flatten / gather that feed them (lh_commit.hip, lh_flatten.hip k_gather_attributes).  Shared by tests/test_oracle_state.py
(CPU: oracle against the compiled reference) and tests/test_gpu_state.py (device).  Test infrastructure.

The families, one or two meshes each, in the dict format tests.golden.make_golden.apply_state_scene takes:
  E0  tiny flat right triangles (legs 1e-3 ... 3e-5), once in an axis plane and once rotated: the two smallest have |e1 x e2|^2 below
      ri_vector_normalize's 1e-17f, so Ng (and Ns, and the ortho basis built on it) stays unnormalised
  E1  flat triangles in exact integer coordinates whose normals sit on ri_ortho_basis's +-0.6 comparisons (3-4-5 triples), the six
      axis directions and three ordinary ones; E1n: the same triangles with normals, tangents and binormals (the branch not taken)
  E2  tangents and binormals WITHOUT normals (the reference ignores them there)
  E3  normals and tangents without binormals; the normals are not unit length (1e-2 ... 50), one triangle's are all zero and one
      vertex other triangles share has a zero normal
  E4  unit normals, binormals without tangents, shared AND unshared texture coordinates (the shared ones win)
  E5  two_side, 5 triangles, no normals: inside = (index >= nindices / 2) on INDICES is 0, 0, 0, 1, 1
  E6  two_side, 7 triangles, normals and colours
The meshes sit far apart and every ray starts closer to its triangle than any other triangle is, so nothing occludes anything."""
import numpy as np

MISS = 0xFFFFFFFF
FAMILIES = ("E0", "E1", "E1n", "E2", "E3", "E4", "E5", "E6")
TINY_LEGS = (1e-3, 1e-4, 6e-5, 5e-5, 3e-5)
# (normal, e1, e2) in integers with e1 x e2 a positive multiple of the normal
# (the 3-4-5 ones: |e1 x e2| = 15, for which x / 15 gives 0.6 and 0.8 to the bit through 1 / sqrt(225); at 5 it gives 0.6000000000000001)
E1_EDGES = (((3, 4, 0), (0, 0, 3), (4, -3, 0)), ((-3, -4, 0), (4, -3, 0), (0, 0, 3)),
            ((0, 3, 4), (3, 0, 0), (0, 4, -3)), ((0, -3, -4), (0, 4, -3), (3, 0, 0)),
            ((4, 0, 3), (0, 3, 0), (-3, 0, 4)),
            ((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1), (0, 1, 0)),
            ((0, 1, 0), (0, 0, 1), (1, 0, 0)), ((0, -1, 0), (1, 0, 0), (0, 0, 1)),
            ((0, 0, 1), (1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0), (1, 0, 0)),
            ((1, 1, 1), (1, -1, 0), (0, 1, -1)), ((2, 2, 1), (1, -1, 0), (0, 1, -2)), ((3, 4, 12), (4, -3, 0), (0, 3, -1)))
BARY = ((1.0 / 3.0, 1.0 / 3.0), (0.1, 0.1), (0.8, 0.1), (0.1, 0.8))           # the four points of every triangle the rays go to
RECORD_UV = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (-0.25, 0.5), (1.5, -0.25), (5e-324, 0.0))
RECORD_T = (0.0, -1.0, 1.0, 1e30)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _strip(rng, ntri, base):
    """ntri triangles over ntri + 2 shared vertices, nearly in a plane: -> P [ntri + 2, 3], idx [3 ntri]"""
    i = np.arange(ntri + 2)
    P = np.stack([0.3 * i, 0.3 * (i % 2), rng.uniform(-0.02, 0.02, ntri + 2)], 1) + np.asarray(base, np.float64)
    idx = np.stack([i[:-2], i[1:-1], i[2:]], 1).reshape(-1).astype(np.uint32)
    return P, idx


def _tiny(rot, base):
    """the TINY_LEGS right triangles, legs along the first two columns of rot, 0.5 apart"""
    P = []
    for k, leg in enumerate(TINY_LEGS):
        v0 = np.asarray(base, np.float64) + np.array([0.5 * k, 0.0, 0.0])
        P += [v0, v0 + leg * rot[:, 0], v0 + leg * rot[:, 1]]
    return np.array(P)


def _e1():
    P = []
    for k, (n, e1, e2) in enumerate(E1_EDGES):
        assert np.array_equal(np.cross(e1, e2) * 1.0 / np.abs(np.cross(e1, e2)).max(), np.asarray(n) * 1.0 / np.abs(n).max())
        v0 = np.array([12.0 * (k % 5), 12.0 * (k // 5), 0.0])
        P += [v0, v0 + np.asarray(e1, np.float64), v0 + np.asarray(e2, np.float64)]
    P = np.array(P)
    assert np.array_equal(P, np.round(P))
    return P


def edge_scene(seed=7):
    """-> (meshes, org, dr): the meshes (each carries its family's name under "family"; apply_state_scene ignores it) and the rays: to
    BARY of every triangle from both sides, direction lengths in [0.5, 3].  Reproducible from the seed."""
    rng = np.random.default_rng(seed)
    meshes = []

    def mesh(family, P, idx, two_side=0, **attr):
        m = {"family": family, "P": np.ascontiguousarray(P, np.float64), "idx": np.ascontiguousarray(idx, np.uint32), "two_side": two_side}
        m.update({k: np.ascontiguousarray(a, np.float64) for k, a in attr.items()})
        meshes.append(m)

    # E0: the axis plane z = 0, and a frame that is no axis plane
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.4), -np.sin(0.4)], [0.0, np.sin(0.4), np.cos(0.4)]])
    P = np.concatenate([_tiny(np.eye(3), (0.0, -10.0, 0.0)), _tiny(rot, (2.5, -10.0, 0.0))])
    mesh("E0", P, np.arange(P.shape[0]))
    # E1 / E1n
    P = _e1()
    mesh("E1", P, np.arange(P.shape[0]))
    n = P.shape[0]
    mesh("E1n", P + np.array([0.0, 0.0, 30.0]), np.arange(n), N=_unit(rng.normal(size=(n, 3))), T=_unit(rng.normal(size=(n, 3))),
         B=_unit(rng.normal(size=(n, 3))))
    # E2: T and B, no N
    P, idx = _strip(rng, 6, (0.0, -20.0, 0.0))
    mesh("E2", P, idx, T=_unit(rng.normal(size=P.shape)), B=_unit(rng.normal(size=P.shape)))
    # E3: N (any length; zeros) and T, no B.  8 strip triangles and one with vertices of its own whose normals are all zero
    P, idx = _strip(rng, 8, (0.0, -30.0, 0.0))
    P = np.concatenate([P, np.array([[3.5, -30.0, 0.0], [3.8, -30.0, 0.01], [3.5, -29.7, 0.0]])])
    idx = np.concatenate([idx, np.array([10, 11, 12], np.uint32)])
    N = _unit(rng.normal(size=P.shape)) * np.geomspace(1e-2, 50.0, P.shape[0])[rng.permutation(P.shape[0])][:, None]
    N[10:13] = 0.0                          # a whole triangle
    N[4] = 0.0                              # a vertex of triangles 2, 3 and 4
    mesh("E3", P, idx, N=N, T=_unit(rng.normal(size=P.shape)))
    # E4: unit N, B without T, ST and STU
    P, idx = _strip(rng, 6, (0.0, -40.0, 0.0))
    mesh("E4", P, idx, N=_unit(rng.normal(size=P.shape)), B=_unit(rng.normal(size=P.shape)), ST=rng.uniform(0, 4, (P.shape[0], 2)),
         STU=rng.uniform(-1, 1, (idx.shape[0], 2)))
    # E5, E6: two_side with an odd number of triangles
    P, idx = _strip(rng, 5, (0.0, -50.0, 0.0))
    mesh("E5", P, idx, two_side=1)
    P, idx = _strip(rng, 7, (0.0, -60.0, 0.0))
    mesh("E6", P, idx, two_side=1, N=_unit(rng.normal(size=P.shape)), C=rng.uniform(0, 1, P.shape))
    assert tuple(m["family"] for m in meshes) == FAMILIES

    T = triangles(meshes)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    nrm = _unit(np.cross(e1, e2)); a1 = _unit(e1); a2 = np.cross(nrm, a1)
    org, dr = [], []
    for (u, v) in BARY:
        for side in (1.0, -1.0):
            tgt = T[:, 0] + u * e1 + v * e2
            tilt = rng.uniform(-0.3, 0.3, (T.shape[0], 2))
            d = _unit(-side * nrm + tilt[:, :1] * a1 + tilt[:, 1:] * a2)
            o = tgt - d * rng.uniform(0.5, 1.5, (T.shape[0], 1))
            org.append(o); dr.append(d * rng.uniform(0.5, 3.0, (T.shape[0], 1)))
    return meshes, np.ascontiguousarray(np.concatenate(org)), np.ascontiguousarray(np.concatenate(dr))


def triangles(meshes):
    """[ntri, 3, 3] in primitive-id order (meshes in order, triangles in index order)"""
    return np.concatenate([m["P"][m["idx"].astype(np.int64)].reshape(-1, 3, 3) for m in meshes if m["idx"].shape[0] >= 3])


def family_of_prim(meshes):
    """per primitive id: the index into FAMILIES of its mesh"""
    return np.concatenate([np.full(m["idx"].shape[0] // 3, FAMILIES.index(m["family"])) for m in meshes])


def edge_records(meshes, seed=7):
    """-> (org, dr, prim, t, u, v): records a caller made, not a ray.  Per primitive RECORD_UV x RECORD_T with an ordinary direction,
    then one direction of length 1e-10 (below the normalise threshold: I stays as it is) and one of length 1e200; every seventh slot is a
    miss (LH_MISS_PRIM) with the values of the record it replaces"""
    rng = np.random.default_rng(seed + 1000)
    ntri = triangles(meshes).shape[0]
    uv = np.array([(u, v) for (u, v) in RECORD_UV for _ in RECORD_T] + [(0.25, 0.25)] * 2)
    tt = np.array([t for _ in RECORD_UV for t in RECORD_T] + [1.0, 1.0])
    per = uv.shape[0]
    prim = np.repeat(np.arange(ntri, dtype=np.uint32), per)
    u = np.tile(uv[:, 0], ntri); v = np.tile(uv[:, 1], ntri); t = np.tile(tt, ntri)
    length = np.tile(np.concatenate([rng.uniform(0.5, 3.0, per - 2), [1e-10, 1e200]]), ntri)
    dr = _unit(rng.normal(size=(prim.shape[0], 3))) * length[:, None]
    org = rng.uniform(-5.0, 5.0, (prim.shape[0], 3))
    prim[6::7] = MISS
    assert np.isfinite(dr).all() and (prim == MISS).sum() >= prim.shape[0] // 7
    return (np.ascontiguousarray(org), np.ascontiguousarray(dr), np.ascontiguousarray(prim), np.ascontiguousarray(t), np.ascontiguousarray(u),
            np.ascontiguousarray(v))


def ortho_axis(n):
    """ri_ortho_basis's choice (reflection.c:311-333): the first axis whose component is inside (-0.6, 0.6), else 0.  n: [k, 3]"""
    inside = (n < 0.6) & (n > -0.6)
    return np.where(inside.any(axis=1), inside.argmax(axis=1), 0)


def assert_coverage(meshes, prim, state):
    """what the edge scene is for, on the REFERENCE's or the ORACLE's records of its rays (never the product's)"""
    hit = prim != MISS
    fam = family_of_prim(meshes)
    per_family = np.bincount(fam[prim[hit]], minlength=len(FAMILIES))
    assert (per_family > 0).all(), per_family                                           # every family is hit
    ng = np.linalg.norm(state[:, 3:6], axis=1)
    assert np.unique(prim[hit & (ng < 1e-8)]).shape[0] >= 2                             # unnormalised Ng: at least two primitives
    has_tb = np.array([("N" in m and "T" in m and "B" in m) for m in meshes])[np.searchsorted(
        np.cumsum([m["idx"].shape[0] // 3 for m in meshes]), prim[hit], side="right")]
    ax = ortho_axis(state[hit, 3:6][~has_tb])
    assert set(np.unique(ax)) == {0, 1, 2}, np.bincount(ax)                             # each choice of the ortho basis
    assert (state[hit, 3:6] == 0.6).any() and (np.abs(state[hit, 3:6]) == 0.8).any()    # a component exactly on the threshold
    for name in ("E5", "E6"):
        ins = state[hit, 23][fam[prim[hit]] == FAMILIES.index(name)]
        assert (ins == 0.0).any() and (ins == 1.0).any(), name
    first5 = int(np.cumsum([0] + [m["idx"].shape[0] // 3 for m in meshes])[FAMILIES.index("E5")])
    for k, want in enumerate((0.0, 0.0, 0.0, 1.0, 1.0)):                                # a rule on triangle counts would say 0 0 1 1 1
        got = state[hit & (prim == first5 + k), 23]
        assert got.shape[0] > 0 and (got == want).all(), (k, got)
    return per_family
