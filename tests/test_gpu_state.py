"""GPU: the device-side hit epilogue (lh_accel_state_build_*: P, Ng, Ns, tangent, binormal, colour, st, I, inside from
SoA per-primitive attributes) against the compiled reference's records and the oracle, bit for bit; and the host
mirror of lucille's plugin API carrying the same attributes (ri_geom_add_colors ... -> ri_raytrace -> state).
Then the edge scene of tests/state_edges.py -- the branches the first scene cannot reach -- through both entry points, from every scene
source, and through the other copies of the epilogue: ao_hit_epilogue, state_core<false>, pt_scatter, the host mirror."""
import ctypes as C

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
from tests import state_edges as se
from tests.golden.make_golden import apply_state_scene, state_scene
from tests.helpers import load_golden
from tests.test_gpu_ao_batch import ao, ao_rays, dev, host
from tests.test_gpu_ao_batch import expected as ao_expected
from tests.test_gpu_device_attr import DeviceScene, dev_f32, dev_pos, dev_strided, device_accel, host_accel, oracle_of
from tests.test_gpu_dirt import dirt, oracle_t
from tests.test_gpu_dirt import scatter as dirt_scatter
from tests.test_gpu_dirt import values as dirt_values
from tests.test_gpu_pt_oracle import close as pt_close
from tests.test_gpu_pt_oracle import mat10

pytestmark = pytest.mark.gpu


class _Prod:
    """adapter: the fixture's scene description onto a HipAccel"""

    def __init__(self):
        self.acc = la.HipAccel(0)

    def add_mesh(self, P, idx):
        self.acc.add_mesh(P, idx)

    def set_normals(self, k, N, two_side):
        self.acc.set_normals(k, N, two_side)

    def set_attribute(self, k, kind, data):
        self.acc.set_attribute(k, kind, data)


def test_device_state_records_equal_the_reference():
    g = load_golden("state_attr")
    meshes, org, dr = state_scene(int(g["seed"]))
    p = _Prod(); apply_state_scene(p, meshes, False); p.acc.commit()
    prim, t, u, v = p.acc.intersect_host(org, dr)
    assert np.array_equal(prim, g["prim"])
    st = p.acc.state_build(org, dr, prim, t, u, v)
    assert np.array_equal(st, g["state"])
    # a second seed against the oracle (no fixture): same arithmetic on other data
    meshes, org, dr = state_scene(5)
    p2 = _Prod(); apply_state_scene(p2, meshes, False); p2.acc.commit()
    o = po.Oracle(); apply_state_scene(o, meshes, False); o.build()
    prim, t, u, v = p2.acc.intersect_host(org, dr)
    op, ost = o.state_batch(org, dr)
    assert np.array_equal(prim, op) and np.array_equal(p2.acc.state_build(org, dr, prim, t, u, v), ost)
    with pytest.raises(la.LucilleHipError, match="needs"):
        bad = la.HipAccel(0); bad.add_mesh(meshes[0]["P"], meshes[0]["idx"]); bad.set_attribute(0, la.ATTR_COLOR, np.zeros((3, 3)))
    p.acc.close(); p2.acc.close()


def host_mirror_states(meshes, org, dr, exp_p, exp, n):
    """include/lucille_accel.h: ri_geom_add_colors / _tangents / _binormals / _texcoords(_unshared) ->
    ri_scene_build_accel(RI_ACCEL_HIP) -> ri_raytrace for the first n rays: the ri_intersection_state_t the caller gets == exp"""
    L = binding.lib()
    vec4 = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros((a.shape[0], 1))], 1))

    class Geom(C.Structure):
        _fields_ = [("positions", C.c_void_p), ("npositions", C.c_uint), ("normals", C.c_void_p), ("nnormals", C.c_uint),
                    ("indices", C.c_void_p), ("nindices", C.c_uint), ("two_side", C.c_int),
                    ("tangents", C.c_void_p), ("ntangents", C.c_uint), ("binormals", C.c_void_p), ("nbinormals", C.c_uint),
                    ("colors", C.c_void_p), ("ncolors", C.c_uint), ("texcoords", C.c_void_p), ("texcoords_unshared", C.c_void_p),
                    ("ntexcoords", C.c_uint)]

    class State(C.Structure):
        _fields_ = [("P", C.c_double * 4), ("Ng", C.c_double * 4), ("Ns", C.c_double * 4), ("E", C.c_double * 4), ("I", C.c_double * 4),
                    ("t", C.c_double), ("inside", C.c_char), ("geom", C.c_void_p), ("index", C.c_uint32),
                    ("color", C.c_double * 4), ("tangent", C.c_double * 4), ("binormal", C.c_double * 4), ("stqr", C.c_double * 4),
                    ("u", C.c_double), ("v", C.c_double)]

    class Ray(C.Structure):
        _fields_ = [("org", C.c_double * 4), ("dir", C.c_double * 4), ("t", C.c_float), ("dir_sign", C.c_int * 3),
                    ("invdir", C.c_double * 4), ("thread_num", C.c_int)]

    L.ri_geom_new.restype = C.POINTER(Geom)
    L.ri_scene_new.restype = C.c_void_p
    L.ri_render_get.restype = C.c_void_p
    for f in ("ri_geom_add_positions", "ri_geom_add_normals", "ri_geom_add_tangents", "ri_geom_add_binormals", "ri_geom_add_colors"):
        getattr(L, f).argtypes = [C.POINTER(Geom), C.c_uint, C.c_void_p]
    L.ri_geom_add_texcoords.argtypes = [C.POINTER(Geom), C.c_uint, C.c_void_p]
    L.ri_geom_add_texcoords_unshared.argtypes = [C.POINTER(Geom), C.c_uint, C.c_void_p]
    L.ri_geom_add_indices.argtypes = [C.POINTER(Geom), C.c_uint, C.c_void_p]
    L.ri_scene_add_geom.argtypes = [C.c_void_p, C.POINTER(Geom)]
    L.ri_scene_build_accel.argtypes = [C.c_void_p]
    L.ri_accel_bind.argtypes = [C.c_void_p, C.c_int]
    L.ri_raytrace.argtypes = [C.c_void_p, C.POINTER(Ray), C.POINTER(State)]
    L.ri_render_init()

    class Render(C.Structure):
        _fields_ = [("scene", C.c_void_p)]
    class Scene(C.Structure):
        _fields_ = [("geom_list", C.c_void_p), ("ngeoms", C.c_uint), ("accel", C.c_void_p)]
    render = C.cast(L.ri_render_get(), C.POINTER(Render))
    scene = render.contents.scene
    keep = []
    for m in meshes:
        gm = L.ri_geom_new()
        P4 = vec4(m["P"]); keep.append(P4)
        L.ri_geom_add_positions(gm, P4.shape[0], P4.ctypes.data)
        idx = np.ascontiguousarray(m["idx"], np.uint32); keep.append(idx)
        L.ri_geom_add_indices(gm, idx.shape[0], idx.ctypes.data)
        for key, fn in (("N", L.ri_geom_add_normals), ("T", L.ri_geom_add_tangents), ("B", L.ri_geom_add_binormals), ("C", L.ri_geom_add_colors)):
            if key in m:
                a = vec4(m[key]); keep.append(a); fn(gm, a.shape[0], a.ctypes.data)
        if "ST" in m:
            a = np.ascontiguousarray(m["ST"]); keep.append(a); L.ri_geom_add_texcoords(gm, a.shape[0], a.ctypes.data)
        if "STU" in m:
            a = np.ascontiguousarray(m["STU"]); keep.append(a); L.ri_geom_add_texcoords_unshared(gm, a.shape[0], a.ctypes.data)
        gm.contents.two_side = m["two_side"]
        L.ri_scene_add_geom(scene, gm)
    sc = C.cast(scene, C.POINTER(Scene))
    assert L.ri_accel_bind(sc.contents.accel, 2) == 0 and L.ri_scene_build_accel(scene) == 0
    for i in range(n):
        ray = Ray(); st = State()
        for k in range(3):
            ray.org[k] = org[i, k]; ray.dir[k] = dr[i, k]
        hit = L.ri_raytrace(render, C.byref(ray), C.byref(st))
        assert bool(hit) == (exp_p[i] != po.MISS)
        if hit:
            got = np.concatenate([st.P[:3], st.Ng[:3], st.Ns[:3], st.tangent[:3], st.binormal[:3], st.color[:3], st.stqr[:2], st.I[:3],
                                  [float(ord(st.inside))]])
            assert np.array_equal(got, exp[i]), (i, got, exp[i])
    L.ri_render_free()


def test_host_mirror_state_carries_the_attributes():
    g = load_golden("state_attr")
    meshes, org, dr = state_scene(int(g["seed"]))
    host_mirror_states(meshes, org, dr, g["prim"], g["state"], 600)


# =====================================================================================================================================
# The edge scene (tests/state_edges.py): every branch of the epilogue, both entry points, every scene source, every copy of the epilogue.
# Expected values are the compiled reference's (tests/golden/state_edges.npz) and the oracle's, never the product's.
# =====================================================================================================================================
FILL = 0xA5                                            # the byte the device entry's outputs are prefilled with: no record holds it
FILL64 = np.uint64(0xA5A5A5A5A5A5A5A5)
TAIL = 3                                               # guard records behind the n the call is given
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


def dv(a):
    """a copy of a host array (the fixtures' arrays are read-only) on the device; uint32 as int32 bits"""
    return dev(np.array(a))


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bytes(a, b):
    """bytes, not values: a NaN or a -0.0 cannot hide a difference"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def device_states(acc, org, dr, prim, t, u, v, stream=None):
    """lh_accel_state_build_device on the first n records into an output of n + TAIL records prefilled with FILL -> the whole output's
    words [n + TAIL, 24] uint64, after the stream has been waited for"""
    import torch
    n = org.shape[0]
    raw = torch.full(((n + TAIL) * 24 * 8,), FILL, dtype=torch.uint8, device="cuda")
    big = raw.view(torch.float64).view(n + TAIL, 24)
    args = [dv(org), dv(dr), dv(np.ascontiguousarray(prim, np.uint32)), dv(t), dv(u), dv(v)]
    torch.cuda.synchronize()
    out = acc.state_build_device(*args, out=big[:n], stream=stream)
    assert out.data_ptr() == big.data_ptr()
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    return raw.cpu().numpy().view(np.uint64).reshape(n + TAIL, 24)


def expected_words(prim, state):
    """what device_states leaves: the record of a hit, FILL in a miss's record and in the tail"""
    n = prim.shape[0]
    w = np.full((n + TAIL, 24), FILL64, np.uint64)
    hit = prim != po.MISS
    w[:n][hit] = u64(state)[hit]
    return w


def assert_states(acc, org, dr, rec, state, what):
    """both entry points on the records rec = (prim, t, u, v): the host form gives `state` (zeros for a miss), the device form writes the hits alone"""
    prim = rec[0]
    got = acc.state_build(org, dr, *rec)
    bad = np.nonzero((u64(got) != u64(state)).any(axis=1))[0]
    assert bad.size == 0, (what, "host entry", bad[:8], got[bad[:1]], state[bad[:1]])
    assert not got[prim == po.MISS].any()
    w = device_states(acc, org, dr, *rec)
    x = expected_words(prim, state)
    bad = np.nonzero((w != x).any(axis=1))[0]
    assert bad.size == 0, (what, "device entry", bad[:8])


@pytest.fixture(scope="module")
def edge():
    """the edge scene of the golden's seed: the oracle over it, the reference's records of its rays (== the oracle's, checked), the
    caller-made records and the oracle's states for them; computed once, read-only"""
    g = load_golden("state_edges")
    seed = int(g["seed"])
    meshes, org, dr = se.edge_scene(seed)
    o = oracle_of(meshes)
    prim, st = o.state_batch(org, dr)
    assert np.array_equal(prim, g["prim"]) and same_bytes(st, g["state"])
    se.assert_coverage(meshes, g["prim"], g["state"])
    rec = o.intersect(org, dr)
    assert np.array_equal(rec[0], prim)
    r = se.edge_records(meshes, seed)
    rst = o.state_records(*r)
    assert not rst[r[2] == po.MISS].any() and (r[2] != po.MISS).sum() > 1500
    for a in (org, dr, prim, st, rst) + tuple(rec) + tuple(r):
        a.setflags(write=False)
    return {"meshes": meshes, "org": org, "dr": dr, "oracle": o, "rec": rec, "state": st, "r": r, "rstate": rst, "seed": seed}


@pytest.fixture(scope="module")
def edge_acc(edge):
    """host arrays through the host builders"""
    p = _Prod(); apply_state_scene(p, edge["meshes"], False); p.acc.commit(); p.acc.wait_exact()
    yield p.acc
    p.acc.close()


def assert_edge_scene(acc, edge, what, oracle=None):
    """an accelerator over the edge scene: its closest hits are the oracle's, bit for bit, and both entry points give the expected
    records for the rays' hits and for the caller-made records.  oracle: one fed other attribute values (fp32 sources)"""
    org, dr, r = edge["org"], edge["dr"], edge["r"]
    st, rst = edge["state"], edge["rstate"]
    if oracle is not None:
        st = oracle.state_batch(org, dr)[1]; rst = oracle.state_records(*r)
    got = acc.intersect_host(org, dr)
    for k, name in enumerate(("prim", "t", "u", "v")):
        assert same_bytes(got[k], edge["rec"][k]), (what, name, int((got[k] != edge["rec"][k]).sum()))
    assert_states(acc, org, dr, got, st, what + ": rays")
    assert_states(acc, r[0], r[1], r[2:], rst, what + ": records")


# ---- 1. k_state_build through both entry points, host builders ---------------------------------------------------------------------
def test_edge_scene_through_both_entry_points(edge, edge_acc):
    assert_edge_scene(edge_acc, edge, "host arrays")
    hit = edge["rec"][0] != po.MISS
    print("edge scene: %d rays, %d hits; %d records, %d of them misses" % (hit.size, int(hit.sum()), edge["r"][2].size, int((edge["r"][2] == po.MISS).sum())))


# ---- 2. the device entry point's own contract -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_device_entry_writes_the_hits_of_its_n_records_alone(edge, edge_acc, n):
    """n around the 256-thread block and the 64-lane wave: a miss's record and the TAIL records behind n keep their bytes"""
    import torch
    r = tuple(a[:n] for a in edge["r"])
    assert n == 1 or (r[2] == po.MISS).any()
    stream = torch.cuda.Stream() if n == 257 else None          # once on a stream that is not the default
    w = device_states(edge_acc, *r, stream=stream)
    x = expected_words(r[2], edge["rstate"][:n])
    assert np.array_equal(w[n:], x[n:]), "the call wrote behind its n records"
    assert np.array_equal(w, x), np.nonzero((w != x).any(axis=1))[0][:8]
    if n == 1:
        miss = tuple(a[6:7] for a in edge["r"])                 # a batch of one miss: nothing is written
        assert miss[2][0] == po.MISS and (device_states(edge_acc, *miss) == FILL64).all()


def test_device_entry_on_nothing_and_on_the_empty_scene(edge, edge_acc):
    import torch
    r = edge["r"]
    raw = torch.full((TAIL * 24 * 8,), FILL, dtype=torch.uint8, device="cuda")
    big = raw.view(torch.float64).view(TAIL, 24)
    none = [dv(a[:0]) for a in r]
    out = edge_acc.state_build_device(*none, out=big[:0]); torch.cuda.synchronize()
    assert tuple(out.shape) == (0, 24) and (raw.cpu().numpy() == FILL).all()
    assert binding.lib().lh_accel_state_build_device(edge_acc.h, 0, None, None, None, None, None, None, None, None) == 0
    empty = la.HipAccel(0); empty.commit()
    try:
        n = 300
        w = device_states(empty, *(a[:n] for a in r))
        assert (w == FILL64).all()                                        # no primitive: every record is a miss, nothing is written
        args = [dv(a[:n]) for a in r]
        assert binding.lib().lh_accel_state_build_device(empty.h, n, *[binding._dptr(a) for a in args], binding._dptr(big), None) == 0
        torch.cuda.synchronize()
        assert (raw.cpu().numpy() == FILL).all()
        assert not empty.state_build(*(a[:n] for a in r)).any()          # the host entry: zeros
    finally:
        empty.close()
    with pytest.raises(ValueError):
        edge_acc.state_build_device(*[dv(a[:5]) for a in r], out=big)     # an output of another length


# ---- 3. scene sources: the same expected bytes ------------------------------------------------------------------------------------------
def f32_values(meshes):
    """the meshes with every attribute rounded to float32 and widened again: what a float32 source holds"""
    return [dict(m, **{k: m[k].astype(np.float32).astype(np.float64) for k in ("N", "C", "T", "B", "ST", "STU") if k in m}) for m in meshes]


@pytest.mark.parametrize("source", ["host_on_device", "device_f64", "device_strided", "device_f32"])
def test_edge_scene_from_every_scene_source(edge, source):
    meshes = edge["meshes"]
    oracle = None
    if source == "host_on_device":
        acc, _ = host_accel(meshes)                     # commit(on_device=True), then wait_exact()
    else:
        acc, _ = device_accel(meshes, {"device_f64": dev_pos, "device_strided": dev_strided, "device_f32": dev_f32}[source])
        if source == "device_f32":
            wide = f32_values(meshes)
            assert not np.array_equal(wide[2]["N"], meshes[2]["N"])
            oracle = oracle_of(wide)
    try:
        assert acc.info()["ntriangles"] == se.triangles(meshes).shape[0]
        assert_edge_scene(acc, edge, source, oracle)
    finally:
        acc.close()


def test_edge_scene_after_a_recommit_of_normals_and_coordinates(edge):
    """an updatable accelerator committed with E3's normals and E4's texture coordinates wrong (the arrays reversed), then given the
    right ones and re-committed: the gather runs again, no tree is built, and the records are the expected ones"""
    meshes = edge["meshes"]
    k3, k4 = se.FAMILIES.index("E3"), se.FAMILIES.index("E4")
    wrong = [dict(m) for m in meshes]
    wrong[k3]["N"] = np.ascontiguousarray(meshes[k3]["N"][::-1]); wrong[k4]["ST"] = np.ascontiguousarray(meshes[k4]["ST"][::-1])
    wrong[k4]["STU"] = np.ascontiguousarray(meshes[k4]["STU"][::-1])
    s = DeviceScene(); s.acc.set_param("updatable", 1); apply_state_scene(s, wrong, False)
    acc = s.acc
    try:
        acc.commit()
        org, dr = edge["org"], edge["dr"]
        before = acc.state_build(org, dr, *edge["rec"])
        assert same_bytes(before, oracle_of(wrong).state_batch(org, dr)[1]) and not same_bytes(before, edge["state"])
        acc.set_normals_device(k3, dev_pos(meshes[k3]["N"]), 0)
        acc.set_attribute_device(k4, la.ATTR_TEXCOORD, dev_pos(meshes[k4]["ST"]))
        acc.set_attribute_device(k4, la.ATTR_TEXCOORD_UNSHARED, dev_pos(meshes[k4]["STU"]))
        assert same_bytes(acc.state_build(org, dr, *edge["rec"]), before)          # staged only
        r = acc.recommit()
        assert (r["flattened"], r["rebuilt_trees"], r["regathered"]) == (0, 0, 1)
        assert_edge_scene(acc, edge, "recommit")
    finally:
        acc.close()


def one_mesh_per_triangle(meshes):
    """every triangle a mesh of its own (three vertices, its corners' attribute values), and in the middle an empty mesh and a mesh with
    no attribute at all, far away: more than 60 meshes inside one 256-corner workgroup of k_gather_attributes"""
    out = []
    for m in meshes:
        idx = m["idx"].astype(np.int64)
        for k in range(idx.shape[0] // 3):
            c = idx[3 * k:3 * k + 3]
            t = {"family": m["family"], "P": np.ascontiguousarray(m["P"][c]), "idx": np.arange(3, dtype=np.uint32), "two_side": m["two_side"]}
            for key in ("N", "C", "T", "B", "ST"):
                if key in m:
                    t[key] = np.ascontiguousarray(m[key][c])
            if "STU" in m:
                t["STU"] = np.ascontiguousarray(m["STU"][3 * k:3 * k + 3])
            out.append(t)
    mid = len(out) // 2
    bare = {"family": "bare", "P": np.array([[100.0, 100.0, 100.0], [101.0, 100.0, 100.0], [100.0, 101.0, 100.0]]), "idx": np.arange(3, dtype=np.uint32), "two_side": 0}
    none = {"family": "empty", "P": np.zeros((0, 3)), "idx": np.zeros(0, np.uint32), "two_side": 0}
    return out[:mid] + [none, bare] + out[mid:]


def test_one_mesh_per_triangle_inside_one_gather_workgroup(edge):
    """k_gather_attributes (lh_flatten.hip) finds a corner's mesh between the meshes of its workgroup's first and last corner: here that
    search runs over 72 meshes with alternating attributes.  tests/test_gpu_device_attr.py's boundary_scene has five"""
    split = one_mesh_per_triangle(edge["meshes"])
    ntri = se.triangles(edge["meshes"]).shape[0] + 1
    assert len(split) == ntri + 1 > 60 and 3 * ntri <= 256
    o = oracle_of(split)
    org = np.concatenate([edge["org"], np.array([[100.2, 100.2, 101.0], [100.2, 100.2, 99.0]])])
    dr = np.concatenate([edge["dr"], np.array([[0.01, 0.02, -1.5], [0.0, 0.01, 0.7]])])
    prim, st = o.state_batch(org, dr)
    rec = o.intersect(org, dr)
    mid = (ntri - 1) // 2
    e = edge["rec"][0]                                                    # the primitives behind the two meshes in the middle move up by one
    assert (prim != po.MISS).all() and (prim[-2:] == mid).all() and np.array_equal(prim[:-2], np.where(e < mid, e, e + 1))
    # a mesh of one triangle has index 0 < nindices / 2: no primitive is inside, whatever two_side says
    assert not st[:, 23].any() and edge["state"][:, 23].any()
    keep = np.r_[0:23]
    assert same_bytes(st[:-2][:, keep], edge["state"][:, keep])           # everything else is the edge scene's
    for name, make in (("device meshes", device_accel), ("host arrays, built on the device", host_accel)):
        acc, info = make(split)
        try:
            assert info["ntriangles"] == ntri
            got = acc.intersect_host(org, dr)
            for k in range(4):
                assert same_bytes(got[k], rec[k]), (name, k)
            assert_states(acc, org, dr, got, st, name)
        finally:
            acc.close()


# ---- 4. the other copies of the epilogue, on the same hits -------------------------------------------------------------------------------
def ao_restated(o, st, hit_ids, uni, ntheta, nphi):
    """calculate_occlusion's rays (oracle/lucille_oracle_ao.c lo_ao_rays: origin P + 1e-6 Ns, ri_ortho_basis(Ns) with the 1e-17f rule, the
    replay arithmetic) of the hits, from the ORACLE's P and Ns and the caller's uniforms"""
    N = ntheta * nphi
    aorg = np.empty((hit_ids.size * N, 3)); adir = np.empty((hit_ids.size * N, 3))
    for s, i in enumerate(hit_ids):
        P = np.ascontiguousarray(st[i, 0:3]); Ns = np.ascontiguousarray(st[i, 6:9]); rnd = np.ascontiguousarray(uni[2 * N * s:2 * N * (s + 1)])
        po.lib().lo_ao_rays(P.ctypes.data_as(po._dp), Ns.ctypes.data_as(po._dp), ntheta, nphi, rnd.ctypes.data_as(po._dp),
                            aorg[N * s:].ctypes.data_as(po._dp), adir[N * s:].ctypes.data_as(po._dp))
    return aorg, adir


def ortho_basis_np(n):
    """ri_ortho_basis (reflection.c:311-333) with ri_vector_normalize's 1e-17f rule, one IEEE operation at a time: (b0, b1)"""
    thr = float(np.float32(1.0e-17))

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    def normalize(a):
        n2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        big = n2 > thr
        r = 1.0 / np.sqrt(np.where(big, n2, 1.0))
        return np.where(big[:, None], a * r[:, None], a)
    b1 = np.zeros_like(n); b1[np.arange(n.shape[0]), se.ortho_axis(n)] = 1.0
    b0 = normalize(cross(b1, n))
    return b0, normalize(cross(n, b0))


@pytest.fixture(scope="module")
def edge_dev(edge, edge_acc):
    """the edge scene's rays and their closest-hit records on the device (the records are the oracle's, checked)"""
    import torch
    to, td = dv(edge["org"]), dv(edge["dr"])
    rec = edge_acc.intersect_device(to, td); torch.cuda.synchronize()
    for k in range(4):
        assert same_bytes(host(rec[k], np.uint32 if k == 0 else None), edge["rec"][k])
    return {"org": to, "dr": td, "rec": rec}


def test_ao_epilogue_on_the_edge_hits(edge, edge_acc, edge_dev):
    """ao_hit_epilogue (lh_render.hip), where the self-primitive skip meets an unnormalised Ng: the AO rays of the edge scene's hits from
    replayed uniforms, and the occluded counts of the fused and the materialised stage.
    (a) one ray per hit with xi' = 0: phi = 0, so sin and cos are 0 and 1 on any machine and the ray is cos(theta) b0 + sqrt(1 - cos^2) Ns from
        P + 1e-6 Ns -- origins and directions equal the restatement bit for bit;
    (b) 16 rays per hit with seeded uniforms: origins bit for bit; a direction is d0 b0 + d1 b1 + d2 Ns with d0, d1 from the device's sincos,
        which is within 2 ulps where libm is within 1: every component is within 8 * 2^-52 * (|d0 b0| + |d1 b1| + |d2 Ns|) of the restatement's
        (3 ulps of the factors, 3 roundings of products, 2 of sums);
    (c) the counts are the oracle's any-hit over the device's own rays of (b)"""
    o, st, acc = edge["oracle"], edge["state"], edge_acc
    org, dr, rec = edge_dev["org"], edge_dev["dr"], edge_dev["rec"]
    prim = edge["rec"][0]
    ids = np.nonzero(prim != po.MISS)[0]
    rng = np.random.default_rng(91)
    # (a)
    uni = np.stack([rng.uniform(0.0, 1.0, ids.size), np.zeros(ids.size)], 1).reshape(-1).copy()
    slot, nslots, aorg, adir = ao_rays(acc, org, dr, rec, 1, uniforms=dv(uni))
    assert nslots == ids.size and np.array_equal(slot[ids], np.arange(ids.size, dtype=np.uint32))
    xo, xd = ao_restated(o, st, ids, uni, 1, 1)
    b0, b1 = ortho_basis_np(st[ids, 6:9])
    ct = np.sqrt(uni[0::2]); d2 = np.sqrt(1.0 - ct * ct)
    mine = (ct[:, None] * b0 + 0.0 * b1) + d2[:, None] * st[ids, 6:9]
    assert same_bytes(mine, xd) and same_bytes(st[ids, 0:3] + st[ids, 6:9] * 1.0e-6, xo)          # the two restatements agree
    print("AO, one ray per hit: origins differ at %d, directions at %d of %d" % (int((u64(aorg) != u64(xo)).any(axis=1).sum()),
                                                                                int((u64(adir) != u64(xd)).any(axis=1).sum()), ids.size))
    assert same_bytes(aorg, xo) and same_bytes(adir, xd)
    tiny = np.linalg.norm(st[ids, 3:6], axis=1) < 1e-8
    assert tiny.sum() >= 16 and (np.linalg.norm(adir[tiny], axis=1) < 1e-8).all()                  # the basis of an unnormalised Ng is not normalised
    # (b), (c)
    NS = N = 16
    uni = rng.uniform(0.0, 1.0, 2 * N * ids.size)
    slot, nslots, aorg, adir = ao_rays(acc, org, dr, rec, NS, uniforms=dv(uni))
    xo, xd = ao_restated(o, st, ids, uni, 4, 4)
    assert same_bytes(aorg, xo)
    z0 = (np.tile(np.arange(4), 4 * ids.size) + uni[0::2]) / 4.0; z1 = (np.tile(np.repeat(np.arange(4), 4), ids.size) + uni[1::2]) / 4.0
    ct = np.sqrt(z0); phi = 2.0 * np.pi * z1
    mag = (np.abs((np.cos(phi) * ct)[:, None] * np.repeat(b0, N, 0)) + np.abs((np.sin(phi) * ct)[:, None] * np.repeat(b1, N, 0))
           + np.abs(np.sqrt(1.0 - ct * ct)[:, None] * np.repeat(st[ids, 6:9], N, 0)))
    err = np.abs(adir - xd)
    print("AO, 16 rays per hit: directions differ in bits at %d of %d rays, largest error / bound %.3g" % (
        int((u64(adir) != u64(xd)).any(axis=1).sum()), adir.shape[0], float((err / np.maximum(8 * 2.0 ** -52 * mag, 1e-300)).max())))
    assert (err <= 8 * 2.0 ** -52 * mag).all()
    occ = o.intersect(aorg, adir, nthreads=8)[0] != po.MISS
    ecnt, erad = ao_expected(slot, occ, N)
    print("AO: %d of %d rays occluded; of the tiny triangles' %d" % (int(occ.sum()), occ.size, int(occ.reshape(-1, N)[tiny].sum())))
    for fused in (1, 0):
        cnt, rad = ao(acc, org, dr, rec, NS, fused, uniforms=dv(uni))
        assert np.array_equal(cnt, ecnt), (fused, np.nonzero(cnt != ecnt)[0][:8], cnt[cnt != ecnt][:8], ecnt[cnt != ecnt][:8])
        assert same_bytes(rad, erad), fused
    # the dirt stage: the same epilogue with eps = 1e-5 (below it the self-primitive skip is off: lh_dirt.h)
    for eps in (1e-5, 1e-6):
        go = np.repeat(st[ids, 0:3] + st[ids, 6:9] * eps, N, axis=0)
        t, hit = oracle_t(o, go, adir)
        near, far = 0.05, 0.6
        nh, val = dirt_values(t, hit, N, near, far)
        ecnt, eval_ = dirt_scatter(slot, nh, val)
        for fused in (1, 0):
            cnt, v = dirt(acc, org, dr, rec, NS, la.DirtParams(near, far, eps), fused, uniforms=dv(uni))
            assert np.array_equal(cnt, ecnt), (eps, fused, np.nonzero(cnt != ecnt)[0][:8])
            assert same_bytes(v, eval_), (eps, fused)
        print("dirt, eps %g: %d gather rays hit something, %d below the far clip" % (eps, int(hit.sum()), int(nh.sum())))


def test_whitted_bounce_on_the_edge_hits(edge, edge_acc, edge_dev):
    """state_core<false> (lh_shade.h) through k_whitted_bounce: one bounce from every hit of the edge scene == the rule of
    tests/whitted_chain.py fed with the oracle's P, Ns and I -- E3's scaled and zero normals are taken as they are, a flat hit's Ng is
    computed there and only there"""
    import torch
    from tests import whitted_chain as wc
    st, prim = edge["state"], edge["rec"][0]
    hit = prim != po.MISS
    n = prim.shape[0]
    fam = se.family_of_prim(edge["meshes"])[prim[hit]]
    ns = np.linalg.norm(st[hit, 6:9], axis=1)[fam == se.FAMILIES.index("E3")]
    assert (ns == 0.0).sum() >= 8 and (ns > 5.0).any() and ((ns > 0.0) & (ns < 0.1)).any()
    for eta in (1.33, 0.75):
        p = la.WhittedParams(1e-7, eta, 8)
        eo, ed, tir = wc.bounce_np(st[hit, 0:3], st[hit, 6:9], st[hit, 20:23], p.eps, p.eta)
        xo = np.full((n, 3), -7.5); xd = np.full((n, 3), -7.5); xo[hit] = eo; xd[hit] = ed
        out = (torch.full((n, 3), -7.5, dtype=torch.float64, device="cuda"), torch.full((n, 3), -7.5, dtype=torch.float64, device="cuda"))
        out = edge_acc.whitted_rays_device(edge_dev["org"], edge_dev["dr"], edge_dev["rec"], p, out=out); torch.cuda.synchronize()
        bad = np.nonzero((u64(host(out[0])) != u64(xo)).any(axis=1) | (u64(host(out[1])) != u64(xd)).any(axis=1))[0]
        assert bad.size == 0, (eta, bad[:8], se.family_of_prim(edge["meshes"])[prim[bad[:8]]])


def pt_camera(w, h, flength, eye):
    """la.Camera and the oracle's: cam2world the identity with `eye` in its last row"""
    m = np.eye(4); m[3, :3] = eye
    oc = po.Camera(); oc.width, oc.height, oc.rh, oc.ortho, oc.flength = w, h, 1, 0, flength
    for i in range(16):
        oc.cam2world[i] = float(m.reshape(16)[i])
    return la.Camera.make(w, h, flength, m, 1), oc


def assert_pt_frame(meshes, cam, ocam, w, h, spp, mats, seed, min_colour_pixels):
    """render_pt_tile2 == Oracle.render_pt: paths, rays and the longest path equal, the frame within tests/test_gpu_pt_oracle.py's tolerance;
    and on the ORACLE's frames the colour attribute matters in at least min_colour_pixels pixels"""
    o = oracle_of(meshes)
    exp, est, _ = o.render_pt(ocam, 0, 0, w, h, 0, spp, spp, max_vertices=8, materials=[mat10(m) for m in mats], seed=seed)
    plain, pst, _ = oracle_of([{k: v for k, v in m.items() if k != "C"} for m in meshes]).render_pt(
        ocam, 0, 0, w, h, 0, spp, spp, max_vertices=8, materials=[mat10(m) for m in mats], seed=seed)
    assert pst == est and int((exp != plain).any(axis=2).sum()) >= min_colour_pixels
    for name, make in (("host arrays", host_accel), ("device meshes", device_accel)):
        acc, _ = make(meshes)
        try:
            for k, m in enumerate(mats):
                acc.set_material(k, m)
            img, st = acc.render_pt_tile2(cam, 0, 0, w, h, 0, spp, spp, max_vertices=8, seed=seed)
            got = img.cpu().numpy()
            print("%s: %s, largest difference %.3g" % (name, st, float(np.abs(got - exp).max())))
            assert st == est, (name, st, est)
            ok = pt_close(got, exp)
            assert ok.all(), (name, float(np.abs(got - exp).max()), int((~ok).sum()))
        finally:
            acc.close()
    return est


def test_path_tracer_reads_the_vertex_colours():
    """pt_scatter (lh_pt.h) interpolates vertex colours from col9: state_scene(5) -- meshes 0 (two_side, normals) and 2 carry colours -- and
    a frame on the edge scene's E6 (two_side, 7 triangles, normals and colours) and E3 (scaled and zero normals) against the oracle's
    path tracer"""
    meshes, _, _ = state_scene(5)
    mats = [la.Material.make(kd=(0.7, 0.6, 0.5)), la.Material.make(kd=(0.3,) * 3, ks=(0.3,) * 3, kt=(0.3,) * 3, ior=1.5), la.Material.make(kd=(0.5, 0.6, 0.7))]
    cam, ocam = pt_camera(32, 32, 2.0, (0.1, 0.0, 3.0))
    est = assert_pt_frame(meshes, cam, ocam, 32, 32, 8, mats, 1, 50)
    assert est["rays"] > est["paths"] + 2000 and est["max_depth_reached"] >= 6
    emeshes, _, _ = se.edge_scene(7)
    mats = [la.Material.make(kd=(0.8, 0.7, 0.6)) for _ in emeshes]
    mats[se.FAMILIES.index("E3")] = la.Material.make(kd=(0.4,) * 3, ks=(0.2,) * 3, kt=(0.3,) * 3, ior=1.5)
    cam, ocam = pt_camera(16, 16, 2.0, (1.35, -59.85, 0.6))
    assert_pt_frame(emeshes, cam, ocam, 16, 16, 4, mats, 3, 50)
    cam, ocam = pt_camera(16, 16, 2.0, (1.2, -29.85, 0.6))
    assert_pt_frame(emeshes, cam, ocam, 16, 16, 4, mats, 3, 0)


def test_host_mirror_state_on_the_edge_scene(edge):
    g = load_golden("state_edges")
    host_mirror_states(edge["meshes"], edge["org"], edge["dr"], g["prim"], g["state"], edge["org"].shape[0])
