"""The whole hit epilogue -- ri_intersection_state_build with colours, tangents / binormals, shared and
unshared texture coordinates, two-sided meshes (intersection_state.c:99-248) -- oracle restatement against the
compiled reference's records (tests/golden/state_attr.npz, made by tests/golden/make_golden.py --state) and,
where the reference can be built, against the live reference; the same for the edge scene of tests/state_edges.py
(tests/golden/state_edges.npz, --state-edges), and the record-driven entry Oracle.state_records.  CPU only."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import state_edges as se
from tests.golden.make_golden import apply_state_scene, state_scene
from tests.helpers import load_golden


def test_oracle_state_records_equal_the_reference_goldens():
    g = load_golden("state_attr")
    meshes, org, dr = state_scene(int(g["seed"]))
    o = po.Oracle(); apply_state_scene(o, meshes, False); o.build()
    prim, st = o.state_batch(org, dr)
    assert np.array_equal(prim, g["prim"])
    assert np.array_equal(st, g["state"])                    # all 24 doubles of every ray, bit for bit
    hit = prim != po.MISS
    assert hit.sum() > 3000 and st[hit, 23].sum() > 100      # two-sided back faces are exercised
    assert (st[hit, 15:18] != 1.0).any() and (st[hit, 18:20] != 0.0).any()


@pytest.mark.skipif(not po.ref_available(), reason="the compiled reference is not available here")
def test_oracle_state_records_equal_the_live_reference():
    meshes, org, dr = state_scene(77)
    ref = po.RefLib(); apply_state_scene(ref, meshes, True); ref.build()
    o = po.Oracle(); apply_state_scene(o, meshes, False); o.build()
    rp, rs = ref.state_batch(org, dr); op, os_ = o.state_batch(org, dr)
    assert np.array_equal(rp, op) and np.array_equal(rs, os_)


# ---- the edge scene (tests/state_edges.py): branches state_scene cannot reach ------------------------------------------------
def _edge_oracle(seed):
    meshes, org, dr = se.edge_scene(seed)
    o = po.Oracle(); apply_state_scene(o, meshes, False); o.build()
    return meshes, org, dr, o


def test_oracle_edge_records_equal_the_reference_goldens():
    g = load_golden("state_edges")
    meshes, org, dr, o = _edge_oracle(int(g["seed"]))
    prim, st = o.state_batch(org, dr)
    assert np.array_equal(prim, g["prim"]) and st.tobytes() == g["state"].tobytes()      # bytes: a -0.0 is not a 0.0
    se.assert_coverage(meshes, g["prim"], g["state"])


@pytest.mark.skipif(not po.ref_available(), reason="the compiled reference is not available here")
def test_oracle_edge_records_equal_the_live_reference():
    meshes, org, dr, o = _edge_oracle(77)
    ref = po.RefLib(); apply_state_scene(ref, meshes, True); ref.build()
    rp, rs = ref.state_batch(org, dr); op, os_ = o.state_batch(org, dr)
    assert np.array_equal(rp, op) and rs.tobytes() == os_.tobytes()
    se.assert_coverage(meshes, rp, rs)


def test_oracle_state_records_equal_state_batch_on_hit_records():
    """the record-driven entry (no ray traced) tied to the pinned ray-driven one: the same records in, the same bytes out"""
    meshes, org, dr, o = _edge_oracle(7)
    prim, st = o.state_batch(org, dr)
    p2, t, u, v = o.intersect(org, dr)
    assert np.array_equal(prim, p2) and (prim != po.MISS).sum() > 500
    assert o.state_records(org, dr, prim, t, u, v).tobytes() == st.tobytes()
    # a miss slot gives zeros and leaves its neighbours alone
    prim = prim.copy(); prim[::5] = po.MISS
    got = o.state_records(org, dr, prim, t, u, v)
    assert not got[::5].any() and got[prim != po.MISS].tobytes() == st[prim != po.MISS].tobytes()
