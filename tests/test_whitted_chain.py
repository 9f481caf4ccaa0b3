"""The refraction chain restated (tests/whitted_chain.py: a loop over po.Oracle.state_batch plus the numpy bounce) against
tests/golden/whitted_chain.npz -- the same loop run with the COMPILED REFERENCE's intersect, state and ri_refract on
po.soup(300, 2000, 0.2, 5) (tests/golden/make_whitted_golden.py wrote it).  Without a GPU: this pins the helper the GPU tests
(tests/test_gpu_whitted.py) compare the device against."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import whitted_chain as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "whitted_chain.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def chain():
    P, idx, org, dr = po.soup(300, 2000, 0.2, 5)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    prim0, st0 = o.state_batch(org, dr)
    return prim0, wc.run_chain(o.state_batch, prim0, st0)


def test_the_scene_exercises_the_chain(chain):
    prim0, (bounces, eo, ed, info) = chain
    assert info["hits"] == int((prim0 != po.MISS).sum()) >= 1000
    assert info["cut"] >= 1 and info["tir"] >= 100
    assert all(r > 0 for r in info["rays"][1:]), info["rays"]          # every depth occupied
    assert info["grazing"] == 0 and info["selfhit"] == 0              # none excluded: no ray in the reference's undefined case, none re-hitting its primitive
    d = bounces[prim0 != po.MISS]
    assert set(int(x) for x in d[(d & wc.CUT) == 0]) == set(range(1, 9)) and (d[(d & wc.CUT) != 0] == (8 | wc.CUT)).all()


def test_the_helper_equals_the_compiled_reference_fixture(chain):
    prim0, (bounces, eo, ed, info) = chain
    z = np.load(GOLDEN)
    hits = np.nonzero(prim0 != po.MISS)[0]
    assert np.array_equal(z["hits"], hits.astype(np.uint32))
    assert np.array_equal(z["bounces"], bounces)
    assert np.array_equal(bits(z["end_org"]), bits(eo[hits])) and np.array_equal(bits(z["end_dir"]), bits(ed[hits]))
    assert int(z["tir"]) == info["tir"] and list(z["rays"]) == info["rays"]
    assert np.isnan(eo[prim0 == po.MISS]).all() and (bounces[prim0 == po.MISS] == wc.MISS).all()


def test_depth_limits_cut_where_the_longer_chain_went_on(chain):
    """a chain under a lower limit is the prefix of the longer one: escapes at d <= limit stay, everything else is cut at the limit"""
    prim0, (b8, _, _, _) = chain
    P, idx, org, dr = po.soup(300, 2000, 0.2, 5)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    _, st0 = o.state_batch(org, dr)
    hit = prim0 != po.MISS
    for lim in (3, 1, 0):
        b, eo, ed, info = wc.run_chain(o.state_batch, prim0, st0, max_depth=lim)
        esc = hit & ((b8 & wc.CUT) == 0) & (b8 <= lim)
        assert np.array_equal(b[esc], b8[esc]) and (b[hit & ~esc] == (lim | wc.CUT)).all() and (b[~hit] == wc.MISS).all()
        assert info["cut"] == int((hit & ~esc).sum())
        if lim == 0:
            assert np.isnan(eo).all() and np.isnan(ed).all() and sum(info["rays"]) == 0
