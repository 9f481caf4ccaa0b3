"""-0.0 and +0.0 direction components through lh_ray_setup / lh_slab (lh_filter.h) on the CPU: the host model of the kernel (tests/cpu_model/lh_model.c,
every node layout, closest-hit and any-hit) and the product's one-ray host walk (lh_hostwalk.c) against the oracle, on the rays of
tests/signed_zero_cases.py.  With a negative clamped inverse next to ng = 0, a ray with a -0.0 component missed every box whose planes of that axis it
starts between."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import signed_zero_cases as sz
from tests.helpers import Model, assert_hits_equal


@pytest.mark.parametrize("name", ["soup", "one triangle"])
def test_signed_zero_directions_in_the_host_model(name):
    P, idx = sz.scenes()[name]
    org, dr, minus = sz.rays(P, idx)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    exp = o.intersect(org, dr, nthreads=4)
    hit = exp[0] != po.MISS
    print("%s: %d rays, %d with a -0.0 component, of which the oracle hits %d; %d of the others" % (name, org.shape[0], int(minus.sum()),
                                                                                           int((hit & minus).sum()), int((hit & ~minus).sum())))
    assert int((hit & minus).sum()) >= 300 and int((hit & ~minus).sum()) >= 90          # the one triangle is hit along z alone
    m = Model(P, idx)
    for q in (0, 2, 4):
        got, _ = m.trace(org, dr, qnodes=q)
        assert_hits_equal(got, exp, "%s, node layout %d" % (name, q))
        occ, _ = m.trace(org, dr, anyhit=True, qnodes=q)
        assert np.array_equal(occ.astype(bool), hit), (name, q)
    m.ref_build()
    try:
        assert_hits_equal(m.hostwalk(org, dr), exp, "%s, host walk" % name)
    finally:
        Model.ref_off()
