"""The rule of the bounded ray batches (lucille_amd/csrc/lh_tmax.h) without a GPU: the product's bounded host walk
(lh_hostwalk.c lh_host_walk_tmax -- the same start values, the same any-hit threshold, the same near-bound fragility and the same final
accept as the bounded kernels, in host C) over the model's trees, against the oracle's unbounded records filtered with t < tmax.
Every ray is compared, bit for bit, closest and any hit."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import tmax_cases as tc
from tests.helpers import assert_hits_equal


@pytest.mark.parametrize("name", list(tc.SCENES))
def test_bounded_host_walk_equals_the_filtered_oracle(name):
    c = tc.case(name)
    m = tc.TmaxModel(c["P"], c["idx"])
    try:
        for seed in (0, 5):            # two phases of the cycle: every ray meets two classes
            tmax, which = tc.bounds_for(c["exp"], seed, sheets=(name == "sheets"))
            assert np.unique(which).size == (21 if name == "sheets" else tc.NCLASSES)
            exp, occ = tc.expected(c["exp"], tmax)
            got = m.walk(c["org"], c["dr"], tmax, anyhit=False)
            assert_hits_equal(got, exp, "%s, closest hit, seed %d" % (name, seed))
            got_occ = m.walk(c["org"], c["dr"], tmax, anyhit=True)
            bad = np.nonzero(got_occ != occ)[0]
            assert bad.size == 0, "%s, any hit, seed %d: %d rays differ, first %s (classes %s)" % (name, seed, bad.size, bad[:5], which[bad[:5]])
    finally:
        m.close()


def test_the_classes_do_what_the_contract_says():
    """the expectation itself, on the scene with the most hits: +inf, 1e38, 1e300, 2 t0 and nextafter(t0, +inf) keep every hit;
    t0, nextafter(t0, 0), t0 / 2, 0, -1 and NaN keep none (the comparison is strict)"""
    c = tc.case("soup_3k_fat")
    hit = c["exp"][0] != po.MISS
    for cls, keeps in ((tc.INF, True), (tc.E38, True), (tc.E300, True), (tc.TWICE, True), (tc.T0_UP, True), (tc.T0_ABOVE, True),
                       (tc.T0, False), (tc.T0_DOWN, False), (tc.T0_BELOW, False), (tc.HALF, False), (tc.ZERO, False), (tc.NEGATIVE, False),
                       (tc.NAN, False)):
        tmax, _ = tc.bounds_for(c["exp"], 1, classes=[cls])
        _, occ = tc.expected(c["exp"], tmax)
        assert np.array_equal(occ.astype(bool), hit if keeps else np.zeros_like(hit)), cls


def test_sheets_between_the_sheets():
    """bounds between the sheets, every ray with every one of them: the answer is prim 0 at t = 1.0 for each (all are above 1.0), and a
    bound of exactly 1.0 gives a miss"""
    c = tc.case("sheets")
    m = tc.TmaxModel(c["P"], c["idx"])
    try:
        n = c["org"].shape[0]
        for k in range(8):
            tmax = np.full(n, 1.0 + (k + 0.5) * 2e-11)
            exp, occ = tc.expected(c["exp"], tmax)
            assert (exp[0] == 0).all() and (exp[1] == 1.0).all()
            assert_hits_equal(m.walk(c["org"], c["dr"], tmax, anyhit=False), exp, "sheets, bound %d" % k)
            assert np.array_equal(m.walk(c["org"], c["dr"], tmax, anyhit=True), occ)
        prim, t, u, v = m.walk(c["org"], c["dr"], np.full(n, 1.0), anyhit=False)
        assert (prim == po.MISS).all() and (t == 1.0e38).all() and (u == 0.0).all() and (v == 0.0).all()
        assert not m.walk(c["org"], c["dr"], np.full(n, 1.0), anyhit=True).any()
    finally:
        m.close()
