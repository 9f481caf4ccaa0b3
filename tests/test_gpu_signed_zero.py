"""-0.0 and +0.0 direction components on the device: closest-hit and any-hit of the rays of tests/signed_zero_cases.py, on a soup with inner nodes and
on a one-triangle scene, equal the oracle's, bit for bit -- over 4-wide and 8-wide nodes, through the device and the host entry points.  Before
lh_safe_dir (lh_filter.h) took its sign from d < 0 as the ng flags do, every such ray with a -0.0 component that starts between a box's planes of that
axis was a miss."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests import signed_zero_cases as sz
from tests.helpers import assert_hits_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["soup", "one triangle"])
def test_signed_zero_directions_against_the_oracle(name):
    import torch
    P, idx = sz.scenes()[name]
    org, dr, minus = sz.rays(P, idx)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    exp = o.intersect(org, dr, nthreads=8)
    hit = exp[0] != po.MISS
    assert int((hit & minus).sum()) >= 300 and int((hit & ~minus).sum()) >= 90
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    try:
        to, td = torch.from_numpy(org).cuda(), torch.from_numpy(dr).cuda()
        for wide8, variants in ((0, (0, 4)), (1, (-1,))):          # the textbook walk, the default over 4-wide nodes; the default over 8-wide nodes
            acc.set_param("wide8", wide8)
            for variant in variants:
                out = acc.intersect_device(to, td, variant=variant)
                occ = acc.intersect_device(to, td, mode=la.MODE_ANY, variant=variant)[0]
                torch.cuda.synchronize()
                got = (out[0].cpu().numpy().view(np.uint32),) + tuple(x.cpu().numpy() for x in out[1:4])
                assert_hits_equal(got, exp, "%s, wide8 %d, variant %d" % (name, wide8, variant))
                assert np.array_equal(occ.cpu().numpy().astype(bool), hit), (name, wide8, variant, int((occ.cpu().numpy().astype(bool) != hit).sum()))
        acc.set_param("wide8", 0)
        assert_hits_equal(acc.intersect_host(org, dr), exp, "%s, host arrays" % name)
        assert np.array_equal(np.asarray(acc.intersect_host(org, dr, mode=la.MODE_ANY)).astype(bool), hit)
    finally:
        acc.close()
