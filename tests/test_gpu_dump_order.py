"""Ray dumps traced from a copy in bin order (lucille_amd/csrc/lh_order.h, lh_order.hip; the hook in lh_query.hip lh_launch): the order never
shows in a record.  Every record of a dump with "dump_order" 1 (forced on every size by "dump_order_min" 1) is bit-equal to the same call with
"dump_order" 0, closest and any hit, at 1, 63, one block, one block + 1, three blocks + 17 and 70 000 rays (from 65 536 on the fix-up queue and
the cooperative walk run, in ordered space), with either key, with the LDS stack capped at 8 rows (rays through the queue and
k_fixups), for a batch of one bin, and for the edge rays of the key's CPU test that a walk may be given.  LH_POISON_OUTPUTS=1 (tests/conftest.py):
a slot the way back leaves out holds 0x77.  Calls in flight on two streams have a workspace each.  What is not a plain dump -- fp32 rays, 16-byte
records, indexed and bounded calls, a workspace over "dump_order_max_mb" -- is traced as given (lh_accel_order_statistics counts no dump) and
is right.  The 2 000-triangle soup of tests/test_gpu_node_step.py."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests.order_cases import edge_rays, one_bin_rays

pytestmark = pytest.mark.gpu

BLOCK = 4096
SIZES = (1, 63, BLOCK, BLOCK + 1, 3 * BLOCK + 17, 70000)          # the issue's sizes
EDGES = (511, 513, 1023, 1024, 1025)          # ... and those of the passes: 512 rays a step of the count, 1 024 a tile of the copy and the way back
MODES = (la.MODE_CLOSEST, la.MODE_ANY)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def soup():
    P, idx, org, dr = po.soup(2000, SIZES[-1], 0.03, 20261)
    return P, idx, _dev(org), _dev(dr)


@pytest.fixture()
def acc(soup):
    a = la.HipAccel(0); a.add_mesh(soup[0], soup[1]); a.commit()
    a.set_param("dump_order_min", 1)
    yield a
    a.close()


def _bits(out):
    """the records as integers: equal means bit-equal"""
    import torch
    torch.cuda.synchronize()
    return [x.view(torch.int64) if x.dtype == torch.float64 else x for x in out]


def _trace(acc, order, d_o, d_d, mode, **kw):
    acc.set_param("dump_order", order)
    return _bits(acc.intersect_device(d_o, d_d, mode=mode, **kw))


def _assert_same(a, b, what):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s: output %d differs in %d slots" % (what, k, int((x != y).sum()))


def _assert_written(out, mode):
    """every slot was written by the launch: none holds the poison"""
    if mode == la.MODE_CLOSEST:
        assert not bool((out[0] == 0x77777777).any())
        assert not any(bool((x == 0x7777777777777777).any()) for x in out[1:])
    else:
        assert int(out[0].max()) <= 1


def _both(acc, d_o, d_d, mode, what, ordered=True, **kw):
    acc.order_statistics(clear=True)
    given = _trace(acc, 0, d_o, d_d, mode, **kw)
    assert acc.order_statistics()["dumps"] == 0
    got = _trace(acc, 1, d_o, d_d, mode, **kw)
    st = acc.order_statistics(clear=True)
    assert st == ({"dumps": 1, "rays": d_o.shape[0]} if ordered else {"dumps": 0, "rays": 0}), (what, st)
    _assert_same(got, given, what)
    return got


@pytest.mark.parametrize("cap", [0, 8])
@pytest.mark.parametrize("mode", MODES)
def test_records_equal_the_given_order(soup, acc, mode, cap):
    _, _, d_o, d_d = soup
    acc.set_param("stack_cap", cap)
    hits = 0
    for n in SIZES + EDGES:
        got = _both(acc, d_o[:n], d_d[:n], mode, "%d rays, mode %d, stack_cap %d" % (n, mode, cap))
        _assert_written(got, mode)
        hits += int((got[0] != -1).sum()) if mode == la.MODE_CLOSEST else int(got[0].sum())
    assert hits > SIZES[-1] // 50


def test_the_key_under_the_octant(soup, acc):
    _, _, d_o, d_d = soup
    acc.set_param("dump_order_bits", 1)          # the other 6-bit key: one cell bit per axis under the direction octant (pass 1 reads dir)
    for n in (1, 255, 257, 1023, 1025, BLOCK + 1, 70000):          # the sizes of its steps: 256 rays a step of the count, 1 024 a tile of the copy
        for mode in MODES:
            _both(acc, d_o[:n], d_d[:n], mode, "%d rays, octant key, mode %d" % (n, mode))


def test_one_bin_and_edge_rays(soup, acc):
    P = soup[0]
    lo, hi = P.min(0), P.max(0)
    n = 3 * BLOCK + 17
    o1, d1 = one_bin_rays(n, lo, hi, 5)
    o2, d2 = edge_rays(70000, lo, hi, 6, legal_only=True)
    assert np.isfinite(o2).all() and np.isfinite(d2).all() and (d2 == 0.0).any() and (np.abs(d2[d2 != 0.0]) < 1e-300).any()
    for what, o, d in (("one bin", o1, d1), ("edge rays", o2, d2)):
        for cap in (0, 8):
            acc.set_param("stack_cap", cap)
            for mode in MODES:
                got = _both(acc, _dev(o), _dev(d), mode, "%s, mode %d, stack_cap %d" % (what, mode, cap))
                _assert_written(got, mode)


def test_two_streams_in_flight(soup, acc):
    import torch
    _, _, d_o, d_d = soup
    n = 70000
    rays = [(d_o[:n], d_d[:n]), (d_o[:n].flip(0).contiguous(), d_d[:n].flip(0).contiguous())]
    given = [_trace(acc, 0, o, d, la.MODE_CLOSEST) for o, d in rays]
    acc.set_param("dump_order", 1)
    acc.order_statistics(clear=True)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = [tuple(torch.empty_like(x) for x in acc.intersect_device(o, d)) for o, d in rays]
    acc.order_statistics(clear=True)
    torch.cuda.synchronize()
    for rep in range(3):          # both streams busy at once: a shared workspace would mix the two dumps
        for k in (0, 1):
            acc.intersect_device(rays[k][0], rays[k][1], out=outs[k], stream=streams[k].cuda_stream)
    for k in (0, 1):
        _assert_same(_bits(outs[k]), given[k], "stream %d" % k)
    assert acc.order_statistics() == {"dumps": 6, "rays": 6 * n}


def test_what_is_not_a_plain_dump_is_traced_as_given(soup, acc):
    import torch
    _, _, d_o, d_d = soup
    n = 70000
    o, d = d_o[:n], d_d[:n]
    ref = _trace(acc, 0, o, d, la.MODE_CLOSEST)
    # the workspace (82 bytes a ray: 5.7 MB) over the cap
    acc.set_param("dump_order_max_mb", 1)
    for mode in MODES:
        _both(acc, o, d, mode, "dump_order_max_mb 1, mode %d" % mode, ordered=False)
    acc.set_param("dump_order_max_mb", 0)
    _both(acc, o, d, la.MODE_CLOSEST, "the cap lifted")
    # fp32 rays, 16-byte records
    o32, d32 = o.float(), d.float()
    got32 = _both(acc, o32, d32, la.MODE_CLOSEST, "fp32 rays", ordered=False)
    occ32 = _both(acc, o32, d32, la.MODE_ANY, "fp32 rays, any hit", ordered=False)
    # ... and right: fp32 rays are traced as the widened fp64 rays, whose records a dump as given supplies
    wide = _trace(acc, 0, o32.double(), d32.double(), la.MODE_CLOSEST)
    _assert_same(got32, wide, "fp32 rays against their widened fp64 rays")
    assert torch.equal(occ32[0].bool(), wide[0] != -1) and int((wide[0] != -1).sum()) > n // 50
    rec = _both(acc, o, d, la.MODE_CLOSEST, "16-byte records", ordered=False, records="rec16")[0]
    assert torch.equal(rec[:, 0], ref[0])
    assert torch.equal(rec[:, 1].view(torch.float32), ref[1].view(torch.float64).float())
    # an indexed call: the listed rays' slots alone are written
    index = torch.arange(0, n, 3, dtype=torch.int32, device=o.device)
    outs = []
    for order in (0, 1):
        out = tuple(x.new_full((n,), 5) for x in acc.intersect_device(o[:1], d[:1]))
        acc.order_statistics(clear=True)
        outs.append(_trace(acc, order, o, d, la.MODE_CLOSEST, out=out, index=index))
        assert acc.order_statistics(clear=True)["dumps"] == 0
    _assert_same(outs[1], outs[0], "indexed")
    assert torch.equal(outs[1][0][::3], ref[0][::3]) and bool((outs[1][0][1::3] == 5).all())
    # a bounded call: a hit beyond its bound is a miss
    tmax = torch.full((n,), 0.25, dtype=torch.float64, device=o.device)
    got = _both(acc, o, d, la.MODE_CLOSEST, "tmax", ordered=False, tmax=tmax)
    t_ref = ref[1].view(torch.float64)
    near = (ref[0] != -1) & (t_ref < 0.25)
    assert torch.equal(got[0][near], ref[0][near]) and bool((got[0][~near] == -1).all()) and 0 < int(near.sum()) < int((ref[0] != -1).sum())


def test_counted_launch_reports_its_rays(soup, acc):
    _, _, d_o, d_d = soup
    n = 70000
    given = _trace(acc, 0, d_o[:n], d_d[:n], la.MODE_CLOSEST)
    acc.set_param("dump_order", 1)
    acc.order_statistics(clear=True)
    out, cnt = acc.intersect_device(d_o[:n], d_d[:n], counters=True)
    assert cnt["rays"] == n and cnt["nodes"] > n
    assert acc.order_statistics(clear=True) == {"dumps": 1, "rays": n}
    _assert_same(_bits(out), given, "counted launch")
