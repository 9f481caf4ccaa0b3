"""Ordered ray dumps run with thresholds of their own (LH_ORDERED_MIN_ACTIVE / LH_ORDERED_TRI_BATCH, lh_device.h; lh_query.hip lh_launch): the regroup comes
sooner and the triangle pass waits for more parked leaves than in a dump traced as given.  That changes which candidates a ray holds when it retires, how
many of them the full pending list resolves inline before that, and what else its wave is doing meanwhile -- and never a record.  "dump_order_min" 1 sends
dumps of every size through the ordered launch; every record (prim, t, u, v) of such a dump is bit-equal to
  - the same call with "dump_order" 0: the given order under the given dumps' thresholds, in the same process,
  - the textbook walk (variant 0) on the host-built tree,
  - the same ordered call on a device-built tree.
Scenes and batches (the 2 000-triangle soup and 65 536 rays of tests/test_gpu_node_step.py):
  (a) the soup with 1, 2, 4, 5, 8 exact copies of every triangle stacked on itself -- ties at bit-equal t through tie_takes_new with pending lists
      of 2 and 4; with 5 and 8 the full list's inline resolve in front of the retire's;
  (b) a batch in which every ray misses;
  (c) a batch in which every ray hits one large triangle, stacked 1, 4 and 8 times: the 64 rays of a wave retire in the same regroup, with 4
      copies each with a full pending list;
  (d) 1, 63, 64, 65 and 4 097 rays: partial waves, a partial block of the ordering;
  (e) the LDS stack capped at 8 rows: rays leave the walk `over`, through the queue;
  (f) two streams in flight;
  (g) any hit on (a).
Every one of the n records is compared in every case."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NRAYS = 65536
COPIES = (1, 2, 4, 5, 8)
SIZES = (1, 63, 64, 65, 4097)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(out):
    """the records as integers: equal means bit-equal"""
    import torch
    torch.cuda.synchronize()
    return [x.view(torch.int64) if x.dtype == torch.float64 else x for x in out]


def _assert_same(a, b, what):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x, y), "%s: output %d differs in %d slots" % (what, k, int((x != y).sum()))


def _accel(P, idx, build="host"):
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(build=build)
    acc.set_param("wide8", 0)
    acc.set_param("dump_order_min", 1)
    return acc


def _trace(acc, order, d_o, d_d, mode=la.MODE_CLOSEST, **kw):
    acc.set_param("dump_order", order)
    return _bits(acc.intersect_device(d_o, d_d, mode=mode, **kw))


def _ordered(acc, d_o, d_d, what, mode=la.MODE_CLOSEST):
    """the ordered dump (counted as one) and the dump as given: bit-equal; returns the records"""
    acc.order_statistics(clear=True)
    given = _trace(acc, 0, d_o, d_d, mode)
    assert acc.order_statistics()["dumps"] == 0
    got = _trace(acc, 1, d_o, d_d, mode)
    assert acc.order_statistics(clear=True) == {"dumps": 1, "rays": d_o.shape[0]}, what
    _assert_same(got, given, what + ": ordered against given")
    assert got[0].shape[0] == d_o.shape[0]
    return got


def _stacked(P, idx, copies):
    """`copies` exact copies of every triangle, one behind the other in the primitive order"""
    return P, np.ascontiguousarray(np.repeat(idx.reshape(-1, 3), copies, axis=0).ravel())


@pytest.fixture(scope="module")
def soup():
    P, idx, org, dr = po.soup(2000, NRAYS, 0.03, 20261)
    return P, idx, _dev(org), _dev(dr)


def _three_references(P, idx, d_o, d_d, what, caps=(0,)):
    acc = _accel(P, idx)
    direct = _bits(acc.intersect_device(d_o, d_d, variant=la.VARIANT_DIRECT))          # the textbook walk on the host-built tree
    got = None
    for cap in caps:
        acc.set_param("stack_cap", cap)
        got = _ordered(acc, d_o, d_d, "%s, stack_cap %d" % (what, cap))
        _assert_same(got, direct, "%s, stack_cap %d: ordered against the textbook walk" % (what, cap))
    acc.close()
    dev = _accel(P, idx, build="device")
    for cap in caps:
        dev.set_param("stack_cap", cap)
        _assert_same(_ordered(dev, d_o, d_d, "%s, device-built tree, stack_cap %d" % (what, cap)), direct, "%s, stack_cap %d: device-built against host-built tree" % (what, cap))
    dev.close()
    return got


@pytest.mark.parametrize("copies", COPIES)
def test_stacked_duplicates(soup, copies):
    """(a), and (e) on it: the capped stack sends rays through the queue, `over`, at every copy count"""
    P, idx, d_o, d_d = soup
    Pc, ic = _stacked(P, idx, copies)
    got = _three_references(Pc, ic, d_o, d_d, "%d copies" % copies, caps=(0, 8))
    hit = got[0] != -1
    assert int(hit.sum()) > NRAYS // 50
    if copies > 1:          # the stack is met: the winners are not all the first copy, nor all the last
        which = got[0][hit] % copies
        assert int((which != 0).sum()) > 0


def test_all_miss(soup):
    """(b): rays that start outside the scene's box and point away from it"""
    P, idx, d_o, d_d = soup
    lo, hi = P.min(0), P.max(0)
    rng = np.random.default_rng(5)
    org = np.empty((NRAYS, 3)); org[:, :2] = rng.uniform(lo[:2], hi[:2], (NRAYS, 2)); org[:, 2] = hi[2] + rng.uniform(0.01, 1.0, NRAYS)
    dr = rng.uniform(-1.0, 1.0, (NRAYS, 3)); dr[:, 2] = rng.uniform(0.05, 1.0, NRAYS)
    got = _three_references(P, idx, _dev(org), _dev(dr), "all miss")
    assert bool((got[0] == -1).all())


@pytest.mark.parametrize("copies", [1, 4, 8])
def test_all_hit_one_large_triangle(copies):
    """(c): one triangle, stacked; every ray of a wave retires in the same regroup with min(copies, 4) candidates"""
    P = np.array([[-10.0, -10.0, 1.0], [10.0, -10.0, 1.0], [0.0, 10.0, 1.25]])
    idx = np.tile(np.arange(3, dtype=np.uint32), copies)
    rng = np.random.default_rng(6 + copies)
    org = np.zeros((NRAYS, 3)); org[:, :2] = rng.uniform(-1.0, 1.0, (NRAYS, 2)); org[:, 2] = rng.uniform(-1.0, 0.5, NRAYS)
    dr = np.zeros((NRAYS, 3)); dr[:, :2] = rng.uniform(-0.05, 0.05, (NRAYS, 2)); dr[:, 2] = 1.0
    got = _three_references(P, idx, _dev(org), _dev(dr), "one triangle x %d" % copies)
    assert bool((got[0] != -1).all())


@pytest.mark.parametrize("copies", [1, 4])
def test_sizes(soup, copies):
    """(d): partial waves, a partial block of the ordering"""
    P, idx, d_o, d_d = soup
    Pc, ic = _stacked(P, idx, copies)
    acc = _accel(Pc, ic)
    hits = 0
    for n in SIZES:
        o, d = d_o[:n], d_d[:n]          # (from the arrays' start: a dump that begins on an odd multiple of 8 bytes is traced as given)
        got = _ordered(acc, o, d, "%d rays, %d copies" % (n, copies))
        _assert_same(got, _bits(acc.intersect_device(o, d, variant=la.VARIANT_DIRECT)), "%d rays, %d copies: ordered against the textbook walk" % (n, copies))
        hits += int((got[0] != -1).sum())
    assert hits > 0
    acc.close()


def test_two_streams_in_flight(soup):
    """(f)"""
    import torch
    P, idx, d_o, d_d = soup
    Pc, ic = _stacked(P, idx, 4)
    acc = _accel(Pc, ic)
    rays = [(d_o, d_d), (d_o.flip(0).contiguous(), d_d.flip(0).contiguous())]
    given = [_trace(acc, 0, o, d) for o, d in rays]
    acc.set_param("dump_order", 1)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [tuple(torch.empty_like(x) for x in acc.intersect_device(o, d)) for o, d in rays]
    torch.cuda.synchronize()
    acc.order_statistics(clear=True)
    for rep in range(3):
        for k in (0, 1):
            acc.intersect_device(rays[k][0], rays[k][1], out=outs[k], stream=streams[k].cuda_stream)
    for k in (0, 1):
        _assert_same(_bits(outs[k]), given[k], "stream %d" % k)
    assert acc.order_statistics() == {"dumps": 6, "rays": 6 * NRAYS}
    acc.close()


@pytest.mark.parametrize("copies", COPIES)
def test_any_hit_has_not_moved(soup, copies):
    """(g)"""
    P, idx, d_o, d_d = soup
    Pc, ic = _stacked(P, idx, copies)
    acc = _accel(Pc, ic)
    occ = _ordered(acc, d_o, d_d, "any hit, %d copies" % copies, mode=la.MODE_ANY)
    closest = _trace(acc, 0, d_o, d_d)
    import torch
    assert torch.equal(occ[0].bool(), closest[0] != -1)
    acc.close()
