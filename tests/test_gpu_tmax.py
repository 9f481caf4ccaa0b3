"""Per-ray maximum distance on the device and host paths (lh_accel_intersect_device_tmax / _host_tmax).

The expectation is the contract: the unbounded record -- the oracle's, or where the test says so the unbounded entry point's of the
same accelerator -- kept where it is a hit with t < tmax (fp64, strict), else the miss record / 0 (tests/tmax_cases.py).  Every
comparison is bit for bit.  LH_POISON_OUTPUTS=1 (tests/conftest.py): a record slot no kernel wrote cannot pass."""
import ctypes as C
import functools

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import binding
from oracle import pyoracle as po
from tests import danger_scenes as ds
from tests import tmax_cases as tc
from tests.helpers import assert_hits_equal

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
NEAR_CLASSES = [tc.T0, tc.T0_UP, tc.T0_DOWN, tc.T0_ABOVE, tc.T0_BELOW]


def cu(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the shared cases are read-only


def pack16(rec4):
    prim, t, u, v = rec4
    rec = np.empty((prim.shape[0], 4), np.uint32)
    rec[:, 0] = prim
    for k, a in ((1, t), (2, u), (3, v)):
        rec[:, k] = np.asarray(a, np.float64).astype(np.float32).view(np.uint32)
    return rec


def dev(acc, org, dr, tmax, mode=la.MODE_CLOSEST, records="f64", **kw):
    """HipAccel.intersect_device(..., tmax=...) -> numpy: (prim u32, t, u, v), the (n, 4) u32 records, or the occluded bytes"""
    import torch
    out = acc.intersect_device(cu(org), cu(dr), mode=mode, records=records, tmax=None if tmax is None else cu(tmax), **kw)
    torch.cuda.synchronize()
    out = tuple(x.cpu().numpy() for x in out)
    if mode == la.MODE_ANY:
        return out[0]
    if records == "rec16":
        return out[0].view(np.uint32)
    return (out[0].view(np.uint32),) + out[1:]


def assert_rec16(got, exp, what):
    bad = np.nonzero((got != exp).any(1))[0]
    assert bad.size == 0, "%s: %d of %d records differ, first %s: got %r expected %r" % (what, bad.size, got.shape[0], bad[:4], got[bad[:4]], exp[bad[:4]])


def assert_occ(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, "%s: %d of %d bytes differ, first %s: got %r expected %r" % (what, bad.size, got.shape[0], bad[:6], got[bad[:6]], exp[bad[:6]])


def check_three(acc, org, dr, tmax, exp, occ, what, **kw):
    """closest hit (SoA and rec16) and any hit of one bounded batch"""
    assert_hits_equal(dev(acc, org, dr, tmax, **kw), exp, what + ": closest hit")
    assert_rec16(dev(acc, org, dr, tmax, records="rec16", **kw), pack16(exp), what + ": closest hit, rec16")
    assert_occ(dev(acc, org, dr, tmax, mode=la.MODE_ANY, **kw), occ, what + ": any hit")


@functools.lru_cache(maxsize=None)
def f32_case(name):
    """the fp32 twins of a scene's rays and the oracle's records of the rays they stand for (computed once, read-only)"""
    c = tc.case(name)
    o32 = np.ascontiguousarray(c["org"], np.float32); d32 = np.ascontiguousarray(c["dr"], np.float32)
    o = po.Oracle(); o.add_mesh(c["P"], c["idx"]); o.build()
    exp = o.intersect(o32.astype(np.float64), d32.astype(np.float64), nthreads=8)
    for a in (o32, d32) + tuple(exp):
        a.setflags(write=False)
    return o32, d32, exp


def f32_bounds(exp, seed, **kw):
    """float bounds and the doubles they ARE"""
    t64, which = tc.bounds_for(exp, seed, **kw)
    with np.errstate(over="ignore"):
        t32 = np.ascontiguousarray(t64.astype(np.float32))
    return t32, t32.astype(np.float64), which


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide8", [0, 1])
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("name", list(tc.SCENES))
def test_oracle_parity(name, build, wide8):
    c = tc.case(name)
    acc = la.HipAccel(0); acc.add_mesh(c["P"], c["idx"]); acc.commit(build=build); acc.wait_exact()
    acc.set_param("wide8", wide8)
    what = "%s, %s tree, wide8 %d" % (name, build, wide8)
    tmax, _ = tc.bounds_for(c["exp"], 3, sheets=(name == "sheets"))
    exp, occ = tc.expected(c["exp"], tmax)
    check_three(acc, c["org"], c["dr"], tmax, exp, occ, what + ", fp64 rays")
    o32, d32, exp32 = f32_case(name)
    t32, t32w, _ = f32_bounds(exp32, 4, sheets=(name == "sheets"))
    e32, occ32 = tc.expected(exp32, t32w)
    check_three(acc, o32, d32, t32, e32, occ32, what + ", fp32 rays")
    acc.close()


# ---- 2. identity -----------------------------------------------------------------------------------------------------------------
def raw(acc, fn, d_org, d_dir, d_tmax, fmt, rf, outs, mode, index=None, n_index=0, count=None):
    """the C entry points themselves: fn "tmax" (d_tmax may be None), "ex" or "indexed"; outs = (prim_or_rec, t, u, v, occ) tensors or None"""
    import torch
    p = [None if x is None else C.c_void_p(x.data_ptr()) for x in outs]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = d_org.shape[0]
    ip = None if index is None else C.c_void_p(index.data_ptr()); cp = None if count is None else C.c_void_p(count.data_ptr())
    if fn == "tmax":
        rc = acc.L.lh_accel_intersect_device_tmax(acc.h, n, d_org.data_ptr(), d_dir.data_ptr(), None if d_tmax is None else C.c_void_p(d_tmax.data_ptr()),
                                                  fmt, rf, p[0], p[1], p[2], p[3], p[4], mode, ip, n_index, cp, s)
    elif fn == "ex":
        rc = acc.L.lh_accel_intersect_device_ex(acc.h, n, d_org.data_ptr(), d_dir.data_ptr(), fmt, rf, p[0], p[1], p[2], p[3], p[4], mode, s)
    else:
        rc = acc.L.lh_accel_intersect_device_indexed(acc.h, n, d_org.data_ptr(), d_dir.data_ptr(), fmt, rf, p[0], p[1], p[2], p[3], p[4], mode, ip, n_index, cp, s)
    assert rc == 0, acc.L.lh_last_error()


def filled_outs(n, mode, rf):
    import torch
    if mode == la.MODE_ANY:
        return (None, None, None, None, torch.full((n,), 0x33, dtype=torch.uint8, device="cuda"))
    if rf == binding.REC16:
        return (torch.full((n, 4), FILL, dtype=torch.int32, device="cuda"), None, None, None, None)
    return (torch.full((n,), FILL, dtype=torch.int32, device="cuda"),) + tuple(torch.full((n,), 0.25, dtype=torch.float64, device="cuda") for _ in range(3)) + (None,)


def same_bytes(a, b):
    import torch
    for x, y in zip(a, b):
        if x is None:
            continue
        if not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
            return False
    return True


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_null_and_infinite_bounds_are_the_unbounded_call(f32):
    import torch
    c = tc.case("soup20k")
    dt = np.float32 if f32 else np.float64
    d_o = cu(c["org"].astype(dt)); d_d = cu(c["dr"].astype(dt)); n = d_o.shape[0]
    fmt = binding.RAYS_F32 if f32 else binding.RAYS_F64
    inf = torch.full((n,), float("inf"), dtype=d_o.dtype, device="cuda")
    index = torch.arange(0, n, 3, dtype=torch.int32, device="cuda"); ni = int(index.numel())
    acc = la.HipAccel(0); acc.add_mesh(c["P"], c["idx"]); acc.commit()
    for mode, rf in ((la.MODE_CLOSEST, binding.REC_F64), (la.MODE_CLOSEST, binding.REC16), (la.MODE_ANY, binding.REC_F64)):
        ref = filled_outs(n, mode, rf); raw(acc, "ex", d_o, d_d, None, fmt, rf, ref, mode)
        for tm in (None, inf):
            got = filled_outs(n, mode, rf); raw(acc, "tmax", d_o, d_d, tm, fmt, rf, got, mode)
            torch.cuda.synchronize()
            assert same_bytes(got, ref), ("dense", mode, rf, tm is None)
        ref = filled_outs(n, mode, rf); raw(acc, "indexed", d_o, d_d, None, fmt, rf, ref, mode, index, ni)
        for tm in (None, inf):
            got = filled_outs(n, mode, rf); raw(acc, "tmax", d_o, d_d, tm, fmt, rf, got, mode, index, ni)
            torch.cuda.synchronize()
            assert same_bytes(got, ref), ("listed", mode, rf, tm is None)
    acc.close()


# ---- 3. lists --------------------------------------------------------------------------------------------------------------------
def test_lists():
    """listed slots equal the dense bounded call, unlisted slots keep their fill pattern: every third id, with duplicates, with ids
    beyond the arrays, with a device count smaller than, larger than and equal to zero, and a count written by compact() earlier on the
    stream.  The bounds are addressed by ray id, not by list position"""
    import torch
    c = tc.case("soup20k")
    n = c["org"].shape[0]
    tmax, _ = tc.bounds_for(c["exp"], 6)
    exp, occ = tc.expected(c["exp"], tmax)
    d_o = cu(c["org"]); d_d = cu(c["dr"]); d_tm = cu(tmax)
    acc = la.HipAccel(0); acc.add_mesh(c["P"], c["idx"]); acc.commit()
    third = np.arange(0, n, 3, dtype=np.int32)
    rng = np.random.default_rng(8)
    dup = np.concatenate([third, third[::5], third[:100]]).astype(np.int32)
    beyond = third.copy(); beyond[::7] = n + rng.integers(0, 1000, beyond[::7].shape[0]); beyond[3] = -1          # 0xFFFFFFFF
    unbounded = acc.intersect_device(d_o, d_d)
    lists = [("every third", third, None), ("duplicates", dup, None), ("ids beyond the arrays", beyond, None),
             ("count below the list", third, 1000), ("count above the list", third, 10 ** 9), ("count zero", third, 0)]
    for what, ids, cnt in lists:
        index = cu(ids); count = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device="cuda")
        m = ids.shape[0] if cnt is None else min(cnt, ids.shape[0])
        listed = np.zeros(n, bool); sel = ids[:m]; listed[sel[(sel >= 0) & (sel < n)]] = True
        for mode, rf in ((la.MODE_CLOSEST, binding.REC_F64), (la.MODE_CLOSEST, binding.REC16), (la.MODE_ANY, binding.REC_F64)):
            outs = filled_outs(n, mode, rf)
            raw(acc, "tmax", d_o, d_d, d_tm, binding.RAYS_F64, rf, outs, mode, index, ids.shape[0], count)
            torch.cuda.synchronize()
            if mode == la.MODE_ANY:
                got = outs[4].cpu().numpy()
                assert_occ(got[listed], occ[listed], what + ": listed bytes"); assert (got[~listed] == 0x33).all(), what + ": an unlisted byte was written"
            elif rf == binding.REC16:
                got = outs[0].cpu().numpy().view(np.uint32)
                assert_rec16(got[listed], pack16(exp)[listed], what + ": listed rec16"); assert (got[~listed] == FILL).all(), what + ": an unlisted record was written"
            else:
                got = tuple(x.cpu().numpy() for x in outs[:4])
                assert_hits_equal(tuple(g[listed] for g in got), tuple(e[listed] for e in exp), what + ": listed records")
                assert (got[0][~listed].view(np.uint32) == FILL).all() and all((g[~listed] == 0.25).all() for g in got[1:]), what + ": an unlisted record was written"
    # the shadow-pass pattern: closest hit, compact the hits, bounded any hit on them -- the count never leaves the device
    index, count = la.compact(unbounded[0], la.SELECT_HIT)
    outs = filled_outs(n, la.MODE_ANY, binding.REC_F64)
    raw(acc, "tmax", d_o, d_d, d_tm, binding.RAYS_F64, binding.REC_F64, outs, la.MODE_ANY, index, int(index.numel()), count)
    torch.cuda.synchronize()
    hit = c["exp"][0] != po.MISS
    got = outs[4].cpu().numpy()
    assert int(count.item()) == int(hit.sum())
    assert_occ(got[hit], occ[hit], "compact(): listed bytes"); assert (got[~hit] == 0x33).all()
    acc.close()


# ---- 4. fix-up paths -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup200k():
    return po.soup(200000, 100000, 0.005, 43)


def retraced(acc):
    return int(acc.L.lh_accel_last_retraced(acc.h))


@pytest.mark.parametrize("nrays", [100000, 30000])
def test_fixup_paths(nrays):
    """a stack capped at 8 rows and a visit budget of 16 (test_rec16_through_the_fixup_paths' shapes): 100 000 rays go through the fix-up
    queue to the cooperative walk, 30 000 stay flagged for k_fixups.  Expectation: the unbounded entry point's records of the same
    accelerator, filtered"""
    P, idx, org, dr = soup200k()
    org = np.ascontiguousarray(org[:nrays]); dr = np.ascontiguousarray(dr[:nrays])
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    acc.set_param("wide8", 0); acc.set_param("stack_cap", 8); acc.set_param("ray_budget", 16)
    unb = dev(acc, org, dr, None)
    assert (unb[0] != po.MISS).sum() > 1000
    tmax, _ = tc.bounds_for(unb, 9)
    exp, occ = tc.expected(unb, tmax)
    check_three(acc, org, dr, tmax, exp, occ, "capped stack, %d rays" % nrays)
    acc.trace_statistics(True); acc.statistics(clear=True)
    assert_hits_equal(dev(acc, org, dr, tmax), exp, "capped stack, counted")
    s = acc.statistics(clear=True); r = retraced(acc)
    acc.trace_statistics(False)
    assert r > 0, r
    assert s["rays"] == nrays and s["hits"] == int(occ.sum()) and s["nodes"] > 0
    acc.close()


# ---- 5. small batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 64])
def test_small_batches(n):
    """batches of at most 64 rays take k_trace_small_tmax, dense and listed"""
    import torch
    c = tc.case("soup_3k_fat")
    org = np.ascontiguousarray(c["org"][:n]); dr = np.ascontiguousarray(c["dr"][:n]); unb = tuple(x[:n] for x in c["exp"])
    acc = la.HipAccel(0); acc.add_mesh(c["P"], c["idx"]); acc.commit()
    for seed in range(4):
        tmax, _ = tc.bounds_for(unb, seed)
        exp, occ = tc.expected(unb, tmax)
        check_three(acc, org, dr, tmax, exp, occ, "%d rays, seed %d" % (n, seed))
    ids = np.arange(n - 1, -1, -2, dtype=np.int32); listed = np.zeros(n, bool); listed[ids] = True
    tmax, _ = tc.bounds_for(unb, 2); exp, occ = tc.expected(unb, tmax)
    outs = filled_outs(n, la.MODE_CLOSEST, binding.REC_F64)
    raw(acc, "tmax", cu(org), cu(dr), cu(tmax), binding.RAYS_F64, binding.REC_F64, outs, la.MODE_CLOSEST, cu(ids), ids.shape[0])
    bytes_ = filled_outs(n, la.MODE_ANY, binding.REC_F64)
    raw(acc, "tmax", cu(org), cu(dr), cu(tmax), binding.RAYS_F64, binding.REC_F64, bytes_, la.MODE_ANY, cu(ids), ids.shape[0])
    torch.cuda.synchronize()
    got = tuple(x.cpu().numpy() for x in outs[:4])
    assert_hits_equal(tuple(g[listed] for g in got), tuple(e[listed] for e in exp), "%d rays, listed" % n)
    assert (got[0][~listed].view(np.uint32) == FILL).all() and (got[1][~listed] == 0.25).all()
    b = bytes_[4].cpu().numpy()
    assert_occ(b[listed], occ[listed], "%d rays, listed bytes" % n); assert (b[~listed] == 0x33).all()
    acc.close()


# ---- 6. reference-walk routing ---------------------------------------------------------------------------------------------------
def _routing(P, idx, org, dr, what):
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    unb = o.intersect(org, dr, nthreads=8)
    assert (unb[0] != po.MISS).sum() > 500
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit(); acc.wait_exact()
    for seed in (0, 1):
        tmax, _ = tc.bounds_for(unb, seed, classes=NEAR_CLASSES)
        exp, occ = tc.expected(unb, tmax)
        check_three(acc, org, dr, tmax, exp, occ, "%s, seed %d" % (what, seed))
    acc.trace_statistics(True)
    dev(acc, org, dr, tmax); r_closest = retraced(acc)
    dev(acc, org, dr, tmax, mode=la.MODE_ANY); r_any = retraced(acc)
    acc.trace_statistics(False)
    acc.close()
    return unb, r_closest, r_any


def test_routing_beyond_deg_dcap():
    """the strip scene of tests/danger_scenes.py: rays beyond deg_dcap that hit the danger box are the reference walk's, whose
    (unbounded) record is filtered with t < tmax -- bounds at and around the hit"""
    P, idx, info = ds.one_leaf_scene()
    org, dr = ds.strip_rays(100000, info)
    unb, r_closest, r_any = _routing(P, idx, org, dr, "strip beyond deg_dcap")
    nz = int((unb[0] == info["zprim"]).sum())
    assert nz >= 500 and r_closest >= nz and r_any > 0, (nz, r_closest, r_any)


def test_routing_of_fragile_hits():
    """the chain scene with rays aimed at vertices, edges and centroids: fragile hits (box faces, exact-t ties) and, with bounds within
    LH_FRAGILE_REL of the hit, the near-bound rule send rays through the reference walk"""
    c = tc.case("chain120")
    unb, r_closest, r_any = _routing(c["P"], c["idx"], c["org"], c["dr"], "chain, vertex-aimed rays")
    assert r_closest > 0 and r_any > 0, (r_closest, r_any)


# ---- 7. empty scene --------------------------------------------------------------------------------------------------------------
def test_empty_scene():
    """300 pre-filled records all become the miss record / 0, dense; listed, only the listed ones do"""
    import torch
    n = 300
    acc = la.HipAccel(0); acc.commit()
    d_o = torch.zeros((n, 3), dtype=torch.float64, device="cuda"); d_d = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    d_tm = torch.full((n,), 5.0, dtype=torch.float64, device="cuda")
    miss = (np.full(n, po.MISS, np.uint32), np.full(n, 1e38), np.zeros(n), np.zeros(n))
    ids = np.arange(1, n, 4, dtype=np.int32); listed = np.zeros(n, bool); listed[ids] = True
    for index, mask in ((None, np.ones(n, bool)), (cu(ids), listed)):
        ni = 0 if index is None else int(index.numel())
        outs = filled_outs(n, la.MODE_CLOSEST, binding.REC_F64); raw(acc, "tmax", d_o, d_d, d_tm, binding.RAYS_F64, binding.REC_F64, outs, la.MODE_CLOSEST, index, ni)
        r16 = filled_outs(n, la.MODE_CLOSEST, binding.REC16); raw(acc, "tmax", d_o, d_d, d_tm, binding.RAYS_F64, binding.REC16, r16, la.MODE_CLOSEST, index, ni)
        occ = filled_outs(n, la.MODE_ANY, binding.REC_F64); raw(acc, "tmax", d_o, d_d, d_tm, binding.RAYS_F64, binding.REC_F64, occ, la.MODE_ANY, index, ni)
        torch.cuda.synchronize()
        got = tuple(x.cpu().numpy() for x in outs[:4])
        assert_hits_equal(tuple(g[mask] for g in got), tuple(e[mask] for e in miss), "empty scene")
        assert (got[0][~mask].view(np.uint32) == FILL).all() and (got[1][~mask] == 0.25).all()
        g16 = r16[0].cpu().numpy().view(np.uint32)
        assert_rec16(g16[mask], pack16(miss)[mask], "empty scene, rec16"); assert (g16[~mask] == FILL).all()
        b = occ[4].cpu().numpy()
        assert (b[mask] == 0).all() and (b[~mask] == 0x33).all()
    acc.close()


# ---- 8. pruning ------------------------------------------------------------------------------------------------------------------
def test_the_bound_prunes_the_walk():
    """statistics on, the any-hit rays of the 200 000-triangle soup, once with every bound +inf and once with every bound 0.01: the short run
    visits strictly fewer nodes and filters strictly fewer triangles, traces as many rays, and its hits are the expected bytes'"""
    P, idx, org, dr = soup200k()
    n = org.shape[0]
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    unb = dev(acc, org, dr, None)
    stats = {}
    acc.trace_statistics(True)
    for name, bound in (("inf", np.inf), ("short", 0.01)):
        tmax = np.full(n, bound)
        _, occ = tc.expected(unb, tmax)
        acc.statistics(clear=True)
        got = dev(acc, org, dr, tmax, mode=la.MODE_ANY)
        stats[name] = acc.statistics(clear=True)
        assert_occ(got, occ, "any hit, bounds %s" % name)
        assert stats[name]["hits"] == int(occ.sum()), (name, stats[name], int(occ.sum()))
    acc.trace_statistics(False)
    a, b = stats["inf"], stats["short"]
    msg = "node visits %d -> %d (x %.3f), triangles through the filter %d -> %d (x %.3f)" % (
        a["nodes"], b["nodes"], b["nodes"] / max(a["nodes"], 1), a["tris"], b["tris"], b["tris"] / max(a["tris"], 1))
    print(msg)
    assert a["rays"] == b["rays"] == n, msg
    assert b["nodes"] < a["nodes"] and b["tris"] < a["tris"], msg
    assert b["hits"] <= a["hits"], (a["hits"], b["hits"])
    acc.close()


# ---- 9. host form ----------------------------------------------------------------------------------------------------------------
def host(acc, org, dr, tmax, fmt, rf, mode=la.MODE_CLOSEST):
    """lh_accel_intersect_host_tmax through ctypes"""
    org = np.ascontiguousarray(org); dr = np.ascontiguousarray(dr); tmax = np.ascontiguousarray(tmax)
    n = org.shape[0]; L = acc.L
    if mode == la.MODE_ANY:
        occ = np.full(n, 0x55, np.uint8)
        rc = L.lh_accel_intersect_host_tmax(acc.h, n, org.ctypes.data, dr.ctypes.data, tmax.ctypes.data, fmt, rf, None, None, None, None, occ.ctypes.data, mode)
        assert rc == 0, L.lh_last_error()
        return occ
    if rf == binding.REC16:
        rec = binding._rec16_host(n)
        rc = L.lh_accel_intersect_host_tmax(acc.h, n, org.ctypes.data, dr.ctypes.data, tmax.ctypes.data, fmt, rf, rec.ctypes.data, None, None, None, None, mode)
        assert rc == 0, L.lh_last_error()
        return rec
    prim = np.empty(n, np.uint32); t = np.empty(n); u = np.empty(n); v = np.empty(n)
    rc = L.lh_accel_intersect_host_tmax(acc.h, n, org.ctypes.data, dr.ctypes.data, tmax.ctypes.data, fmt, rf, prim.ctypes.data, t.ctypes.data, u.ctypes.data,
                                        v.ctypes.data, None, mode)
    assert rc == 0, L.lh_last_error()
    return prim, t, u, v


def test_host_form():
    c = tc.case("soup20k")
    acc = la.HipAccel(0); acc.add_mesh(c["P"], c["idx"]); acc.commit()
    tmax, _ = tc.bounds_for(c["exp"], 11)
    exp, occ = tc.expected(c["exp"], tmax)
    assert_hits_equal(host(acc, c["org"], c["dr"], tmax, binding.RAYS_F64, binding.REC_F64), exp, "host, fp64 rays")
    assert_rec16(host(acc, c["org"], c["dr"], tmax, binding.RAYS_F64, binding.REC16), pack16(exp), "host, fp64 rays, rec16")
    assert_occ(host(acc, c["org"], c["dr"], tmax, binding.RAYS_F64, binding.REC_F64, la.MODE_ANY), occ, "host, fp64 rays, any hit")
    o32, d32, exp32 = f32_case("soup20k")
    t32, t32w, _ = f32_bounds(exp32, 12)
    e32, occ32 = tc.expected(exp32, t32w)
    assert_hits_equal(host(acc, o32, d32, t32, binding.RAYS_F32, binding.REC_F64), e32, "host, fp32 rays")
    assert_rec16(host(acc, o32, d32, t32, binding.RAYS_F32, binding.REC16), pack16(e32), "host, fp32 rays, rec16")
    assert_occ(host(acc, o32, d32, t32, binding.RAYS_F32, binding.REC_F64, la.MODE_ANY), occ32, "host, fp32 rays, any hit")
    # the binding: numpy in, numpy out (what intersect_host(..., tmax=...) calls); a NULL bound is lh_accel_intersect_host_ex
    assert_hits_equal(acc.intersect_host_tmax(c["org"], c["dr"], tmax), exp, "binding, host")
    assert_rec16(acc.intersect_host_tmax(o32, d32, t32, records="rec16"), pack16(e32), "binding, host, fp32 rays, rec16")
    assert_occ(acc.intersect_host_tmax(c["org"], c["dr"], tmax, mode=la.MODE_ANY), occ, "binding, host, any hit")
    prim = np.empty(8, np.uint32); t = np.empty(8); u = np.empty(8); v = np.empty(8)
    o8 = np.ascontiguousarray(c["org"][:8]); d8 = np.ascontiguousarray(c["dr"][:8])
    assert acc.L.lh_accel_intersect_host_tmax(acc.h, 8, o8.ctypes.data, d8.ctypes.data, None, binding.RAYS_F64, binding.REC_F64, prim.ctypes.data,
                                              t.ctypes.data, u.ctypes.data, v.ctypes.data, None, la.MODE_CLOSEST) == 0
    assert_hits_equal((prim, t, u, v), tuple(x[:8] for x in c["exp"]), "host, NULL bound")
    # statistics on: the bounded host form counts its rays and the hits that are left after the bound, the unbounded one the oracle's hits
    n = c["org"].shape[0]
    acc.trace_statistics(True); acc.statistics(clear=True)
    for mode in (la.MODE_CLOSEST, la.MODE_ANY):
        host(acc, c["org"], c["dr"], tmax, binding.RAYS_F64, binding.REC_F64, mode)
        s = acc.statistics(clear=True)
        assert s["rays"] == n and s["hits"] == int(occ.sum()) and s["nodes"] > 0, (mode, s, int(occ.sum()))
    rec = binding._rec16_host(n)
    assert acc.L.lh_accel_intersect_host_ex(acc.h, n, c["org"].ctypes.data, c["dr"].ctypes.data, binding.RAYS_F64, binding.REC16, rec.ctypes.data,
                                            None, None, None, None, la.MODE_CLOSEST) == 0, acc.L.lh_last_error()
    s = acc.statistics(clear=True)
    acc.trace_statistics(False)
    assert s["rays"] == n and s["hits"] == tc.SCENES["soup20k"][2] == 13568 and s["nodes"] > 0, s
    assert_rec16(rec, pack16(c["exp"]), "host_ex, counted, rec16")
    acc.close()


def test_host_form_two_chunks(monkeypatch):
    """2^21 + 777 rays: more than one chunk of the host form, on an accelerator created under a small pipeline ring (which the bounded
    host form does not use: it takes the plain path in chunks).  Expectation: the unbounded device records of the same accelerator, filtered"""
    P, idx, _, _ = po.soup(20000, 10, 0.01, 46)
    n = 2 ** 21 + 777
    rng = np.random.default_rng(46)
    o32 = rng.uniform(-0.2, 1.2, (n, 3)).astype(np.float32); d32 = rng.normal(size=(n, 3)).astype(np.float32)
    monkeypatch.setenv("LH_PIPE_CHUNK", str(1 << 16)); monkeypatch.setenv("LH_PIPE_DEPTH", "2")
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    unb = dev(acc, o32.astype(np.float64), d32.astype(np.float64), None)
    t32, t32w, _ = f32_bounds(unb, 13)
    exp, occ = tc.expected(unb, t32w)
    assert (exp[0] != po.MISS).sum() > 10000
    assert_rec16(host(acc, o32, d32, t32, binding.RAYS_F32, binding.REC16), pack16(exp), "two chunks, fp32 rays, rec16")
    assert_occ(host(acc, o32, d32, t32, binding.RAYS_F32, binding.REC_F64, la.MODE_ANY), occ, "two chunks, any hit")
    acc.trace_statistics(True); acc.statistics(clear=True)          # statistics add up over the chunks
    assert_occ(host(acc, o32, d32, t32, binding.RAYS_F32, binding.REC_F64, la.MODE_ANY), occ, "two chunks, any hit, counted")
    s = acc.statistics(clear=True)
    acc.trace_statistics(False)
    assert s["rays"] == n and s["hits"] == int(occ.sum()), (s, n, int(occ.sum()))
    acc.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    """each refusal returns -1 with its message and leaves the caller's outputs as they were, device and host forms; n == 0 is no work"""
    import torch
    P, idx, org, dr = po.soup(2000, 1000, 0.01, 48)
    acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.commit()
    o32 = np.ascontiguousarray(org, np.float32); d32 = np.ascontiguousarray(dr, np.float32)
    n = o32.shape[0]; L = acc.L
    F32, R16, R64 = binding.RAYS_F32, binding.REC16, binding.REC_F64
    # host form
    rec = binding._rec16_host(n); rec[:] = FILL
    t = np.full(n, 0.25); occ = np.full(n, 0x33, np.uint8); tm = np.ones(n + 1, np.float32)
    cases = [
        (tm.ctypes.data, 2, R64, rec.ctypes.data, None, None, la.MODE_CLOSEST, "ray format"),
        (tm.ctypes.data, F32, 2, rec.ctypes.data, None, None, la.MODE_CLOSEST, "record format"),
        (tm.ctypes.data, F32, R16, rec.ctypes.data, None, None, 3, "mode"),
        (tm.ctypes.data, F32, R16, rec.ctypes.data, None, occ.ctypes.data, la.MODE_ANY, "any-hit"),
        (tm.ctypes.data, F32, R16, rec.ctypes.data, t.ctypes.data, None, la.MODE_CLOSEST, "must be NULL"),
        (tm.ctypes.data, F32, R16, rec.ctypes.data + 8, None, None, la.MODE_CLOSEST, "aligned"),
        (tm.ctypes.data + 2, F32, R16, rec.ctypes.data, None, None, la.MODE_CLOSEST, "tmax not aligned"),
    ]
    for tp, rf, cf, r, tt, op, mode, msg in cases:
        rc = L.lh_accel_intersect_host_tmax(acc.h, n, o32.ctypes.data, d32.ctypes.data, tp, rf, cf, r, tt, None, None, op, mode)
        assert rc == -1 and msg in L.lh_last_error().decode(), (msg, L.lh_last_error())
    assert np.all(rec == FILL) and np.all(t == 0.25) and np.all(occ == 0x33)
    # device form
    d_o = cu(o32); d_d = cu(d32)
    d_tm = torch.ones(n + 1, dtype=torch.float32, device="cuda")
    d_rec = torch.full((n + 1, 4), FILL, dtype=torch.int32, device="cuda")
    d_t = torch.full((n,), 0.25, dtype=torch.float64, device="cuda")
    d_occ = torch.full((n,), 0x33, dtype=torch.uint8, device="cuda")
    d_idx = torch.arange(0, n, dtype=torch.int32, device="cuda")
    base, TM, IX = d_rec.data_ptr(), d_tm.data_ptr(), d_idx.data_ptr()
    dcases = [
        (n, TM, 2, R64, base, None, None, la.MODE_CLOSEST, None, 0, None, "ray format"),
        (n, TM, F32, 2, base, None, None, la.MODE_CLOSEST, None, 0, None, "record format"),
        (n, TM, F32, R16, base, None, None, 3, None, 0, None, "mode"),
        (n, TM, F32, R16, base, None, d_occ.data_ptr(), la.MODE_ANY, None, 0, None, "any-hit"),
        (n, TM, F32, R16, base, d_t.data_ptr(), None, la.MODE_CLOSEST, None, 0, None, "must be NULL"),
        (n, TM, F32, R16, base + 4, None, None, la.MODE_CLOSEST, None, 0, None, "aligned"),
        (n, TM + 2, F32, R16, base, None, None, la.MODE_CLOSEST, None, 0, None, "tmax not aligned"),
        (n, TM + 2, F32, R16, base, None, None, la.MODE_CLOSEST, IX, n, None, "tmax not aligned"),
        ((1 << 30) + 1, TM, F32, R16, base, None, None, la.MODE_CLOSEST, IX, n, None, "2^30 rays"),
        (n, TM, F32, R16, base, None, None, la.MODE_CLOSEST, None, (1 << 30) + 1, None, "2^30"),
        (n, TM, F32, R16, base, None, None, la.MODE_CLOSEST, IX + 2, 4, None, "4-byte aligned"),
        (n, TM, F32, R16, base, None, None, la.MODE_CLOSEST, IX, n, IX + 1, "4-byte aligned"),
    ]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda x: C.c_void_p(x) if x else None
    for nn, tp, rf, cf, r, tt, op, mode, ip, ni, cp, msg in dcases:
        rc = L.lh_accel_intersect_device_tmax(acc.h, nn, d_o.data_ptr(), d_d.data_ptr(), vp(tp), rf, cf, vp(r), vp(tt), None, None, vp(op), mode,
                                              vp(ip), ni, vp(cp), s)
        assert rc == -1 and msg in L.lh_last_error().decode(), (msg, L.lh_last_error())
    torch.cuda.synchronize()
    assert bool((d_rec == FILL).all()) and bool((d_t == 0.25).all()) and bool((d_occ == 0x33).all())
    for r in (base, None):
        assert L.lh_accel_intersect_device_tmax(acc.h, 0, d_o.data_ptr(), d_d.data_ptr(), vp(TM), F32, R16, vp(r), None, None, None, None, la.MODE_CLOSEST,
                                                None, 0, None, s) == 0
        assert L.lh_accel_intersect_host_tmax(acc.h, 0, o32.ctypes.data, d32.ctypes.data, tm.ctypes.data, F32, R16, rec.ctypes.data if r else None,
                                              None, None, None, None, la.MODE_CLOSEST) == 0
    torch.cuda.synchronize()
    assert bool((d_rec == FILL).all())
    # the binding's own refusals
    with pytest.raises(ValueError):
        acc.intersect_device(d_o, d_d, tmax=d_tm[:n], variant=la.VARIANT_DIRECT)
    with pytest.raises(ValueError):
        acc.intersect_device(d_o, d_d, tmax=d_tm[:n].double())
    acc.close()
