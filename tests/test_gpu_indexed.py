"""Indexed ray batches with a device-resident count, and hit compaction (lh_accel_intersect_device_indexed / lh_accel_compact_device).

Two identities, checked bit for bit on every launch path:
  * the record of a LISTED ray is the record the full-batch call (intersect_device, pinned to the oracle by the other suites)
    writes for that ray, in that ray's slot;
  * the record of a ray that is NOT listed is what the caller's array held before the call -- a byte pattern, or the fix-up
    protocol's own flag words, which no kernel of an indexed launch may act on.
The calls go through HipAccel.intersect_device_indexed (what intersect_device(index=, count=) forwards to): the record arrays are
the test's own, pre-filled, and nothing synchronises behind the caller's back."""
import os

import numpy as np
import pytest

import lucille_amd as la
from lucille_amd import rib
from oracle import pyoracle as po
from tests.helpers import assert_hits_equal, load_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RIB_FILE = os.path.join(HERE, "golden", "rib", "ambient_occlusion.rib")
PRIM_RETRACE, PRIM_OVERFLOW, OCC_RETRACE, OCC_OVERFLOW = 0xFFFFFFFE, 0xFFFFFFFD, 2, 4      # lh_reftrace.h, lh_device.h
PAT32, PAT8, PATF = 0x5A5A5A5A, 0x5A, -12345.678
MODES = ("soa", "rec16", "any")
SMALL = 64                                                                                  # LH_SMALL_BATCH


def golden_scene(name):
    if name.startswith("fuzz_"):
        z = load_golden(name)
        return z["P"], z["idx"], z["org"], z["dr"]
    g = load_golden(name)
    return po.soup(int(g["ntri"]), int(g["nrays"]), float(g["half_extent"]), int(g["seed"]))


def grow_rays(org, dr, n, seed):
    """the golden's rays tiled to n, every copy after the first with its origin and direction perturbed (fixed seed)"""
    rng = np.random.default_rng(seed)
    m = org.shape[0]
    k = np.arange(n) % m
    o = np.ascontiguousarray(org[k], np.float64); d = np.ascontiguousarray(dr[k], np.float64)
    scale = np.abs(org).max() * 1e-3 + 1e-12
    o[m:] += rng.uniform(-scale, scale, (max(n - m, 0), 3))
    d[m:] += rng.uniform(-1e-3, 1e-3, (max(n - m, 0), 3)) * np.abs(d[m:]).max(axis=1, keepdims=True)
    return o, d


class Batch:
    """a committed scene, n device rays (fp64 and their fp32 twins) and the full-batch records of both, computed once"""

    def __init__(self, P, idx, org, dr, build="host"):
        import torch
        self.acc = la.HipAccel(0)
        if P is not None:
            self.acc.add_mesh(P, idx)
        self.acc.commit(build=build); self.acc.wait_exact()
        self.n = org.shape[0]
        self.rays = {"f64": (torch.from_numpy(org).cuda(), torch.from_numpy(dr).cuda())}
        self.rays["f32"] = tuple(x.to(torch.float32).contiguous() for x in self.rays["f64"])
        self.full = {}

    def expected(self, mode, fmt):
        """host copies of the full-batch call's records: any -> (occ,), soa -> (prim, t, u, v), rec16 -> (rec [n, 4],)"""
        import torch
        key = (mode, fmt)
        if key not in self.full:
            o, d = self.rays[fmt]
            if mode == "any":
                out = self.acc.intersect_device(o, d, mode=la.MODE_ANY)
            else:
                out = self.acc.intersect_device(o, d, records="rec16" if mode == "rec16" else "f64")
            torch.cuda.synchronize()
            self.full[key] = tuple(x.cpu().numpy() for x in out)
        return self.full[key]


def prefilled(n, mode, fill):
    """the caller's record arrays before the call: `pattern`, or the fix-up protocol's flag words in every slot"""
    import torch
    k = np.arange(n)
    if mode == "any":
        a = np.full(n, PAT8, np.uint8) if fill == "pattern" else np.where(k & 1, OCC_RETRACE, OCC_OVERFLOW).astype(np.uint8)
        return (torch.from_numpy(a).cuda(),)
    w = np.full(n, PAT32, np.uint32) if fill == "pattern" else np.where(k & 1, PRIM_RETRACE, PRIM_OVERFLOW).astype(np.uint32)
    if mode == "rec16":
        rec = np.full((n, 4), PAT32, np.uint32); rec[:, 0] = w
        return (torch.from_numpy(rec.view(np.int32)).cuda(),)
    return (torch.from_numpy(w.view(np.int32)).cuda(),) + tuple(torch.full((n,), PATF, dtype=torch.float64, device="cuda") for _ in range(3))


def run_and_check(b, mode, fmt, index, count, fill, what, traced=None):
    """one indexed call into pre-filled arrays; `traced`: how many list entries the count lets through (default: all)"""
    import torch
    o, d = b.rays[fmt]
    out = prefilled(b.n, mode, fill)
    before = tuple(x.cpu().numpy().copy() for x in out)
    it = None if index is None else torch.from_numpy(np.asarray(index, np.uint32).view(np.int32)).cuda()
    ct = None if count is None else (count if hasattr(count, "is_cuda") else torch.tensor([count], dtype=torch.int32, device="cuda"))
    got = b.acc.intersect_device_indexed(o, d, out=out, mode=la.MODE_ANY if mode == "any" else la.MODE_CLOSEST,
                                         records="rec16" if mode == "rec16" else "f64", index=it, count=ct)
    torch.cuda.synchronize()
    assert got is out
    lst = np.arange(b.n, dtype=np.int64) if index is None else np.asarray(index, np.uint32).astype(np.int64)
    if traced is not None:
        lst = lst[:traced]
    listed = np.zeros(b.n, bool); listed[lst[lst < b.n]] = True
    exp = b.expected(mode, fmt)
    for k, (g, e, w) in enumerate(zip(out, exp, before)):
        g = g.cpu().numpy()
        gb, eb, wb = (x.reshape(b.n, -1).view(np.uint8) for x in (g, e, w))
        bad = np.nonzero((gb[listed] != eb[listed]).any(1))[0]
        assert bad.size == 0, "%s: array %d: %d of %d listed records differ from the full-batch call, first ray %d: %r != %r" % (
            what, k, bad.size, int(listed.sum()), np.nonzero(listed)[0][bad[0]], g[listed][bad[0]], e[listed][bad[0]])
        bad = np.nonzero((gb[~listed] != wb[~listed]).any(1))[0]
        assert bad.size == 0, "%s: array %d: %d of %d unlisted slots were written, first ray %d: %r" % (
            what, k, bad.size, int((~listed).sum()), np.nonzero(~listed)[0][bad[0]], g[~listed][bad[0]])
    return int(listed.sum())


def subset(n, size, seed):
    """`size` distinct ray ids in shuffled order"""
    return np.random.default_rng(seed).permutation(n)[:size].astype(np.uint32)


@pytest.fixture(scope="module")
def soup():
    P, idx, org, dr = golden_scene("soup_20k")
    o, d = grow_rays(org, dr, 100000, 11)
    b = Batch(P, idx, o, d)
    yield b
    b.acc.close()


@pytest.fixture(scope="module")
def fat():
    P, idx, org, dr = golden_scene("soup_3k_fat")
    o, d = grow_rays(org, dr, 100000, 12)
    b = Batch(P, idx, o, d)
    for mode in MODES:                      # the expectations come from the default launch parameters
        b.expected(mode, "f64")
    yield b
    b.acc.close()


# ---- list sizes on each launch path, unlisted slots untouched -----------------------------------------------------------

@pytest.mark.parametrize("fill", ["pattern", "flags"])
@pytest.mark.parametrize("size", [SMALL - 24, 5000, 70000])          # the small-batch kernel; no cooperative walk; past the 65 536 line
@pytest.mark.parametrize("mode", MODES)
def test_listed_records_equal_the_full_batch_and_the_rest_is_untouched(soup, mode, size, fill):
    nl = run_and_check(soup, mode, "f64", subset(soup.n, size, size), None, fill, "%s, %d listed, %s" % (mode, size, fill))
    assert nl == size


@pytest.mark.parametrize("size", [SMALL, 5000])
@pytest.mark.parametrize("mode", MODES)
def test_fp32_rays(soup, mode, size):
    run_and_check(soup, mode, "f32", subset(soup.n, size, 3 * size), None, "pattern", "fp32 rays, %s, %d listed" % (mode, size))


@pytest.mark.parametrize("mode", MODES)
def test_identity_list(soup, mode):
    import torch
    run_and_check(soup, mode, "f64", None, None, "pattern", "identity list, all rays, " + mode)
    run_and_check(soup, mode, "f64", None, 3001, "flags", "identity list, count 3001, " + mode, traced=3001)
    # through intersect_device itself: the listed slots are the full-batch call's (closest hit into a fresh `out`, whose other slots
    # are unspecified; any hit into zeros)
    o, d = soup.rays["f64"]
    lst = subset(soup.n, 777, 5)
    out = soup.acc.intersect_device(o, d, out=(torch.zeros(soup.n, dtype=torch.uint8, device="cuda"),) if mode == "any" else None, mode=la.MODE_ANY if mode == "any" else la.MODE_CLOSEST, records="rec16" if mode == "rec16" else "f64",
                                    index=torch.from_numpy(lst.view(np.int32)).cuda())
    torch.cuda.synchronize()
    for g, e in zip(out, soup.expected(mode, "f64")):
        assert np.array_equal(g.cpu().numpy()[lst], e[lst])


# ---- the count -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [SMALL - 24, 5000, 70000])
@pytest.mark.parametrize("mode", MODES)
def test_count_smaller_larger_and_zero(soup, mode, size):
    lst = subset(soup.n, size, 7 + size)
    for count, traced in ((size // 3, size // 3), (size + 12345, size), (0, 0)):
        nl = run_and_check(soup, mode, "f64", lst, count, "flags", "%s, %d listed, count %d" % (mode, size, count), traced=traced)
        assert nl == traced


@pytest.mark.parametrize("mode", MODES)
def test_count_written_by_the_preceding_work_on_the_stream(soup, mode):
    """the count is what a torch kernel enqueued just before the call leaves in the tensor: nothing synchronises in between"""
    import torch
    lst = subset(soup.n, 9000, 99)
    torch.cuda.synchronize()
    flags = torch.zeros(9000, dtype=torch.int32, device="cuda"); flags[:4321] = 1
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.sum(flags, dim=0, keepdim=True, dtype=torch.int32, out=count)          # enqueued, not waited for
    run_and_check(soup, mode, "f64", lst, count, "pattern", "count from a preceding kernel, " + mode, traced=4321)


# ---- shuffled lists, duplicates, ids beyond the batch ---------------------------------------------------------------------

@pytest.mark.parametrize("size", [SMALL - 24, 5000, 70000])
@pytest.mark.parametrize("mode", MODES)
def test_duplicates_and_ids_beyond_the_batch(soup, mode, size):
    rng = np.random.default_rng(size)
    lst = subset(soup.n, size, 21)
    dup = lst.copy(); dup[rng.integers(0, size, size // 2)] = lst[rng.integers(0, size, size // 2)]       # about a third of the entries repeat an id
    run_and_check(soup, mode, "f64", dup, None, "pattern", "%s, %d entries with duplicates" % (mode, size))
    far = lst.copy(); far[::3] = soup.n + np.arange(far[::3].size, dtype=np.uint32); far[1::7] = 0xFFFFFFFF
    far[-1] = soup.n
    run_and_check(soup, mode, "f64", far, None, "flags", "%s, %d entries, a third beyond the batch" % (mode, size))
    gap = lst.copy(); gap[size // 8:size // 2] = 0xFFFFFFFF              # whole waves' worth of entries in a row to skip, valid ids behind them
    nl = run_and_check(soup, mode, "f64", gap, None, "pattern", "%s, %d entries, a run of them beyond the batch" % (mode, size))
    assert nl == size - (size // 2 - size // 8)


# ---- forced slow paths: stack overflow, the cooperative walk, k_fixups ------------------------------------------------------

@pytest.mark.parametrize("knobs", [{"stack_cap": 8}, {"dump_budget": 16}, {"stack_cap": 8, "dump_budget": 16}])
@pytest.mark.parametrize("mode", MODES)
def test_forced_slow_paths(fat, mode, knobs):
    """a capped LDS stack (rays leave for the overflow walk / the cooperative walk) and a tiny visit budget (most rays go through
    the fix-up queue): the listed records are still the full-batch call's, the unlisted flag words are still there"""
    try:
        for k, v in knobs.items():
            fat.acc.set_param(k, v)
        for size in (5000, 70000):
            lst = subset(fat.n, size, 31 + size)
            run_and_check(fat, mode, "f64", lst, None, "flags", "%s, %r, %d listed" % (mode, knobs, size))
        run_and_check(fat, mode, "f64", subset(fat.n, 30000, 4), 20000, "pattern", "%s, %r, count 20000 of 30000" % (mode, knobs), traced=20000)
    finally:
        fat.acc.set_param("stack_cap", 0); fat.acc.set_param("dump_budget", 2048)


@pytest.mark.parametrize("mode", MODES)
def test_wide8(fat, mode):
    try:
        fat.acc.set_param("wide8", 1)
        for size in (5000, 70000):
            run_and_check(fat, mode, "f64", subset(fat.n, size, 41 + size), None, "flags", "wide8, %s, %d listed" % (mode, size))
    finally:
        fat.acc.set_param("wide8", -1)


# ---- the reference-walk re-trace (fragile hits), other scenes ----------------------------------------------------------------

@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("name", ["fuzz_r06_f661_359", "fuzz_r06_f662_99"])
def test_retraced_rays(name, build):
    P, idx, org, dr = golden_scene(name)
    o, d = grow_rays(org, dr, 6000, 13)
    b = Batch(P, idx, o, d, build=build)
    try:
        m = org.shape[0]
        first = np.arange(min(m, SMALL - 4), dtype=np.uint32)              # the golden's own rays, through the small-batch kernel
        for mode in MODES:
            run_and_check(b, mode, "f64", first, None, "flags", "%s (%s tree), %s, the golden's first rays" % (name, build, mode))
            run_and_check(b, mode, "f64", np.concatenate([first, first]), None, "pattern", "%s (%s tree), %s, twice" % (name, build, mode))
            run_and_check(b, mode, "f64", subset(b.n, 3000, 17), None, "flags", "%s (%s tree), %s, 3000 listed" % (name, build, mode))
            run_and_check(b, mode, "f32", subset(b.n, 3000, 18), 2500, "pattern", "%s (%s tree), %s, fp32, count" % (name, build, mode), traced=2500)
    finally:
        b.acc.close()


def test_listed_records_equal_the_oracle():
    P, idx, org, dr = golden_scene("soup_3k_fat")
    o, d = grow_rays(org, dr, 4000, 14)
    b = Batch(P, idx, o, d)
    try:
        import torch
        lst = subset(b.n, 1500, 19)
        out = prefilled(b.n, "soa", "pattern")
        b.acc.intersect_device_indexed(*b.rays["f64"], out=out, index=torch.from_numpy(lst.view(np.int32)).cuda())
        torch.cuda.synchronize()
        orc = po.Oracle(); orc.add_mesh(P, idx); orc.build()
        exp = orc.intersect(o[lst], d[lst])
        got = tuple(x.cpu().numpy()[lst] for x in out)
        assert_hits_equal((got[0].view(np.uint32),) + got[1:], exp, "indexed launch against the oracle")
    finally:
        b.acc.close()


def test_rib_scene_camera_rays():
    import torch
    sc = rib.RibScene(RIB_FILE)
    acc = la.HipAccel(0); sc.add_to(acc); acc.commit()
    try:
        cam = la.Camera.make(96, 96, sc.camera.flength, list(sc.camera.cam2world), sc.camera.rh)
        org, dr = acc.primary_rays(cam, 0, 0, 96, 96, 1)
        torch.cuda.synchronize()
        b = Batch.__new__(Batch)
        b.acc, b.n, b.full = acc, org.shape[0], {}
        b.rays = {"f64": (org.contiguous(), dr.contiguous())}
        for mode in MODES:
            run_and_check(b, mode, "f64", subset(b.n, 4000, 23), None, "flags", "RIB scene, " + mode)
    finally:
        acc.close()


@pytest.mark.parametrize("mode", MODES)
def test_empty_scene(mode):
    rng = np.random.default_rng(3)
    o = rng.uniform(-1, 1, (3000, 3)); d = rng.uniform(-1, 1, (3000, 3))
    b = Batch(None, None, o, d)
    try:
        run_and_check(b, mode, "f64", subset(b.n, 1000, 29), None, "flags", "empty scene, " + mode)
        run_and_check(b, mode, "f64", subset(b.n, 1000, 30), 10, "pattern", "empty scene, count, " + mode, traced=10)
        exp = b.expected(mode, "f64")
        assert (exp[0] == 0).all() if mode == "any" else (exp[0].reshape(b.n, -1)[:, 0].view(np.uint32) == po.MISS).all()
    finally:
        b.acc.close()


def test_device_built_scene():
    P, idx, org, dr = golden_scene("soup_20k")
    o, d = grow_rays(org, dr, 80000, 15)
    b = Batch(P, idx, o, d, build="device")
    try:
        for mode in MODES:
            run_and_check(b, mode, "f64", subset(b.n, 70000, 37), 66000, "flags", "device-built tree, " + mode, traced=66000)
            run_and_check(b, mode, "f64", subset(b.n, 50, 38), None, "pattern", "device-built tree, small, " + mode)
    finally:
        b.acc.close()


def test_statistics_count_the_traced_rays(soup):
    import torch
    far = subset(soup.n, 5000, 43); far[::5] = soup.n + 7                      # 1000 entries beyond the batch
    acc = soup.acc
    acc.trace_statistics(True)
    try:
        acc.statistics(clear=True)
        run_and_check(soup, "soa", "f64", far, 4000, "pattern", "statistics on", traced=4000)
        s = acc.statistics(clear=True)
        assert s["rays"] == 4000 - 800 and s["hits"] == 0, s                    # an unbounded indexed call counts no hits: its records stay on the device
        run_and_check(soup, "any", "f64", subset(soup.n, 40, 44), None, "pattern", "statistics on, small")
        s = acc.statistics(clear=True)
        assert s["rays"] == 40 and s["hits"] == 0, s
    finally:
        acc.trace_statistics(False)
    torch.cuda.synchronize()


# ---- compaction ------------------------------------------------------------------------------------------------------------

def records_for(n, kind, p_sel, seed):
    """synthetic records: a prim array (or rec16 array) with misses, or any-hit bytes; p_sel: the share that hits / is occluded"""
    rng = np.random.default_rng(seed)
    hit = rng.random(n) < p_sel if 0.0 < p_sel < 1.0 else np.full(n, p_sel >= 1.0)
    if kind == "occ":
        return hit.astype(np.uint8), hit
    prim = np.where(hit, rng.integers(0, 1 << 20, n), 0xFFFFFFFF).astype(np.uint32)
    if kind == "rec16":
        rec = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32); rec[:, 0] = prim
        return rec.view(np.int32), hit
    return prim.view(np.int32), hit


SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4 * 2048 + 1, 200001]


@pytest.mark.parametrize("kind", ["prim", "rec16", "occ"])
@pytest.mark.parametrize("n", SIZES)
def test_compact_equals_nonzero(n, kind):
    import torch
    sels = (la.SELECT_OCCLUDED, la.SELECT_UNOCCLUDED) if kind == "occ" else (la.SELECT_HIT, la.SELECT_MISS)
    rng = np.random.default_rng(n)
    for p_sel in (0.4, 1.0, 0.0):                                              # mixed, all hits, no hit
        rec, hit = records_for(n, kind, p_sel, n + 1)
        r = torch.from_numpy(rec).cuda()
        for sel in sels:
            keep = hit if sel in (la.SELECT_HIT, la.SELECT_OCCLUDED) else ~hit
            idx, cnt = la.compact(r, sel)
            torch.cuda.synchronize()
            exp = np.nonzero(keep)[0]
            c = int(cnt.item())
            assert c == exp.size, (n, kind, sel, p_sel, c, exp.size)
            assert np.array_equal(idx.cpu().numpy()[:c], exp), (n, kind, sel, p_sel)          # the order, not just the set
            # a given list: shuffled, with repeats and ids beyond the records, cut by a count
            m = max(1, (3 * n) // 2)
            lst = rng.integers(0, n + max(1, n // 8), m).astype(np.uint32)
            count = (2 * m) // 3 + 1
            li = torch.from_numpy(lst.view(np.int32)).cuda()
            idx2, cnt2 = la.compact(r, sel, index=li, count=torch.tensor([count], dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            cand = lst[:min(count, m)].astype(np.int64)
            cand = cand[cand < n]
            exp2 = cand[keep[cand]]
            c2 = int(cnt2.item())
            assert c2 == exp2.size and np.array_equal(idx2.cpu().numpy()[:c2].view(np.uint32), exp2), (n, kind, sel, p_sel, "given list")
            idx3, cnt3 = la.compact(r, sel, count=torch.tensor([n // 2], dtype=torch.int32, device="cuda"))       # the identity list, cut
            torch.cuda.synchronize()
            exp3 = np.nonzero(keep[:n // 2])[0]
            assert int(cnt3.item()) == exp3.size and np.array_equal(idx3.cpu().numpy()[:exp3.size], exp3), (n, kind, sel, p_sel, "count")


def test_compact_refuses_outputs_that_alias_the_input_list():
    """both passes read the input list and count while the outputs are written: in-place compaction is refused, nothing is written;
    two buffers in turn compact a list again"""
    import torch
    rec, hit = records_for(5000, "prim", 0.5, 77)
    r = torch.from_numpy(rec).cuda()
    idx, cnt = la.compact(r, la.SELECT_HIT)
    torch.cuda.synchronize()
    before = (idx.clone(), cnt.clone())
    other_i, other_c = torch.empty_like(idx), torch.empty_like(cnt)
    for out in ((idx, other_c), (other_i, cnt), (idx, cnt)):
        with pytest.raises(la.LucilleHipError, match="alias|overlap"):
            la.compact(r, la.SELECT_MISS, index=idx, count=cnt, out=out)
    torch.cuda.synchronize()
    assert torch.equal(idx, before[0]) and torch.equal(cnt, before[1])
    r2 = r.clone(); r2[::2] = -1                                               # every second ray dies
    la.compact(r2, la.SELECT_HIT, index=idx, count=cnt, out=(other_i, other_c))
    torch.cuda.synchronize()
    exp = np.nonzero(hit & (np.arange(5000) % 2 == 1))[0]
    assert int(other_c.item()) == exp.size and np.array_equal(other_i.cpu().numpy()[:exp.size], exp)


def test_compact_of_traced_records(soup):
    import torch
    for mode, sels in (("soa", (la.SELECT_HIT, la.SELECT_MISS)), ("rec16", (la.SELECT_HIT, la.SELECT_MISS)), ("any", (la.SELECT_OCCLUDED, la.SELECT_UNOCCLUDED))):
        exp = soup.expected(mode, "f64")[0]
        hit = exp != 0 if mode == "any" else exp.reshape(soup.n, -1)[:, 0].view(np.uint32) != po.MISS
        assert 0 < hit.sum() < soup.n
        r = torch.from_numpy(exp).cuda()
        for sel, keep in zip(sels, (hit, ~hit)):
            idx, cnt = la.compact(r, sel)
            torch.cuda.synchronize()
            c = int(cnt.item())
            assert np.array_equal(idx.cpu().numpy()[:c], np.nonzero(keep)[0])


# ---- the round trip the feature exists for -----------------------------------------------------------------------------------

def test_closest_hit_compact_shadow_rays_without_a_host_read(soup):
    """closest hit over all rays -> compact(HIT) -> any-hit of a second ray set for the rays that hit, listed by the compaction's
    output and count: one stream, no host read, one synchronisation at the end; equal to gather / trace / scatter done with torch"""
    import torch
    acc, n = soup.acc, soup.n
    o, d = soup.rays["f64"]
    rng = np.random.default_rng(51)
    o2 = torch.from_numpy(np.ascontiguousarray(o.cpu().numpy() + rng.uniform(-1e-3, 1e-3, (n, 3)))).cuda()
    d2 = torch.from_numpy(np.ascontiguousarray(-d.cpu().numpy()[:, ::-1])).cuda()
    shadow = torch.full((n,), PAT8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rec = acc.intersect_device_indexed(o, d, out=prefilled(n, "soa", "pattern"))           # the identity list: every ray
        idx, cnt = la.compact(rec[0], la.SELECT_HIT)
        acc.intersect_device_indexed(o2, d2, out=(shadow,), mode=la.MODE_ANY, index=idx, count=cnt)
    s.synchronize()
    # today's way
    prim = soup.expected("soa", "f64")[0].view(np.uint32)
    for g, e in zip(rec, soup.expected("soa", "f64")):
        assert np.array_equal(g.cpu().numpy(), e)
    hits = torch.from_numpy(np.nonzero(prim != po.MISS)[0]).cuda()
    assert int(cnt.item()) == hits.numel() and torch.equal(idx[:hits.numel()].long(), hits)
    occ = acc.intersect_device(o2.index_select(0, hits).contiguous(), d2.index_select(0, hits).contiguous(), mode=la.MODE_ANY)[0]
    exp = torch.full((n,), PAT8, dtype=torch.uint8, device="cuda")
    exp.index_copy_(0, hits, occ)
    torch.cuda.synchronize()
    assert torch.equal(shadow, exp)
    assert 0 < int((exp == 1).sum()) and 0 < int((exp == 0).sum()) and 0 < int((exp == PAT8).sum())
