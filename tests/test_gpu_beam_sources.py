"""Beam queries (lh_beam.hip: k_beam_visibility, k_beam_raster) over every way an accelerator gets lucille's own tree and its
scene box -- the host build, the device build, the background host thread, device meshes through the flatten kernel, a re-commit's
swap, a replica -- at the batch edges, and through the device entry points on a caller's stream.  Everything is compared exactly:
integer classes and statuses, every double of every raster plane, against the compiled reference's goldens where they exist and
against the oracle elsewhere."""
import functools

import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests.helpers import (RASTER_GOLDEN_CASES, beam_hits_box_np, beam_set_np, grazing_beams, load_golden, random_beams,
                           raster_beam_dirs, raster_camera, raster_case)
from tests.test_beam import golden_case
from tests.test_beam_raster import oracle_planes
from tests.test_gpu_recommit import dev_idx, dev_pos, sliver_soup

gpu = pytest.mark.gpu

SOURCES = ("a", "b", "c", "d", "e", "f", "g", "h")


# ---------------------------------------------------------------------------------------------------------------------
# scenes, however they are made
# ---------------------------------------------------------------------------------------------------------------------
def as_f32_rows(P):
    """the positions as fp32 rows of 16 bytes (xyz and a word nobody reads), and the doubles they widen to"""
    Q = np.full((P.shape[0], 4), 9.0, np.float32); Q[:, :3] = P.astype(np.float32)
    return Q, np.ascontiguousarray(Q[:, :3].astype(np.float64))


class Scene:
    """the accelerators of one source over `meshes` = [(positions [n,3] float64, indices)]: .accels answer the queries"""

    def __init__(self, source, meshes, monkeypatch=None):
        self.owner = None; self.accels = []
        if source in ("g", "h"):
            m = la.HipMulti([0, 0]); self.owner = m
            for P, I in meshes:
                m.add_mesh(P, I)
            m.commit(-2 if source == "h" else 0)
            self.accels = [m.accel(1)] if source == "g" else [m.accel(0), m.accel(1)]
            return
        acc = la.HipAccel(0); self.owner = acc; self.accels = [acc]
        if source in ("a", "b", "c"):
            for P, I in meshes:
                acc.add_mesh(P, I)
            if source == "a":
                acc.commit(build="host")
            elif source == "b":
                acc.commit(on_device=True)                       # beams are issued at once: no wait_exact
            else:
                monkeypatch.setenv("LH_REF_BUILD", "host")       # lucille's own tree by the background thread: the beam call joins it
                acc.commit(on_device=True)
                monkeypatch.delenv("LH_REF_BUILD")
        elif source == "d":
            for P, I in meshes:
                acc.add_mesh_device(dev_pos(P), dev_idx(I))
            acc.commit()
        elif source == "e":
            for P, I in meshes:
                Q = dev_pos(as_f32_rows(P)[0])
                assert Q.stride(0) * 4 == 16
                acc.add_mesh_device(Q, dev_idx(I))
            acc.commit()
        elif source == "f":
            acc.set_param("updatable", 1)
            for P, I in meshes:
                acc.add_mesh_device(dev_pos(np.ascontiguousarray(0.9 * P + 0.05)), dev_idx(I))
            acc.commit()
            for k, (P, I) in enumerate(meshes):
                acc.update_mesh_device(k, dev_pos(P))
            r = acc.recommit()
            assert r["rebuilt_trees"] == 1
        else:
            raise ValueError(source)

    def close(self):
        for a in self.accels:
            a.close()
        self.owner.close()


def oracle_of(meshes):
    o = po.Oracle()
    for P, I in meshes:
        o.add_mesh(P, I)
    o.build()
    return o


def widened(meshes):
    return [(as_f32_rows(P)[1], I) for P, I in meshes]


@functools.lru_cache(maxsize=None)
def vis_golden(name):
    return golden_case(name)


@functools.lru_cache(maxsize=None)
def vis_golden_f32(name):
    """what source e is compared with: the ORACLE on the doubles the fp32 positions widen to"""
    P, idx, cases = vis_golden(name)
    o = oracle_of(widened([(P, idx)]))
    return [o.beam_visibility(org, d) for org, d, _ in cases]


@functools.lru_cache(maxsize=None)
def raster_golden(k):
    c = raster_case(**RASTER_GOLDEN_CASES[k])
    g = load_golden("beam_raster")
    return c, g["rc%d" % k], g["t%d" % k]


@functools.lru_cache(maxsize=None)
def raster_golden_f32(k):
    c = dict(raster_golden(k)[0]); c["P"] = as_f32_rows(c["P"])[1]
    return oracle_planes(c)


def hip_raster(acc, c, **kw):
    return acc.beam_raster(c["org"], c["dirs"], c["corners"], c["width"], c["height"], c["frame"], c["eye"], c["fov"], **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 0. the helpers (CPU)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup3k():
    P, idx, _, _ = po.soup(3000, 1, 0.05, 77)
    return P, idx, oracle_of([(P, idx)])


def test_beam_set_np_refuses_what_the_oracle_refuses():
    P, idx, o = soup3k()
    refused = 0
    for k, spread in enumerate((0.0005, 0.02, 0.2)):
        org, d = random_beams(np.random.default_rng(40 + k), 2001, spread)
        b, ref = beam_set_np(org, d)
        assert np.array_equal(ref, o.beam_visibility(org, d) == -1)
        assert b.dtype == la.binding.BEAM_SET_DTYPE and b.dtype.itemsize == 232
        refused += int(ref.sum())
    assert refused > 100


def test_beams_that_miss_the_box_miss_the_scene():
    P, idx, o = soup3k()
    bmin, bmax = o.bbox()
    missed = 0
    rng = np.random.default_rng(60)
    for k, spread in enumerate((0.0005, 0.02, 0.2)):
        org, d = random_beams(np.random.default_rng(40 + k), 2001, spread)
        # the batch as it is (origins around the unit cube, aimed into it: nearly every beam meets the box), and moved aside
        for org in (org, org + rng.normal(size=org.shape)):
            b, ref = beam_set_np(org, d)
            miss = ~beam_hits_box_np(b, bmin, bmax) & ~ref
            assert (o.beam_visibility(org, d)[miss] == 0).all()
            missed += int(miss.sum())
    assert missed > 1000


def grazing_set(o, seed, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """64 pairs on the box of a soup that is the unit-cube soup moved by `shift` and scaled by `scale`"""
    rng = np.random.default_rng(seed)
    org, d = random_beams(rng, 400, 0.02)
    org = (org + np.asarray(shift)) * scale
    b, ref = beam_set_np(org, d)
    ok = np.nonzero(beam_hits_box_np(b, *o.bbox()) & ~ref)[0][:64]
    assert ok.size == 64
    c = d[ok].mean(axis=1)
    u = np.cross(c, rng.normal(size=c.shape)); u /= np.linalg.norm(u, axis=1, keepdims=True)      # sideways: a narrow beam moved far enough misses
    return grazing_beams(o, org[ok], d[ok], u)


def faces_seen(o, org, d, hits):
    """per face of the box: the beams whose answer flips when that face alone moves outwards by one ulp"""
    bmin, bmax = o.bbox()
    b, _ = beam_set_np(org, d)
    out = []
    for f in range(6):
        lo, hi = bmin.copy(), bmax.copy()
        if f < 3: lo[f] = np.nextafter(lo[f], -np.inf)
        else: hi[f - 3] = np.nextafter(hi[f - 3], np.inf)
        out.append(int((beam_hits_box_np(b, lo, hi) != hits).sum()))
    return out


@functools.lru_cache(maxsize=None)
def grazing_case():
    """-> [(meshes, oracle, org [128,3], dirs, hits)] for the 3 000-triangle soup and for the same soup moved and scaled"""
    P, idx, o = soup3k()
    shift = np.array([3.0, -2.0, 5.0])
    P2 = np.ascontiguousarray((P + shift) * 1000.0)
    o2 = oracle_of([(P2, idx)])
    return [([(P, idx)], o) + grazing_set(o, 3), ([(P2, idx)], o2) + grazing_set(o2, 4, 1000.0, shift)]


def test_grazing_beams_straddle_the_box_by_one_ulp():
    for meshes, o, org, d, hits in grazing_case():
        assert org.shape == (128, 3) and d.shape == (128, 4, 3)
        b, ref = beam_set_np(org, d)
        assert not ref.any()
        assert np.array_equal(beam_hits_box_np(b, *o.bbox()), hits)
        assert (hits[0::2] != hits[1::2]).all()
        assert np.array_equal(d[0::2], d[1::2])
        differs = org[0::2] != org[1::2]
        assert (differs.sum(axis=1) == 1).all()
        lo = np.minimum(org[0::2], org[1::2])[differs]; hi = np.maximum(org[0::2], org[1::2])[differs]
        assert np.array_equal(np.nextafter(lo, np.inf), hi)
        # the pairs see every face of the box: one ulp on any of the six numbers changes an answer
        assert min(faces_seen(o, org, d, hits)) >= 1, faces_seen(o, org, d, hits)
        # a beam that misses the box misses the scene
        assert (o.beam_visibility(org, d)[~hits] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 1. scene sources x the compiled reference's goldens
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", ["beams_300", "beams_2k"])
def test_visibility_of_every_source_equals_the_golden(name, source, monkeypatch):
    P, idx, cases = vis_golden(name)
    exp = vis_golden_f32(name) if source == "e" else [c[2] for c in cases]
    sc = Scene(source, [(P, idx)], monkeypatch)
    for acc in sc.accels:
        for (org, d, _), e in zip(cases, exp):
            assert np.array_equal(acc.beam_visibility(org, d), e)
    sc.close()


@gpu
@pytest.mark.parametrize("source", SOURCES)
def test_raster_of_every_source_equals_the_golden(source, monkeypatch):
    for k in range(len(RASTER_GOLDEN_CASES)):
        c, rc, t_exp = raster_golden(k)
        sc = Scene(source, [(c["P"], c["idx"])], monkeypatch)
        for acc in sc.accels:
            t, st, fl = hip_raster(acc, c)
            if source == "e":
                rc_o, t_o, fl_o = raster_golden_f32(k)
                assert np.array_equal(np.where(st == 1, 0, st), rc_o) and np.array_equal(t, t_o) and np.array_equal(fl, fl_o)
            else:
                assert np.array_equal(st, rc)
                assert np.array_equal(t, t_exp)                # every double of every plane
                assert not fl[:, :3].any()
        sc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. degenerate triangles stay in lucille's tree
# ---------------------------------------------------------------------------------------------------------------------
SLIVER_SPREADS = (0.0005, 0.02)


@functools.lru_cache(maxsize=None)
def sliver_case():
    """the sliver soup as two meshes of 1 000 triangles, plain (P) and degenerate (D), the two beam batches and the oracle's
    answers on both forms -- with the conditions that keep the comparison from turning vacuous"""
    P, D, idx, _, _ = sliver_soup()
    assert np.array_equal(idx, np.arange(6000, dtype=np.uint32))
    cut = lambda X: [(np.ascontiguousarray(X[:3000]), idx[:3000]), (np.ascontiguousarray(X[3000:]), idx[:3000])]
    mP, mD = cut(P), cut(D)
    oP, oD = oracle_of(mP), oracle_of(mD)
    batches = []
    for spread in SLIVER_SPREADS:
        org, d = random_beams(np.random.default_rng(1), 2001, spread)
        batches.append((org, d, oP.beam_visibility(org, d), oD.beam_visibility(org, d)))
    seen_p, seen_d = set(), set()
    for org, d, rp, rd in batches:
        assert (rp == -1).sum() <= 0.1 * rp.size and np.array_equal(rp == -1, rd == -1)
        seen_p |= set(rp.tolist()); seen_d |= set(rd.tolist())
    assert {0, 1, 2} <= seen_p and {1, 2} <= seen_d
    assert (batches[0][2] != batches[0][3]).sum() > batches[0][2].size // 2      # P and D differ for more than half the narrow beams
    return mP, mD, batches


def test_the_sliver_batches_tell_the_two_forms_apart():
    sliver_case()


@gpu
@pytest.mark.parametrize("source", ["a", "b", "d"])
def test_degenerate_triangles_answer_beams(source):
    mP, mD, batches = sliver_case()
    sc = Scene(source, mD)
    for org, d, rp, rd in batches:
        assert np.array_equal(sc.accels[0].beam_visibility(org, d), rd)
    sc.close()


@gpu
def test_beams_follow_the_recommit_into_the_degenerate_form_and_back():
    mP, mD, batches = sliver_case()
    acc = la.HipAccel(0); acc.set_param("updatable", 1)
    for X, I in mP:
        acc.add_mesh_device(dev_pos(X), dev_idx(I))
    acc.commit()

    def check(which, what):
        for b in batches:
            assert np.array_equal(acc.beam_visibility(b[0], b[1]), b[which]), what

    def stage(meshes):
        for k, (X, I) in enumerate(meshes):
            acc.update_mesh_device(k, dev_pos(X))

    check(2, "first commit")
    stage(mD)
    check(2, "staged, not re-committed")
    assert acc.recommit()["rebuilt_trees"] == 1
    check(3, "degenerate form")
    bad = mD[0][0].copy(); bad[int(mD[0][1][99]), 1] = np.nan
    acc.update_mesh_device(0, dev_pos(bad))
    with pytest.raises(la.LucilleHipError, match="lh_accel_recommit: a vertex coordinate is NaN, infinite or beyond 1e30"):
        acc.recommit()
    check(3, "after the refused re-commit")
    stage(mP)
    assert acc.recommit()["rebuilt_trees"] == 1
    check(2, "back to the plain form")
    acc.close()


@functools.lru_cache(maxsize=None)
def degenerate_raster_case():
    c = dict(raster_case(seed=31, ntri=200, width=48, height=48, nbeams=10))
    T = c["P"].reshape(-1, 3, 3).copy()
    T[0:8:4, 1] = T[0:8:4, 0]; T[1:8:4, 2] = T[1:8:4, 0]; T[2:8:4, 2] = T[2:8:4, 1]       # zero area: two vertices equal
    T[8:14, 2] = T[8:14, 0] + 2.0 * (T[8:14, 1] - T[8:14, 0])                             # collinear
    T[14:20] = T[100]                                                                     # duplicates
    c["P"] = np.ascontiguousarray(T.reshape(-1, 3))
    return c, oracle_planes(c)


@gpu
@pytest.mark.parametrize("source", ["a", "b", "d"])
def test_degenerate_triangles_in_the_raster(source):
    c, (rc, t_exp, fl_exp) = degenerate_raster_case()
    assert (rc == 0).all() and (t_exp != 0).sum() > 1000
    sc = Scene(source, [(c["P"], c["idx"])])
    t, st, fl = hip_raster(sc.accels[0], c)
    assert np.array_equal(np.where(st == 1, 0, st), rc)
    assert np.array_equal(t, t_exp)
    assert np.array_equal(fl, fl_exp)
    sc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. beams that graze the scene box
# ---------------------------------------------------------------------------------------------------------------------
def grazing_window(meshes):
    """a 16 x 16 window in front of the soup (the beams' own origins are the grazing ones)"""
    allp = np.concatenate([m[0] for m in meshes]); lo, hi = allp.min(axis=0), allp.max(axis=0)
    eye = 0.5 * (lo + hi) - np.array([0.0, 0.0, 2.0 * (hi[2] - lo[2])])
    corner, frame = raster_camera(eye, eye + np.array([0.0, 0.0, 1.0]), [0.0, 1.0, 0.0], 16, 16, 45.0)
    return dict(width=16, height=16, frame=frame, eye=eye, fov=45.0, corner=corner)


@functools.lru_cache(maxsize=None)
def grazing_expected(k):
    meshes, o, org, d, hits = grazing_case()[k]
    w = grazing_window(meshes)
    c = dict(w, P=None, org=org, dirs=d, corners=np.repeat(w["corner"][None], org.shape[0], 0))
    st = np.where(hits, 0, 1).astype(np.int32)
    t = np.full((org.shape[0], 16, 16), 7.0)
    for i in np.nonzero(hits)[0]:
        rc, ti, _ = o.beam_raster(org[i], d[i], 16, 16, w["frame"], w["corner"], w["eye"], w["fov"])
        assert rc == 0
        t[i] = ti
    return c, st, t, o.beam_visibility(org, d)


@gpu
@pytest.mark.parametrize("k", [0, 1], ids=["unit", "moved-and-scaled"])
def test_beams_that_graze_the_scene_box(k):
    meshes = grazing_case()[k][0]
    c, st_exp, t_exp, vis_exp = grazing_expected(k)
    assert (st_exp == 1).sum() == 64 and (vis_exp[st_exp == 1] == 0).all()
    init = np.full(t_exp.shape, 7.0)
    first = None
    for source in ("a", "b", "d", "f", "g", "h"):             # (g, h: a replica's box, beyond the four sources that make one)
        sc = Scene(source, meshes)
        got = [hip_raster(acc, c, t_init=init)[:2] + (acc.beam_visibility(c["org"], c["dirs"]),) for acc in sc.accels]
        sc.close()
        for t, st, vis in got:
            bad = np.nonzero(st != st_exp)[0]
            assert bad.size == 0, "source %s: the scene box differs from the reference's: statuses of beams %s" % (source, bad[:8])
            assert np.array_equal(t, t_exp), "source %s" % source
            assert np.array_equal(vis, vis_exp), "source %s" % source
            if first is None:
                first = (t.tobytes(), st.tobytes())
            assert (t.tobytes(), st.tobytes()) == first, "source %s against source a" % source


# ---------------------------------------------------------------------------------------------------------------------
# 4. batch edges
# ---------------------------------------------------------------------------------------------------------------------
EDGE_COUNTS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """257 beams over a 300-triangle soup, ordered so that beam 0 is refused, beam 4 misses and beam 64 hits partially: the
    last beam of the batches of 1, 5 and 65 -- the one group of 16 lanes that works beside dead ones -- takes each way out"""
    P, idx, _, _ = po.soup(300, 1, 0.05, 4300)
    o = oracle_of([(P, idx)])
    org, d = random_beams(np.random.default_rng(9), 1200, 0.002)
    r = o.beam_visibility(org, d)
    order = list(range(257))
    for at, cls in ((0, -1), (4, 0), (64, 2)):
        j = next(i for i in range(257, 1200) if r[i] == cls)
        order[at] = j; r[j] = 99                              # taken
    org, d = np.ascontiguousarray(org[order]), np.ascontiguousarray(d[order])
    exp = o.beam_visibility(org, d)
    assert (exp[0], exp[4], exp[64]) == (-1, 0, 2) and set(exp.tolist()) == {-1, 0, 1, 2}
    return P, idx, org, d, exp


@gpu
@pytest.mark.parametrize("source", ["a", "d"])
def test_visibility_batches_that_end_inside_a_wave(source):
    P, idx, org, d, exp = edge_batch()
    sc = Scene(source, [(P, idx)])
    for n in EDGE_COUNTS:
        got = sc.accels[0].beam_visibility(org[:n], d[:n])
        assert np.array_equal(got, exp[:n]), "%d beams" % n
    sc.close()


# window, where the last beam's 3 x 3 pixels go
EDGE_WINDOWS = (((8, 8), (5, 5)),           # narrower than a wave
                ((66, 10), (63, 0)),        # one column past a wave: columns 63 .. 65 are lanes 63, 0 and 1
                ((10, 66), (7, 33)),        # tall
                ((66, 66), (63, 63)))       # one column past a wave, square: the beam's whole footprint is written
# (the 66-wide windows look through 30 degrees, the others through 45: the last columns still face the scene)


@functools.lru_cache(maxsize=None)
def edge_raster_cases():
    """1 and 3 beams per window.  raster_case's beams are a few pixels wide and land anywhere, so the LAST beam of every case is
    put on the window's last columns.  A window that is not square keeps little: the reference scales a projected triangle's
    rows by height / 2 where its pixel rays are spaced for width / 2 (rb_rasterize_triangle in lh_beam.hip restates both), so
    the pixel box and the rays through it rarely meet -- there the cleared plane and the count of pixel tests cut at the
    window's edge (flags[0]) are most of what is compared, and the planes start as 7.0 to show the clearing."""
    out = []
    for seed, ((w, h), (s, t)) in enumerate(EDGE_WINDOWS):
        for n in (1, 3):
            c = dict(raster_case(seed=410 + seed, ntri=300, width=w, height=h, nbeams=n, fov=30.0 if w == 66 else 45.0))
            c["dirs"] = c["dirs"].copy()
            c["dirs"][n - 1] = raster_beam_dirs(c["corner"], c["frame"], 3, s, t)
            rc, tt, fl = oracle_planes(c)
            b, refused = beam_set_np(c["org"], c["dirs"])
            st = np.where(beam_hits_box_np(b, *oracle_of([(c["P"], c["idx"])]).bbox()), 0, 1).astype(np.int32)
            assert (rc == 0).all() and not refused.any() and st[n - 1] == 0
            tt[st == 1] = 7.0                                    # a beam beside the scene box: nothing done, the plane keeps its 7.0
            if w == h:
                assert not fl[:, :3].any()
                assert (tt[n - 1][t:t + 3, s:s + 3] != 0).all() and (tt[n - 1] != 0).sum() == 9 and st[n - 1] == 0       # the whole footprint, the last column with it
            out.append((c, (st, tt, fl)))
    return out


@gpu
@pytest.mark.parametrize("source", ["a", "d"])
def test_raster_windows_at_the_edges_of_a_wave(source):
    for c, (st_exp, t_exp, fl_exp) in edge_raster_cases():
        sc = Scene(source, [(c["P"], c["idx"])])
        t, st, fl = hip_raster(sc.accels[0], c, t_init=np.full(t_exp.shape, 7.0))
        sc.close()
        what = "%d x %d, %d beams" % (c["width"], c["height"], c["org"].shape[0])
        assert np.array_equal(st, st_exp), what
        assert np.array_equal(t, t_exp), what                 # traced: cleared to 0.0 and written
        assert np.array_equal(fl, fl_exp), what


# ---------------------------------------------------------------------------------------------------------------------
# 5. the _device entry points on a caller's stream
# ---------------------------------------------------------------------------------------------------------------------
GUARD32 = 0x5A5A5A5A
GUARD64 = 0x5A5A5A5A5A5A5A5A


@functools.lru_cache(maxsize=None)
def stream_batch():
    P, idx, o = soup3k()
    org, d = random_beams(np.random.default_rng(11), 2001, 0.002)
    exp = o.beam_visibility(org, d)
    assert {-1, 0, 1, 2} == set(exp.tolist())
    return org, d, exp


@gpu
@pytest.mark.parametrize("source", ["a", "d"])
def test_visibility_device_runs_in_the_callers_stream_order(source):
    import torch
    P, idx, o = soup3k()
    org, d, exp = stream_batch()
    n = org.shape[0]
    sc = Scene(source, [(P, idx)]); acc = sc.accels[0]
    h_org = torch.from_numpy(org).pin_memory(); h_d = torch.from_numpy(d).pin_memory()
    d_org = torch.zeros((n, 3), dtype=torch.float64, device="cuda"); d_d = torch.zeros((n, 4, 3), dtype=torch.float64, device="cuda")
    res = torch.full((n + 16,), GUARD32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    busy = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(s):
        for k in range(8):
            busy.fill_(k)                                   # the stream is kept busy: the copies below start late
        d_org.copy_(h_org, non_blocking=True); d_d.copy_(h_d, non_blocking=True)
        acc.beam_visibility_device(d_org, d_d, res, stream=s)       # behind the copies: a launch on another stream would read zeros
    s.synchronize()
    got = res.cpu().numpy()
    assert np.array_equal(got[:n], exp)
    assert (got[n:] == GUARD32).all()
    # the host form afterwards, through the accelerator's own stream and staging: the same answer
    assert np.array_equal(acc.beam_visibility(org, d), exp)
    sc.close()


@functools.lru_cache(maxsize=None)
def stream_raster_case():
    """eight beams over a 3 000-triangle scene, a beam ri_beam_set refuses and a beam that starts far to the side"""
    c = dict(raster_case(seed=520, ntri=3000, width=32, height=32, nbeams=8, tri_size=0.2))
    straddle = raster_beam_dirs(c["corner"], c["frame"], 16, 8, 8)
    c["dirs"] = np.concatenate([c["dirs"], straddle[None], c["dirs"][:1]])
    far = c["eye"].copy(); far[0] += 100.0
    c["org"] = np.concatenate([c["org"], c["eye"][None], far[None]])
    c["corners"] = np.repeat(c["corner"][None], 10, 0)
    rc, t, fl = oracle_planes(c)
    o = oracle_of([(c["P"], c["idx"])])
    b, refused = beam_set_np(c["org"], c["dirs"])
    st = np.where(refused, -1, np.where(beam_hits_box_np(b, *o.bbox()), 0, 1)).astype(np.int32)
    assert st.tolist() == [0] * 8 + [-1, 1] and np.array_equal(np.where(st == 1, 0, st), rc)
    t[st != 0] = 7.0                                         # untraced planes keep what the caller put there
    assert not fl[st != 0].any() and (t[:8] != 7.0).all() and (t[:8] != 0).sum() > 500
    return c, st, t, fl


@gpu
@pytest.mark.parametrize("source", ["a", "d"])
@pytest.mark.parametrize("with_flags", [True, False])
def test_raster_device_on_the_callers_buffers(source, with_flags):
    import torch
    c, st_exp, t_exp, fl_exp = stream_raster_case()
    n = 10; px = 32 * 32
    sc = Scene(source, [(c["P"], c["idx"])]); acc = sc.accels[0]
    pin = lambda x: torch.from_numpy(np.ascontiguousarray(x)).pin_memory()
    h = [pin(c["org"]), pin(c["dirs"]), pin(c["corners"])]
    dev = [torch.zeros(x.shape, dtype=torch.float64, device="cuda") for x in h]
    d_t = torch.full((n * px + 64,), 7.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((n + 16,), GUARD32, dtype=torch.int32, device="cuda")
    d_fl = torch.full((4 * n + 16,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for x, y in zip(dev, h):
            x.copy_(y, non_blocking=True)
        acc.beam_raster_device(dev[0], dev[1], dev[2], 32, 32, c["frame"], c["eye"], c["fov"], d_t, d_st, d_fl if with_flags else None, stream=s)
    s.synchronize()
    t = d_t.cpu().numpy(); st = d_st.cpu().numpy(); fl = d_fl.cpu().numpy().view(np.uint64)
    assert np.array_equal(st[:n], st_exp) and (st[n:] == GUARD32).all()
    assert np.array_equal(t[:n * px].reshape(n, 32, 32), t_exp) and (t[n * px:] == 7.0).all()
    if with_flags:
        assert np.array_equal(fl[:4 * n].reshape(n, 4), fl_exp) and (fl[4 * n:] == GUARD64).all()
    else:
        assert (fl == GUARD64).all()
    sc.close()


@gpu
@pytest.mark.parametrize("source", ["a", "d"])
def test_preset_beams_answer_like_the_beams_they_were_set_from(source):
    P, idx, o = soup3k()
    org, d, exp = stream_batch()
    b, refused = beam_set_np(org, d)
    sc = Scene(source, [(P, idx)]); acc = sc.accels[0]
    got = acc.beam_visibility(org, d)
    assert np.array_equal(got, exp)
    assert np.array_equal(acc.beam_visibility_set(b[~refused]), got[~refused])
    sc.close()


@gpu
@pytest.mark.parametrize("scene", ["no mesh", "device mesh of nothing", "points"])
def test_beams_on_empty_scenes(scene):
    import torch
    org, d = random_beams(np.random.default_rng(12), 2001, 0.002)
    if scene == "points":
        # every triangle collapsed to a point: nothing is left in the traversal tree, lucille's own tree keeps 2 000 triangles a beam
        # "hits completely" (their determinant is 0: u = v = t = 0)
        mP, _, _ = sliver_case()
        mZ = [(np.ascontiguousarray(np.repeat(X.reshape(-1, 3, 3)[:, :1], 3, axis=1).reshape(-1, 3)), I) for X, I in mP]
        acc = la.HipAccel(0); acc.set_param("updatable", 1)
        for X, I in mP:
            acc.add_mesh_device(dev_pos(X), dev_idx(I))
        acc.commit()
        for k, (Z, I) in enumerate(mZ):
            acc.update_mesh_device(k, dev_pos(Z))
        r = acc.recommit()
        assert r["ntriangles"] == 2000
        exp = oracle_of(mZ).beam_visibility(org, d)
        assert (exp == 1).sum() > 100                        # not all zeros
    else:
        acc = la.HipAccel(0)
        if scene == "device mesh of nothing":
            acc.add_mesh_device(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), dev_idx(np.zeros(0, np.uint32)))
        acc.commit()
        exp = oracle_of([(np.zeros((0, 3)), np.zeros(0, np.uint32))]).beam_visibility(org, d)
        assert set(exp.tolist()) == {0, -1}
    assert np.array_equal(acc.beam_visibility(org, d), exp)
    acc.close()
