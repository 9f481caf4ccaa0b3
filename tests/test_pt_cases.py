"""No GPU: the inputs and the restatements tests/test_gpu_pt_edges.py compares the device's path tracer with (tests/pt_cases.py).

  - the cases reach the branches they are for -- a condition on the INPUTS, read off the oracle's counters (lo_render_pt_detail), never off
    the product.  A case that misses the bar is a case to change, not a bar to lower;
  - pt_fix restated in float32 against the exact integer floor(r x 2^32);
  - lh_div restated in integers against n // d;
  - the pixel model (integer sums of the oracle's per-path radiances) against the oracle's own fp32 sums."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import pt_cases as pc
from tests.test_gpu_pt_oracle import close              # the tolerance the GPU parity tests have always used (importing needs no GPU)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_branches_it_is_for():
    total = dict.fromkeys(po.PT_COUNTERS, 0)
    oracles = {}
    short = {"diffuse": "D", "mirror": "S", "refracted": "T", "tir": "tir", "back": "back", "interior": "int", "axis0": "ax0", "axis1": "ax1",
             "axis2": "ax2", "flat_unnormalised": "flat", "normals": "nrm", "colours": "col", "miss_first": "miss0", "miss_later": "miss+",
             "roulette": "rr", "limit": "lim"}
    print("\n%-36s %2s %7s " % ("case", "fl", "paths") + " ".join("%6s" % short[k] for k in po.PT_COUNTERS))
    for case in pc.all_cases():
        o = oracles.setdefault(id(case["meshes"]), pc.oracle_of(case["meshes"]))
        for flags in case["flags"]:
            _, st, per, rad, cnt = pc.render_oracle(o, case, flags)
            print("%-36s %2d %7d " % (case["name"], flags, st["paths"]) + " ".join("%6d" % cnt[k] for k in po.PT_COUNTERS))
            for k in case["reach"]:
                assert cnt[k] >= pc.REACH_BAR, (case["name"], flags, k, cnt[k])
            # the counters are consistent with what the oracle always returned
            ends = cnt["miss_first"] + cnt["miss_later"] + cnt["roulette"] + cnt["limit"]
            vertices = cnt["diffuse"] + cnt["mirror"] + cnt["refracted"] + cnt["tir"]
            assert ends == st["paths"] and vertices + st["paths"] == st["rays"] == int(per.sum())
            assert cnt["axis0"] + cnt["axis1"] + cnt["axis2"] == cnt["diffuse"]
            assert rad.shape == (case["tile"][2] * case["tile"][3], case["spp"], 3)
            for k in po.PT_COUNTERS:
                total[k] += cnt[k]
    print("%-36s %2s %7s " % ("all cases", "", "") + " ".join("%6d" % total[k] for k in po.PT_COUNTERS))
    assert all(total[k] >= pc.REACH_BAR for k in po.PT_COUNTERS), total


def test_chains_are_alive_at_the_read_backs():
    """pt_tile reads a survivor count back after bounces 7 and 15 (depth & 7 == 7): the chain cases end on either side of each, with paths
    that reach the limit; on the lone plane no path is left long before the first"""
    o = pc.oracle_of(pc.slab_meshes())
    for case in pc.chain_cases()[:-1]:
        _, st, per, _, cnt = pc.render_oracle(o, case)
        assert st["max_depth_reached"] == int(per.max()) == case["max_vertices"] - 1
        assert int((per == case["max_vertices"] - 1).sum()) >= cnt["limit"] >= pc.REACH_BAR
        assert cnt["limit"] < 0.9 * st["paths"] or case["max_vertices"] <= 3     # ... and many end earlier: the counts shrink along the chain
    plane = pc.chain_cases()[-1]
    _, st, per, _, cnt = pc.render_oracle(pc.oracle_of(plane["meshes"]), plane)
    assert plane["max_vertices"] == 400 and st["max_depth_reached"] == 2 and cnt["limit"] == 0


def test_detail_changes_nothing_for_existing_callers():
    case = pc.branch_cases()[2]
    o = pc.oracle_of(case["meshes"])
    x0, y0, w, h = case["tile"]
    ocam = pc.cameras(case["cam"])[1]
    a = o.render_pt(ocam, x0, y0, w, h, 0, 4, 4, max_vertices=12, materials=case["mats"], seed=5)
    b = o.render_pt(ocam, x0, y0, w, h, 0, 4, 4, max_vertices=12, materials=case["mats"], seed=5, detail=True)
    assert len(a) == 3 and len(b) == 5
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    # a pixel's fp32 sum in sample order, from the per-path radiances: the oracle's own frame
    s = np.zeros((w * h, 3), np.float32)
    for k in range(4):
        s = s + b[3][:, k]
    assert np.array_equal((s * (np.float32(1.0) / np.float32(4))).reshape(h, w, 3)[::-1], a[0])


# ---- pt_fix ------------------------------------------------------------------------------------------------------------------------
def fix_inputs():
    rng = np.random.default_rng(5)
    n = 200000
    rnd = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-40, 21, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p2 = (2.0 ** np.arange(-40, 21)).astype(np.float32)
    near = np.concatenate([p2, np.nextafter(p2, np.float32(0)), np.nextafter(p2, np.float32(np.inf))])
    c = np.float32(262144.0)
    clamp = np.array([c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(np.inf))], np.float32)
    return np.concatenate([rnd, np.array([0.0, -0.0], np.float32), near, -near, clamp, -clamp]).astype(np.float32)


def exact_fix(r):
    """floor(r x 2^32) of the clamped float, in exact integers (a float32 x 2^32 is exact in fp64; floor of an fp64 is exact)"""
    r = np.clip(r.astype(np.float64), -262144.0, 262144.0)
    return np.array([int(x) for x in np.floor(r * 4294967296.0)], dtype=object)


def test_pt_fix_restated_against_exact_integers():
    r = fix_inputs()
    got = np.array([int(x) for x in pc.pt_fix_np(r)], dtype=object)
    exp = exact_fix(r)
    nonneg = r >= 0
    assert nonneg.sum() > 50000 and (got[nonneg] == exp[nonneg]).all()
    below = r <= -1                                          # r - floorf(r) is a multiple of ulp(r) below 1: exact
    assert below.sum() > 20000 and (got[below] == exp[below]).all()
    frac = (r > -1) & (r < 0)                                # r + 1 rounds to 24 bits in [0.5, 1): at most 2^-25, 2^7 quanta
    d = got[frac] - exp[frac]
    assert frac.sum() > 20000 and max(abs(int(x)) for x in d) <= 2 ** 7
    assert any(int(x) != 0 for x in d)                       # ... and the rounding really happens
    # the carry: floorf(-1e-10f) = -1, -1e-10f + 1 rounds to 1.0f
    assert int(pc.pt_fix_np(np.float32(-1.0e-10))) == 0
    assert int(pc.pt_fix_np(np.float32(-0.0))) == 0 and int(pc.pt_fix_np(np.float32(0.0))) == 0
    # the clamp
    assert int(pc.pt_fix_np(np.float32(1.0e9))) == 2 ** 18 * 2 ** 32 and int(pc.pt_fix_np(np.float32(-1.0e9))) == -(2 ** 18) * 2 ** 32
    # the word as the device holds it: two's complement in 64 bits
    assert int(pc.pt_fix_np(np.float32(-1.5)).astype(np.uint64)) == (1 << 64) - 3 * 2 ** 31


# ---- lh_div ------------------------------------------------------------------------------------------------------------------------
def test_lh_div_restated_against_integer_division():
    rng = np.random.default_rng(9)
    divisors = set(range(1, 4098))
    for k in range(1, 31):
        divisors.update(d for d in (2 ** k - 1, 2 ** k, 2 ** k + 1) if 1 <= d < 2 ** 30 + 2)
    top = 2 ** 30 - 1
    wrong_without_plus_one = 0
    for d in sorted(divisors):
        dv = pc.lh_div_make_py(d)
        assert dv[0] < 2 ** 32 and dv[1] < 32
        ns = {0, 1, d - 1, d, d + 1, top}
        for q in rng.integers(1, max(2, top // d + 1), 6):
            ns.update((int(q) * d - 1, int(q) * d))
        for n in ns:
            if 0 <= n <= top:
                assert pc.lh_div_py(n, dv) == n // d, (n, d)
        bad = pc.lh_div_make_py(d, plus_one=0)
        wrong_without_plus_one += any(pc.lh_div_py(n, bad) != n // d for n in ns if 0 <= n <= top)
    # the inputs tell the formula from its nearest wrong neighbour: m = floor(2^k / d) is wrong for every divisor that is no power of two
    assert wrong_without_plus_one >= len(divisors) - 32


# ---- the pixel model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [1, 2, 3])
def test_pixel_model_agrees_with_the_oracles_own_sums(which):
    """pixel_from_paths (integer sums, one conversion) against lo_render_pt's frame (fp32 sums in sample order): the same pixels within the
    tolerance the GPU parity tests have always used"""
    case = pc.branch_cases()[which]
    o = pc.oracle_of(case["meshes"])
    for env_map in (None, pc.random_probe()):
        img, st, _, rad, _ = pc.render_oracle(o, case, env_rgb=pc.PROBE_RGB, env_map=env_map)
        _, _, w, h = case["tile"]
        model = pc.frame_from_paths(rad, w, h, case["spp"])
        assert np.isfinite(img).all() and (img != 0).mean() > 0.2
        assert close(model, img).all(), float(np.abs(model - img).max())


def test_pixel_model_on_edge_radiances():
    """NaN and zero add nothing, a tiny negative carries to zero, the clamp holds per sample, and the order of the samples does not matter"""
    f = np.float32
    rad = np.array([[[1.0e9, -1.0e9, np.nan], [0.5, -1.0e-10, 0.25], [1.0e9, 0.0, -0.0], [-0.75, -0.75, np.nan]]], f)
    px = pc.pixel_from_paths(rad, 4)
    assert px.dtype == np.float32 and px.shape == (1, 3)
    assert px[0, 0] == f((2 * 262144.0 + 0.5 - 0.75) * 0.25) and px[0, 1] == f((-262144.0 - 0.75) * 0.25) and px[0, 2] == f(0.0625)
    assert np.array_equal(pc.pixel_from_paths(rad[:, ::-1], 4), px)
    assert np.array_equal(pc.pixel_from_paths(np.full((2, 3, 3), np.nan, f), 3), np.zeros((2, 3), f))
