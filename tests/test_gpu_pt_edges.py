"""The wavefront path tracer at its edges, against oracle/lucille_oracle_pt.c path for path (cases: tests/pt_cases.py; that the cases reach
their branches is tests/test_pt_cases.py's business, on the oracle alone).

Every comparison asserts the statistics first -- paths, rays, longest path: a branch that goes the other way changes a ray count -- and then
the frame.  Under a CONSTANT environment (and under a light probe whose texels are all one float) nothing in a path goes through libm: the
cosine lobe is the same fp32 polynomial on both sides, the pixel sums are integers, so the frame rendered into a zeroed buffer is predicted
from the oracle's per-path radiances TO THE BIT (pt_cases.pixel_from_paths: pt_fix per sample, one conversion, x 1 / spp; with `out` zeroed
a contracted sum x inv + 0 is the same float as the uncontracted one).  Under the random light probe the probe's acos is libm's on one side
and the device's on the other: those frames compare by tests/test_gpu_pt_oracle.py's `close`, against the same prediction.

One input the oracle and the device agree on and a reader may not expect: under the default weights a refraction that turns into a total
internal reflection takes the MIRROR lobe's reflectance and weight (brdf, pathtrace.c:533-565), so glass with ks = 0 ("S1 glass plane")
carries 0 x (1 / 0) = NaN from there on.  pt_accumulate drops a NaN radiance; the prediction drops it too."""
import numpy as np
import pytest

import lucille_amd as la
from tests import pt_cases as pc
from tests.test_gpu_pt_oracle import close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    """meshes -> (committed accelerator, oracle), one of each per scene for the whole module"""
    made = {}

    def get(meshes):
        if id(meshes) not in made:
            made[id(meshes)] = (pc.accel_of(meshes), pc.oracle_of(meshes))
        return made[id(meshes)]
    yield get
    for acc, _ in made.values():
        acc.close()


def device_frame(acc, case, flags, env_rgb, env_map):
    """the case through render_pt_tile2 into a zeroed frame -> (float32 [h, w, 3], stats)"""
    for k, m in enumerate(case["mats"]):
        acc.set_material(k, pc.la_material(m))
    acc.set_environment(env_rgb, env_map)
    x0, y0, w, h = case["tile"]
    img, st = acc.render_pt_tile2(pc.cameras(case["cam"])[0], x0, y0, w, h, 0, case["spp"], case["spp"], max_vertices=case["max_vertices"],
                                  flags=flags, seed=case["seed"])
    return img.cpu().numpy(), st


def assert_frame(got, model, exact, what):
    if exact:
        bad = np.argwhere(got.view(np.uint32) != model.view(np.uint32))
        assert bad.shape[0] == 0, "%s: %d of %d channels differ, first (line, column, channel) %s: device %r, predicted %r" % (
            what, bad.shape[0], got.size, tuple(bad[0]), got[tuple(bad[0])], model[tuple(bad[0])])
    else:
        ok = close(got, model)
        assert ok.all(), (what, float(np.abs(got - model).max()), int((~ok).sum()))


def assert_case(scenes, case, flags=0, env_rgb=(1.0, 1.0, 1.0), env_map=None, exact=True):
    acc, o = scenes(case["meshes"])
    _, est, _, rad, _ = pc.render_oracle(o, case, flags, env_rgb, env_map)
    got, st = device_frame(acc, case, flags, env_rgb, env_map)
    what = "%s, flags %d, environment %s%s" % (case["name"], flags, env_rgb, "" if env_map is None else " x probe")
    assert st == est, (what, st, est)
    _, _, w, h = case["tile"]
    assert_frame(got, pc.frame_from_paths(rad, w, h, case["spp"]), exact, what)
    return est


ENVIRONMENTS = [(name, rgb, None) for name, rgb in pc.CONSTANT_ENVS] + [("probe of one float", pc.PROBE_RGB, "flat")]


# ---- a. exact pixel sums ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, rgb, probe", ENVIRONMENTS, ids=[e[0] for e in ENVIRONMENTS])
def test_pixel_sums_are_exact(scenes, name, rgb, probe):
    """pt_accumulate's segmented scan (later bounces; the first bounce too under a probe: k_pt_decide<true, true>), pt_accumulate_uniform
    (camera misses under a constant), pt_fix's carry and clamp per sample, the NaN rule: frames that are no power of two at sample counts
    whose runs of a pixel are one lane, straddle a wave and are longer than a wave.  A probe of one float c fetches
    float(c x (w0 + w1 + w2 + w3)) = c whatever acos returned: exact as well."""
    env_map = pc.flat_probe() if probe else None
    for case in pc.sum_cases():
        assert_case(scenes, case, 0, rgb, env_map, exact=True)


# ---- b. every vertex branch ------------------------------------------------------------------------------------------------------
BRANCH_IDS = [c["name"] for c in pc.branch_cases()]


@pytest.mark.parametrize("which", range(len(BRANCH_IDS)), ids=BRANCH_IDS)
def test_vertex_branches_equal_the_oracle(scenes, which):
    """S1 - S4: total internal reflection and the interior bit (both sides of `interior ? ior : 1 / ior`, the bit through k_pt_decide's
    compaction and k_pt_scatter's rewrite), the mirror and roulette ends, the lobe basis on its +-0.6 thresholds, unnormalised Ng"""
    case = pc.branch_cases()[which]
    for flags in case["flags"]:
        assert_case(scenes, case, flags, (0.9, 0.8, 0.7), None, exact=True)
        assert_case(scenes, case, flags, pc.PROBE_RGB, pc.random_probe(), exact=False)


# ---- c. cameras ------------------------------------------------------------------------------------------------------------------
CAMERA_IDS = [c["name"] for c in pc.camera_cases()]


@pytest.mark.parametrize("which", range(len(CAMERA_IDS)), ids=CAMERA_IDS)
def test_cameras_equal_the_oracle(scenes, which):
    """S5: pt_primary_ray's orthographic branch, both handednesses, a turned and non-uniformly scaled cam2world, width != height, tiles
    off the origin that are narrower than the frame"""
    case = pc.camera_cases()[which]
    assert_case(scenes, case, 0, (0.9, 0.8, 0.7), None, exact=True)
    assert_case(scenes, case, 0, pc.PROBE_RGB, pc.random_probe(), exact=False)


# ---- d. divisions on the device ----------------------------------------------------------------------------------------------------
def test_divisions_by_tile_width_and_sample_count(scenes):
    """lh_div by spp and w (lh_pt.h; the formula itself: tests/test_pt_cases.py): a wrong quotient is another pixel or another key"""
    for case in pc.division_tile_cases():
        assert_case(scenes, case, 0, (0.9, 0.8, 0.7), None, exact=True)


@pytest.mark.parametrize("band_rows", pc.DIV_BAND_ROWS)
def test_divisions_by_band_height(scenes, band_rows):
    """render_pt_bands: the bands three ranks would own, each rank's as one pass, put back together as
    test_interleaved_bands_as_one_pass_equal_the_frame does == the oracle's frame, to the bit"""
    import torch
    for spp in (3, 7):
        case = pc.division_band_case(spp)
        acc, o = scenes(case["meshes"])
        cam = pc.cameras(case["cam"])[0]
        W, H = cam.width, cam.height
        assert H % (3 * band_rows) == 0
        _, est, _, rad, _ = pc.render_oracle(o, case, 0, (0.9, 0.8, 0.7), None)
        for k, m in enumerate(case["mats"]):
            acc.set_material(k, pc.la_material(m))
        acc.set_environment((0.9, 0.8, 0.7), None)
        nb = H // band_rows
        img = torch.zeros((nb, band_rows, W, 3), dtype=torch.float32, device="cuda")
        rays = 0; paths = 0; longest = 0
        for r in range(3):
            mine = len(range(r, nb, 3))
            out, s = acc.render_pt_bands(cam, band_rows * r, band_rows, 3 * band_rows, mine, 0, spp, spp, max_vertices=case["max_vertices"],
                                         seed=case["seed"])
            img[r::3] = out
            rays += s["rays"]; paths += s["paths"]; longest = max(longest, s["max_depth_reached"])
        torch.cuda.synchronize()
        what = "%s, bands of %d" % (case["name"], band_rows)
        assert {"paths": paths, "rays": rays, "max_depth_reached": longest} == est, what
        assert_frame(img.flip(0).reshape(H, W, 3).cpu().numpy(), pc.frame_from_paths(rad, W, H, spp), True, what)


# ---- e. chain lengths --------------------------------------------------------------------------------------------------------------
CHAIN_IDS = [c["name"] for c in pc.chain_cases()]


@pytest.mark.parametrize("which", range(len(CHAIN_IDS)), ids=CHAIN_IDS)
def test_chain_lengths_equal_the_oracle(scenes, which):
    """pt_tile reads the survivor count back after every 8th bounce and may stop there: vertex limits either side of the read-backs of
    bounces 7 and 15 with paths alive at both, and a limit of 400 on a scene whose paths have all ended by then"""
    case = pc.chain_cases()[which]
    est = assert_case(scenes, case, 0, (0.9, 0.8, 0.7), None, exact=True)
    assert est["max_depth_reached"] == (case["max_vertices"] - 1 if case["max_vertices"] < 400 else 2)
