"""The gather stage's path that reads the hit count BEFORE its fused launch (fused and not late: lh_gather.h lh_gather_plan): reached
through LH_AO_SYNC, which the library reads per call, and -- for AO tiles -- through the grouped order (set_param "ao_group").  Whatever
the path, the frame and the statistics are the default call's, bit for bit.  One 32 x 32 tile of the c1 scene, 2 x 2 pixel samples,
16 gather samples: a few launches of about a thousand hit slots each."""
import numpy as np
import pytest

import lucille_amd as la
from tests.test_gpu_ao_batch import NO_HIT, ao, host
from tests.test_gpu_dirt import same_bits, scene_clips
from tests.test_gpu_envgather import INV_PI, c1  # noqa: F401 -- c1: the fixture (ao_c1 with the seeded light probe as its environment)
from tests.test_gpu_sky import make_sky
from tests.test_sky_rule import GOLDEN

pytestmark = pytest.mark.gpu

T, PXS, NS = 32, 2, 16


def corner(cam):
    return (cam.width - T) // 2, (cam.height - T) // 2


def tiles(case):
    """name -> a call that renders the tile and returns (rgb on the host, stats)"""
    acc, cam = case["acc"], case["cam"]
    x0, y0 = corner(cam)
    envp = la.EnvParams(1e-5, INV_PI)

    def run(f, *a):
        rgb, st = f(cam, x0, y0, T, T, PXS, NS, *a, seed=5)
        return host(rgb).copy(), dict(st)
    return {"ao": lambda: run(acc.render_ao_tile), "dirt": lambda: run(acc.render_dirt_tile, scene_clips(case)),
            "env": lambda: run(acc.render_env_tile, envp)}


def check_hits(st):
    assert 0 < st["primary_hits"] <= st["primary_rays"] == T * T * PXS * PXS
    assert st["ao_rays"] == st["primary_hits"] * NS and st["ao_occluded"] > 0


@pytest.mark.parametrize("kind", ["ao", "dirt", "env", "sky"])
def test_count_read_first_equals_the_default(c1, monkeypatch, kind):
    acc = c1["acc"]
    monkeypatch.delenv("LH_AO_SYNC", raising=False)
    if kind == "sky":
        acc.set_sky(make_sky(np.load(GOLDEN), 0, la.SKY_SUN))
    try:
        render = tiles(c1)["env" if kind == "sky" else kind]
        rgb, st = render()
        check_hits(st)
        assert (rgb > 0.0).any()
        monkeypatch.setenv("LH_AO_SYNC", "1")
        rgb1, st1 = render()
        assert st1 == st
        assert same_bits(rgb1, rgb), int((rgb1 != rgb).sum())
    finally:
        if kind == "sky":
            acc.reset_sky()


def test_grouped_order_tile_equals_the_plain_order(c1, monkeypatch):
    acc = c1["acc"]
    monkeypatch.delenv("LH_AO_SYNC", raising=False)
    render = tiles(c1)["ao"]
    rgb, st = render()
    check_hits(st)
    acc.set_param("ao_group", 16)
    try:
        rgb1, st1 = render()
    finally:
        acc.set_param("ao_group", 0)
    assert st1 == st
    assert same_bits(rgb1, rgb), int((rgb1 != rgb).sum())


def test_grouped_order_batch_equals_the_plain_order(c1):
    import torch
    acc, cam = c1["acc"], c1["cam"]
    x0, y0 = corner(cam)
    org, dr = acc.primary_rays(cam, x0, y0, T, T, PXS)
    rec = acc.intersect_device(org, dr); torch.cuda.synchronize()
    cnt, rad = ao(acc, org, dr, rec, NS, seed=5)
    assert (cnt != NO_HIT).any() and (rad > 0.0).any()
    acc.set_param("ao_group", 16)
    try:
        cnt1, rad1 = ao(acc, org, dr, rec, NS, seed=5)
    finally:
        acc.set_param("ao_group", 0)
    assert np.array_equal(cnt1, cnt)
    assert same_bits(rad1, rad)
