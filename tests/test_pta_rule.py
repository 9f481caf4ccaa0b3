"""The rule of area lights at the path tracer's vertices (lucille_amd/csrc/lh_ptl.h: the key of an entry, the seed of a bounce, the add of the two
stages' values, the refusal of a frame whose keys do not fit 34 bits) on the CPU: the header, compiled into the stand-alone program
tests/cpu_model/lh_pta_check.c with -fsanitize=address,undefined, against a restatement in numpy, bit for bit.

The restatement (area_key, area_seed, value_add, keys_ok, pass_pixel, path_keys below) is what tests/test_gpu_pt_area.py holds the device to."""
import os

import numpy as np
import pytest

from tests import pt_cases as pc
from tests.test_ptl_rule import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_pta_check.c")

CASE = np.dtype([("px", np.int32), ("py", np.int32), ("width", np.int32), ("height", np.int32), ("spp_total", np.int32), ("spp_begin", np.int32),
                 ("s", np.int32), ("d", np.int32), ("seed", np.uint64), ("delta", np.float32, (3,)), ("area", np.float32, (3,))])
OUT = np.dtype([("key", np.uint64), ("seed", np.uint64), ("value", np.float32, (3,)), ("ok", np.uint32)])
BOUNCE = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1


# ---- the rule, restated -------------------------------------------------------------------------------------------------------------------------
def area_key(px, py, width, spp_total, spp_begin, s):
    """((py * width + px) * spp_total) + (spp_begin + s), in uint64"""
    px, py, s = (np.asarray(x).astype(np.uint64) for x in (px, py, s))
    return (py * np.uint64(width) + px) * np.uint64(spp_total) + (np.uint64(spp_begin) + s)


def area_seed(seed, d):
    """seed + (d + 1) * 0xD1B54A32D192ED03 modulo 2^64, as a Python int"""
    return (int(seed) + (int(d) + 1) * BOUNCE) & M64


def value_add(delta, area):
    """one float32 add per channel"""
    with np.errstate(all="ignore"):
        r = np.asarray(delta, np.float32) + np.asarray(area, np.float32)
    assert r.dtype == np.float32
    return r


def keys_ok(width, height, spp_total):
    """a frame's keys fit the generator's 34 bits (Python integers: no overflow to think of)"""
    return width >= 1 and height >= 1 and spp_total >= 1 and width * height * spp_total <= 1 << 34


def pass_pixel(pix, x0, y0, w, band_rows, band_stride):
    """lh_pt.h pt_pixel: pixel of the pass -> frame pixel (px, py); a tile: band_rows = its height"""
    pix = np.asarray(pix).astype(np.uint64)
    row = pc.lh_div_py(pix, pc.lh_div_make_py(w))
    band = pc.lh_div_py(row, pc.lh_div_make_py(band_rows))
    px = x0 + (pix - row * np.uint64(w)).astype(np.int64)
    py = y0 + band.astype(np.int64) * band_stride + (row - band * np.uint64(band_rows)).astype(np.int64)
    return px, py


def path_keys(path, spp, spp_begin, spp_total, width, x0, y0, w, band_rows, band_stride=0):
    """the keys of a pass's path ids (pixel of the pass x spp + sample): k_pt_area_keys"""
    path = np.asarray(path).astype(np.uint64)
    pix = pc.lh_div_py(path, pc.lh_div_make_py(spp))
    s = path - pix * np.uint64(spp)
    px, py = pass_pixel(pix, x0, y0, w, band_rows, band_stride)
    return area_key(px, py, width, spp_total, spp_begin, s)


# ---- the program --------------------------------------------------------------------------------------------------------------------------------
def _run(exe, tmp, table):
    import subprocess
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint64(table.size).tobytes()); f.write(table.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    out = np.fromfile(fout, OUT)
    assert out.size == table.size
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert CASE.itemsize == 64 and OUT.itemsize == 32          # the C program's case_t and out_t
    d = tmp_path_factory.mktemp("pta")
    exe = _build(d, SRC, "lh_pta_check")
    return lambda table: _run(exe, d, table)


def _cases(n, width=1, height=1, spp_total=1):
    t = np.zeros(n, CASE)
    t["width"] = width; t["height"] = height; t["spp_total"] = spp_total
    return t


def _pass_cases(width, height, spp, spp_begin, spp_total, x0, y0, w, band_rows, band_stride, nbands=1):
    """every path of a pass as a case: px, py through the restated pt_pixel"""
    path = np.arange(w * band_rows * nbands * spp, dtype=np.uint64)
    pix = pc.lh_div_py(path, pc.lh_div_make_py(spp))
    t = _cases(path.shape[0], width, height, spp_total)
    t["px"], t["py"] = pass_pixel(pix, x0, y0, w, band_rows, band_stride)
    t["s"] = (path - pix * np.uint64(spp)).astype(np.int32); t["spp_begin"] = spp_begin
    return t, path_keys(path, spp, spp_begin, spp_total, width, x0, y0, w, band_rows, band_stride)


def test_keys_of_tiles_and_bands(program):
    """a 41 x 45 frame of 7 samples: as four unequal tiles, as the bands of three ranks (1, 3 and 5 lines), and as two passes over the samples --
    every decomposition gives each (pixel, sample) of the frame its key py * W * spp + px * spp + s once"""
    W, H, spp = 41, 45, 7
    want = np.arange(W * H * spp, dtype=np.uint64)
    tiles = [(0, 0, 23, 17), (23, 0, 18, 17), (0, 17, 1, 28), (1, 17, 40, 28)]
    got = []
    for x0, y0, w, h in tiles:
        t, keys = _pass_cases(W, H, spp, 0, spp, x0, y0, w, h, 0)
        out = program(t)
        assert np.array_equal(out["key"], keys) and out["ok"].all()
        assert (t["px"] >= x0).all() and (t["px"] < x0 + w).all() and (t["py"] >= y0).all() and (t["py"] < y0 + h).all()
        got.append(keys)
    assert np.array_equal(np.sort(np.concatenate(got)), want)
    for rows in pc.DIV_BAND_ROWS:
        got = []
        nb = H // rows
        for r in range(3):
            mine = len(range(r, nb, 3))
            t, keys = _pass_cases(W, H, spp, 0, spp, 0, rows * r, W, rows, 3 * rows, mine)
            assert np.array_equal(program(t)["key"], keys)
            got.append(keys)
        assert np.array_equal(np.sort(np.concatenate(got)), want), rows
    # spp_begin > 0: samples 0 .. 4 and 5 .. 6 as passes of their own
    a, ka = _pass_cases(W, H, 5, 0, spp, 3, 2, 11, 9, 0)
    b, kb = _pass_cases(W, H, 2, 5, spp, 3, 2, 11, 9, 0)
    assert np.array_equal(program(a)["key"], ka) and np.array_equal(program(b)["key"], kb)
    whole = path_keys(np.arange(11 * 9 * spp), spp, 0, spp, W, 3, 2, 11, 9)
    assert np.array_equal(np.sort(np.concatenate([ka, kb])), np.sort(whole))
    assert np.array_equal(kb, whole.reshape(-1, spp)[:, 5:].reshape(-1))          # sample s of the second pass is sample 5 + s of the whole


def test_the_largest_frame(program):
    """width x height x spp_total exactly 2^34: pixel 0 has key 0 .. spp - 1, the last pixel's last sample 2^34 - 1; and plain Python integers agree"""
    W, H, spp = 1 << 15, 1 << 13, 1 << 6
    assert W * H * spp == 1 << 34
    t = _cases(6, W, H, spp)
    t["px"] = [0, 0, W - 1, W - 1, W - 1, 12345]; t["py"] = [0, 0, H - 1, H - 1, 0, 6789]
    t["spp_begin"] = [0, 60, 0, 60, 7, 31]; t["s"] = [0, 3, 0, 3, 1, 32]
    out = program(t)
    want = [(int(r["py"]) * W + int(r["px"])) * spp + int(r["spp_begin"]) + int(r["s"]) for r in t]
    assert [int(k) for k in out["key"]] == want
    assert want[0] == 0 and want[1] == spp - 1 and want[3] == (1 << 34) - 1
    assert np.array_equal(out["key"], area_key(t["px"], t["py"], W, spp, 0, t["spp_begin"] + t["s"]))
    # a frame of 2^31 - 1 columns: the products stay in 64 bits
    t = _cases(1, (1 << 31) - 1, 8, 1); t["px"] = (1 << 31) - 2; t["py"] = 7
    assert int(program(t)["key"][0]) == 7 * ((1 << 31) - 1) + (1 << 31) - 2


def test_the_seed_of_a_bounce(program):
    seeds = [0, 1, 21, M64, M64 - BOUNCE + 1, M64 - BOUNCE, (1 << 63) + 5, 0x9E3779B97F4A7C15]
    ds = [0, 1, 2, 7, 398, 65534]
    t = _cases(len(seeds) * len(ds))
    t["seed"] = np.repeat(np.array(seeds, np.uint64), len(ds)); t["d"] = np.tile(np.array(ds, np.int32), len(seeds))
    out = program(t)
    want = [area_seed(int(s), int(d)) for s, d in zip(t["seed"], t["d"])]
    assert [int(x) for x in out["seed"]] == want
    # d = 0 adds the constant once; a seed where that sum passes 2^64 wraps; the seed itself (the path's own draws) is never a bounce's
    assert area_seed(21, 0) == 21 + BOUNCE and area_seed(M64, 0) == BOUNCE - 1 and area_seed(M64 - BOUNCE + 1, 0) == 0
    assert all(area_seed(s, d) != s for s in seeds for d in ds)
    assert len({area_seed(21, d) for d in range(65535)}) == 65535


def test_the_value_add(program):
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1.0e-45, 3.0e38, -3.0e38, 0.1, 16777216.0], np.float32)
    a, b = np.meshgrid(sp, sp, indexing="ij")
    rng = np.random.default_rng(9)
    n = a.size
    t = _cases(n + 3000)
    t["delta"][:n] = a.reshape(-1)[:, None]; t["area"][:n] = b.reshape(-1)[:, None]
    t["delta"][n:] = (rng.uniform(1.0, 2.0, (3000, 3)) * 2.0 ** rng.integers(-20, 20, (3000, 3))).astype(np.float32)
    t["area"][n:] = (rng.uniform(-2.0, 2.0, (3000, 3)) * 2.0 ** rng.integers(-20, 20, (3000, 3))).astype(np.float32)
    out = program(t)
    want = value_add(t["delta"], t["area"])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out["value"]), nan)
    assert np.array_equal(out["value"].view(np.uint32)[~nan], want.view(np.uint32)[~nan])

    def one(x, y):
        return value_add(np.float32(x), np.float32(y))
    assert np.signbit(one(-0.0, -0.0)) and not np.signbit(one(0.0, -0.0)) and not np.signbit(one(-0.0, 0.0))
    assert np.isnan(one(np.inf, -np.inf)) and one(np.inf, 1.0) == np.inf and np.isnan(one(np.nan, 0.0)) and one(3.0e38, 3.0e38) == np.inf


def test_the_refusal(program):
    frames = [(1 << 15, 1 << 13, 1 << 6, True), (1 << 15, 1 << 13, (1 << 6) + 1, False), (1 << 17, 1 << 17, 1, True), ((1 << 17) + 1, 1 << 17, 1, False),
              (131073, 131071, 1, True), (131071, 3, 43691, True),                      # 2^34 - 1 = 3 x 43691 x 131071
              (652805, 26317, 1, False), (26317, 5, 137 * 953, False),                  # 2^34 + 1 = 5 x 137 x 953 x 26317
              (1, 1, (1 << 31) - 1, True), (8, 1, (1 << 31) - 1, True), (9, 1, (1 << 31) - 1, False),
              ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, False),                      # the product passes 2^64
              ((1 << 31) - 1, (1 << 31) - 1, 1, False), (1 << 16, 1 << 16, 4, True), (1 << 16, 1 << 16, 5, False),
              (23, 17, 65, True), (0, 17, 3, False), (23, -1, 3, False), (23, 17, 0, False)]
    t = _cases(len(frames))
    for k, (w, h, s, _) in enumerate(frames):
        t[k]["width"] = w; t[k]["height"] = h; t[k]["spp_total"] = s
    out = program(t)
    for k, (w, h, s, ok) in enumerate(frames):
        assert keys_ok(w, h, s) == ok and bool(out["ok"][k]) == ok, (w, h, s)
    assert 652805 * 26317 == (1 << 34) + 1 == 26317 * 5 * 137 * 953
    # exactly at 2^34 and a column more
    assert keys_ok(1 << 34 >> 20, 1 << 10, 1 << 10) and not keys_ok((1 << 14) + 1, 1 << 10, 1 << 10)
    t = _cases(2, 1 << 14, 1 << 10, 1 << 10); t[1]["width"] = (1 << 14) + 1
    assert list(program(t)["ok"]) == [1, 0]
