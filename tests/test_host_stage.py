"""The layout of a host form's staging block (lucille_amd/csrc/lh_stage.h) on the CPU: the header, compiled into the stand-alone program
tests/cpu_model/lh_stage_check.c with -fsanitize=address,undefined, over field lists of 1 to 12 fields whose byte counts cross the rule's edges -- nothing,
a byte, either side of the 16-byte boundary and of a page, beyond 2^31 -- in every position; and over the field lists of the eleven entry points that
take host arrays, restated here, against the bytes the hand-kept size expressions they replace asked for (without their slack constants): no array
shrank."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_stage_check.c")

MAXF = 12
ALIGN = 16
ABSENT = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZE_MAX = (1 << 64) - 1
SCRATCH, UP, UP_NULL, DOWN, DOWN_NULL, BOTH, BOTH_NULL = range(7)          # KIND_*
GIVEN = {SCRATCH: True, UP: True, UP_NULL: False, DOWN: True, DOWN_NULL: False, BOTH: True, BOTH_NULL: False}
CASE = np.dtype([("nf", np.uint32), ("kind", np.uint8, MAXF), ("bytes", np.uint64, MAXF)])
OUT = np.dtype([("rc", np.int32), ("pad", np.uint32), ("total", np.uint64), ("bytes", np.uint64, MAXF), ("off", np.uint64, MAXF), ("dev", np.uint64, MAXF)])
EDGES = [0, 1, 15, 16, 17, 4095, 4096, (1 << 31) + 4]
HUGE = SIZE_MAX // 2 + 16


def _case(fields):
    """fields: (kind, bytes) pairs"""
    c = np.zeros(1, CASE)
    c["nf"] = len(fields)
    for k, (kind, b) in enumerate(fields):
        c["kind"][0, k] = kind
        c["bytes"][0, k] = b
    return c


def _sweep():
    parts = []
    # every byte count in every position of every field count, over every background the other fields share
    for nf in range(1, MAXF + 1):
        for pos, b, bg in itertools.product(range(nf), EDGES, EDGES):
            parts.append(_case([(SCRATCH, b if k == pos else bg) for k in range(nf)]))
    # every combination of byte counts up to four fields
    for nf in range(1, 5):
        for bs in itertools.product(EDGES, repeat=nf):
            parts.append(_case([(SCRATCH, b) for b in bs]))
    # mixed lists of every length: byte counts and constructors drawn from the tables (a constructor handed NULL makes an absent field)
    rng = np.random.default_rng(20)
    for nf in range(1, MAXF + 1):
        for _ in range(200):
            parts.append(_case([(int(rng.integers(0, 7)), EDGES[int(rng.integers(0, len(EDGES)))]) for _ in range(nf)]))
    return np.concatenate(parts)


REFUSED = [
    [(SCRATCH, HUGE), (SCRATCH, HUGE)],
    [(UP, HUGE), (DOWN, 16), (BOTH, HUGE)],
    [(SCRATCH, SIZE_MAX)],                                   # rounding it up would wrap
    [(SCRATCH, SIZE_MAX - 14)],
    [(SCRATCH, 16), (SCRATCH, SIZE_MAX - 15 - 15)],          # a total of 2^64 exactly
]
FITS = [
    [(SCRATCH, HUGE), (UP_NULL, HUGE)],                      # the second is absent: the caller left it NULL
    [(SCRATCH, SIZE_MAX - 15)],
    [(SCRATCH, 16), (SCRATCH, SIZE_MAX - 15 - 16)],
]


def _run(tmp, table):
    exe, fin, fout = str(tmp / "lh_stage_check"), str(tmp / "in.bin"), str(tmp / "out.bin")
    if not os.path.exists(exe):
        subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               SRC, "-o", exe])
    with open(fin, "wb") as f:
        f.write(np.uint64(table.size).tobytes()); f.write(table.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report, or two layouts of one list that differ, end the program with a message
    out = np.fromfile(fout, OUT)
    assert out.size == table.size
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("stage")


@pytest.fixture(scope="module")
def sweep(tmp):
    t = _sweep()
    return t, _run(tmp, t)


def _check_layout(t, out):
    """what must hold of every list that was laid out, in Python integers"""
    for c, o in zip(t, out):
        nf = int(c["nf"])
        assert o["rc"] == 0
        end = 0
        for k in range(nf):
            want = int(c["bytes"][k]) if GIVEN[int(c["kind"][k])] else 0
            b, off = int(o["bytes"][k]), int(o["off"][k])
            assert b == want
            if b == 0:
                assert o["dev"][k] == ABSENT and off == end          # no pointer, and nothing moved: the next present field starts where this one would have
                continue
            assert off % ALIGN == 0 and off == end and int(o["dev"][k]) == off          # aligned, in order, directly behind its predecessor's rounded end
            end = off + (b + ALIGN - 1) // ALIGN * ALIGN
            assert off + b <= end
        assert int(o["total"]) == end and end % ALIGN == 0


def test_every_edge_in_every_position(sweep):
    t, out = sweep
    assert t.size == 78 * 64 + (8 + 64 + 512 + 4096) + 12 * 200 and {int(n) for n in t["nf"]} == set(range(1, MAXF + 1))
    _check_layout(t, out)


def test_an_absent_field_shifts_nothing(tmp, sweep):
    """a list with its zero-byte fields taken out lays its other fields out at the same places"""
    t, out = sweep
    rows = [k for k in range(0, t.size, 37) if 1 < int(t["nf"][k]) and 0 < int((out["bytes"][k][:int(t["nf"][k])] != 0).sum()) < int(t["nf"][k])]
    assert len(rows) > 100
    dense = np.concatenate([_case([(SCRATCH, int(b)) for b in out["bytes"][k][:int(t["nf"][k])] if b != 0]) for k in rows])
    got = _run(tmp, dense)
    for k, g, d in zip(rows, got, dense):
        present = [int(o) for o, b in zip(out["off"][k][:int(t["nf"][k])], out["bytes"][k][:int(t["nf"][k])]) if b != 0]
        assert present == [int(o) for o in g["off"][:int(d["nf"])]] and g["total"] == out["total"][k]


def test_a_total_beyond_size_t_is_refused(tmp):
    out = _run(tmp, np.concatenate([_case(f) for f in REFUSED]))
    assert np.all(out["rc"] == -1) and np.all(out["total"] == 0)
    fits = np.concatenate([_case(f) for f in FITS])
    _check_layout(fits, _run(tmp, fits))


# ---- the eleven entry points: their field lists as the code states them, and the bytes the size expressions they replace named -------------------------

BEAM_SET = 24 + 96 + 96 + 4 + 12          # sizeof(lh_beam_set_t)
STATE_DOUBLES = 24                        # LH_STATE_DOUBLES
PX = 5 * 3                                # a raster window
GATHER_N = 16                             # gather rays per hit the replayed uniforms are sized for


def _r(x, to):
    return (x + to - 1) // to * to


def _gather(n, key, uni_per_item, rad_floats, counts, rad):
    need = uni_per_item * GATHER_N * n
    fields = [(UP, 24 * n), (UP, 24 * n), (UP, 8 * n), (UP, 8 * n), (UP, 8 * n), (UP, 4 * n), (UP if key else UP_NULL, 8 * n), (UP if need else UP_NULL, 8 * need),
              (DOWN if counts else DOWN_NULL, 4 * n), (DOWN if rad else DOWN_NULL, 4 * rad_floats * n)]
    # the parent allocated both outputs whether asked for or not: what a call USES is what must not shrink
    return fields, 2 * 24 * n + 3 * 8 * n + (8 * n if key else 0) + 8 * need + 4 * n + (4 * n if counts else 0) + (4 * rad_floats * n if rad else 0)


def _entry_points(n):
    """name -> (fields, the parent's bytes)"""
    e = {
        "beam_visibility_host": ([(UP, 24 * n), (UP, 96 * n), (UP_NULL, BEAM_SET * n), (DOWN, 4 * n)], 24 * n + 96 * n + 4 * n),
        "beam_visibility_set_host": ([(UP_NULL, 24 * n), (UP_NULL, 96 * n), (UP, BEAM_SET * n), (DOWN, 4 * n)], BEAM_SET * n + 4 * n),
        "beam_raster_host": ([(UP, 24 * n), (UP, 96 * n), (UP_NULL, BEAM_SET * n), (UP, 24 * n), (BOTH, 8 * PX * n), (DOWN, 4 * n), (DOWN, 32 * n)],
                             2 * 24 * n + 96 * n + 8 * PX * n + _r(4 * n, 8) + 32 * n),
        "beam_raster_set_host": ([(UP_NULL, 24 * n), (UP_NULL, 96 * n), (UP, BEAM_SET * n), (UP, 24 * n), (BOTH, 8 * PX * n), (DOWN, 4 * n), (DOWN, 32 * n)],
                                 _r(BEAM_SET * n, 16) + 24 * n + 8 * PX * n + _r(4 * n, 8) + 32 * n),
        "environment_host": ([(UP, 24 * n), (DOWN, 12 * n)], n * (24 + 12)),
        "sky_host": ([(UP, 24 * n), (DOWN, 12 * n)], n * (24 + 12)),
        "state_build_host": ([(DOWN, 8 * STATE_DOUBLES * n), (UP, 24 * n), (UP, 24 * n), (UP, 8 * n), (UP, 8 * n), (UP, 8 * n), (UP, 4 * n)],
                             2 * 24 * n + 3 * 8 * n + 4 * n + 8 * STATE_DOUBLES * n),
        # a tile of n x 1 pixels, one sample each, every sample a hit: two uniforms per gather ray, three floats per pixel (the parent: two blocks)
        "render_ao_tile_host": ([(UP, 8 * 2 * GATHER_N * n), (DOWN, 12 * n)], 8 * 2 * GATHER_N * n + 12 * n),
        "render_ao_tile_host, no uniforms": ([(UP_NULL, 8 * 2 * GATHER_N * n), (DOWN, 12 * n)], 12 * n),
        "texture_host": ([(DOWN, 4 * 8 * n), (UP, 8 * n), (UP, 8 * n), (UP, 4 * n)], 6 * 8 * n + 4 * n),
        "whitted_host": ([(UP, 24 * n), (UP, 24 * n), (BOTH, 24 * n), (BOTH, 24 * n), (UP, 8 * n), (UP, 8 * n), (UP, 8 * n), (UP, 4 * n), (DOWN, 4 * n), (DOWN, 12 * n)],
                         4 * 24 * n + 3 * 8 * n + 2 * 4 * n + 12 * n),
    }
    # gather_batch_host, a row per transport (uniforms per gather ray, floats of radiance per ray), with and without its optional arrays
    for kind, upi, rf in (("ao", 2, 1), ("dirt", 2, 1), ("env", 2, 3), ("lights", 0, 3), ("area_lights", 3, 3)):
        for key, uni, counts, rad in ((1, 1, 1, 1), (0, 0, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0)):
            e["%s_host key=%d uniforms=%d counts=%d radiance=%d" % (kind, key, uni, counts, rad)] = _gather(n, key, upi if uni else 0, rf, counts, rad)
    return e


@pytest.mark.parametrize("n", [1, 3, 257])
def test_no_array_of_an_entry_point_shrank(tmp, n):
    e = _entry_points(n)
    names = sorted(e)
    t = np.concatenate([_case(e[k][0]) for k in names])
    out = _run(tmp, t)
    _check_layout(t, out)
    for k, c, o in zip(names, t, out):
        nf = int(c["nf"])
        assert int(o["total"]) >= e[k][1], (k, n)
        assert int(o["total"]) >= int(o["bytes"][:nf].sum()) and int(o["total"]) - int(o["bytes"][:nf].sum()) < ALIGN * nf, (k, n)
