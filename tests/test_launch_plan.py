"""The geometry of a persistent launch (lucille_amd/csrc/lh_plan.h) on the CPU: the header, compiled into the stand-alone program
tests/cpu_model/lh_plan_check.c with -fsanitize=address,undefined, against a restatement of the rules in numpy written from the launchers as they were
before the header existed (rows4, coop_rows, top_nodes_for, clamp_chunk and the inline 8-wide and textbook rules of lh_kernels.hip, size_grid of
lh_commit.hip) -- over a table that crosses the edges of every rule -- against rows computed from those functions themselves, and against what must
hold of every plan: even rows, 64 at most; unchecked pushes only where the rows cover the tree; no persistent workgroup above 64 KiB of LDS (which is
why the launchers raise no kernel's LDS limit for one); a copy of the tree's top that never costs a workgroup per CU; the grid sized by the same
workgroups per CU the copy counted on.

One thing the table shows and the parent did the same way: an odd "stack_cap" (9; the 8-wide walk's 15 and 63) is rounded up to an even row count AFTER the
guard is decided, so a tree that asks for exactly cap + 1 rows gets them and checks its pushes all the same.  The guard is therefore asserted as: unchecked
only if the rows cover the tree; checked only if the tree asks for at least the rows; the two coincide (checked exactly when the tree asks for more
than it gets) at every even cap."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_plan_check.c")

AUTO = 0xFFFFFFFF
DIRECT, SPEC = 0, 4                               # LH_VARIANT_*
BATCH, AO, DIRT = 0, 1, 2                         # LH_PLAN_*
W_DIRECT, W_Q4, W_Q8, W_Q4_CHECKED = 0, 3, 7, 8   # LH_WALK_*
ERR_ROWS, ERR_COOP = 1, 2
CASE = np.dtype([(k, np.uint32) for k in ("q4_stack", "q4_depth", "stack_cap", "top_nodes", "nq4nodes", "q8_depth", "prefer_q8", "max_depth", "ray_chunk",
                                          "ray_budget", "n_dev", "kind", "variant", "have_queue")] + [("grid_blocks", np.int32), ("pad", np.uint32), ("n", np.uint64)])
OUT = np.dtype([(k, np.uint32) for k in ("walk", "rows", "guard", "top_nodes", "lds_bytes", "wgs_per_cu", "ray_chunk", "coop", "ray_budget", "coop_rows",
                                         "coop_lds_bytes", "err", "trace_rows", "grid_wgs")])
DEFAULTS = dict(q4_stack=0, q4_depth=14, stack_cap=0, top_nodes=AUTO, nq4nodes=400000, q8_depth=0, prefer_q8=0, max_depth=20, ray_chunk=256, ray_budget=128,
                n_dev=0, kind=BATCH, variant=SPEC, have_queue=1, grid_blocks=1024, n=65536)
DEPTH_EDGES = [0, 3, 4, 8, 9, 19, 20, 40, 41, 83, 84, 168, 169, 175]          # the cooperative ring passes 16, 32, .. 512 rows and beyond (3 d + 6)


# q4_stack / q4_depth / stack_cap / top_nodes / dense / nq4nodes -> rows / guard / top nodes / persistent LDS bytes / cooperative rows, from the parent's functions
RECORDED = [
    ((44, 14, 0, AUTO, 1, 400000), (34, 1, 16, 35840, 64)),
    ((59, 19, 0, 512, 1, 400000), (34, 1, 16, 35840, 64)),          # a caller's 512 nodes held to the room beside 34 dense rows
    ((59, 19, 0, AUTO, 0, 400000), (60, 0, 64, 65536, 64)),
    ((0, 3, 0, AUTO, 0, 21), (16, 0, 21, 17728, 16)),
    ((0, 21, 0, AUTO, 0, 400000), (34, 1, 0, 34816, 128)),
    ((44, 14, 8, AUTO, 1, 400000), (8, 1, 432, 35840, 64)),
    ((44, 14, 64, AUTO, 1, 400000), (44, 0, 48, 48128, 64)),
    ((34, 10, 0, AUTO, 1, 400000), (34, 0, 16, 35840, 64)),
    ((35, 10, 0, AUTO, 1, 400000), (34, 1, 16, 35840, 64)),
    ((0, 169, 0, AUTO, 1, 400000), (34, 1, 96, 40960, 0)),          # deeper than any builder hands over: refused
]


def _cross(**axes):
    """every combination of the axes given; the other fields at their defaults"""
    names = list(axes)
    mesh = np.meshgrid(*[np.asarray(axes[k], np.int64) for k in names], indexing="ij")
    t = np.zeros(mesh[0].size, CASE)
    for k, v in DEFAULTS.items():
        t[k] = v
    for k, m in zip(names, mesh):
        t[k] = m.ravel()
    return t


def _table():
    q4 = dict(stack_cap=[0, 7, 8, 9, 34, 62, 64, 65], n=[65535, 65536], top_nodes=[0, 1, 15, 16, 17, 512, 513, AUTO], nq4nodes=[1, 15, 16, 21, 400000],
              kind=[BATCH, AO, DIRT])
    parts = [
        # the 4-wide rule: the bound of a tree of every depth; the builder's own count beside the depths at which the cooperative ring doubles
        _cross(q4_stack=[0], q4_depth=range(176), **q4),
        _cross(q4_stack=[14, 15, 16, 17, 33, 34, 35, 36, 63, 64, 65, 66], q4_depth=DEPTH_EDGES, **q4),
        # who counts as dense and who runs the cooperative walk: the count on the device, a launch without a queue, a handful of rays
        _cross(q4_stack=[0, 44, 59], q4_depth=[3, 14, 19, 21, 169], n=[1, 64, 65535, 65536], n_dev=[0, 1], have_queue=[0, 1], ray_budget=[128, 2048],
               kind=[BATCH, AO, DIRT]),
        # the 8-wide rule
        _cross(prefer_q8=[1], q8_depth=range(11), stack_cap=[0, 15, 16, 48, 63, 64], n=[65535, 65536], have_queue=[0, 1], q4_depth=[14, 169]),
        # the textbook rule: 16 rows up to 14 levels, refused beyond 62
        _cross(variant=[DIRECT], max_depth=[0, 12, 13, 14, 15, 16, 60, 61, 62, 63, 64, 100], n=[64, 65536], prefer_q8=[0, 1]),
        # the cursor chunk
        _cross(n=[1, 64, 65535, 65536, 1 << 20, 1 << 30], grid_blocks=[-1, 0, 1, 256, 1024], ray_chunk=[0, 64, 256, 1024, 65536], kind=[BATCH, AO, DIRT],
               variant=[DIRECT, SPEC]),
    ]
    for (q4_stack, q4_depth, stack_cap, top_nodes, dense, nq4nodes), _ in RECORDED:
        parts.append(_cross(q4_stack=[q4_stack], q4_depth=[q4_depth], stack_cap=[stack_cap], top_nodes=[top_nodes], n=[65536 if dense else 65535], nq4nodes=[nq4nodes]))
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(the table, the program's plans): built and run once for every test of the module"""
    d = tmp_path_factory.mktemp("plan")
    exe, fin, fout = str(d / "lh_plan_check"), str(d / "in.bin"), str(d / "out.bin")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           SRC, "-o", exe])
    t = _table()
    with open(fin, "wb") as f:
        f.write(np.uint64(t.size).tobytes()); f.write(t.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    out = np.fromfile(fout, OUT)
    assert out.size == t.size
    return t, out


# ---- the rules again, from the launchers as they were ----------------------------------------------------------------------------------------------

def _even_rows(need, cap):
    guard = need > cap
    rows = np.minimum(need, cap)
    rows = rows + (rows & 1)
    return np.where((rows < 16) & ~guard, 16, rows), guard


def _rows4(c, dense):
    need = np.where(c["q4_stack"] > 0, c["q4_stack"], 3 * c["q4_depth"] + 5)
    cap = np.where((c["stack_cap"] >= 8) & (c["stack_cap"] <= 64), c["stack_cap"], np.where(dense | (need > 64), 34, 64))
    return _even_rows(need, cap) + (need,)


def _coop_rows(c):
    need = 3 * c["q4_depth"] + 6
    ring = np.zeros_like(need)
    for r in (512, 256, 128, 64, 32, 16):
        ring = np.where(need <= r, r, ring)
    return ring


def _top_nodes(c, rows, ring):
    coop = np.where(ring > 0, (ring * 64 + 128) * 4 + 1024, 0)
    cu, stack = 160 * 1024 - coop, rows * 1024
    wgs = np.minimum(4, (160 * 1024) // stack)
    spare = np.minimum((cu // wgs - stack) // 64, 512)
    spare = np.where(stack <= 64 * 1024, np.minimum(spare, (64 * 1024 - stack) // 64), spare)
    want = np.where((c["top_nodes"] == AUTO) | (c["top_nodes"] > spare), spare, c["top_nodes"])
    want = np.minimum(want - want % 16, c["nq4nodes"])
    return np.where((c["top_nodes"] == 0) | (cu < wgs * stack), 0, want)


def _expected(t):
    c = {k: t[k].astype(np.int64) for k in CASE.names}
    fused, direct = c["kind"] != BATCH, (c["kind"] == BATCH) & (c["variant"] == DIRECT)
    q8 = ~fused & ~direct & (c["prefer_q8"] != 0)
    dense = (c["n"] >= 65536) | (~fused & (c["n_dev"] != 0))
    rows4, guard4, need4 = _rows4(c, dense)
    need8 = 7 * c["q8_depth"] + 10
    rows8, guard8 = _even_rows(need8, np.where((c["stack_cap"] >= 16) & (c["stack_cap"] < 64), c["stack_cap"], 48))
    rowsd = c["max_depth"] + 2
    rowsd = np.maximum(rowsd + (rowsd & 1), 16)
    rows = np.where(direct, rowsd, np.where(q8, rows8, rows4))
    guard = np.where(direct, False, np.where(q8, guard8, guard4))
    walk = np.where(direct, W_DIRECT, np.where(q8, W_Q8, np.where(guard, W_Q4_CHECKED, W_Q4)))
    ring = _coop_rows(c)
    top = np.where(direct | q8, 0, _top_nodes(c, rows, ring))
    coop = fused | (~direct & (c["have_queue"] != 0) & dense)
    waves = np.maximum(c["grid_blocks"], 1) * 4
    chunk = np.minimum(c["ray_chunk"], np.maximum(c["n"] // (waves * 4), 64))
    trace_rows = _rows4(c, True)[0]
    e = dict(walk=walk, rows=rows, guard=guard, top_nodes=top, lds_bytes=rows * 1024 + top * 64, wgs_per_cu=np.minimum(4, 160 // rows),
             ray_chunk=np.where(chunk == 0, 64, chunk), coop=coop, ray_budget=np.where(coop, c["ray_budget"], 0xFFFFFFFF), coop_rows=ring,
             coop_lds_bytes=(ring * 64 + 192) * 4, err=np.where(rows > 64, ERR_ROWS, np.where(coop & (ring == 0), ERR_COOP, 0)),
             trace_rows=trace_rows, grid_wgs=np.maximum(np.minimum(4, 160 // trace_rows), 1))
    e["need"] = np.where(direct, rowsd, np.where(q8, need8, need4))
    e["dense"] = dense
    return e


def test_plans_agree_with_the_restated_rules(plans):
    t, out = plans
    e = _expected(t)
    for k in OUT.names:
        bad = np.flatnonzero(out[k].astype(np.int64) != e[k].astype(np.int64))
        assert bad.size == 0, (k, bad.size, t[bad[:3]], out[bad[:3]], e[k][bad[:3]])


def test_recorded_rows(plans):
    t, out = plans
    for (q4_stack, q4_depth, stack_cap, top_nodes, dense, nq4nodes), want in RECORDED:
        hit = np.flatnonzero((t["q4_stack"] == q4_stack) & (t["q4_depth"] == q4_depth) & (t["stack_cap"] == stack_cap) & (t["top_nodes"] == top_nodes) &
                             (t["n"] == (65536 if dense else 65535)) & (t["nq4nodes"] == nq4nodes) & (t["kind"] == BATCH) & (t["variant"] == SPEC) &
                             (t["prefer_q8"] == 0) & (t["n_dev"] == 0) & (t["have_queue"] == 1))
        assert hit.size >= 1, (q4_stack, q4_depth, stack_cap, top_nodes, dense, nq4nodes)
        for o in out[hit]:
            assert (int(o["rows"]), int(o["guard"]), int(o["top_nodes"]), int(o["lds_bytes"]), int(o["coop_rows"])) == want
            # the cooperative walk runs beside a dense launch: without a ring for it the launch is refused, as it was when launch_coop found out
            assert int(o["err"]) == (ERR_COOP if dense and want[4] == 0 else 0) and int(o["coop"]) == dense
            assert int(o["walk"]) == (W_Q4_CHECKED if want[1] else W_Q4)


def test_invariants(plans):
    t, out = plans
    e = _expected(t)
    o = {k: out[k].astype(np.int64) for k in OUT.names}
    ok = o["err"] != ERR_ROWS
    assert ok.sum() > t.size // 2 and (o["err"] == ERR_ROWS).any() and (o["err"] == ERR_COOP).any()
    assert np.all((o["rows"][ok] % 2 == 0) & (o["rows"][ok] <= 64) & (o["rows"][ok] >= 8))
    guard, need, rows = o["guard"] != 0, e["need"], o["rows"]
    assert np.all(need[~guard] <= rows[~guard])          # unchecked pushes only where the rows cover the tree
    assert np.all(need[guard] >= rows[guard])            # checked only where the tree asks for at least the rows ...
    direct = o["walk"] == W_DIRECT
    q8 = o["walk"] == W_Q8
    cap = np.where(q8, np.where((t["stack_cap"] >= 16) & (t["stack_cap"] < 64), t["stack_cap"], 48), np.where((t["stack_cap"] >= 8) & (t["stack_cap"] <= 64), t["stack_cap"], 0))
    even = ~direct & (cap % 2 == 0)
    assert np.array_equal(guard[even], need[even] > rows[even])          # ... exactly where it asks for more than it gets, at every even cap
    assert (guard & ~even).any() and guard[even].any() and (~guard[even]).any()
    # no persistent workgroup above 64 KiB of LDS: no launcher raises a persistent kernel's limit
    assert np.all(o["lds_bytes"][ok] <= 64 * 1024) and (o["lds_bytes"] == 64 * 1024).any()
    # the copy of the tree's top never costs a workgroup per CU: the workgroups, the cooperative walk's beside them and a KiB fit a CU's 160 KiB
    top = o["top_nodes"] > 0
    # (a tree too deep for any ring -- RECORDED's last row -- has no cooperative walk to leave room for: a launch that would run one is refused)
    beside = np.where(o["coop_rows"] > 0, o["coop_lds_bytes"] + 1024, 0)
    assert top.any() and np.all(o["wgs_per_cu"][top] * o["lds_bytes"][top] + beside[top] <= 160 * 1024)
    assert np.all(o["err"][(o["coop_rows"] == 0) & (o["coop"] != 0)] == ERR_COOP)
    assert np.all((o["top_nodes"] % 16 == 0) | (o["top_nodes"] == t["nq4nodes"]))
    assert np.all(o["top_nodes"][direct | q8] == 0)
    # the grid is sized (size_grid) by the workgroups per CU the top-of-tree rule counted on, for every launch of the default walk that fills the chip
    fills = e["dense"] & ~direct & ~q8
    assert fills.any() and np.array_equal(o["grid_wgs"][fills], o["wgs_per_cu"][fills]) and np.array_equal(o["trace_rows"][fills], o["rows"][fills])
    assert np.all((o["grid_wgs"] >= 2) & (o["grid_wgs"] <= 4))
    # the cooperative walk's ring: a power of two from 16 to 512 that covers 3 levels + 6, or none
    ring = o["coop_rows"]
    assert np.all((ring == 0) | ((ring >= 16) & (ring <= 512) & (ring & (ring - 1) == 0) & (ring >= 3 * t["q4_depth"] + 6)))
    assert (o["coop_lds_bytes"] > 64 * 1024).any()          # trees of 41 levels and more: the one kernel whose LDS limit is raised
