"""The gather stage's plan (lucille_amd/csrc/lh_gather.h lh_gather_plan: does a stage run fused, and is it late -- the hit count left on the
device) on the CPU: the header, compiled into the stand-alone program tests/cpu_model/lh_gather_check.c with -fsanitize=address,undefined, against
a restatement in numpy of the two pairs of expressions it replaced, written from ao_region and ao_batch_device of lh_tile.hip as they were before
the header existed, over a table that steps across every edge of either.

What the table shows of the differences between the two callers, all of them as before: a tile keeps a grouped-order AO stage fused and reads the
count first, a batch runs it materialised; a batch decides "fused" on the worst case (entries x N below 2^31), a tile leaves that to the stage,
which knows the hits; only a tile consults the request to read the count first (LH_AO_SYNC)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_gather_check.c")

AO, DIRT, ENV = 0, 1, 2          # LH_GATHER_*
TILE, BATCH = 0, 1
SUN_LATE_MAX, ENV_LATE_MAX, DIRT_LATE_MAX = 1 << 30, 1 << 28, 1 << 27
CASE = np.dtype([(k, np.uint32) for k in ("kind", "where", "ao_fused", "uniforms", "ao_group", "sun", "sync", "pad")] + [("entries", np.uint64), ("N", np.uint64)])
OUT = np.dtype([("fused", np.uint32), ("late", np.uint32)])

# (entries, N): entries x N at 2^31 - 1 / 2^31 and around; at each LATE_MAX and LATE_MAX + 1 (N = 1), and the nearest products on either side of them with
# N = 16 and 64; entries at 2^30 and 2^30 + 1 (the sun's list); small stages
SIZES = ([(e, 1) for e in (1, 1024, DIRT_LATE_MAX - 1, DIRT_LATE_MAX, DIRT_LATE_MAX + 1, ENV_LATE_MAX - 1, ENV_LATE_MAX, ENV_LATE_MAX + 1,
                           SUN_LATE_MAX - 1, SUN_LATE_MAX, SUN_LATE_MAX + 1, (1 << 31) - 1, 1 << 31)] +
         [(e, 16) for e in (1, 1024, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, 1 << 24, (1 << 24) + 1, (1 << 27) - 1, 1 << 27, (1 << 27) + 1, SUN_LATE_MAX, SUN_LATE_MAX + 1)] +
         [(e, 64) for e in (1 << 21, (1 << 21) + 1, 1 << 22, (1 << 22) + 1, (1 << 25) - 1, 1 << 25, SUN_LATE_MAX, SUN_LATE_MAX + 1)])


def _table():
    axes = dict(kind=[AO, DIRT, ENV], where=[TILE, BATCH], ao_fused=[0, 1], uniforms=[0, 1], ao_group=[0, 16], sun=[0, 1], sync=[0, 1],
                size=range(len(SIZES)))
    names = list(axes)
    mesh = np.meshgrid(*[np.asarray(axes[k], np.int64) for k in names], indexing="ij")
    t = np.zeros(mesh[0].size, CASE)
    for k, m in zip(names, mesh):
        if k == "size":
            sz = np.asarray(SIZES, np.uint64)[m.ravel()]
            t["entries"], t["N"] = sz[:, 0], sz[:, 1]
        else:
            t[k] = m.ravel()
    return t


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(the table, the program's plans): built and run once for every test of the module"""
    d = tmp_path_factory.mktemp("gather")
    exe, fin, fout = str(d / "lh_gather_check"), str(d / "in.bin"), str(d / "out.bin")
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


# ---- the expressions again, from ao_region and ao_batch_device as they were ----------------------------------------------------------------------

def _tile(c):
    """const bool fused = a->ao_fused && !d_uniforms;
    const bool late = fused && S * N < 2^31 && (dirt ? S * N <= LH_DIRT_LATE_MAX : env ? S * N <= LH_ENV_LATE_MAX : !a->dev.ao_group) &&
                      !getenv("LH_AO_SYNC") && !(sun && S > LH_SUN_LATE_MAX);"""
    S, rays = c["entries"], c["entries"] * c["N"]
    dirt, env = c["kind"] == DIRT, c["kind"] == ENV
    fused = (c["ao_fused"] != 0) & (c["uniforms"] == 0)
    by_kind = np.where(dirt, rays <= DIRT_LATE_MAX, np.where(env, rays <= ENV_LATE_MAX, c["ao_group"] == 0))
    late = fused & (rays < (1 << 31)) & by_kind & (c["sync"] == 0) & ~((c["sun"] != 0) & (S > SUN_LATE_MAX))
    return fused, late


def _batch(c):
    """const bool fused = a->ao_fused && !d_uniforms && L * N < 2^31 && (dirt || env || !a->dev.ao_group);
    const bool late = fused && (!dirt || L * N <= LH_DIRT_LATE_MAX) && (!env || L * N <= LH_ENV_LATE_MAX) && !(sun && L > LH_SUN_LATE_MAX);"""
    L, rays = c["entries"], c["entries"] * c["N"]
    dirt, env = c["kind"] == DIRT, c["kind"] == ENV
    fused = (c["ao_fused"] != 0) & (c["uniforms"] == 0) & (rays < (1 << 31)) & (dirt | env | (c["ao_group"] == 0))
    late = fused & (~dirt | (rays <= DIRT_LATE_MAX)) & (~env | (rays <= ENV_LATE_MAX)) & ~((c["sun"] != 0) & (L > SUN_LATE_MAX))
    return fused, late


def _expected(t):
    c = {k: t[k].astype(np.int64) for k in CASE.names}
    tf, tl = _tile(c)
    bf, bl = _batch(c)
    tile = c["where"] == TILE
    return np.where(tile, tf, bf), np.where(tile, tl, bl)


def test_plans_agree_with_the_restated_expressions(plans):
    t, out = plans
    fused, late = _expected(t)
    for k, e in (("fused", fused), ("late", late)):
        bad = np.flatnonzero((out[k] != 0) != e)
        assert bad.size == 0, (k, bad.size, t[bad[:3]], out[bad[:3]])
    assert np.all(out["fused"] <= 1) and np.all(out["late"] <= out["fused"])          # late is a way of running fused


def test_the_table_crosses_every_edge(plans):
    """each clause of either expression decides at least one row: flipping that input alone flips the plan"""
    t, out = plans
    rays = t["entries"] * t["N"]
    for lim in (DIRT_LATE_MAX, ENV_LATE_MAX, (1 << 31) - 1):
        assert (rays == lim).any() and (rays == lim + 1).any()
    for e in (SUN_LATE_MAX, SUN_LATE_MAX + 1):
        assert ((t["entries"] == e) & (t["sun"] == 1)).any() and ((t["entries"] == e) & (t["sun"] == 0)).any()
    late, fused = out["late"] != 0, out["fused"] != 0
    ok = (t["ao_fused"] == 1) & (t["uniforms"] == 0) & (t["ao_group"] == 0) & (t["sync"] == 0) & (t["sun"] == 0)
    for kind, lim in ((DIRT, DIRT_LATE_MAX), (ENV, ENV_LATE_MAX), (AO, (1 << 31) - 1)):
        for where in (TILE, BATCH):
            m = ok & (t["kind"] == kind) & (t["where"] == where)
            assert late[m & (rays == lim)].all() and not late[m & (rays == lim + 1)].any(), (kind, where)
            assert fused[m & (rays == lim + 1)].all() or (kind == AO and where == BATCH)
    # the sun's list: late at 2^30 slots, not beyond -- seen where nothing else forbids late (AO-sized limits: kind AO, N = 1)
    m = (t["ao_fused"] == 1) & (t["uniforms"] == 0) & (t["ao_group"] == 0) & (t["sync"] == 0) & (t["kind"] == AO) & (t["N"] == 1)
    assert late[m & (t["entries"] == SUN_LATE_MAX + 1) & (t["sun"] == 0)].all() and not late[m & (t["entries"] == SUN_LATE_MAX + 1) & (t["sun"] == 1)].any()
    assert late[m & (t["entries"] == SUN_LATE_MAX) & (t["sun"] == 1)].all()
    # the callers' differences
    small = (t["ao_fused"] == 1) & (t["uniforms"] == 0) & (t["entries"] == 1024) & (t["sun"] == 0)
    grouped = small & (t["kind"] == AO) & (t["ao_group"] != 0)
    assert fused[grouped & (t["where"] == TILE)].all() and not late[grouped & (t["where"] == TILE)].any()          # a tile: fused, the count read first
    assert not fused[grouped & (t["where"] == BATCH)].any()                                                        # a batch: materialised
    assert fused[small & (t["kind"] != AO) & (t["ao_group"] != 0)].all()                                           # the grouped order is the AO kernel's alone
    sync = small & (t["ao_group"] == 0) & (t["sync"] == 1)
    assert not late[sync & (t["where"] == TILE)].any() and late[sync & (t["where"] == BATCH)].all()               # only a tile consults the request
    big = (t["ao_fused"] == 1) & (t["uniforms"] == 0) & (rays == (1 << 31))
    assert fused[big & (t["where"] == TILE)].all() and not fused[big & (t["where"] == BATCH)].any()
    assert not fused[(t["ao_fused"] == 0) | (t["uniforms"] == 1)].any()
