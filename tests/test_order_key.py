"""The bin order of ray dumps (lucille_amd/csrc/lh_order.h) on the CPU: the header, compiled into the stand-alone program
tests/cpu_model/lh_order_check.c with -fsanitize=address,undefined, against numpy -- a ray's key (the Morton code of the origin's clamped cell, with or without
the direction octant by sign bit above it), the run table (counts and offsets per block and bin) and every ray's destination, which
is its place in numpy.argsort(key, kind="stable"); dest is a permutation.  Rays: -0.0 / +0.0 and denormal directions, origins on, outside
and far outside the bounds, NaN and infinite coordinates (tests/order_cases.py); all rays in one bin; n = one block, one block + 1, 1."""
import os
import subprocess

import numpy as np
import pytest

from tests.order_cases import edge_rays, one_bin_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_model", "lh_order_check.c")
LO = np.array([-1.5, 0.25, 10.0], np.float32)
STEP = (np.array([3.0, 0.5, 7.0]) / 65535.0 * (1.0 + 1e-6)).astype(np.float32)          # the 16-bit grid of a box of that size (lh_bvh.c)
KEYS = [(0, 1), (1, 1), (2, 1), (1, 0), (2, 0), (3, 0)]          # (cell bits per axis, octant): keys of 3, 6 and 9 bits
BLOCK = {3: 4096, 6: 4096, 9: 32768}          # by key bits; 48 rays or more in an average run: 512 bins grow the block


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("order") / "lh_order_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           SRC, "-o", exe])
    return exe


def _run(program, tmp_path, org, dr, bits, octant):
    n = org.shape[0]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint64(n).tobytes()); f.write(np.array([bits, octant], np.uint32).tobytes()); f.write(LO.tobytes()); f.write(STEP.tobytes())
        f.write(np.ascontiguousarray(org, np.float64).tobytes()); f.write(np.ascontiguousarray(dr, np.float64).tobytes())
    r = subprocess.run([program, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr          # a sanitizer report ends the program with a message
    raw = np.fromfile(fout, np.uint32)
    nblocks, nbins, block = (int(x) for x in raw[:3])
    at = 4
    key = raw[at:at + n]; at += n
    dest = raw[at:at + n]; at += n
    counts = raw[at:at + nblocks * nbins].reshape(nblocks, nbins); at += nblocks * nbins
    offset = raw[at:at + nblocks * nbins].reshape(nblocks, nbins); at += nblocks * nbins
    plan = raw[at:].view(np.uint64)
    assert plan.shape == (15,)
    return nblocks, nbins, block, key, dest, counts, offset, plan


def _expected_key(org, dr, bits, octant):
    top = float(1 << bits)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (org - LO.astype(np.float64)) * (top / (65535.0 * STEP.astype(np.float64)))
        inside = (f >= 0.0) & (f < top)
        cell = np.where(inside, np.floor(np.where(inside, f, 0.0)), np.where(f >= top, top - 1.0, 0.0)).astype(np.uint32)      # NaN: neither comparison holds -> 0
    m = np.zeros(org.shape[0], np.uint32)
    for b in range(bits):
        for a in range(3):
            m |= ((cell[:, a] >> b) & 1) << np.uint32(3 * b + a)
    sign = np.signbit(dr).astype(np.uint32)
    return ((sign[:, 0] | (sign[:, 1] << 1) | (sign[:, 2] << 2)) << np.uint32(3 * bits)) | m if octant else m


def _check(program, tmp_path, org, dr, bits, octant):
    n = org.shape[0]; kb = 3 * bits + 3 * octant
    nblocks, nbins, block, key, dest, counts, offset, plan = _run(program, tmp_path, org, dr, bits, octant)
    assert (nbins, block, nblocks) == (1 << kb, BLOCK[kb], -(-n // BLOCK[kb]))
    exp = _expected_key(org, dr, bits, octant)
    assert np.array_equal(key, exp)
    assert int(key.max()) < nbins
    blk = np.arange(n) // block
    exp_counts = np.zeros((nblocks, nbins), np.uint32)
    np.add.at(exp_counts, (blk, exp), 1)
    assert np.array_equal(counts, exp_counts)
    flat = exp_counts.T.ravel().astype(np.int64)          # bins outermost, blocks within a bin
    exp_offset = (np.cumsum(flat) - flat).reshape(nbins, nblocks).T
    assert np.array_equal(offset, exp_offset)
    order = np.argsort(exp, kind="stable")
    exp_dest = np.empty(n, np.int64); exp_dest[order] = np.arange(n)
    assert np.array_equal(dest, exp_dest)
    assert np.array_equal(np.sort(dest), np.arange(n))          # a permutation
    # the workspace: arrays in turn, none overlapping, each on a 256-byte boundary
    org_o, dir_o, t_o, u_o, v_o, prim_o, dest_o, counts_o, offset_o, tot_o, base_o, size, occ_o, size_any, slot_o = (int(x) for x in plan)
    starts = [org_o, dir_o, t_o, u_o, v_o, prim_o, dest_o, slot_o, counts_o, offset_o, tot_o, base_o, size]
    need = [24 * n, 24 * n, 8 * n, 8 * n, 8 * n, 4 * n, 4 * n, 2 * n, 4 * nblocks * nbins, 4 * nblocks * nbins, 4 * nbins, 4 * nbins]
    assert all(s % 256 == 0 for s in starts) and all(b - a >= w for a, b, w in zip(starts, starts[1:], need))
    assert occ_o == dir_o + (dir_o - org_o) and size_any < size
    return key


@pytest.mark.parametrize("bits,octant", KEYS)
def test_edge_rays(program, tmp_path, bits, octant):
    org, dr = edge_rays(10000, LO.astype(np.float64), LO.astype(np.float64) + 65535.0 * STEP.astype(np.float64), 7 + bits, legal_only=False)
    assert np.isnan(org).any() and np.isinf(org).any() and np.isnan(dr).any() and (dr == 0.0).any()
    key = _check(program, tmp_path, org, dr, bits, octant)
    assert len(np.unique(key)) == 1 << (3 * bits + 3 * octant)          # every bin is met


@pytest.mark.parametrize("bits,octant", KEYS)
def test_all_rays_in_one_bin(program, tmp_path, bits, octant):
    org, dr = one_bin_rays(10000, LO.astype(np.float64), LO.astype(np.float64) + 65535.0 * STEP.astype(np.float64), 3)
    key = _check(program, tmp_path, org, dr, bits, octant)
    assert len(np.unique(key)) == 1


@pytest.mark.parametrize("bits,octant,n", [(2, 0, 1), (2, 0, 4096), (2, 0, 4097), (1, 1, 4096), (1, 1, 4097), (3, 0, 32768), (2, 1, 32769), (0, 1, 4097)])
def test_block_edges(program, tmp_path, bits, octant, n):
    org, dr = edge_rays(n, LO.astype(np.float64), LO.astype(np.float64) + 65535.0 * STEP.astype(np.float64), 100 + n, legal_only=False)
    _check(program, tmp_path, org, dr, bits, octant)
