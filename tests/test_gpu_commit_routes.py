"""What a commit does when its device build does not end in a scene (lucille_amd/csrc/lh_route.h; lh_commit.hip device_upload): the rows of the
route table a test can reach through the binding, on the 300-triangle "exponential line" of tests/test_gpu_recommit.py with "build_depth_cap" lowered
to the depth of a soup of as many triangles, so that the line's device-built tree is "too deep".  Whatever route a commit took, the accelerator must be
the one the host builders make: the same info(), hit records bit-equal to it and to oracle.pyoracle, lucille's own tree byte for byte, the same state
records.  Every case is run five times, device memory measured around the last three (the method and the allowance of
tests/test_gpu_devbuild.py::test_device_commit_does_not_leak_device_memory): a fallback frees what the device builders made.  Three sides of the
300-triangle line are some 300 KB, which that allowance (16 MB) cannot see; so each case is run five times more on a soup of 150 000 triangles
with the cap one level under its device-built depth -- a side of it is above 50 MB with its trees, 10.8 MB as bare triangle records (the NaN case of
device meshes), so three that leaked are 32 MB at the least.

  - host meshes, the device asked for: too deep -> the host builders;
  - host meshes, the device chosen by the scene's size (LH_AUTO_DEVICE_TRIANGLES lowered): the same, also with per-vertex normals;
  - device meshes with normals and a colour: the fallback carries the gathered arrays (tests/test_gpu_device_attr.py
    test_the_deep_tree_keeps_its_attributes names this path but does not lower the cap: its tree is device-built nowadays);
  - a NaN vertex on the device path, host meshes and device meshes: the error, and an accelerator that refuses a second commit;
  - the 8-wide nodes of a device-built scene asked for after the commit: the build run once more, only its 8-wide collapse installed.

Not reachable from the binding: the replica row with a lowered cap (HipMulti has no set_param on its replicas before their commit), the limit of a
32-bit byte offset on the 4-wide nodes (some 10^8 triangles), and a builder that fails for lack of memory."""
import numpy as np
import pytest

import lucille_amd as la
from oracle import pyoracle as po
from tests.helpers import assert_hits_equal
from tests.test_gpu_recommit import dev_idx, dev_pos, line_and_soup

pytestmark = pytest.mark.gpu

INFO_KEYS = ("ntriangles", "ntriangles_in_tree", "nnodes_traversal", "nnodes", "max_depth", "nleaves")
NAN_VERTEX = "a vertex coordinate is NaN, infinite or beyond 1e30"


def host_accel(P, idx, N=None, C=None):
    acc = la.HipAccel(0); acc.add_mesh(P, idx)
    if N is not None:
        acc.set_normals(0, N)
    if C is not None:
        acc.set_attribute(0, la.ATTR_COLOR, C)
    return acc


def records(acc, org, dr):
    """closest hits, any hits and the state records of the host batch path"""
    hit = acc.intersect_host(org, dr)
    return hit, acc.intersect_host(org, dr, mode=la.MODE_ANY).astype(bool), acc.state_build(org, dr, *hit)


@pytest.fixture(scope="module")
def line():
    """the line, its rays, the cap; the oracle's records; what the host builders make of it without attributes, with normals, with normals and a colour"""
    E, org, dr, _, _, _, idx, cap = line_and_soup()
    rng = np.random.default_rng(17)
    N = rng.normal(size=E.shape); N /= np.linalg.norm(N, axis=1, keepdims=True)
    C = rng.uniform(0, 1, E.shape)
    o = po.Oracle(); o.add_mesh(E, idx); o.build()
    exp = o.intersect(org, dr, nthreads=8)
    assert (exp[0] != po.MISS).sum() > 100
    want = {}
    for key, (n, c) in {"plain": (None, None), "normals": (N, None), "colour": (N, C)}.items():
        acc = host_accel(E, idx, n, c)
        info = acc.commit(build="host")
        want[key] = (info, records(acc, org, dr), acc.ref_tree())
        assert_hits_equal(want[key][1][0], exp, "the host-built accelerator against the oracle")
        acc.close()
    # the fallback is visible in info(): the tree the device builders make of the line is another one than the host builders'
    acc = host_accel(E, idx); dinfo = acc.commit(build="device"); acc.close()
    assert dinfo["max_depth"] > cap and any(dinfo[k] != want["plain"][0][k] for k in INFO_KEYS), (dinfo, want["plain"][0])
    return dict(E=E, idx=idx, org=org, dr=dr, cap=cap, N=N, C=C, exp=exp, want=want)


@pytest.fixture(scope="module")
def big():
    """the soup of the leak loops: 150 000 triangles, the cap one level under the depth of its device-built tree, what the host builders make of it"""
    P, idx, _, _ = po.soup(150000, 10, 0.01, 6300)
    rng = np.random.default_rng(18)
    N = rng.normal(size=P.shape); N /= np.linalg.norm(N, axis=1, keepdims=True)
    acc = host_accel(P, idx); dinfo = acc.commit(build="device"); acc.close()
    acc = host_accel(P, idx); hinfo = acc.commit(build="host"); acc.close()
    assert dinfo["max_depth"] >= 2 and any(dinfo[k] != hinfo[k] for k in INFO_KEYS), (dinfo, hinfo)
    return dict(E=P, idx=idx, cap=dinfo["max_depth"] - 1, N=N, C=rng.uniform(0, 1, P.shape), host_info=hinfo)


def check_fell_back(acc, info, scene, key, what):
    """the line: everything against the host-built accelerator and the oracle; the soup of the leak loop: the host builders' tree"""
    if "want" in scene:
        check_like_host_built(acc, info, scene, key, what)
    else:
        assert all(info[k] == scene["host_info"][k] for k in INFO_KEYS), (what, info, scene["host_info"])


def check_like_host_built(acc, info, line, key, what):
    winfo, (whit, wany, wstate), (wnodes, wprims) = line["want"][key]
    assert all(info[k] == winfo[k] for k in INFO_KEYS), (what, info, winfo)          # the host builders' tree: the commit fell back
    hit, anyhit, state = records(acc, line["org"], line["dr"])
    assert_hits_equal(hit, line["exp"], what + ": against the oracle")
    assert_hits_equal(hit, whit, what + ": against the host-built accelerator")
    assert np.array_equal(anyhit, line["exp"][0] != po.MISS) and np.array_equal(anyhit, wany), what + ": any hit"
    assert state.tobytes() == wstate.tobytes(), what + ": state records"
    nodes, prims = acc.ref_tree()
    assert nodes.tobytes() == wnodes.tobytes() and np.array_equal(prims, wprims), what + ": lucille's own tree"


def five_times_without_a_leak(once):
    import torch
    once(); once()                                    # allocator pools, code objects
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 16 << 20, "device memory shrank by %.1f MB over three commits" % ((free0 - free1) / 1e6)


def test_host_meshes_device_asked_for_too_deep(line, big):
    def once(scene):
        acc = host_accel(scene["E"], scene["idx"])
        acc.set_param("build_depth_cap", scene["cap"])
        info = acc.commit(build="device")
        check_fell_back(acc, info, scene, "plain", "device asked for, too deep")
        acc.close()
    five_times_without_a_leak(lambda: once(line))
    five_times_without_a_leak(lambda: once(big))


@pytest.mark.parametrize("key", ["plain", "normals"])
def test_host_meshes_device_chosen_by_size_too_deep(line, big, key, monkeypatch):
    monkeypatch.setenv("LH_AUTO_DEVICE_TRIANGLES", "100")
    monkeypatch.delenv("LH_BUILD", raising=False)

    def once(scene):
        acc = host_accel(scene["E"], scene["idx"], scene["N"] if key == "normals" else None)
        acc.set_param("build_depth_cap", scene["cap"])
        info = acc.commit(build_threads=0)
        check_fell_back(acc, info, scene, key, "device chosen by size, too deep (%s)" % key)
        acc.close()
    five_times_without_a_leak(lambda: once(line))
    five_times_without_a_leak(lambda: once(big))
    # the device builders were on the way: without the lowered cap the same call ends in the tree they make when asked for, deeper than the cap
    acc = host_accel(line["E"], line["idx"]); info = acc.commit(build_threads=0); acc.close()
    ref = host_accel(line["E"], line["idx"]); rinfo = ref.commit(build="device"); ref.close()
    assert info["max_depth"] > line["cap"] and all(info[k] == rinfo[k] for k in INFO_KEYS), (info, rinfo)


def test_device_meshes_too_deep_carry_their_attributes(line, big):
    def once(scene, tensors):
        acc = la.HipAccel(0)
        acc.add_mesh_device(tensors[0], tensors[1])
        acc.set_normals_device(0, tensors[2])
        acc.set_attribute_device(0, la.ATTR_COLOR, tensors[3])
        acc.set_param("build_depth_cap", scene["cap"])
        info = acc.commit()
        check_fell_back(acc, info, scene, "colour", "device meshes, too deep")
        acc.close()
    for scene in (line, big):          # the tensors are made once: only the accelerator's own memory is measured
        tensors = (dev_pos(scene["E"]), dev_idx(scene["idx"]), dev_pos(scene["N"]), dev_pos(scene["C"]))
        five_times_without_a_leak(lambda: once(scene, tensors))
    hit = line["exp"][0] != po.MISS
    state = line["want"]["colour"][1][2]
    assert np.abs(state[hit][:, 15:18]).sum() > 0 and state[hit][:, 6:9].tobytes() != state[hit][:, 3:6].tobytes()      # the colour is there, Ns is not Ng


@pytest.mark.parametrize("source", ["host meshes", "device meshes"])
def test_a_nan_vertex_on_the_device_path(line, big, source):
    def once(E, idx):
        acc = la.HipAccel(0)
        if source == "host meshes":
            acc.add_mesh(E, idx)
        else:
            acc.add_mesh_device(E, idx)
        with pytest.raises(la.LucilleHipError, match=NAN_VERTEX):
            acc.commit(build="device")
        with pytest.raises(la.LucilleHipError, match="create a new one"):
            acc.commit(build="device")
        acc.close()
    for scene in (line, big):
        E = scene["E"].copy(); E[451, 1] = np.nan
        arrays = (E, scene["idx"]) if source == "host meshes" else (dev_pos(E), dev_idx(scene["idx"]))
        five_times_without_a_leak(lambda: once(*arrays))


@pytest.mark.parametrize("ntri", [1, 300])
def test_eight_wide_nodes_asked_for_after_the_commit(ntri):
    """1 triangle: a tree of one node has no 8-wide form (lh_ensure_formats does not ask); 300: the second run of the builder"""
    P, idx, org, dr = po.soup(ntri, 20000, 0.2 if ntri == 1 else 0.08, 6200)
    o = po.Oracle(); o.add_mesh(P, idx); o.build()
    exp = o.intersect(org, dr, nthreads=8)
    got = []
    for wide8 in (-1, 1):
        acc = la.HipAccel(0); acc.add_mesh(P, idx); acc.set_param("wide8", wide8)
        acc.commit(build="device"); acc.wait_exact()
        if wide8 == -1:
            assert acc.dump_node_bytes() == 64 or ntri == 1
            acc.set_param("wide8", 1)
        hit = acc.intersect_host(org, dr)               # the ray dump that needs them
        assert_hits_equal(hit, exp, "wide8 %d at the commit, %d triangles" % (wide8, ntri))
        info = acc.info()
        got.append((hit, {k: info[k] for k in INFO_KEYS + ("device_bytes",)}, acc.dump_node_bytes()))
        acc.close()
    assert_hits_equal(got[0][0], got[1][0], "asked for after the commit against asked for before it")
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2], got
    if ntri > 16:
        assert got[0][2] == 128
