"""tests/tree_check.py proven on the CPU: the host builder's 4- and 8-wide trees of a 3 000-triangle soup pass, and every single corruption a
subtly wrong builder could leave is reported by the invariant that names it, with the node and the slot.  This is what shows that
tests/test_gpu_tree_image.py, which runs the same checker on the trees the device holds, would fail on such a builder."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import tree_check as tc
from tests.helpers import Model

NTRI = 3000


class Soup:
    def __init__(self):
        P, idx, _, _ = po.soup(NTRI, 1, 0.02, 20261)
        self.tris = P[idx].reshape(-1, 3, 3)
        m = Model(P, idx)
        self.tri32 = tc.as_tri32(m.tri32())
        self.lo, self.step = m.grid()
        self.nodes = {4: tc.split_nodes(m.q4nodes(), 4), 8: tc.split_nodes(m.q8nodes(), 8)}
        self.depth = {4: m.q4info()[1], 8: m.q8info()[1]}
        assert m.q4info()[0] == self.nodes[4][1].shape[0] and m.q8info()[0] == self.nodes[8][1].shape[0]

    def check(self, width, words=None, refs=None, tri32=None, depth=None, stack=None, device_built=False, tol=0.0):
        w0, r0 = self.nodes[width]
        nodes = np.concatenate([(w0 if words is None else words).reshape(len(r0), -1), (r0 if refs is None else refs).view(np.uint32)], axis=1)
        return tc.check_tree(nodes, width, self.tri32 if tri32 is None else tri32, self.tris, self.lo, self.step, NTRI,
                             self.depth[width] if depth is None else depth, stack=stack, device_built=device_built, tol=tol)


@pytest.fixture(scope="module")
def soup():
    return Soup()


def leaf_range(ref):
    x = (~int(ref)) & 0xFFFFFFFF
    return x >> 2, (x & 3) + 1


@pytest.mark.parametrize("width", [4, 8])
def test_the_host_builders_trees_pass_at_zero_tolerance(soup, width):
    """... which is itself a finding about lh_bvh.c: its decoded 16-bit boxes contain the fp64 vertices exactly, without the 1e-12 that
    tests/test_bvh_builder.py grants.  The declared depth of a host-built tree is its level count; it declares no stack rows (0)"""
    got = soup.check(width, stack=0 if width == 4 else None)
    assert got["levels"] == soup.depth[width] and got["nleaves"] >= NTRI // 4
    assert (got["npad"] > 0) == (width == 4)            # only the 4-wide tree moves sibling groups onto 128-byte lines
    assert 0 < got["need"] <= (width - 1) * (got["levels"] - 1)
    tc.check_records(soup.tri32, None, soup.tris, NTRI)
    # the figure of a builder that counts: the recomputed one + 5 passes as a bound and as the device builder's own definition
    if width == 4:
        soup.check(4, stack=got["need"] + 5, device_built=True)
        soup.check(4, stack=got["need"] + 9)


@pytest.mark.parametrize("width", [4, 8])
def test_a_box_code_moved_inward_by_one_is_detected(soup, width):
    """twenty faces of leaf boxes, each moved one grid code inward on its own: the builder's codes are the tightest that hold (lh_bvh.c and
    lh_build.hip quantise outward, then step back while the plane still holds), so every one of them cuts a vertex off"""
    words, refs = soup.nodes[width]
    rng = np.random.default_rng(5)
    ln, ls = np.nonzero((refs < 0) & (refs != tc.EMPTY))
    for i in rng.choice(len(ln), 20, replace=False):
        k, s, ax, upper = int(ln[i]), int(ls[i]), int(rng.integers(3)), bool(rng.integers(2))
        w = words.copy()
        lo, hi = int(w[k, s, ax]) & 0xFFFF, int(w[k, s, ax]) >> 16
        if upper:
            hi -= 1
        else:
            lo += 1
        if hi < 0 or lo > 65535:
            continue
        w[k, s, ax] = lo | (hi << 16)
        with pytest.raises(tc.TreeError) as e:
            soup.check(width, words=w)
        assert (e.value.invariant, e.value.node, e.value.slot) == ("boxes.child", k, s), str(e.value)
        assert "axis %d" % ax in str(e.value)
    # an inner child's box too: the first inner slot of the root
    s = int(np.flatnonzero(refs[0] >= 0)[0])
    w = words.copy(); w[0, s, 0] += 1
    with pytest.raises(tc.TreeError) as e:
        soup.check(width, words=w)
    assert (e.value.invariant, e.value.node, e.value.slot) == ("boxes.child", 0, s)


@pytest.mark.parametrize("width", [4, 8])
def test_a_leaf_count_raised_by_one_is_detected(soup, width):
    _, refs = soup.nodes[width]
    ln, ls = np.nonzero((refs < 0) & (refs != tc.EMPTY))
    k, s = next((int(a), int(b)) for a, b in zip(ln, ls) if leaf_range(refs[a, b])[1] < 4 and sum(leaf_range(refs[a, b])) < NTRI)
    first, cnt = leaf_range(refs[k, s])
    r = refs.copy(); r[k, s] = ~np.int32((first << 2) | cnt)            # count - 1 + 1
    assert leaf_range(r[k, s]) == (first, cnt + 1)
    with pytest.raises(tc.TreeError) as e:
        soup.check(width, refs=r)
    assert e.value.invariant == "leaves.tiling" and "overlaps" in str(e.value)
    assert "node %d slot %d" % (k, s) in str(e.value)                   # named as the range the neighbour runs into


@pytest.mark.parametrize("width", [4, 8])
def test_a_leaf_duplicated_into_an_empty_slot_is_detected(soup, width):
    _, refs = soup.nodes[width]
    isleaf = (refs < 0) & (refs != tc.EMPTY)
    k = int(np.flatnonzero(isleaf.any(1) & (refs == tc.EMPTY).any(1))[0])
    s_leaf, s_empty = int(np.flatnonzero(isleaf[k])[0]), int(np.flatnonzero(refs[k] == tc.EMPTY)[0])
    r = refs.copy(); r[k, s_empty] = r[k, s_leaf]
    with pytest.raises(tc.TreeError) as e:
        soup.check(width, refs=r)
    assert e.value.invariant == "leaves.tiling" and e.value.node == k and e.value.slot in (s_leaf, s_empty)


@pytest.mark.parametrize("width", [4, 8])
def test_an_inner_reference_pointed_at_a_sibling_is_detected(soup, width):
    _, refs = soup.nodes[width]
    k = int(np.flatnonzero((refs >= 0).sum(1) >= 2)[3])
    s0, s1 = (int(x) for x in np.flatnonzero(refs[k] >= 0)[:2])
    r = refs.copy(); r[k, s1] = r[k, s0]
    with pytest.raises(tc.TreeError) as e:
        soup.check(width, refs=r)
    assert (e.value.invariant, e.value.node, e.value.slot) == ("shape.once", k, s0)


def test_a_reference_to_a_padding_record_is_detected(soup):
    """(the 4-wide tree: sibling groups start on 128-byte lines, the records skipped are padding; the 8-wide tree has none)"""
    _, refs = soup.nodes[4]
    pads = np.flatnonzero((refs == tc.EMPTY).all(1))
    assert len(pads) > 0
    p = int(pads[-1])
    k = int(np.flatnonzero((refs[:p] == tc.EMPTY).any(1) & ~(refs[:p] == tc.EMPTY).all(1))[-1])
    s = int(np.flatnonzero(refs[k] == tc.EMPTY)[0])
    r = refs.copy(); r[k, s] = p
    with pytest.raises(tc.TreeError) as e:
        soup.check(4, refs=r)
    assert (e.value.invariant, e.value.node, e.value.slot) == ("shape.padding", k, s)
    # ... and a padding record that is not hollow, or a record that lost its parent
    w = soup.nodes[4][0].copy(); w[p, 2, 1] = 7
    with pytest.raises(tc.TreeError) as e:
        soup.check(4, words=w)
    assert (e.value.invariant, e.value.node) == ("shape.unreferenced", p)
    k = int(np.flatnonzero((refs >= 0).any(1))[5]); s = int(np.flatnonzero(refs[k] >= 0)[0])
    r = refs.copy(); lost = int(r[k, s]); r[k, s] = tc.EMPTY
    with pytest.raises(tc.TreeError) as e:
        soup.check(4, refs=r)
    assert (e.value.invariant, e.value.node) == ("shape.unreferenced", lost)


def test_two_equal_primitive_ids_are_detected(soup):
    t = soup.tri32.copy(); t["prim"][1234] = t["prim"][77]
    with pytest.raises(tc.TreeError) as e:
        tc.check_records(t, None, soup.tris, NTRI)
    assert e.value.invariant == "leaves.perm" and "[77, 1234]" in str(e.value)


def test_the_other_record_rules_are_detected(soup):
    t = soup.tri32.copy(); t["e1"][5, 1] = np.nextafter(t["e1"][5, 1], np.float32(9))
    with pytest.raises(tc.TreeError) as e:
        tc.check_records(t, None, soup.tris, NTRI)
    assert e.value.invariant == "records.tri32" and "position 5" in str(e.value)
    t = soup.tri32.copy(); t["ne2"][9] *= np.float32(0.999)
    with pytest.raises(tc.TreeError) as e:
        tc.check_records(t, None, soup.tris, NTRI)
    assert e.value.invariant == "records.tri32"
    t64 = soup.tris.copy(); t64[100, 2, 0] = np.nextafter(t64[100, 2, 0], 9.0)
    with pytest.raises(tc.TreeError) as e:
        tc.check_records(soup.tri32, t64, soup.tris, NTRI)
    assert e.value.invariant == "records.tri64" and "primitive 100" in str(e.value)
    with pytest.raises(tc.TreeError) as e:            # a live triangle behind nlive
        tc.check_records(soup.tri32, None, soup.tris, NTRI - 1)
    assert e.value.invariant == "leaves.dead"
    hi = soup.tris.reshape(-1, 3).max(0).astype(np.float32)
    with pytest.raises(tc.TreeError) as e:            # the scene box rounded to nearest, not outward, on the axis where that falls short
        tc.check_records(soup.tri32, None, soup.tris, NTRI, bmin=np.float32([-9, -9, -9]), bmax=np.nextafter(hi, np.float32(-9)))
    assert e.value.invariant == "boxes.scene"
    with pytest.raises(tc.TreeError) as e:
        tc.check_records(soup.tri32, None, soup.tris, NTRI, bmin=np.float32([-9, -9, -9]), bmax=np.float32([9, 9, 9]), scene_r=0.5)
    assert e.value.invariant == "boxes.scene"


def test_a_dead_triangle_inside_the_tree_is_detected(soup):
    """a primitive with v0 == v1 belongs behind nlive when the drop applies"""
    tris = soup.tris.copy(); p = int(soup.tri32["prim"][10]); tris[p, 1] = tris[p, 0]
    t = soup.tri32.copy(); t["e1"][10] = 0; t["ne1"][10] = 0
    with pytest.raises(tc.TreeError) as e:
        tc.check_records(t, None, tris, NTRI)
    assert e.value.invariant == "leaves.dead" and "primitive %d " % p in str(e.value)


def test_a_declared_stack_figure_lowered_by_one_is_detected(soup):
    need = soup.check(4)["need"]
    for device_built in (False, True):
        with pytest.raises(tc.TreeError) as e:
            soup.check(4, stack=need + 4, device_built=device_built)
        assert e.value.invariant == "stack.rows"
    with pytest.raises(tc.TreeError) as e:            # the device builder's figure is its own count: one too many is wrong as well
        soup.check(4, stack=need + 6, device_built=True)
    assert e.value.invariant == "stack.rows"


@pytest.mark.parametrize("width", [4, 8])
def test_a_declared_depth_lowered_by_one_is_detected(soup, width):
    with pytest.raises(tc.TreeError) as e:
        soup.check(width, depth=soup.depth[width] - 1)
    assert e.value.invariant == "stack.depth"


def test_the_recomputed_stack_need_is_the_walks(soup):
    """the definition, by the slow way round: a depth-first walk that pushes every child but the one it descends into holds, when it steps at a
    node, (children - 1) entries per ancestor"""
    for width in (4, 8):
        _, refs = soup.nodes[width]
        best, stack = 0, [(0, 0)]
        while stack:
            k, held = stack.pop()
            best = max(best, held)
            nch = int((refs[k] != tc.EMPTY).sum())
            stack.extend((int(r), held + nch - 1) for r in refs[k] if r >= 0)
        assert soup.check(width)["need"] == best
