"""A structural checker for the wide traversal trees on the scene's 16-bit grid (lh_q4node_t / lh_q8node_t, lh_bvh.h), whichever builder
made them: lh_bvh.c on the host or lh_build.hip on the device.  It sees a tree as the walks do -- node words, child references, the leaf-order
triangle records, the grid -- beside the fp64 triangles the scene was made from, and raises TreeError at the first violated invariant, with the
node and the slot where it occurred.  Level by level with numpy: children have larger indices than their parent and every record is referred to
once, so one sweep down the levels (depths, stack rows) and one sweep up (boxes) visit everything; a 70 000-triangle tree takes well under a
second.  tests/test_tree_check.py proves it on the host model's trees, untouched and corrupted; tests/test_gpu_tree_image.py runs it on what
the device holds (lh_accel_tree_image)."""
import numpy as np

EMPTY = -(2 ** 31)            # LH_REF_EMPTY
TRI32 = np.dtype([("v0", "<f4", (3,)), ("e1", "<f4", (3,)), ("e2", "<f4", (3,)), ("prim", "<u4"), ("ne1", "<f4"), ("ne2", "<f4")])      # lh_tri32_t
DEG_S2CAP = 1.0e-14 / (1.0e-15 * 1024.0)      # lh_bvh.c tri_dead_class / lh_build.hip LH_DEG_S2CAP: v1 == v2 is dead up to this squared L1 edge


class TreeError(AssertionError):
    """invariant: the name of the violated invariant ("shape.once", "boxes.child", ...); node / slot: where (None where it has no place)"""

    def __init__(self, invariant, text, node=None, slot=None):
        where = "" if node is None else (" at node %d" % node + ("" if slot is None else " slot %d" % slot))
        super().__init__("[%s]%s: %s" % (invariant, where, text))
        self.invariant, self.node, self.slot = invariant, node, slot


def _first(mask):
    """(node, slot) of the first set element of a [n, width] mask, or None"""
    flat = np.flatnonzero(mask)
    if flat.size == 0:
        return None
    return int(flat[0] // mask.shape[1]), int(flat[0] % mask.shape[1])


def as_tri32(a):
    """lh_tri32_t records as the structured TRI32, from that or from float32 [n, 12]"""
    a = np.ascontiguousarray(a)
    if a.dtype.names is None:
        a = a.reshape(-1, 12).view(TRI32).reshape(-1)
    return a


def split_nodes(nodes, width):
    """(words uint32 [n, width, 3], refs int32 [n, width]) of lh_q4node_t / lh_q8node_t records given as a structured array with the fields
    w and ref, or as flat uint16 / uint32 rows"""
    nodes = np.ascontiguousarray(nodes)
    if nodes.dtype.names is not None:
        return nodes["w"].astype(np.uint32), nodes["ref"].astype(np.int32)
    flat = nodes.view(np.uint32).reshape(-1, 4 * width)
    return flat[:, :3 * width].reshape(-1, width, 3).copy(), flat[:, 3 * width:].view(np.int32).copy()


def dead_classes(tris):
    """(two vertices equal, v0 == v1 or v0 == v2, dead by the builders' rule) per fp64 triangle [n, 3, 3]"""
    e01 = (tris[:, 0] == tris[:, 1]).all(1); e02 = (tris[:, 0] == tris[:, 2]).all(1); e12 = (tris[:, 1] == tris[:, 2]).all(1)
    s = np.abs(tris[:, 1] - tris[:, 0]).sum(1)
    return e01 | e02 | e12, e01 | e02, e01 | e02 | (e12 & (s * s * (1.0 + 1e-9) <= DEG_S2CAP))


def check_records(tri32, tri64, tris, nlive, bmin=None, bmax=None, scene_r=None):
    """invariants of the triangle records and the scene's figures: `leaves.perm`, `leaves.dead`, `records.tri64`, `records.tri32`, `boxes.scene`.
    tris: the scene's fp64 triangles [ntris, 3, 3] in primitive-id order; tri64: the resident copy, or None (the host model keeps none)"""
    tri32 = as_tri32(tri32); tris = np.ascontiguousarray(tris, np.float64).reshape(-1, 3, 3)
    nt = tris.shape[0]
    if tri32.shape[0] != nt:
        raise TreeError("leaves.perm", "%d tri32 records for %d triangles" % (tri32.shape[0], nt))
    if not 0 < nlive <= nt:
        raise TreeError("leaves.dead", "nlive = %d of %d triangles" % (nlive, nt))
    prim = tri32["prim"]
    if (prim >= nt).any():
        i = int(np.flatnonzero(prim >= nt)[0])
        raise TreeError("leaves.perm", "tri32.prim is not a permutation of 0 .. %d: position %d holds %d" % (nt - 1, i, int(prim[i])))
    cnt = np.bincount(prim, minlength=nt)
    if (cnt != 1).any():
        p = int(np.flatnonzero(cnt > 1)[0])
        raise TreeError("leaves.perm", "tri32.prim is not a permutation of 0 .. %d: the positions %s hold primitive %d, nobody holds %s"
                        % (nt - 1, np.flatnonzero(prim == p)[:4].tolist(), p, np.flatnonzero(cnt == 0)[:4].tolist()))
    two_equal, dead1, dead = dead_classes(tris)
    pos_of = np.empty(nt, np.int64); pos_of[prim] = np.arange(nt)
    behind = prim[nlive:]
    if not two_equal[behind].all():
        p = int(behind[~two_equal[behind]][0])
        raise TreeError("leaves.dead", "primitive %d at position %d >= nlive = %d has three different vertices" % (p, int(pos_of[p]), nlive))
    if nt > 4 and not dead.all():            # the drop applies (a scene of one leaf, or of dead triangles only, is built as handed over)
        inside = dead1 & (pos_of < nlive)
        if inside.any():
            p = int(np.flatnonzero(inside)[0])
            raise TreeError("leaves.dead", "primitive %d (v0 == v1 or v0 == v2) sits at position %d < nlive = %d" % (p, int(pos_of[p]), nlive))
    if tri64 is not None:
        t64 = np.ascontiguousarray(tri64, np.float64).reshape(-1, 3, 3)
        if t64.shape != tris.shape or not np.array_equal(t64.view(np.uint64), tris.view(np.uint64)):
            p = 0 if t64.shape != tris.shape else int(np.flatnonzero((t64.view(np.uint64) != tris.view(np.uint64)).any(axis=(1, 2)))[0])
            raise TreeError("records.tri64", "tri64 differs from the input at primitive %d" % p)
    v = tris[prim]
    e1 = v[:, 1] - v[:, 0]; e2 = v[:, 2] - v[:, 0]
    for name, want in (("v0", v[:, 0]), ("e1", e1), ("e2", e2)):
        if not np.array_equal(tri32[name], want.astype(np.float32)):
            i = int(np.flatnonzero((tri32[name] != want.astype(np.float32)).any(1))[0])
            raise TreeError("records.tri32", "%s of position %d (primitive %d) is not the fp64 value rounded once" % (name, i, int(prim[i])))
    for name, e in (("ne1", e1), ("ne2", e2)):
        short = ~(tri32[name].astype(np.float64) >= np.linalg.norm(e, axis=1))
        if short.any():
            i = int(np.flatnonzero(short)[0])
            raise TreeError("records.tri32", "%s of position %d is below the fp64 edge length" % (name, i))
    flat = tris.reshape(-1, 3)
    if bmin is not None:
        lo = np.asarray(bmin, np.float32).astype(np.float64); hi = np.asarray(bmax, np.float32).astype(np.float64)
        if not ((lo <= flat.min(0)).all() and (hi >= flat.max(0)).all()):
            raise TreeError("boxes.scene", "bmin %s / bmax %s do not contain the vertices' %s / %s" % (lo, hi, flat.min(0), flat.max(0)))
    if scene_r is not None and not float(scene_r) >= np.abs(flat).max():
        raise TreeError("boxes.scene", "scene_r %r is below max |coordinate| %r" % (float(scene_r), float(np.abs(flat).max())))


def check_tree(nodes, width, tri32, tris, grid_lo, grid_step, nlive, depth, stack=None, device_built=False, pairs=True, tol=0.0):
    """invariants of one wide tree.  nodes: lh_q4node_t (width 4) or lh_q8node_t (width 8) records (split_nodes takes them); depth: the declared
    level count (q4_depth / q8_depth); stack: the declared q4_stack (width 4), None where there is none (width 8); device_built: the figure is the
    device builder's own count and must EQUAL the recomputed one; pairs: sibling groups of the 4-wide tree sit on 128-byte lines (not under
    LH_Q4_PAIRS=0); tol: what a decoded box may miss a vertex by (0).  Returns {"levels", "need", "npad", "nleaves"}: the measured level
    count (the root alone is 1), the largest sum of (children - 1) over the ancestors of a node, the padding records, the leaves."""
    words, refs = split_nodes(nodes, width)
    tri32 = as_tri32(tri32); tris = np.ascontiguousarray(tris, np.float64).reshape(-1, 3, 3)
    n, nt = refs.shape[0], tris.shape[0]
    if n < 1 or refs.shape[1] != width or words.shape != (n, width, 3):
        raise TreeError("shape.root", "no record 0 (%d records of width %d)" % (n, width))
    idx = np.arange(n)[:, None]
    inner = refs >= 0; empty = refs == EMPTY; leaf = ~inner & ~empty
    lo16 = (words & 0xFFFF).astype(np.int64); hi16 = (words >> 16).astype(np.int64)

    # ---- 1. shape
    at = _first(inner & ((refs < 1) | (refs >= n)))
    if at:
        raise TreeError("shape.range", "inner reference %d outside [1, %d)" % (refs[at], n), *at)
    at = _first(inner & (refs <= idx))
    if at:
        raise TreeError("shape.order", "inner reference %d is not larger than its parent's index" % refs[at], *at)
    times = np.bincount(refs[inner], minlength=n)
    if (times > 1).any():
        k = int(np.flatnonzero(times > 1)[0])
        at = _first(refs == k)
        raise TreeError("shape.once", "record %d is referred to %d times (first here; also by node %s)"
                        % (k, int(times[k]), np.flatnonzero((refs == k).any(1))[1:4].tolist()), *at)
    hollow = empty.all(1)                         # a record without a child: padding, or the corruption of one
    hollow[0] = False                             # (the root is never padding)
    at = _first(inner & hollow[np.where(inner, refs, 0)])
    if at:
        raise TreeError("shape.padding", "reference to the padding record %d" % refs[at], *at)
    pad = times == 0; pad[0] = False
    if (pad & ~hollow).any() or (words[pad] != 65535).any():
        k = int(np.flatnonzero(pad & (~hollow | (words != 65535).any(axis=(1, 2))))[0])
        raise TreeError("shape.unreferenced", "nobody refers to this record and it is not padding (every reference empty, every box word 65535)", k)
    at = _first(empty & ~(lo16 > hi16).all(2))
    if at:
        raise TreeError("shape.empty-box", "an empty slot's box %s is not inverted on every axis" % [hex(int(x)) for x in words[at]], *at)
    ninner = inner.sum(1)
    if width == 4 and pairs:
        big = np.where(inner, refs, n + 1).min(1)
        grp = ninner >= 2
        srt = np.sort(np.where(inner, refs, np.iinfo(np.int32).max), axis=1)
        consecutive = np.ones(n, bool)
        for c in range(1, width):
            consecutive &= (ninner <= c) | (srt[:, c] == srt[:, 0] + c)
        bad = grp & ((big % 2 != 0) | ~consecutive)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise TreeError("shape.pairs", "the sibling group %s is not consecutive from an even index" % refs[k][inner[k]].tolist(), k)

    # ---- levels from the root down: parents, depths, the stack rows a ray holds when it steps at a node
    parent = np.full(n, -1, np.int64); pslot = np.full(n, -1, np.int64)
    pn, ps = np.nonzero(inner)
    parent[refs[pn, ps]] = pn; pslot[refs[pn, ps]] = ps
    nch = (~empty).sum(1)
    held = np.zeros(n, np.int64)
    levels = [np.array([0])]
    while True:
        cur = levels[-1]
        kids = refs[cur][inner[cur]]
        if kids.size == 0:
            break
        held[kids] = held[parent[kids]] + nch[parent[kids]] - 1
        levels.append(kids.astype(np.int64))
        if len(levels) > n:
            raise TreeError("shape.order", "the levels do not end")
    reached = sum(len(l) for l in levels)
    if reached + int(pad.sum()) != n:
        raise TreeError("shape.once", "%d records reached from the root, %d padding, %d in all" % (reached, int(pad.sum()), n))
    real = ~pad
    need = int(held[real].max())

    # ---- 2. leaves
    ln, ls = np.nonzero(leaf)
    x = (~refs[ln, ls]).astype(np.int64) & 0xFFFFFFFF
    first, cnt = x >> 2, (x & 3) + 1
    if ln.size == 0:
        raise TreeError("leaves.tiling", "the tree has no leaf")
    if (cnt > 4).any():
        raise TreeError("leaves.count", "more than 4 triangles in a leaf", int(ln[cnt > 4][0]), int(ls[cnt > 4][0]))
    limit = nlive if nt > 4 else nt
    over = first + cnt > limit
    if over.any():
        i = int(np.flatnonzero(over)[0])
        raise TreeError("leaves.tiling", "the leaf range [%d, %d) ends behind the %d triangles of the tree" % (first[i], first[i] + cnt[i], limit), int(ln[i]), int(ls[i]))
    order = np.argsort(first, kind="stable")
    f, c = first[order], cnt[order]
    clash = np.flatnonzero(f[1:] < f[:-1] + c[:-1])
    if clash.size:
        i, j = int(order[clash[0]]), int(order[clash[0] + 1])
        raise TreeError("leaves.tiling", "the leaf range [%d, %d) overlaps [%d, %d) of node %d slot %d"
                        % (first[j], first[j] + cnt[j], first[i], first[i] + cnt[i], int(ln[i]), int(ls[i])), int(ln[j]), int(ls[j]))
    if nt > 4:            # (a scene of one leaf is built as it was handed over)
        gap = np.flatnonzero(f[1:] > f[:-1] + c[:-1])
        if f[0] != 0 or gap.size or f[-1] + c[-1] != nlive:
            i = int(order[0]) if f[0] != 0 else (int(order[gap[0] + 1]) if gap.size else int(order[-1]))
            raise TreeError("leaves.tiling", "the leaf ranges leave a gap in [0, %d): next to [%d, %d)" % (nlive, first[i], first[i] + cnt[i]), int(ln[i]), int(ls[i]))

    # ---- 3. boxes, from the leaves up: the decoded box of a child contains the fp64 vertices of every triangle below it
    g = np.asarray(grid_lo, np.float32).astype(np.float64); st = np.asarray(grid_step, np.float32).astype(np.float64)
    blo = g + lo16.astype(np.float64) * st; bhi = g + hi16.astype(np.float64) * st          # as lh_build.hip quant_axis states it
    v = tris[tri32["prim"]]
    pmin, pmax = v.min(1), v.max(1)                # per position of the leaf order
    smin = np.full((n, width, 3), np.inf); smax = np.full((n, width, 3), -np.inf)
    lmin = np.full((ln.size, 3), np.inf); lmax = np.full((ln.size, 3), -np.inf)
    for k in range(4):
        m = cnt > k
        lmin[m] = np.minimum(lmin[m], pmin[first[m] + k]); lmax[m] = np.maximum(lmax[m], pmax[first[m] + k])
    smin[ln, ls] = lmin; smax[ln, ls] = lmax
    for cur in levels[:0:-1]:
        smin[parent[cur], pslot[cur]] = smin[cur].min(1); smax[parent[cur], pslot[cur]] = smax[cur].max(1)
    miss = ~empty & real[:, None] & ~((blo <= smin + tol) & (bhi >= smax - tol)).all(2)
    at = _first(miss)
    if at:
        ax = int(np.flatnonzero(~((blo[at] <= smin[at] + tol) & (bhi[at] >= smax[at] - tol)))[0])
        raise TreeError("boxes.child", "axis %d: the decoded box [%.17g, %.17g] (codes %d, %d) does not contain [%.17g, %.17g] of the vertices below"
                        % (ax, blo[at][ax], bhi[at][ax], lo16[at][ax], hi16[at][ax], smin[at][ax], smax[at][ax]), *at)

    # ---- 5. the declared figures
    nlev = len(levels)
    if depth < nlev:
        raise TreeError("stack.depth", "declared depth %d, the tree has %d levels" % (depth, nlev))
    if stack is not None and stack != 0 and (stack != need + 5 if device_built else stack < need + 5):
        raise TreeError("stack.rows", "declared stack rows %d, the deepest path holds %d + 5" % (stack, need))
    return {"levels": nlev, "need": need, "npad": int(pad.sum()), "nleaves": int(ln.size)}


# ---- the rows a launch walks with (lh_plan.h), in Python: what the stack figures are FOR
ROWS_UNCHECKED, ROWS_CHECKED, ROWS8_CAP = 64, 34, 48


def plan_rows4(q4_stack, q4_depth, dense=False):
    """lh_plan_rows4 without a forced cap -> (rows, guard)"""
    need = q4_stack if q4_stack else 3 * q4_depth + 5
    cap = ROWS_CHECKED if (dense or need > ROWS_UNCHECKED) else ROWS_UNCHECKED
    guard = need > cap
    need = (min(need, cap) + 1) & ~1
    return (need if guard or need >= 16 else 16), guard


def plan_rows8(q8_depth):
    """lh_plan_rows8 without a forced cap -> (rows, guard)"""
    need = 7 * q8_depth + 10
    guard = need > ROWS8_CAP
    need = (min(need, ROWS8_CAP) + 1) & ~1
    return (need if guard or need >= 16 else 16), guard
