"""The rule a device-built hierarchy follows (drt_rebuild_hierarchy; csrc/drt_build_rule.h), restated in numpy:
boxes -> keys -> leaf order -> nodes. Nothing here knows how the kernels work: the tree is a deterministic function of the surfaces'
boxes, so tests/test_gpu_hierarchy.py holds drt_read_hierarchy to this byte for byte, and tests/test_hierarchy_cpu.py holds this and the
C++ text of the rule to each other.

    boxes(rows)                      the tree surfaces of raw surface rows (pydrt.surface_rows) and their boxes: prim_bounds
    keys(lo, hi)                     the 63-bit key of every tree surface
    build(lo, hi, budget=True)       {"key", "order", "child", "count", "depth"}: order[j] is the tree POSITION in leaf slot j
    build_rows(rows, budget=True)    the same from raw rows, with "leaf_surface": the surface index in every leaf slot

budget=False turns the depth budget of the split off, so a test can show that the budget is what bounds a case."""
import numpy as np

GEO_SPHERE, GEO_PLANE = 2, 3  # DRT_GEO_*
BVH_STACK = 32
UNBOUNDED = np.uint64(2 ** 63 - 1)
POS, RADIUS, NORMAL, U, V = slice(1, 4), 4, slice(5, 8), slice(8, 11), slice(11, 14)


def _plane_box(r):
    """prim_bounds (drt_launcher.hip) for a plane, operation for operation on float64 scalars"""
    f = np.float64
    u, v, n, p = [f(x) for x in r[U]], [f(x) for x in r[V]], [f(x) for x in r[NORMAL]], [f(x) for x in r[POS]]
    with np.errstate(all="ignore"):
        ul = np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        vl = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        un, vn = [x / ul for x in u], [x / vl for x in v]
        c0 = [vn[1] * n[2] - vn[2] * n[1], vn[2] * n[0] - vn[0] * n[2], vn[0] * n[1] - vn[1] * n[0]]
        c1 = [n[1] * un[2] - n[2] * un[1], n[2] * un[0] - n[0] * un[2], n[0] * un[1] - n[1] * un[0]]
        det = un[0] * c0[0] + un[1] * c0[1] + un[2] * c0[2]
        ok = np.isfinite(det) and abs(det) > 1e-6 and np.isfinite(ul) and np.isfinite(vl)
        lo, hi = [f(np.inf)] * 3, [f(-np.inf)] * 3
        if ok:
            for corner in range(4):
                a, b = (ul if corner & 1 else f(0.0)), (vl if corner & 2 else f(0.0))
                for k in range(3):
                    x = p[k] + (a * c0[k] + b * c1[k]) / det
                    lo[k] = x if x < lo[k] else lo[k]  # std::min / std::max: the first argument stays when the comparison is false
                    hi[k] = x if hi[k] < x else hi[k]
        else:
            lo, hi = [f(-1e300)] * 3, [f(1e300)] * 3
    return lo, hi


def boxes(rows):
    """(surface index of every tree surface [m], lo [m][3], hi [m][3]): spheres and planes in surface order, points left out"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    types = rows[:, 0].copy().view("<u4")[0::2] if len(rows) else np.zeros(0, dtype="<u4")
    surf = np.flatnonzero((types == GEO_SPHERE) | (types == GEO_PLANE)).astype(np.uint32)
    lo, hi = np.empty((len(surf), 3)), np.empty((len(surf), 3))
    for k, i in enumerate(surf):
        if types[i] == GEO_SPHERE:
            lo[k], hi[k] = rows[i, POS] - np.abs(rows[i, RADIUS]), rows[i, POS] + np.abs(rows[i, RADIUS])
        else:
            lo[k], hi[k] = _plane_box(rows[i])
    with np.errstate(all="ignore"):
        a, b = np.abs(lo), np.abs(hi)
        pad = 1e-5 + 1e-9 * np.where(a < b, b, a)  # std::max(|lo|, |hi|)
        lo, hi = lo - pad, hi + pad
    return surf, lo, hi


def _spread3(v):
    x = v.astype(np.uint64) & np.uint64(0x1FFFFF)
    for shift, mask in ((32, 0x001F00000000FFFF), (16, 0x001F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def keys(lo, hi):
    """steps 2-4 of the rule: bounded surfaces, the smallest and largest centre, the quantised coordinates, the interleave"""
    m = len(lo)
    key = np.full(m, UNBOUNDED, dtype=np.uint64)
    if m == 0:
        return key
    with np.errstate(all="ignore"):
        bounded = (np.abs(lo) < 1e299).all(axis=1) & (np.abs(hi) < 1e299).all(axis=1)
        c = 0.5 * (lo + hi)
    if not bounded.any():
        return key
    cb = c[bounded]
    clo, chi = cb.min(axis=0), cb.max(axis=0)
    ext = chi - clo
    q = np.zeros((len(cb), 3), dtype=np.uint32)
    for a in range(3):
        if ext[a] > 0.0:
            q[:, a] = np.minimum(((cb[:, a] - clo[a]) / ext[a] * 2097152.0).astype(np.uint64), 2 ** 21 - 1).astype(np.uint32)
    key[bounded] = (_spread3(q[:, 0]) << np.uint64(2)) | (_spread3(q[:, 1]) << np.uint64(1)) | _spread3(q[:, 2])
    return key


def _split(key, b, e, depth, budget):
    log2m = 0
    while (1 << log2m) < e - b:
        log2m += 1
    first, last = int(key[b]), int(key[e - 1])
    if (budget and not depth + 2 + log2m < BVH_STACK) or first == last:
        return (b + e) // 2
    top = (first ^ last).bit_length() - 1
    # the first position whose key has bit `top`: keys ascend and agree above it
    return b + int(np.searchsorted((key[b:e] >> np.uint64(top)) & np.uint64(1), 1, side="left"))


def topology(key, budget=True):
    """steps 6-8 on sorted keys: (child [n][2] int32, count [n][2] int32, levels as BvhBuilder counts them)"""
    m = len(key)
    n = max(m - 1, 1)
    child, count = np.full((n, 2), -1, dtype=np.int32), np.full((n, 2), -1, dtype=np.int32)
    if m == 0:
        return child, count, 0
    if m == 1:
        child[0, 0], count[0, 0] = -2, 1
        return child, count, 1
    depth = 0
    todo = [(0, 0, m, 0)]
    while todo:
        node, b, e, d = todo.pop()
        depth = max(depth, d + 1)
        mid = _split(key, b, e, d, budget)
        for c, (cb, ce) in enumerate(((b, mid), (mid, e))):
            if ce - cb == 1:
                child[node, c], count[node, c] = -2 - 8 * cb, 1
            else:
                me = node + 1 if c == 0 else node + (mid - b)
                child[node, c], count[node, c] = me, 0
                todo.append((me, cb, ce, d + 1))
    return child, count, depth


def build(lo, hi, budget=True):
    key = keys(lo, hi)
    order = np.argsort(key, kind="stable").astype(np.uint32)  # (key, position) ascending
    child, count, depth = topology(key[order], budget)
    return {"key": key, "order": order, "child": child, "count": count, "depth": depth}


def build_rows(rows, budget=True):
    surf, lo, hi = boxes(rows)
    t = build(lo, hi, budget)
    t["leaf_surface"] = surf[t["order"]]
    t["lo"], t["hi"] = lo, hi
    return t


NODE_DTYPE = np.dtype([("lo", "<f4", (2, 3)), ("hi", "<f4", (2, 3)), ("child", "<i4", (2,)), ("count", "<i4", (2,))])  # BvhNode, 64 bytes


def check_tree(child, count, m):
    """what every tree over m surfaces must be, whatever its shape: returns (levels, the range [b, e) of every node). Every leaf slot
    hangs in exactly one place, the nodes are in pre-order, a node's range is the union of its children's."""
    n = max(m - 1, 1)
    assert child.shape == (n, 2) and count.shape == (n, 2)
    if m == 0:
        assert (child == -1).all() and (count == -1).all()
        return 0, [(0, 0)]
    if m == 1:
        assert child.tolist() == [[-2, -1]] and count.tolist() == [[1, -1]]
        return 1, [(0, 1)]
    seen = np.zeros(m, dtype=np.int64)
    ranges = [None] * n
    visited = []
    levels = 0

    def walk(node, d):  # (the depth is at most BVH_STACK: far inside Python's recursion limit; a deeper tree fails the caller's assert)
        nonlocal levels
        assert d < 4 * BVH_STACK, "a chain deeper than any tree the rule allows"
        visited.append(node)
        levels = max(levels, d + 1)
        span = []
        for c in range(2):
            if count[node, c] == 1:
                packed = -2 - int(child[node, c])
                assert packed >= 0 and packed % 8 == 0
                seen[packed // 8] += 1
                span.append((packed // 8, packed // 8 + 1))
            else:
                assert count[node, c] == 0 and 0 < child[node, c] < n
                span.append(walk(int(child[node, c]), d + 1))
        assert span[0][1] == span[1][0], "node %d: its children's ranges %s do not meet" % (node, span)
        ranges[node] = (span[0][0], span[1][1])
        return ranges[node]

    assert walk(0, 0) == (0, m)
    assert (seen == 1).all()
    assert visited == list(range(n)), "not in pre-order"
    return levels, ranges


def level_entries(child, count):
    """the inner nodes below the root by depth, from the links of a tree check_tree has passed: entries[d] is the sorted list of
    (node, parent * 2 + child slot) of the inner nodes at depth d (entries[0] is empty: the root has no parent). What
    drt_build_topology_kernel's level table and level counts must hold."""
    entries, level = [[]], [0]
    while level:
        below = [(int(child[i, c]), 2 * i + c) for i in level for c in range(2) if count[i, c] == 0]
        if below:
            entries.append(sorted(below))
        level = [node for node, _ in below]
    return entries
