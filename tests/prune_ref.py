"""The pruning rule of include/pnr_hip.h (pnr_prune_tree, pnr_prune_tree_host, pnr_prune_apply) restated in numpy and plain Python from
the header's text: sequential and unhurried -- every quantity is computed from its definition, a node at a time, by walking up or down
the parent links.  Also the forests the tests run on."""
import math
import numpy as np

LIMIT = 2 ** 32
INFO_KEYS = ("n", "n_roots", "n_leaves", "n_branch", "n_segments", "n_removed", "n_removed_segments", "n_removed_trees", "length_in", "length_out", "h_max", "order_max")


class RangeError(Exception):
    pass


def Q(x):
    return math.floor(256.0 * float(x) + 0.5)


def prune(xyz, radius, parent, zscale=1, min_length=0, radius_factor=0, min_tree=0):
    """-> (info dict without the rounds, keep, height, path, order, seg, depth) with depth = the most edges between a node and its root"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    parent = [int(p) for p in np.asarray(parent).reshape(-1)]
    n = len(parent)
    radius = np.zeros(n, np.float32) if radius is None else np.asarray(radius, np.float32)
    zs = float(np.float32(zscale))
    children = [[] for _ in range(n)]
    for i, p in enumerate(parent):  # (ascending index)
        if p >= 0:
            children[p].append(i)
    # 1: the edges
    q = [0] * n
    for i, p in enumerate(parent):
        if p >= 0:
            dx, dy, dz = xyz[i, 0] - xyz[p, 0], xyz[i, 1] - xyz[p, 1], (xyz[i, 2] - xyz[p, 2]) * zs
            q[i] = Q(math.sqrt(dx * dx + dy * dy + dz * dz))
    # the nodes with every parent in front of its children, and their depth
    roots = [i for i in range(n) if parent[i] < 0]
    order_down, depth = list(roots), [0] * n
    for v in order_down:
        for c in children[v]:
            depth[c] = depth[v] + 1
            order_down.append(c)
    assert len(order_down) == n, "a cycle"
    # 2, 3: heights and continuing children
    H, cont = [0] * n, [-1] * n
    for v in reversed(order_down):
        for c in children[v]:
            s = q[c] + H[c]
            if s >= LIMIT:
                raise RangeError
            if cont[v] < 0 or s > H[v]:  # (the children come in ascending index: a tie keeps the smaller)
                H[v], cont[v] = s, c
    # 4, 5, 6
    t_len, t_tree = Q(np.float32(min_length)), Q(np.float32(min_tree))
    k = float(np.float32(radius_factor))
    head, gone_head = [False] * n, [False] * n
    for i, p in enumerate(parent):
        head[i] = p < 0 or cont[p] != i
        if p < 0:
            gone_head[i] = H[i] < t_tree
        elif head[i]:
            gone_head[i] = q[i] + H[i] < max(t_len, Q(k * float(radius[p])))
    keep, path, order, seg = np.ones(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for v in order_down:  # (the walk up from every node, memoised on its parent)
        p = parent[v]
        if p < 0:
            far, o, s, gone = 0, 0, v, gone_head[v]
        else:
            far = int(path[p]) + q[v]
            o = int(order[p]) + (1 if head[v] else 0)
            s = v if head[v] else int(seg[p])
            gone = (not keep[p]) or gone_head[v]
        if far >= LIMIT:
            raise RangeError
        path[v], order[v], seg[v], keep[v] = far, o, s, 0 if gone else 1
    info = {"n": n, "n_roots": len(roots), "n_leaves": sum(1 for c in children if not c), "n_branch": sum(1 for c in children if len(c) >= 2),
            "n_segments": sum(head), "n_removed": int((keep == 0).sum()), "n_removed_segments": sum(1 for i in range(n) if head[i] and not keep[i]),
            "n_removed_trees": sum(1 for i in roots if not keep[i]), "length_in": sum(q), "length_out": sum(q[i] for i in range(n) if keep[i]),
            "h_max": max(H), "order_max": int(order.max())}
    return info, keep, np.array(H, np.uint32), path, order, seg, max(depth)


def apply(parent, keep):
    """the order-preserving compaction -> (new_index, parent of the kept nodes)"""
    parent, keep = np.asarray(parent), np.asarray(keep)
    idx = np.where(keep != 0, np.cumsum(keep != 0) - 1, -1).astype(np.int32)
    return idx, np.array([idx[p] if p >= 0 else -1 for p, k in zip(parent, keep) if k], np.int32)


STEPS = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float32)


def forest(n, trees, chain, seed=0, permute=True):
    """n nodes in `trees` trees: a node grows from the previous one with probability `chain`, else from a random earlier one, by one of
    the 26 lattice steps; radii are small integers.  The indices are then permuted, so a parent comes after its child as often as
    before -> (xyz float32[n, 3], radius float32[n], parent int32[n])"""
    rng = np.random.default_rng(seed)
    trees = min(trees, n)
    xyz, parent = np.zeros((n, 3), np.float32), np.full(n, -1, np.int32)
    xyz[:trees] = rng.integers(0, 64, (trees, 3))
    for i in range(trees, n):
        p = i - 1 if rng.random() < chain else int(rng.integers(0, i))
        parent[i] = p
        xyz[i] = xyz[p] + STEPS[rng.integers(0, 26)]
    radius = rng.integers(1, 5, n).astype(np.float32)
    if permute:
        new = rng.permutation(n)  # new[i]: the new index of node i
        xyz2, radius2, parent2 = np.empty_like(xyz), np.empty_like(radius), np.empty_like(parent)
        xyz2[new], radius2[new] = xyz, radius
        parent2[new] = np.where(parent >= 0, new[np.maximum(parent, 0)], -1)
        xyz, radius, parent = xyz2, radius2, parent2
    return xyz, radius, parent


# closed forms
def y_tie():
    """a root, a stem of 3 unit edges, then two arms of 4 unit edges: nodes 0..3 the stem, 4..7 one arm, 8..11 the other"""
    xyz = [(0, i, 0) for i in range(4)] + [(j, 3, 0) for j in range(1, 5)] + [(-j, 3, 0) for j in range(1, 5)]
    parent = [-1, 0, 1, 2, 3, 4, 5, 6, 3, 8, 9, 10]
    return np.array(xyz, np.float32), np.ones(12, np.float32), np.array(parent, np.int32)


def star(leaves=3000, length=2.0):
    """the root 0 with `leaves` leaves 1 .. leaves, each `length` away along +x, -x, +y, -y in turn: exactly equal lengths"""
    xyz = np.zeros((leaves + 1, 3), np.float32)
    k = np.arange(leaves)
    xyz[1:, 0] = np.where(k % 4 == 0, length, np.where(k % 4 == 1, -length, 0))
    xyz[1:, 1] = np.where(k % 4 == 2, length, np.where(k % 4 == 3, -length, 0))
    parent = np.zeros(leaves + 1, np.int32)
    parent[0] = -1
    return xyz, np.ones(leaves + 1, np.float32), parent


def chain(n=5000):
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = np.arange(n)
    return xyz, np.ones(n, np.float32), np.arange(-1, n - 1).astype(np.int32)


def radius_case(r_parent):
    """a chain of 8 along x and a side branch of length 3 on node 4, whose radius is r_parent"""
    xyz = [(i, 0, 0) for i in range(8)] + [(4, 3, 0)]
    radius = np.ones(9, np.float32)
    radius[4] = r_parent
    return np.array(xyz, np.float32), radius, np.array([-1, 0, 1, 2, 3, 4, 5, 6, 4], np.int32)
