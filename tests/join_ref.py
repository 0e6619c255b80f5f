"""numpy restatement of the join's rule (include/pnr_hip.h: pnr_nearest_other, pnr_join_trees, pnr_join_reroot), for the tests: the
nearest point of another label by a dense float32 distance matrix with the packed-key minimum; the bridges by Kruskal's algorithm over all
cross pairs sorted by (bits(d2), lo, hi); the same bridges by Boruvka's rounds over nearest_other (an independent form); the re-rooting
and ordering by a recursive-free depth-first walk."""
import numpy as np

F = np.float32
BRIDGE = np.dtype([("lo", np.int32), ("hi", np.int32), ("d", np.float32)])


def scaled(xyz, zscale):
    x = np.array(xyz, F).reshape(-1, 3)
    x[:, 2] = x[:, 2] * F(zscale)
    return x


def d2_rows(x, p0, p1):
    """d2 of the points [p0, p1) against all points: (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j, float32"""
    d = [x[p0:p1, None, k] - x[None, :, k] for k in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    assert d2.dtype == F
    return np.ascontiguousarray(d2)


def nearest_other(xyz, label, rows=512, root=True):
    """-> (d float32[n], j int32[n]); root=False: d2 instead of its root"""
    x = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    label = np.asarray(label).reshape(-1)
    n = len(x)
    idx = np.arange(n, dtype=np.uint64)
    d = np.full(n, np.inf, F)
    j = np.full(n, -1, np.int32)
    none = np.uint64(0xffffffffffffffff)
    for p0 in range(0, n, rows):
        d2 = d2_rows(x, p0, p0 + rows)
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None, :]
        ok = (label[None, :] >= 0) & (label[None, :] != label[p0:p0 + rows, None]) & (label[p0:p0 + rows, None] >= 0) & np.isfinite(d2)
        best = np.where(ok, key, none).min(1)
        hit = best != none
        d[p0:p0 + rows][hit] = (best[hit] >> np.uint64(32)).astype(np.uint32).view(F)
        j[p0:p0 + rows][hit] = (best[hit] & np.uint64(0xffffffff)).astype(np.int32)
    return (np.sqrt(d) if root else d), j


def input_trees(parent):
    """-> label int[n]: the smallest node index of every node's input tree; ValueError for a parent >= n or a cycle"""
    parent = np.asarray(parent).reshape(-1)
    n = len(parent)
    if (parent >= n).any():
        raise ValueError("parent >= n")
    top = np.arange(n)
    for i in range(n):  # walk every chain to its end, at most n steps
        v, steps = i, 0
        while parent[v] >= 0:
            v, steps = parent[v], steps + 1
            if steps > n:
                raise ValueError("cycle")
        top[i] = v
    label = np.full(n, n)
    np.minimum.at(label, top, np.arange(n))
    return label[top]


class _Sets:
    def __init__(self, label):
        self.up = np.array(label)

    def find(self, a):
        while self.up[a] != a:
            self.up[a] = self.up[self.up[a]]
            a = self.up[a]
        return a

    def unite(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.up[max(a, b)] = min(a, b)
        return True

    def all(self):
        return np.array([self.find(i) for i in range(len(self.up))])


def _bridges(keys):
    keys = sorted(keys)
    out = np.zeros(len(keys), BRIDGE)
    for k, (bits, lo, hi) in enumerate(keys):
        out[k] = (lo, hi, np.sqrt(np.array([bits], np.uint32).view(F)[0]))
    return out


def bridges_kruskal(xyz, parent, zscale=1, gap=0, chunk=1 << 16):
    """Kruskal over all pairs of different input trees with d2 <= gap * gap, ascending in (bits(d2), lo, hi) -> BRIDGE[k] in that order"""
    x = scaled(xyz, zscale)
    n = len(x)
    assert n < 1 << 16
    label = input_trees(parent)
    g2 = F(gap) * F(gap)
    keys = []
    for p0 in range(0, n, 512):
        d2 = d2_rows(x, p0, p0 + 512)
        i, j = np.nonzero((label[p0:p0 + 512, None] != label[None, :]) & (np.arange(p0, min(p0 + 512, n))[:, None] < np.arange(n)[None, :]))
        v = d2[i, j]
        if gap > 0:
            keep = v <= g2
            i, j, v = i[keep], j[keep], v[keep]
        keys.append((v.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ((i + p0).astype(np.uint64) << np.uint64(16)) | j.astype(np.uint64))
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.uint64)
    sets = _Sets(label)
    trees = len(np.unique(label))
    out = []
    for c0 in range(0, len(keys), chunk):  # (pairs already inside one component are dropped a chunk at a time: the loop stays short)
        if trees - len(out) == 1:
            break
        k = keys[c0:c0 + chunk]
        lo, hi = ((k >> np.uint64(16)) & np.uint64(0xffff)).astype(np.int64), (k & np.uint64(0xffff)).astype(np.int64)
        cur = sets.all()
        for t in np.flatnonzero(cur[lo] != cur[hi]):
            if sets.unite(lo[t], hi[t]):
                out.append((int(k[t] >> np.uint64(32)), int(lo[t]), int(hi[t])))
    return _bridges(out)


def bridges_boruvka(xyz, parent, zscale=1, gap=0):
    """Boruvka's rounds: every live component takes its smallest edge; one whose smallest edge exceeds gap * gap leaves -> (BRIDGE[k], rounds)"""
    x = scaled(xyz, zscale)
    n = len(x)
    sets = _Sets(input_trees(parent))
    g2 = F(gap) * F(gap)
    dead = np.zeros(n, bool)
    out, rounds = [], 0
    while True:
        rep = sets.all()
        live = np.unique(rep[~dead[rep]])
        if len(live) < 2:
            break
        d2, j = nearest_other(x, np.where(dead[rep], -1, rep), root=False)
        rounds += 1
        best = {}
        for i in np.flatnonzero(j >= 0):
            key = (int(d2[i:i + 1].view(np.uint32)[0]), min(i, int(j[i])), max(i, int(j[i])))
            if rep[i] not in best or key < best[rep[i]]:
                best[rep[i]] = key
        edges = set()
        for r, key in best.items():
            if gap > 0 and not np.array([key[0]], np.uint32).view(F)[0] <= g2:
                dead[r] = True
            else:
                edges.add(key)
        if not edges:
            break
        for key in sorted(edges):
            if sets.unite(key[1], key[2]):
                out.append(key)
    return _bridges(out), rounds


def reroot(parent, bridges, root=-1):
    """-> (parent_out, order, comp, trees_out); bridges: BRIDGE[k] or (lo, hi) pairs"""
    parent = np.asarray(parent).reshape(-1)
    n = len(parent)
    in_label = input_trees(parent)
    pairs = [(int(b["lo"]), int(b["hi"])) for b in bridges] if isinstance(bridges, np.ndarray) and bridges.dtype == BRIDGE else [tuple(map(int, b)) for b in bridges]
    nbr = [[] for _ in range(n)]
    sets = _Sets(in_label)
    for a, b in [(i, int(parent[i])) for i in range(n) if parent[i] >= 0] + pairs:
        nbr[a].append(b)
        nbr[b].append(a)
        sets.unite(a, b)
    out_label = sets.all()
    in_size = np.bincount(in_label, minlength=n)
    comps = []
    for c in np.unique(out_label):
        members = np.flatnonzero(out_label == c)
        if root >= 0 and out_label[root] == c:
            top, first = root, 0
        else:
            roots = [i for i in members if parent[i] < 0]
            top, first = min(roots, key=lambda r: (-in_size[in_label[r]], r)), 1
        comps.append((first, -len(members), top))
    parent_out = np.full(n, -1, np.int32)
    comp = np.full(n, -1, np.int32)
    order = []
    for ci, (_, _, top) in enumerate(sorted(comps)):
        stack = [top]
        while stack:
            v = stack.pop()
            order.append(v)
            comp[v] = ci
            for u in sorted(nbr[v], reverse=True):
                if u != parent_out[v]:
                    parent_out[u] = v
                    stack.append(u)
    return parent_out, np.array(order, np.int32), comp, len(comps)


def join(xyz, parent, zscale=1, gap=0, root=-1, bridges=None):
    """-> (parent_out, order, comp, bridges, {"trees_in", "trees_out"}) by Kruskal (or with the bridges given)"""
    if bridges is None:
        bridges = bridges_kruskal(xyz, parent, zscale, gap)
    po, order, comp, t1 = reroot(parent, bridges, root)
    return po, order, comp, bridges, {"trees_in": int((np.asarray(parent).reshape(-1) < 0).sum()), "trees_out": t1}


def random_forest(rng, n, trees, extent=16.0, integer=True):
    """n nodes in `trees` random-recursive trees around scattered centres: node i < trees is a root at a random centre, every later
    node hangs off a random earlier node of a random tree, a step away; integer coordinates in [0, extent) give massive ties"""
    xyz = np.zeros((n, 3), F)
    parent = np.full(n, -1, np.int32)
    tree = np.zeros(n, np.int64)
    trees = min(trees, n)
    xyz[:trees] = rng.random((trees, 3)) * extent
    tree[:trees] = np.arange(trees)
    members = [[t] for t in range(trees)]
    for i in range(trees, n):
        t = int(rng.integers(trees))
        p = members[t][int(rng.integers(len(members[t])))]
        parent[i], tree[i] = p, t
        xyz[i] = np.clip(xyz[p] + rng.normal(0, 1.0, 3), 0, extent - 0.01)
        members[t].append(i)
    if integer:
        xyz = np.floor(xyz).astype(F)
    return xyz, parent
