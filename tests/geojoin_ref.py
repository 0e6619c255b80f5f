"""numpy restatement of the rule of pnr_geodesic_bridges / pnr_join_expand (include/pnr_hip.h), for the tests, on top of geodesic_ref (keys,
pred), distance_ref (the sample points) and join_ref (input trees, union-find, re-rooting): the meet edges over the 13 shifted arrays,
Kruskal's algorithm over the ascending keys (W, p, o - 13), the two walks of every bridge, attachment, and the expansion.  Everything is
exact integer arithmetic on the keys."""
import numpy as np
import distance_ref
import geodesic_ref as geo
import join_ref
import radius_ref

F = np.float32
GEO_BRIDGE = np.dtype([("a", np.int32), ("b", np.int32), ("p", np.int64), ("o", np.int32), ("path_len", np.int32), ("w", np.uint64), ("path_off", np.int64)])


def forest_sources(xyz, parent, step=1):
    """-> (pts float32[k, 3], owner int32[k], label int[k], tree label per node): the sample points, each labelled with its owner's tree"""
    tree = join_ref.input_trees(parent)
    pts, owner = distance_ref.tree_sample(xyz, parent, 1, step)
    return pts, owner, tree[owner], tree


def dmax_of(limit):
    return int(limit) if 0 < limit <= geo.DMAX else geo.DMAX


def meet_edges(V, K, zd=1.0, thr=0, cost=None, limit=0):
    """-> (W, p, o) int64 / python-int arrays of all meet edges within the limit, sorted by the key (W, p, o - 13); o in 13..25"""
    V, t, ln, tab = geo._setup(V, thr, zd, cost)
    l, h, w = V.shape
    D, L = geo.split(K)
    D = D.astype(np.uint64)
    reached = K != geo.NONE
    Cv = tab[V].astype(np.uint64)
    idx = np.arange(V.size, dtype=np.int64).reshape(V.shape)
    Ws, Ps, Os = [], [], []
    for o in range(13, 26):
        dx, dy, dz = geo.OFFSETS[o]
        if (dx and w == 1) or (dy and h == 1) or (dz and l == 1):
            continue
        (px, qx), (py, qy), (pz, qz) = geo._slices(dx, w), geo._slices(dy, h), geo._slices(dz, l)
        p, q = (pz, py, px), (qz, qy, qx)
        assert (idx[q] > idx[p]).all()
        ok = reached[p] & reached[q] & (L[p] != L[q])
        W = D[p] + np.uint64(ln[o]) * (Cv[p] + Cv[q]) + D[q]
        if limit:
            ok &= W <= np.uint64(limit)
        Ws.append(W[ok])
        Ps.append(idx[p][ok])
        Os.append(np.full(int(ok.sum()), o, np.int64))
    W, P, O = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (Ws, Ps, Os))
    order = np.lexsort((O, P, W))
    return W[order], P[order], O[order]


def solve(V, xyz, parent, zd=1.0, limit=0, thr=0, step=1, cost=None):
    """-> (bridges GEO_BRIDGE[k], vox int64[sum(path_len)], info dict without `rounds`, K the keys)"""
    V = np.asarray(V, np.uint8)
    l, h, w = V.shape
    pts, owner, lab, tree = forest_sources(xyz, parent, step)
    t = geo.threshold(V, thr)
    src, kept, dropped = geo.sources(V, t, pts, lab)
    K, t, _ = geo.sweeps(V, src, thr, zd, dmax_of(limit), cost, inplace=True)
    _, _, ln, tab = geo._setup(V, thr, zd, cost)
    D, L = geo.split(K)
    Lf = L.ravel()
    # the first sample point of every source voxel's tree on it, and the trees that take part
    _, c = radius_ref.centres(pts, V.shape)
    cg = c[:, 0] + w * (c[:, 1] + h * c[:, 2])
    first_at, part = {}, set()
    for k in range(len(pts)):
        g = int(cg[k])
        if src.get(g) == int(lab[k]):
            part.add(int(lab[k]))
            first_at.setdefault(g, k)
    labels = sorted(set(int(v) for v in tree))
    # Kruskal over the ascending keys
    W, P, O = meet_edges(V, K, zd, thr, cost, limit)
    sets = join_ref._Sets(np.arange(len(tree)))
    la = Lf[P]
    lb = Lf[P + np.array([geo.OFFSETS[o][0] + w * (geo.OFFSETS[o][1] + h * geo.OFFSETS[o][2]) for o in O], np.int64)] if len(O) else la
    picked = []
    for e in range(len(W)):
        if len(picked) == len(part) - 1:
            break
        if sets.unite(int(la[e]), int(lb[e])):
            picked.append(e)
    bridges = np.zeros(len(picked), GEO_BRIDGE)
    vox = []
    for k, e in enumerate(picked):
        p, o = int(P[e]), int(O[e])
        dx, dy, dz = geo.OFFSETS[o]
        q = p + dx + w * (dy + h * dz)
        walks = []
        for g in (p, q):
            walk = [g]
            while int(K.ravel()[walk[-1]]) >> 32:
                walk.append(geo.pred(V, K, t, ln, tab, walk[-1]))
                assert walk[-1] is not None
            walks.append(walk)
        sa, sb = walks[0][-1], walks[1][-1]
        assert src[sa] == Lf[p] and src[sb] == Lf[q] and Lf[p] != Lf[q]
        chain = walks[0][::-1] + walks[1]
        bridges[k] = (owner[first_at[sa]], owner[first_at[sb]], p, o, len(chain), int(W[e]), len(vox))
        vox += chain
    info = dict(n_trees_in=len(labels), n_trees_lost=len(labels) - len(part), n_trees_out=len(labels) - len(picked), n_bridges=len(picked),
                n_inserted=int(sum(int(b["path_len"]) - 2 for b in bridges)), n_src=int(kept), n_src_dropped=int(dropped),
                w_max=int(bridges["w"].max()) if len(bridges) else 0, thr_used=int(t))
    return bridges, np.array(vox, np.int64), info, K


def expand(xyz, parent, bridges, vox, shape):
    """-> (xyz float32[n2, 3], parent int32[n2], bridge_of int32[n2 - n], join BRIDGE[k] for join_ref.reroot)"""
    l, h, w = shape
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    parent = np.asarray(parent).reshape(-1)
    n = len(xyz)
    new_xyz, new_parent, of = [], [], []
    join = np.zeros(len(bridges), join_ref.BRIDGE)
    for k, b in enumerate(bridges):
        chain = vox[int(b["path_off"]):int(b["path_off"]) + int(b["path_len"])]
        prev = int(b["a"])
        for g in chain[1:-1]:
            g = int(g)
            new_xyz.append((g % w, g // w % h, g // (w * h)))
            new_parent.append(prev)
            of.append(k)
            prev = n + len(new_xyz) - 1
        join[k] = (min(prev, int(b["b"])), max(prev, int(b["b"])), F(np.float64(int(b["w"])) / np.float64(64.0)))
    xyz2 = np.concatenate([xyz, np.array(new_xyz, F).reshape(-1, 3)])
    parent2 = np.concatenate([np.where(parent < 0, -1, parent), np.array(new_parent, np.int64)]).astype(np.int32)
    return xyz2, parent2, np.array(of, np.int32), join


def brute_force_weights(V, xyz, parent, zd=1.0, limit=0, thr=0, step=1, cost=None):
    """the bridge weights of Kruskal's algorithm over the TRUE pairwise geodesic distances of the trees (one heap per tree), ascending"""
    V = np.asarray(V, np.uint8)
    pts, owner, lab, tree = forest_sources(xyz, parent, step)
    t = geo.threshold(V, thr)
    labels = sorted(set(int(v) for v in tree))
    per = {}
    for a in labels:
        per[a] = geo.sources(V, t, pts[lab == a], lab[lab == a])[0]
    pairs = []
    for a in labels:
        Ka = geo.dijkstra(V, per[a], thr, zd, geo.DMAX, cost)[0].ravel()
        for b in labels:
            if b > a and per[b]:
                d = min(int(Ka[g]) >> 32 if Ka[g] != geo.NONE else 1 << 62 for g in per[b])
                if d < 1 << 62 and (not limit or d <= limit):
                    pairs.append((d, a, b))
    sets = join_ref._Sets(np.arange(len(tree)))
    return [d for d, a, b in sorted(pairs) if sets.unite(a, b)]
