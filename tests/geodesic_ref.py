"""numpy restatement of pnr_geodesic_distance's rule (include/pnr_hip.h), for the tests.  The rule twice: sweeps() is the recursion as it
is written -- every voxel's key from the keys of its 26 neighbours, over the 26 shifted arrays, until a sweep changes nothing (literal
Jacobi sweeps, or with inplace=True each offset applied at once: the same fixed point in fewer sweeps) --, dijkstra() is the
lexicographic minimum over all paths of (cost, source label) with heapq.  f32 exactly where the rule says f32 (the 26 step lengths);
everything else is exact integer arithmetic.  Keys are uint64 (D << 32) | label, NONE is all ones."""
import heapq
import numpy as np
import radius_ref

F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
DMAX = 2**31 - 1
UNREACHED = 0xFFFFFFFF
# the offset order: dz slowest, then dy, then dx, each ascending; the centre is left out
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def threshold(V, thr=0):
    return int(thr) if thr >= 0 else max(1, int(V.sum(dtype=np.uint64)) // V.size)


def lengths(zd):
    """len[o] = (uint32) rintf(32 * sqrtf((float)(dx^2 + dy^2) + (zd (float)dz) (zd (float)dz))), in the offset order"""
    zd = F(zd)
    out = []
    for dx, dy, dz in OFFSETS:
        zt = zd * F(dz)
        s = F(dx * dx + dy * dy) + zt * zt
        r = np.rint(F(32.0) * np.sqrt(s, dtype=F))
        assert s.dtype == F and r.dtype == F
        out.append(int(r))
    return out


def cost_table(cost=None):
    tab = np.asarray(cost, np.int64) if cost is not None else 256 - np.arange(256, dtype=np.int64)
    assert tab.shape == (256,) and tab.min() >= 1 and tab.max() <= 0xFFFF
    return tab


def sources(V, t, xyz, labels=None):
    """-> ({linear index: the smallest label of the kept sources on it}, n kept, n dropped)"""
    l, h, w = V.shape
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    labels = np.arange(len(xyz), dtype=np.int64) if labels is None else np.asarray(labels, np.int64)
    assert len(labels) == len(xyz) and (labels >= 0).all()
    fin, c = radius_ref.centres(xyz, V.shape)
    at, dropped = {}, 0
    for i in range(len(xyz)):
        if not fin[i] or V[c[i, 2], c[i, 1], c[i, 0]] < t:
            dropped += 1
            continue
        g = int(c[i, 0] + w * (c[i, 1] + h * c[i, 2]))
        at[g] = min(at.get(g, 2**31), int(labels[i]))
    return at, len(xyz) - dropped, dropped


def _setup(V, thr, zd, cost):
    V = np.asarray(V, np.uint8)
    t = threshold(V, thr)
    ln = lengths(zd)
    tab = cost_table(cost)
    assert max(ln) * 2 * int(tab.max()) <= 2**31 - 1
    return V, t, ln, tab


def _slices(o, n):
    """(destination, neighbour) slices of an axis of extent n for the offset component o: the neighbour of p is p + o"""
    return (slice(0, n - 1), slice(1, n)) if o == 1 else (slice(1, n), slice(0, n - 1)) if o == -1 else (slice(0, n), slice(0, n))


def sweeps(V, src, thr=0, zd=1.0, dmax=DMAX, cost=None, inplace=False):
    """-> (keys uint64 (l, h, w), t, the number of sweeps that changed something).  src: sources()[0]"""
    V, t, ln, tab = _setup(V, thr, zd, cost)
    l, h, w = V.shape
    P = V >= t
    Cv = tab[V].astype(np.uint64)
    K = np.full(V.shape, NONE, np.uint64)
    for g, lab in src.items():
        assert P.ravel()[g]
        K.ravel()[g] = np.uint64(lab)
    n = 0
    while True:
        new = K if inplace else K.copy()
        changed = False
        for (dx, dy, dz), le in zip(OFFSETS, ln):
            if (dx and w == 1) or (dy and h == 1) or (dz and l == 1):
                continue
            (px, qx), (py, qy), (pz, qz) = _slices(dx, w), _slices(dy, h), _slices(dz, l)
            p, q = (pz, py, px), (qz, qy, qx)
            Kq = K[q]
            wt = np.uint64(le) * (Cv[p] + Cv[q])
            ok = P[p] & P[q] & (Kq != NONE) & ((Kq >> np.uint64(32)) + wt <= np.uint64(dmax))  # (an unreached q fails the last test too)
            cand = np.where(ok, (Kq & np.uint64(0xFFFFFFFF)) | (((Kq >> np.uint64(32)) + wt) << np.uint64(32)), NONE)
            lower = cand < new[p]
            if lower.any():
                changed = True
                new[p] = np.where(lower, cand, new[p])
        if not changed:
            return K, t, n
        K = new
        n += 1


def dijkstra(V, src, thr=0, zd=1.0, dmax=DMAX, cost=None):
    """-> (keys uint64 (l, h, w), t): (cost, label) tuples through a heap"""
    V, t, ln, tab = _setup(V, thr, zd, cost)
    l, h, w = V.shape
    Vf = V.ravel()
    best = {}
    heap = [(0, lab, g) for g, lab in src.items()]
    for d, lab, g in heap:
        best[g] = (d, lab)
    heapq.heapify(heap)
    done = set()
    while heap:
        d, lab, g = heapq.heappop(heap)
        if g in done or best[g] != (d, lab):
            continue
        done.add(g)
        x, y, z = g % w, g // w % h, g // (w * h)
        cp = int(tab[Vf[g]])
        for (dx, dy, dz), le in zip(OFFSETS, ln):
            qx, qy, qz = x + dx, y + dy, z + dz
            if not (0 <= qx < w and 0 <= qy < h and 0 <= qz < l):
                continue
            q = qx + w * (qy + h * qz)
            if Vf[q] < t or q in done:
                continue
            nd = d + le * (cp + int(tab[Vf[q]]))
            if nd <= dmax and (nd, lab) < best.get(q, (1 << 62, 0)):
                best[q] = (nd, lab)
                heapq.heappush(heap, (nd, lab, q))
    K = np.full(V.size, NONE, np.uint64)
    for g, (d, lab) in best.items():
        K[g] = np.uint64((d << 32) | lab)
    return K.reshape(V.shape), t


def split(K):
    """-> (D uint32, L int32): 0xFFFFFFFF and -1 where unreached"""
    return (K >> np.uint64(32)).astype(np.uint32), (K & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).reshape(K.shape)


def info(V, K, t, n_src, n_dropped):
    """the summary as Context.geodesic returns it, without `rounds` (scheduling, not the rule)"""
    l, h, w = V.shape
    reached = K != NONE
    out = dict(n_vox=int(V.size), n_pass=int((np.asarray(V) >= t).sum()), n_reached=int(reached.sum()), n_src=int(n_src), n_src_dropped=int(n_dropped), first_max=-1,
               d_max=0, thr_used=int(t), max_at=None)
    if reached.any():
        D = K >> np.uint64(32)
        m = int(D[reached].max())
        i = int(np.flatnonzero(reached.ravel() & (D.ravel() == np.uint64(m)))[0])
        out.update(first_max=i, d_max=m, max_at=(i % w, (i // w) % h, i // (w * h)))
    return out


def at(K, xyz):
    """(d uint32, label int32) at the centre voxels; 0xFFFFFFFF and -1 for a position that is not finite"""
    fin, c = radius_ref.centres(xyz, K.shape)
    D, L = split(np.where(fin, K[c[:, 2], c[:, 1], c[:, 0]], NONE))
    return D, L


def pred(V, K, t, ln, tab, g):
    """the first q in the offset order with key(q) + (wt(q, p) << 32) == key(p); None if there is none"""
    l, h, w = V.shape
    Vf, Kf = V.ravel(), K.ravel()
    x, y, z = g % w, g // w % h, g // (w * h)
    for (dx, dy, dz), le in zip(OFFSETS, ln):
        qx, qy, qz = x + dx, y + dy, z + dz
        if not (0 <= qx < w and 0 <= qy < h and 0 <= qz < l):
            continue
        q = qx + w * (qy + h * qz)
        if Vf[q] < t or Kf[q] == NONE:
            continue
        wt = le * (int(tab[Vf[g]]) + int(tab[Vf[q]]))
        if int(Kf[q]) + (wt << 32) == int(Kf[g]):
            return q
    return None


def paths(V, K, xyz, path_cap, thr=0, zd=1.0, cost=None):
    """-> (path_len int32[m], a list of m int64 arrays) by the path rule: k > 0 complete, 0 unreached or not finite, -path_cap cut"""
    V, t, ln, tab = _setup(V, thr, zd, cost)
    l, h, w = V.shape
    fin, c = radius_ref.centres(xyz, K.shape)
    lens, out = [], []
    for i in range(len(c)):
        p = int(c[i, 0] + w * (c[i, 1] + h * c[i, 2]))
        walk, n = [], 0
        if fin[i] and K.ravel()[p] != NONE:
            while True:
                if len(walk) == path_cap:
                    n = -path_cap
                    break
                walk.append(p)
                if int(K.ravel()[p]) >> 32 == 0:
                    n = len(walk)
                    break
                p = pred(V, K, t, ln, tab, p)
                assert p is not None  # the rule has a predecessor at every reached voxel with D > 0
        lens.append(n)
        out.append(np.array(walk, np.int64))
    return np.array(lens, np.int32), out
