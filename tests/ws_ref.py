"""The rule of the marker-controlled watershed (include/pnr_hip.h: pnr_watershed) restated in numpy, in two independent forms: a heap on the
keys (M, D) followed by the labels in key order, and the literal relaxation of both passes in random order -- and that relaxation once
more in whole-volume sweeps, the fast form for the larger stacks of the GPU tests.  Exact integer arithmetic;
volumes are (l, h, w).  Also the test volumes that the host and the GPU tests share, and the chain of Context.split_touching stage by
stage from the other restatements."""
import heapq
import os
import re
import numpy as np
import components_ref
import edt_ref
import morph_ref
import radius_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNS = (4, 8, 6, 26)
INF = (255 << 24) | 0xFFFFFF  # no key
DSAT = 0xFFFFFF
offsets = morph_ref.offsets


def tile():
    """(TZ, TY, TX) of watershed.h"""
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "watershed.h")).read()
    t = {k: int(v) for k, v in re.findall(r"constexpr int WS_(TX|TY|TZ) = (\d+);", txt)}
    return t["TZ"], t["TY"], t["TX"]


def g(ks, r):
    """g(K(s), t) for a voxel t of relief r; keys as M << 24 | D, D saturating"""
    if r > ks >> 24:
        return (r << 24) | 1
    return ks if ks & DSAT == DSAT else ks + 1


def setup(V, thr=-1, relief=None, markers=None, points=None, labels=None):
    """-> (mask bool, R uint8, mark int64 (0: none; only inside the mask), t, n_dropped)"""
    V = np.ascontiguousarray(V, np.uint8)
    t = components_ref.threshold(V, thr)
    mask = V >= t
    R = (255 - V).astype(np.uint8) if relief is None else np.ascontiguousarray(relief, np.uint8).reshape(V.shape)
    assert (markers is None) != (points is None)
    if markers is not None:
        mark = np.asarray(markers, np.int64).reshape(V.shape)
        assert (mark >= 0).all()
        dropped = int(((mark > 0) & ~mask).sum())
        mark = np.where(mask, mark, 0)
    else:
        xyz = np.asarray(points, np.float32).reshape(-1, 3)
        lab = np.arange(1, len(xyz) + 1, dtype=np.int64) if labels is None else np.asarray(labels, np.int64)
        assert (lab >= 1).all()
        fin, c = radius_ref.centres(xyz, V.shape)
        mark = np.zeros(V.shape, np.int64)
        dropped = 0
        for ok, (cx, cy, cz), lb in zip(fin, c, lab):
            if not ok or not mask[cz, cy, cx]:
                dropped += 1
            elif mark[cz, cy, cx] == 0 or lb < mark[cz, cy, cx]:
                mark[cz, cy, cx] = lb
    return mask, R, mark, t, dropped


def _neighbours(shape, C):
    l, h, w = shape
    offs = offsets(C)

    def nb(i):
        z, y, x = i // (w * h), i // w % h, i % w
        for dz, dy, dx in offs:
            qz, qy, qx = z + dz, y + dy, x + dx
            if 0 <= qz < l and 0 <= qy < h and 0 <= qx < w:
                yield (qz * h + qy) * w + qx
    return nb


def flood_heap(mask, R, mark, C):
    """the keys by Dijkstra's algorithm on (M, D), then the labels in ascending key order -> (K int64 (INF: none), L int64), flat"""
    nb = _neighbours(mask.shape, C)
    m, r, mk = mask.ravel(), R.ravel().astype(np.int64), mark.ravel()
    K = np.full(m.size, INF, np.int64)
    heap = []
    for i in np.flatnonzero(mk > 0):
        K[i] = int(r[i]) << 24
        heap.append((int(K[i]), int(i)))
    heapq.heapify(heap)
    order = []
    done = np.zeros(m.size, bool)
    while heap:
        k, i = heapq.heappop(heap)
        if done[i] or k > K[i]:
            continue
        done[i] = True
        order.append(i)
        for q in nb(i):
            if m[q] and mk[q] == 0:
                cand = g(k, int(r[q]))
                if cand < K[q]:
                    K[q] = cand
                    heapq.heappush(heap, (cand, q))
    L = mk.copy()
    for i in order:  # ascending keys: every tight neighbour is final
        if mk[i] == 0 and K[i] != INF:
            tight = [int(L[q]) for q in nb(i) if K[q] != INF and g(int(K[q]), int(r[i])) == K[i]]
            L[i] = min(tight)
    return K, L


def flood_relax(mask, R, mark, C, seed=0):
    """the literal relaxation in random order: keys until nothing falls, then labels until nothing falls -> (K, L), flat"""
    rng = np.random.default_rng(seed)
    nb = _neighbours(mask.shape, C)
    m, r, mk = mask.ravel(), R.ravel().astype(np.int64), mark.ravel()
    K = np.where(mk > 0, r << 24, INF).astype(np.int64)
    free = np.flatnonzero(m & (mk == 0))
    changed = True
    while changed:
        changed = False
        for i in rng.permutation(free):
            best = min([g(int(K[q]), int(r[i])) for q in nb(i) if m[q]], default=INF)
            if best < K[i]:
                K[i], changed = best, True
    NOL = 1 << 40
    L = np.where(mk > 0, mk, NOL).astype(np.int64)
    changed = True
    while changed:
        changed = False
        for i in rng.permutation(free):
            if K[i] == INF:
                continue
            best = min([int(L[q]) for q in nb(i) if K[q] != INF and g(int(K[q]), int(r[i])) == K[i]], default=NOL)
            if best < L[i]:
                L[i], changed = best, True
    assert not ((L == NOL) & (K != INF)).any()
    return K, np.where(L == NOL, 0, L)


def flood_sweeps(mask, R, mark, C):
    """the same relaxation in whole-volume sweeps (every voxel from the previous sweep's values): fast in numpy where the paths are short;
    test_watershed_host.py holds it against the two forms above -> (K, L), flat"""
    l, h, w = mask.shape
    offs = offsets(C)
    r = R.astype(np.int64)
    free = mask & (mark == 0)
    K = np.where(mark > 0, r << 24, INF).astype(np.int64)
    NOL = 1 << 40

    def shifted(A, o, fill):
        P = np.full((l + 2, h + 2, w + 2), fill, np.int64)
        P[1:-1, 1:-1, 1:-1] = A
        return P[1 + o[0]:1 + o[0] + l, 1 + o[1]:1 + o[1] + h, 1 + o[2]:1 + o[2] + w]

    def cand(o):
        Ks = shifted(K, o, INF)
        return np.where(r > Ks >> 24, (r << 24) | 1, np.where(Ks & DSAT == DSAT, Ks, Ks + 1))
    while True:
        best = K
        for o in offs:
            best = np.minimum(best, np.where(free, cand(o), INF))
        if np.array_equal(best, K):
            break
        K = best
    L = np.where(mark > 0, mark, NOL).astype(np.int64)
    tight = [free & (K != INF) & (cand(o) == K) for o in offs]
    while True:
        best = L
        for o, tg in zip(offs, tight):
            best = np.minimum(best, np.where(tg, shifted(L, o, NOL), NOL))
        if np.array_equal(best, L):
            break
        L = best
    return K.ravel(), np.where(L == NOL, 0, L).ravel()


def run(V, thr=-1, connectivity=26, relief=None, markers=None, points=None, labels=None, solver=flood_heap):
    """-> (info dict of the exact fields, L int32 (l, h, w), M uint8 (l, h, w), K int64 (l, h, w))"""
    V = np.ascontiguousarray(V, np.uint8)
    C = connectivity or 26
    mask, R, mark, t, dropped = setup(V, thr, relief, markers, points, labels)
    K, L = solver(mask, R, mark, C)
    reached = K != INF
    assert not (reached & (K & DSAT == DSAT)).any()
    TZ, TY, TX = tile()
    l, h, w = V.shape
    info = {"n_vox": V.size, "n_mask": int(mask.sum()), "n_marker_vox": int((mark > 0).sum()), "n_dropped": dropped, "n_reached": int(reached.sum()),
            "n_unreached": int(mask.sum() - reached.sum()), "n_regions": len(np.unique(L[L > 0])), "tiles": -(-l // TZ) * -(-h // TY) * -(-w // TX),
            "m_max": int((K[reached] >> 24).max()) if reached.any() else 0, "d_max": int((K[reached] & DSAT).max()) if reached.any() else 0, "thr_used": t,
            "connectivity": C}
    M = np.where(reached, K >> 24, 0).astype(np.uint8)
    return info, L.astype(np.int32).reshape(V.shape), M.reshape(V.shape), K.reshape(V.shape)


EXACT = ("n_vox", "n_mask", "n_marker_vox", "n_dropped", "n_reached", "n_unreached", "n_regions", "tiles", "m_max", "d_max", "thr_used", "connectivity")


def regions_hold_their_markers(L, mark, C):
    """every voxel of a region is C-connected inside it to a marker voxel of its label (a label with one marker component: the region is
    C-connected and holds its marker)"""
    L = np.asarray(L, np.int64)
    nb = _neighbours(L.shape, C)
    Lf, mf = L.ravel(), np.asarray(mark, np.int64).ravel()
    for lab in np.unique(Lf[Lf > 0]):
        vox = np.flatnonzero(Lf == lab)
        start = [int(i) for i in vox if mf[i] == lab]
        if not start:
            return False
        seen, stack = set(start), list(start)
        while stack:
            for q in nb(stack.pop()):
                if Lf[q] == lab and q not in seen:
                    seen.add(q)
                    stack.append(q)
        if len(seen) != len(vox):
            return False
    return True


def minimax(mask, R, mark, C):
    """M from the merged rule: the reconstruction by erosion (tests/morph_ref.py) of the marker function -- R on the markers, 255 elsewhere --
    under the relief, with everything outside the mask walled off at 255 -> (M uint8, reached bool)"""
    Rw = np.where(mask, R, 255).astype(np.uint8)
    f = np.where(mark > 0, Rw, 255).astype(np.uint8)
    E = morph_ref.erode(f, Rw, C)
    # a voxel is reached iff it is connected to a marker inside the mask
    seed = np.where(mark > 0, 255, 0).astype(np.uint8)
    conn = morph_ref.dilate(seed, np.where(mask, 255, 0).astype(np.uint8), C) > 0
    return E, conn


# ---- test volumes: (V, relief or None, marker volume) ----
def serpentine(shape, level=200):
    """a one-voxel-wide corridor through every tile of the stack: along x in every second row of a slice, joined at alternating ends, the
    slices joined at alternating corners two slices apart"""
    l, h, w = shape
    V = np.zeros(shape, np.uint8)
    at = []
    for zi, z in enumerate(range(0, l, 2)):
        rows = list(range(0, h, 2))
        if zi % 2:
            rows.reverse()
        cells = []
        right = True
        for yi, y in enumerate(rows):
            xs = list(range(w)) if right else list(range(w - 1, -1, -1))
            cells += [(z, y, x) for x in xs]
            if yi + 1 < len(rows):
                step = 1 if rows[yi + 1] > y else -1
                cells.append((z, y + step, xs[-1]))
            right = not right
        at += cells
        if z + 2 < l:
            at.append((z + 1,) + cells[-1][1:])
    for p in at:
        V[p] = level
    return V, at


def two_balls(shape=(16, 16, 32), r=6, c1=(8, 8, 11), c2=(8, 8, 20)):
    """two overlapping balls (200 in 0) whose centres are 9 apart along x -> (V, the two centres as (x, y, z))"""
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    V = np.zeros(shape, np.uint8)
    for cz, cy, cx in (c1, c2):
        V[(z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 <= r * r] = 200
    return V, [(c1[2], c1[1], c1[0]), (c2[2], c2[1], c2[0])]


def split_touching(V, h, zd, thr=-1, rmax=64, scale=4, connectivity=26):
    """the chain of Context.split_touching from the restatements of its stages -> (labels int32, n_cells)"""
    F = np.float32
    d2, _ = edt_ref.transform(V, thr, zd, rmax)
    q = np.minimum(F(255), np.floor(F(scale) * np.sqrt(d2.astype(F)))).astype(np.uint8)
    hm, _ = morph_ref.run(q, "hmax", h=h, C=26)
    dome, _ = morph_ref.run(hm, "hdome", h=1, C=26)
    cinfo, markers, _ = components_ref.label(dome, 1, 26)
    _, L, _, _ = run(V, thr, connectivity, relief=(255 - q).astype(np.uint8), markers=markers)
    return L, int(cinfo["n_comp"])
