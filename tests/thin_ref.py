"""The thinning rule and the forest rule of include/pnr_hip.h (pnr_skeletonize, pnr_skeleton_forest) restated in numpy, the volumes the
thinning tests share, and the topological invariants (against scipy.ndimage.label) that hold the restatement itself to account.

Arrays are (l, h, w) = (z, y, x), C order: the linear index of a voxel is x + w * (y + h * z).  A neighbourhood is a 27-bit word of the
3 x 3 x 3 cube, bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1), the centre (bit 13) clear.  The two connectivity tests flood a reached-set over
per-cell adjacency masks, for all candidates of a pass at once."""
import os
import re
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(i % 3 - 1, i // 3 % 3 - 1, i // 9 - 1) for i in range(27)]  # (dx, dy, dz) of bit i


def _mask(pred):
    return sum(1 << i for i, c in enumerate(CELLS) if pred(c))


N6 = _mask(lambda c: sum(map(abs, c)) == 1)
N18 = _mask(lambda c: 1 <= sum(map(abs, c)) <= 2)
N26 = _mask(lambda c: c != (0, 0, 0))
# the cells one 26-step from cell i inside N26, and one 6-step from cell i inside N18
ADJ26 = [_mask(lambda c, a=a: c != a and c != (0, 0, 0) and max(abs(c[k] - a[k]) for k in range(3)) == 1) if a != (0, 0, 0) else 0 for a in CELLS]
ADJ6 = [_mask(lambda c, a=a: 1 <= sum(map(abs, c)) <= 2 and sum(abs(c[k] - a[k]) for k in range(3)) == 1) if 1 <= sum(map(abs, a)) <= 2 else 0 for a in CELLS]


def tile():
    """(TX, TY, TZ) of pnr_amd/csrc/thin.h"""
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "thin.h")).read()
    t = {k: int(v) for k, v in re.findall(r"constexpr int (THIN_TX|THIN_TY|THIN_TZ) = (\d+);", txt)}
    return t["THIN_TX"], t["THIN_TY"], t["THIN_TZ"]


def _lowest(m):
    return m & (~m + np.uint32(1))


def _flood(seed, allowed, adj):
    r = seed
    while True:
        g = r.copy()
        for i, a in enumerate(adj):
            if a:
                g |= np.where((r >> np.uint32(i)) & np.uint32(1) != 0, np.uint32(a), np.uint32(0))
        g &= allowed
        if np.array_equal(g, r):
            return r
        r = g


def is_simple(m):
    """m: uint32 words of the object voxels of N26(p) -> the simple points (conditions (a) and (b) of the rule)"""
    m = np.asarray(m, np.uint32)
    a = (m != 0) & (_flood(_lowest(m), m, ADJ26) == m)
    b = ~m & np.uint32(N18)
    f = b & np.uint32(N6)
    return a & (f != 0) & ((f & ~_flood(_lowest(f), b, ADJ6)) == 0)


def is_end(m):
    m = np.asarray(m, np.uint32)
    return (m != 0) & (m & (m - np.uint32(1)) == 0)


def words(P, idx):
    """the neighbourhood words of the voxels at the flat indices idx of the padded object P"""
    _, H, W = P.shape
    flat = P.ravel()
    m = np.zeros(len(idx), np.uint32)
    for i, (dx, dy, dz) in enumerate(CELLS):
        if i != 13:
            m |= flat[idx + ((dz * H + dy) * W + dx)].astype(np.uint32) << np.uint32(i)
    return m


def thin(obj, max_rounds=0, history=None):
    """the rule on a boolean object -> (skeleton bool[l, h, w], rounds); history (a list): gains the object after every round"""
    obj = np.asarray(obj, bool)
    P = np.pad(obj, 1)  # outside the volume is background
    L, H, W = P.shape
    core = P[1:-1, 1:-1, 1:-1]
    rounds = 0
    while True:
        rounds += 1
        inner = P[:-2, 1:-1, 1:-1] & P[2:, 1:-1, 1:-1] & P[1:-1, :-2, 1:-1] & P[1:-1, 2:, 1:-1] & P[1:-1, 1:-1, :-2] & P[1:-1, 1:-1, 2:]
        cand = core & ~inner  # taken at the round's start
        z, y, x = np.nonzero(cand)
        sub = (x & 1) | (y & 1) << 1 | (z & 1) << 2
        flat = ((z + 1) * H + y + 1) * W + x + 1
        deleted = 0
        for s in range(8):
            idx = flat[sub == s]  # (a candidate is deleted in its own pass or never: all of them are still object)
            m = words(P, idx)
            gone = idx[is_simple(m) & ~is_end(m)]
            P.ravel()[gone] = False
            deleted += len(gone)
        if history is not None:
            history.append(core.copy())
        if deleted == 0 or rounds == max_rounds:
            return core.copy(), rounds


def degrees(skel):
    """the skeleton voxels in N26 of every skeleton voxel, in raster order"""
    P = np.pad(np.asarray(skel, bool), 1)
    L, H, W = P.shape
    z, y, x = np.nonzero(skel)
    m = words(P, ((z + 1) * H + y + 1) * W + x + 1)
    return np.array([bin(int(v)).count("1") for v in m], np.uint8)


def threshold(V, thr):
    return int(thr) if thr >= 0 else max(1, int(V.sum(dtype=np.uint64)) // V.size)


def skeletonize(V, thr=-1, max_rounds=0, history=None):
    """pnr_skeletonize on the u8 volume V -> (info without tiles / tile_visits, skel uint8 of 0 / 255, vox int64, deg uint8).  history:
    the list thin() filled on a run of this volume and threshold without a limit; the result is read from it, not computed again."""
    t = threshold(V, thr)
    obj = V >= t
    if history:
        rounds = min(max_rounds, len(history)) if max_rounds else len(history)
        skel = history[rounds - 1]
    else:
        skel, rounds = thin(obj, max_rounds)
    vox = np.flatnonzero(skel).astype(np.int64)
    deg = degrees(skel)
    info = {"n_vox": V.size, "n_fg": int(obj.sum()), "n_skel": len(vox), "n_end": int((deg == 1).sum()), "n_branch": int((deg >= 3).sum()),
            "n_isolated": int((deg == 0).sum()), "rounds": rounds, "thr_used": t}
    return info, np.where(skel, 255, 0).astype(np.uint8), vox, deg


def forest(vox, shape):
    """pnr_skeleton_forest: Kruskal over the 26-adjacent pairs under (len2, lo, hi) -> [(lo, hi, len2)] sorted by (lo, hi)"""
    l, h, w = shape
    node = {int(v): i for i, v in enumerate(vox)}
    edges = []
    for v, i in node.items():
        x, y, z = v % w, v // w % h, v // (w * h)
        for dx, dy, dz in CELLS:
            nx, ny, nz = x + dx, y + dy, z + dz
            if (dx, dy, dz) == (0, 0, 0) or not (0 <= nx < w and 0 <= ny < h and 0 <= nz < l):
                continue
            j = node.get(nx + w * (ny + h * nz))
            if j is not None and i < j:
                edges.append((dx * dx + dy * dy + dz * dz, i, j))
    up = list(range(len(node)))

    def find(a):
        while up[a] != a:
            up[a] = up[up[a]]
            a = up[a]
        return a

    kept = []
    for len2, i, j in sorted(edges):
        a, b = find(i), find(j)
        if a != b:
            up[max(a, b)] = min(a, b)
            kept.append((i, j, len2))
    return sorted(kept)


# ---- the invariants: what deleting simple points must keep ----
def topology(obj):
    """(26-components of the object, 6-components of the background padded by one, Euler number of the union of the closed voxels)"""
    from scipy import ndimage
    obj = np.asarray(obj, bool)
    n_obj = ndimage.label(obj, np.ones((3, 3, 3), int))[1]
    n_bg = ndimage.label(~np.pad(obj, 1), ndimage.generate_binary_structure(3, 1))[1]
    P = np.pad(obj, 1)

    def join(a, axis):  # the cells between two neighbours along the axis: present when either is
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        return a[tuple(lo)] | a[tuple(hi)]

    cubes = int(P.sum())
    faces = sum(int(join(P, k).sum()) for k in range(3))
    lines = sum(int(join(join(P, j), k).sum()) for j, k in ((0, 1), (0, 2), (1, 2)))
    points = int(join(join(join(P, 0), 1), 2).sum())
    return n_obj, n_bg, points - lines + faces - cubes


def simple_by_labels(m):
    """conditions (a) and (b) for ONE word by scipy.ndimage.label on the 3 x 3 x 3 cube: the check of is_simple"""
    from scipy import ndimage
    cube = np.array([(m >> i) & 1 for i in range(27)], bool).reshape(3, 3, 3)  # [dz + 1, dy + 1, dx + 1]
    n18 = np.array([(N18 >> i) & 1 for i in range(27)], bool).reshape(3, 3, 3)
    n6 = np.array([(N6 >> i) & 1 for i in range(27)], bool).reshape(3, 3, 3)
    if ndimage.label(cube, np.ones((3, 3, 3), int))[1] != 1:
        return False
    lab = ndimage.label(~cube & n18, ndimage.generate_binary_structure(3, 1))[0]
    ids = set(lab[n6 & ~cube].tolist())
    return len(ids) == 1


# ---- the volumes of the tests: object voxels are >= 100, the background is below ----
THR = 100
KINDS = ("zero", "full", "rand10", "rand31", "rand60", "rand90", "checker", "diagonal", "shell", "tubes", "blobs", "faces")


def ball(shape, centre, r):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= r * r


def objects(shape, kind, seed=7):
    l, h, w = shape
    rng = np.random.default_rng(seed + sum(map(ord, kind)) + 131 * l + 17 * h + w)
    z, y, x = np.ogrid[:l, :h, :w]
    TX, TY, TZ = tile()
    if kind == "zero":
        return np.zeros(shape, bool)
    if kind == "full":
        return np.ones(shape, bool)
    if kind.startswith("rand"):
        return rng.random(shape) < int(kind[4:]) / 100
    if kind == "checker":
        return ((x + y + z) & 1 == 0) & np.ones(shape, bool)
    if kind == "diagonal":  # 2 x 2 x 2 blocks that meet through the tile corners only
        o = np.zeros(shape, bool)
        for k in range(1, max(-(-w // TX), -(-h // TY), -(-l // TZ)) + 1):
            cx, cy, cz = k * TX, k * TY, k * TZ
            o |= (abs(2 * x - 2 * cx + 1) <= 3) & (abs(2 * y - 2 * cy + 1) <= 3) & (abs(2 * z - 2 * cz + 1) <= 3) & (
                ((x < cx) & (y < cy) & (z < cz)) | ((x >= cx) & (y >= cy) & (z >= cz)))
        return o
    if kind == "shell":  # a hollow box: the cavity has to stay
        lo = [1 if n > 4 else 0 for n in shape]
        box = lambda d: (z >= lo[0] + d) & (z < l - lo[0] - d) & (y >= lo[1] + d) & (y < h - lo[1] - d) & (x >= lo[2] + d) & (x < w - lo[2] - d)
        return box(0) & ~box(1)
    if kind == "tubes":
        o = np.zeros(shape, bool)
        for _ in range(4):
            a, b = rng.random(3) * shape, rng.random(3) * shape
            r = rng.integers(1, 3)
            for t in np.linspace(0, 1, 2 * max(shape)):
                o |= ball(shape, a + t * (b - a), r)
        return o
    if kind == "blobs":
        o = np.zeros(shape, bool)
        for _ in range(6):
            o |= ball(shape, rng.random(3) * shape, rng.integers(1, max(2, min(7, max(shape) // 4))))
        return o
    if kind == "faces":  # voxels on the tile faces only
        on = (x % TX == 0) | (x % TX == TX - 1) | (y % TY == 0) | (y % TY == TY - 1) | (z % TZ == 0) | (z % TZ == TZ - 1)
        return on & (rng.random(shape) < 0.6)
    raise ValueError(kind)


def volume(shape, kind, seed=7):
    """the u8 stack of a kind: the object voxels in 100..255, the others in 0..99"""
    o = objects(shape, kind, seed)
    rng = np.random.default_rng(seed + 1)
    return np.where(o, rng.integers(THR, 256, shape), rng.integers(0, THR, shape)).astype(np.uint8)
