"""The rule of pnr_label_components / pnr_despeckle_volume (include/pnr_hip.h) restated in numpy only: foreground V >= t, 6- or
26-neighbours, a component's `first` is its smallest linear index x + w * (y + h * z), the components of at least min_size voxels are
numbered 1..K in ascending first.  A union-find over the neighbour pairs of the 3 / 13 forward offsets: the larger root is hooked to
the smaller (np.minimum.at), the parents are compressed (P = P[P]) until nothing changes, and the roots are numbered by np.unique."""
import numpy as np

COMPONENT_DT = np.dtype([(k, np.int64) for k in ("first", "size", "sum", "sx", "sy", "sz")] + [(k, np.int32) for k in ("x0", "y0", "z0", "x1", "y1", "z1", "vmax", "pad")])


def threshold(V, thr=-1):
    """t of the rule: thr, or for thr == -1 max(1, floor(sum(V) / N)) from the exact integer sum"""
    return int(thr) if thr >= 0 else max(1, int(V.astype(np.uint64).sum()) // V.size)


def offsets(connectivity):
    """the forward half of the neighbourhood as (dz, dy, dx): 3 or 13 offsets"""
    out = []
    for dz in (0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) <= (0, 0, 0):
                    continue
                if connectivity == 6 and abs(dz) + abs(dy) + abs(dx) != 1:
                    continue
                out.append((dz, dy, dx))
    assert len(out) == {6: 3, 26: 13}[connectivity]
    return out


def _pairs(F, connectivity):
    l, h, w = F.shape
    idx = np.arange(F.size, dtype=np.int64).reshape(F.shape)
    a, b = [], []
    for dz, dy, dx in offsets(connectivity):
        za, zb = slice(0, l - dz), slice(dz, l)
        ya, yb = slice(max(0, -dy), h - max(0, dy)), slice(max(0, dy), h - max(0, -dy))
        xa, xb = slice(max(0, -dx), w - max(0, dx)), slice(max(0, dx), w - max(0, -dx))
        m = F[za, ya, xa] & F[zb, yb, xb]
        a.append(idx[za, ya, xa][m])
        b.append(idx[zb, yb, xb][m])
    return np.concatenate(a), np.concatenate(b)


def roots(F, connectivity):
    """per voxel the smallest linear index of its component (-1: background)"""
    P = np.arange(F.size, dtype=np.int64)
    a, b = _pairs(F, connectivity)
    while True:
        ra, rb = P[a], P[b]
        live = ra != rb
        if not live.any():
            break
        a, b = a[live], b[live]
        ra, rb = ra[live], rb[live]
        np.minimum.at(P, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            Q = P[P]
            if np.array_equal(Q, P):
                break
            P = Q
    P = P.reshape(F.shape)
    return np.where(F, P, -1)


def label(V, thr=-1, connectivity=26, min_size=1):
    """-> (info dict, labels int32[l, h, w], comps COMPONENT_DT[K])"""
    V = np.asarray(V, np.uint8)
    l, h, w = V.shape
    t = threshold(V, thr)
    F = V >= t
    R = roots(F, connectivity)
    fg = R[F]
    first, inv, size = np.unique(fg, return_inverse=True, return_counts=True)
    keep = size >= min_size
    number = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
    labels = np.zeros(V.shape, np.int32)
    labels[F] = number[inv]
    z, y, x = np.nonzero(F)
    v = V[F].astype(np.int64)
    n_all = len(first)
    comps = np.zeros(n_all, COMPONENT_DT)
    comps["first"], comps["size"] = first, size
    for name, val in (("sum", v), ("sx", x), ("sy", y), ("sz", z)):
        comps[name] = _isum(inv, val, n_all)
    for name, val, fn, init in (("x0", x, np.minimum, 2**31 - 1), ("y0", y, np.minimum, 2**31 - 1), ("z0", z, np.minimum, 2**31 - 1), ("x1", x, np.maximum, -1),
                                ("y1", y, np.maximum, -1), ("z1", z, np.maximum, -1), ("vmax", v, np.maximum, -1)):
        acc = np.full(n_all, init, np.int64)
        fn.at(acc, inv, val)
        comps[name] = acc
    info = dict(n_vox=V.size, n_fg=int(F.sum()), n_comp=int(keep.sum()), n_small=int((~keep).sum()), vox_small=int(size[~keep].sum()),
                largest=int(size[keep].max()) if keep.any() else 0, thr_used=t)
    return info, labels, comps[keep]


def _isum(inv, val, n):
    """exact integer sums per group"""
    acc = np.zeros(n, np.int64)
    np.add.at(acc, inv, val.astype(np.int64))
    return acc


def despeckle(V, min_size, thr=-1, connectivity=26):
    """-> (the volume with the foreground components below min_size cleared, info)"""
    V = np.asarray(V, np.uint8)
    info, labels, _ = label(V, thr, connectivity, min_size)
    F = V >= info["thr_used"]
    return np.where(F & (labels == 0), 0, V).astype(np.uint8), info


def centroid_rows(comps):
    """the rows of advantra_cli --per-component: id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax with the centroid as %.3f of the f64 quotient"""
    return ["%d,%d,%d,%.3f,%.3f,%.3f,%d,%d,%d,%d,%d,%d,%d" % (i + 1, c["size"], c["sum"], c["sx"] / c["size"], c["sy"] / c["size"], c["sz"] / c["size"],
                                                             c["x0"], c["y0"], c["z0"], c["x1"], c["y1"], c["z1"], c["vmax"]) for i, c in enumerate(comps)]
