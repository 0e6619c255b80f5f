"""numpy restatement of the tree distance's rule (include/pnr_hip.h: pnr_point_segment_distance, pnr_tree_sample, pnr_tree_distance), for
the tests: the point-to-segment distance in float32 over the whole n x m matrix with the packed-key minimum, the sampling in float64,
the metrics from sequential float64 sums (np.cumsum(...)[-1]; np.sum adds pairwise)."""
import numpy as np

F = np.float32


def point_segment(pts, a, b, rows=512):
    """n x 3 points against the m segments (a[j], b[j]) -> (d float32[n], j int32[n]); `rows` points at a time"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    a = np.ascontiguousarray(a, F).reshape(-1, 3)
    b = np.ascontiguousarray(b, F).reshape(-1, 3)
    m = len(a)
    ab = b - a
    den = (ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]) + ab[:, 2] * ab[:, 2]
    with np.errstate(divide="ignore"):
        r = np.where(den > 0, F(1) / den, F(0)).astype(F)
    idx = np.arange(m, dtype=np.uint64)
    d = np.empty(len(pts), F)
    j = np.empty(len(pts), np.int32)
    for p0 in range(0, len(pts), rows):
        p = pts[p0:p0 + rows]
        ap = [p[:, None, k] - a[None, :, k] for k in range(3)]
        num = (ap[0] * ab[:, 0] + ap[1] * ab[:, 1]) + ap[2] * ab[:, 2]
        t = np.minimum(np.maximum(num * r, F(0)), F(1))
        e = [p[:, None, k] - (a[None, :, k] + t * ab[None, :, k]) for k in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        assert d2.dtype == F and not np.signbit(d2).any()
        key = (np.ascontiguousarray(d2).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None, :]
        best = key.min(1)
        d[p0:p0 + rows] = np.sqrt((best >> np.uint64(32)).astype(np.uint32).view(F))
        j[p0:p0 + rows] = (best & np.uint64(0xffffffff)).astype(np.int32)
    return d, j


def scaled(xyz, zscale):
    x = np.array(xyz, F).reshape(-1, 3)
    x[:, 2] = x[:, 2] * F(zscale)
    return x


def tree_sample(xyz, parent, zscale=1, step=1):
    """-> (pts float32[k, 3], owner int32[k]): in node order the node, then the interior points of its segment"""
    x = scaled(xyz, zscale)
    step = np.float64(F(step))
    pts, owner = [], []
    for i, par in enumerate(np.asarray(parent).reshape(-1)):
        pts.append(x[i])
        owner.append(i)
        if par < 0 or not step > 0:
            continue
        a, b = x[i].astype(np.float64), x[par].astype(np.float64)
        d = b - a
        L = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        q = int(np.ceil(L / step))
        for k in range(1, q):
            pts.append((a + d * (np.float64(k) / np.float64(q))).astype(F))
            owner.append(i)
    return np.array(pts, F).reshape(-1, 3), np.array(owner, np.int32)


def segments(xyz, parent, zscale=1):
    """one segment per node: (x_i, x_parent[i]), or (x_i, x_i) without a parent"""
    x = scaled(xyz, zscale)
    parent = np.asarray(parent).reshape(-1)
    return x, x[np.where(parent < 0, np.arange(len(x)), parent)]


def direction(d, thr):
    d64 = d.astype(np.float64)
    big = d >= F(thr)
    nb = int(big.sum())
    return {"n": len(d), "n_big": nb, "mean": float(np.cumsum(d64)[-1] / len(d)), "ssd": float(np.cumsum(d64[big])[-1] / nb) if nb else 0.0,
            "pct": nb / len(d), "max": float(d.max())}


def tree_distance(xyzA, parentA, xyzB, parentB, zscale=1, step=1, thr=2):
    """-> (result dict as Context.tree_distance gives it, (dA, ownerA), (dB, ownerB))"""
    pa, oa = tree_sample(xyzA, parentA, zscale, step)
    pb, ob = tree_sample(xyzB, parentB, zscale, step)
    da, _ = point_segment(pa, *segments(xyzB, parentB, zscale))
    db, _ = point_segment(pb, *segments(xyzA, parentA, zscale))
    ab, ba = direction(da, thr), direction(db, thr)
    res = {"ab": ab, "ba": ba, "sd": (ab["mean"] + ba["mean"]) / 2, "ssd": (ab["ssd"] + ba["ssd"]) / 2, "pct": (ab["pct"] + ba["pct"]) / 2,
           "hausdorff": max(ab["max"], ba["max"])}
    return res, (da, oa), (db, ob)


def random_forest(rng, n, roots=3, extent=64.0, step=1.5):
    """n nodes in `roots` trees: every later node hangs off an earlier node of its tree, `step` away on average, inside [0, extent)"""
    xyz = np.zeros((n, 3), F)
    parent = np.full(n, -1, np.int32)
    xyz[:roots] = rng.random((min(roots, n), 3)) * extent
    for i in range(roots, n):
        p = int(rng.integers(max(0, i - 6), i))
        parent[i] = p
        xyz[i] = np.clip(xyz[p] + rng.normal(0, step, 3), 0, extent - 0.01)
    return xyz, parent
