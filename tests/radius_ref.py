"""numpy restatement of pnr_measure_radii's rule (include/pnr_hip.h), for the tests: the shells from the f32 distance, and the
measurement vectorised per shell over the nodes that are still alive.  Exact integer arithmetic; f32 where the rule says f32."""
import numpy as np

F = np.float32


def shells(zdist, rmax, is2d=False):
    """[O_0, ..., O_rmax]: int arrays (n_k, 3) of (dx, dy, dz)"""
    zd = F(zdist)
    r = np.arange(-rmax, rmax + 1)
    dz, dy, dx = np.meshgrid(np.array([0]) if is2d else r, r, r, indexing="ij")
    zt = zd * dz.astype(F)
    d2 = (dx * dx + dy * dy).astype(F) + zt * zt
    assert d2.dtype == F
    out = [np.zeros((1, 3), np.int64)]
    for k in range(1, rmax + 1):
        m = (d2 > F((k - 1) * (k - 1))) & (d2 <= F(k * k))
        out.append(np.stack([dx[m], dy[m], dz[m]], 1).astype(np.int64))
    return out


def centres(xyz, shape):
    """(finite mask, int64 centres (n, 3) as (cx, cy, cz)): c = (int) fminf(fmaxf(v + 0.5f, 0), n - 1)"""
    l, h, w = shape
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    fin = np.isfinite(xyz).all(1)
    v = np.where(fin[:, None], xyz, F(0))
    with np.errstate(over="ignore"):
        c = [np.minimum(np.maximum(v[:, a] + F(0.5), F(0)), F(n - 1)).astype(np.int64) for a, n in enumerate((w, h, l))]
    return fin, np.stack(c, 1)


def _gather(V, c, off):
    """in-volume mask and voxel values of the offsets `off` around the centres c: (n, n_off) each"""
    l, h, w = V.shape
    x = c[:, 0, None] + off[None, :, 0]
    y = c[:, 1, None] + off[None, :, 1]
    z = c[:, 2, None] + off[None, :, 2]
    inb = (x >= 0) & (x < w) & (y >= 0) & (y < h) & (z >= 0) & (z < l)
    idx = np.where(inb, (z * h + y) * w + x, 0)
    return inb, V.reshape(-1)[idx].astype(np.int64)


def measure(V, zdist, xyz, thr=-1, rel_pct=50, rmax=32, bg_permille=1, sh=None):
    """-> (k int32[n], thr_used)"""
    V = np.ascontiguousarray(V, np.uint8)
    is2d = V.shape[0] == 1
    sh = sh if sh is not None else shells(zdist, rmax, is2d)
    fin, c = centres(xyz, V.shape)
    n = len(c)
    k_out = np.full(n, -1, np.int32)
    thr_used = 0
    if rel_pct == 0:
        thr_used = thr if thr >= 0 else max(1, int(V.sum(dtype=np.uint64)) // V.size)
        t = np.full(n, thr_used, np.int64)
    else:
        inb, val = _gather(V, c, np.concatenate(sh[:2]))
        m = np.where(inb, val, 0).max(1)
        t = np.maximum(1, (rel_pct * m + 99) // 100)
    alive = np.flatnonzero(fin)
    tot = np.zeros(n, np.int64)
    bg = np.zeros(n, np.int64)
    for k in range(rmax + 1):
        if len(alive) == 0:
            break
        off = sh[k]
        step = max(1, (1 << 22) // max(1, len(off)))  # nodes per chunk
        for s in range(0, len(alive), step):
            a = alive[s:s + step]
            inb, val = _gather(V, c[a], off)
            tot[a] += inb.sum(1)
            bg[a] += (inb & (val < t[a, None])).sum(1)
        fail = 1000 * bg[alive] > bg_permille * tot[alive]
        k_out[alive[fail]] = max(0, k - 1)
        alive = alive[~fail]
    k_out[alive] = rmax
    return k_out, thr_used
