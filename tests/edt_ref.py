"""numpy restatement of pnr_distance_transform's rule (include/pnr_hip.h), for the tests.  brute() is the rule as it is written: every
foreground voxel against every background voxel, for tiny stacks.  transform() is the separable min-plus form over shifted arrays
(O(N) memory, offsets up to min(rmax, extent) - 1): integer minima along x and y, one f32 addition per z offset.  f32 exactly where the
rule says f32; everything else is exact integer arithmetic."""
import numpy as np
import radius_ref

F = np.float32


def threshold(V, thr=-1):
    return int(thr) if thr >= 0 else max(1, int(V.sum(dtype=np.uint64)) // V.size)


def brute(V, t, zd, rmax):
    """D2 float32 (l, h, w): min(cap, min over the background q of (float)(dx^2 + dy^2) + (zd (float)dz) (zd (float)dz))"""
    V = np.asarray(V, np.uint8)
    zd, cap = F(zd), F(rmax * rmax)
    fg = np.argwhere(V >= t).astype(np.int64)  # (z, y, x)
    bg = np.argwhere(V < t).astype(np.int64)
    out = np.zeros(V.shape, F)
    if len(fg) == 0:
        return out
    best = np.full(len(fg), cap, F)
    if len(bg):
        d = bg[None, :, :] - fg[:, None, :]
        zt = zd * d[..., 0].astype(F)
        d2 = (d[..., 2] * d[..., 2] + d[..., 1] * d[..., 1]).astype(F) + zt * zt
        assert d2.dtype == F
        best = np.minimum(best, d2.min(1))
    out[fg[:, 0], fg[:, 1], fg[:, 2]] = best
    return out


def transform(V, thr, zd, rmax):
    """-> (D2 float32 (l, h, w), t)"""
    V = np.asarray(V, np.uint8)
    l, h, w = V.shape
    t = threshold(V, thr)
    zd, cap = F(zd), rmax * rmax
    bg = V < t
    gx = np.where(bg, 0, cap).astype(np.int64)
    for k in range(1, min(rmax, w)):
        gx[:, :, k:] = np.minimum(gx[:, :, k:], np.where(bg[:, :, :-k], k * k, cap))
        gx[:, :, :-k] = np.minimum(gx[:, :, :-k], np.where(bg[:, :, k:], k * k, cap))
    gy = gx.copy()
    for k in range(1, min(rmax, h)):
        gy[:, k:, :] = np.minimum(gy[:, k:, :], gx[:, :-k, :] + k * k)
        gy[:, :-k, :] = np.minimum(gy[:, :-k, :], gx[:, k:, :] + k * k)
    g = gy.astype(F)  # (at most rmax^2 <= 2^20: exact)
    D = g.copy()
    for k in range(1, min(rmax, l)):
        zt = (zd * F(k)) * (zd * F(k))
        D[k:] = np.minimum(D[k:], g[:-k] + zt)
        D[:-k] = np.minimum(D[:-k], g[k:] + zt)
    assert D.dtype == F
    return D, t


def info(V, D2, t, rmax):
    """the summary as Context.distance_transform returns it"""
    l, h, w = V.shape
    fg = np.asarray(V) >= t
    n_fg = int(fg.sum())
    out = dict(n_vox=int(V.size), n_fg=n_fg, n_capped=int((fg & (D2 == F(rmax * rmax))).sum()), first_max=-1, d2_max=0.0, thr_used=int(t), d_max=0.0, max_at=None)
    if n_fg:
        m = D2[fg].max()
        i = int(np.flatnonzero(fg.ravel() & (D2.ravel() == m))[0])
        out.update(first_max=i, d2_max=float(m), d_max=float(np.sqrt(F(m))), max_at=(i % w, (i // w) % h, i // (w * h)))
    return out


def at(D2, xyz):
    """D2 at the centre voxels of the radius rule; -1 for a position that is not finite"""
    fin, c = radius_ref.centres(xyz, D2.shape)
    return np.where(fin, D2[c[:, 2], c[:, 1], c[:, 0]], F(-1)).astype(F)
