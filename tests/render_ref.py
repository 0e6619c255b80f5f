"""numpy restatement of the render rule (include/pnr_hip.h: pnr_render_tree, pnr_tree_coverage), for the tests: every voxel of the grid
against every segment in float32, one IEEE operation per numpy operation, with the conventions of distance_ref.py (its `scaled`, its F,
the float32 assertion on d2); the coverage counts in exact integers."""
import numpy as np
from distance_ref import F, scaled


def radii(radius, rscale=1, radd=0):
    """rr = fmaxf(radius * rscale + radd, 0): one multiply, one add"""
    return np.maximum(np.asarray(radius, F).reshape(-1) * F(rscale) + F(radd), F(0))


def inside(shape, a, b, ra, rb, zscale=1, origin=(0, 0, 0)):
    """bool[l, h, w]: the voxels of the grid inside the segment (a, b) with the radii (ra, rb); a, b scaled float32[3].  origin = (z0, y0, x0):
    the grid is the part of a larger one that starts at this voxel (the voxel coordinates, not the array indices, enter the f32 arithmetic)"""
    l, h, w = shape
    z0, y0, x0 = origin
    px = np.arange(x0, x0 + w, dtype=F)[None, None, :]
    py = np.arange(y0, y0 + h, dtype=F)[None, :, None]
    pz = (np.arange(z0, z0 + l, dtype=F) * F(zscale))[:, None, None]
    a, b = np.asarray(a, F), np.asarray(b, F)
    ab = b - a
    den = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2]
    r = F(1) / den if den > 0 else F(0)
    dr = F(rb) - F(ra)
    apx, apy, apz = px - a[0], py - a[1], pz - a[2]
    num = (apx * ab[0] + apy * ab[1]) + apz * ab[2]
    t = np.minimum(np.maximum(num * r, F(0)), F(1))
    ex, ey, ez = px - (a[0] + t * ab[0]), py - (a[1] + t * ab[1]), pz - (a[2] + t * ab[2])
    d2 = (ex * ex + ey * ey) + ez * ez
    rt = F(ra) + t * dr
    assert d2.dtype == F and rt.dtype == F and t.dtype == F
    return d2 <= rt * rt


def render(xyz, radius, parent, shape, zscale=1, rscale=1, radd=0, origin=(0, 0, 0)):
    """-> L int32[l, h, w]: 1 + the smallest segment that holds the voxel, 0 for none (origin: see inside())"""
    x = scaled(xyz, zscale)
    rr = radii(radius, rscale, radd)
    parent = np.asarray(parent).reshape(-1)
    L = np.zeros(shape, np.int32)
    for i in range(len(x) - 1, -1, -1):  # descending: the smallest index is written last
        q = i if parent[i] < 0 else int(parent[i])
        L[inside(shape, x[i], x[q], rr[i], rr[q], zscale, origin)] = i + 1
    return L


def threshold(V, thr=-1):
    return int(thr) if thr >= 0 else max(1, int(V.astype(np.uint64).sum()) // V.size)


def coverage(V, L, n, thr=-1):
    """-> (dict as Context.tree_coverage gives it, seg_vox, seg_fg, seg_sum int64[n], residual uint8) from exact integer sums"""
    t = threshold(V, thr)
    fg, tree = V >= t, L > 0
    V64 = V.astype(np.int64)
    c = {"n_vox": int(V.size), "n_tree": int(tree.sum()), "n_fg": int(fg.sum()), "n_both": int((fg & tree).sum()), "sum_fg": int(V64[fg].sum()),
         "sum_both": int(V64[fg & tree].sum()), "thr_used": t}
    c["covered"] = c["n_both"] / c["n_fg"] if c["n_fg"] else 0.0
    c["on_signal"] = c["n_both"] / c["n_tree"] if c["n_tree"] else 0.0
    c["covered_intensity"] = c["sum_both"] / c["sum_fg"] if c["sum_fg"] else 0.0
    lab = L[tree].astype(np.int64) - 1
    seg_vox = np.bincount(lab, minlength=n).astype(np.int64)
    seg_fg = np.bincount(lab, weights=fg[tree], minlength=n).astype(np.int64)
    seg_sum = np.bincount(lab, weights=V64[tree], minlength=n).astype(np.int64)
    return c, seg_vox, seg_fg, seg_sum, np.where(tree, 0, V).astype(np.uint8)


def radius_mix(rng, n, kind):
    """the radii of the fuzz: all 0, one constant, tapering along the node order, or small ones with a single 12"""
    if kind == "zero":
        return np.zeros(n, F)
    if kind == "const":
        return np.full(n, 1.5, F)
    if kind == "taper":
        return np.linspace(4, 0.25, n).astype(F)
    r = rng.uniform(0, 2.5, n).astype(F)
    r[int(rng.integers(0, n))] = 12
    return r
