"""The rule of pnr_filter_volume (include/pnr_hip.h) restated in numpy: a sort over the edge-padded shifted copies for the median,
a plain loop over the in-volume offsets of every axis for the top-hat.  Volumes are u8 (l, h, w).  Nothing here shares an algorithm
with the kernels (pnr_amd/csrc/filter.hip)."""
import numpy as np


def median(V, mode):
    """mode 2: rank 4 of the 3 x 3 window in every slice; mode 3: rank 13 of the 3 x 3 x 3 window; coordinates clamped to the edge"""
    assert mode in (2, 3)
    V = np.asarray(V, np.uint8)
    l, h, w = V.shape
    P = np.pad(V, 1, mode="edge")
    dzs = (-1, 0, 1) if mode == 3 else (0,)
    stack = [P[1 + dz:1 + dz + l, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dz in dzs for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.ascontiguousarray(np.sort(np.stack(stack), axis=0)[len(stack) // 2])


def box(R, zdist, l):
    """half-widths (rz, ry, rx) of the top-hat's box: rz = (int)((float)R / zd) as one f32 division, 0 in the 2-D mode"""
    rz = 0 if l == 1 else int(np.float32(R) / np.float32(zdist))
    return rz, R, R


def _extreme(V, r, axis, fn):
    """fn (np.minimum / np.maximum) over the offsets -r..r of one axis that stay inside the volume"""
    n = V.shape[axis]
    out = V.copy()
    for d in range(1, min(r, n - 1) + 1):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
        lo, hi = tuple(lo), tuple(hi)
        out[lo] = fn(out[lo], V[hi])  # the neighbour at +d
        out[hi] = fn(out[hi], V[lo])  # the neighbour at -d
    return out


def erode(V, radii):
    for axis, r in enumerate(radii):
        V = _extreme(V, r, axis, np.minimum)
    return V


def dilate(V, radii):
    for axis, r in enumerate(radii):
        V = _extreme(V, r, axis, np.maximum)
    return V


def opening(V, R, zdist):
    V = np.asarray(V, np.uint8)
    radii = box(R, zdist, V.shape[0])
    return dilate(erode(V, radii), radii)


def tophat(V, R, zdist):
    """V - max over the box of (min over the box of V), the box cut to the volume"""
    V = np.asarray(V, np.uint8)
    o = opening(V, R, zdist)
    assert (o <= V).all()
    return V - o


def apply(V, median_mode, R, zdist):
    """both stages in the order of the rule: median first, then top-hat; 0 skips a stage"""
    V = np.ascontiguousarray(V, np.uint8)
    if median_mode:
        V = median(V, median_mode)
    if R:
        V = tophat(V, R, zdist)
    return V
