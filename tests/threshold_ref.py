"""The threshold rules of include/pnr_hip.h restated in numpy and plain Python: the methods on a 256-bin histogram in Python ints (and
float64 in the stated order for Otsu's score), the local threshold on an int64 summed-volume table -- and, for tiny shapes, as the
literal triple loop over the box."""
import numpy as np

METHODS = ("mean", "otsu", "triangle", "top", "maxentropy")
F = np.float32


def histogram(V):
    return np.bincount(np.asarray(V, np.uint8).reshape(-1), minlength=256).astype(np.uint64)


def _otsu(H, lo, n, S):
    best, raw = None, None
    n0 = S0 = 0
    for t in range(lo + 1, 256):
        n0, S0 = n0 + H[t - 1], S0 + (t - 1) * H[t - 1]  # the bins [lo, t)
        n1, S1 = n - n0, S - S0
        if n0 == 0 or n1 == 0:
            continue
        w0, w1 = float(n0), float(n1)
        d = float(S1) / w1 - float(S0) / w0
        score = ((w0 * w1) * d) * d
        if best is None or score > best:
            best, raw = score, t
    if raw is None:
        (raw,) = [v for v in range(lo, 256) if H[v]]
    return raw


def _triangle(H, lo):
    counted = range(lo, 256)
    p = max(counted, key=lambda v: (H[v], -v))
    e = max(v for v in counted if H[v] > 0)
    if e - p < 2:
        return e
    g = {b: (H[p] - H[e]) * (e - b) + (H[e] - H[b]) * (e - p) for b in range(p + 1, e)}
    return max(g, key=lambda b: (g[b], -b)) + 1


def _top(H, lo, n, top_ppm):
    k = n * top_ppm // 10**6
    for t in range(lo, 256):
        if sum(H[t:]) <= k:
            return t
    return 255


def from_hist(H, method, lo=0, top_ppm=None, maxentropy=None):
    """-> the info dict of pnr_threshold_from_hist.  maxentropy: the oracle's function on an int64 histogram (that method only)"""
    H = [int(v) for v in np.asarray(H).reshape(-1)]
    assert len(H) == 256 and method in METHODS and 0 <= lo <= 255
    n, S = sum(H[lo:]), sum(v * H[v] for v in range(lo, 256))
    nz = [v for v in range(lo, 256) if H[v]]
    info = dict(n_vox=sum(H), n_counted=n, sum_counted=S, method=method, lo=lo, v_min=nz[0] if nz else -1, v_max=nz[-1] if nz else -1,
                peak=max(nz, key=lambda v: (H[v], -v)) if nz else -1)
    if n == 0:
        thr = 255
    else:
        if method == "mean":
            raw = S // n
        elif method == "otsu":
            raw = _otsu(H, lo, n, S)
        elif method == "triangle":
            raw = _triangle(H, lo)
        elif method == "top":
            raw = _top(H, lo, n, top_ppm)
        else:
            assert lo == 0 and max(H) < 2**31
            raw = int(maxentropy(np.array(H, np.int64)))
        thr = min(255, max(raw, lo, 1))
    info.update(thr=thr, n_fg=sum(H[thr:]))
    return info


def resolve(V, word, maxentropy=None):
    """a threshold word ("otsu", "triangle:1", "top1.5", ...) on the volume V -> the number"""
    name, _, lo = word.partition(":")
    ppm = None
    if name.startswith("top"):
        name, ppm = "top", int(round(float(name[3:]) * 1e4))
    return from_hist(histogram(V), name, int(lo) if lo else 0, ppm, maxentropy)["thr"]


def box(r, zdist, l):
    """(rx, ry, rz) of the local threshold: the top-hat's box"""
    return r, r, 0 if l == 1 else int(F(r) / F(zdist))


def _decide(V, n, S, offset, scale_256, floor, binary):
    v = V.astype(np.int64)
    keep = (v >= floor) & (256 * n * v >= scale_256 * S + 256 * offset * n)
    out = np.where(keep, 255 if binary else V, 0).astype(np.uint8)
    return out, keep


def local_sums(V, r, zdist):
    """-> (n, S): the size and the sum of the box around every voxel, cut to the volume; an int64 summed-volume table"""
    l, h, w = V.shape
    rx, ry, rz = box(r, zdist, l)
    T = np.zeros((l + 1, h + 1, w + 1), np.int64)
    T[1:, 1:, 1:] = V.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    z0, z1 = np.maximum(np.arange(l) - rz, 0), np.minimum(np.arange(l) + rz, l - 1) + 1
    y0, y1 = np.maximum(np.arange(h) - ry, 0), np.minimum(np.arange(h) + ry, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - rx, 0), np.minimum(np.arange(w) + rx, w - 1) + 1
    Z0, Z1, Y0, Y1, X0, X1 = z0[:, None, None], z1[:, None, None], y0[None, :, None], y1[None, :, None], x0[None, None, :], x1[None, None, :]
    S = (T[Z1, Y1, X1] - T[Z0, Y1, X1] - T[Z1, Y0, X1] - T[Z1, Y1, X0] + T[Z0, Y0, X1] + T[Z0, Y1, X0] + T[Z1, Y0, X0] - T[Z0, Y0, X0])
    n = (Z1 - Z0) * (Y1 - Y0) * (X1 - X0)
    return n.astype(np.int64), S


def local(V, r, zdist, offset=0, scale_256=256, floor=1, binary=False):
    """-> (out uint8, info dict of pnr_local_threshold)"""
    V = np.asarray(V, np.uint8)
    n, S = local_sums(V, r, zdist)
    out, keep = _decide(V, n, S, offset, scale_256, floor, binary)
    rx, ry, rz = box(r, zdist, V.shape[0])
    return out, dict(n_vox=V.size, n_kept=int(keep.sum()), sum_in=int(V.sum(dtype=np.int64)), sum_out=int(out.sum(dtype=np.int64)), rx=rx, ry=ry, rz=rz)


def local_loops(V, r, zdist, offset=0, scale_256=256, floor=1, binary=False):
    """the rule as it is written: a loop over the box of every voxel (tiny shapes)"""
    V = np.asarray(V, np.uint8)
    l, h, w = V.shape
    rx, ry, rz = box(r, zdist, l)
    out = np.zeros_like(V)
    for z in range(l):
        for y in range(h):
            for x in range(w):
                n = S = 0
                for zz in range(z - rz, z + rz + 1):
                    for yy in range(y - ry, y + ry + 1):
                        for xx in range(x - rx, x + rx + 1):
                            if 0 <= zz < l and 0 <= yy < h and 0 <= xx < w:
                                n += 1
                                S += int(V[zz, yy, xx])
                v = int(V[z, y, x])
                if v >= floor and 256 * n * v >= scale_256 * S + 256 * offset * n:
                    out[z, y, x] = 255 if binary else v
    return out
