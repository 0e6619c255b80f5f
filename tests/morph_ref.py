"""The rule of the grey-level morphological reconstruction (include/pnr_hip.h: pnr_morph_reconstruct, pnr_morph_volume) restated in numpy, in
two independent forms: the literal recursion R <- min(V, max over the offsets of shifted R) iterated until nothing changes, and a max-heap
widest-path solver of the path definition.  Exact u8 arithmetic; volumes are (l, h, w).  Also the test volumes that the host and the GPU
tests share."""
import heapq
import os
import re
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"dilate": 1, "erode": 2, "fill": 3, "hmax": 4, "hdome": 5}
CONNS = (4, 8, 6, 26)


def tile():
    """(TZ, TY, TX) of morph.h"""
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "morph.h")).read()
    t = {k: int(v) for k, v in re.findall(r"constexpr int MORPH_(TX|TY|TZ) = (\d+);", txt)}
    return t["TZ"], t["TY"], t["TX"]


def offsets(C):
    """the (dz, dy, dx) of N_C"""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nz = (dz != 0) + (dy != 0) + (dx != 0)
                if nz == 0 or (C in (4, 8) and dz) or (C in (4, 6) and nz != 1):
                    continue
                out.append((dz, dy, dx))
    assert len(out) == C
    return out


def default_conn(op):
    return 6 if OPS.get(op, op) == 3 else 26


def dilate(M, V, C):
    """rho_C(M, V), the literal recursion: a neighbour outside the volume does not exist (the padding is 0 and never wins a maximum)"""
    V = np.ascontiguousarray(V, np.uint8)
    R = np.minimum(np.asarray(M, np.uint8), V)
    l, h, w = V.shape
    offs = offsets(C)
    P = np.zeros((l + 2, h + 2, w + 2), np.uint8)
    iterations = 0
    while True:
        P[1:-1, 1:-1, 1:-1] = R
        D = R.copy()
        for dz, dy, dx in offs:
            np.maximum(D, P[1 + dz:1 + dz + l, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w], out=D)
        np.minimum(D, V, out=D)
        if np.array_equal(D, R):
            dilate.iterations = iterations
            return R
        R = D
        iterations += 1


def dilate_heap(M, V, C):
    """rho_C(M, V) from the path definition: R(p) = the maximum over the C-paths p0 .. pk = p of min(M'(p0), V(p1), .., V(pk)) -- the widest
    path from any start, settled in descending order with a max-heap"""
    V = np.ascontiguousarray(V, np.uint8)
    l, h, w = V.shape
    Mp = np.minimum(np.asarray(M, np.uint8), V)
    R = Mp.astype(np.int64).ravel().copy()
    Vf = V.astype(np.int64).ravel()
    done = np.zeros(V.size, bool)
    heap = [(-int(r), i) for i, r in enumerate(R) if r > 0]
    heapq.heapify(heap)
    offs = offsets(C)
    while heap:
        r, i = heapq.heappop(heap)
        r = -r
        if done[i] or r < R[i]:
            continue
        done[i] = True
        z, y, x = i // (w * h), i // w % h, i % w
        for dz, dy, dx in offs:
            qz, qy, qx = z + dz, y + dy, x + dx
            if 0 <= qz < l and 0 <= qy < h and 0 <= qx < w:
                q = (qz * h + qy) * w + qx
                cand = min(r, Vf[q])
                if cand > R[q]:
                    R[q] = cand
                    heapq.heappush(heap, (-int(cand), q))
    return R.astype(np.uint8).reshape(V.shape)


def erode(M, V, C, solver=dilate):
    """rho*_C(M, V) = 255 - rho_C(255 - M, 255 - V)"""
    return (255 - solver(255 - np.asarray(M, np.uint8), 255 - np.asarray(V, np.uint8), C)).astype(np.uint8)


def border(shape, C):
    """B_C: x or y on the first or last voxel of its axis, and for C in {6, 26} and l > 1 also z"""
    l, h, w = shape
    B = np.zeros(shape, bool)
    B[:, 0, :] = B[:, -1, :] = B[:, :, 0] = B[:, :, -1] = True
    if C in (6, 26) and l > 1:
        B[0] = B[-1] = True
    return B


def run(V, op, marker=None, h=0, C=0, solver=dilate):
    """the `out` volume of the op (a name of OPS) and the connectivity used"""
    V = np.ascontiguousarray(V, np.uint8)
    C = C or default_conn(op)
    if op == "dilate":
        out = solver(marker, V, C)
    elif op == "erode":
        out = erode(marker, V, C, solver)
    elif op == "fill":
        out = erode(np.where(border(V.shape, C), V, 255).astype(np.uint8), V, C, solver)
    else:
        assert 1 <= h <= 255
        hm = solver(np.maximum(V.astype(np.int32) - h, 0).astype(np.uint8), V, C)
        out = hm if op == "hmax" else (V - hm).astype(np.uint8)
    return out, C


def info(V, out, C):
    """the exact fields of pnr_morph_info (tile_visits and rounds are scheduling)"""
    TZ, TY, TX = tile()
    l, h, w = V.shape
    d = np.abs(out.astype(np.int32) - V.astype(np.int32))
    return {"n_vox": V.size, "n_changed": int((out != V).sum()), "n_nonzero": int((out > 0).sum()), "sum_in": int(V.sum(dtype=np.uint64)),
            "sum_out": int(out.sum(dtype=np.uint64)), "tiles": -(-l // TZ) * -(-h // TY) * -(-w // TX), "max_delta": int(d.max()), "connectivity": C}


# ---- test volumes ----
KINDS = ("zero", "full", "rand", "smooth", "steps", "snake", "faces", "hollow")


def shell(V, oz, oy, ox, n, wall, inside):
    """a cube of side n at (oz, oy, ox), clipped to the volume: walls one voxel thick around an inside of side n - 2"""
    l, h, w = V.shape

    def cut(o, m, ext):
        return slice(max(o, 0), max(min(o + m, ext), 0))
    V[cut(oz, n, l), cut(oy, n, h), cut(ox, n, w)] = wall
    V[cut(oz + 1, n - 2, l), cut(oy + 1, n - 2, h), cut(ox + 1, n - 2, w)] = inside


def hollow_ball(shape=(19, 21, 37), centre=(9, 10, 10), r_in=5, r_out=8):
    """the hollow soma of the issue: a shell of radii r_in .. r_out (200) around a dark nucleus (10), one neurite leaving it along x"""
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    d2 = (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2
    V = np.full(shape, 10, np.uint8)
    V[(d2 >= r_in * r_in) & (d2 <= r_out * r_out)] = 200
    V[centre[0], centre[1], centre[2] + r_out:shape[2] - 2] = 200
    return V


def volume(shape, kind, seed=11):
    l, h, w = shape
    TZ, TY, TX = tile()
    rng = np.random.default_rng(seed + 7919 * KINDS.index(kind) + l * 1000003 + h * 1009 + w)
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    if kind == "zero":
        return np.zeros(shape, np.uint8)
    if kind == "full":
        return np.full(shape, 255, np.uint8)
    if kind == "rand":
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == "smooth":  # blurred noise in steps of 8 grey levels: plateaus
        A = np.pad(rng.integers(0, 256, shape).astype(np.float64), 2, mode="edge")
        for ax in range(3):
            A = sum(np.roll(A, s, ax) for s in (-2, -1, 0, 1, 2)) / 5
        return (A[2:-2, 2:-2, 2:-2].astype(np.int64) // 8 * 8).astype(np.uint8)
    if kind == "steps":  # a few large flat levels
        coarse = rng.choice(np.array([0, 60, 120, 200, 255]), (-(-l // 3), -(-h // 7), -(-w // 9)))
        return coarse[z // 3, y // 7, x // 9].astype(np.uint8)
    if kind == "snake":  # a one-voxel corridor (200 in 0) in the planes z = 0 and the last, back and forth across the first x face between
        V = np.zeros(shape, np.uint8)  # tiles and down across three y faces: short enough for the literal recursion
        x0, x1 = max(min(TX - 3, w - 1), 0), max(min(TX + 2, w - 1), 0)
        for zz in {0, l - 1}:
            for yy in range(0, min(h, 3 * TY + 2), 2):
                V[zz, yy, x0:x1 + 1] = 200
                if yy + 1 < h:
                    V[zz, yy + 1, x1 if yy % 4 == 0 else x0] = 200
        V[:, 0, x0] = 200  # the planes are joined along z
        V[0, 0, x0] = 255  # a maximum at the start of the corridor
        return V
    if kind == "faces":  # structure on the first and last voxels of tiles only
        on = (x % TX == 0) | (x % TX == TX - 1) | (y % TY == 0) | (y % TY == TY - 1) | (z % TZ == 0) | (z % TZ == TZ - 1)
        return np.where(on, rng.integers(0, 256, shape), 128).astype(np.uint8)
    # hollow: cavities (20) behind walls (200) in a background of 60 -- inside one tile, across a tile corner, touching the border (not
    # filled), and one open only through a diagonal gap at a corner of its wall (filled under C = 6 and 4, not under C = 26 and 8)
    V = np.full(shape, 60, np.uint8)
    z1 = 1 if l >= 7 else -1 if l == 1 else 0  # (a single slice cuts every cube through its inside: rings)
    shell(V, z1, 1, 1, 5, 200, 20)
    shell(V, TZ - 2 if l > TZ + 3 else z1, TY - 2, TX - 2, 5, 200, 20)
    shell(V, z1, TY + 5, -1, 5, 200, 20)
    shell(V, z1, 1, 8, 5, 200, 20)
    if w > 8 and h > 1:
        V[max(z1, 0), 1, 8] = 20  # the corner of the last cube's wall
    return V


def markers(V, seed=5):
    """a random marker, a marker >= V, a zero marker"""
    rng = np.random.default_rng(seed + V.size)
    r = rng.integers(0, 256, V.shape).astype(np.uint8)
    return {"rand": r, "above": np.maximum(V, r), "zero": np.zeros(V.shape, np.uint8)}
