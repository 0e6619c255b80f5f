"""Plain numpy reference of what the GPU half of the seed stage computes per layer of J8 -- the extremes, the pixels above the
minimum, the 8-neighbour local maxima and their sort keys (oracle/pnr_oracle.c:437-469, its restatement of seed.cpp:578-632) -- in
integer and float32 arithmetic, and the stacks on which tests/test_gpu_seed_handover.py, tests/test_gpu_seeds.py and
tests/test_seed_handover_host.py use it.  Everything here is computed once per stack and handed out read-only."""
import functools
import numpy as np

# (w, h, l): no interior / tiny layers; the 256-pixel wave tile; the 1024-pixel work-group and its trailing waves; a second round of
# the values' per-row prefix (w > 4352); the row scan's carry with a partial last round (h > 256); the 16 download chunks
SHAPES = [(1, 1, 1), (2, 5, 2), (5, 2, 2), (3, 3, 1), (4, 3, 3), (7, 9, 2),
          (255, 4, 2), (256, 4, 2), (257, 5, 3), (259, 3, 2),
          (1023, 3, 2), (1025, 3, 2), (1281, 4, 1), (2049, 3, 1),
          (4400, 3, 2), (8500, 3, 1),
          (37, 257, 2), (12, 600, 2), (8, 512, 1),
          (16, 9, 15), (16, 9, 16), (16, 9, 17), (16, 9, 33)]
KINDS = ["sparse", "dense", "mix", "edge"]
E2E_KINDS = ["sparse", "dense", "mix"]
TOLERANCES = [0, 0.5, 5, 100, 254, 255, 1000]
J8_CHUNKS = 16  # pnr_ctx::J8_CHUNKS: the values come down in 16 chunks of ceil(l / 16) layers


def shape_id(shape):
    return "%dx%dx%d" % shape


def has_interior(shape):
    return shape[0] >= 3 and shape[1] >= 3


def _freeze(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def stack(shape, kind):
    """J8 (l, h, w) u8 of one content kind, from a RandomState fixed by (shape, kind)"""
    w, h, l = shape
    rs = np.random.RandomState(1000 * SHAPES.index(shape) + KINDS.index(kind))
    dims = (l, h, w)
    if kind == "sparse":  # the production case: ~5 % above a minimum of 0, most wave tiles empty
        J8 = np.where(rs.rand(*dims) < 0.05, rs.randint(1, 256, dims), 0).astype(np.uint8)
        if has_interior(shape):  # a 255 inside every layer: the one maximum that a tolerance of 254 still accepts
            for z in range(l):
                J8[z, rs.randint(1, h - 1), rs.randint(1, w - 1)] = 255
    elif kind == "dense":  # minimum 7 at a single pixel, everything else above it
        J8 = rs.randint(8, 256, dims).astype(np.uint8)
        for z in range(l):
            J8[z, rs.randint(h), rs.randint(w)] = 7
    elif kind == "mix":  # products of two draws: many plateaus and ties (tests/test_gpu_seeds.py test_seeds_random_layers)
        J8 = (rs.randint(0, 6, dims) * rs.randint(0, 50, dims)).astype(np.uint8)
    else:  # edge: values on both sides of 128 side by side, a plateau of equal values on the image border, a 255 and a 0
        J8 = rs.randint(100, 156, dims).astype(np.uint8)
        J8[:, :h // 2 + 1, :w // 3 + 1] = 140
        for z in range(l):
            p = rs.choice(w * h, min(2, w * h), replace=False)
            J8[z].flat[p[0]] = 255
            if len(p) > 1:
                J8[z].flat[p[1]] = 0
    if l >= 15:
        # every third layer flat (alternately 0 and 9); one whole download chunk all zero: no value to copy for it, and layers
        # without candidates between layers that wait for their chunk
        for z in range(2, l, 3):
            J8[z] = 0 if (z // 3) % 2 == 0 else 9
        per = -(-l // J8_CHUNKS)
        J8[2 * per:3 * per] = 0
    return _freeze(J8)


@functools.lru_cache(maxsize=None)
def directions(shape):
    """random Vx, Vy, Vz (l, h, w) u8 for the end-to-end runs"""
    w, h, l = shape
    rs = np.random.RandomState(77 + SHAPES.index(shape))
    return tuple(_freeze(rs.randint(0, 256, (l, h, w)).astype(np.uint8)) for _ in range(3))


def layer_keys(L):
    """sorted candidate keys of one layer (h, w) u8: pixels inside the border, not at the layer minimum, without a greater
    8-neighbour; key = (int32)(float32(v - gmin) * float32(2e9 / (gmax - gmin))) << 32 | y * w + x"""
    h, w = L.shape
    gmin, gmax = int(L.min()), int(L.max())
    if gmin == gmax or w < 3 or h < 3:  # a flat layer has no candidate (every pixel is the minimum)
        return np.zeros(0, np.int64)
    v = L[1:-1, 1:-1].astype(np.int32)
    nb = np.zeros_like(v)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                nb = np.maximum(nb, L[dy:dy + h - 2, dx:dx + w - 2])
    ys, xs = np.nonzero((v != gmin) & (nb <= v))
    vfactor = np.float32(2e9 / float(np.float32(gmax) - np.float32(gmin)))  # double division, rounded to float (:458)
    ivalue = ((v[ys, xs].astype(np.float32) - np.float32(gmin)) * vfactor).astype(np.int32)  # float32 product, truncated (:465)
    p = (ys + 1).astype(np.int64) * w + (xs + 1)
    return np.sort((ivalue.astype(np.int64) << 32) | p)


def handover(J8):
    """the reference hand-over of a stack (n, h, w): vmin, vmax, ltot, key_off, keys as Context.seed_handover returns them"""
    n = len(J8)
    flat = J8.reshape(n, -1)
    vmin = flat.min(1).astype(np.int32) if n else np.zeros(0, np.int32)
    vmax = flat.max(1).astype(np.int32) if n else np.zeros(0, np.int32)
    ltot = np.count_nonzero(flat > vmin[:, None].astype(np.uint8), axis=1).astype(np.int64) if n else np.zeros(0, np.int64)
    keys = [layer_keys(L) for L in J8]
    key_off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    return dict(vmin=vmin, vmax=vmax, ltot=ltot, key_off=key_off, keys=np.concatenate(keys + [np.zeros(0, np.int64)]))


@functools.lru_cache(maxsize=None)
def stack_handover(shape, kind):
    return {k: _freeze(a) for k, a in handover(stack(shape, kind)).items()}


_oracle_seeds = {}


def oracle_seeds(oracle, shape, kind, tol):
    """orc.extract_seeds of one stack with its random directions, (n, 8) f32: computed once per (stack, tolerance)"""
    import orc
    key = (shape, kind, float(tol))
    if key not in _oracle_seeds:
        _oracle_seeds[key] = _freeze(orc.extract_seeds(oracle, tol, stack(shape, kind), *directions(shape)))
    return _oracle_seeds[key]
