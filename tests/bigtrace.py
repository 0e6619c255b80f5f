"""The stack of 2048 x 2048 x 536 voxels (N = 2 248 146 944 > 2^31) that takes the tracing path -- the Gaussian and Hessian stages of Frangi,
J8, the direction bytes, seed extraction, ZNCC scoring, the SMC tracer, the replay's density map and the streaming scheduler -- above the
sign bit of a 32-bit voxel index, and a stack of 160 x 96 x 72 with the same blocks at the same offsets from the faces, which the oracle
can take as a whole.  bigvol.py does the same for the volume tools; this module borrows its cropping and nothing else.

The stack is zero but for two blocks of synthetic tubes (synth.synth, one seed each, 96 x 64 in x / y): the near one in the first
planes at bigvol's even origin, the far one over the planes [l - 40, l) in the corner of the three far faces.  On the large stack the
far block therefore holds the last voxel, crosses plane 512 = l - TAIL -- voxel index 2^31 and, hess_chunk_planes() giving chunks of
32 planes at 2048 x 2048, the face between Hessian chunks 15 and 16 -- and ends in the ragged last chunk of 24 planes.

Expected values come from the oracle alone.  Frangi: on a crop around each block, one halo of background wide (HALO: what the Gaussian
of the largest scale plus the radius-2 Hessian stencil reads) or cut at the stack's own face where that comes first; beyond a halo of
a block every smoothed value and so every response is exactly 0, and the clamped reads of a crop's cut side repeat a plane of zeros,
which is what lies there.  Seeds: MaximumFinder is per layer, its keys order by (value, y, x) and a layer outside the crops is its
minimum, so the crops' seeds, translated, are the stack's in z-major order.  Scores, traces and replay depend on absolute coordinates
(the rounding of every sample position): the oracle runs them on the whole stack on the host, indexing in 64 bits.
tests/test_bigvol_host.py holds these claims on the small stack and the conditions the GPU tests rely on at both."""
import math
import os
import re
import numpy as np
import bigvol
import orc
import synth

SHAPE = (536, 2048, 2048)  # (l, h, w)
SMALL = (72, 96, 160)
NEAR, FAR = (16, 64, 96), (40, 64, 96)  # the extents of the two blocks
BLOCK_SEEDS = (3, 7)  # synth's seed of the near and of the far block
TAIL = 24  # the far block's planes from plane l - TAIL on: from plane 512 = voxel index 2^31 on the large stack
SIGMAS, ZD = (2.0, 3.0), 2.0
PARAMS = dict(sigmas=list(SIGMAS), somaradius=0, step=2, kappa=3.0, zdist=ZD, np_=50, ni=20, tolerance=5, znccth=0.3, nodepervol=4, vol=1)
HX, HZ = math.ceil(3 * max(SIGMAS)) + 2, math.ceil(3 * max(SIGMAS) / ZD) + 2
HALO = (HZ, HX, HX)
NSEL = 6  # far seeds traced
INDEX = np.int64  # the type of every absolute voxel index formed here
TWO31 = 2**31


def ht_z():
    """the planes of one march of hessian_tile (pnr_amd/csrc/frangi.hip)"""
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pnr_amd", "csrc", "frangi.hip")).read()
    return int(re.search(r"#define PNR_HT_Z (\d+)", txt).group(1))


def chunk_planes(shape, hess_chunk=0):
    """hess_chunk_planes() of frangi.hip"""
    l, h, w = shape
    z = ht_z()
    cz = (1 << 27) // (w * h) // z * z
    if hess_chunk > 0:
        cz = min(cz, max(z, hess_chunk // z * z))
    return min(max(cz, z), -(-l // z) * z)


def index_of(x, y, z, shape):
    _, h, w = shape
    return INDEX(x) + INDEX(w) * (INDEX(y) + INDEX(h) * INDEX(z))


def origins(shape):
    """(z0, y0, x0) of the near and of the far block"""
    l, h, w = shape
    return bigvol.origins(shape)[0], (l - FAR[0], h - FAR[1], w - FAR[2])


_blocks = {}


def blocks(shape):
    """[(origin, block)]: the same two blocks at either shape"""
    if not _blocks:
        for k, (n, seed) in enumerate(zip((NEAR, FAR), BLOCK_SEEDS)):
            _blocks[k] = synth.synth(n[2], n[1], n[0], seed=seed, zdist=ZD)
            _blocks[k].setflags(write=False)
    return [(o, _blocks[k]) for k, o in enumerate(origins(shape))]


def check_placement(blk, shape):
    """the placement rules of the tracing path -> the absolute index of the far block's first voxel in plane l - TAIL + 1"""
    l, h, w = shape
    (on, near), (of, far) = blk
    plane = l - TAIL
    assert all(v % 2 == 0 for v in on) and on == bigvol.origins(shape)[0], "the near block lies at the even origin of bigvol"
    assert of[0] == l - 40 and far.shape[0] == 40, "the far block spans the planes [l - 40, l)"
    assert tuple(o + n for o, n in zip(of, far.shape)) == (l, h, w), "the far block touches the three far faces"
    assert far[-1, -1, -1] == whole_at(blk, shape, w - 1, h - 1, l - 1) and int(index_of(w - 1, h - 1, l - 1, shape)) == l * h * w - 1, "it holds the last voxel"
    assert of[0] < plane < l, "it crosses plane l - TAIL"
    assert on[0] + near.shape[0] + HZ <= of[0] - HZ, "the crops share no plane"
    if shape == SHAPE:
        cz = chunk_planes(shape)
        assert int(index_of(0, 0, plane, shape)) == TWO31, "plane 512 is voxel index 2^31"
        assert cz == ht_z() == 32 and plane % cz == 0 and plane // cz == 16, "and the face between Hessian chunks 15 and 16"
        assert l % cz == TAIL and l - l // cz * cz == 24, "the far block ends in the ragged last chunk of 24 planes"
    first = index_of(of[2], of[1], plane + 1, shape)
    assert first.dtype == INDEX
    if shape == SHAPE:
        assert int(first) > TWO31 and int(first) == TWO31 + h * w + of[1] * w + of[2], "the far block's first voxel at z = 513 is above 2^31"
    return int(first)


def whole_at(blk, shape, x, y, z):
    return int(bigvol.stack_crop(blk, shape, (z, y, x), (z + 1, y + 1, x + 1))[0][0, 0, 0])


def crops(blk, shape):
    """a crop around every block: the block and one halo of background, or up to the stack's face -> [(array, origin)]"""
    return [bigvol.stack_crop(blk, shape, [p - m for p, m in zip(o, HALO)], [p + n + m for p, n, m in zip(o, B.shape, HALO)]) for o, B in blk]


def region(o, a):
    return tuple(slice(p, p + n) for p, n in zip(o, a.shape))


def outside(shape, parts):
    """bool [l][h][w]: the voxels outside every crop (`parts`: (origin, array) pairs)"""
    m = np.ones(shape, bool)
    for o, a in parts:
        m[region(o, a)] = False
    return m


def frangi_want(L, shape):
    """the oracle's Frangi on the crops with the extremes over both -> dict(jmin, jmax, crops=[dict(o, img, J, J8, Vx, Vy, Vz)])"""
    out = []
    for C, o in crops(blocks(shape), shape):
        J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(L, C, list(SIGMAS), ZD)
        out.append(dict(o=o, img=C, J=J, Vx=Vx, Vy=Vy, Vz=Vz, ext=(jmin, jmax)))
    jmin, jmax = min(c["ext"][0] for c in out), max(c["ext"][1] for c in out)
    for c in out:
        c["J8"] = orc.j8(L, c["J"], jmin, jmax)
    return dict(jmin=jmin, jmax=jmax, crops=out)


def frangi_whole(L, shape):
    """the oracle's Frangi on the whole stack (the small shape) -> dict(J, J8, Vx, Vy, Vz, jmin, jmax)"""
    img = host_stack(shape)
    J, jmin, jmax, Vx, Vy, Vz = orc.frangi3d(L, img, list(SIGMAS), ZD)
    return dict(J=J, J8=orc.j8(L, J, jmin, jmax), Vx=Vx, Vy=Vy, Vz=Vz, jmin=jmin, jmax=jmax)


def host_stack(shape):
    """the whole stack on the host (the large one: 2.2 GB, all but the blocks' pages untouched)"""
    return bigvol.whole(blocks(shape), shape)


def seeds_want(L, fw):
    """the oracle's seeds of the crops, translated: (n, 6) float32 x, y, z, vx, vy, vz in the stack's z-major order"""
    out = []
    for c in fw["crops"]:
        s = orc.extract_seeds(L, PARAMS["tolerance"], c["J8"], c["Vx"], c["Vy"], c["Vz"])[:, :6]
        s[:, :3] += np.array(c["o"][::-1], np.float32)  # (whole numbers below 2^24: exact)
        out.append(s)
    assert out[0][:, 2].max() < out[1][:, 2].min()
    return np.concatenate(out)


def layer_want(L, fw, shape, z):
    """orc.extract_seeds on layer z of the stack as a one-slice stack, built from the crops' J8 and direction bytes -> (n, 6)"""
    _, h, w = shape
    lay = {k: np.zeros((1, h, w), np.uint8) for k in ("J8", "Vx", "Vy", "Vz")}
    for c in fw["crops"]:
        (z0, y0, x0), (n, ch, cw) = c["o"], c["J8"].shape
        if z0 <= z < z0 + n:
            for k in lay:
                lay[k][0, y0:y0 + ch, x0:x0 + cw] = c[k][z - z0]
    s = orc.extract_seeds(L, PARAMS["tolerance"], *[lay[k] for k in ("J8", "Vx", "Vy", "Vz")])[:, :6]
    s[:, 2] = z
    return s


def compared_layers(shape):
    """the four layers whose seeds are compared whole: one of the near block, plane l - TAIL itself, the two above it (the far layers
    that hold more than 5 seeds)"""
    l = shape[0]
    return [origins(shape)[0][0] + NEAR[0] // 2, l - TAIL, l - TAIL + 1, l - TAIL + 2]


def tracker(L):
    p = PARAMS
    return orc.Tracker(L, p["sigmas"], p["step"], p["np_"], p["ni"], p["kappa"], p["znccth"], zdist=p["zdist"], nodespervol=p["nodepervol"])


def scores_want(T, img, seeds):
    """-> (corr of every seed, the kept seeds sorted as pnr_score_filter_sort_seeds sorts them (n, 6), their corr)"""
    corr = T.zncc(img, seeds)[0]
    keep = corr >= np.float32(PARAMS["znccth"])
    order = np.argsort(-corr[keep], kind="stable")
    return corr, seeds[keep][order], corr[keep][order]


def select(sorted6, shape):
    """rows of the sorted seeds that are traced: of those at z >= l - TAIL + 4 (plane 516) the first NSEL - 2, which stay up there, and
    the first two of the planes 516 .. 519 that are not among them, from where 20 iterations reach below plane 512; last the best
    seed of the near block"""
    l = shape[0]
    far = np.flatnonzero(sorted6[:, 2] >= l - TAIL + 4)
    best = far[:NSEL - 2]
    low = np.array([k for k in far if sorted6[k, 2] < l - TAIL + 8 and k not in best][:2], np.int64)
    near = np.flatnonzero(sorted6[:, 2] < origins(shape)[0][0] + NEAR[0])[:1]
    return np.concatenate([best, low, near])


def traces_want(T, img, sel6):
    """Tracker.trace of every selected seed in both directions -> [(T, stop, xc)] in trace_batch's order"""
    out = []
    for q0 in sel6:
        for sgn in (1, -1):
            q = q0.astype(np.float32).copy()
            q[3:] *= sgn
            Tn, st, xc, *_ = T.trace(img, q)
            out.append((Tn, st, xc))
    return out


def centroid_index(xc, rows, shape):
    """the voxel index of the first `rows` centroids of a trace, in INDEX"""
    l, h, w = shape
    c = np.rint(xc[:rows, :3].astype(np.float64))
    x, y, z = (np.clip(c[:, k], 0, n - 1).astype(INDEX) for k, n in enumerate((w, h, l)))
    return x + INDEX(w) * (y + INDEX(h) * z)


def conditions(shape, fw, seeds, sorted6, sel, traces):
    """the counts the GPU tests rely on; the asserts that hold them are in test_bigvol_host.py and repeated by the GPU tests"""
    l, h, w = shape
    ni = PARAMS["ni"]
    sign = index_of(0, 0, l - TAIL, shape)
    far_sel = sel[:-1]
    above, crossing = 0, 0
    for k in range(len(far_sel)):
        for d in range(2):
            Tn, st, xc = traces[2 * k + d]
            rows = min(Tn + 1, ni)
            idx = centroid_index(xc, rows, shape)
            above += bool(rows >= 8 and (idx > sign).all())
            crossing += bool((xc[:rows, 2] < l - TAIL).any())
    return dict(layer_seeds={z: int((seeds[:, 2] == z).sum()) for z in compared_layers(shape)}, far_kept=int((sorted6[:, 2] >= l - TAIL + 4).sum()),
                traces_above=above, traces_crossing=crossing, seeds=len(seeds), kept=len(sorted6))


_ref, _fref = {}, {}


def frangi_reference(L, shape):
    """frangi_want, computed once"""
    if shape not in _fref:
        _fref[shape] = frangi_want(L, shape)
    return _fref[shape]


def reference(L, shape):
    """everything the oracle says about the stack of `shape`, computed once and never changed: frangi (frangi_want), seeds, img (the
    host stack), tracker, corr / sorted6 / corr6 (scores_want), sel (select), traces (traces_want), counts (conditions)"""
    if shape not in _ref:
        r = dict(frangi=frangi_reference(L, shape), img=host_stack(shape), tracker=tracker(L))
        r["seeds"] = seeds_want(L, r["frangi"])
        r["corr"], r["sorted6"], r["corr6"] = scores_want(r["tracker"], r["img"], r["seeds"])
        r["sel"] = select(r["sorted6"], shape)
        r["traces"] = traces_want(r["tracker"], r["img"], r["sorted6"][r["sel"]])
        r["counts"] = conditions(shape, r["frangi"], r["seeds"], r["sorted6"], r["sel"], r["traces"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ref[shape] = r
    return _ref[shape]


def open_stack(shape, params=None):
    """the zero stack with the blocks on the device, borrowed by a new context with make_params(**params) -> (tensor, context)"""
    import torch
    import pnr_amd
    t = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    for (z0, y0, x0), B in blocks(shape):
        t[z0:z0 + B.shape[0], y0:y0 + B.shape[1], x0:x0 + B.shape[2]] = torch.from_numpy(np.array(B)).cuda()  # (a copy: the blocks are read-only)
    torch.cuda.synchronize()
    c = pnr_amd.Context(pnr_amd.make_params(**(params or PARAMS)), 0)
    c.set_volume_device(t.data_ptr(), shape, keepalive=t)
    return t, c


def boxes(c, fw, **what):
    return [c.get_frangi_box(k["o"], [p + n for p, n in zip(k["o"], k["J8"].shape)], **what) for k in fw["crops"]]


def check_frangi(c, fw, whole_j8=True):
    """the context's Frangi outputs against the oracle's: J8 over the whole stack (equal on the crops, nothing outside them), then J
    (rtol 2e-6: the fp64 exp of ocml and of glibc, as test_gpu_fullsize.py), J8 and the direction bytes of the crops"""
    if whole_j8:
        J8 = c.get_frangi(J=False, J8=True, V=False)["J8"]
        inside = 0
        for k in fw["crops"]:
            assert np.array_equal(J8[region(k["o"], k["J8"])], k["J8"]), ("J8 of the run as it stands", k["o"])
            inside += int(np.count_nonzero(k["J8"]))
        assert inside > 10000 and int(np.count_nonzero(J8)) == inside, "J8 outside the crops is 0"
        del J8
    for k, g in zip(fw["crops"], boxes(c, fw)):
        assert np.allclose(g["J"], k["J"], rtol=2e-6, atol=0) and (g["J"] > 0).sum() > 1000, ("J", k["o"])
        for v in ("J8", "Vx", "Vy", "Vz"):
            assert np.array_equal(g[v], k[v]), (v, k["o"])
