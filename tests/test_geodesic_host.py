"""CPU: the numpy restatement of the geodesic rule (geodesic_ref.py) -- the literal sweeps against the heap of (cost, label) tuples, bit for
bit, and against scipy.sparse.csgraph.dijkstra for D where scipy is present --, hand-made stacks with known answers, the path rule, the
ctypes mirrors of the structs against the header text, and the usage errors of advantra_cli --geodesic (caught before a device is
opened)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from pnr_amd import lib
import geodesic_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
SHAPES = [(3, 7, 9), (1, 12, 13), (2, 2, 2), (4, 5, 6), (3, 17, 40)]
ZDS = (1.0, 2.0, 3.3)
DMAXS = (500, 5000, ref.DMAX)


def _case(shape, density, seed):
    rng = np.random.default_rng(seed)
    V = np.where(rng.random(shape) < density, rng.integers(128, 256, shape), rng.integers(0, 128, shape)).astype(np.uint8)
    l, h, w = shape
    n = 5
    xyz = np.stack([rng.uniform(-1, e, n) for e in (w, h, l)], 1).astype(np.float32)
    xyz = np.concatenate([xyz, xyz[:1], [[np.nan, 0, 0]]]).astype(np.float32)  # two labels on one voxel, a source that is not finite
    labels = np.array([7, 3, 3, 11, 0, 2, 9], np.int32)
    return V, xyz, labels


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sweeps_equal_the_heap(shape):
    for di, density in enumerate((0.3, 0.6, 1.0)):
        V, xyz, labels = _case(shape, density, 10 * SHAPES.index(shape) + di)
        thr = 128 if density < 1.0 else 0
        for zd in ZDS:
            for dmax in DMAXS:
                src, kept, dropped = ref.sources(V, thr, xyz, labels)
                assert kept + dropped == len(xyz) and dropped >= 1
                K, t, n = ref.sweeps(V, src, thr, zd, dmax)
                K2, _, n2 = ref.sweeps(V, src, thr, zd, dmax, inplace=True)
                K3, _ = ref.dijkstra(V, src, thr, zd, dmax)
                assert t == thr and K.dtype == np.uint64 and K.tobytes() == K2.tobytes() == K3.tobytes(), (shape, density, zd, dmax)
                assert n2 <= n
                D, L = ref.split(K)
                reached = K != ref.NONE
                assert not reached[V < thr].any() and (D[reached] <= dmax).all() and (D[~reached] == ref.UNREACHED).all() and (L[~reached] == -1).all()
                assert set(np.unique(L[reached])) <= set(src.values())
                if len(src) and dmax == ref.DMAX and density == 1.0:
                    assert reached.all()
                # the path rule finds a predecessor at every reached voxel with D > 0, and D strictly decreases along it
                ln, tab = ref.lengths(zd), ref.cost_table()
                for g in np.flatnonzero(reached.ravel() & (D.ravel() > 0))[:200]:
                    q = ref.pred(V, K, t, ln, tab, int(g))
                    assert q is not None and D.ravel()[q] < D.ravel()[g] and L.ravel()[q] == L.ravel()[g]


@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_reference_against_scipy(shape):
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    l, h, w = shape
    for zd in ZDS:
        V, xyz, labels = _case(shape, 0.6, 5)
        src, _, _ = ref.sources(V, 128, xyz, labels)
        K, t, _ = ref.sweeps(V, src, 128, zd)
        ln, tab = ref.lengths(zd), ref.cost_table()
        rows, cols, wts = [], [], []
        for g in range(V.size):
            x, y, z = g % w, g // w % h, g // (w * h)
            if V.ravel()[g] < t:
                continue
            for (dx, dy, dz), le in zip(ref.OFFSETS, ln):
                qx, qy, qz = x + dx, y + dy, z + dz
                if 0 <= qx < w and 0 <= qy < h and 0 <= qz < l and V[qz, qy, qx] >= t:
                    rows.append(g), cols.append(qx + w * (qy + h * qz)), wts.append(le * (int(tab[V.ravel()[g]]) + int(tab[V[qz, qy, qx]])))
        G = sparse.csr_matrix((np.array(wts, np.float64), (rows, cols)), shape=(V.size, V.size))
        theirs = csgraph.dijkstra(G, indices=sorted(src), min_only=True)
        D, _ = ref.split(K)
        mine = np.where(D.ravel() == ref.UNREACHED, np.inf, D.ravel().astype(np.float64))
        assert np.array_equal(mine, theirs), (shape, zd)


def test_lengths_and_the_offset_order():
    assert len(ref.OFFSETS) == 26 and ref.OFFSETS[0] == (-1, -1, -1) and ref.OFFSETS[1] == (0, -1, -1) and ref.OFFSETS[12] == (-1, 0, 0) and ref.OFFSETS[13] == (1, 0, 0)
    ln = ref.lengths(1.0)
    assert sorted(set(ln)) == [32, 45, 55] and ln[12] == ln[13] == 32
    for zd in ZDS:
        ln = ref.lengths(zd)
        assert all(ln[i] == ln[25 - i] for i in range(26))  # symmetric under o -> -o
    assert ref.lengths(2.0)[4] == 64 and ref.lengths(3.3)[4] == 106  # (0, 0, -1): 32 zd


def test_hand_made_stacks():
    # a straight bright line: D = 64 c steps (c = 256 - 255 = 1), the path runs along it
    V = np.zeros((3, 5, 20), np.uint8)
    V[1, 2, :] = 255
    src, kept, dropped = ref.sources(V, 0, [[0, 2, 1]])
    K, t, _ = ref.sweeps(V, src)
    D, L = ref.split(K)
    assert (kept, dropped) == (1, 0) and np.array_equal(D[1, 2], 64 * np.arange(20)) and (L == 0).all() and (K != ref.NONE).all()
    assert D[1, 1, 0] == 32 * (1 + 256)  # one step off the line: len 32, costs 1 and 256
    lens, walks = ref.paths(V, K, [[19, 2, 1], [np.nan, 0, 0]], 64)
    line = 20 * (2 + 5 * 1)
    assert lens.tolist() == [20, 0] and walks[0].tolist() == [line + x for x in range(19, -1, -1)] and len(walks[1]) == 0
    lens, walks = ref.paths(V, K, [[19, 2, 1], [3, 2, 1]], 5)
    assert lens.tolist() == [-5, 4] and walks[0].tolist() == [line + x for x in range(19, 14, -1)] and walks[1].tolist() == [line + 3, line + 2, line + 1, line]
    got = ref.info(V, K, t, kept, dropped)
    far = int(np.flatnonzero(D.ravel() == D.max())[0])
    assert got == dict(n_vox=300, n_pass=300, n_reached=300, n_src=1, n_src_dropped=0, first_max=far, d_max=int(D.max()), thr_used=0, max_at=(far % 20, far // 20 % 5, far // 100))
    # a wall with one hole: the path goes through the hole, and without the hole the far side is unreached
    W = np.full((1, 9, 11), 200, np.uint8)
    W[0, :, 5] = 0
    W[0, 7, 5] = 200
    src, _, _ = ref.sources(W, 100, [[1, 1, 0]], [4])
    K, t, _ = ref.sweeps(W, src, 100)
    lens, walks = ref.paths(W, K, [[9, 1, 0]], 64, thr=100)
    assert lens[0] > 0 and 5 + 11 * 7 in walks[0].tolist() and walks[0][-1] == 1 + 11 * 1 and (ref.split(K)[1][W >= 100] == 4).all()
    W[0, 7, 5] = 0
    K, t, _ = ref.sweeps(W, src, 100)
    reached = K != ref.NONE
    assert reached[0, :, :5].all() and not reached[0, :, 5:].any()
    got = ref.info(W, K, t, 1, 0)
    assert (got["n_pass"], got["n_reached"]) == (90, 45)
    # nothing reached; a source on an impassable voxel is dropped
    src, kept, dropped = ref.sources(W, 100, [[5, 3, 0], [np.inf, 0, 0]])
    K, t, n = ref.sweeps(W, src, 100)
    assert (kept, dropped, n) == (0, 2, 0) and (K == ref.NONE).all()
    assert ref.info(W, K, t, kept, dropped) == dict(n_vox=99, n_pass=90, n_reached=0, n_src=0, n_src_dropped=2, first_max=-1, d_max=0, thr_used=100, max_at=None)
    assert ref.threshold(W, -1) == int(W.sum(dtype=np.int64)) // W.size and ref.threshold(np.zeros((2, 2, 2), np.uint8), -1) == 1


def test_ties_take_the_smallest_label():
    """a constant stack, mirror-symmetric source columns: on the mid-plane both sources attain the cost, and the smaller label wins"""
    for shape in ((3, 9, 33), (1, 8, 65)):
        l, h, w = shape
        V = np.full(shape, 100, np.uint8)
        pts = [[3, y, z] for z in range(l) for y in range(h)] + [[w - 4, y, z] for z in range(l) for y in range(h)]
        labels = [5] * (h * l) + [2] * (h * l)
        src, _, _ = ref.sources(V, 0, pts, labels)
        K, _, _ = ref.sweeps(V, src, zd=2.0)
        D, L = ref.split(K)
        assert (L[:, :, w // 2] == 2).all() and (L[:, :, :w // 2] == 5).all() and (L[:, :, w // 2 + 1:] == 2).all()
        assert np.array_equal(D, D[:, :, ::-1])


def test_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "const uint16_t *": C.POINTER(C.c_uint16)}

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        out = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.match(r"(const uint16_t \*|\w+)\s*(.*)", decl)
            out += [(n.strip(), ctype[m.group(1)]) for n in m.group(2).split(",")]
        return out

    assert fields("pnr_geo_opts") == list(lib.GeoOpts._fields_)
    assert fields("pnr_geo_info") == list(lib.GeoInfo._fields_)
    assert C.sizeof(lib.GeoOpts) == 16 and C.sizeof(lib.GeoInfo) == 64
    assert "pnr_geodesic_distance" in lib.PRODUCT_EXPORTS and re.search(r"^int pnr_geodesic_distance\(", hdr, re.M)
    assert int(re.search(r"#define PNR_GEO_MAX_PATH \(1 << (\d+)\)", hdr).group(1)) == 16 and lib.PNR_GEO_MAX_PATH == 1 << 16
    assert hasattr(lib.load(), "pnr_geodesic_distance")


def test_tile_constants_are_where_the_tests_read_them():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "geodesic.h")).read()
    got = dict(re.findall(r"constexpr int (GEO_TX|GEO_TY|GEO_TZ) = (\d+);", txt))
    assert sorted(got) == ["GEO_TX", "GEO_TY", "GEO_TZ"] and all(int(v) >= 2 for v in got.values())


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


G = ("--geodesic", "-i", "x.raw", "--from", "t.swc")


@pytest.mark.parametrize("args,msg", [
    (("--geodesic", "--from", "t.swc"), "--geodesic needs -i"), (("--geodesic", "-i", "x.raw"), "--geodesic needs --from"),
    ((*G, "--geo-max", "0"), "--geo-max D"), ((*G, "--geo-max", "2147483648"), "--geo-max D"), ((*G, "--geo-max", "x"), "--geo-max D"), ((*G, "--geo-max"), "--geo-max D"),
    (("--geodesic", "-i", "x.raw", "--from"), "--from tree.swc"), ((*G, "--to"), "--to other.swc"), ((*G, "--paths"), "--paths OUT.swc"), ((*G, "--geo-out"), "--geo-out PREFIX"),
    ((*G, "--to", "o.swc"), "go together"), ((*G, "--per-node", "n.csv"), "go together"), ((*G, "--paths", "p.swc"), "--paths OUT.swc needs --to"),
    ((*G, "--threshold", "256"), "--threshold T"), ((*G, "--zscale", "0.5"), "--zscale Z"),
    (("--from", "t.swc", "-i", "x.raw"), "need --geodesic"), (("--to", "t.swc", "-i", "x.raw"), "need --geodesic"), (("--paths", "t.swc", "-i", "x.raw"), "need --geodesic"),
    (("--geo-max", "3", "-i", "x.raw"), "need --geodesic"), (("--geo-out", "p", "-i", "x.raw"), "need --geodesic"),
    ((*G, "--edt"), "--geodesic: not with"), ((*G, "--edt-max", "3"), "need --edt"), ((*G, "--components"), "--geodesic: not with"),
    ((*G, "--min-size", "3"), "need --components"), ((*G, "--render-swc", "t.swc"), "--geodesic: not with"), ((*G, "--distance", "a.swc", "b.swc"), "--geodesic: not with"),
    ((*G, "--join-swc", "a.swc", "b.swc"), "--geodesic: not with"), ((*G, "--info"), "--geodesic: not with"), ((*G, "--despeckle", "3"), "--geodesic: not with"),
    ((*G, "--measure-radius"), "--geodesic: not with"), ((*G, "--join", "3"), "--geodesic: not with"),
    (("--geodesic", "--from", "t.swc", "-f", "advantra_func", "-i", "x.raw", "-p", "2,3", "0", "5", "0.3", "3", "2", "40", "50", "2", "4", "5"), "--geodesic: not with")])
def test_cli_usage_errors(args, msg):
    r = _cli(*args, "-g", "99") if "-p" not in args else _cli("-g", "99", *args)  # (a device that does not exist: the error comes first)
    assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)


def test_cli_help_lists_the_flags():
    r = _cli("--help")
    assert r.returncode == 0
    for flag in ("--geodesic -i stack --from tree.swc", "--threshold T", "--geo-max D", "--zscale Z", "--to other.swc --per-node FILE.csv", "--paths OUT.swc", "--geo-out PREFIX"):
        assert flag in r.stdout, flag
