"""The tree distance on the GPU (pnr_point_segment_distance, pnr_tree_distance, Context.tree_distance, advantra_cli --distance): closed
forms, the tie rule, a fuzz against the rule of include/pnr_hip.h restated in numpy (distance_ref.py) with automatic and with forced
slices and launches, trees, the pipeline, the CLI and the contract of the call.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import distance_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)  # no volume: the distance needs none
    yield c
    c.close()


def forced(c, on):
    c.set_option("dist_split", 64 if on else 0)
    c.set_option("dist_pairs_per_launch", 100000 if on else 0)


# ---- closed forms: do not depend on the restatement ----
def test_closed_forms(ctx):
    a, b = np.array([[0, 0, 0]], F), np.array([[10, 0, 0]], F)
    d, j = ctx.point_segment_distance([[3, 4, 0], [-3, 0, 4], [13, 4, 0], [5, 0, 0], [0, 0, 0], [10, 0, 0]], a, b)
    print("3-4-5:", d.tolist())
    assert d.dtype == F and j.dtype == np.int32
    assert np.array_equal(d, [4, 5, 5, 0, 0, 0]) and np.array_equal(j, np.zeros(6))  # beside, before, behind, on it, its two ends
    d, _ = ctx.point_segment_distance([[3, 4, 0], [2, 2, 14], [2, 2, 2]], [[2, 2, 2]], [[2, 2, 2]])  # a degenerate segment: point to point
    assert np.array_equal(d, [np.sqrt(F(1 + 4 + 4)), 12, 0])


def test_tie_rule(ctx):
    """two identical segments at indices 4 and 5 (and again at 300 and 301, in another slice when the split is forced): j = 4"""
    rng = np.random.default_rng(2)
    a = (rng.random((302, 3)) * 64).astype(F)
    b = (rng.random((302, 3)) * 64).astype(F)
    a[:, 2] += 100  # ... all far from the points, but for
    b[:, 2] += 100
    a[4] = a[5] = a[300] = a[301] = [1, 1, 1]
    b[4] = b[5] = b[300] = b[301] = [9, 1, 1]
    pts = np.array([[5, 3, 1], [0, 1, 1], [9.5, 1, 1], [4, 1, 1]], F)
    for on in (False, True):
        forced(ctx, on)
        d, j = ctx.point_segment_distance(pts, a, b)
        assert np.array_equal(j, [4, 4, 4, 4]) and np.array_equal(d, [2, 1, 0.5, 0]), (on, d, j)
    forced(ctx, False)


# ---- fuzz against the restatement ----
def fuzz_case(n, m):
    """coordinates uniform in [0, 64); every fifth segment has length exactly 0, every seventh repeats its predecessor, the others are
    at least 2^-10 long"""
    rng = np.random.default_rng(1000 * n + m)
    pts = (rng.random((n, 3)) * 64).astype(F)
    a = (rng.random((m, 3)) * 64).astype(F)
    b = (rng.random((m, 3)) * 64).astype(F)
    short = np.linalg.norm(b.astype(np.float64) - a, axis=1) < 2.0 ** -10
    b[short] = np.clip(a[short] + F(1), 0, 63)
    b[::5] = a[::5]
    a[7::7], b[7::7] = a[6:-1:7], b[6:-1:7]
    pts[:min(n, m):3] = a[:min(n, m):3]  # points that sit on a segment's start
    lengths = np.linalg.norm(b.astype(np.float64) - a, axis=1)
    assert ((lengths == 0) | (lengths >= 2.0 ** -10)).all()
    assert pts.min() >= 0 and max(pts.max(), a.max(), b.max()) < 64
    return pts, a, b


FUZZ_REF = {}


@pytest.mark.parametrize("n,m", [(1, 1), (63, 1), (65, 257), (1000, 777), (4099, 2053),
                                 (1000, 100)])  # forced: two row launches of 768 and 232 points, each over all segments (tests/test_pair_tiles.py)
def test_fuzz_against_the_restatement(ctx, n, m):
    pts, a, b = fuzz_case(n, m)
    if (n, m) not in FUZZ_REF:
        FUZZ_REF[(n, m)] = distance_ref.point_segment(pts, a, b)
    want_d, want_j = FUZZ_REF[(n, m)]
    forced(ctx, False)
    d0, j0 = ctx.point_segment_distance(pts, a, b)
    forced(ctx, True)
    d1, j1 = ctx.point_segment_distance(pts, a, b)
    forced(ctx, False)
    print(f"n={n} m={m}: d mismatches auto {int((d0 != want_d).sum())} forced {int((d1 != want_d).sum())}, j mismatches auto {int((j0 != want_j).sum())} "
          f"forced {int((j1 != want_j).sum())}, zeros {int((want_d == 0).sum())}")
    assert np.array_equal(d0, d1) and np.array_equal(j0, j1)
    assert np.array_equal(d0, want_d), np.flatnonzero(d0 != want_d)[:5]
    assert np.array_equal(j0, want_j), np.flatnonzero(j0 != want_j)[:5]


# ---- trees ----
def same(got, want):
    for k in ("ab", "ba"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("sd", "ssd", "pct", "hausdorff"):
        assert got[k] == want[k], (k, got[k], want[k])


def check_tree_pair(ctx, xa, pa, xb, pb, **kw):
    got, (da, oa), (db, ob) = ctx.tree_distance(xa, pa, xb, pb, per_point=True, **kw)
    want, (wda, woa), (wdb, wob) = distance_ref.tree_distance(xa, pa, xb, pb, **kw)
    print(kw, json.dumps(got))
    same(got, want)
    assert np.array_equal(da, wda) and np.array_equal(db, wdb) and np.array_equal(oa, woa) and np.array_equal(ob, wob)
    same(ctx.tree_distance(xa, pa, xb, pb, **kw), want)
    return got


def test_tree_against_itself_and_shifted_chain(ctx):
    """(A, A): every metric is 0 -- exactly so on the nodes (step = 0); with the default step the interior points are f32 roundings of
    f64 positions and lie a few ulp off their segment: pct and ssd stay exactly 0, the mean is the restatement's (of the order 1e-7)"""
    rng = np.random.default_rng(4)
    xyz, parent = distance_ref.random_forest(rng, 200)
    # the nodes only: every point is the start of a segment of the other tree, so every distance is exactly 0
    r = ctx.tree_distance(xyz, parent, xyz, parent, step=0)
    assert r["ab"]["n"] == r["ba"]["n"] == 200
    for side in (r["ab"], r["ba"]):
        assert side["n_big"] == 0 and side["mean"] == 0 and side["ssd"] == 0 and side["pct"] == 0 and side["max"] == 0
    assert r["sd"] == r["ssd"] == r["pct"] == r["hausdorff"] == 0
    # resampled: an interior point is rounded to f32 from f64, so it lies within a few ulp of its segment, not on it: nothing is
    # "big", ssd and pct are exactly 0, and the few-ulp mean is the restatement's
    r = check_tree_pair(ctx, xyz, parent, xyz, parent)
    assert r["ab"]["n"] > 200 and r["ab"] == r["ba"] and r["ab"]["n_big"] == 0 and r["ssd"] == 0 and r["pct"] == 0
    # a straight chain along x against its copy shifted by (0, 0, 3): every distance is exactly 3; with zscale = 2 exactly 6
    chain = np.stack([np.arange(40) * 1.5, np.full(40, 7.0), np.full(40, 2.0)], 1).astype(F)
    par = np.arange(-1, 39)
    for zscale, want in ((1, 3.0), (2, 6.0)):
        r, (da, _), (db, _) = ctx.tree_distance(chain, par, chain + F([0, 0, 3]), par, zscale=zscale, per_point=True)
        assert (da == want).all() and (db == want).all() and len(da) == len(db) == 40 + 39
        assert r["sd"] == r["ssd"] == r["hausdorff"] == want and r["pct"] == 1 and r["ab"]["n_big"] == len(da)
    r = ctx.tree_distance(chain, par, chain + F([0, 0, 3]), par, thr=3.5)
    assert r["sd"] == 3 and r["ssd"] == 0 and r["pct"] == 0  # nothing is "big" at thr 3.5: ssd = 0 by definition


def test_random_forests_against_the_restatement(ctx):
    rng = np.random.default_rng(5)
    xa, pa = distance_ref.random_forest(rng, 300, roots=3)
    xb = (xa + rng.normal(0, 1.2, xa.shape)).astype(F)  # a jittered copy: a mix of near and far points
    xb[250:] += F(9)
    check_tree_pair(ctx, xa, pa, xb, pa)
    check_tree_pair(ctx, xa, pa, xb, pa, zscale=2.5, step=0.5, thr=1.25)
    forced(ctx, True)
    check_tree_pair(ctx, xa, pa, xb, pa, step=3.7)
    forced(ctx, False)
    check_tree_pair(ctx, xa, pa, xb, pa, step=0)
    # asymmetric sizes (37 nodes against 1201, isolated nodes among the 37): the two directions differ
    xs, ps = distance_ref.random_forest(rng, 37, roots=9, step=0.5)
    xl, pl = distance_ref.random_forest(rng, 1201, roots=2)
    r = check_tree_pair(ctx, xs, ps, xl, pl)
    assert r["ab"]["n"] != r["ba"]["n"] and r["ab"]["mean"] != r["ba"]["mean"]
    r2 = check_tree_pair(ctx, xl, pl, xs, ps)
    assert r2["ab"] == r["ba"] and r2["ba"] == r["ab"] and r2["sd"] == r["sd"]


def _trace(img, seed):
    p = pnr_amd.make_params(sigmas=(2, 3), np_=32, ni=12, zdist=2, rng_seed=seed)
    c = pnr_amd.Context(p, 0)
    res = pnr_amd.advantra.run_pipeline(c, img)
    tree, parent = res["tree"], res["parent"]
    xyz = np.stack([tree["x"], tree["y"], tree["z"]], 1)[1:]  # without the dummy node
    par = np.where(parent[1:] > 0, parent[1:] - 1, -1).astype(np.int32)
    return c, xyz, par


def test_pipeline_two_rng_seeds(ctx):
    """the 48 x 40 x 24 synth stack traced with two rng_seed values and reconstructed: the distance of the two trees (in xy voxels:
    zscale = zdist) equals the restatement's; the value itself is printed, not judged.  The tracing context's state survives the call."""
    img = synth.synth(48, 40, 24, seed=1)
    c1, x1, p1 = _trace(img, 42)
    c2, x2, p2 = _trace(img, 7)
    assert len(x1) > 20 and len(x2) > 20
    seeds = c1.extract_seeds()
    got = c1.tree_distance(x1, p1, x2, p2, zscale=2.0)
    want, _, _ = distance_ref.tree_distance(x1, p1, x2, p2, zscale=2.0)
    print(f"nodes {len(x1)} / {len(x2)}: {json.dumps(got)}")
    same(got, want)
    assert np.array_equal(c1.extract_seeds(), seeds) and len(c1.score_filter_sort(seeds)) > 0  # Frangi and seed state still usable
    c1.close()
    c2.close()


# ---- the CLI ----
def write_swc(path, xyz, parent, ids):
    with open(path, "w") as f:
        f.write("# test tree\n")
        for i in np.random.default_rng(len(xyz)).permutation(len(xyz)):  # lines in any order
            f.write(f"{ids[i]} 2 {xyz[i, 0]:.3f} {xyz[i, 1]:.3f} {xyz[i, 2]:.3f} 1.000 {ids[parent[i]] if parent[i] >= 0 else -1}\n")


def test_cli_distance(ctx, tmp_path):
    rng = np.random.default_rng(6)
    xa, pa = distance_ref.random_forest(rng, 150, roots=2)
    xb, pb = distance_ref.random_forest(rng, 90, roots=3)
    fa, fb = str(tmp_path / "a.swc"), str(tmp_path / "b.swc")
    write_swc(fa, xa, pa, np.arange(len(xa)) + 1)
    write_swc(fb, xb, pb, 1000 - 3 * np.arange(len(xb)))
    (xa, pa, ia), (xb, pb, ib) = lib.read_swc(fa), lib.read_swc(fb)  # (the %.3f coordinates, in file order)
    for flags, kw in (((), {}), (("--distance-step", "0.5", "--distance-threshold", "1.5", "--zscale", "2"), dict(step=0.5, thr=1.5, zscale=2))):
        prefix = str(tmp_path / "pn")
        r = subprocess.run([CLI, "--distance", fa, fb, *flags, "--per-node", prefix], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and len(r.stdout.splitlines()) == 1, r.stderr[-1500:]
        got = json.loads(r.stdout)
        want, (da, oa), (db, ob) = distance_ref.tree_distance(xa, pa, xb, pb, **kw)
        print(r.stdout.strip())
        same(got, want)
        assert got["nodes_a"] == 150 and got["nodes_b"] == 90 and got["step"] == kw.get("step", 1) and got["thr"] == kw.get("thr", 2) and got["zscale"] == kw.get("zscale", 1)
        for tag, d, owner, ids in (("_ab.csv", da, oa, ia), ("_ba.csv", db, ob, ib)):
            rows = open(prefix + tag).read().splitlines()
            assert rows[0] == "id,d" and len(rows) == 1 + len(d)  # one row per sample point
            col = np.array([ln.split(",") for ln in rows[1:]])
            assert np.array_equal(col[:, 0].astype(np.int64), ids[owner]) and np.array_equal(col[:, 1].astype(np.float64).astype(F), d)
    same(ctx.tree_distance(xa, pa, xb, pb), distance_ref.tree_distance(xa, pa, xb, pb)[0])


# ---- the contract of the call ----
def test_argument_errors(ctx):
    L = lib.load()
    pts = np.array([[1, 2, 3], [4, 5, 6]], F)
    a, b = np.array([[0, 0, 0], [1, 1, 1]], F), np.array([[5, 0, 0], [2, 2, 2]], F)
    d = np.full(2, 77, F)
    j = np.full(2, 77, np.int32)

    def call(p=pts, n=2, sa=a, sb=b, m=2, out=d, jo=j):
        ptr = lambda v: v.ctypes.data if v is not None else None
        return L.pnr_point_segment_distance(ctx.h, ptr(p), n, ptr(sa), ptr(sb), m, ptr(out), ptr(jo))

    for v in (np.nan, np.inf, -np.inf):
        for which in range(3):
            arrs = [pts.copy(), a.copy(), b.copy()]
            arrs[which][1, 2] = v
            assert call(p=arrs[0], sa=arrs[1], sb=arrs[2]) == -1 and b"not finite" in L.pnr_last_error()
    assert call(m=0) == -1 and call(m=-1) == -1 and call(m=lib.PNR_DISTANCE_MAX_N + 1) == -1
    assert call(n=-1) == -1 and call(n=lib.PNR_DISTANCE_MAX_N + 1) == -1
    assert call(p=None) == -1 and call(sa=None) == -1 and call(sb=None) == -1 and call(out=None) == -1
    assert L.pnr_point_segment_distance(None, pts.ctypes.data, 2, a.ctypes.data, b.ctypes.data, 2, d.ctypes.data, None) == -1
    assert (d == 77).all() and (j == 77).all()
    assert call(n=0, p=None, out=None, jo=None) == 0  # n = 0 is a valid no-op
    assert call(n=0, p=None, out=None, jo=None, m=0) == -1
    assert call(jo=None) == 0 and np.array_equal(d, distance_ref.point_segment(pts, a, b)[0])  # j_out is optional
    assert call() == 0 and np.array_equal(j, distance_ref.point_segment(pts, a, b)[1])
    # pnr_tree_distance
    xyz = np.array([[0, 0, 0], [4, 0, 0], [4, 3, 0]], F)
    par = np.array([-1, 0, 1], np.int32)
    res = lib.DistanceResult()

    def tree(xa=xyz, pa=par, na=3, xb=xyz, pb=par, nb=3, opts=(1, 1, 2), r=res):
        o = lib.DistanceOpts(*opts) if opts is not None else None
        return L.pnr_tree_distance(ctx.h, xa.ctypes.data, pa.ctypes.data, na, xb.ctypes.data, pb.ctypes.data, nb, C.byref(o) if o is not None else None,
                                   C.byref(r) if r is not None else None, None, None, 0, None, None, 0)

    assert tree(opts=None) == 0 and res.sd == 0 and res.ab.n == 3 + 3 + 2  # NULL options = {1, 1, 2}
    for opts in ((0, 1, 2), (-1, 1, 2), (np.nan, 1, 2), (1, -0.5, 2), (1, np.inf, 2), (1, 1, np.nan)):
        assert tree(opts=opts) == -1, opts
    assert tree(na=0) == -1 and tree(nb=0) == -1 and b"nodes" in L.pnr_last_error()  # an empty tree on either side
    assert tree(na=lib.PNR_DISTANCE_MAX_N + 1) == -1 and tree(r=None) == -1
    bad = xyz.copy()
    bad[1, 0] = np.nan
    assert tree(xb=bad) == -1 and tree(pb=np.array([-1, 0, 3], np.int32)) == -1
    far = np.array([[0, 0, 0], [3e6, 0, 0]], F)
    assert tree(xa=far, pa=np.array([-1, 0], np.int32), na=2, opts=(1, 0.5, 2)) == -1 and b"sample points" in L.pnr_last_error()
    with pytest.raises(pnr_amd.PnrError):
        ctx.tree_distance(xyz, par, xyz, par, zscale=0)
    assert ctx.tree_distance(xyz, par, xyz + F([0, 0, 1]), par)["sd"] == 1  # ... and the context still works


def test_stream_timer_and_memory(ctx):
    """a foreign stream gives the same result; kernel_ms("distance") is (0, 0) before a call and counts its launches (the preparation,
    the launches of the pair budget, the unpacking) after it; live_bytes() is unchanged by a call"""
    import torch
    pts, a, b = fuzz_case(1000, 777)
    want = distance_ref.point_segment(pts, a, b)
    live = lib.live_bytes()
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    d, j = ctx.point_segment_distance(pts, a, b)
    ctx.set_stream(None)
    assert np.array_equal(d, want[0]) and np.array_equal(j, want[1])
    assert lib.live_bytes() == live
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("distance") == (0.0, 0)
    ctx.point_segment_distance(pts, a, b)
    ms, launches = ctx.kernel_ms("distance")
    assert ms > 0 and launches == 3, (ms, launches)
    forced(ctx, True)  # 1000 x 777 at 100 000 pairs per launch: 256 points x 390 segments -> 4 x 2 launches
    ctx.point_segment_distance(pts, a, b)
    forced(ctx, False)
    assert ctx.kernel_ms("distance")[1] == 3 + 2 + 8
    xyz, par = distance_ref.random_forest(np.random.default_rng(8), 50)
    ctx.tree_distance(xyz, par, xyz[::-1].copy(), (49 - par[::-1]) * (par[::-1] >= 0) - (par[::-1] < 0))
    assert ctx.kernel_ms("distance")[1] == 3 + 2 + 8 + 6  # two directions
    ctx.set_profiling(False)
    assert lib.live_bytes() == live
