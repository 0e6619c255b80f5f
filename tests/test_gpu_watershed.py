"""The marker-controlled watershed on the GPU (pnr_watershed, Context.watershed / split_touching, advantra_cli --watershed) against the rule
of include/pnr_hip.h restated in numpy (ws_ref.py; test_watershed_host.py shows that its forms agree voxel for voxel).  The rule fixes
every bit: every byte of L and M and every exact info field is compared with array_equal / ==, there is no tolerance.  The references are
computed once per case and shared; every case runs under the automatic options and with ws_iters = 1, ws_tiles_per_launch = 1 (tiles
re-queue themselves, halos go stale inside a round, every tile is a launch of its own)."""
import ctypes as C
import functools
import json
import os
import subprocess
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import ws_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
TZ, TY, TX = ref.tile()
# (l, h, w) around the 32 x 8 x 8 tile: two tiles per axis; three, three and two tiles of odd extents; a 2-D stack; the smallest stack a context
# takes, 2 x 2 x 1 (pnr_set_volume refuses 1 x 1 x 1: test_a_single_voxel_is_no_volume); a single row of tiles; exactly one tile
SHAPES = [(TZ + 1, TY + 1, TX + 1), (10, 17, 70), (1, 7, 31), (1, 2, 2), (TZ, TY, 2 * TX), (TZ, TY, TX)]
# the connectivities of a shape: all four on the two-tiles-per-axis and the 2-D stack
CONNS = {SHAPES[0]: (4, 8, 6, 26), SHAPES[1]: (6, 26), SHAPES[2]: (4, 8, 6, 26), SHAPES[3]: (26,), SHAPES[4]: (4, 26), SHAPES[5]: (6, 26)}
KINDS = ("plateau", "ridge", "serpentine", "adjacent", "drops", "norelief", "rand3")
BIG = 2**31 - 1


def sid(s):
    return "x".join(map(str, s))


def _ro(A):
    if A is not None:
        A = np.ascontiguousarray(A)
        A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """-> dict(V, thr, relief, and markers (an int32 volume) or points + labels): one content, aimed at one way the kernels can go wrong"""
    l, h, w = shape
    rng = np.random.default_rng(KINDS.index(kind) * 1009 + l * 10007 + h * 101 + w)
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    out = {"thr": 0, "relief": None, "markers": None, "points": None, "labels": None}
    if kind == "plateau":  # a constant relief: BFS Voronoi cells, minimum-label ties across the tile borders
        V = np.full(shape, 100, np.uint8)
        out["relief"] = np.full(shape, 7, np.uint8)
        pts = [(0, 0, 0), (w - 1, h - 1, l - 1), (w // 2, h // 2, l // 2), (w - 1, 0, 0), (0, h - 1, l - 1)]
        out["points"], out["labels"] = np.array(pts, np.float32), np.array([5, 2, 9, 2, 7], np.int32)
    elif kind == "ridge":  # low ground, a ridge across x with one pass, a basin behind it that is lower than the pass
        V = np.full(shape, 50, np.uint8)
        R = np.full(shape, 30, np.uint8)
        xr = min(max(w // 2, 1), w - 1)
        R[:, :, xr] = 200
        R[l // 2, h // 2, xr] = 120  # the pass
        R[:, :, xr + 1:] = 10  # the basin
        out["relief"] = R
        out["points"] = np.array([(0, 0, 0)], np.float32)
    elif kind == "serpentine":  # a one-voxel-wide mask through every tile: many rounds
        V, at = ref.serpentine(shape)
        out["thr"] = 1
        out["relief"] = rng.choice(np.array([3, 90, 200], np.uint8), shape)
        mk = np.zeros(shape, np.int32)
        mk[at[0]] = 4
        mk[at[(2 * len(at)) // 3]] = 3
        out["markers"] = mk
    elif kind == "adjacent":  # two markers on adjacent voxels on either side of a tile face (of a stack face where there is one tile)
        V = rng.integers(0, 256, shape).astype(np.uint8)
        xa = min(TX - 1, max(w - 2, 0))
        mk = np.zeros(shape, np.int32)
        mk[l // 2, h // 2, xa] = 8
        mk[l // 2, h // 2, min(xa + 1, w - 1)] = 6 if w > 1 else 8
        out["markers"] = mk
    elif kind == "drops":  # a marker outside the mask, a point that is not finite, a component without a marker, duplicates, labels near 2^31 - 1
        V = np.full(shape, 90, np.uint8)
        V[:, :, w // 2] = 0  # a wall: the far side holds no marker
        V[0, 0, 0] = 0
        out["thr"] = 1
        out["relief"] = rng.integers(0, 4, shape).astype(np.uint8)
        x1 = max(w // 2 - 1, 0)
        pts = [(0, 0, 0), (np.inf, 0, 0), (x1, h - 1, l - 1), (x1 + 0.3, h - 1.2, l - 0.8), (0, h - 1, 0), (0, np.nan, 0), (x1, h - 1, l - 1)]
        out["points"], out["labels"] = np.array(pts, np.float32), np.array([1, 2, BIG, BIG - 1, BIG - 2, 3, BIG - 1], np.int32)
    elif kind == "norelief":  # relief = NULL: 255 - V, under the mean threshold
        V = (rng.integers(0, 256, shape) // 32 * 32).astype(np.uint8)
        out["thr"] = -1
        n = max(1, V.size // 200)
        out["points"] = np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, l, n)], 1).astype(np.float32)
    else:  # rand3: three grey levels of relief, ties everywhere, holes in the mask
        V = np.where(rng.random(shape) < 0.2, 0, 200).astype(np.uint8)
        out["thr"] = 1
        out["relief"] = rng.choice(np.array([0, 128, 255], np.uint8), shape)
        mk = np.zeros(shape, np.int32)
        n = max(1, V.size // 150)
        mk.ravel()[rng.choice(V.size, n, replace=False)] = rng.integers(1, 6, n)
        out["markers"] = mk
    out["V"] = V
    return {k: _ro(v) if isinstance(v, np.ndarray) else v for k, v in out.items()}


def marker_args(c):
    return {k: c[k] for k in ("markers", "points", "labels", "relief", "thr")}


@functools.lru_cache(maxsize=None)
def want(shape, kind, C_):
    c = case(shape, kind)
    solver = ref.flood_heap if kind == "serpentine" else ref.flood_sweeps  # (few voxels and long paths: the heap; else the sweeps)
    info, L, M, _ = ref.run(c["V"], c["thr"], C_, c["relief"], c["markers"], c["points"], c["labels"], solver=solver)
    return info, _ro(L), _ro(M)


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20), 0)
    yield c
    c.close()


def same(got, wanted, what):
    info, L, M = got
    winfo, wL, wM = wanted
    assert L.dtype == np.int32 and L.shape == wL.shape and np.array_equal(L, wL), (what, int((L != wL).sum()), np.argwhere(L != wL)[:4].tolist())
    assert M.dtype == np.uint8 and np.array_equal(M, wM), (what, int((M != wM).sum()), np.argwhere(M != wM)[:4].tolist())
    assert {k: info[k] for k in ref.EXACT} == winfo, (what, info, winfo)
    assert info["flood_rounds"] >= 1 and info["label_rounds"] >= 1 and min(info["flood_visits"], info["label_visits"]) >= info["tiles"], (what, info)


@pytest.mark.parametrize("sched", ("auto", "requeue"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_every_content_shape_and_connectivity(ctx, shape, kind, sched):
    c = case(shape, kind)
    ctx.set_volume(c["V"])
    try:
        if sched == "requeue":
            ctx.set_option("ws_iters", 1)
            ctx.set_option("ws_tiles_per_launch", 1)
        for C_ in CONNS[shape]:
            got = ctx.watershed(connectivity=C_, levels=True, **marker_args(c))
            same(got, want(shape, kind, C_), (shape, kind, C_, sched))
            assert got[0]["flood_rounds"] + got[0]["label_rounds"] == ctx.get_option("ws_rounds")
            assert got[0]["flood_visits"] + got[0]["label_visits"] == ctx.get_option("ws_visits")
    finally:
        ctx.set_option("ws_iters", 0)
        ctx.set_option("ws_tiles_per_launch", 0)
    assert np.array_equal(ctx.get_volume(), c["V"])  # pnr_watershed leaves the volume alone


def test_a_single_voxel_is_no_volume():
    """1 x 1 x 1 never reaches the watershed: the context takes no stack below 2 x 2 x 1, and without a volume the call is PNR_E_STATE"""
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20), 0)
    try:
        with pytest.raises(pnr_amd.PnrError, match="at least 2x2x1"):
            c.set_volume(np.full((1, 1, 1), 9, np.uint8))
        c.shape = (1, 1, 1)
        with pytest.raises(pnr_amd.PnrError, match="error -4: pnr_watershed: no volume set"):
            c.watershed(points=[[0, 0, 0]])
    finally:
        c.close()


def test_the_contents_are_what_they_are_aimed_at():
    """the references themselves: the properties each content is there for"""
    s = SHAPES[1]
    info, L, M = want(s, "plateau", 26)
    assert info["m_max"] == 7 and info["n_regions"] == 4 and info["n_unreached"] == 0 and (M == 7).all()
    info, L, M = want(s, "ridge", 6)
    R = case(s, "ridge")["relief"]
    xr = s[2] // 2
    assert (M[:, :, xr + 1:] == 120).all() and (R[:, :, xr + 1:] == 10).all() and info["m_max"] == 200  # the basin keeps the pass height
    info, L, M = want(s, "serpentine", 26)
    assert info["n_unreached"] == 0 and info["d_max"] > 3 * TX and set(np.unique(L)) == {0, 3, 4}
    info, L, M = want(s, "drops", 26)
    assert info["n_dropped"] == 3 and info["n_unreached"] > 0 and info["n_marker_vox"] == 2 and set(np.unique(L)) == {0, BIG - 2, BIG - 1}
    info, _, _ = want(s, "adjacent", 6)
    assert info["n_regions"] == 2 and info["n_marker_vox"] == 2
    for kind in KINDS:  # a single slice: 6 is 4 and 26 is 8
        assert np.array_equal(want(SHAPES[2], kind, 6)[1], want(SHAPES[2], kind, 4)[1]) and np.array_equal(want(SHAPES[2], kind, 26)[1], want(SHAPES[2], kind, 8)[1])


def test_requeueing_takes_more_rounds_and_changes_no_bit(ctx):
    shape = SHAPES[1]
    c = case(shape, "serpentine")
    ctx.set_volume(c["V"])
    a = ctx.watershed(connectivity=6, levels=True, **marker_args(c))
    try:
        ctx.set_option("ws_iters", 1)
        b = ctx.watershed(connectivity=6, levels=True, **marker_args(c))
    finally:
        ctx.set_option("ws_iters", 0)
    same(a, want(shape, "serpentine", 6), "auto")
    same(b, want(shape, "serpentine", 6), "ws_iters = 1")
    assert b[0]["flood_rounds"] > a[0]["flood_rounds"] >= 2 and b[0]["label_rounds"] > a[0]["label_rounds"] >= 2, (a[0], b[0])


@pytest.mark.parametrize("shape", SHAPES[:3], ids=sid)
def test_the_point_form_equals_the_volume_form(ctx, shape):
    c = case(shape, "drops")
    mask, R, mark, t, dropped = ref.setup(c["V"], c["thr"], c["relief"], points=c["points"], labels=c["labels"])
    ctx.set_volume(c["V"])
    a = ctx.watershed(points=c["points"], labels=c["labels"], relief=c["relief"], thr=c["thr"], levels=True)
    b = ctx.watershed(markers=mark.astype(np.int32), relief=c["relief"], thr=c["thr"], levels=True)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert {k: a[0][k] for k in ref.EXACT if k != "n_dropped"} == {k: b[0][k] for k in ref.EXACT if k != "n_dropped"}
    assert a[0]["n_dropped"] == dropped == 3 and b[0]["n_dropped"] == 0
    # labels = None numbers the points 1 .. n; volume / levels = False return None
    info, L, M = ctx.watershed(points=c["points"], relief=c["relief"], thr=c["thr"], volume=False)
    winfo, _, _, _ = ref.run(c["V"], c["thr"], 26, c["relief"], points=c["points"])
    assert L is None and M is None and {k: info[k] for k in ref.EXACT} == winfo


def test_volume_and_pipeline_state_are_untouched(ctx):
    import synth
    Lb = lib.load()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30), 0)
    try:
        V = np.clip(synth.synth(64, 64, 32, seed=2, zdist=2.0).astype(np.int32) + 20, 0, 255).astype(np.uint8)
        c.set_volume(V)
        c.frangi()
        seeds_ = c.extract_seeds()
        assert len(seeds_) > 0
        c.frangi()
        live, pinned, after, pinned2 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        Lb.pnr_live_bytes(C.byref(live), C.byref(pinned))
        pts = np.array([[10, 10, 5], [50, 40, 20]], np.float32)
        info, L, M = c.watershed(points=pts, thr=-1, levels=True)
        Lb.pnr_live_bytes(C.byref(after), C.byref(pinned2))
        assert after.value == live.value and pinned2.value == pinned.value  # every buffer of the call is gone
        assert c.extract_seeds().tobytes() == seeds_.tobytes() and np.array_equal(c.get_volume(), V)
        winfo, wL, wM, _ = ref.run(V, -1, 26, points=pts, solver=ref.flood_sweeps)
        same((info, L, M), (winfo, wL, wM), "pipeline")
    finally:
        c.close()


def test_arguments(ctx):
    """code and full text per bad argument, in the order of the checks"""
    L = lib.load()
    shape = (2, 3, 4)
    V = np.full(shape, 9, np.uint8)
    ctx.set_volume(V)
    n = V.size
    mk = np.zeros(n, np.int32)
    mk[5] = 1
    xyz = np.zeros(3, np.float32)
    lab = np.array([1], np.int32)
    o = lib.WatershedOpts(0, 26)

    def call(h, opts, relief, mv, pts, labels, n_src):
        rc = L.pnr_watershed(h, C.byref(opts) if opts is not None else None, relief, mv.ctypes.data if mv is not None else None,
                             pts.ctypes.data if pts is not None else None, labels.ctypes.data if labels is not None else None, n_src, None, None, None)
        return rc, L.pnr_last_error().decode()

    assert call(None, o, None, mk, None, None, 0) == (-1, "null argument") and call(ctx.h, None, None, mk, None, None, 0) == (-1, "null argument")
    assert call(ctx.h, lib.WatershedOpts(-2, 26), None, mk, None, None, 0) == (-1, "pnr_watershed: thr = -2 outside [-1, 255]")
    assert call(ctx.h, lib.WatershedOpts(256, 5), None, mk, None, None, 0) == (-1, "pnr_watershed: thr = 256 outside [-1, 255]")
    assert call(ctx.h, lib.WatershedOpts(0, 5), None, mk, None, None, -1) == (-1, "pnr_watershed: connectivity = 5, not 0, 4, 8, 6 or 26")
    assert call(ctx.h, o, None, mk, None, None, -1) == (-1, "pnr_watershed: n_src = -1 outside [0, 2^31 - 2]")
    assert call(ctx.h, o, None, None, xyz, None, 2**31 - 1) == (-1, "pnr_watershed: n_src = 2147483647 outside [0, 2^31 - 2]")
    both = "pnr_watershed: markers as a volume and as points, exactly one of the two forms"
    assert call(ctx.h, o, None, mk, xyz, None, 1) == (-1, both) and call(ctx.h, o, None, mk, None, lab, 0) == (-1, both) and call(ctx.h, o, None, mk, xyz, None, 0) == (-1, both)
    assert call(ctx.h, o, None, None, xyz, None, 0) == (-1, "pnr_watershed: no markers, neither marker_vol nor n_src > 0")
    assert call(ctx.h, o, None, None, None, None, 0) == (-1, "pnr_watershed: no markers, neither marker_vol nor n_src > 0")
    assert call(ctx.h, o, None, None, None, lab, 1) == (-1, "pnr_watershed: n_src = 1 needs src_xyz")
    assert call(ctx.h, o, None, None, xyz, np.array([0], np.int32), 1) == (-1, "pnr_watershed: src_label[0] = 0, labels are at least 1")
    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20), 0)
    try:
        assert call(fresh.h, o, None, mk, None, None, 0) == (-4, "pnr_watershed: no volume set")  # PNR_E_STATE
        assert call(fresh.h, o, None, None, xyz, np.array([-3], np.int32), 1)[0] == -1  # ... after the arguments
    finally:
        fresh.close()
    bad = mk.copy()
    bad[7] = -2
    assert call(ctx.h, o, None, bad, None, None, 0) == (-1, "pnr_watershed: marker_vol[7] = -2 is negative")
    assert call(ctx.h, o, None, mk, None, None, 0)[0] == 0 and call(ctx.h, lib.WatershedOpts(0, 0), None, None, xyz, lab, 1)[0] == 0
    info, Lv, _ = ctx.watershed(markers=np.zeros(shape, np.int32), thr=0, connectivity=0)  # no marker at all: nothing is reached
    assert info["connectivity"] == 26 and info["n_reached"] == 0 and info["n_unreached"] == n and info["n_regions"] == 0 and not Lv.any()
    for key in ("ws_iters", "ws_tiles_per_launch"):
        with pytest.raises(pnr_amd.PnrError):
            ctx.set_option(key, -1)
    with pytest.raises(pnr_amd.PnrError):
        ctx.set_option("ws_rounds", 1)


def test_kernel_times(ctx):
    c = case(SHAPES[0], "rand3")
    ctx.set_volume(c["V"])
    ctx.set_profiling(True)
    try:
        ctx.reset_kernel_ms()
        info, _, _ = ctx.watershed(**marker_args(c))
        parts = [ctx.kernel_ms("watershed_" + k) for k in ("init", "compact", "flood", "label", "finish")]
        total = ctx.kernel_ms("watershed")
        assert total[1] == sum(p[1] for p in parts) and abs(total[0] - sum(p[0] for p in parts)) < 1e-6 and all(p[1] >= 1 for p in parts)
        assert parts[1][1] == info["flood_rounds"] + info["label_rounds"] + 2 and parts[2][1] == info["flood_rounds"] and parts[3][1] == info["label_rounds"]
    finally:
        ctx.set_profiling(False)


def test_split_touching_parts_two_overlapping_balls(ctx):
    V, centres = ref.two_balls()
    V = _ro(V)
    ctx.set_volume(V)
    cinfo, _, _ = ctx.label_components(thr=100, connectivity=26)
    assert cinfo["n_comp"] == 1  # one component, whatever the threshold
    info, L, n_cells = ctx.split_touching(h=2, thr=100)
    assert n_cells == 2 and info["n_regions"] == 2 and info["n_unreached"] == 0
    (x1, y1, z1), (x2, y2, z2) = centres
    assert L[z1, y1, x1] > 0 and L[z2, y2, x2] > 0 and L[z1, y1, x1] != L[z2, y2, x2]
    assert ((L > 0) == (V >= 100)).all()
    wL, wn = ref.split_touching(V, 2, ctx.p.zdist, thr=100)
    assert wn == 2 and np.array_equal(L, wL)
    assert np.array_equal(ctx.get_volume(), V)


def test_cli_labels_equal_the_python_call(ctx, tmp_path):
    shape = SHAPES[0]
    l, h, w = shape
    c = case(shape, "norelief")
    raw, swc, out, lev = (str(tmp_path / n) for n in ("v.raw", "t.swc", "labels.raw", "levels.raw"))
    c["V"].tofile(raw)
    # two trees: a chain of three nodes and a single node
    nodes = [(1, 2.0, 3.0, 1.0, -1), (2, 10.0, 4.0, 2.0, 1), (3, 20.0, 5.0, 4.0, 2), (4, 30.0, 7.0, 8.0, -1)]
    with open(swc, "w") as f:
        for i, x, y, z, p in nodes:
            f.write("%d 3 %g %g %g 1 %d\n" % (i, x, y, z, p))
    pts = np.array([n[1:4] for n in nodes], np.float32)
    ctx.set_volume(c["V"])
    for by, labels in (("tree", [1, 1, 1, 2]), ("node", [1, 2, 3, 4])):
        r = subprocess.run([CLI, "--watershed", "-i", raw, "-d", "%d,%d,%d" % (w, h, l), "--markers-swc", swc, "--markers-by", by, "--threshold", "0",
                            "--connectivity", "6", "--labels", out, "--levels", lev], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        info, L, M = ctx.watershed(points=pts, labels=labels, thr=0, connectivity=6, levels=True)
        assert np.array_equal(np.fromfile(out, np.int32).reshape(shape), L) and np.array_equal(np.fromfile(lev, np.uint8).reshape(shape), M), by
        js = json.loads(r.stdout.strip().splitlines()[-1])
        assert {k: js[k] for k in ref.EXACT} == {k: info[k] for k in ref.EXACT} and (js["w"], js["h"], js["l"]) == (w, h, l) and js["markers_by"] == by
        assert js["n_regions"] == len(set(labels))


# ---- voxel indices above 2^31 ----
def _two_blocks(shape):
    """the "rand3" content (holes in the mask, three levels of relief, ties everywhere, labels 1..5) and the "adjacent" pair (two markers on
    either side of a tile face) in both blocks of a stack that is background elsewhere (bigvol.ws_case), borrowed from the device; the
    markers are points, the relief is 255 - V, for 26 and 6 neighbours -> (the smallest index of the far block, the infos).  The mask is
    V >= 1 and a key passes between mask voxels only, so no region leaves its block: L and M on the crop around each block are those of
    ws_ref.run on the crop, L is 0 everywhere else (counted over the whole array), the counts are the sums and the maxima."""
    import bigvol
    case = bigvol.ws_case(shape)
    first = bigvol.check_placement(case["blocks"], shape, (TZ, TY, TX))
    t, c = bigvol.open_stack(case["blocks"], shape)
    infos = []
    try:
        for conn in (26, 6):
            winfo, parts = bigvol.ws_want(case, conn)
            info, L, M = c.watershed(points=case["points"], labels=case["labels"], relief=None, thr=case["thr"], connectivity=conn, volume=True, levels=True)
            assert {k: info[k] for k in ref.EXACT} == winfo, (conn, info, winfo)
            assert L.dtype == np.int32 and M.dtype == np.uint8 and L.shape == M.shape == tuple(shape)
            for (z0, y0, x0), wl, wm in parts:
                at = (slice(z0, z0 + wl.shape[0]), slice(y0, y0 + wl.shape[1]), slice(x0, x0 + wl.shape[2]))
                assert np.array_equal(L[at], wl), (conn, (z0, y0, x0), int((L[at] != wl).sum()), np.argwhere(L[at] != wl)[:4].tolist())
                assert np.array_equal(M[at], wm), (conn, (z0, y0, x0), int((M[at] != wm).sum()), np.argwhere(M[at] != wm)[:4].tolist())
            assert np.count_nonzero(L) == winfo["n_reached"] and np.count_nonzero(M) == sum(np.count_nonzero(wm) for _, _, wm in parts)  # no stray store
            assert info["flood_rounds"] >= 1 and info["label_rounds"] >= 1 and min(info["flood_visits"], info["label_visits"]) >= info["tiles"]
            infos.append(info)
            del L, M
    finally:
        c.close()
    assert bigvol.untouched(t, case["blocks"])
    return first, infos


def test_two_blocks_on_a_small_stack():
    """the placement of the case below at 96 x 64 x 41, where test_bigvol_host.py restates the whole stack"""
    import bigvol
    _two_blocks(bigvol.SMALL)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31): ws_init's indices and marker list, the stores of both relaxations, ws_finish's statistics; the far
    block is the last plane, in the one-plane partial tile, and holds the stack's last voxel.  Round 1 of either pass lists every tile,
    more than the 2^20 of an automatic launch, so the cut launches run.  The one test here that downloads whole volumes (L and M)."""
    import bigvol
    l, h, w = bigvol.SHAPE
    first, infos = _two_blocks(bigvol.SHAPE)
    assert first > 2**31
    for info in infos:
        assert info["tiles"] == -(-l // TZ) * -(-h // TY) * -(-w // TX) and info["flood_visits"] >= info["tiles"] > 2**20 and info["n_vox"] == l * h * w
