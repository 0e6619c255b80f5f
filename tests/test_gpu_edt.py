"""The exact Euclidean distance transform on the GPU (pnr_distance_transform, Context.distance_transform, advantra_cli --edt) against the
rule of include/pnr_hip.h restated in numpy (edt_ref.py).  The rule fixes every bit: every comparison is array_equal / ==, there is no
tolerance.  (The 1 x 1 x 1 stack cannot be held by a context and is not listed.)"""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import edt_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")


def _tile_constants():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "edt.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (EDT_WX|EDT_ROWS|EDT_TPB) = (\d+);", txt)}


TILE = _tile_constants()
WX, ROWS, TPB = TILE["EDT_WX"], TILE["EDT_ROWS"], TILE["EDT_TPB"]
assert TPB % WX == 0
# (l, h, w): the smallest stacks, a 2-D one, long thin ones, odd sizes over several tiles; then the tiles: the x pass's is ROWS rows of one
# WX-voxel word, the other passes' is TPB consecutive voxels (TPB / WX rows of one word) -- exactly one tile of each, one voxel more than
# a tile, one voxel less than two tiles, exactly two tiles (equal shapes are listed once)
SHAPES = [(1, 2, 2), (2, 2, 2), (3, 3, 3), (1, 21, 33), (70, 2, 2), (2, 300, 2), (2, 2, 300), (5, 67, 131), (1, ROWS, WX), (1, TPB // WX, WX), (2, ROWS + 1, WX + 1),
          (1, TPB // WX, WX + 1), (3, 2 * ROWS - 1, 2 * WX - 1), (1, 2 * TPB // WX, WX - 1), (2, 2 * ROWS, 2 * WX), (2, TPB // WX, WX)]
SHAPES = list(dict.fromkeys(SHAPES))
BIG = (33, 129, 257)
KINDS = ("zero", "full", "corner", "centre", "slab", "wall_x", "wall_y", "rand50", "rand90", "rand99", "faces", "ball")
ZDS = (1.0, 2.0, 3.3)
RMAXS = (1, 3, 64, 1024)
THR = 128


def sid(s):
    return "x".join(map(str, s))


def _ro(V):
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    """foreground (>= THR) / background (< THR) of the kind, random values on either side"""
    l, h, w = shape
    rng = np.random.default_rng(abs(hash((shape, KINDS.index(kind)))) % 2**32)
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    if kind == "zero":
        B = np.ones(shape, bool)
    elif kind == "full":
        B = np.zeros(shape, bool)
    elif kind == "corner":
        B = (x == 0) & (y == 0) & (z == 0)
    elif kind == "centre":
        B = (x == w // 2) & (y == h // 2) & (z == l // 2)
    elif kind == "slab":  # only the z pass finds anything
        B = z == 0
    elif kind == "wall_x":
        B = x == 0
    elif kind == "wall_y":
        B = y == 0
    elif kind.startswith("rand"):
        B = rng.random(shape) >= int(kind[4:]) / 100
    elif kind == "faces":  # background on the faces of the tiles only: word ends, the rows at a work-group's ends, the ends of a linear tile
        i = x + w * (y + h * z)
        r = y + h * z
        B = ((x % WX == 0) | (x % WX == WX - 1) | (r % ROWS == 0) | (r % ROWS == ROWS - 1) | (i % TPB == 0) | (i % TPB == TPB - 1)) & (rng.random(shape) < 0.5)
    else:  # a foreground sphere of radius 9 (clipped by small stacks)
        B = (x - w // 2) ** 2 + (y - h // 2) ** 2 + (z - l // 2) ** 2 > 81
    return _ro(np.where(B, rng.integers(0, THR, shape), rng.integers(THR, 256, shape)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def points(shape):
    """integer grid points, points at the +-0.5 boundaries between centres, coordinates below 0 and beyond the extent, NaN and inf"""
    l, h, w = shape
    rng = np.random.default_rng(l * 1000003 + h * 1009 + w)
    grid = np.stack([rng.integers(0, n, 24) for n in (w, h, l)], 1).astype(np.float32)
    half = grid[:8] + np.array([[0.5, -0.5, 0.49]], np.float32)
    nudge = grid[8:16] + np.array([[-0.5, 0.4999, -0.51]], np.float32)
    far = np.array([[-3, 1, 0], [w + 7, -0.6, l - 0.5], [1e9, -1e9, 0], [w - 0.5, h - 0.5, l - 0.5], [-0.5, -0.5, -0.5]], np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    return _ro(np.concatenate([grid, half, nudge, far, bad]))


@functools.lru_cache(maxsize=None)
def want(shape, kind, zd, rmax, thr=THR):
    V = volume(shape, kind)
    D, t = ref.transform(V, thr, zd, rmax)
    D.setflags(write=False)
    return D, ref.info(V, D, t, rmax), ref.at(D, points(shape))


@pytest.fixture(scope="module")
def ctxs():
    c = {zd: pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=zd, np_=20), 0) for zd in ZDS}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope="module")
def ctx(ctxs):
    return ctxs[2.0]


def same(got, wanted, what):
    info, d2, at = got
    wd2, winfo, wat = wanted
    assert d2.dtype == np.float32 and np.array_equal(d2, wd2), (what, int((d2 != wd2).sum()), np.argwhere(d2 != wd2)[:4].tolist())
    assert info == winfo, (what, info, winfo)
    assert at.dtype == np.float32 and np.array_equal(at, wat), (what, at, wat)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_d2_info_and_points(ctxs, shape, kind):
    V = volume(shape, kind)
    for zd in ZDS:
        c = ctxs[zd]
        c.set_volume(V)
        for rmax in RMAXS:
            same(c.distance_transform(THR, rmax, points=points(shape)), want(shape, kind, zd, rmax), (shape, kind, zd, rmax))
        assert np.array_equal(c.get_volume(), V)  # never written


def test_the_kinds_are_what_they_claim():
    """a single background voxel gives the formula itself, and the cap edge is crossed; the full stack is the cap everywhere"""
    shape = (3, 2 * ROWS - 1, 2 * WX - 1)
    l, h, w = shape
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    for zd in ZDS:
        zt = np.float32(zd) * z.astype(np.float32)
        formula = (x * x + y * y).astype(np.float32) + zt * zt
        for rmax in RMAXS:
            D, info, _ = want(shape, "corner", zd, rmax)
            assert np.array_equal(D, np.minimum(formula, np.float32(rmax * rmax)))
            assert (info["n_capped"] > 0) == (rmax <= 64) and info["n_fg"] == l * h * w - 1
            D, info, _ = want(shape, "full", zd, rmax)
            assert (D == rmax * rmax).all() and info["n_capped"] == info["n_fg"] == l * h * w and info["first_max"] == 0
    assert not want(shape, "zero", 2.0, 64)[0].any() and want(shape, "zero", 2.0, 64)[1]["first_max"] == -1


def test_larger_stack_once(ctx):
    ctx.set_volume(volume(BIG, "rand99"))
    same(ctx.distance_transform(THR, 64, points=points(BIG)), want(BIG, "rand99", 2.0, 64), BIG)


def test_threshold_modes(ctx):
    """thr = -1 on a tube stack: thr_used is the floor of the exact mean; thr = 0: everything is foreground, the cap everywhere; thr = 255"""
    V = synth.synth(48, 40, 24, seed=3)
    ctx.set_volume(V)
    t = max(1, int(V.astype(np.uint64).sum()) // V.size)
    for thr in (-1, 0, 255):
        D, tu = ref.transform(V, thr, 2.0, 8)
        info, d2, at = ctx.distance_transform(thr, 8)
        assert at is None and tu == info["thr_used"] == (t if thr < 0 else thr)
        assert np.array_equal(d2, D) and info == ref.info(V, D, tu, 8)
    assert (ctx.distance_transform(0, 8)[1] == 64).all()
    got = ctx.distance_transform()  # the defaults: {-1, 64}
    D, tu = ref.transform(V, -1, 2.0, 64)
    assert np.array_equal(got[1], D) and got[0] == ref.info(V, D, tu, 64) and 0 < got[0]["n_fg"] < V.size
    L = lib.load()
    ei = lib.EdtInfo()
    assert L.pnr_distance_transform(ctx.h, None, C.byref(ei), None, None, 0, None) == 0 and ei.as_dict() == {k: got[0][k] for k in ei.as_dict()}  # opts = NULL
    assert L.pnr_distance_transform(ctx.h, None, None, None, None, 0, None) == 0  # every output is optional
    ctx.set_volume(np.zeros((3, 5, 7), np.uint8))
    info, d2, _ = ctx.distance_transform()
    assert info == dict(n_vox=105, n_fg=0, n_capped=0, first_max=-1, d2_max=0.0, thr_used=1, d_max=0.0, max_at=None) and not d2.any()


def test_square_roots_and_points_only(ctx):
    shape = (5, 67, 131)
    ctx.set_volume(volume(shape, "ball"))
    D, winfo, wat = want(shape, "ball", 2.0, 64)
    info, d, at = ctx.distance_transform(THR, 64, points=points(shape), squared=False)
    assert info == winfo and d.dtype == at.dtype == np.float32 and np.array_equal(d, np.sqrt(D))
    assert np.array_equal(at, np.where(wat < 0, np.float32(-1), np.sqrt(np.maximum(wat, 0))).astype(np.float32)) and (at == -1).sum() == 4
    assert info["d_max"] == float(np.sqrt(np.float32(info["d2_max"]))) and D[info["max_at"][::-1]] == info["d2_max"] == D.max()
    info, none, at = ctx.distance_transform(THR, 64, volume=False, points=points(shape))
    assert none is None and info == winfo and np.array_equal(at, wat)
    info, d2, at = ctx.distance_transform(THR, 64, points=np.zeros((0, 3), np.float32))  # n = 0
    assert info == winfo and np.array_equal(d2, D) and at.shape == (0,)


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_a_borrowed_volume_is_not_written_and_stays_borrowed(ctx, shift):
    import torch
    shape = (5, 67, 131)
    V = volume(shape, "rand90")
    flat = torch.from_numpy(np.concatenate([np.full(shift, 99, np.uint8), V.ravel(), np.full(7, 99, np.uint8)])).cuda()
    before = flat.clone()
    torch.cuda.synchronize()
    ctx.set_volume_device(flat.data_ptr() + shift, shape, keepalive=flat)
    same(ctx.distance_transform(THR, 64, points=points(shape)), want(shape, "rand90", 2.0, 64), "borrowed")
    torch.cuda.synchronize()
    assert ctx._keep is flat and torch.equal(flat, before)
    flat[shift:shift + V.size] = 255  # still the caller's memory: the next call sees it
    torch.cuda.synchronize()
    assert (ctx.distance_transform(THR, 3)[1] == 9).all()


def test_after_filter_volume_the_filtered_bytes_are_transformed(ctx):
    import filter_ref
    V = np.clip(synth.synth(48, 40, 24, seed=3).astype(np.int32) + np.random.default_rng(1).integers(0, 40, (24, 40, 48)), 0, 255).astype(np.uint8)
    ctx.set_volume(V)
    plain = ctx.distance_transform(60, 16)[1]
    ctx.filter_volume(median=3)
    Fv = filter_ref.median(V, 3)
    assert np.array_equal(ctx.get_volume(), Fv) and not np.array_equal(Fv, V)
    D, t = ref.transform(Fv, 60, 2.0, 16)
    info, d2, _ = ctx.distance_transform(60, 16)
    assert np.array_equal(d2, D) and info == ref.info(Fv, D, t, 16) and not np.array_equal(d2, plain)


def test_pipeline_state_survives():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30), 0)
    V = np.clip(synth.synth(64, 64, 32, seed=2, zdist=2.0).astype(np.int32) + 20, 0, 255).astype(np.uint8)
    c.set_volume(V)
    c.frangi()
    seeds = c.extract_seeds()
    assert len(seeds) > 0
    c.frangi()
    info, d2, _ = c.distance_transform()
    assert c.extract_seeds().tobytes() == seeds.tobytes()
    D, t = ref.transform(V, -1, 2.0, 64)
    assert np.array_equal(d2, D) and info == ref.info(V, D, t, 64)
    c.close()


def test_argument_and_state_errors(ctx):
    L = lib.load()
    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    o, ei = lib.EdtOpts(-1, 64), lib.EdtInfo()
    assert L.pnr_distance_transform(fresh.h, C.byref(o), C.byref(ei), None, None, 0, None) == -4 and b"no volume" in L.pnr_last_error()
    bad = lib.EdtOpts(-1, 0)
    assert L.pnr_distance_transform(fresh.h, C.byref(bad), None, None, None, 0, None) == -1  # arguments are checked first
    fresh.close()
    shape = (3, 3, 3)
    ctx.set_volume(volume(shape, "rand50"))
    live, pinned, after = C.c_int64(), C.c_int64(), C.c_int64()
    L.pnr_live_bytes(C.byref(live), C.byref(pinned))
    for thr, rmax in ((-1, 0), (-1, 1025), (-1, -5), (-2, 64), (256, 64)):
        with pytest.raises(lib.PnrError, match="error -1"):
            ctx.distance_transform(thr, rmax)
        same(ctx.distance_transform(THR, 3, points=points(shape)), want(shape, "rand50", 2.0, 3), "usable after an error")
    xyz, out = np.zeros((2, 3), np.float32), np.zeros(2, np.float32)
    assert L.pnr_distance_transform(None, None, None, None, None, 0, None) == -1
    assert L.pnr_distance_transform(ctx.h, None, None, None, None, -1, None) == -1
    assert L.pnr_distance_transform(ctx.h, None, None, None, None, (1 << 28) + 1, None) == -1
    assert L.pnr_distance_transform(ctx.h, None, None, None, None, 2, out.ctypes.data) == -1  # points without xyz
    assert L.pnr_distance_transform(ctx.h, None, None, None, xyz.ctypes.data, 2, None) == -1  # ... without d2_at
    L.pnr_live_bytes(C.byref(after), C.byref(pinned))
    assert after.value == live.value  # a failing call leaves no device buffer behind, nor does a good one
    for thr, rmax in ((0, 1), (255, 1024)):  # the ends of the ranges are valid
        D, t = ref.transform(volume(shape, "rand50"), thr, 2.0, rmax)
        assert np.array_equal(ctx.distance_transform(thr, rmax)[1], D)


@pytest.mark.parametrize("rm", [2, 5, 64])
def test_cross_check_against_the_radius_kernel(ctxs, rm):
    """two independent kernels: the largest ball without background (pnr_measure_radii, bg_permille = 0) is
    min(rm, max{k : (float)(k * k) < D2}) of the transform capped at rm + 1 or more"""
    shape = (9, 40, 70)
    rng = np.random.default_rng(rm)
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    blobs = np.zeros(shape, bool)
    for _ in range(6):
        cz, cy, cx = (rng.integers(0, n) for n in shape)
        r = rng.uniform(2, 14)
        blobs |= (x - cx) ** 2 + (y - cy) ** 2 + (2 * (z - cz)) ** 2 < r * r
    for zd, F in ((2.0, blobs), (1.0, rng.random(shape) < 0.97), (3.3, blobs | (rng.random(shape) < 0.3))):
        V = np.where(F, 200, 10).astype(np.uint8)
        pts = np.stack([rng.uniform(-1, n, 300) for n in shape[::-1]], 1).astype(np.float32)
        c = ctxs[zd]
        c.set_volume(V)
        k, t = c.measure_radii(pts, thr=THR, rel_pct=0, rmax=rm, bg_permille=0)
        _, _, d2 = c.distance_transform(THR, rm + 1, volume=False, points=pts)
        ks = np.arange(0, rm + 2)
        below = (ks * ks).astype(np.float32)[None, :] < d2[:, None]  # (float)(k * k) < D2 holds for k = 0 .. the largest such k (none: a background centre)
        wantk = np.minimum(rm, np.maximum(below.sum(1) - 1, 0))
        assert t == THR and (d2 >= 0).all() and np.array_equal(k, wantk.astype(np.int32)), (zd, rm, k[:10], wantk[:10])
        assert len(set(k.tolist())) > 2


def test_kernel_time_group_stream_and_live_bytes(ctx):
    import torch
    shape = (5, 67, 131)
    ctx.set_volume(volume(shape, "rand90"))
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("edt") == (0.0, 0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    got = ctx.distance_transform(-1, 64, points=points(shape))
    ctx.set_stream(None)
    ctx.set_profiling(False)
    V = volume(shape, "rand90")
    D, t = ref.transform(V, -1, 2.0, 64)
    same(got, (D, ref.info(V, D, t, 64), ref.at(D, points(shape))), "stream")
    ms, launches = ctx.kernel_ms("edt")
    parts = [ctx.kernel_ms("edt_" + p) for p in ("threshold", "x", "y", "z", "stats", "sample")]
    assert ms > 0 and launches == 6 and all(p[0] > 0 and p[1] == 1 for p in parts), (ms, launches, parts)
    assert abs(ms - sum(p[0] for p in parts)) < 1e-9
    live, pinned, after = C.c_int64(), C.c_int64(), C.c_int64()
    lib.load().pnr_live_bytes(C.byref(live), C.byref(pinned))
    ctx.distance_transform(THR, 64, points=points(shape))
    lib.load().pnr_live_bytes(C.byref(after), C.byref(pinned))
    assert after.value == live.value  # every device buffer of the call is freed


# ---- the CLI ----
DIMS = (12, 40, 56)  # (l, h, w)


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def test_cli_json_raw_and_csv(tmp_path):
    l, h, w = DIMS
    V = synth.synth(w, h, l, seed=2)
    raw, swc = str(tmp_path / "s.raw"), tmp_path / "t.swc"
    V.tofile(raw)
    swc.write_text("# a comment\n1 2 10 10 3 3 -1\n2 2 50.4 30.5 6.2 2.5 1\n7 2 20 35 11 2 2\n4 2 -3 60 2.5 1.5 -1\n")
    xyz, radius, typ, parent, ids = pnr_amd.read_swc_nodes(swc)
    dims = ",".join(str(v) for v in DIMS[::-1])
    for thr, rmax, zd in ((-1, 64, 1.0), (40, 5, 2.0), (100, 1024, 3.3)):
        c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=zd), 0)
        c.set_volume(V)
        info, d2, at = c.distance_transform(thr, rmax, points=xyz)
        c.close()
        assert info["n_fg"] > 0
        flags = (["--threshold", str(thr)] if thr >= 0 else []) + (["--edt-max", str(rmax)] if rmax != 64 else []) + (["--zscale", str(zd)] if zd != 1.0 else [])
        r = _cli("--edt", "-i", raw, "-d", dims, *flags, "--edt-out", str(tmp_path / "d.raw"), "--at", str(swc), "--per-node", str(tmp_path / "n.csv"))
        assert r.returncode == 0, r.stderr[-1500:]
        got = json.loads(r.stdout)
        assert list(got) == ["n_vox", "n_fg", "n_capped", "thr_used", "rmax", "zdist", "d_max", "max_at"]
        assert got == dict(n_vox=info["n_vox"], n_fg=info["n_fg"], n_capped=info["n_capped"], thr_used=info["thr_used"], rmax=rmax, zdist=float(np.float32(zd)),
                           d_max=info["d_max"], max_at=list(info["max_at"])), (got, info)
        assert open(tmp_path / "d.raw", "rb").read() == np.sqrt(d2).astype("<f4").tobytes()
        rows = open(tmp_path / "n.csv").read().split("\n")
        assert rows[0] == "id,d" and rows[-1] == "" and [int(r.split(",")[0]) for r in rows[1:-1]] == [int(i) for i in ids]
        assert np.array_equal(np.array([r.split(",")[1] for r in rows[1:-1]], np.float32), np.sqrt(at))
    assert np.array_equal(ref.transform(V, 100, 3.3, 1024)[0], d2)  # the Python side of the last round is the rule
    import filter_ref
    r = _cli("--edt", "-i", raw, "-d", dims, "--median", "3d", "--threshold", "40", "--edt-max", "5", "--zscale", "2")
    Fv = filter_ref.median(V, 3)
    D, t = ref.transform(Fv, 40, 2.0, 5)
    winfo = ref.info(Fv, D, t, 5)
    got = json.loads(r.stdout)
    assert r.returncode == 0 and (got["n_fg"], got["n_capped"], got["d_max"], got["max_at"]) == (winfo["n_fg"], winfo["n_capped"], winfo["d_max"], list(winfo["max_at"]))
    blank = str(tmp_path / "z.raw")
    np.zeros(DIMS, np.uint8).tofile(blank)
    r = _cli("--edt", "-i", blank, "-d", dims)
    assert r.returncode == 0 and json.loads(r.stdout) == dict(n_vox=l * h * w, n_fg=0, n_capped=0, thr_used=1, rmax=64, zdist=1.0, d_max=0.0, max_at=None)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 520 voxels (N > 2^31: 64-bit voxel arithmetic in every pass, ~index of the statistics above the sign bit), made on the
    device and borrowed: all background but for two foreground blocks with holes, one in the first planes and one in the last (every
    voxel index of it above 2^31).  A block surrounded by background transforms like the block with a one-voxel margin of background on its own
    (clamping a background voxel's coordinates to the margin never increases a component of the offset); the points read D2 there."""
    import torch
    l, h, w = 520, 2048, 2048
    rng = np.random.default_rng(5)
    blocks = [((1, 3, 5), np.where(rng.random((7, 20, 70)) < 0.97, 255, 0).astype(np.uint8)), ((l - 7, 777, 1000), np.where(rng.random((6, 40, 150)) < 0.995, 200, 0).astype(np.uint8))]
    t = torch.zeros((l, h, w), dtype=torch.uint8, device="cuda")
    for (z0, y0, x0), B in blocks:
        t[z0:z0 + B.shape[0], y0:y0 + B.shape[1], x0:x0 + B.shape[2]] = torch.from_numpy(B).cuda()
    torch.cuda.synchronize()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=2.0), 0)
    c.set_volume_device(t.data_ptr(), (l, h, w), keepalive=t)
    pts, wd2, n_fg, best = [], [], 0, (0.0, -1)
    for (z0, y0, x0), B in blocks:
        D = ref.transform(np.pad(B, 1), 100, 2.0, 64)[0][1:-1, 1:-1, 1:-1]
        zz, yy, xx = np.nonzero(np.ones(B.shape, bool))
        pts.append(np.stack([xx + x0, yy + y0, zz + z0], 1).astype(np.float32))
        wd2.append(D.ravel())
        n_fg += int((B >= 100).sum())
        i = int(np.flatnonzero(D.ravel() == D.max())[0])
        idx = (xx[i] + x0) + w * ((yy[i] + y0) + h * (zz[i] + z0))
        if D.max() > best[0]:
            best = (float(D.max()), int(idx))
    info, _, at = c.distance_transform(100, 64, volume=False, points=np.concatenate(pts))
    c.close()
    assert np.array_equal(at, np.concatenate(wd2))
    assert (info["n_vox"], info["n_fg"], info["n_capped"], info["d2_max"], info["first_max"]) == (l * h * w, n_fg, 0, best[0], best[1])
    assert blocks[1][0][0] * h * w > 2**31 and best[1] > 2**31
    assert int(torch.count_nonzero(t)) == sum(int(np.count_nonzero(B)) for _, B in blocks)  # the borrowed tensor is as it was
