"""The gray-weighted geodesic distance on the GPU (pnr_geodesic_distance, Context.geodesic, advantra_cli --geodesic) against the rule of
include/pnr_hip.h restated in numpy (geodesic_ref.py).  The rule fixes every bit: every comparison is array_equal / ==, there is no
tolerance.  The references are computed once per case and shared (sweeps with each offset applied at once: test_geodesic_host.py shows that
they equal the literal sweeps and the heap bit for bit)."""
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
import geodesic_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")


def _tile_constants():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "geodesic.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (GEO_TX|GEO_TY|GEO_TZ) = (\d+);", txt)}


TILE = _tile_constants()
TX, TY, TZ = TILE["GEO_TX"], TILE["GEO_TY"], TILE["GEO_TZ"]
# (l, h, w): the smallest stacks, a 2-D one, long thin ones, odd sizes over several tiles; then exactly one tile, one voxel more than a tile in
# every axis, two tiles minus one, exactly two tiles
SHAPES = [(1, 2, 2), (2, 2, 2), (3, 3, 3), (1, 21, 33), (70, 2, 2), (2, 300, 2), (2, 2, 300), (5, 67, 131), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1),
          (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1), (2 * TZ, 2 * TY, 2 * TX)]
SHAPES = list(dict.fromkeys(SHAPES))
KINDS = ("open", "rand50", "rand90", "islands", "wall", "faces")
ZDS = (1.0, 2.0, 3.3)
THR = {"open": 0}  # (the other kinds: 128)
MID = (5, 67, 131)


def sid(s):
    return "x".join(map(str, s))


def _ro(V):
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    l, h, w = shape
    rng = np.random.default_rng(abs(hash((shape, KINDS.index(kind)))) % 2**32)
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    if kind == "open":  # random bytes, every voxel passable: the cost does the work
        return _ro(rng.integers(0, 256, shape).astype(np.uint8))
    if kind.startswith("rand"):
        P = rng.random(shape) < int(kind[4:]) / 100
    elif kind == "islands":  # passable blobs of 3 x 3 x 2 voxels in a lattice with impassable gaps: a blob without a source stays NONE
        P = (x % 5 < 3) & (y % 5 < 3) & (z % 3 < 2)
    elif kind == "wall":  # an impassable plane across the longest axis with one hole
        ax = int(np.argmax((w, h, l)))
        c = (x, y, z)[ax]
        P = c != (w, h, l)[ax] // 2
        if min(shape) >= 1 and max(shape) >= 3:
            hole = tuple(int(rng.integers(0, n)) for n in (l, h, w))
            idx = list(hole)
            idx[2 - ax] = (w, h, l)[ax] // 2
            P[tuple(idx)] = True
    else:  # faces: cost steps and impassable voxels on the first and last voxel of tiles only
        on = (x % TX == 0) | (x % TX == TX - 1) | (y % TY == 0) | (y % TY == TY - 1) | (z % TZ == 0) | (z % TZ == TZ - 1)
        V = np.where(on, rng.integers(0, 256, shape), 250)
        return _ro(np.where(on & (rng.random(shape) < 0.25), 5, np.maximum(V, 128)).astype(np.uint8))
    return _ro(np.where(P, rng.integers(128, 256, shape), rng.integers(0, 128, shape)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def seeds(shape, kind):
    """(xyz, labels): several sources of one label, two labels on one voxel, tile corners, a source on an impassable voxel (where there is
    one), a source that is not finite"""
    l, h, w = shape
    V = volume(shape, kind)
    thr = THR.get(kind, 128)
    rng = np.random.default_rng(l * 7919 + h * 104729 + w + KINDS.index(kind))
    ok = np.argwhere(V >= thr)
    pick = ok[rng.integers(0, len(ok), 6)][:, ::-1].astype(np.float32)  # (x, y, z)
    corner = np.array([[min(TX - 1, w - 1), min(TY - 1, h - 1), min(TZ - 1, l - 1)], [min(TX, w - 1), min(TY, h - 1), min(TZ, l - 1)]], np.float32)
    xyz = np.concatenate([pick, pick[:1] + np.float32(0.25), corner, [[np.nan, 1, 1], [0, -np.inf, 0]]])
    labels = [6, 4, 4, 9, 4, 1, 3, 12, 8, 20, 21]
    bad = np.argwhere(V < thr)
    if len(bad):
        xyz = np.concatenate([xyz, bad[:1, ::-1].astype(np.float32)])
        labels = labels + [0]
    return _ro(xyz.astype(np.float32)), _ro(np.array(labels, np.int32))


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


def solve(V, xyz, labels, thr, zd, dmax=ref.DMAX, cost=None, pts=None):
    """-> (K, D, L, info, (d_at, label_at))"""
    t = ref.threshold(V, thr)
    src, kept, dropped = ref.sources(V, t, xyz, labels)
    K, t, _ = ref.sweeps(V, src, thr, zd, dmax, cost, inplace=True)
    D, L = ref.split(K)
    for a in (K, D, L):
        a.setflags(write=False)
    return K, D, L, ref.info(V, K, t, kept, dropped), ref.at(K, pts) if pts is not None else None


@functools.lru_cache(maxsize=None)
def want(shape, kind, zd, dmax=ref.DMAX):
    xyz, labels = seeds(shape, kind)
    return solve(volume(shape, kind), xyz, labels, THR.get(kind, 128), zd, dmax, pts=points(shape))


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
    info, D, L, at = got
    _, wD, wL, winfo, wat = wanted
    assert D.dtype == np.uint32 and np.array_equal(D, wD), (what, int((D != wD).sum()), np.argwhere(D != wD)[:4].tolist())
    assert L.dtype == np.int32 and np.array_equal(L, wL), (what, int((L != wL).sum()), np.argwhere(L != wL)[:4].tolist())
    info = dict(info)
    rounds = info.pop("rounds")
    assert info == winfo and rounds >= (1 if winfo["n_src"] else 0), (what, info, winfo, rounds)
    if wat is not None:
        assert at["d"].dtype == np.uint32 and np.array_equal(at["d"], wat[0]) and at["label"].dtype == np.int32 and np.array_equal(at["label"], wat[1]), (what, at, wat)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_keys_info_and_targets(ctxs, shape, kind):
    V = volume(shape, kind)
    xyz, labels = seeds(shape, kind)
    for zd in ZDS:
        c = ctxs[zd]
        c.set_volume(V)
        same(c.geodesic(xyz, labels, thr=THR.get(kind, 128), targets=points(shape)), want(shape, kind, zd), (shape, kind, zd))
        assert np.array_equal(c.get_volume(), V)  # never written


def test_the_kinds_are_what_they_claim():
    for shape in (MID, (2 * TZ, 2 * TY, 2 * TX)):
        K, D, L, info, _ = want(shape, "open", 2.0)
        assert info["n_reached"] == info["n_pass"] == info["n_vox"] and info["n_src_dropped"] == 2 and info["n_src"] == 9
        K, D, L, info, _ = want(shape, "islands", 2.0)
        assert 0 < info["n_reached"] < info["n_pass"] < info["n_vox"] and info["n_src_dropped"] >= 3 and info["n_src"] + info["n_src_dropped"] == 12  # blobs without a source stay NONE
        for kind in ("rand50", "rand90", "wall", "faces"):
            info = want(shape, kind, 2.0)[3]
            assert 0 < info["n_reached"] <= info["n_pass"] < info["n_vox"] and info["n_src_dropped"] >= 3 and info["n_src"] >= 6, (shape, kind, info)
        # the wall: both sides are reached, so some path went through the hole
        V = volume(shape, "wall")
        ax = int(np.argmax(shape[::-1]))
        half = shape[::-1][ax] // 2
        reached = np.moveaxis(want(shape, "wall", 2.0)[0] != ref.NONE, 2 - ax, 0)
        assert reached[:half].any() and reached[half + 1:].any() and reached[half].sum() == 1
    xyz, labels = seeds(MID, "open")
    c = np.rint(xyz[:7]).astype(int)
    assert (c[0] == c[6]).all() and labels[0] == 6 and labels[6] == 3 and want(MID, "open", 2.0)[2][c[0, 2], c[0, 1], c[0, 0]] == 3  # two labels on one voxel: the smaller


def dmax_values(shape, kind, zd):
    """a cap that cuts close to the sources (inside their tiles) and a medium one, from the reference's own uncapped costs: the 3 % and the
    50 % quantile of D over the reached voxels"""
    K, D = want(shape, kind, zd)[:2]
    d = np.sort(D[K != ref.NONE])
    return max(1, int(d[len(d) * 3 // 100])), int(d[len(d) // 2])


@pytest.mark.parametrize("kind", ["open", "rand90"])
@pytest.mark.parametrize("shape", [MID, (2 * TZ, 2 * TY, 2 * TX), (1, 21, 33)], ids=sid)
def test_dmax_cuts(ctxs, shape, kind):
    """both caps leave reached and unreached passable voxels behind, and change no kept value"""
    V = volume(shape, kind)
    xyz, labels = seeds(shape, kind)
    for zd in (1.0, 2.0):
        c = ctxs[zd]
        c.set_volume(V)
        full = want(shape, kind, zd)
        for dmax in dmax_values(shape, kind, zd):
            w = want(shape, kind, zd, dmax)
            assert 0 < w[3]["n_reached"] < w[3]["n_pass"], (shape, kind, zd, dmax, w[3])
            same(c.geodesic(xyz, labels, thr=THR.get(kind, 128), dmax=dmax, targets=points(shape)), w, (shape, kind, zd, dmax))
            kept = w[0] != ref.NONE
            assert np.array_equal(w[0][kept], full[0][kept]) and (full[1][~kept & (full[0] != ref.NONE)] > dmax).all()


def test_cost_table_threshold_modes_and_defaults(ctx):
    V = synth.synth(48, 40, 24, seed=3)
    ctx.set_volume(V)
    rng = np.random.default_rng(4)
    xyz = np.stack([rng.uniform(0, n, 5) for n in (48, 40, 24)], 1).astype(np.float32)
    cost = rng.integers(1, 400, 256).astype(np.uint16)
    for thr, tab in ((0, cost), (-1, None), (-1, cost), (255, None), (0, np.full(256, 65535, np.uint16)), (0, np.ones(256, np.uint16))):
        w = solve(V, xyz, None, thr, 2.0, cost=tab)
        assert w[3]["thr_used"] == (thr if thr >= 0 else max(1, int(V.astype(np.uint64).sum()) // V.size))
        same(ctx.geodesic(xyz, thr=thr, cost=tab), w, (thr, tab is None))
    w = solve(V, xyz, None, 0, 2.0)
    assert set(np.unique(w[2])) <= set(range(5)) and w[3]["n_reached"] == V.size  # labels = NULL: label i = i
    same(ctx.geodesic(xyz), w, "defaults")
    L = lib.load()
    gi = lib.GeoInfo()
    assert L.pnr_geodesic_distance(ctx.h, xyz.ctypes.data, None, 5, None, C.byref(gi), None, None, None, 0, None, None, 0, None, None) == 0  # opts = NULL
    got = gi.as_dict()
    got.pop("rounds")
    assert got == {k: v for k, v in w[3].items() if k != "max_at"}
    assert L.pnr_geodesic_distance(ctx.h, xyz.ctypes.data, None, 5, None, None, None, None, None, 0, None, None, 0, None, None) == 0  # every output is optional
    ones = solve(V, xyz, None, 0, 2.0, cost=np.ones(256, np.uint16))
    assert ones[3]["d_max"] // 64 <= 48 + 40 + 24  # D / 64: the path length in xy voxels at the brightest cost


def test_sources(ctx):
    shape = (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1)
    V = volume(shape, "rand90")
    ctx.set_volume(V)
    ok = np.argwhere(V >= 128)[:, ::-1].astype(np.float32)
    bad = np.argwhere(V < 128)[:, ::-1].astype(np.float32)
    for xyz, labels in ((ok[:1], [5]), (ok[::97], [3] * len(ok[::97])), (np.concatenate([ok[40:41], ok[40:41], ok[40:41]]), [9, 2, 7]),
                        (np.concatenate([bad[:3], [[np.nan, 0, 0]], ok[-1:]]), [0, 1, 2, 3, 4]), (bad[:2], [1, 1]), (np.zeros((0, 3), np.float32), [])):
        w = solve(V, xyz, np.array(labels, np.int32), 128, 2.0)
        same(ctx.geodesic(xyz, np.array(labels, np.int32), thr=128), w, labels)
    assert solve(V, np.zeros((0, 3), np.float32), [], 128, 2.0)[3]["n_reached"] == 0 and solve(V, bad[:2], [1, 1], 128, 2.0)[3]["n_src_dropped"] == 2
    got = ctx.geodesic(np.zeros((0, 3), np.float32), thr=128)  # n_src = 0: everything is unreached
    assert got[0]["rounds"] == 0 and (got[1] == ref.UNREACHED).all() and (got[2] == -1).all() and got[0]["first_max"] == -1 and got[0]["max_at"] is None


def test_paths(ctx):
    shape = MID
    for kind in ("open", "rand90"):
        V = volume(shape, kind)
        xyz, labels = seeds(shape, kind)
        thr = THR.get(kind, 128)
        K = want(shape, kind, 2.0)[0]
        ctx.set_volume(V)
        pts = points(shape)
        info, _, _, at = ctx.geodesic(xyz, labels, thr=thr, volume=False, targets=pts, path_cap=0)
        assert sorted(at) == ["d", "label"]
        seen = set()
        for cap in (20, lib.PNR_GEO_MAX_PATH):
            lens, walks = ref.paths(V, K, pts, cap, thr=thr, zd=2.0)
            info, D, L, at = ctx.geodesic(xyz, labels, thr=thr, volume=False, targets=pts, path_cap=cap)
            assert D is None and L is None and np.array_equal(at["path_len"], lens), (kind, cap, at["path_len"], lens)
            assert len(at["paths"]) == len(walks) and all(np.array_equal(a, b) for a, b in zip(at["paths"], walks))
            assert np.array_equal(at["d"], ref.at(K, pts)[0])
            seen |= {int(np.sign(n)) for n in lens}
            if cap == 20:
                assert (lens == -20).any() and ((lens > 0) & (lens <= 20)).any() and (lens == 0).any()  # cut, complete and no paths in one call
            else:
                assert (lens > 20).any() and not (lens < 0).any()
                for k, wk in enumerate(walks):  # a complete path ends on a source voxel of the target's label, and its cost is the sum of its edges
                    if len(wk):
                        assert int(K.ravel()[wk[-1]]) >> 32 == 0 and int(K.ravel()[wk[-1]]) == at["label"][k]
        assert seen == {-1, 0, 1}


def test_scheduling_options_change_no_bit(ctx):
    """geo_iters = 1: every visit is one LDS iteration and a tile that changed re-queues itself; geo_tiles_per_launch: launch cuts"""
    shape = MID
    V = volume(shape, "rand90")
    xyz, labels = seeds(shape, "rand90")
    ctx.set_volume(V)
    base = ctx.geodesic(xyz, labels, thr=128, targets=points(shape))
    r0, v0 = ctx.get_option("geo_rounds"), ctx.get_option("geo_visits")
    assert r0 == base[0]["rounds"] >= 2 and v0 >= r0
    same(base, want(shape, "rand90", 2.0), "defaults")
    try:
        for iters, per in ((1, 0), (0, 1), (0, 3), (1, 3), (2, 1)):
            ctx.set_option("geo_iters", iters)
            ctx.set_option("geo_tiles_per_launch", per)
            got = ctx.geodesic(xyz, labels, thr=128, targets=points(shape))
            rounds = got[0]["rounds"]
            same(got, want(shape, "rand90", 2.0), (iters, per))
            # (a launch cut lets later tiles of a round see the keys earlier ones wrote: fewer rounds, the same bits)
            assert ctx.get_option("geo_rounds") == rounds >= 2 and ((iters, per) != (1, 0) or rounds > r0), (iters, per, rounds, r0)
    finally:
        ctx.set_option("geo_iters", 0)
        ctx.set_option("geo_tiles_per_launch", 0)


@pytest.mark.parametrize("shape", [(TZ, TY, TX), (TZ + 1, TY + 1, TX + 1), (1, 21, 33)], ids=sid)
def test_scheduling_options_change_no_bit_at_the_tile_edges(ctx, shape):
    """the re-queue path and a launch per tile where the tile arithmetic has no room: exactly one tile (no neighbour to mark, so one round
    may do), one voxel more than a tile on every axis, and a stack with l = 1"""
    xyz, labels = seeds(shape, "rand90")
    ctx.set_volume(volume(shape, "rand90"))
    try:
        ctx.set_option("geo_iters", 1)
        ctx.set_option("geo_tiles_per_launch", 1)
        same(ctx.geodesic(xyz, labels, thr=128, targets=points(shape)), want(shape, "rand90", 2.0), shape)
    finally:
        ctx.set_option("geo_iters", 0)
        ctx.set_option("geo_tiles_per_launch", 0)


def _snake(shape):
    """a one-voxel corridor in the plane z = 0 that winds back and forth along x, two rows apart"""
    l, h, w = shape
    P = np.zeros(shape, bool)
    rows = list(range(0, h, 2))
    for k, y in enumerate(rows):
        P[0, y, :] = True
        if k + 1 < len(rows):
            P[0, y + 1, w - 1 if k % 2 == 0 else 0] = True
    return _ro(np.where(P, 200, 0).astype(np.uint8)), int(P.sum())


def test_snake_needs_fewer_rounds_than_voxels(ctx):
    V, n = _snake((2, 33, 65))
    src = np.array([[0, 0, 0]], np.float32)
    w = solve(V, src, None, 100, 2.0)
    assert w[3]["n_reached"] == n == w[3]["n_pass"] and w[3]["d_max"] > 64 * 56 * (n - 1) // 2
    ctx.set_volume(V)
    got = ctx.geodesic(src, thr=100)
    rounds = got[0]["rounds"]
    same(got, w, "snake")
    assert 1 < rounds < n, (rounds, n)


@pytest.mark.parametrize("shape", [(3, 9, 33), (1, 8, 65)], ids=sid)
def test_ties_take_the_smallest_label(ctx, shape):
    l, h, w = shape
    V = _ro(np.full(shape, 100, np.uint8))
    xyz = np.array([[3, y, z] for z in range(l) for y in range(h)] + [[w - 4, y, z] for z in range(l) for y in range(h)], np.float32)
    labels = np.array([5] * (h * l) + [2] * (h * l), np.int32)
    want_ = solve(V, xyz, labels, 0, 2.0)
    K = want_[0]
    # the condition: voxels whose equal-cost predecessors carry different labels -- exactly the mid-plane
    ln, tab = ref.lengths(2.0), ref.cost_table()
    tied = 0
    for g in range(V.size):
        x, y, z = g % w, g // w % h, g // (w * h)
        labs = set()
        for (dx, dy, dz), le in zip(ref.OFFSETS, ln):
            qx, qy, qz = x + dx, y + dy, z + dz
            if 0 <= qx < w and 0 <= qy < h and 0 <= qz < l and int(K[qz, qy, qx] >> np.uint64(32)) + le * 2 * int(tab[100]) == int(K.ravel()[g] >> np.uint64(32)):
                labs.add(int(K[qz, qy, qx] & np.uint64(0xFFFFFFFF)))
        if len(labs) > 1:
            tied += 1
            assert x == w // 2 and want_[2].ravel()[g] == 2
    assert tied == h * l
    ctx.set_volume(V)
    same(ctx.geodesic(xyz, labels), want_, "ties")


@pytest.mark.parametrize("shift", [0, 3])
def test_a_borrowed_volume_is_not_written_and_stays_borrowed(ctx, shift):
    import torch
    shape = MID
    V = volume(shape, "rand90")
    xyz, labels = seeds(shape, "rand90")
    flat = torch.from_numpy(np.concatenate([np.full(shift, 99, np.uint8), V.ravel(), np.full(7, 99, np.uint8)])).cuda()
    before = flat.clone()
    torch.cuda.synchronize()
    ctx.set_volume_device(flat.data_ptr() + shift, shape, keepalive=flat)
    same(ctx.geodesic(xyz, labels, thr=128, targets=points(shape)), want(shape, "rand90", 2.0), "borrowed")
    torch.cuda.synchronize()
    assert ctx._keep is flat and torch.equal(flat, before)


def test_pipeline_state_survives():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30), 0)
    V = np.clip(synth.synth(64, 64, 32, seed=2, zdist=2.0).astype(np.int32) + 20, 0, 255).astype(np.uint8)
    c.set_volume(V)
    c.frangi()
    seeds_ = c.extract_seeds()
    assert len(seeds_) > 0
    c.frangi()
    xyz = np.array([[10, 10, 5], [50, 40, 20]], np.float32)
    got = c.geodesic(xyz, thr=-1)
    assert c.extract_seeds().tobytes() == seeds_.tobytes()
    same(got, solve(V, xyz, None, -1, 2.0), "pipeline")
    c.close()


def test_argument_and_state_errors(ctx):
    L = lib.load()
    xyz, out_d, out_l = np.zeros((2, 3), np.float32), np.zeros(2, np.uint32), np.zeros(2, np.int32)
    plen, pvox = np.zeros(2, np.int32), np.zeros((2, 4), np.int64)

    def call(h, src=xyz, lab=None, n=2, opts=None, at=None, m=0, d_at=None, l_at=None, cap=0, pl=None, pv=None):
        p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        return L.pnr_geodesic_distance(h, p(src), p(lab), n, C.byref(opts) if opts is not None else None, None, None, None, p(at), m, p(d_at), p(l_at), cap, p(pl), p(pv))

    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    assert call(fresh.h) == -4 and b"no volume" in L.pnr_last_error()
    assert call(fresh.h, opts=lib.GeoOpts(-1, 0, None)) == -1  # arguments are checked first
    fresh.close()
    shape = (3, 3, 3)
    V = volume(shape, "rand50")
    sx, sl = seeds(shape, "rand50")
    ctx.set_volume(V)
    live, pinned, after, pinned2 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    L.pnr_live_bytes(C.byref(live), C.byref(pinned))
    zero = np.ones(256, np.uint16)
    zero[77] = 0
    for kw in (dict(thr=-2), dict(thr=256), dict(dmax=0), dict(dmax=2**31), dict(cost=zero), dict(labels=np.array([1, -1], np.int32)), dict(path_cap=-1, targets=xyz),
               dict(path_cap=lib.PNR_GEO_MAX_PATH + 1, targets=xyz)):
        with pytest.raises(lib.PnrError, match="error -1"):
            ctx.geodesic(**{"sources": xyz, **kw})
        same(ctx.geodesic(sx, sl, thr=128, targets=points(shape)), want(shape, "rand50", 2.0), "usable after an error")
    assert L.pnr_geodesic_distance(None, None, None, 0, None, None, None, None, None, 0, None, None, 0, None, None) == -1
    assert call(ctx.h, n=-1) == -1 and call(ctx.h, n=(1 << 28) + 1) == -1 and call(ctx.h, src=None) == -1  # sources without src_xyz
    assert call(ctx.h, at=xyz, m=-1, d_at=out_d) == -1 and call(ctx.h, at=xyz, m=(1 << 28) + 1, d_at=out_d) == -1
    assert call(ctx.h, at=None, m=2, d_at=out_d, l_at=out_l) == -1  # targets without at_xyz
    assert call(ctx.h, at=xyz, m=2) == -1  # ... without any output
    assert call(ctx.h, at=xyz, m=2, cap=4, pl=plen) == -1 and call(ctx.h, at=xyz, m=2, cap=4, pv=pvox) == -1  # paths without path_len / path_vox
    assert call(ctx.h, at=xyz, m=2, d_at=out_d) == 0 and call(ctx.h, at=xyz, m=2, l_at=out_l) == 0 and call(ctx.h, at=xyz, m=2, cap=4, pl=plen, pv=pvox) == 0
    L.pnr_live_bytes(C.byref(after), C.byref(pinned2))
    assert after.value == live.value and pinned2.value == pinned.value  # a failing call leaves no buffer behind, nor does a good one
    # the largest edge: max(len) * 2 * max(c) above 2^31 - 1
    steep = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=1000.0), 0)
    steep.set_volume(V)
    with pytest.raises(lib.PnrError, match="error -1"):
        steep.geodesic(sx, sl, cost=np.full(256, 65535, np.uint16))
    same(steep.geodesic(sx, sl, thr=128), solve(V, sx, sl, 128, 1000.0), "zdist 1000")
    steep.close()
    for thr, dmax in ((0, 1), (255, 2**31 - 1)):  # the ends of the ranges are valid
        same(ctx.geodesic(sx, sl, thr=thr, dmax=dmax), solve(V, sx, sl, thr, 2.0, dmax), (thr, dmax))


def test_kernel_time_group_stream_and_live_bytes(ctx):
    import torch
    shape = MID
    V = volume(shape, "rand90")
    xyz, labels = seeds(shape, "rand90")
    ctx.set_volume(V)
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("geodesic") == (0.0, 0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    got = ctx.geodesic(xyz, labels, thr=-1, targets=points(shape), path_cap=16)
    ctx.set_stream(None)
    ctx.set_profiling(False)
    same(got, solve(V, xyz, labels, -1, 2.0, pts=points(shape)), "stream")
    ms, launches = ctx.kernel_ms("geodesic")
    names = ("threshold", "init", "compact", "relax", "stats", "split", "sample", "paths")
    parts = {p: ctx.kernel_ms("geodesic_" + p) for p in names}
    rounds = got[0]["rounds"]
    assert ms > 0 and all(v[0] > 0 for v in parts.values()), (ms, parts)
    assert parts["compact"][1] == rounds + 1 and parts["relax"][1] == rounds and all(parts[p][1] == 1 for p in names if p not in ("compact", "relax")), (parts, rounds)
    assert launches == sum(v[1] for v in parts.values()) and abs(ms - sum(v[0] for v in parts.values())) < 1e-9
    live, pinned, after = C.c_int64(), C.c_int64(), C.c_int64()
    lib.load().pnr_live_bytes(C.byref(live), C.byref(pinned))
    ctx.geodesic(xyz, labels, thr=128, targets=points(shape), path_cap=16)
    lib.load().pnr_live_bytes(C.byref(after), C.byref(pinned))
    assert after.value == live.value  # every device buffer of the call is freed


# ---- the CLI ----
DIMS = (12, 40, 56)  # (l, h, w)


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def test_cli_json_csv_paths_and_raw(tmp_path):
    l, h, w = DIMS
    V = synth.synth(w, h, l, seed=2)
    tif, a, b = str(tmp_path / "s.tif"), tmp_path / "a.swc", tmp_path / "b.swc"
    lib.write_tiff(tif, V)
    a.write_text("# the tree\n1 2 10 10 3 3 -1\n2 2 30.4 20.5 6.2 2.5 1\n7 2 20 35 11 2 2\n")
    b.write_text("4 2 50 30 2.5 1.5 -1\n9 2 -3 60 2.5 1.5 4\n5 2 12 11 3 1 -1\n")
    axyz, _, _, aparent, aids = pnr_amd.read_swc_nodes(a)
    bxyz, _, _, _, bids = pnr_amd.read_swc_nodes(b)
    pts, owner = pnr_amd.tree_sample(axyz, aparent, 1.0, 1.0)
    labels = np.asarray(aids)[owner].astype(np.int32)
    for thr, dmax, zd in ((0, ref.DMAX, 1.0), (-1, ref.DMAX, 2.0), (0, 150000, 3.3)):
        K, D, L, winfo, wat = solve(V, pts, labels, thr, zd, dmax, pts=bxyz)
        lens, walks = ref.paths(V, K, bxyz, lib.PNR_GEO_MAX_PATH, thr=thr, zd=zd)
        flags = (["--threshold", str(thr)] if thr else []) + (["--geo-max", str(dmax)] if dmax != ref.DMAX else []) + (["--zscale", str(zd)] if zd != 1.0 else [])
        r = _cli("--geodesic", "-i", tif, "--from", str(a), "--to", str(b), "--per-node", str(tmp_path / "n.csv"), "--paths", str(tmp_path / "p.swc"), *flags,
                 "--geo-out", str(tmp_path / "g"))
        assert r.returncode == 0, r.stderr[-1500:]
        got = json.loads(r.stdout)
        assert list(got) == ["n_vox", "n_pass", "n_reached", "n_src", "n_src_dropped", "thr_used", "dmax", "zdist", "d_max", "len_max", "max_at", "rounds"]
        rounds = got.pop("rounds")
        assert rounds >= 1 and got == dict(n_vox=winfo["n_vox"], n_pass=winfo["n_pass"], n_reached=winfo["n_reached"], n_src=winfo["n_src"], n_src_dropped=winfo["n_src_dropped"],
                                           thr_used=winfo["thr_used"], dmax=dmax, zdist=float(np.float32(zd)), d_max=winfo["d_max"], len_max=winfo["d_max"] / 64,
                                           max_at=list(winfo["max_at"])), (got, winfo)
        assert open(tmp_path / "g_d.raw", "rb").read() == D.astype("<u4").tobytes() and open(tmp_path / "g_label.raw", "rb").read() == L.astype("<i4").tobytes()
        rows = open(tmp_path / "n.csv").read().split("\n")
        assert rows[0] == "id,d,label" and rows[-1] == ""
        assert [tuple(int(v) for v in r_.split(",")) for r_ in rows[1:-1]] == [(int(i), -1 if d == ref.UNREACHED else int(d), int(lab)) for i, d, lab in zip(bids, *wat)]
        # the chains: one per complete path, under its comment line, from the target's voxel to the source voxel (the root)
        text = open(tmp_path / "p.swc").read().split("\n")
        assert text[-1] == ""
        chains, heads = [], []
        for ln in text[:-1]:
            if ln.startswith("#"):
                heads.append(ln)
                chains.append([])
            else:
                chains[-1].append(ln.split())
        wantc = [(int(bids[k]), int(wat[1][k]), walks[k], int(wat[0][k])) for k in range(len(bids)) if lens[k] > 0]
        assert len(wantc) == len(chains) == len(heads) >= 1, (len(wantc), len(chains), len(heads))
        if dmax != ref.DMAX:
            assert len(wantc) < len(bids)  # the cap leaves a target unreached: no chain for it
        nid = 1
        for (tid, lab, wk, d), head, ch in zip(wantc, heads, chains):
            assert head == "# path %d -> %d: %d voxels, cost %d" % (tid, lab, len(wk), d) and len(ch) == len(wk)
            for j, (f, g) in enumerate(zip(ch, wk)):
                assert [int(v) for v in f] == [nid + j, 2, g % w, g // w % h, g // (w * h), 1, nid + j + 1 if j + 1 < len(wk) else -1]
            nid += len(wk)


# ---- voxel indices above 2^31 ----
def _two_blocks(shape):
    """two blocks of passable and impassable voxels in a stack that is background elsewhere (bigvol.geo_case), borrowed from the device, with
    sources in both (on tile faces, two on one voxel, labels just below 2^31, one on background: dropped), every voxel of both blocks
    as a target and the walks of five targets per block -> (the smallest index of the far block, the expected result).  A step needs both
    of its voxels passable and the threshold is 100, so no path leaves a block: D, L, the walks and the counts are those of
    geodesic_ref.sweeps on the crop around each block, translated; d_max is the larger, max_at its first voxel.  Under the automatic
    options and with one iteration per visit and one tile per launch."""
    import bigvol
    case = bigvol.geo_case(shape)
    first = bigvol.check_placement(case["blocks"], shape, (TZ, TY, TX))
    want = bigvol.geo_want(case)
    reached = want["d"] != ref.UNREACHED
    t, c = bigvol.open_stack(case["blocks"], shape)
    try:
        for iters, per in ((0, 0), (1, 1)):
            c.set_option("geo_iters", iters)
            c.set_option("geo_tiles_per_launch", per)
            info, D, L, at = c.geodesic(case["sources"], case["labels"], thr=case["thr"], volume=False, targets=case["targets"], path_cap=case["path_cap"])
            assert D is None and L is None
            assert {k: info[k] for k in bigvol.GEO_INFO} == want["info"], (iters, info, want["info"])
            assert at["d"].dtype == np.uint32 and np.array_equal(at["d"], want["d"]), (iters, int((at["d"] != want["d"]).sum()))
            assert at["label"].dtype == np.int32 and np.array_equal(at["label"], want["label"]), (iters, int((at["label"] != want["label"]).sum()))
            assert np.array_equal(at["path_len"] > 0, reached) and (at["path_len"] >= 0).all()  # every walk is complete: the cap is enough
            for k, wk in want["paths"].items():
                assert at["path_len"][k] == want["path_len"][k] and at["paths"][k].dtype == np.int64 and np.array_equal(at["paths"][k], wk), (iters, k)
    finally:
        c.set_option("geo_iters", 0)
        c.set_option("geo_tiles_per_launch", 0)
        c.close()
    assert bigvol.untouched(t, case["blocks"])
    return first, want


def test_two_blocks_on_a_small_stack():
    """the placement of the case below at 96 x 64 x 41, where test_bigvol_host.py restates the whole stack"""
    import bigvol
    _two_blocks(bigvol.SMALL)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31): the u64 key volume, geo_sources' tile flags, the ~index word of geo_stats, geo_sample, int64
    voxels from geo_paths; the far block is the last plane, in the one-plane partial tile, and holds the stack's last voxel (a source)"""
    import bigvol
    first, want = _two_blocks(bigvol.SHAPE)
    far = [k for k, p in want["paths"].items() if len(p) and p[0] > 2**31]
    assert first > 2**31 and len(far) >= 3 and all((want["paths"][k] > 2**31).all() for k in far) and max(want["path_len"][k] for k in far) > 3
    assert want["info"]["n_vox"] == int(np.prod(bigvol.SHAPE, dtype=np.int64)) and want["info"]["n_src_dropped"] == 1 and want["info"]["d_max"] > 0
