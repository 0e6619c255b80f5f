"""Joining trace fragments along the signal on the GPU (pnr_geodesic_bridges, Context.join_trees_geodesic, pnr_amd.join_expand, advantra_cli
--join-geodesic) against the rule of include/pnr_hip.h restated in numpy (geojoin_ref.py).  The rule fixes every bit: bridges, paths, info,
the expanded arrays and the CLI's file are compared with array_equal / ==, there is no tolerance.  The images come from the generators of
test_gpu_geodesic.py; the references are computed once per case and shared."""
import ctypes as C
import functools
import json
import os
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import geodesic_ref as geo
import geojoin_ref as ref
import join_ref
from test_gpu_geodesic import MID, TX, TY, TZ, ZDS, sid, volume

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
ONE, MORE, TWO = (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1), (2 * TZ, 2 * TY, 2 * TX)
# (l, h, w): the smallest volume a context takes (2 x 2 x 1; the two-adjacent-voxels case runs on it), the smallest cube, the 2-D mode, long thin ones, exactly one tile, one voxel more in every axis, exactly two tiles
# in every axis, odd sizes over several tiles
SHAPES = list(dict.fromkeys([(1, 2, 2), (2, 2, 2), (1, 21, 33), (70, 2, 2), (2, 2, 300), ONE, MORE, TWO, MID]))
KINDS = ("open", "rand50", "wall", "const")
THR = {"open": 0, "const": 0}  # (the other kinds: 128)


def image(shape, kind):
    if kind == "const":  # massive ties in W: the second pass and the (p, o) order decide
        V = np.full(shape, 255, np.uint8)
        V.setflags(write=False)
        return V
    return volume(shape, kind)


@functools.lru_cache(maxsize=None)
def forest(shape, kind, trees):
    """`trees` fragments on distinct passable voxels; every second one has a child a few voxels away (its segment is sampled at step 1, and
    the child may sit on an impassable voxel or on another fragment's), every fifth a grandchild"""
    l, h, w = shape
    V = image(shape, kind)
    rng = np.random.default_rng(l * 7919 + h * 104729 + w + 31 * KINDS.index(kind) + trees)
    ok = np.argwhere(V >= THR.get(kind, 128))[:, ::-1]
    roots = ok[rng.permutation(len(ok))[:trees]]
    xyz, parent = [], []
    for k, r in enumerate(roots):
        xyz.append(r)
        parent.append(-1)
        for _ in range((k % 2) + (k % 5 == 4)):
            parent.append(len(xyz) - 1)
            xyz.append(np.clip(xyz[-1] + rng.integers(-4, 5, 3), 0, (w - 1, h - 1, l - 1)))
    xyz, parent = np.array(xyz, np.float32), np.array(parent, np.int32)
    xyz.setflags(write=False), parent.setflags(write=False)
    return xyz, parent


@functools.lru_cache(maxsize=None)
def want(shape, kind, trees, zd, limit=0):
    xyz, parent = forest(shape, kind, trees)
    bridges, vox, info, K = ref.solve(image(shape, kind), xyz, parent, zd, limit=limit, thr=THR.get(kind, 128))
    return bridges, vox, info, ref.expand(xyz, parent, bridges, vox, shape)


def solved(V, xyz, parent, zd, **kw):
    """-> (bridges, vox, info, the expanded arrays) of the reference"""
    bridges, vox, info, _ = ref.solve(V, xyz, parent, zd, **kw)
    return bridges, vox, info, ref.expand(xyz, parent, bridges, vox, V.shape)


@pytest.fixture(scope="module")
def ctxs():
    c = {zd: pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=zd, np_=20), 0) for zd in ZDS}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope="module")
def ctx(ctxs):
    return ctxs[2.0]


def same(got, wanted, xyz, parent, what, rounds_min=1):
    bridges, paths, info = got
    wb, wvox, winfo, wexp = wanted
    assert bridges.dtype == lib.GEO_BRIDGE and bridges.tobytes() == wb.astype(lib.GEO_BRIDGE).tobytes(), (what, bridges, wb)
    assert paths["vox"].dtype == np.int64 and np.array_equal(paths["vox"], wvox), what
    info = dict(info)
    rounds = info.pop("rounds")
    assert info == winfo and rounds >= (rounds_min if winfo["n_trees_in"] >= 2 else 0), (what, info, winfo, rounds)
    exp = pnr_amd.join_expand(xyz, parent, bridges, paths)
    assert all(np.array_equal(a, b) for a, b in zip(exp[:3], wexp[:3])) and exp[3].tobytes() == wexp[3].tobytes(), what


def run(c, shape, kind, trees, zd, limit=0):
    xyz, parent = forest(shape, kind, trees)
    return c.join_trees_geodesic(xyz, parent, limit=limit, thr=THR.get(kind, 128))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_bridges_paths_info_and_expansion(ctxs, shape, kind):
    V = image(shape, kind)
    for zd in ZDS if V.size <= 4096 else ZDS[SHAPES.index(shape) % 3:][:1]:
        c = ctxs[zd]
        c.set_volume(V)
        xyz, parent = forest(shape, kind, 5)
        same(run(c, shape, kind, 5, zd), want(shape, kind, 5, zd), xyz, parent, (shape, kind, zd))
        assert np.array_equal(c.get_volume(), V)  # never written


@pytest.mark.parametrize("trees", [2, 40])
@pytest.mark.parametrize("shape,kind,zd", [(MID, "open", 1.0), (MID, "rand50", 3.3), ((2, 2, 300), "rand50", 1.0), ((70, 2, 2), "rand50", 2.0), (TWO, "const", 2.0),
                                           ((1, 21, 33), "wall", 2.0)], ids=str)
def test_two_and_forty_trees(ctxs, shape, kind, zd, trees):
    ctxs[zd].set_volume(image(shape, kind))
    xyz, parent = forest(shape, kind, trees)
    same(run(ctxs[zd], shape, kind, trees, zd), want(shape, kind, trees, zd), xyz, parent, (shape, kind, trees))


def test_the_kinds_are_what_they_claim():
    for shape in (MID, TWO):
        for trees in (5, 40):
            info = want(shape, "open", trees, 2.0 if shape == TWO else 1.0)[2] if (shape, trees) != (TWO, 40) else None
            if info:
                assert info["n_trees_out"] == 1 and info["n_trees_lost"] == 0 and info["n_bridges"] == trees - 1 and info["n_inserted"] > 0, (shape, trees, info)
    # rand50: whole trees are unreachable -- the reference leaves at least one unjoined
    for shape, zd in (((2, 2, 300), 1.0), ((70, 2, 2), 2.0)):
        info = want(shape, "rand50", 40, zd)[2]
        assert info["n_trees_out"] > 1 and info["n_bridges"] >= 1 and info["n_src_dropped"] >= 1, info
    assert want((70, 2, 2), "rand50", 40, 2.0)[2]["n_trees_lost"] >= 1
    # wall: both sides hold fragments, so a bridge passes the one hole
    shape = MID
    bridges, vox, info, _ = want(shape, "wall", 5, ZDS[SHAPES.index(shape) % 3])
    V = image(shape, "wall")
    ax = int(np.argmax(shape[::-1]))
    half = shape[::-1][ax] // 2
    coord = [vox % shape[2], vox // shape[2] % shape[1], vox // (shape[2] * shape[1])][ax]
    assert info["n_trees_out"] == 1 and (coord < half).any() and (coord > half).any() and (coord == half).sum() >= 1
    hole = np.flatnonzero(np.moveaxis(V >= 128, 2 - ax, 0)[half].ravel())
    assert len(hole) == 1
    # const: every bridge weight occurs on many meet edges -- the second pass decides
    bridges, vox, info, _ = want(TWO, "const", 5, ZDS[SHAPES.index(TWO) % 3])
    xyz, parent = forest(TWO, "const", 5)
    K = ref.solve(image(TWO, "const"), xyz, parent, ZDS[SHAPES.index(TWO) % 3])[3]
    W, P, O = ref.meet_edges(image(TWO, "const"), K, ZDS[SHAPES.index(TWO) % 3])
    assert all((W == b["w"]).sum() > 1 for b in bridges) and len(bridges) == 4


def test_two_one_node_trees_on_adjacent_voxels(ctxs):
    """k = 0: the chain is the two source voxels, nothing is inserted, and the bridge handed to the re-rooting is (a, b)"""
    for shape, kind in (((1, 2, 2), "const"), ((1, 2, 2), "open"), ((2, 2, 2), "open")):
        V = image(shape, kind)
        for zd in ZDS:
            ctxs[zd].set_volume(V)
            for a, b in (((0, 0, 0), (1, 0, 0)), ((1, 0, 0), (0, 1, 0)), ((1, 1, shape[0] - 1), (0, 0, 0))):
                xyz, parent = np.array([a, b], np.float32), np.array([-1, -1], np.int32)
                w = solved(V, xyz, parent, zd)
                assert len(w[0]) == 1
                if kind == "const" or a[1:] == b[1:]:  # (across a diagonal of random costs a detour over a third voxel can be cheaper)
                    assert w[0]["path_len"][0] == 2 and w[2]["n_inserted"] == 0 and w[3][3][0]["lo"] == 0 and w[3][3][0]["hi"] == 1 and len(w[3][0]) == 2
                same(ctxs[zd].join_trees_geodesic(xyz, parent), w, xyz, parent, (shape, kind, zd, a, b))


def test_eight_trees_on_a_line_take_two_rounds(ctx):
    shape = (1, 3, 64)
    V = np.full(shape, 255, np.uint8)
    xyz = np.array([[4 + 8 * k, 1, 0] for k in range(8)], np.float32)
    parent = np.full(8, -1, np.int32)
    w = solved(V, xyz, parent, 2.0)
    assert len(w[0]) == 7 and len(set(w[0]["w"].tolist())) == 1
    ctx.set_volume(V)
    got = ctx.join_trees_geodesic(xyz, parent)
    same(got, w, xyz, parent, "line")
    assert ctx.get_option("geojoin_rounds") == got[2]["rounds"] >= 2


def test_shared_voxels_hidden_trees_and_impassable_sources(ctx):
    shape = MORE
    V = volume(shape, "rand50")
    ok = np.argwhere(V >= 128)[:, ::-1].astype(np.float32)
    bad = np.argwhere(V < 128)[:, ::-1].astype(np.float32)
    # tree 0: ok[0] - ok[5]; tree 2 (node 2, 3): a node on ok[5] as well, and one elsewhere; tree 4: one node, hidden under tree 0 on ok[0];
    # tree 5 (node 5, 6): a node on an impassable voxel and one on a passable; tree 7: only an impassable voxel -- lost as well
    xyz = np.stack([ok[0], ok[5], ok[5] + np.float32(0.25), ok[40], ok[0], bad[0], ok[90], bad[3]]).astype(np.float32)
    parent = np.array([-1, 0, -1, 2, -1, -1, 5, -1], np.int32)
    for step in (0, 1):
        w = solved(V, xyz, parent, 2.0, thr=128, step=step)
        assert w[2]["n_trees_in"] == 5 and w[2]["n_trees_lost"] == 2 and w[2]["n_src_dropped"] >= 2 and not {4, 7} & (set(w[0]["a"].tolist()) | set(w[0]["b"].tolist()))
        ctx.set_volume(V)
        same(ctx.join_trees_geodesic(xyz, parent, thr=128, step=step), w, xyz, parent, ("hidden", step))
    # one tree all of whose sources are hidden
    xyz2, parent2 = xyz[[0, 1, 4, 3]], np.array([-1, 0, -1, -1], np.int32)
    w = solved(V, xyz2, parent2, 2.0, thr=128)
    assert w[2]["n_trees_lost"] == 1 and w[2]["n_trees_in"] == 3
    same(ctx.join_trees_geodesic(xyz2, parent2, thr=128), w, xyz2, parent2, "one lost")


@pytest.mark.parametrize("kind", ["const", "open"])
def test_meet_pairs_across_a_tile_face_edge_and_corner(ctxs, kind):
    """two one-node trees symmetrically about a tile face, edge and corner: the meet pair (p, q) straddles it"""
    shape = TWO
    V = image(shape, kind)
    for zd in ZDS:
        ctxs[zd].set_volume(V)
        for a, b in (((TX - 1, 3, 1), (TX, 3, 1)), ((TX - 1, TY - 1, 2), (TX, TY, 2)), ((TX - 1, TY - 1, TZ - 1), (TX, TY, TZ)), ((TX - 2, TY - 2, TZ - 2), (TX + 1, TY + 1, TZ + 1)),
                     ((TX, TY - 1, TZ - 1), (TX - 1, TY, TZ)), ((5, TY - 1, 0), (5, TY, 0)), ((7, 2, TZ - 1), (7, 2, TZ))):
            xyz, parent = np.array([a, b], np.float32), np.array([-1, -1], np.int32)
            w = solved(V, xyz, parent, zd)
            assert len(w[0]) == 1
            same(ctxs[zd].join_trees_geodesic(xyz, parent), w, xyz, parent, (kind, zd, a, b))


@pytest.mark.parametrize("shape,kind,trees,zd", [(MID, "open", 40, 1.0), (TWO, "const", 40, 2.0), (MID, "rand50", 40, 3.3)], ids=str)
def test_limit(ctxs, shape, kind, trees, zd):
    """the limit from the reference: the median bridge W of the unlimited run keeps at least one bridge and drops at least one"""
    full = want(shape, kind, trees, zd)[0]
    limit = int(np.sort(full["w"])[len(full) // 2])
    w = want(shape, kind, trees, zd, limit)
    assert 1 <= len(w[0]) < len(full) and w[2]["w_max"] <= limit and w[0].tobytes() == full[full["w"] <= limit].tobytes()
    ctxs[zd].set_volume(image(shape, kind))
    xyz, parent = forest(shape, kind, trees)
    same(run(ctxs[zd], shape, kind, trees, zd, limit), w, xyz, parent, (shape, kind, limit))
    if limit > 2**31:  # (not reached on these stacks; the 64-bit test has such a limit)
        return
    # a limit below every meet edge: nothing is bridged, in one round
    got = ctxs[zd].join_trees_geodesic(xyz, parent, limit=1, thr=THR.get(kind, 128))
    assert len(got[0]) == 0 and len(got[1]["vox"]) == 0 and got[2]["n_bridges"] == 0 and got[2]["n_trees_out"] == got[2]["n_trees_in"] and got[2]["rounds"] == 1


def test_a_bridge_weight_above_32_bits(ctx):
    """a stack of two rows (a context takes no thinner one), every voxel at the cost 65535 (one value at the cost 1 is kept for tuning, and is not
    needed): two one-node trees 1025 steps apart along a row meet in the middle, each side 512 steps = 2147450880 <= dmax = 2^31 - 1, so
    W = 1025 * 4194240 = 4299096000 > 2^32 - 1"""
    n = 1026
    V = np.full((1, 2, n), 200, np.uint8)
    cost = np.full(256, 65535, np.uint16)
    cost[7] = 1
    xyz, parent = np.array([[0, 0, 0], [n - 1, 0, 0]], np.float32), np.array([-1, -1], np.int32)
    w = solved(V, xyz, parent, 2.0, cost=cost)
    assert len(w[0]) == 1 and int(w[0]["w"][0]) == 1025 * 32 * 2 * 65535 > 2**32 - 1 and w[2]["w_max"] > 2**32 - 1 and w[0]["path_len"][0] == n
    ctx.set_volume(V)
    same(ctx.join_trees_geodesic(xyz, parent, cost=cost), w, xyz, parent, "64-bit W")
    for limit, k in ((int(w[0]["w"][0]), 1), (int(w[0]["w"][0]) - 1, 0)):  # a limit above 2^31 - 1: dmax stays 2^31 - 1, the edge test is 64-bit
        got = ctx.join_trees_geodesic(xyz, parent, limit=limit, cost=cost)
        assert len(got[0]) == k and (k == 0 or got[0].tobytes() == w[0].astype(lib.GEO_BRIDGE).tobytes())


@pytest.mark.parametrize("shape,kind,trees,zd", [(TWO, "const", 5, 2.0), (MID, "open", 40, 1.0), (MID, "rand50", 40, 3.3)], ids=str)
def test_launch_cuts_change_no_bit(ctxs, shape, kind, trees, zd):
    c = ctxs[zd]
    c.set_volume(image(shape, kind))
    xyz, parent = forest(shape, kind, trees)
    try:
        for per in (1, 3):
            c.set_option("geojoin_tiles_per_launch", per)
            same(run(c, shape, kind, trees, zd), want(shape, kind, trees, zd), xyz, parent, (shape, kind, per))
    finally:
        c.set_option("geojoin_tiles_per_launch", 0)


def test_no_side_effects_stream_timers_and_live_bytes(ctx):
    import torch
    shape, kind, trees, zd = MID, "rand50", 40, 2.0
    V = image(shape, kind)
    xyz, parent = forest(shape, kind, trees)
    ctx.set_volume(V)
    src = np.array([[3, 3, 1], [100, 50, 3]], np.float32)
    before = ctx.geodesic(src, thr=128)
    live, pinned, after, pinned2 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    lib.load().pnr_live_bytes(C.byref(live), C.byref(pinned))
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("geojoin") == (0.0, 0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    got = ctx.join_trees_geodesic(xyz, parent, thr=128)
    ctx.set_stream(None)
    ctx.set_profiling(False)
    same(got, want(shape, kind, trees, zd), xyz, parent, "stream")
    rounds = got[2]["rounds"]
    (ms, launches), (mw, lw), (me, le) = (ctx.kernel_ms(g) for g in ("geojoin", "geojoin_meet_w", "geojoin_meet_e"))
    assert rounds >= 2 and mw > 0 and me > 0 and lw == le == rounds and launches == 2 * rounds and abs(ms - (mw + me)) < 1e-9, (rounds, mw, me, lw, le)
    assert ctx.kernel_ms("geodesic_relax")[0] > 0  # the relaxation keeps counting under "geodesic"
    lib.load().pnr_live_bytes(C.byref(after), C.byref(pinned2))
    assert after.value == live.value and pinned2.value == pinned.value  # every buffer of the call is freed
    assert np.array_equal(ctx.get_volume(), V)
    again = ctx.geodesic(src, thr=128)
    assert again[0] == before[0] and np.array_equal(again[1], before[1]) and np.array_equal(again[2], before[2])
    # a borrowed device volume is not written and stays borrowed
    flat = torch.from_numpy(np.concatenate([np.full(3, 99, np.uint8), V.ravel(), np.full(7, 99, np.uint8)])).cuda()
    keep = flat.clone()
    torch.cuda.synchronize()
    ctx.set_volume_device(flat.data_ptr() + 3, shape, keepalive=flat)
    same(ctx.join_trees_geodesic(xyz, parent, thr=128), want(shape, kind, trees, zd), xyz, parent, "borrowed")
    torch.cuda.synchronize()
    assert ctx._keep is flat and torch.equal(flat, keep)


def test_pipeline_state_survives():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30), 0)
    V = np.clip(synth.synth(64, 64, 32, seed=2, zdist=2.0).astype(np.int32) + 20, 0, 255).astype(np.uint8)
    c.set_volume(V)
    c.frangi()
    seeds_ = c.extract_seeds()
    assert len(seeds_) > 0
    c.frangi()
    xyz = np.array([[10, 10, 5], [14, 12, 6], [50, 40, 20], [30, 60, 12]], np.float32)
    parent = np.array([-1, 0, -1, -1], np.int32)
    got = c.join_trees_geodesic(xyz, parent, thr=-1)
    assert c.extract_seeds().tobytes() == seeds_.tobytes()
    w = solved(V, xyz, parent, 2.0, thr=-1)
    assert w[2]["thr_used"] == max(1, int(V.astype(np.uint64).sum()) // V.size)
    same(got, w, xyz, parent, "pipeline")
    c.close()


def test_argument_and_state_errors_and_the_count_convention(ctx):
    L = lib.load()
    shape, kind = MORE, "open"
    V = image(shape, kind)
    xyz, parent = forest(shape, kind, 5)
    wb, wvox, winfo, _ = want(shape, kind, 5, 2.0)
    nb, npath = C.c_int64(), C.c_int64()

    def call(h, x=xyz, p=parent, n=len(xyz), opts=None, bridges=None, cap_b=0, vox=None, cap_p=0, counts=True):
        q = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        return L.pnr_geodesic_bridges(h, q(x), q(p), n, C.byref(opts) if opts is not None else None, None, q(bridges), cap_b, C.byref(nb) if counts else None, q(vox), cap_p,
                                      C.byref(npath) if counts else None)

    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    assert call(fresh.h) == -4 and b"no volume" in L.pnr_last_error()
    assert call(fresh.h, opts=lib.GeoJoinOpts(-2, 0, 1.0, None)) == -1  # arguments are checked first
    fresh.close()
    ctx.set_volume(V)
    # the counts come back with no room at all, and with too little room the first entries are written
    assert call(ctx.h) == 0 and nb.value == len(wb) and npath.value == len(wvox)  # opts = NULL
    bridges, vox = np.zeros(2, lib.GEO_BRIDGE), np.full(5, -7, np.int64)
    assert call(ctx.h, bridges=bridges, cap_b=2, vox=vox, cap_p=5) == 0 and nb.value == len(wb) > 2 and npath.value == len(wvox) > 5
    assert bridges.tobytes() == wb[:2].astype(lib.GEO_BRIDGE).tobytes() and np.array_equal(vox, wvox[:5])
    zero = np.ones(256, np.uint16)
    zero[77] = 0
    cyc = parent.copy()
    cyc[0] = 1 if parent[1] == 0 else 0
    if parent[1] != 0:
        cyc[0], cyc[1] = 1, 0
    big = parent.copy()
    big[0] = len(xyz)
    nan = xyz.copy()
    nan[1, 2] = np.nan
    for kw in (dict(thr=-2), dict(thr=256), dict(step=-1.0), dict(step=float("nan")), dict(cost=zero), dict(parent=cyc), dict(parent=big), dict(xyz=nan)):
        with pytest.raises(lib.PnrError, match="error -1"):
            ctx.join_trees_geodesic(**{"xyz": xyz, "parent": parent, **kw})
    assert call(ctx.h, n=0) == -1 and call(ctx.h, n=(1 << 22) + 1) == -1 and call(ctx.h, x=None) == -1 and call(ctx.h, p=None) == -1 and call(ctx.h, counts=False) == -1
    assert call(ctx.h, cap_b=2) == -1 and call(ctx.h, cap_p=2) == -1 and call(ctx.h, cap_b=-1) == -1  # room without a buffer
    assert call(None) == -1
    same(ctx.join_trees_geodesic(xyz, parent), want(shape, kind, 5, 2.0), xyz, parent, "usable after the errors")
    # a single tree: nothing to join, no round
    one = ctx.join_trees_geodesic(xyz[:1], parent[:1])
    assert len(one[0]) == 0 and one[2]["n_trees_in"] == one[2]["n_trees_out"] == 1 and one[2]["rounds"] == 0 and ctx.get_option("geojoin_rounds") == 0


# ---- the CLI ----
def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def test_cli_join_swc_geodesic_and_an_unchanged_tracing_run(tmp_path):
    l, h, w = MID
    V = volume(MID, "open")
    tif, a, out = str(tmp_path / "s.tif"), tmp_path / "a.swc", tmp_path / "o.swc"
    lib.write_tiff(tif, V)
    # three fragments: (1, 2), (4, 9, 5) with a soma-typed node, (7)
    a.write_text("# fragments\n1 3 10 10 1 3 -1\n2 3 30.4 20.5 2.2 2.5 1\n4 1 120 60 4 1.5 -1\n9 2 100 50 3 1.25 4\n5 2 112 11 3 1 9\n7 4 60 5 0 0.75 -1\n")
    xyz, radius, types, parent, ids = pnr_amd.read_swc_nodes(a)
    n = len(xyz)
    for zd, limit, thr, extra in ((1.0, 0, 0, []), (2.0, 0, -1, ["--join-keep-largest"]), (3.3, None, 0, ["--join-root", "9"])):
        full = ref.solve(V, xyz, parent, zd, thr=thr)
        if limit is None:  # the median bridge: one bridge is made, one is not
            limit = int(np.sort(full[0]["w"])[0])
        bridges, vox, winfo, _ = ref.solve(V, xyz, parent, zd, limit=limit, thr=thr)
        assert len(bridges) == (2 if extra != ["--join-root", "9"] else 1)
        xyz2, parent2, of, join = ref.expand(xyz, parent, bridges, vox, MID)
        root = list(ids).index(9) if "--join-root" in extra else -1
        po, order, comp, trees_out = join_ref.reroot(parent2, join, root)
        flags = (["--zscale", str(zd)] if zd != 1.0 else []) + (["--join-threshold", str(thr)] if thr else []) + extra
        r = _cli("--join-swc", str(a), str(out), "--join-geodesic", str(limit), "-i", tif, *flags)
        assert r.returncode == 0, r.stderr[-1500:]
        got = json.loads(r.stdout)
        lines, pos = [], {}
        for v in order:
            if "--join-keep-largest" in extra and comp[v] != 0:
                break
            pos[v] = len(lines) + 1
            b = bridges[of[v - n]] if v >= n else None
            typ = types[b["a"]] if b is not None else types[v]
            rad = min(radius[b["a"]], radius[b["b"]]) if b is not None else radius[v]
            lines.append((pos[v], int(typ), float(xyz2[v, 0]), float(xyz2[v, 1]), float(xyz2[v, 2]), float(rad), pos[po[v]] if po[v] >= 0 else -1))
        assert got.pop("rounds") >= 2 and got == dict(nodes=len(lines), n_trees_in=winfo["n_trees_in"], n_trees_lost=winfo["n_trees_lost"], n_trees_out=winfo["n_trees_out"],
                                                      n_bridges=winfo["n_bridges"], n_inserted=winfo["n_inserted"], w_max=winfo["w_max"], thr_used=winfo["thr_used"],
                                                      n_src=winfo["n_src"], n_src_dropped=winfo["n_src_dropped"], limit=limit, zdist=float(np.float32(zd))), (got, winfo)
        text = out.read_text().split("\n")
        assert text[0] == "#join=geodesic:%d,thr:%d,bridges:%d,trees:%d->%d,inserted:%d" % (limit, winfo["thr_used"], len(bridges), 3, 3 - len(bridges), winfo["n_inserted"])
        assert text[1] == "##n,type,x,y,z,radius,parent" and text[-1] == ""
        rows = [ln.split() for ln in text[2:-1]]
        assert [(int(f[0]), int(f[1])) + tuple(float(np.float32(v)) for v in f[2:6]) + (int(f[6]),) for f in rows] == lines
        assert all(int(f[6]) < int(f[0]) for f in rows) and [int(f[0]) for f in rows] == list(range(1, len(rows) + 1))  # every parent precedes its children
        assert np.array_equal(np.array([[np.float32(f[2]), np.float32(f[3]), np.float32(f[4])] for f in rows], np.float32), xyz2[[v for v in order if v in pos]])
    # usage errors: both joins at once; the tool mode without a stack; a threshold without the flag
    assert _cli("--join-swc", str(a), str(out), "--join-geodesic", "0", "--join", "3", "-i", tif).returncode == 1
    assert _cli("--join-swc", str(a), str(out), "--join-geodesic", "0").returncode == 1
    assert _cli("--join-swc", str(a), str(out), "--join-threshold", "3").returncode == 1
    assert _cli("--join-swc", str(a), str(out), "--join-geodesic", "-4", "-i", tif).returncode == 1
    help_ = _cli("--help").stdout
    assert "--join-geodesic D" in help_ and "--join-swc IN.swc OUT.swc --join-geodesic D -i stack" in help_


def test_cli_tracing_run_with_and_without_the_flag(tmp_path):
    """the forest the plain run writes, joined by the reference, is the file the run with --join-geodesic writes; without the flag the comment
    block is the one of before"""
    from test_gpu_join import PARAS, PLAIN_COMMENT, read_lines, two_fragment_stack
    img = two_fragment_stack()
    outs = {}
    for name, flags in (("plain", []), ("geo", ["--join-geodesic", "0"]), ("cut", ["--join-geodesic", "1", "--join-threshold", "-1"])):
        tif = str(tmp_path / (name + ".tif"))
        lib.write_tiff(tif, img)
        r = _cli(*flags, "-f", "advantra_func", "-i", tif, "-p", *PARAS)
        assert r.returncode == 0, r.stderr[-1500:]
        outs[name] = tif + "_Advantra.swc"
    c0, rows0 = read_lines(outs["plain"])
    assert PLAIN_COMMENT in "\n".join(c0) and not [ln for ln in c0 if "join" in ln]
    xyz, radius, types, parent, ids = pnr_amd.read_swc_nodes(outs["plain"])
    n = len(xyz)
    assert (parent < 0).sum() >= 2
    bridges, vox, winfo, _ = ref.solve(img, xyz, parent, 2.0)
    assert len(bridges) >= 1 and winfo["n_inserted"] > 0
    xyz2, parent2, of, join = ref.expand(xyz, parent, bridges, vox, img.shape)
    po, order, comp, trees_out = join_ref.reroot(parent2, join, -1)
    c1, rows1 = read_lines(outs["geo"])
    # with the flag the comment block gains one line, after the parameters
    assert [ln for ln in c1 if ln not in c0] == ["#join=geodesic:0,thr:0,bridges:%d,trees:%d->%d,inserted:%d" % (len(bridges), winfo["n_trees_in"], trees_out, winfo["n_inserted"])]
    assert [ln for ln in c1 if ln in c0] == c0
    pos = {int(v): k + 1 for k, v in enumerate(order)}
    lines = []
    for v in order:
        b = bridges[of[v - n]] if v >= n else None
        typ = types[b["a"]] if b is not None else types[v]
        rad = min(radius[b["a"]], radius[b["b"]]) if b is not None else radius[v]
        lines.append((pos[int(v)], int(typ), float(xyz2[v, 0]), float(xyz2[v, 1]), float(xyz2[v, 2]), float(rad), pos[int(po[v])] if po[v] >= 0 else -1))
    assert [(int(f[0]), int(f[1])) + tuple(float(np.float32(v)) for v in f[2:6]) + (int(f[6]),) for f in rows1] == lines
    assert all(int(f[6]) < int(f[0]) for f in rows1)  # every parent precedes its children
    # a limit below every edge: the forest as it was, in tree order, under its own comment line
    c2, rows2 = read_lines(outs["cut"])
    thr = max(1, int(img.astype(np.uint64).sum()) // img.size)
    assert [ln for ln in c2 if ln not in c0] == ["#join=geodesic:1,thr:%d,bridges:0,trees:%d->%d,inserted:0" % (thr, winfo["n_trees_in"], winfo["n_trees_in"])] and len(rows2) == n
    # usage: one join or the other
    assert _cli("--join", "0", "--join-geodesic", "0", "-f", "advantra_func", "-i", str(tmp_path / "plain.tif"), "-p", *PARAS).returncode == 1


# ---- voxel indices above 2^31 ----
def _two_blocks(shape):
    """seven fragments, three in the near and four in the far block of a stack that is background elsewhere (bigvol.join_case), borrowed from the
    device -> (the bridges of the far block, the expected info).  The threshold is 100 and the background 0, so there is no passable route
    between the blocks and no meet edge joins them: Kruskal's algorithm over two edge sets that share no tree is the merge by key of
    its runs on the crops (geojoin_ref.solve), their voxels and nodes translated.  The raster order of a crop's voxels is that of their
    absolute indices (both lexicographic in z, y, x), so the tie-break (W, p, o) carries over; the far block is uniform and its fragments
    F1, F2, F3 lie equally far apart, so ties on W decide there.  The fragments of the two blocks alternate in the node order: the tree
    numbers are those of the whole forest."""
    import bigvol
    case = bigvol.join_case(shape)
    bigvol.check_placement(case["blocks"], shape, (TZ, TY, TX))
    wb, wvox, winfo, per_block = bigvol.join_want(case)
    t, c = bigvol.open_stack(case["blocks"], shape)
    try:
        bridges, paths, info = c.join_trees_geodesic(case["xyz"], case["parent"], case["limit"], thr=case["thr"])
    finally:
        c.close()
    assert bridges.dtype == lib.GEO_BRIDGE and bridges.tobytes() == wb.astype(lib.GEO_BRIDGE).tobytes(), (bridges, wb)
    assert paths["vox"].dtype == np.int64 and np.array_equal(paths["vox"], wvox) and paths["shape"] == tuple(shape)
    assert {k: info[k] for k in bigvol.JOIN_INFO} == winfo, (info, winfo)
    assert all(i["n_bridges"] >= 1 for i in per_block) and info["n_trees_in"] == 7 and info["n_trees_out"] == 7 - info["n_bridges"] >= 2
    far = bridges[bridges["p"] >= int(bigvol.index_of(0, 0, shape[0] - 1, shape))]
    assert len(far) >= 2 and len(set(far["w"].tolist())) < len(far), "a tie on W in the far block"
    assert bigvol.untouched(t, case["blocks"])
    return far, winfo


def test_two_blocks_on_a_small_stack():
    """the placement of the case below at 96 x 64 x 41, where test_bigvol_host.py restates the whole stack"""
    import bigvol
    _two_blocks(bigvol.SMALL)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31): the edge key (13 p + (o - 13)) << 22 with 13 p above 2^32, unpacked by the host with e / 13, on top
    of the geodesic flood's u64 keys; the far block is the last plane, in the one-plane partial tile"""
    import bigvol
    far, winfo = _two_blocks(bigvol.SHAPE)
    assert all(13 * int(p) > 2**32 and int(p) > 2**31 for p in far["p"])
    assert bigvol.check_placement(bigvol.join_case(bigvol.SHAPE)["blocks"], bigvol.SHAPE, (TZ, TY, TX)) > 2**31
