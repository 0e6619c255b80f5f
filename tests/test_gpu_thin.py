"""GPU: pnr_skeletonize against the numpy restatement of the rule (thin_ref.py) -- the 0 / 255 volume, the voxel list, the degrees and
every info field but tile_visits, bit for bit -- on the shapes and kinds at which the tiling can go wrong; the shrinking work per round;
and advantra_cli --skeleton --swc on a synthetic tube stack."""
import ctypes as C
import functools
import json
import os
import subprocess
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import thin_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
TX, TY, TZ = ref.tile()
THR = ref.THR
# (l, h, w): degenerate and odd extents, then one tile, one tile plus a voxel, two tiles minus a voxel and two tiles in every axis
SHAPES = ((1, 2, 2), (2, 2, 2), (3, 3, 3), (1, 21, 33), (70, 2, 2), (2, 2, 300), (5, 67, 131), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1), (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1),
          (2 * TZ, 2 * TY, 2 * TX))


def tiles_of(shape):
    l, h, w = shape
    return -(-w // TX) * -(-h // TY) * -(-l // TZ)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, thr):
    """the volume and the object after every round of the rule: computed once, shared by the tests, never written"""
    V = ref.volume(shape, kind)
    history = []
    ref.thin(V >= ref.threshold(V, thr), history=history)
    V.setflags(write=False)
    for a in history:
        a.setflags(write=False)
    return V, tuple(history)


def want(shape, kind, thr, max_rounds):
    V, history = reference(shape, kind, thr)
    return ref.skeletonize(V, thr, max_rounds, history=history)


def same(got, exp, tag):
    info, skel, vox, deg = got
    winfo, wskel, wvox, wdeg = exp
    for k, v in winfo.items():
        assert info[k] == v, (tag, k, info, winfo)
    assert np.array_equal(skel, wskel), tag
    assert vox.dtype == np.int64 and np.array_equal(vox, wvox), tag
    assert deg.dtype == np.uint8 and np.array_equal(deg, wdeg), tag


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2.0, np_=20), 0)
    yield c
    c.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_kind_equals_the_rule(ctx, shape):
    for kind in ref.KINDS:
        ctx.set_volume(reference(shape, kind, THR)[0])
        for max_rounds in (0, 1, 2):
            got = ctx.skeletonize(THR, max_rounds)
            same(got, want(shape, kind, THR, max_rounds), (shape, kind, max_rounds))
            assert got[0]["tiles"] == tiles_of(shape) and got[0]["tile_visits"] >= 8 * tiles_of(shape)


def test_mean_threshold_equals_the_rule(ctx):
    """thr = -1: every shape with one kind, every kind at least once"""
    for i, shape in enumerate(SHAPES + ((2 * TZ, 2 * TY, 2 * TX),)):
        kind = ref.KINDS[i % len(ref.KINDS)]
        V = reference(shape, kind, -1)[0]
        ctx.set_volume(V)
        for max_rounds in (0, 1, 2):
            got = ctx.skeletonize(-1, max_rounds)
            same(got, want(shape, kind, -1, max_rounds), (shape, kind, max_rounds))
            assert got[0]["thr_used"] == max(1, int(V.sum(dtype=np.uint64)) // V.size)


# N = 4095, 4096, 4097, 8192, 8193 and 4095 voxels: the ends of the 4096-voxel chunks of the voxel list
CHUNK_SHAPES = ((1, 3, 1365), (1, 2, 2048), (1, 17, 241), (1, 2, 4096), (1, 3, 2731), (3, 5, 273))


@pytest.mark.parametrize("shape", CHUNK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lattice_of_isolated_voxels_at_the_chunk_ends(ctx, shape):
    """every second voxel of every axis: nothing is deleted, and the list meets every wave quarter, lane and k of the compaction"""
    z, y, x = np.indices(shape)
    V = np.where((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0), 200, 0).astype(np.uint8)
    ctx.set_volume(V)
    got = ctx.skeletonize(1)
    same(got, ref.skeletonize(V, 1), shape)
    info, skel, vox, deg = got
    assert np.array_equal(vox, np.flatnonzero(skel)) and len(vox) == np.count_nonzero(V)
    assert not deg.any()


def test_a_larger_stack_of_blobs(ctx):
    shape = (33, 65, 129)
    ctx.set_volume(reference(shape, "blobs", THR)[0])
    got = ctx.skeletonize(THR)
    same(got, want(shape, "blobs", THR, 0), shape)
    assert got[0]["rounds"] > 3 and got[0]["tile_visits"] < 8 * got[0]["rounds"] * got[0]["tiles"]


def test_cap_outputs_borrowed_volume_and_live_bytes(ctx):
    import torch
    shape, kind = (5, 67, 131), "rand31"
    exp = want(shape, kind, THR, 0)
    n = exp[0]["n_skel"]
    assert n > 10
    V = reference(shape, kind, THR)[0]
    for shift in (0, 1, 3):  # a borrowed device volume, also one that is not aligned: read, never written
        flat = torch.from_numpy(np.concatenate([np.full(shift, 99, np.uint8), V.ravel(), np.full(7, 99, np.uint8)])).cuda()
        before = flat.clone()
        torch.cuda.synchronize()
        ctx.set_volume_device(flat.data_ptr() + shift, shape, keepalive=flat)
        same(ctx.skeletonize(THR), exp, ("borrowed", shift))
        same(ctx.skeletonize(-1), want(shape, kind, -1, 0), ("borrowed, mean", shift))
        torch.cuda.synchronize()
        assert torch.equal(flat, before) and ctx._keep is flat
    ctx.set_volume(V)
    info, skel, vox, deg = ctx.skeletonize(THR, cap=7)  # the prefix, and the full count
    assert info["n_skel"] == n and np.array_equal(vox, exp[2][:7]) and np.array_equal(deg, exp[3][:7]) and np.array_equal(skel, exp[1])
    info, skel, vox, deg = ctx.skeletonize(THR, cap=n + 5)
    assert len(vox) == len(deg) == n and np.array_equal(vox, exp[2])
    info, skel, vox, deg = ctx.skeletonize(THR, voxels=False)
    assert vox is None and deg is None and np.array_equal(skel, exp[1]) and info["n_end"] == exp[0]["n_end"]
    info, skel, vox, deg = ctx.skeletonize(THR, volume=False)
    assert skel is None and np.array_equal(vox, exp[2])
    assert np.array_equal(ctx.get_volume(), V)  # the context's own volume is as it was
    live, pinned, after = C.c_int64(), C.c_int64(), C.c_int64()
    lib.load().pnr_live_bytes(C.byref(live), C.byref(pinned))
    ctx.skeletonize(THR)
    lib.load().pnr_live_bytes(C.byref(after), C.byref(pinned))
    assert after.value == live.value  # every device buffer of the call is freed


def test_argument_errors_and_kernel_times(ctx):
    L = lib.load()
    ctx.set_volume(reference((3, 3, 3), "rand31", THR)[0])
    for kw in (dict(thr=-2), dict(thr=256), dict(max_rounds=-1), dict(cap=-1)):
        with pytest.raises(lib.PnrError, match="error -1"):
            ctx.skeletonize(**kw)
    assert L.pnr_skeletonize(None, None, None, None, None, None, 0) == -1
    assert L.pnr_skeletonize(ctx.h, None, None, None, None, None, 0) == 0  # NULL options are the defaults; every output is optional
    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=2.0), 0)
    info = lib.ThinInfo()
    assert L.pnr_skeletonize(fresh.h, None, C.byref(info), None, None, None, 0) == -4  # PNR_E_STATE: no volume
    fresh.close()
    shape = (5, 67, 131)
    ctx.set_volume(reference(shape, "rand60", THR)[0])
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("thin") == (0.0, 0)
    got = ctx.skeletonize(-1, cap=10**6)  # (one call: without a cap the wrapper counts first)
    ctx.set_profiling(False)
    same(got, want(shape, "rand60", -1, 0), "profiled")
    ms, launches = ctx.kernel_ms("thin")
    parts = [ctx.kernel_ms("thin_" + p) for p in ("threshold", "init", "mark", "pass", "list", "finish")]
    assert ms > 0 and all(p[0] > 0 and p[1] >= 1 for p in parts), (ms, launches, parts)
    assert abs(ms - sum(p[0] for p in parts)) < 1e-9 and launches == sum(p[1] for p in parts)
    rounds = got[0]["rounds"]
    assert parts[2][1] == rounds and parts[3][1] == 8 * rounds + 8 * (rounds - 1)  # a mark per round; a pass per subfield, a plan in front from round 2 on


def ball_and_lines():
    """one radius-10 ball and one-voxel lines far from it: the lines delete nothing, so only the ball's tiles stay live"""
    shape = (48, 64, 160)
    centre, r = (24, 32, 40), 10
    o = ref.ball(shape, centre, r)
    o[4, 4, 100:150] = True
    o[40, 10:60, 140] = True
    o[2:46, 60, 120] = True
    for k in range(30):
        o[8 + k, 12 + k, 100 + k] = True
    lo = [(c - r) // t - 1 for c, t in zip(centre, (TZ, TY, TX))]
    hi = [(c + r) // t + 1 for c, t in zip(centre, (TZ, TY, TX))]
    n = [-(-e // t) for e, t in zip(shape, (TZ, TY, TX))]
    B = int(np.prod([min(h, m - 1) - max(l, 0) + 1 for l, h, m in zip(lo, hi, n)]))
    return np.where(o, 200, 0).astype(np.uint8), B


def test_the_work_per_round_shrinks_to_the_live_tiles(ctx):
    V, B = ball_and_lines()
    ctx.set_volume(V)
    info, skel, vox, deg = ctx.skeletonize(THR)
    winfo, wskel, wvox, wdeg = ref.skeletonize(V, THR)
    same((info, skel, vox, deg), (winfo, wskel, wvox, wdeg), "ball")
    tiles, rounds = info["tiles"], info["rounds"]
    assert tiles == tiles_of(V.shape) and B < tiles and rounds >= 5
    assert skel[4, 4, 100:150].all() and skel[40, 10:60, 140].all()  # the lines are as they were
    assert info["tile_visits"] <= 8 * tiles + 8 * (rounds - 1) * B, (info, B)
    assert ctx.skeletonize(THR, volume=False, voxels=False)[0]["tile_visits"] == info["tile_visits"]  # decided from completed passes only


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_cli_skeleton_swc(ctx, tmp_path):
    """--skeleton --swc on a tube stack: the JSON line is the info, the SWC's nodes are vox, parents come first, the radii are those of
    --edt --at at the same points, and the comment block ends in #skeleton="""
    shape = (12, 40, 72)
    l, h, w = shape
    V = ref.volume(shape, "tubes")
    raw, swc, vol, csv = (str(tmp_path / n) for n in ("t.raw", "t.swc", "t_skel.raw", "t.csv"))
    V.tofile(raw)
    dims = f"{w},{h},{l}"
    r = run("--skeleton", "-i", raw, "-d", dims, "--threshold", str(THR), "--zscale", "2", "--swc", swc, "--skeleton-out", vol)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    ctx.set_volume(V)
    info, skel, vox, deg = ctx.skeletonize(THR)
    same((info, skel, vox, deg), ref.skeletonize(V, THR), "cli volume")
    line = json.loads(r.stdout)
    from scipy import ndimage
    trees = ndimage.label(skel, np.ones((3, 3, 3), int))[1]
    assert line == {**info, "trees": trees} and info["n_skel"] > 20
    assert np.array_equal(np.fromfile(vol, np.uint8).reshape(shape), skel)
    rows = [ln.split() for ln in open(swc) if not ln.startswith("#")]
    ids, par = [int(f[0]) for f in rows], [int(f[6]) for f in rows]
    xyz = np.array([[float(v) for v in f[2:5]] for f in rows])
    assert ids == list(range(1, len(vox) + 1)) and all(f[1] == "2" for f in rows)
    assert np.array_equal(np.sort((xyz[:, 0] + w * (xyz[:, 1] + h * xyz[:, 2])).astype(np.int64)), vox)
    assert all(p == -1 or 1 <= p < i for i, p in zip(ids, par)) and par.count(-1) == trees  # parents before children, one root per tree
    for i, p in zip(ids, par):  # a link joins 26-neighbours
        assert p == -1 or np.abs(xyz[i - 1] - xyz[p - 1]).max() == 1
    comments = [ln.rstrip("\n") for ln in open(swc) if ln.startswith("#")]
    assert comments[-1] == f"#skeleton=thr:{THR},rounds:{info['rounds']},voxels:{len(vox)},trees:{trees}"
    e = run("--edt", "-i", raw, "-d", dims, "--threshold", str(THR), "--zscale", "2", "--at", swc, "--per-node", csv)
    assert e.returncode == 0, e.stderr
    radii = [ln.strip().split(",") for ln in open(csv)][1:]
    assert [int(a) for a, _ in radii] == ids
    assert np.array_equal(np.array([f[5] for f in rows], np.float32), np.array([b for _, b in radii], np.float32))
    at = np.array([f[5] for f in rows], np.float32)
    assert par[0] == -1 and at[0] == at.max()  # the first root is the thickest skeleton voxel


# ---- voxel indices above 2^31 ----
def _two_blocks(shape):
    """two thick objects in a stack that is background elsewhere (bigvol.thin_case), borrowed from the device -> (the smallest index of the far
    block, info, vox).  Outside the volume is background under the rule, so each block thins like the crop around it on its own, and
    the crops start at even coordinates, so their voxels keep their subfields: vox and deg are the crops' lists translated and merged
    in ascending order, the counts their sums, the rounds those of the slowest block."""
    import bigvol
    case = bigvol.thin_case(shape)
    first = bigvol.check_placement(case["blocks"], shape, (TZ, TY, TX))
    winfo, wvox, wdeg = bigvol.thin_want(case)
    t, c = bigvol.open_stack(case["blocks"], shape)
    try:
        info, skel, vox, deg = c.skeletonize(case["thr"], volume=False, voxels=True)
    finally:
        c.close()
    assert skel is None
    for k, v in winfo.items():
        assert info[k] == v, (k, info, winfo)
    assert vox.dtype == np.int64 and np.array_equal(vox, wvox), (len(vox), len(wvox), vox[:4], wvox[:4])
    assert deg.dtype == np.uint8 and np.array_equal(deg, wdeg)
    assert info["tiles"] == tiles_of(shape) and info["rounds"] >= 3 and info["tile_visits"] >= 8 * info["tiles"]
    assert bigvol.untouched(t, case["blocks"])
    return first, info, vox


def test_two_blocks_on_a_small_stack():
    """the placement of the case below at 96 x 64 x 41, where test_bigvol_host.py restates the whole stack"""
    import bigvol
    _two_blocks(bigvol.SMALL)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31): 64-bit voxel arithmetic in thin_mark and thin_pass, voxel indices above the sign bit in thin_list,
    x, y, z recovered from them; the far block is the last plane, in the one-plane partial tile, and holds the stack's last voxel"""
    import bigvol
    l, h, w = bigvol.SHAPE
    first, info, vox = _two_blocks(bigvol.SHAPE)
    assert first > 2**31 and vox.max() > 2**31 and info["n_vox"] == l * h * w and (vox > 2**31).sum() > 5
    assert info["tile_visits"] < 9 * info["tiles"]  # after round 1 only the tiles around the blocks are visited
