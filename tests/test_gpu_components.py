"""Connected components on the GPU (pnr_label_components, pnr_despeckle_volume, Context.label_components / despeckle, advantra_cli
--components / --despeckle) against the rule of include/pnr_hip.h restated in numpy (components_ref.py).  The rule is integer-exact:
every comparison is array_equal, there is no tolerance.

The context holds volumes of at least 2 x 2 x 1 voxels (pnr_set_volume, pinned by test_gpu_volume16.py), so the 1 x 1 x 1 stack of the
shape list cannot be handed to the library: for that shape the test checks the restatement and that the context refuses the volume."""
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
import components_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")


def _tile_constants():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "components.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (CC_TX|CC_TY|CC_TZ) = (\d+);", txt)}


TILE = _tile_constants()
TX, TY, TZ = TILE["CC_TX"], TILE["CC_TY"], TILE["CC_TZ"]
# (l, h, w): the smallest stacks, a 2-D one, long thin ones, odd sizes over several tiles, exactly one tile, one voxel more than a
# tile, one voxel less than two tiles, exactly two tiles in every axis
SHAPES = [(1, 1, 1), (1, 2, 2), (2, 2, 2), (3, 3, 3), (1, 21, 33), (70, 2, 2), (2, 2, 300), (5, 67, 131), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1),
          (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1), (2 * TZ, 2 * TY, 2 * TX)]
BIG = (33, 129, 257)
KINDS = ("zero", "full", "rand05", "rand10", "rand31", "rand60", "checker", "diagonal", "serpentine", "comb", "faces")
THR = 128


def sid(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    l, h, w = shape
    rng = np.random.default_rng(abs(hash((shape, KINDS.index(kind)))) % 2**32)
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    if kind == "zero":
        return _ro(np.zeros(shape, np.uint8))
    if kind == "full":
        return _ro(np.full(shape, 255, np.uint8))
    if kind.startswith("rand"):  # near the percolation thresholds of the two connectivities (0.10 / 0.31), below and above
        F = rng.random(shape) < int(kind[4:]) / 100
    elif kind == "checker":  # N / 2 singletons at 6, one component at 26
        F = ((x + y + z) & 1) == 0
    elif kind == "diagonal":  # joined through tile corners only
        F = (x == y) & (y == z)
    elif kind == "serpentine":  # a one-voxel path through every second row of every second slice, joined at alternating ends
        F = ((y & 1) == 0) & ((z & 1) == 0)
        F |= ((y & 1) == 1) & ((z & 1) == 0) & (y + 1 < h) & (x == np.where(((y >> 1) & 1) == 0, w - 1, 0))
        ylast = 2 * ((h + 1) // 2 - 1)  # consecutive even slices are joined at x = 0 of their last or of their first row in turn
        F |= ((z & 1) == 1) & (z + 1 < l) & (x == 0) & (y == np.where(((z >> 1) & 1) == 0, ylast, 0))
    elif kind == "comb":  # pillars along z that meet only in the last slice, along its last row
        F = ((x & 1) == 0) & ((y & 1) == 0)
        F |= (z == l - 1) & ((x & 1) == 0)
        F |= (z == l - 1) & (y == h - 1)
    else:  # voxels on tile faces only
        F = ((x % TX == 0) | (x % TX == TX - 1) | (y % TY == 0) | (y % TY == TY - 1) | (z % TZ == 0) | (z % TZ == TZ - 1)) & (rng.random(shape) < 0.5)
    V = np.where(F, rng.integers(THR, 256, shape), rng.integers(0, THR, shape)).astype(np.uint8)
    return _ro(V)


def _ro(V):
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def want(shape, kind, conn, thr=THR, min_size=1):
    return ref.label(volume(shape, kind), thr, conn, min_size)


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2.0, np_=20), 0)
    yield c
    c.close()


def same(got, wanted, what):
    info, labels, comps = got
    winfo, wlabels, wcomps = wanted
    assert info == winfo, (what, info, winfo)
    assert labels.dtype == np.int32 and np.array_equal(labels, wlabels), (what, int((labels != wlabels).sum()), np.argwhere(labels != wlabels)[:4].tolist())
    assert comps.dtype == ref.COMPONENT_DT and len(comps) == len(wcomps), (what, len(comps), len(wcomps))
    for f in ref.COMPONENT_DT.names:
        assert np.array_equal(comps[f], wcomps[f]), (what, f, comps[f][:8], wcomps[f][:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_labels_components_and_info(ctx, shape, kind):
    V = volume(shape, kind)
    if shape == (1, 1, 1):  # not a volume a context can hold: the restatement alone, and the refusal
        for conn in (6, 26):
            info, labels, comps = ref.label(V, THR, conn)
            assert info["n_comp"] == len(comps) == int(V[0, 0, 0] >= THR) == int(labels[0, 0, 0])
        with pytest.raises(lib.PnrError, match="at least 2x2x1"):
            ctx.set_volume(V)
        return
    ctx.set_volume(V)
    for conn in (6, 26):
        same(ctx.label_components(THR, conn), want(shape, kind, conn), (shape, kind, conn))
    assert np.array_equal(ctx.get_volume(), V)  # never written


# N = 4095, 4096, 4097, 8192, 8193 and 4095 voxels: the ends of the 4096-voxel chunks of the numbering
CHUNK_SHAPES = [(1, 3, 1365), (1, 2, 2048), (1, 17, 241), (1, 2, 4096), (1, 3, 2731), (3, 5, 273)]


@pytest.mark.parametrize("shape", CHUNK_SHAPES, ids=sid)
def test_checkerboard_numbering_at_the_chunk_ends(ctx, shape):
    """every foreground voxel is a 6-component of its own: the numbering is the raster rank, in every wave quarter, lane and k"""
    z, y, x = np.indices(shape)
    V = np.where((x + y + z) % 2 == 0, 200, 0).astype(np.uint8)
    fg = np.flatnonzero(V)
    ctx.set_volume(V)
    info, labels, comps = ctx.label_components(1, 6, 1)
    assert info["n_comp"] == len(comps) == len(fg)
    assert np.array_equal(comps["first"], fg) and (comps["size"] == 1).all()
    wlabels = np.zeros(V.size, np.int32)
    wlabels[fg] = np.arange(1, len(fg) + 1)
    assert np.array_equal(labels, wlabels.reshape(shape))


def test_larger_stack_once(ctx):
    ctx.set_volume(volume(BIG, "rand31"))
    for conn in (6, 26):
        same(ctx.label_components(THR, conn), want(BIG, "rand31", conn), (BIG, conn))


def test_serpentine_and_comb_are_what_they_claim():
    """the inputs themselves: one chain / one comb across many tiles (and many pieces before the last row joins them)"""
    shape = (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1)
    for kind in ("serpentine", "comb"):
        for conn in (6, 26):
            assert want(shape, kind, conn)[0]["n_comp"] == 1, (kind, conn)
    V = volume(shape, "comb").copy()
    V[-1] = 0
    assert ref.label(V, THR, 26)[0]["n_comp"] == TX * TY
    assert want(shape, "checker", 6)[0]["n_comp"] == (int(np.prod(shape)) + 1) // 2 and want(shape, "checker", 26)[0]["n_comp"] == 1
    assert want(shape, "diagonal", 26)[0]["n_comp"] == 1 and want(shape, "diagonal", 6)[0]["n_comp"] == min(shape)


def test_threshold_modes(ctx):
    """thr = -1 on a tube stack: thr_used is the floor of the exact mean; thr = 0: one component of every voxel; an all-zero stack at
    thr = -1 has t = 1 and no foreground"""
    V = synth.synth(48, 40, 24, seed=3)
    ctx.set_volume(V)
    t = max(1, int(V.astype(np.uint64).sum()) // V.size)
    for conn in (6, 26):
        got = ctx.label_components(-1, conn)
        assert got[0]["thr_used"] == t
        same(got, ref.label(V, -1, conn), ("synth", conn))
        assert got[0] == ctx.label_components(connectivity=conn, labels=False)[0]
    info, labels, comps = ctx.label_components(0, 6)
    assert info["n_comp"] == 1 and info["n_fg"] == V.size and (labels == 1).all() and comps["sum"][0] == int(V.astype(np.int64).sum())
    ctx.set_volume(np.zeros((3, 5, 7), np.uint8))
    info, labels, comps = ctx.label_components()
    assert info == dict(n_vox=105, n_fg=0, n_comp=0, n_small=0, vox_small=0, largest=0, thr_used=1) and not labels.any() and len(comps) == 0


@pytest.mark.parametrize("min_size", [2, 5, 100])
def test_min_size_skips_in_the_numbering(ctx, min_size):
    for shape, kind in (((5, 67, 131), "rand10"), ((2 * TZ - 1, 2 * TY - 1, 2 * TX - 1), "rand10"), ((1, 21, 33), "rand31"), ((5, 67, 131), "rand31")):
        ctx.set_volume(volume(shape, kind))
        for conn in (6, 26):
            w = want(shape, kind, conn, THR, min_size)
            same(ctx.label_components(THR, conn, min_size), w, (shape, kind, conn, min_size))
            full = want(shape, kind, conn)[0]
            assert w[0]["n_small"] > 0 and w[0]["n_comp"] + w[0]["n_small"] == full["n_comp"]
            assert w[0]["vox_small"] == full["n_fg"] - int((w[1] > 0).sum())


def test_cap_and_two_calls(ctx):
    shape, kind = (5, 67, 131), "rand10"
    ctx.set_volume(volume(shape, kind))
    winfo, wlabels, wcomps = want(shape, kind, 26)
    assert winfo["n_comp"] > 7
    info, labels, comps = ctx.label_components(THR, 26, cap=7)
    assert info == winfo and len(comps) == 7 and comps.tobytes() == wcomps[:7].tobytes() and np.array_equal(labels, wlabels)
    L = lib.load()
    o, ci = lib.ComponentsOpts(THR, 26, 1), lib.ComponentsInfo()
    buf = np.full(9, -1, ref.COMPONENT_DT)  # exactly cap entries are written
    assert L.pnr_label_components(ctx.h, C.byref(o), C.byref(ci), None, buf.ctypes.data, 7) == 0
    assert ci.n_comp == winfo["n_comp"] and buf[:7].tobytes() == wcomps[:7].tobytes() and (buf["first"][7:] == -1).all()
    assert L.pnr_label_components(ctx.h, C.byref(o), None, None, None, 0) == 0  # every output is optional
    a, b = ctx.label_components(THR, 26, cap=10**6), ctx.label_components(THR, 26, cap=10**6)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() == wcomps.tobytes()


@pytest.mark.parametrize("shape,kind", [((5, 67, 131), "rand10"), ((2 * TZ, 2 * TY, 2 * TX), "rand10"), ((1, 21, 33), "rand31"), ((TZ + 1, TY + 1, TX + 1), "faces")],
                         ids=lambda v: sid(v) if isinstance(v, tuple) else v)
def test_despeckle_owned_volume(ctx, shape, kind):
    V = volume(shape, kind)
    for conn in (6, 26):
        for min_size in (2, 5, 100):
            ctx.set_volume(V)
            info = ctx.despeckle(min_size, THR, conn)
            wv, winfo = ref.despeckle(V, min_size, THR, conn)
            got = ctx.get_volume()
            assert info == winfo and np.array_equal(got, wv), (shape, kind, conn, min_size, int((got != wv).sum()))
            assert (got != V).sum() == winfo["vox_small"]
    ctx.set_volume(V)
    assert ctx.despeckle(1, THR)["n_small"] == 0 and np.array_equal(ctx.get_volume(), V)  # a valid no-op


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_despeckle_never_writes_a_borrowed_volume(ctx, shift):
    import torch
    shape = (5, 67, 131)
    V = volume(shape, "rand10")
    flat = torch.from_numpy(np.concatenate([np.full(shift, 99, np.uint8), V.ravel(), np.full(7, 99, np.uint8)])).cuda()
    before = flat.clone()
    torch.cuda.synchronize()
    ctx.set_volume_device(flat.data_ptr() + shift, shape, keepalive=flat)
    same(ctx.label_components(THR, 26), want(shape, "rand10", 26), "borrowed")
    assert ctx._keep is flat
    ctx.despeckle(1, THR)  # the no-op keeps borrowing
    assert ctx._keep is flat
    info = ctx.despeckle(4, THR, 26)
    torch.cuda.synchronize()
    assert torch.equal(flat, before) and ctx._keep is None
    wv, winfo = ref.despeckle(V, 4, THR, 26)
    assert info == winfo and np.array_equal(ctx.get_volume(), wv)
    flat.zero_()
    torch.cuda.synchronize()
    assert np.array_equal(ctx.get_volume(), wv)


def _noisy_stack():
    img = synth.synth(64, 64, 32, seed=2, zdist=2.0).astype(np.int32)
    return np.clip(img + 20, 0, 255).astype(np.uint8)


def test_pipeline_state():
    """label_components leaves Frangi, seeds and the graph valid; despeckle invalidates them exactly as filter_volume does; a failing
    argument leaves the volume alone"""
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30), 0)
    V = _noisy_stack()
    c.set_volume(V)
    c.frangi()
    seeds = c.extract_seeds()
    nodes, _, _, _ = c.trace_replay(c.score_filter_sort(seeds))
    assert len(seeds) > 0 and len(nodes) > 1
    c.get_graph()
    c.label_components()
    c.get_graph()
    assert c.extract_seeds().tobytes() == seeds.tobytes()
    for kw in (dict(min_size=0), dict(min_size=-3), dict(min_size=2, thr=256), dict(min_size=2, thr=-2), dict(min_size=2, connectivity=18), dict(min_size=2, connectivity=0)):
        with pytest.raises(lib.PnrError, match="error -1"):
            c.despeckle(**kw)
        assert np.array_equal(c.get_volume(), V)
    c.extract_seeds()  # still valid
    c.despeckle(3)
    with pytest.raises(lib.PnrError, match="error -4"):  # PNR_E_STATE: J8 is gone
        c.extract_seeds()
    with pytest.raises(lib.PnrError, match="error -4"):
        c.get_graph()
    c.frangi()
    c.extract_seeds()
    c.close()


def test_argument_and_state_errors(ctx):
    L = lib.load()
    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    o, info = lib.ComponentsOpts(-1, 26, 1), lib.ComponentsInfo()
    assert L.pnr_label_components(fresh.h, C.byref(o), C.byref(info), None, None, 0) == -4 and b"no volume" in L.pnr_last_error()
    assert L.pnr_despeckle_volume(fresh.h, C.byref(o), None) == -4
    bad = lib.ComponentsOpts(-1, 18, 1)
    assert L.pnr_label_components(fresh.h, C.byref(bad), None, None, None, 0) == -1  # arguments are checked first
    assert L.pnr_despeckle_volume(fresh.h, C.byref(bad), None) == -1
    fresh.close()
    ctx.set_volume(volume((3, 3, 3), "rand31"))
    for thr, conn, ms in ((-2, 26, 1), (256, 26, 1), (0, 18, 1), (0, 8, 1), (0, 26, 0), (0, 6, -1)):
        with pytest.raises(lib.PnrError, match="error -1"):
            ctx.label_components(thr, conn, ms)
    assert L.pnr_label_components(None, None, None, None, None, 0) == -1 and L.pnr_despeckle_volume(None, None, None) == -1
    assert L.pnr_label_components(ctx.h, None, None, None, None, -1) == -1  # a negative cap
    assert L.pnr_label_components(ctx.h, None, C.byref(info), None, None, 0) == 0  # opts = NULL = {-1, 26, 1}
    assert info.n_comp == ref.label(volume((3, 3, 3), "rand31"))[0]["n_comp"]
    for thr, conn in ((0, 6), (255, 26)):  # the ends of the ranges are valid
        same(ctx.label_components(thr, conn), ref.label(volume((3, 3, 3), "rand31"), thr, conn), (thr, conn))


def test_kernel_time_group_and_stream(ctx):
    import torch
    ctx.set_volume(volume((5, 67, 131), "rand10"))
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("components") == (0.0, 0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    got = ctx.label_components(-1, 26, cap=10**6)
    ctx.set_stream(None)
    ctx.set_profiling(False)
    same(got, ref.label(volume((5, 67, 131), "rand10"), -1, 26), "stream")
    ms, launches = ctx.kernel_ms("components")
    parts = [ctx.kernel_ms("components_" + p) for p in ("threshold", "local", "merge", "flatten", "number", "stats", "finish")]
    assert ms > 0 and launches == 7 and all(p[0] > 0 and p[1] == 1 for p in parts), (ms, launches, parts)
    assert abs(ms - sum(p[0] for p in parts)) < 1e-9
    live, pinned, after = C.c_int64(), C.c_int64(), C.c_int64()
    lib.load().pnr_live_bytes(C.byref(live), C.byref(pinned))
    ctx.label_components(THR, 6)
    lib.load().pnr_live_bytes(C.byref(after), C.byref(pinned))
    assert after.value == live.value  # every device buffer of the call is freed


# ---- the CLI ----
DIMS = (32, 56, 64)  # (l, h, w) of the small tube stack of the CLI tests
PARAS = "2,3 0 5 0.3 3 2 40 50 2 4 5".split()


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


@functools.lru_cache(maxsize=None)
def speckled_stack():
    """the tube stack with forty connected blobs of 2-6 voxels (value 200), each in a 3 x 3 x 3 cube whose surroundings, three voxels
    further out in every direction, hold nothing brighter than 50 (no tube, no other blob)"""
    l, h, w = DIMS
    img = synth.synth(w, h, l, seed=2).copy()
    rng = np.random.default_rng(17)
    placed = 0
    for _ in range(20000):
        if placed == 40:
            break
        z0, y0, x0 = (int(rng.integers(5, n - 5)) for n in (l, h, w))
        if img[z0 - 4:z0 + 5, y0 - 4:y0 + 5, x0 - 4:x0 + 5].max() >= 50:
            continue
        z, y, x = z0, y0, x0
        for _ in range(int(rng.integers(2, 7))):  # a walk of face steps inside the cube: connected under both connectivities
            img[z, y, x] = 200
            d = int(rng.integers(0, 3))
            step = int(rng.integers(0, 2)) * 2 - 1
            z, y, x = (int(np.clip(v + step * (d == k), c - 1, c + 1)) for k, (v, c) in enumerate(((z, z0), (y, y0), (x, x0))))
        placed += 1
    assert placed == 40
    return _ro(img)


def _dims():
    return ",".join(str(v) for v in DIMS[::-1])


def test_cli_components_json_labels_and_csv(tmp_path):
    V = speckled_stack()
    raw = str(tmp_path / "s.raw")
    V.tofile(raw)
    for thr, conn, ms in ((100, 26, 2), (-1, 26, 1), (100, 6, 1), (37, 6, 5)):
        info, labels, comps = ref.label(V, thr, conn, ms)
        flags = (["--threshold", str(thr)] if thr >= 0 else []) + (["--connectivity", str(conn)] if conn != 26 else []) + (["--min-size", str(ms)] if ms != 1 else [])
        r = _cli("--components", "-i", raw, "-d", _dims(), *flags, "--labels", str(tmp_path / "l.raw"), "--per-component", str(tmp_path / "c.csv"))
        assert r.returncode == 0, r.stderr[-1500:]
        got = json.loads(r.stdout)
        assert got == info and list(got) == ["n_vox", "n_fg", "n_comp", "n_small", "vox_small", "largest", "thr_used"], (got, info)
        assert np.array_equal(np.fromfile(tmp_path / "l.raw", "<i4").reshape(V.shape), labels)
        rows = open(tmp_path / "c.csv").read().split("\n")
        assert rows[0] == "id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax" and rows[-1] == "" and rows[1:-1] == ref.centroid_rows(comps)
    info = ref.label(V, 100, 26)[0]
    assert info["n_comp"] >= 41 and info["n_small"] == 0  # the blobs are there, and are components of their own
    # the same volume setup as tracing: the median removes nothing the rule would not see
    import filter_ref
    r = _cli("--components", "-i", raw, "-d", _dims(), "--median", "3d", "--threshold", "100")
    assert r.returncode == 0 and json.loads(r.stdout) == ref.label(filter_ref.median(V, 3), 100, 26)[0]


def _parse(text):
    lines = text.splitlines()
    return [ln for ln in lines if ln.startswith("#")], [ln for ln in lines if ln and not ln.startswith("#")]


def test_cli_despeckle_equals_tracing_the_despeckled_stack(tmp_path):
    """an exact end-to-end check: --despeckle 8,100 writes the SWC of the reference-despeckled stack traced without the flag, apart from
    the #despeckle= line; two ranks sharing the GPU write the same file; without the flag there is no such line"""
    V = speckled_stack()
    clean, info = ref.despeckle(V, 8, 100, 26)
    assert info["n_small"] >= 40 and not np.array_equal(clean, V)
    raw, pre = str(tmp_path / "raw.raw"), str(tmp_path / "pre.raw")
    V.tofile(raw)
    clean.tofile(pre)

    def go(path, *flags):
        r = _cli(*flags, "-d", _dims(), "-f", "advantra_func", "-i", path, "-p", *PARAS)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(path + "_Advantra.swc").read(), r

    plain, _ = go(pre)
    flagged, r = go(raw, "--despeckle", "8,100")
    assert "despeckle... %d components" % info["n_small"] in r.stdout
    c0, d0 = _parse(plain)
    c1, d1 = _parse(flagged)
    line = "#despeckle=min:8,thr:100,conn:26,removed:%d,voxels:%d" % (info["n_small"], info["vox_small"])
    assert d1 == d0 and len(d0) > 10
    assert c0[-1].startswith("##n,") and c1 == c0[:-1] + [line] + c0[-1:]
    assert go(raw, "--despeckle", "8,100", "--ranks", "2", "--share-gpu")[0] == flagged
    unflagged, _ = go(raw)
    assert "#despeckle" not in unflagged and _parse(unflagged)[0] == c0
    # behind the pre-filter, with the mean as the threshold and 6-connectivity
    import filter_ref
    clean6, info6 = ref.despeckle(filter_ref.tophat(V, 3, 2.0), 5, -1, 6)
    assert info6["n_small"] > 40
    clean6.tofile(pre)
    both, _ = go(raw, "--subtract-background", "3", "--despeckle", "5,-1,6")
    cb, db = _parse(both)
    assert db == _parse(go(pre)[0])[1]
    assert cb[-3:-1] == ["#filter=median:off,tophat:3", "#despeckle=min:5,thr:%d,conn:6,removed:%d,voxels:%d" % (info6["thr_used"], info6["n_small"], info6["vox_small"])]


def test_cli_components_of_the_residual(tmp_path):
    """--render-swc ... --residual R.raw, then --components on R.raw: the list of what the tree missed == the rule on the numpy residual"""
    import render_ref
    V = speckled_stack()
    raw, swc = str(tmp_path / "s.raw"), tmp_path / "t.swc"
    V.tofile(raw)
    swc.write_text("1 2 10 10 8 3 -1\n2 2 50 40 20 2.5 1\n3 2 20 45 12 2 2\n4 2 60 6 28 1.5 -1\n")
    xyz, radius, typ, parent, ids = pnr_amd.read_swc_nodes(swc)
    L = render_ref.render(xyz, radius, parent, V.shape, 2, 1, 0)
    residual = render_ref.coverage(V, L, len(xyz), 100)[4]
    r = _cli("--render-swc", str(swc), "-i", raw, "-d", _dims(), "--zscale", "2", "--coverage-threshold", "100", "--residual", str(tmp_path / "r.raw"))
    assert r.returncode == 0, r.stderr[-1500:]
    assert open(tmp_path / "r.raw", "rb").read() == residual.tobytes() and (residual != V).any()
    for ms in (1, 4):
        info, labels, comps = ref.label(residual, 100, 26, ms)
        r = _cli("--components", "-i", str(tmp_path / "r.raw"), "-d", _dims(), "--threshold", "100", "--min-size", str(ms), "--per-component", str(tmp_path / "m.csv"))
        assert r.returncode == 0, r.stderr[-1500:]
        assert json.loads(r.stdout) == info and info["n_comp"] > 0
        assert open(tmp_path / "m.csv").read().split("\n")[1:-1] == ref.centroid_rows(comps)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31: u32 links above the sign bit, 64-bit voxel arithmetic), made on the device and borrowed: zero
    but for two random blocks, one in the first planes and one in the last six (voxel indices above 2^31), each across several tiles.
    The rule on the blocks alone, moved to their place, is the expected component list; the despeckled volume is read back in full."""
    import torch
    l, h, w = 513, 2048, 2048
    rng = np.random.default_rng(5)
    blocks = [((0, 3, 5), np.where(rng.random((7, 20, 70)) < 0.2, 255, 0).astype(np.uint8)), ((l - 6, 777, 1000), np.where(rng.random((6, 40, 90)) < 0.15, 200, 0).astype(np.uint8))]
    t = torch.zeros((l, h, w), dtype=torch.uint8, device="cuda")
    for (z0, y0, x0), B in blocks:
        t[z0:z0 + B.shape[0], y0:y0 + B.shape[1], x0:x0 + B.shape[2]] = torch.from_numpy(B).cuda()
    torch.cuda.synchronize()
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=2.0), 0)
    c.set_volume_device(t.data_ptr(), (l, h, w), keepalive=t)
    for conn, ms in ((26, 1), (6, 3)):
        want_rows, n_small, vox_small = [], 0, 0
        for (z0, y0, x0), B in blocks:
            info, _, comps = ref.label(B, 100, conn, ms)
            n_small, vox_small = n_small + info["n_small"], vox_small + info["vox_small"]
            bl, bh, bw = B.shape
            f = comps["first"]
            fx, fy, fz = f % bw, (f // bw) % bh, f // (bw * bh)
            comps = comps.copy()
            comps["first"] = (fx + x0) + w * ((fy + y0) + h * (fz + z0))
            for s, o in (("sx", x0), ("sy", y0), ("sz", z0)):
                comps[s] += comps["size"] * o
            for k, o in (("x0", x0), ("x1", x0), ("y0", y0), ("y1", y0), ("z0", z0), ("z1", z0)):
                comps[k] += o
            want_rows.append(comps)
        wcomps = np.concatenate(want_rows)
        info, _, comps = c.label_components(100, conn, ms, labels=False, cap=len(wcomps) + 5)
        assert info["n_vox"] == l * h * w and info["n_comp"] == len(wcomps) and (info["n_small"], info["vox_small"]) == (n_small, vox_small)
        assert wcomps["first"].max() > 2**31 and comps.tobytes() == wcomps.tobytes()
    info = c.despeckle(3, 100, 6)
    assert (info["n_small"], info["vox_small"]) == (n_small, vox_small) and n_small > 0
    got = c.get_volume()
    c.close()
    for (z0, y0, x0), B in blocks:
        sub = got[z0:z0 + B.shape[0], y0:y0 + B.shape[1], x0:x0 + B.shape[2]]
        assert np.array_equal(sub, ref.despeckle(B, 3, 100, 6)[0])
    assert int(np.count_nonzero(got)) == sum(int(np.count_nonzero(ref.despeckle(B, 3, 100, 6)[0])) for _, B in blocks)
    assert int(torch.count_nonzero(t)) == sum(int(np.count_nonzero(B)) for _, B in blocks)  # the borrowed tensor is as it was
