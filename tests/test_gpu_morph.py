"""Grey-level morphological reconstruction on the GPU (pnr_morph_reconstruct, pnr_morph_volume, Context.morph_reconstruct / morph_volume,
advantra_cli --fill-holes / --hmax / --hdome / --morph) against the rule of include/pnr_hip.h restated in numpy (morph_ref.py: the literal
recursion; test_morph_host.py shows that it equals the widest-path solver bit for bit).  The rule fixes every bit: every comparison is
array_equal / ==, there is no tolerance.  The references are computed once per case and shared."""
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
import morph_ref as ref
import thin_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
TZ, TY, TX = ref.tile()
# (l, h, w): the smallest stacks, a 2-D one, long thin ones, odd sizes over several tiles; then exactly one tile, one voxel more than a tile in
# every axis, two tiles minus one, exactly two tiles
SHAPES = [(1, 2, 2), (2, 2, 2), (3, 3, 3), (1, 21, 33), (70, 2, 2), (2, 2, 300), (5, 67, 131), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1),
          (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1), (2 * TZ, 2 * TY, 2 * TX)]
SHAPES = list(dict.fromkeys(SHAPES))
HS = (1, 40, 255)
EXACT = ("n_vox", "n_changed", "n_nonzero", "sum_in", "sum_out", "tiles", "max_delta", "connectivity")


def sid(s):
    return "x".join(map(str, s))


def _ro(V):
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    return _ro(ref.volume(shape, kind))


@functools.lru_cache(maxsize=None)
def marker(shape, kind, name):
    return _ro(ref.markers(volume(shape, kind))[name])


def cases():
    """(op, marker name or None, h) of every run of one (volume, connectivity)"""
    out = [(op, m, 0) for op in ("dilate", "erode") for m in ("rand", "above", "zero")] + [("fill", None, 0)]
    return out + [(op, None, h) for op in ("hmax", "hdome") for h in HS]


@functools.lru_cache(maxsize=None)
def want(shape, kind, op, mname, h, C_):
    V = volume(shape, kind)
    out, used = ref.run(V, op, marker(shape, kind, mname) if mname else None, h, C_)
    return _ro(out), ref.info(V, out, used)


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20), 0)
    yield c
    c.close()


def same(got, wanted, what):
    info, out = got
    wout, winfo = wanted
    assert out.dtype == np.uint8 and out.shape == wout.shape and np.array_equal(out, wout), (what, int((out != wout).sum()), np.argwhere(out != wout)[:4].tolist())
    assert {k: info[k] for k in EXACT} == winfo, (what, info, winfo)
    assert info["rounds"] >= 1 and info["tile_visits"] >= info["tiles"], (what, info)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_every_op_and_connectivity(ctx, shape, kind):
    ctx.set_volume(volume(shape, kind))
    for C_ in ref.CONNS:
        for op, mname, h in cases():
            got = ctx.morph_reconstruct(marker(shape, kind, mname) if mname else None, op, h, C_)
            same(got, want(shape, kind, op, mname, h, C_), (shape, kind, op, mname, h, C_))
    assert np.array_equal(ctx.get_volume(), volume(shape, kind))  # pnr_morph_reconstruct leaves the volume alone


def test_default_connectivity(ctx):
    shape = (TZ + 1, TY + 1, TX + 1)
    ctx.set_volume(volume(shape, "hollow"))
    same(ctx.morph_reconstruct(op="fill"), want(shape, "hollow", "fill", None, 0, 6), "fill")
    same(ctx.morph_reconstruct(op="hmax", h=40), want(shape, "hollow", "hmax", None, 40, 26), "hmax")
    same(ctx.morph_reconstruct(marker(shape, "hollow", "rand")), want(shape, "hollow", "dilate", "rand", 0, 26), "dilate")
    info, out = ctx.morph_reconstruct(op="hdome", h=40, volume=False)
    assert out is None and {k: info[k] for k in EXACT} == want(shape, "hollow", "hdome", None, 40, 26)[1]
    assert not np.array_equal(want(shape, "hollow", "fill", None, 0, 6)[0], want(shape, "hollow", "fill", None, 0, 26)[0])  # the diagonal gap


@pytest.mark.parametrize("shape", [(5, 67, 131), (2 * TZ, 2 * TY, 2 * TX), (TZ + 1, TY + 1, TX + 1)], ids=sid)
def test_scheduling_changes_no_bit(ctx, shape):
    """morph_iters = 1: every visit is one LDS iteration and a tile that changed re-queues itself; morph_tiles_per_launch: launch cuts"""
    ctx.set_volume(volume(shape, "snake"))
    runs = (("hmax", None, 100, 26), ("fill", None, 0, 6), ("dilate", "rand", 0, 4))
    base = {}
    for op, mname, h, C_ in runs:
        info, out = ctx.morph_reconstruct(marker(shape, "snake", mname) if mname else None, op, h, C_)
        base[op] = (info, out)
        assert info["rounds"] == ctx.get_option("morph_rounds") >= 2 and info["tile_visits"] == ctx.get_option("morph_visits")
    try:
        for iters, per in ((1, 0), (1, 1), (0, 1), (0, 3), (2, 3)):
            ctx.set_option("morph_iters", iters)
            ctx.set_option("morph_tiles_per_launch", per)
            for op, mname, h, C_ in runs:
                info, out = ctx.morph_reconstruct(marker(shape, "snake", mname) if mname else None, op, h, C_)
                i0, o0 = base[op]
                assert np.array_equal(out, o0) and {k: info[k] for k in EXACT} == {k: i0[k] for k in EXACT}, (shape, iters, per, op)
                assert info["rounds"] >= 2 and info["tile_visits"] >= info["tiles"]
        # rounds grow: a corridor that turns three times inside the first tile (rows y = 0, 2, 4, 6 of x = 2 .. TX - 3, joined at alternating
        # ends) takes an LDS iteration per row: one visit with the automatic bound, a visit per row and one more with morph_iters = 1
        T = np.zeros(shape, np.uint8)
        for k, yy in enumerate((0, 2, 4, 6)):
            T[0, yy, 2:TX - 2] = 200
            if k < 3:
                T[0, yy + 1, TX - 3 if k % 2 == 0 else 2] = 200
        T[0, 0, 2] = 255
        ctx.set_volume(T)
        wout, _ = ref.run(T, "hmax", h=100, C=6)
        assert int((wout == 155).sum()) == 4 * (TX - 4) + 3
        rounds = {}
        ctx.set_option("morph_tiles_per_launch", 0)
        for iters in (0, 1):
            ctx.set_option("morph_iters", iters)
            info, out = ctx.morph_reconstruct(op="hmax", h=100, connectivity=6)
            assert np.array_equal(out, wout)
            rounds[iters] = info["rounds"]
        assert rounds[0] <= 2 and rounds[1] >= rounds[0] + 3, rounds
    finally:
        ctx.set_option("morph_iters", 0)
        ctx.set_option("morph_tiles_per_launch", 0)


@pytest.mark.parametrize("shape", [(TZ, TY, TX), (1, 21, 33)], ids=sid)
def test_scheduling_changes_no_bit_at_one_tile_and_one_slice(ctx, shape):
    """the re-queue path and a launch per tile where the tile arithmetic has no room: exactly one tile (no neighbour to mark, so the
    automatic bound needs one round only and test_scheduling_changes_no_bit cannot take the shape), and a stack with l = 1"""
    ctx.set_volume(volume(shape, "snake"))
    try:
        ctx.set_option("morph_iters", 1)
        ctx.set_option("morph_tiles_per_launch", 1)
        for op, mname, h, C_ in (("hmax", None, 100, 26), ("fill", None, 0, 6), ("dilate", "rand", 0, 4)):
            got = ctx.morph_reconstruct(marker(shape, "snake", mname) if mname else None, op, h, C_)
            same(got, want(shape, "snake", op, mname, h, C_), (shape, op, C_))
    finally:
        ctx.set_option("morph_iters", 0)
        ctx.set_option("morph_tiles_per_launch", 0)


def test_a_tile_is_visited_again_after_its_neighbour_changed(ctx):
    shape = (5, 67, 131)
    ctx.set_volume(volume(shape, "snake"))
    info, out = ctx.morph_reconstruct(op="hmax", h=100, connectivity=6)
    same((info, out), want(shape, "snake", "hmax", None, 100, 6), "snake")
    assert info["rounds"] > 3 and info["tile_visits"] > info["tiles"], info
    assert int(out.max()) == 155 and int((out == 155).sum()) > 100  # the start's maximum, cut by h, ran down the whole corridor


# ---- pnr_morph_volume ----
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_borrowed_volume_is_never_written(ctx, shift):
    """a torch tensor, also one whose first voxel sits `shift` bytes past an alignment boundary: bit-identical after the call, the context
    holds the result in a buffer of its own (the tensor can be overwritten afterwards)"""
    import torch
    shape = (5, 67, 131)
    V = volume(shape, "smooth")
    for op, h, C_ in (("fill", 0, 0), ("hmax", 40, 0), ("hdome", 40, 8)):
        flat = torch.from_numpy(np.concatenate([np.full(shift, 99, np.uint8), V.ravel(), np.full(7, 99, np.uint8)])).cuda()
        before = flat.clone()
        torch.cuda.synchronize()
        ctx.set_volume_device(flat.data_ptr() + shift, shape, keepalive=flat)
        info, out = ctx.morph_reconstruct(op=op, h=h, connectivity=C_)
        wout, winfo = want(shape, "smooth", op, None, h, C_ or ref.default_conn(op))
        assert np.array_equal(out, wout) and ctx._keep is flat
        vinfo = ctx.morph_volume(op, h, C_)
        torch.cuda.synchronize()
        assert torch.equal(flat, before)
        assert {k: vinfo[k] for k in EXACT} == winfo == {k: info[k] for k in EXACT}
        assert np.array_equal(ctx.get_volume(), wout) and ctx._keep is None
        flat.zero_()
        torch.cuda.synchronize()
        assert np.array_equal(ctx.get_volume(), wout)


def test_a_second_call_works_on_the_result_of_the_first(ctx):
    shape = (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1)
    V = volume(shape, "rand")
    ctx.set_volume(V)
    ctx.morph_volume("fill", connectivity=4)
    F = want(shape, "rand", "fill", None, 0, 4)[0]
    assert np.array_equal(ctx.get_volume(), F)
    info = ctx.morph_volume("hdome", 30)
    D, _ = ref.run(F, "hdome", h=30)
    assert np.array_equal(ctx.get_volume(), D) and {k: info[k] for k in EXACT} == ref.info(F, D, 26)
    assert int(D.max()) == 30 and info["max_delta"] > 0


def noisy_stack():
    img = synth.synth(64, 64, 32, seed=2, zdist=2.0).astype(np.int32)
    rng = np.random.default_rng(21)
    img += 25 + rng.poisson(6.0, img.shape)  # a background pedestal and shot noise
    return np.clip(img, 0, 255).astype(np.uint8)


def test_morph_volume_invalidates_the_pipeline_state_and_reconstruct_does_not():
    ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30), 0)
    x = noisy_stack()
    ctx.set_volume(x)
    ctx.frangi()
    seeds = ctx.extract_seeds()
    nodes, _, _, _ = ctx.trace_replay(ctx.score_filter_sort(seeds))
    assert len(seeds) > 0 and len(nodes) > 1
    ctx.morph_reconstruct(op="fill")  # the state stays
    assert ctx.extract_seeds().tobytes() == seeds.tobytes() and len(ctx.get_graph()[0]) == len(nodes)
    assert np.array_equal(ctx.get_volume(), x)
    ctx.morph_volume("hdome", 30)
    with pytest.raises(pnr_amd.lib.PnrError, match="error -4"):  # PNR_E_STATE: J8 is gone
        ctx.extract_seeds()
    with pytest.raises(pnr_amd.lib.PnrError, match="error -4"):
        ctx.get_graph()
    ctx.frangi()
    ctx.extract_seeds()
    ctx.close()


def test_errors_and_their_messages(ctx):
    L = lib.load()
    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    o = lib.MorphOpts(3, 0, 0, 0)
    assert L.pnr_morph_volume(fresh.h, C.byref(o), None) == -4 and b"pnr_morph_volume: no volume set" in L.pnr_last_error()  # PNR_E_STATE
    assert L.pnr_morph_reconstruct(fresh.h, C.byref(o), None, None, None) == -4 and b"pnr_morph_reconstruct: no volume set" in L.pnr_last_error()
    bad = lib.MorphOpts(6, 0, 0, 0)
    assert L.pnr_morph_reconstruct(fresh.h, C.byref(bad), None, None, None) == -1  # arguments are checked first
    fresh.close()
    shape = (5, 67, 131)
    V = volume(shape, "rand")
    ctx.set_volume(V)
    m = marker(shape, "rand", "rand")
    for kw, msg in ((dict(op=0), "op = 0 outside [1, 5]"), (dict(op=6), "op = 6 outside [1, 5]"), (dict(op="fill", connectivity=5), "connectivity = 5, not 0, 4, 8, 6 or 26"),
                    (dict(op="fill", connectivity=-1), "connectivity = -1"), (dict(op="hmax", h=0), "h = 0, outside [1, 255]"), (dict(op="hdome", h=256), "h = 256, outside [1, 255]"),
                    (dict(op="fill", h=3), "h = 3, not 0"), (dict(marker=m, op="dilate", h=1), "h = 1, not 0"), (dict(op="dilate"), "op = 1 needs a marker"),
                    (dict(op="erode"), "op = 2 needs a marker"), (dict(marker=m, op="fill"), "op = 3 takes no marker"), (dict(marker=m, op="hmax", h=3), "op = 4 takes no marker")):
        with pytest.raises(pnr_amd.lib.PnrError, match="error -1") as e:
            ctx.morph_reconstruct(**kw)
        assert "pnr_morph_reconstruct: " + msg in str(e.value), (kw, str(e.value))
    for op, h, C_, msg in ((1, 0, 0, "op = 1 outside [3, 5]"), (2, 0, 0, "op = 2 outside [3, 5]"), (6, 0, 0, "op = 6 outside [3, 5]"), (3, 1, 0, "h = 1, not 0"),
                           (4, 0, 0, "h = 0, outside [1, 255]"), (5, 3, 7, "connectivity = 7")):
        with pytest.raises(pnr_amd.lib.PnrError, match="error -1") as e:
            ctx.morph_volume(op, h, C_)
        assert "pnr_morph_volume: " + msg in str(e.value), (op, h, C_, str(e.value))
        assert np.array_equal(ctx.get_volume(), V)
    assert L.pnr_morph_volume(ctx.h, None, None) == -1 and L.pnr_morph_volume(None, C.byref(o), None) == -1 and L.pnr_morph_reconstruct(ctx.h, None, None, None, None) == -1
    with pytest.raises(ValueError, match="marker of"):
        ctx.morph_reconstruct(m[1:], "dilate")
    assert np.array_equal(ctx.get_volume(), V)


def test_kernel_times_and_live_bytes(ctx):
    shape = (5, 67, 131)
    ctx.set_volume(volume(shape, "smooth"))
    dev0, pin0 = lib.live_bytes()
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("morph") == (0.0, 0)
    info, _ = ctx.morph_reconstruct(op="fill")
    ms, launches = ctx.kernel_ms("morph")
    parts = {p: ctx.kernel_ms("morph_" + p) for p in ("init", "compact", "relax", "finish")}
    ctx.set_profiling(False)
    assert ms > 0 and launches == sum(v[1] for v in parts.values()) and abs(ms - sum(v[0] for v in parts.values())) < 1e-6
    assert parts["init"][1] == parts["finish"][1] == 1 and parts["compact"][1] == info["rounds"] + 1 and parts["relax"][1] == info["rounds"]
    assert lib.live_bytes() == (dev0, pin0)  # every buffer of the call is freed


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31), made on the device and borrowed: a plateau of 200 with one voxel of 255, across tile faces, in
    the first plane and one in the last (its voxel indices are above 2^31).  H-maxima 100 turns both into 155 and nothing else: the summary
    says so exactly (the literal recursion on 2^31 voxels is out of reach; the plateaus' answer is known)"""
    import torch
    l, h, w = 513, 2048, 2048
    t = torch.zeros((l, h, w), dtype=torch.uint8, device="cuda")
    for z in (0, l - 1):
        t[z, h - 45:h - 5, w - 55:w - 5] = 200
        t[z, h - 45, w - 55] = 255
    torch.cuda.synchronize()
    ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=2.0), 0)
    ctx.set_volume_device(t.data_ptr(), (l, h, w), keepalive=t)
    info, out = ctx.morph_reconstruct(op="hmax", h=100, volume=False)
    ctx.close()
    n = 2 * 40 * 50
    assert out is None and {k: info[k] for k in EXACT} == {"n_vox": l * h * w, "n_changed": n, "n_nonzero": n, "sum_in": (n - 2) * 200 + 2 * 255, "sum_out": n * 155,
                                                          "tiles": -(-l // TZ) * -(-h // TY) * -(-w // TX), "max_delta": 100, "connectivity": 26}, info


# ---- the reason for the feature, through the product ----
def test_the_hollow_soma_thins_to_a_curve_once_filled(ctx):
    V = ref.hollow_ball()
    ctx.set_volume(V)
    before, _, _, _ = ctx.skeletonize(100, volume=False)
    ctx.morph_volume("fill")
    F, _ = ref.run(V, "fill")
    assert np.array_equal(ctx.get_volume(), F)
    info, skel, vox, deg = ctx.skeletonize(100)
    winfo, wskel, wvox, wdeg = thin_ref.skeletonize(F, 100)
    assert np.array_equal(skel, wskel) and np.array_equal(vox, wvox) and np.array_equal(deg, wdeg)
    assert {k: info[k] for k in winfo} == winfo
    assert 0 < info["n_skel"] < before["n_skel"], (info, before)


# ---- the CLI ----
def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def _save8(path, x):
    from PIL import Image
    pages = [Image.fromarray(z) for z in x]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression=None)


def _load8(path, shape):
    from PIL import Image, ImageSequence
    return np.stack([np.array(p) for p in ImageSequence.Iterator(Image.open(path))]).reshape(shape)


def _parse(text):
    lines = text.splitlines()
    return [ln for ln in lines if ln.startswith("#")], [ln for ln in lines if ln and not ln.startswith("#")]


def test_cli_morph_tool(tmp_path):
    shape = (2 * TZ - 1, 2 * TY - 1, 2 * TX - 1)
    V = volume(shape, "smooth")
    l, h, w = shape
    raw = str(tmp_path / "v.raw")
    V.tofile(raw)
    dims = "%d,%d,%d" % (w, h, l)
    F6 = want(shape, "smooth", "fill", None, 0, 6)
    for flags, stages in ((("--fill-holes", "3d"), [("fill", 0, 6)]), (("--fill-holes", "2d", "--hdome", "40"), [("fill", 0, 4), ("hdome", 40, 26)]), (("--hmax", "1"), [("hmax", 1, 26)])):
        for name in ("o.raw", "o.tif"):
            out = str(tmp_path / name)
            r = _cli("--morph", "-i", raw, "-d", dims, *flags, "--morph-out", out)
            assert r.returncode == 0, r.stderr[-1500:]
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            assert len(lines) == 1
            js = json.loads(lines[0])
            cur = V
            assert len(js["stages"]) == len(stages)
            for st, (op, hh, C_) in zip(js["stages"], stages):
                res, used = ref.run(cur, op, h=hh, C=C_)
                assert st["op"] == op and st["h"] == hh and {k: st[k] for k in EXACT} == ref.info(cur, res, used), (flags, st)
                assert st["rounds"] >= 1 and st["tile_visits"] >= st["tiles"]
                cur = res
            got = np.fromfile(out, np.uint8).reshape(shape) if name.endswith(".raw") else _load8(out, shape)
            assert np.array_equal(got, cur), (flags, name)
    assert np.array_equal(F6[0], ref.run(V, "fill", C=6)[0])


def test_cli_skeleton_after_fill(tmp_path, ctx):
    V = ref.hollow_ball()
    l, h, w = V.shape
    raw, out = str(tmp_path / "ball.raw"), str(tmp_path / "skel.raw")
    V.tofile(raw)
    r = _cli("--skeleton", "-i", raw, "-d", "%d,%d,%d" % (w, h, l), "--threshold", "100", "--fill-holes", "3d", "--skeleton-out", out)
    assert r.returncode == 0, r.stderr[-1500:]
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    ctx.set_volume(V)
    ctx.morph_volume("fill", connectivity=6)
    info, skel, _, _ = ctx.skeletonize(100, voxels=False)
    assert np.array_equal(np.fromfile(out, np.uint8).reshape(V.shape), skel)
    assert all(js[k] == info[k] for k in ("n_fg", "n_skel", "n_end", "n_branch", "thr_used")), (js, info)
    r0 = _cli("--skeleton", "-i", raw, "-d", "%d,%d,%d" % (w, h, l), "--threshold", "100")
    assert r0.returncode == 0 and json.loads([ln for ln in r0.stdout.splitlines() if ln.startswith("{")][0])["n_skel"] > js["n_skel"]


def dim_stack():
    """tubes of at most 31 grey levels on a pedestal of 40 with pits and bumps of up to 3: the fill closes the pits, and the h-domes of
    height 30 are the tubes themselves (a dome keeps only the top h levels of anything brighter)"""
    img = synth.synth(64, 64, 32, seed=2, zdist=2.0, noise=0).astype(np.int32) // 7
    return np.clip(img + 40 + np.random.default_rng(21).integers(0, 4, img.shape), 0, 255).astype(np.uint8)


def test_cli_tracing_flags(tmp_path):
    """--fill-holes 3d --hdome 30 on a TIFF == the CLI on the pre-computed TIFF: identical SWC bodies; the comment block gains #morph=
    behind #filter; two ranks sharing the GPU write the same file; without the flags there is no #morph line"""
    x = dim_stack()
    raw, pre = str(tmp_path / "raw.tif"), str(tmp_path / "pre.tif")
    _save8(raw, x)
    F, _ = ref.run(x, "fill", C=6)
    D, _ = ref.run(F, "hdome", h=30, C=26)
    _save8(pre, D)
    tail = ("-f", "advantra_func", "-p", *"2,3 0 5 0.3 3 2 40 50 2 4 5".split())

    def go(tif, *flags):
        r = _cli(*flags, "-i", tif, *tail)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(tif + "_Advantra.swc").read(), r

    flags = ("--fill-holes", "3d", "--hdome", "30")
    plain, _ = go(pre)
    morphed, r = go(raw, *flags, "--timing")
    assert "fill holes 3d" in r.stdout and "h-dome 30" in r.stdout and "[pnr host] morph:" in r.stderr
    c0, d0 = _parse(plain)
    c1, d1 = _parse(morphed)
    assert d1 == d0 and len(d0) > 10
    assert c0[-1].startswith("##n,") and c1 == c0[:-1] + ["#morph=fill:3d,hmax:off,hdome:30"] + c0[-1:]
    both, _ = go(raw, "--median", "2d", *flags, "--despeckle", "4")
    cb = _parse(both)[0]
    k = cb.index("#morph=fill:3d,hmax:off,hdome:30")
    assert cb[k - 1].startswith("#filter=median:2d") and cb[k + 1].startswith("#despeckle=")
    assert go(raw, *flags, "--ranks", "2", "--share-gpu")[0] == morphed
    untouched, _ = go(raw)
    assert "#morph" not in untouched and _parse(untouched)[0] == c0
    only, _ = go(raw, "--hmax", "12")
    assert "#morph=fill:off,hmax:12,hdome:off" in _parse(only)[0]
