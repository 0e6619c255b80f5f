"""The pre-filters of the traced volume on the GPU (pnr_filter_volume, Context.filter_volume, advantra_cli --median /
--subtract-background) against the rule of include/pnr_hip.h restated in numpy (filter_ref.py).  The rule is integer-exact: every
comparison is array_equal over the whole volume."""
import ctypes as C
import functools
import os
import re
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import filter_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")


def _tile_constants():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "filter.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (MED_TX|MED_TY|MED_ZC|TH_CH) = (\d+);", txt)}


TILE = _tile_constants()
TX, TY, ZC, CH = TILE["MED_TX"], TILE["MED_TY"], TILE["MED_ZC"], TILE["TH_CH"]
# (l, h, w).  From the kernels' own constants: a median tile boundary one voxel short of the edge in every axis (the last tile is one
# voxel thick) and one voxel past it (the last tile lacks one voxel); rows one voxel longer than a chunk of the top-hat's x pass,
# and rows of more than two chunks (the raw tail carried twice)
SHAPES = [(1, 2, 2), (2, 2, 2), (3, 3, 3), (1, 21, 33), (70, 2, 2), (2, 2, 300), (5, 67, 131), (33, 129, 257), (64, 64, 64),
          (ZC + 1, TY + 1, TX + 1), (2 * ZC - 1, 2 * TY - 1, 2 * TX - 1), (2, 3, CH + 1), (1, 2, 2 * CH + 5)]
INPUTS = ("uniform", "two", "zero", "full", "mix", "ramp")
ZDS = (1.0, 2.0, 3.5)
RS = (1, 2, 7, 64)


def sid(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    rng = np.random.default_rng(abs(hash((shape, INPUTS.index(kind)))) % 2**32)
    if kind == "uniform":
        V = rng.integers(0, 256, shape, dtype=np.uint8)
    elif kind == "two":  # ties dominate
        V = np.where(rng.random(shape) < 0.5, 37, 38).astype(np.uint8)
    elif kind == "zero":
        V = np.zeros(shape, np.uint8)
    elif kind == "full":
        V = np.full(shape, 255, np.uint8)
    elif kind == "mix":
        V = np.where(rng.random(shape) < 0.5, 0, 255).astype(np.uint8)
    else:  # a smooth ramp with 5 % salt and pepper
        l, h, w = shape
        z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
        V = (20 + 180 * (x / max(w - 1, 1) + y / max(h - 1, 1) + z / max(l - 1, 1)) / 3).astype(np.uint8)
        u = rng.random(shape)
        V[u < 0.025] = 0
        V[u > 0.975] = 255
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def want_median(shape, kind, mode):
    return filter_ref.median(volume(shape, kind), mode)


@pytest.fixture(scope="module")
def ctxs():
    c = {zd: pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=zd, np_=20), 0) for zd in ZDS}
    yield c
    for x in c.values():
        x.close()


def differs(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} voxels differ, first (z, y, x) {bad[:4].tolist()}: got {got[got != want][:4].tolist()}, want {want[got != want][:4].tolist()}"


def run(ctx, V, median=0, tophat=0):
    ctx.set_volume(V)
    ctx.filter_volume(median=median, tophat=tophat)
    got = ctx.get_volume()
    assert got.dtype == np.uint8 and got.shape == V.shape
    return got


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_median(ctxs, shape, kind):
    V = volume(shape, kind)
    for mode in (2, 3):
        got, want = run(ctxs[2.0], V, median=mode), want_median(shape, kind, mode)
        assert np.array_equal(got, want), (shape, kind, mode, differs(got, want))
    if shape[0] == 1:
        assert np.array_equal(want_median(shape, kind, 3), want_median(shape, kind, 2))


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("zd", ZDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_tophat(ctxs, shape, zd, R, kind):
    """rz = R, R div 2 and (int)(R / 3.5), rz = 0 among them; boxes larger than the stack"""
    V = volume(shape, kind)
    got, want = run(ctxs[zd], V, tophat=R), filter_ref.tophat(V, R, zd)
    assert np.array_equal(got, want), (shape, kind, zd, R, filter_ref.box(R, zd, shape[0]), differs(got, want))


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_both_stages_and_two_calls(ctxs, shape):
    for kind, mode, R, zd in (("uniform", 3, 2, 2.0), ("ramp", 2, 7, 3.5), ("two", 3, 64, 1.0)):
        V = volume(shape, kind)
        ctx = ctxs[zd]
        got, want = run(ctx, V, median=mode, tophat=R), filter_ref.apply(V, mode, R, zd)
        assert np.array_equal(got, want), (shape, kind, mode, R, zd, differs(got, want))
        ctx.filter_volume(median=mode, tophat=R)  # a second call filters the filtered volume
        got2, want2 = ctx.get_volume(), filter_ref.apply(want, mode, R, zd)
        assert np.array_equal(got2, want2), (shape, kind, mode, R, zd, differs(got2, want2))
        ctx.filter_volume()  # both stages off: a valid no-op
        assert np.array_equal(ctx.get_volume(), want2)


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_borrowed_volume_is_never_written(ctxs, shift):
    """a torch tensor, also one whose first voxel sits `shift` bytes past an alignment boundary: bit-identical after the call, the
    context holds the filtered bytes in a buffer of its own (the tensor can be overwritten afterwards)"""
    import torch
    ctx = ctxs[2.0]
    for shape in ((5, 67, 131), (9, 16, 256)):
        V = volume(shape, "ramp")
        for kw in (dict(median=3), dict(median=2), dict(tophat=3), dict(median=3, tophat=5)):
            flat = torch.from_numpy(np.concatenate([np.full(shift, 99, np.uint8), V.ravel(), np.full(7, 99, np.uint8)])).cuda()
            before = flat.clone()
            torch.cuda.synchronize()
            assert (flat.data_ptr() + shift) % 4 == shift % 4
            ctx.set_volume_device(flat.data_ptr() + shift, shape, keepalive=flat)
            ctx.filter_volume(**kw)
            torch.cuda.synchronize()
            assert torch.equal(flat, before)
            want = filter_ref.apply(V, kw.get("median", 0), kw.get("tophat", 0), 2.0)
            got = ctx.get_volume()
            assert np.array_equal(got, want), (shape, kw, shift, differs(got, want))
            assert ctx._keep is None
            flat.zero_()
            torch.cuda.synchronize()
            assert np.array_equal(ctx.get_volume(), want)


def np_map(x, lo, hi):
    """the windowing rule of pnr_set_volume_u16 (include/pnr_hip.h): 255 a / d rounded half up, a = clamp(v, lo, hi) - lo, d = hi - lo"""
    a = np.clip(np.asarray(x).astype(np.int64), lo, hi) - lo
    d = hi - lo
    return ((510 * a + d) // (2 * d)).astype(np.uint8)


def test_sixteen_bit_input_is_filtered_after_windowing(ctxs):
    rng = np.random.default_rng(12)
    img8 = synth.synth(40, 36, 12, seed=3)
    x = (img8.astype(np.uint16) * 14 + 300 + rng.integers(0, 200, img8.shape)).astype(np.uint16)
    lo, hi = 350, 3300
    ctx = ctxs[2.0]
    ctx.set_volume(x, window=(lo, hi))
    ctx.filter_volume(median=3, tophat=6)
    want = filter_ref.apply(np_map(x, lo, hi), 3, 6, 2.0)
    got = ctx.get_volume()
    assert np.array_equal(got, want), differs(got, want)
    assert got.max() > 50  # (the window and the top-hat left something to compare)


def test_errors_leave_the_volume(ctxs):
    L = lib.load()
    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    o = lib.FilterOpts(3, 4)
    assert L.pnr_filter_volume(fresh.h, C.byref(o)) == -4 and b"no volume" in L.pnr_last_error()  # PNR_E_STATE
    bad = lib.FilterOpts(4, 0)
    assert L.pnr_filter_volume(fresh.h, C.byref(bad)) == -1  # arguments are checked first
    fresh.close()
    ctx = ctxs[2.0]
    V = volume((5, 67, 131), "uniform")
    ctx.set_volume(V)
    for median, tophat in ((1, 0), (4, 0), (-1, 0), (27, 3), (0, -1), (0, 65), (3, 1000)):
        with pytest.raises(pnr_amd.lib.PnrError, match="error -1"):
            ctx.filter_volume(median=median, tophat=tophat)
        assert np.array_equal(ctx.get_volume(), V)
    assert L.pnr_filter_volume(ctx.h, None) == -1 and L.pnr_filter_volume(None, C.byref(o)) == -1
    assert np.array_equal(ctx.get_volume(), V)
    ctx.filter_volume(median=0, tophat=64)  # the ends of the ranges are valid
    assert np.array_equal(ctx.get_volume(), filter_ref.tophat(V, 64, 2.0))


def noisy_stack():
    img = synth.synth(64, 64, 32, seed=2, zdist=2.0).astype(np.int32)
    rng = np.random.default_rng(21)
    img += 25 + rng.poisson(6.0, img.shape)  # a background pedestal and shot noise
    img[rng.random(img.shape) < 0.01] = 255
    return np.clip(img, 0, 255).astype(np.uint8)


def test_filter_invalidates_the_pipeline_state():
    ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30), 0)
    ctx.set_volume(noisy_stack())
    ctx.frangi()
    seeds = ctx.extract_seeds()
    nodes, _, _, _ = ctx.trace_replay(ctx.score_filter_sort(seeds))
    assert len(seeds) > 0 and len(nodes) > 1
    ctx.get_graph()
    ctx.filter_volume(median=3)
    with pytest.raises(pnr_amd.lib.PnrError, match="error -4"):  # PNR_E_STATE: J8 is gone
        ctx.extract_seeds()
    with pytest.raises(pnr_amd.lib.PnrError, match="error -4"):
        ctx.get_graph()
    ctx.frangi()
    ctx.extract_seeds()
    ctx.close()


def test_pipeline_on_the_filtered_volume(ctxs):
    """filter_volume on the device, then the pipeline == the pipeline on the restatement's bytes: J8, seeds, nodes and links; the
    "filter" kernel-time group; a stream that is not the context's own"""
    import torch
    x = noisy_stack()
    p = pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20, ni=30)
    out = []
    for pre in (False, True):
        ctx = pnr_amd.Context(p, 0)
        if pre:
            ctx.set_volume(filter_ref.apply(x, 3, 6, 2.0))
        else:
            ctx.set_volume(x)
            ctx.set_profiling(True)
            ctx.reset_kernel_ms()
            assert ctx.kernel_ms("filter") == (0.0, 0)
            s = torch.cuda.Stream()
            ctx.set_stream(s.cuda_stream)
            ctx.filter_volume(3, 6)
            ctx.set_stream(None)
            ms, launches = ctx.kernel_ms("filter")
            assert ms > 0 and launches == 7, (ms, launches)  # the median and six passes (rz = 3)
            ctx.set_profiling(False)
        ctx.frangi()
        J8 = ctx.get_frangi(J=False, V=False)["J8"]
        seeds_init = ctx.extract_seeds()
        seeds = ctx.score_filter_sort(seeds_init)
        nodes, links, ntr, _ = ctx.trace_replay(seeds)
        out.append((J8, seeds_init, seeds, nodes, links, ntr))
        ctx.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and a[0].max() == 255
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and len(a[2]) > 5
    assert a[3].tobytes() == b[3].tobytes() and np.array_equal(a[4], b[4]) and a[5] == b[5] and len(a[3]) > 10


# ---- the CLI ----
def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def _save8(path, x):
    from PIL import Image
    pages = [Image.fromarray(z) for z in x]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression=None)


def _parse(text):
    lines = text.splitlines()
    return [ln for ln in lines if ln.startswith("#")], [ln for ln in lines if ln and not ln.startswith("#")]


def test_cli_filter_flags(tmp_path):
    """--median 3d --subtract-background 6 on a TIFF == the CLI on the pre-filtered TIFF: identical SWC bodies; the comment block
    gains #filter= (in front of #radius with --measure-radius); two ranks sharing the GPU write the same file; without the flags
    there is no #filter line"""
    x = noisy_stack()
    raw, pre = str(tmp_path / "raw.tif"), str(tmp_path / "pre.tif")
    _save8(raw, x)
    _save8(pre, filter_ref.apply(x, 3, 6, 2.0))
    tail = ("-f", "advantra_func", "-p", *"2,3 0 5 0.3 3 2 40 50 2 4 5".split())

    def go(tif, *flags):
        r = _cli(*flags, "-i", tif, *tail)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(tif + "_Advantra.swc").read(), r

    flags = ("--median", "3d", "--subtract-background", "6")
    plain, _ = go(pre)
    filt, r = go(raw, *flags, "--timing")
    assert "pre-filter... median 3d, top-hat 6" in r.stdout and "[pnr host] filter:" in r.stderr
    c0, d0 = _parse(plain)
    c1, d1 = _parse(filt)
    assert d1 == d0 and len(d0) > 10
    assert c0[-1].startswith("##n,") and c1 == c0[:-1] + ["#filter=median:3d,tophat:6"] + c0[-1:]
    measured, _ = go(raw, *flags, "--measure-radius")
    cm = _parse(measured)[0]
    assert cm[-3] == "#filter=median:3d,tophat:6" and cm[-2].startswith("#radius=measured") and cm[-1] == c0[-1]
    assert _parse(measured)[1] == _parse(go(pre, "--measure-radius")[0])[1]  # measured on the filtered bytes
    assert go(raw, *flags, "--ranks", "2", "--share-gpu")[0] == filt
    unfiltered, _ = go(raw)
    assert "#filter" not in unfiltered and _parse(unfiltered)[0] == c0
    only, _ = go(raw, "--median", "2d")
    assert "#filter=median:2d,tophat:off" in _parse(only)[0]
    _save8(pre, filter_ref.apply(x, 2, 0, 2.0))
    assert _parse(only)[1] == _parse(go(pre)[0])[1]
    only, _ = go(raw, "--subtract-background", "64", "-v")
    assert "#filter=median:off,tophat:64" in _parse(only)[0]


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31), made on the device and borrowed: two 64 x 64 crops over the first and the last six planes
    (the last plane's voxel indices are above 2^31) against the restatement on the crops with their halo (1 for the median, twice the
    box for the opening: 9 voxels in x and y, 5 planes)"""
    import torch
    l, h, w = 513, 2048, 2048
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.randint(0, 256, (l, h, w), dtype=torch.uint8, device="cuda", generator=g)
    t[-8:, 700:900, 900:1200] //= 3  # structure where the last planes are compared
    torch.cuda.synchronize()
    ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=2.0), 0)
    ctx.set_volume_device(t.data_ptr(), (l, h, w), keepalive=t)
    ctx.filter_volume(3, 4)
    got = ctx.get_volume()
    ctx.close()
    hx, hz = 9, 5
    for zs in (slice(0, 6), slice(l - 6, l)):
        for y0, x0 in ((0, 0), (777, 1000), (h - 64, w - 64)):
            za, zb = max(zs.start - hz, 0), min(zs.stop + hz, l)
            ya, yb, xa, xb = max(y0 - hx, 0), min(y0 + 64 + hx, h), max(x0 - hx, 0), min(x0 + 64 + hx, w)
            sub = t[za:zb, ya:yb, xa:xb].cpu().numpy()
            want = filter_ref.apply(sub, 3, 4, 2.0)[zs.start - za:zs.stop - za, y0 - ya:y0 - ya + 64, x0 - xa:x0 - xa + 64]
            have = got[zs, y0:y0 + 64, x0:x0 + 64]
            assert np.array_equal(have, want), (zs, y0, x0, differs(have, want))
            assert want.max() > 0
