"""The thresholds on the GPU (pnr_auto_threshold, pnr_local_threshold[_volume], the threshold words of the Context methods and of
advantra_cli) against the rules of include/pnr_hip.h restated in numpy (threshold_ref.py).  The rules are integer-exact: every
comparison is array_equal / ==."""
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
import threshold_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")


def _constants():
    txt = open(os.path.join(ROOT, "pnr_amd", "csrc", "threshold.h")).read()
    xch = int(re.search(r"constexpr int LT_XCH = (\d+);", txt).group(1))
    shift = int(re.search(r"constexpr long long LT_SLAB_VOX = 1LL << (\d+);", txt).group(1))
    return xch, 1 << shift


XCH, SLAB_VOX = _constants()
ZDS = (1.0, 2.0, 3.7)
# one grid-stride sweep of the histogram: 512 work-groups of 1024 lanes, 16 bytes each
SWEEP = 512 * 1024 * 16
HIST_NS = (1, 15, 16, 17, 31, 4097)
HIST_SHAPES = [(1, 2, 2), (70, 2, 2), (2, 2, 300), (5, 67, 131), (33, 512, 512)]
assert 33 * 512 * 512 > SWEEP
LOCAL_SHAPES = [(1, 1, 1), (3, 1, 5), (1, 21, 33), (70, 2, 2), (2, 2, 300), (5, 67, 131), (2, 3, XCH + 1), (1, 2, 2 * XCH + 5)]
# (offset, scale_256, floor, binary): every value of the four at least once, the extremes together
COMBOS = ((0, 256, 1, False), (-20, 320, 1, True), (20, 0, 40, False), (0, 4096, 1, False), (20, 256, 40, True), (-20, 0, 1, False), (-255, 4096, 255, True))


def sid(s):
    return "x".join(map(str, s))


KINDS = ("uniform", "zero", "full", "but_one", "but_first", "sparse")


@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    rng = np.random.default_rng([*shape, KINDS.index(kind)])
    if kind == "uniform":
        V = rng.integers(0, 256, shape, dtype=np.uint8)
    elif kind == "zero":
        V = np.zeros(shape, np.uint8)
    elif kind == "full":
        V = np.full(shape, 255, np.uint8)
    elif kind == "but_one":  # every voxel equal but one (the last: the hot bin is the first voxel's)
        V = np.full(shape, 37, np.uint8)
        V.reshape(-1)[-1] = 38
    elif kind == "but_first":
        V = np.full(shape, 37, np.uint8)
        V.reshape(-1)[0] = 200
    else:  # dark with bright sparse structure and holes of zeros
        V = (rng.integers(0, 40, shape) + np.where(rng.random(shape) < 0.1, rng.integers(60, 216, shape), 0)).astype(np.uint8)
        V[rng.random(shape) < 0.2] = 0
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def sums(shape, kind, r, zd):
    n, S = ref.local_sums(volume(shape, kind), r, zd)
    return n, S


def want_local(shape, kind, r, zd, combo):
    V = volume(shape, kind)
    n, S = sums(shape, kind, r, zd)
    out, keep = ref._decide(V, n, S, *combo)
    rx, ry, rz = ref.box(r, zd, shape[0])
    return out, dict(n_vox=V.size, n_kept=int(keep.sum()), sum_in=int(V.sum(dtype=np.int64)), sum_out=int(out.sum(dtype=np.int64)), rx=rx, ry=ry, rz=rz)


@pytest.fixture(scope="module")
def ctxs():
    c = {zd: pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=zd, np_=20), 0) for zd in ZDS}
    yield c
    for x in c.values():
        x.close()


def differs(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} voxels differ, first (z, y, x) {bad[:4].tolist()}: got {got[got != want][:4].tolist()}, want {want[got != want][:4].tolist()}"


# ---- the histogram ----
@pytest.mark.parametrize("shape", HIST_SHAPES, ids=sid)
def test_histogram_equals_bincount(ctxs, shape):
    ctx = ctxs[2.0]
    for kind in ("zero", "full", "but_one", "but_first", "uniform", "sparse"):
        V = volume(shape, kind)
        ctx.set_volume(V)
        info, H = ctx.auto_threshold("otsu", hist=True)
        want = ref.histogram(V)
        assert H.dtype == np.uint64 and np.array_equal(H, want), (shape, kind, np.flatnonzero(H != want)[:8])
        assert info == ref.from_hist(want, "otsu"), (shape, kind)


@pytest.mark.parametrize("n", HIST_NS)
def test_histogram_of_n_bytes(ctxs, n):
    """a context's volume is at least 2 x 2 x 1: the kernel on n bytes through its test tap, the first byte 0..15 bytes past a
    16-byte boundary"""
    ctx = ctxs[2.0]
    for kind in ("zero", "full", "but_one", "but_first", "uniform", "sparse"):
        V = volume((1, 1, n), kind)
        for off in range(16):
            H = ctx.tap_histogram(V, off)
            assert np.array_equal(H, ref.histogram(V)), (n, kind, off)


def test_histogram_of_the_synthetic_stack_and_every_method(ctxs, oracle):
    ctx = ctxs[2.0]
    img = synth.synth(48, 40, 24, seed=1, zdist=2.0)
    ctx.set_volume(img)
    want = ref.histogram(img)
    for method, lo, ppm in (("mean", 0, None), ("otsu", 0, None), ("otsu", 1, None), ("triangle", 0, None), ("triangle", 17, None), ("top", 0, 10000), ("top", 1, 1),
                            ("maxentropy", 0, None)):
        info, H = ctx.auto_threshold(method, lo, ppm, hist=True)
        assert np.array_equal(H, want)
        assert info == ref.from_hist(want, method, lo, ppm, oracle.orc_maxentropy_hist), (method, lo, ppm)
    assert ctx.auto_threshold("mean")["thr"] == max(1, int(img.sum(dtype=np.int64)) // img.size)


def test_histogram_of_a_borrowed_volume_at_every_alignment(ctxs):
    """a torch tensor sliced so that its first voxel sits 1..15 bytes past a 16-byte boundary: the scalar head and tail; the tensor is
    as it was afterwards"""
    import torch
    ctx = ctxs[2.0]
    shape = (3, 37, 41)
    n = int(np.prod(shape))
    V = volume((1, 1, n + 64), "sparse").reshape(-1)
    t = torch.from_numpy(V.copy()).cuda()
    assert t.data_ptr() % 16 == 0
    for off in range(1, 16):
        for shp in (shape, (1, 2, 2), (1, 2, 4), (1, 3, 5), (1, 2, 9)):  # also: a head alone, no vector, a tail (smaller: test_histogram_of_n_bytes)
            m = int(np.prod(shp))
            view = t[off:off + m]
            ctx.set_volume_device(view.data_ptr(), shp, keepalive=t)
            _, H = ctx.auto_threshold("mean", hist=True)
            assert np.array_equal(H, ref.histogram(V[off:off + m])), (off, m)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), V)


def test_auto_threshold_leaves_the_context(ctxs):
    ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20), 0)
    img = synth.synth(48, 40, 24, seed=1, zdist=2.0)
    ctx.set_volume(img)
    jmin, jmax = ctx.frangi()
    before = ctx.get_frangi()
    ctx.auto_threshold("otsu")
    ctx.local_threshold(3)
    assert np.array_equal(ctx.get_volume(), img)
    after = ctx.get_frangi()  # the Frangi state is still there
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert ctx.frangi() == (jmin, jmax)
    ctx.close()


def test_errors(ctxs):
    L = lib.load()
    import ctypes as C
    fresh = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    o, info = lib.ThresholdOpts(1, 0, 0, 0), lib.ThresholdInfo()
    assert L.pnr_auto_threshold(fresh.h, C.byref(o), C.byref(info), None) == -4 and L.pnr_last_error() == b"pnr_auto_threshold: no volume set"
    bad = lib.ThresholdOpts(7, 0, 0, 0)
    assert L.pnr_auto_threshold(fresh.h, C.byref(bad), C.byref(info), None) == -1 and L.pnr_last_error() == b"pnr_auto_threshold: method = 7 outside [0, 4]"
    lo, linfo = lib.LocalOpts(3, 0, 256, 1, 0, 0), lib.LocalInfo()
    assert L.pnr_local_threshold(fresh.h, C.byref(lo), C.byref(linfo), None) == -4 and L.pnr_last_error() == b"pnr_local_threshold: no volume set"
    assert L.pnr_local_threshold_volume(fresh.h, C.byref(lo), None) == -4 and L.pnr_last_error() == b"pnr_local_threshold_volume: no volume set"
    fresh.close()
    ctx = ctxs[2.0]
    V = volume((5, 67, 131), "sparse")
    ctx.set_volume(V)
    who = "pnr_local_threshold_volume: "
    for kw, text in ((dict(r=0), "r = 0 outside [1, 64]"), (dict(r=65), "r = 65 outside [1, 64]"), (dict(r=3, offset=256), "offset = 256 outside [-255, 255]"),
                     (dict(r=3, offset=-256), "offset = -256 outside [-255, 255]"), (dict(r=3, scale_256=4097), "scale_256 = 4097 outside [0, 4096]"),
                     (dict(r=3, scale_256=-1), "scale_256 = -1 outside [0, 4096]"), (dict(r=3, floor=0), "floor = 0 outside [1, 255]"),
                     (dict(r=3, floor=256), "floor = 256 outside [1, 255]")):
        with pytest.raises(pnr_amd.PnrError) as e:
            ctx.local_threshold_volume(**kw)
        assert who + text in str(e.value) and "error -1" in str(e.value), str(e.value)
    bin2 = lib.LocalOpts(3, 0, 256, 1, 2, 0)
    assert L.pnr_local_threshold(ctx.h, C.byref(bin2), None, None) == -1 and L.pnr_last_error() == b"pnr_local_threshold: binary = 2, not 0 or 1"
    assert L.pnr_local_threshold(ctx.h, None, None, None) == -1 and L.pnr_last_error() == b"null argument"
    assert np.array_equal(ctx.get_volume(), V)  # every failure left the volume


# ---- the local threshold ----
@pytest.mark.parametrize("zd", ZDS)
@pytest.mark.parametrize("r", (1, 3, 64))
@pytest.mark.parametrize("shape", LOCAL_SHAPES, ids=sid)
def test_local_threshold_equals_the_restatement(ctxs, shape, r, zd):
    ctx = ctxs[zd]
    tap = shape[1] < 2 or shape[2] < 2  # below the 2 x 2 x 1 of a context's volume: the same kernels through their test tap
    for kind in ("sparse", "uniform"):
        V = volume(shape, kind)
        if not tap:
            ctx.set_volume(V)
        for combo in COMBOS if kind == "sparse" else COMBOS[:2]:
            info, got = ctx.tap_local_threshold(V, r, *combo) if tap else ctx.local_threshold(r, *combo)
            want, winfo = want_local(shape, kind, r, zd, combo)
            assert np.array_equal(got, want), (shape, kind, r, zd, combo, differs(got, want))
            assert info == winfo, (shape, kind, r, zd, combo)
        if not tap:
            assert np.array_equal(ctx.get_volume(), V)


def test_the_tap_is_the_call(ctxs):
    ctx = ctxs[2.0]
    V = volume((5, 67, 131), "sparse")
    ctx.set_volume(V)
    a, b = ctx.local_threshold(3, 5, 260), ctx.tap_local_threshold(V, 3, 5, 260)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(ctx.auto_threshold("mean", hist=True)[1], ctx.tap_histogram(V))


def test_local_threshold_largest_partial_sums(ctxs):
    """129^3 voxels of 255 under the box of R = 64 at zdist 1: the centre voxel's x sum is 129 * 255 (u16), its x-y sum 129^2 * 255 and
    its box sum 129^3 * 255 (u32)"""
    ctx = ctxs[1.0]
    shape = (129, 129, 129)
    ctx.set_volume(volume(shape, "full"))
    for combo in ((0, 256, 1, False), (1, 256, 1, False), (0, 257, 1, True), (-255, 4096, 1, False)):
        info, got = ctx.local_threshold(64, *combo)
        want, winfo = want_local(shape, "full", 64, 1.0, combo)
        assert np.array_equal(got, want) and info == winfo, (combo, info, winfo)
    assert int(sums(shape, "full", 64, 1.0)[1].max()) == 129**3 * 255


@pytest.mark.parametrize("r,zd", [(1, 1.0), (3, 1.0), (64, 2.0), (3, 3.7)])
def test_local_threshold_slab_boundaries(ctxs, r, zd):
    """option lt_slab_vox lowers the slab of LT_SLAB_VOX voxels: slabs of one, two and three planes of a stack of 7 (the ring of x-y sums
    wraps, the running sums are carried from slab to slab; with R = 64 the box is deeper than the stack), the same bytes"""
    ctx = ctxs[zd]
    shape = (7, 19, 23)
    plane = shape[1] * shape[2]
    V = volume(shape, "sparse")
    ctx.set_volume(V)
    try:
        for vox in (1, plane, 2 * plane, 3 * plane + 1, 7 * plane):
            ctx.set_option("lt_slab_vox", vox)
            for combo in COMBOS[:3]:
                info, got = ctx.local_threshold(r, *combo)
                want, winfo = want_local(shape, "sparse", r, zd, combo)
                assert np.array_equal(got, want) and info == winfo, (vox, combo, differs(got, want))
    finally:
        ctx.set_option("lt_slab_vox", 0)


def test_local_threshold_one_plane_more_than_a_slab(ctxs):
    """planes of 512 x 512: LT_SLAB_VOX / 2^18 planes are a slab, the stack has one more"""
    ctx = ctxs[1.0]
    planes = SLAB_VOX // (512 * 512)
    assert planes * 512 * 512 == SLAB_VOX and planes >= 4
    shape = (planes + 1, 512, 512)
    ctx.set_volume(volume(shape, "uniform"))
    combo = (5, 260, 1, False)
    info, got = ctx.local_threshold(3, *combo)
    want, winfo = want_local(shape, "uniform", 3, 1.0, combo)
    assert np.array_equal(got, want) and info == winfo, differs(got, want)
    sums.cache_clear()


def test_local_threshold_volume_form(ctxs):
    """the result becomes the context's own volume: a borrowed tensor is never written, the Frangi state is gone, and a second call
    filters the filtered bytes"""
    import torch
    ctx = pnr_amd.Context(pnr_amd.make_params(sigmas=(2, 3), zdist=2, np_=20), 0)
    shape = (5, 67, 131)
    V = volume(shape, "sparse")
    t = torch.from_numpy(V.copy()).cuda()
    ctx.set_volume_device(t.data_ptr(), shape, keepalive=t)
    ctx.frangi()
    ctx.get_frangi()
    info = ctx.local_threshold_volume(3, 5, 260)
    want, winfo = ref.local(V, 3, 2.0, 5, 260)
    assert info == winfo and 0 < info["n_kept"] < V.size
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), V)
    t.zero_()  # the context's volume is its own
    torch.cuda.synchronize()
    assert np.array_equal(ctx.get_volume(), want)
    with pytest.raises(pnr_amd.PnrError, match="error -4"):  # PNR_E_STATE: the Frangi state is gone
        ctx.get_frangi()
    info2 = ctx.local_threshold_volume(1, 0, 256, binary=True)
    want2, winfo2 = ref.local(want, 1, 2.0, 0, 256, 1, True)
    assert info2 == winfo2 and np.array_equal(ctx.get_volume(), want2)
    ctx.frangi()
    ctx.close()


# ---- the stack above 2^31 voxels ----
@pytest.fixture(scope="module")
def big():
    import bigvol
    rng = np.random.default_rng(17)
    near, far = (np.where(rng.random(s) < 0.7, rng.integers(60, 256, s), rng.integers(0, 30, s)).astype(np.uint8) for s in (bigvol.NEAR, bigvol.FAR))
    far[-1, -1, -1] = 250

    def make(shape):
        blocks = bigvol._blocks(shape, near, far)
        t, c = bigvol.open_stack(blocks, shape)
        return blocks, t, c
    return make


@pytest.mark.parametrize("which", ("SMALL", "SHAPE"))
def test_histogram_and_local_threshold_above_2_to_31(big, which):
    """2048 x 2048 x 513 voxels, zero but for two blocks, the far one in the last plane (voxel indices above 2^31): the histogram's
    bin 0 holds more than 2^31 voxels; the local threshold's bytes are the restatement's on crops of R around the blocks (cut at the
    stack's faces, which cut the boxes there too) and zero elsewhere, since floor >= 1.  Also at bigvol.SMALL, where numpy restates
    the whole stack."""
    import bigvol
    shape = getattr(bigvol, which)
    blocks, t, ctx = big(shape)
    N = int(np.prod(shape, dtype=np.int64))
    want_h = np.zeros(256, np.uint64)
    for _, B in blocks:
        want_h += ref.histogram(B)
    want_h[0] += np.uint64(N - sum(B.size for _, B in blocks))
    info, H = ctx.auto_threshold("otsu", 1, hist=True)
    assert np.array_equal(H, want_h) and info == ref.from_hist(want_h, "otsu", 1)
    if which == "SHAPE":
        assert int(H[0]) > 2**31
    R, combo = 8, (3, 300, 1, False)
    linfo = ctx.local_threshold_volume(R, *combo)
    assert bigvol.untouched(t, blocks)
    got = ctx.get_volume()
    kept = sum_out = 0
    for C, o in bigvol.crops(blocks, shape, margin=R):
        want, wi = ref.local(C, R, bigvol.ZD, *combo)
        sl = tuple(slice(a, a + n) for a, n in zip(o, C.shape))
        assert np.array_equal(got[sl], want), (which, o, differs(got[sl], want))
        kept, sum_out = kept + wi["n_kept"], sum_out + wi["sum_out"]
    assert kept > 0 and int(np.count_nonzero(got)) == kept  # zero elsewhere
    assert linfo == dict(n_vox=N, n_kept=kept, sum_in=int(sum(int(B.sum(dtype=np.int64)) for _, B in blocks)), sum_out=sum_out, rx=R, ry=R, rz=4)
    if which == "SMALL":
        whole = bigvol.whole(blocks, shape)
        assert np.array_equal(got, ref.local(whole, R, bigvol.ZD, *combo)[0])
    ctx.close()
    del t


# ---- threshold words where a number is taken ----
def test_threshold_words_in_the_python_tools(ctxs, oracle):
    ctx = ctxs[2.0]
    img = synth.synth(48, 40, 24, seed=1, zdist=2.0)
    ctx.set_volume(img)
    for word in ("otsu", "triangle:1", "top1.5", "maxentropy", "mean"):
        t = ref.resolve(img, word, oracle.orc_maxentropy_hist)
        a, b = ctx.label_components(thr=word), ctx.label_components(thr=t)
        assert a[0] == b[0] and a[0]["thr_used"] == t and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), word
    t = ref.resolve(img, "otsu")
    assert t != max(1, int(img.sum(dtype=np.int64)) // img.size)
    a, b = ctx.distance_transform(thr="otsu"), ctx.distance_transform(thr=t)
    assert a[0] == b[0] and a[0]["thr_used"] == t and np.array_equal(a[1], b[1])
    a, b = ctx.skeletonize(thr="otsu"), ctx.skeletonize(thr=t)
    assert a[0] == b[0] and a[0]["thr_used"] == t and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    with pytest.raises(ValueError):
        ctx.label_components(thr="isodata")


# ---- the CLI ----
def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    img = synth.synth(48, 40, 24, seed=1, zdist=2.0)
    path = str(tmp_path_factory.mktemp("thr") / "stack.raw")
    img.tofile(path)
    l, h, w = img.shape
    return img, path, f"{w},{h},{l}"


COMPONENT_KEYS = ["n_vox", "n_fg", "n_comp", "n_small", "vox_small", "largest", "thr_used"]


def test_cli_threshold_word(stack):
    """--components --threshold otsu == --threshold <the restatement's number>, but for thr_method; the line of the run with a number has
    the keys it always had, and the word's line is that line with thr_method in front of the brace"""
    img, path, dims = stack
    t = ref.resolve(img, "otsu")
    word = _cli("--components", "--threshold", "otsu", "-i", path, "-d", dims)
    number = _cli("--components", "--threshold", str(t), "-i", path, "-d", dims)
    assert word.returncode == 0 and number.returncode == 0, (word.stderr, number.stderr)
    a, b = json.loads(word.stdout), json.loads(number.stdout)
    assert list(b) == COMPONENT_KEYS and b["thr_used"] == t and b["n_fg"] == int((img >= t).sum())
    assert a.pop("thr_method") == "otsu" and a == b
    assert word.stdout == number.stdout.replace("}", ', "thr_method": "otsu"}')
    mean = _cli("--components", "-i", path, "-d", dims)
    assert list(json.loads(mean.stdout)) == COMPONENT_KEYS and json.loads(mean.stdout)["thr_used"] == ref.resolve(img, "mean")
    lo1 = json.loads(_cli("--skeleton", "--threshold", "top1.5:1", "-i", path, "-d", dims).stdout)
    assert lo1["thr_method"] == "top1.5:1" and lo1["thr_used"] == ref.resolve(img, "top1.5:1")
    for bad in ("isodata", "top", "top0", "top100", "otsu:256", "otsu:"):
        r = _cli("--components", "--threshold", bad, "-i", path, "-d", dims)
        assert (r.returncode, r.stderr) == (1, "--threshold T: an integer from 0 to 255, or -1 for the stack's mean\n"), bad


def test_cli_auto_threshold(stack, oracle, tmp_path):
    img, path, dims = stack
    H = ref.histogram(img)
    for lo in (0, 1):
        csv = str(tmp_path / f"h{lo}.csv")
        r = _cli("--auto-threshold", "-i", path, "-d", dims, "--threshold-lo", str(lo), "--histogram", csv)
        assert r.returncode == 0, r.stderr
        got = json.loads(r.stdout)
        want = {"w": 48, "h": 40, "l": 24, "n_vox": img.size, "lo": lo}
        for key, method, mlo, ppm in (("mean", "mean", lo, None), ("otsu", "otsu", lo, None), ("triangle", "triangle", lo, None), ("maxentropy", "maxentropy", 0, None),
                                      ("top1", "top", lo, 10000)):
            i = ref.from_hist(H, method, mlo, ppm, oracle.orc_maxentropy_hist)
            want[key] = {"thr": i["thr"], "n_fg": i["n_fg"]}
        assert got == want and list(got) == list(want)
        rows = open(csv).read().splitlines()
        assert rows[0] == "v,count" and rows[1:] == [f"{v},{int(H[v])}" for v in range(256)]
    assert len({got[k]["thr"] for k in ("mean", "otsu", "top1")}) == 3
    r = _cli("--threshold-lo", "1", "-i", path, "-d", dims)
    assert (r.returncode, r.stderr) == (1, "--threshold-lo / --histogram need --auto-threshold -i stack\n")


def test_cli_local_threshold_in_a_tracing_run(stack, tmp_path):
    """--local-threshold 8,5 while tracing: #local= with the restatement's count behind the other set-up lines; none without the flag;
    --morph-out shows the bytes the run traced"""
    img, path, dims = stack
    tail = ("-f", "advantra_func", "-p", *"2,3 0 5 0.3 3 2 40 50 2 4 5".split())
    want, winfo = ref.local(img, 8, 2.0, 5, 256)
    r = _cli("--local-threshold", "8,5", "-i", path, "-d", dims, *tail)
    assert r.returncode == 0, r.stderr[-1500:]
    comments = [ln for ln in open(path + "_Advantra.swc").read().splitlines() if ln.startswith("#")]
    assert f"#local=r:8,offset:5,scale:256,kept:{winfo['n_kept']}" in comments and 0 < winfo["n_kept"] < img.size
    assert "local threshold... box 8 x 8 x 4, offset 5, scale 256/256" in r.stdout
    r = _cli("-i", path, "-d", dims, *tail)
    assert r.returncode == 0 and "#local" not in open(path + "_Advantra.swc").read() and "local threshold" not in r.stdout
    # the tool modes take the stage too: the components of the thresholded bytes (zdist = 2 through --zscale)
    got = json.loads(_cli("--components", "--threshold", "1", "--local-threshold", "8,5", "--local-binary", "--zscale", "2", "-i", path, "-d", dims).stdout)
    assert got["n_fg"] == winfo["n_kept"]
    r = _cli("--local-binary", "-i", path, "-d", dims, *tail)
    assert (r.returncode, r.stderr) == (1, "--local-binary needs --local-threshold R\n")
