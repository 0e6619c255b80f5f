"""SWC node radii measured from the image on the GPU (pnr_measure_radii, Context.measure_radii, advantra_cli --measure-radius): the
rule of include/pnr_hip.h restated in numpy (radius_ref.py), closed forms on solid cylinders and balls, a fuzz over volumes,
geometries, positions and options, the pipeline and the CLI.  Every comparison is exact."""
import ctypes as C
import itertools
import os
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import radius_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
F = np.float32


def context(zdist=2.0, **kw):
    return pnr_amd.Context(pnr_amd.make_params(sigmas=(2,), zdist=zdist, **kw), 0)


def check(ctx, V, zd, xyz, sh=None, **opts):
    """the device's k and thr_used against the restatement's; returns k"""
    k, t = ctx.measure_radii(xyz, **opts)
    want, t_want = radius_ref.measure(V, zd, xyz, sh=sh, **opts)
    print(f"zd={zd} shape={V.shape} n={len(k)} opts={opts} thr_used={t} (want {t_want}) mismatches={int((k != want).sum())} hist={np.bincount(k[k >= 0], minlength=1)[:16].tolist()}")
    assert t == t_want and k.dtype == np.int32
    assert np.array_equal(k, want), (opts, np.flatnonzero(k != want)[:5], k[k != want][:5], want[k != want][:5])
    return k


# ---- closed forms: do not depend on the restatement ----
RADII = (1, 1.5, 2.5, 3.5, 6, 11.2)


@pytest.mark.parametrize("zd", [1, 2, 4])
def test_closed_form_cylinders_and_balls(zd):
    """solid objects at value 200, thr = 100, bg_permille = 0, centres on the axis.  Axis-aligned cylinder (along x) and ball
    (z half-axis in xy units): every ball of radius k <= R is foreground and the offset (0, floor(R) + 1, 0) resp. (floor(R) + 1, 0, 0)
    is background, so k* = min(floor(R), rmax).  A cylinder along the in-plane direction (3, 4) / 5: the same argument gives
    k* >= min(floor(R), rmax) (there need not be a lattice offset at distance floor(R) + 1 across an oblique axis)."""
    ctx = context(zd)
    w, h, l = 56, 52, 2 * (12 // zd + 2) + 1
    cx, cy, cz = 27, 25, l // 2
    z, y, x = np.meshgrid(np.arange(l), np.arange(h), np.arange(w), indexing="ij")
    zz = (zd * (z - cz)) ** 2
    for R in RADII:
        solids = {
            "cyl_x": ((y - cy) ** 2 + zz <= R * R, [[0, cy, cz], [7.3, cy + 0.2, cz - 0.4], [cx, cy, cz], [w - 1, cy, cz], [w + 5, cy, cz]]),
            "ball": ((x - cx) ** 2 + (y - cy) ** 2 + zz <= R * R, [[cx, cy, cz], [cx + 0.49, cy - 0.5, cz + 0.3]]),
            "cyl_34": ((-4 * (x - cx) + 3 * (y - cy)) ** 2 + 25 * zz <= 25 * R * R, [[cx + 3 * m, cy + 4 * m, cz] for m in (-5, -2, 0, 1, 4)]),
        }
        for name, (mask, pos) in solids.items():
            V = np.where(mask, 200, 0).astype(np.uint8)
            ctx.set_volume(V)
            for rmax in (32, 7, 2):
                k, t = ctx.measure_radii(pos, thr=100, rel_pct=0, rmax=rmax, bg_permille=0)
                want = np.full(len(pos), min(int(R), rmax), np.int32)
                print(f"zd={zd} R={R} {name} rmax={rmax}: k={k.tolist()} closed form {'>=' if name == 'cyl_34' else '=='} {want[0]}")
                assert t == 100
                if name == "cyl_34":
                    assert np.array_equal(np.maximum(k, want), k), (zd, R, name, rmax, k)
                    assert np.array_equal(k, radius_ref.measure(V, zd, pos, thr=100, rel_pct=0, rmax=rmax, bg_permille=0)[0])
                else:
                    assert np.array_equal(k, want), (zd, R, name, rmax, k)
    ctx.close()


# ---- fuzz against the restatement ----
MODES = [dict(rel_pct=0, thr=t) for t in (-1, 0, 1, 37, 255)] + [dict(rel_pct=p) for p in (1, 50, 100)]
BGS = (0, 1, 50, 500, 999)
RMAXS = (1, 7, 32, 64)
GEOMS = [("3d", 1.0), ("3d", 2.0), ("3d", 2.5), ("3d", 4.0), ("2d", 2.0)]


def volumes(is2d):
    rng = np.random.default_rng(11)
    v = {
        "noise": rng.integers(0, 256, (20, 36, 40), dtype=np.uint8),
        "synth": synth.synth(48, 40, 24, seed=3),
        "zero": np.zeros((10, 18, 16), np.uint8),
        "full": np.full((10, 18, 16), 255, np.uint8),
        "ragged": rng.integers(0, 256, (3, 5, 7), dtype=np.uint8),
    }
    if not is2d:
        return v
    v = {k: np.ascontiguousarray(a.max(0, keepdims=True)) for k, a in v.items()}
    v["tiny"] = np.array([[[0, 200], [90, 255]]], np.uint8)
    return v


def positions(rng, shape, per_kind):
    """uniform in the volume (up to half a voxel outside), on faces / edges / corners, far outside, not finite, exactly on .5"""
    l, h, w = shape
    ext = np.array([w, h, l], F)
    n = per_kind
    uni = rng.random((n, 3)).astype(F) * (ext + F(1)) - F(1)
    face = rng.random((n, 3)).astype(F) * ext
    for i in range(n):  # 1, 2 or 3 coordinates on a face
        for a in rng.choice(3, 1 + i % 3, replace=False):
            face[i, a] = rng.choice([0, ext[a] - 1])
    far = rng.random((n, 3)).astype(F) * ext
    for i in range(n):
        far[i, rng.integers(3)] = rng.choice([F(1e9), F(-1e9), F(3e38), F(-3e38), ext[0] + F(64), F(-65)])
    bad = rng.random((n, 3)).astype(F) * ext
    for i in range(n):
        bad[i, rng.integers(3)] = [np.nan, np.inf, -np.inf][i % 3]
    half = np.floor(rng.random((n, 3)).astype(F) * (ext + F(2))) - F(1.5)
    return np.concatenate([uni, face, far, bad, half]).astype(F)


@pytest.mark.parametrize("mode,zd", GEOMS, ids=[f"{m}-zd{z}" for m, z in GEOMS])
def test_fuzz_against_the_restatement(mode, zd):
    """every (threshold mode, bg_permille, rmax) triple of the grid is dealt to the (geometry, volume) cases in turn: each geometry
    sees all 160 triples spread over its volumes"""
    is2d = mode == "2d"
    triples = list(itertools.product(range(len(MODES)), BGS, RMAXS))
    np.random.default_rng(5).shuffle(triples)
    vols = volumes(is2d)
    ctx = context(zd)
    shells = {r: radius_ref.shells(zd, r, is2d) for r in RMAXS}
    rng = np.random.default_rng(int(zd * 10) + is2d)
    measured = 0
    for i, (m, bg, rmax) in enumerate(triples):
        name = list(vols)[i % len(vols)]
        V = vols[name]
        ctx.set_volume(V)
        xyz = positions(rng, V.shape, 3 if rmax == 64 else 8)
        k = check(ctx, V, zd, xyz, sh=shells[rmax], rmax=rmax, bg_permille=bg, **MODES[int(m)])
        assert (k[-2 * (len(k) // 5):-(len(k) // 5)] == -1).all()  # the positions that are not finite
        measured += int((k >= 0).sum())
    assert measured > 1000
    ctx.close()


def test_large_case_device_volume_and_order():
    """20 000 positions in a 256^3 synth stack that stays on the device (borrowed: set_volume_device), rmax = 12: half of them near
    bright voxels; a permutation of the positions gives the permuted output; the same from an owned copy of the volume"""
    import torch
    t = synth.synth_torch(256, 256, 256, seed=4, zdist=2.0)
    V = t.cpu().numpy()
    ctx = context(2.0)
    torch.cuda.synchronize()
    ctx.set_volume_device(t.data_ptr(), V.shape, keepalive=t)
    rng = np.random.default_rng(6)
    uni = rng.random((10000, 3)).astype(F) * F(256) - F(0.5)
    zyx = np.argwhere(V > 80)
    pick = zyx[rng.choice(len(zyx), 10000)]
    near = pick[:, ::-1].astype(F) + (rng.random((10000, 3)).astype(F) - F(0.5)) * F(3)
    xyz = np.concatenate([uni, near])
    sh = radius_ref.shells(2.0, 12)
    k = check(ctx, V, 2.0, xyz, sh=sh, rmax=12)
    assert (k >= 2).sum() > 500 and k.max() <= 12
    k_abs = check(ctx, V, 2.0, xyz, sh=sh, rmax=12, rel_pct=0, thr=-1, bg_permille=50)
    perm = rng.permutation(len(xyz))
    assert np.array_equal(ctx.measure_radii(xyz[perm], rmax=12)[0], k[perm])
    ctx.set_volume(V)  # an owned copy
    assert np.array_equal(ctx.measure_radii(xyz, rmax=12)[0], k)
    assert np.array_equal(ctx.measure_radii(xyz, rmax=12, rel_pct=0, thr=-1, bg_permille=50)[0], k_abs)
    ctx.close()


def test_threshold_used():
    """thr_used: max(1, sum // N) in the mean mode (1 on an all-zero volume), the given thr in the absolute mode, 0 in the relative
    mode; n = 0 is valid and still reports it; odd sizes and a volume pointer that is not 16-byte aligned"""
    import torch
    ctx = context()
    rng = np.random.default_rng(7)
    for shape in ((1, 2, 2), (3, 5, 7), (9, 31, 33), (40, 100, 101)):
        for V in (rng.integers(0, 256, shape, dtype=np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8),
                  (rng.random(shape) < 0.01).astype(np.uint8) * 255):
            ctx.set_volume(V)
            mean = max(1, int(V.sum(dtype=np.uint64)) // V.size)
            none = np.zeros((0, 3), F)
            k, t = ctx.measure_radii(none, thr=-1, rel_pct=0)
            assert len(k) == 0 and t == mean, (shape, t, mean)
            assert ctx.measure_radii(none, thr=37, rel_pct=0)[1] == 37 and ctx.measure_radii(none, thr=0, rel_pct=0)[1] == 0
            assert ctx.measure_radii(none, thr=37, rel_pct=50)[1] == 0
            assert ctx.measure_radii([[1, 1, 0]], thr=-1, rel_pct=0)[1] == mean
    ctx.set_volume(np.zeros((4, 6, 8), np.uint8))
    assert ctx.measure_radii(np.zeros((0, 3), F), thr=-1, rel_pct=0)[1] == 1
    V = rng.integers(0, 256, (7, 19, 23), dtype=np.uint8)
    for shift in (1, 5, 15):  # a borrowed volume that starts off a 16-byte boundary: the sum's scalar head and tail
        flat = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), V.ravel()])).cuda()
        torch.cuda.synchronize()
        ctx.set_volume_device(flat.data_ptr() + shift, V.shape, keepalive=flat)
        xyz = rng.random((50, 3)).astype(F) * np.array([23, 19, 7], F)
        check(ctx, V, 2.0, xyz, thr=-1, rel_pct=0, rmax=7)
    ctx.close()


def test_windowed_u16_volume_stream_and_timer():
    """a 16-bit stack is measured on the windowed bytes (get_volume); a non-default stream gives the same results; the "radius"
    kernel-time group counts the sum and the measurement"""
    import torch
    img8 = synth.synth(64, 56, 32, seed=2)
    x = (img8.astype(np.uint16) * 15 + 40 + np.random.default_rng(8).integers(0, 15, img8.shape)).astype(np.uint16)
    ctx = context()
    ctx.set_volume(x, window={"saturate": (0, 0.35)})
    V = ctx.get_volume()
    assert V.dtype == np.uint8 and V.max() == 255
    rng = np.random.default_rng(9)
    zyx = np.argwhere(V > 60)
    xyz = zyx[rng.choice(len(zyx), 400)][:, ::-1].astype(F) + (rng.random((400, 3)).astype(F) - F(0.5))
    k = check(ctx, V, 2.0, xyz)
    k_abs = check(ctx, V, 2.0, xyz, thr=-1, rel_pct=0, bg_permille=50)
    assert (k >= 1).sum() > 50
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    assert np.array_equal(ctx.measure_radii(xyz)[0], k)
    assert np.array_equal(ctx.measure_radii(xyz, thr=-1, rel_pct=0, bg_permille=50, rmax=9)[0], np.minimum(k_abs, 9))
    ctx.set_stream(None)
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("radius") == (0.0, 0)
    ctx.measure_radii(xyz)
    ms, launches = ctx.kernel_ms("radius")
    assert ms > 0 and launches == 1, (ms, launches)
    ctx.measure_radii(xyz, thr=-1, rel_pct=0)
    ms2, launches = ctx.kernel_ms("radius")
    assert ms2 > ms and launches == 3, (ms2, launches)  # + the sum and the measurement
    ctx.close()


def test_shell_table_cache():
    """one context keeps one shell table: rmax 8, 12, 8 again, then the 2-D table of a one-slice volume and the 3-D one once more, each
    call equal to a fresh context's that does only that call; the third call holds the device bytes of the first (one table, nothing
    else left behind), and close returns everything"""
    import gc

    def live():
        gc.collect()
        return lib.live_bytes()[0]

    V = synth.synth(40, 40, 40, seed=6)
    S = np.ascontiguousarray(V[20:21])
    rng = np.random.default_rng(12)
    xyz = rng.random((50, 3)).astype(F) * F(40) - F(0.5)
    opts = dict(thr=-1, rel_pct=0, bg_permille=800)  # balls that grow until four fifths of them lie below the mean: the tables differ in k

    def fresh(vol, rmax):
        c = context()
        c.set_volume(vol)
        k, t = c.measure_radii(xyz, rmax=rmax, **opts)
        c.close()
        return k, t

    want = {(name, rmax): fresh(vol, rmax) for name, vol, rmax in (("3d", V, 8), ("3d", V, 12), ("2d", S, 8))}
    print({key: np.bincount(k, minlength=13).tolist() for key, (k, _) in want.items()})
    assert not np.array_equal(want["3d", 8][0], want["3d", 12][0]) and not np.array_equal(want["3d", 8][0], want["2d", 8][0])
    d0 = live()
    ctx = context()
    ctx.set_volume(V)
    held = []
    for name, vol, rmax in (("3d", None, 8), ("3d", None, 12), ("3d", None, 8), ("2d", S, 8), ("3d", V, 8)):
        if vol is not None:
            ctx.set_volume(vol)
        k, t = ctx.measure_radii(xyz, rmax=rmax, **opts)
        held.append(live() - d0)
        print(f"{name} rmax={rmax}: device bytes held {held[-1]}")
        assert t == want[name, rmax][1] and np.array_equal(k, want[name, rmax][0]), (name, rmax)
    assert held[2] == held[0]
    ctx.close()
    assert live() == d0


def test_errors_leave_the_context_working():
    """no volume: PNR_E_STATE; every option outside its range: PNR_E_ARG; after each the context measures as before"""
    L = lib.load()
    ctx = context()
    xyz = np.array([[3, 4, 2], [10.2, 8.7, 5.1]], F)
    k = np.zeros(2, np.int32)
    t = C.c_int32()

    def call(opts, n=2, pos=xyz, out=k):
        o = lib.RadiusOpts(*opts) if opts is not None else None
        return L.pnr_measure_radii(ctx.h, pos.ctypes.data if pos is not None else None, n, C.byref(o) if o is not None else None,
                                   out.ctypes.data if out is not None else None, C.byref(t))

    assert call(None) == -4 and b"no volume" in L.pnr_last_error()
    assert call((-1, 50, 0, 1)) == -1  # arguments are checked first
    V = synth.synth(32, 24, 12, seed=5)
    ctx.set_volume(V)
    want, _ = radius_ref.measure(V, 2.0, xyz)
    assert call(None) == 0 and np.array_equal(k, want) and t.value == 0  # NULL options = {-1, 50, 32, 1}
    bad = [(-1, 50, 0, 1), (-1, 50, 65, 1), (-2, 50, 32, 1), (256, 50, 32, 1), (-1, -1, 32, 1), (-1, 101, 32, 1), (-1, 50, 32, -1), (-1, 50, 32, 1000)]
    for opts in bad:
        k[:] = 77
        assert call(opts) == -1, (opts, L.pnr_last_error())
        assert (k == 77).all()
        assert np.array_equal(ctx.measure_radii(xyz)[0], want)
    assert call(None, n=-1) == -1 and call(None, pos=None) == -1 and call(None, out=None) == -1
    assert call(None, n=0, pos=None, out=None) == 0
    assert L.pnr_measure_radii(None, xyz.ctypes.data, 2, None, k.ctypes.data, None) == -1
    for opts in ((255, 0, 64, 999), (0, 0, 1, 0), (-1, 100, 64, 0), (-1, 1, 1, 999)):  # the ends of the ranges are valid
        assert call(opts) == 0, (opts, L.pnr_last_error())
        assert np.array_equal(k, radius_ref.measure(V, 2.0, xyz, thr=opts[0], rel_pct=opts[1], rmax=opts[2], bg_permille=opts[3])[0]), opts
    ctx.close()


def test_pipeline_state_is_left_alone():
    """frangi -> seeds -> trace_replay -> reconstruct, the tree's nodes measured, frangi and the seeds once more: unchanged; and the
    measurement needs none of them (a fresh context with only a volume gives the same k)"""
    img = synth.synth(64, 56, 32, seed=2)
    p = pnr_amd.make_params(sigmas=[2, 3], tolerance=5, znccth=0.3, kappa=3, step=2, ni=40, np_=50, zdist=2, nodepervol=4, vol=5)
    ctx = pnr_amd.Context(p, 0)
    ctx.set_volume(img)
    jmin, jmax = ctx.frangi()
    seeds_init = ctx.extract_seeds()
    seeds = ctx.score_filter_sort(seeds_init)
    nodes, links, ntr, _ = ctx.trace_replay(seeds)
    tree, parent = ctx.reconstruct(nodes, links)
    assert len(tree) > 50
    xyz = np.stack([tree["x"], tree["y"], tree["z"]], 1)[1:]
    k = check(ctx, img, 2.0, xyz)
    k1 = check(ctx, img, 2.0, xyz, thr=-1, rel_pct=0, bg_permille=50)
    assert (k >= 1).sum() > len(k) // 4 and len(np.unique(k)) >= 3  # measured radii, not two or three scale values
    nodes2, links2 = ctx.get_graph()
    assert nodes2.tobytes() == nodes.tobytes() and np.array_equal(links2, links)
    assert np.array_equal(ctx.extract_seeds(), seeds_init)  # (the seeds of the J8 that is still in HBM)
    assert ctx.frangi() == (jmin, jmax)
    assert np.array_equal(ctx.extract_seeds(), seeds_init) and np.array_equal(ctx.score_filter_sort(seeds_init), seeds)
    fresh = pnr_amd.Context(p, 0)
    fresh.set_volume(img)
    assert np.array_equal(fresh.measure_radii(xyz)[0], k) and np.array_equal(fresh.measure_radii(xyz, thr=-1, rel_pct=0, bg_permille=50)[0], k1)
    fresh.close()
    ctx.close()


# ---- the CLI ----
def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def _save8(path, x):
    from PIL import Image
    pages = [Image.fromarray(z) for z in x]
    pages[0].save(path, save_all=True, append_images=pages[1:], compression=None)


def _parse(text):
    lines = text.splitlines()
    return [ln for ln in lines if ln.startswith("#")], [ln.split() for ln in lines if ln and not ln.startswith("#")]


def _column(tree, k, plain_rows):
    """the radius column of a measured file: k* >= 1 -> k*, 0 -> 0.5; soma nodes (type 1) and k = -1 keep the unmeasured text"""
    out = []
    for i, row in enumerate(plain_rows):
        out.append(row[5] if tree["type"][i + 1] == 1 or k[i] < 0 else (f"{k[i]:.3f}" if k[i] >= 1 else "0.500"))
    return out


@pytest.mark.parametrize("case", ["plain", "soma"])
def test_cli_measure_radius(tmp_path, case):
    """the same TIFF with and without --measure-radius: the unflagged file is reproducible byte for byte; the flagged file has the same
    ids, types, coordinates and parents, one more comment line at the end of the block, and the radius column of Context.measure_radii
    at the tree's positions (the Python pipeline's tree: its %.3f coordinates are the file's); soma lines keep their radius;
    other options, --single-tree, --save-midres and the sharded path"""
    img = synth.synth(64, 56, 32, seed=2)
    if case == "soma":
        img = synth.add_somas(img, ((20, 28, 16, 6), (48, 20, 14, 5)))
        paras, kw = "2,3 3 5 0.3 3 2 25 40 2 4 1".split(), dict(somaradius=3, ni=25, np_=40, vol=1)
    else:
        paras, kw = "2,3 0 5 0.3 3 2 40 50 2 4 5".split(), dict(ni=40, np_=50, vol=5)
    tif = str(tmp_path / "stack.tif")
    _save8(tif, img)
    swc = tif + "_Advantra.swc"
    tail = ("-f", "advantra_func", "-i", tif, "-p", *paras)

    def run(*flags, out=swc):
        r = _cli(*flags, *tail)
        assert r.returncode == 0, r.stderr[-1500:]
        return open(out).read(), r

    plain, r0 = run()
    again, _ = run()
    assert plain == again and "#radius=" not in plain and "radius measurement" not in r0.stdout
    flagged, r1 = run("--measure-radius", "--timing")
    assert "radius measurement..." in r1.stdout and "[pnr host] radius:" in r1.stderr
    c0, d0 = _parse(plain)
    c1, d1 = _parse(flagged)
    # one more line, the last of the comment block (c0[-1] is the column header "##n,type,...")
    assert c0[-1].startswith("##n,") and c1 == c0[:-1] + ["#radius=measured,thr=rel:50,rmax=32,bg=1"] + c0[-1:]
    assert len(d1) == len(d0) > 30
    assert [r[:5] + r[6:] for r in d1] == [r[:5] + r[6:] for r in d0]
    # the tree the CLI wrote, with its unrounded positions
    p = pnr_amd.make_params(sigmas=[2, 3], tolerance=5, znccth=0.3, kappa=3, step=2, zdist=2, nodepervol=4, **kw)
    ctx = pnr_amd.Context(p, 0)
    res = pnr_amd.advantra.run_pipeline(ctx, img)
    tree = res["tree"]
    assert len(tree) - 1 == len(d0)
    assert [[f"{tree[a][i + 1]:.3f}" for a in "xyz"] for i in range(len(d0))] == [r[2:5] for r in d0]
    xyz = np.stack([tree["x"], tree["y"], tree["z"]], 1)[1:]
    k, _ = ctx.measure_radii(xyz)
    assert np.array_equal(k, radius_ref.measure(img, 2.0, xyz)[0])
    assert [r[5] for r in d1] == _column(tree, k, d0)
    if case == "soma":
        somas = [i for i, r in enumerate(d0) if r[1] == "1"]
        assert somas and all(d1[i][5] == d0[i][5] for i in somas)
    # the flag had an effect: the scale radius (SIG2RADIUS * a mean of the scales) of a non-soma node is k* or 0.5 only by accident.
    # (How many lines change is the case's business: in the soma case most nodes are soma-typed and keep their radius.)
    changed = sum(a[5] != b[5] for a, b in zip(d1, d0))
    print(f"{case}: {changed} of {len(d0)} radius entries changed, {sum(r[1] == '1' for r in d0)} soma-typed lines")
    assert changed > 0 and all(a[5] == b[5] for a, b in zip(d1, d0) if b[1] == "1")
    # the absolute mode with the mean, another rmax and bg
    other, _ = run("--measure-radius", "--radius-threshold", "-1", "--radius-max", "5", "--radius-bg", "50")
    k2, mean = ctx.measure_radii(xyz, thr=-1, rel_pct=0, rmax=5, bg_permille=50)
    assert mean == max(1, int(img.sum(dtype=np.uint64)) // img.size)
    c2, d2 = _parse(other)
    assert c2 == c0[:-1] + [f"#radius=measured,thr={mean},rmax=5,bg=50"] + c0[-1:]
    assert [r[5] for r in d2] == _column(tree, k2, d0)
    rel, _ = run("--measure-radius", "--radius-rel", "30")
    assert [r[5] for r in _parse(rel)[1]] == _column(tree, ctx.measure_radii(xyz, rel_pct=30)[0], d0)
    # the sharded path: a world of one over RCCL, and two ranks sharing the GPU; rank 0 measures and writes
    for flags in (("--ranks", "1", "--exchange", "rccl"), ("--ranks", "2", "--share-gpu")):
        assert run(*flags, "--measure-radius")[0] == flagged, flags
        assert run(*flags)[0] == plain, flags
    if case == "plain":
        # --save-midres: the intermediate lists keep the scale radius; --single-tree: the kept tree is measured
        run("--save-midres")
        mid = {t: open(tif + t + ".swc").read() for t in ("_n0_", "_n0res_", "_n1_", "_n2_", "_n2tree_")}
        assert run("--save-midres", "--measure-radius")[0] == flagged
        assert all(open(tif + t + ".swc").read() == mid[t] for t in mid)
        one, _ = run("--single-tree", "--measure-radius", out=tif + "_Advantra1.swc")
        one_plain, _ = run("--single-tree", out=tif + "_Advantra1.swc")
        t1, _ = ctx.reconstruct(res["nodes"], res["links"], tree_size_min=-1)
        xyz1 = np.stack([t1["x"], t1["y"], t1["z"]], 1)[1:]
        d_one, d_one_plain = _parse(one)[1], _parse(one_plain)[1]
        assert len(d_one) == len(t1) - 1 and [r[5] for r in d_one] == _column(t1, ctx.measure_radii(xyz1)[0], d_one_plain)
    ctx.close()


# ---- voxel indices above 2^31 ----
def _two_blocks(shape):
    """balls, slabs and discs in both blocks of a stack that is background elsewhere (bigvol.radius_case), borrowed from the device; positions at
    their centres and off them, on the far faces and beyond them, and one that is not finite; absolute and relative mode -> the radii.
    A shell voxel outside the volume is not counted and one inside counts by its value, so the radii are those of radius_ref.measure
    on crops that reach rmax = 12 beyond every centre, or to the stack's face where that comes first: the far faces of the far crop are the stack's."""
    import bigvol
    case = bigvol.radius_case(shape)
    bigvol.check_placement(case["blocks"], shape, (1, 1, 1))  # (no tiles in this tool: the other placement rules)
    t, c = bigvol.open_stack(case["blocks"], shape)
    out = []
    try:
        for rel_pct in (0, 50):
            want = bigvol.radius_want(case, rel_pct)
            k, thr_used = c.measure_radii(case["xyz"], thr=case["thr"], rel_pct=rel_pct, rmax=bigvol.RAD_RMAX)
            assert k.dtype == np.int32 and np.array_equal(k, want), (rel_pct, k, want)
            assert thr_used == (0 if rel_pct else case["thr"]) and (k == -1).sum() == 1 and len(set(k.tolist())) >= 4
            out.append(k)
    finally:
        c.close()
    assert bigvol.untouched(t, case["blocks"])
    return case, out


def test_two_blocks_on_a_small_stack():
    """the placement of the case below at 96 x 64 x 41, where test_bigvol_host.py restates the whole stack"""
    import bigvol
    _two_blocks(bigvol.SMALL)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31): rad_measure gathers through voxel_index at the last plane, the shells cut at the three far faces;
    the far block is the last plane and holds the stack's last voxel, which is one of the positions"""
    import bigvol
    l, h, w = bigvol.SHAPE
    case, (k_abs, k_rel) = _two_blocks(bigvol.SHAPE)
    assert bigvol.check_placement(case["blocks"], bigvol.SHAPE, (1, 1, 1)) > 2**31
    far = np.flatnonzero(case["xyz"][:, 2] >= l - 1)
    assert len(far) >= 5 and (k_abs[far] > 0).sum() >= 2 and (case["xyz"][far] == (w - 1, h - 1, l - 1)).all(1).any()
