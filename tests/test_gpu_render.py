"""The render on the GPU (pnr_render_tree, pnr_tree_coverage, Context.render_tree / tree_coverage, advantra_cli --render-swc / --mask /
--coverage): closed forms, a fuzz against the rule of include/pnr_hip.h restated in numpy (render_ref.py), the same bits however the
work is cut into pieces, boxes and launches, the order rule, the coverage counts, the contract of the calls and the CLI.  Every
comparison is exact."""
import json
import os
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import distance_ref
import render_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
F = np.float32
BALLS = {0: 1, 1: 7, 2.5: 81, 4: 257}  # lattice points with dx^2 + dy^2 + dz^2 <= R^2
DISK2, BALL2 = 13, 33
KINDS = ("zero", "const", "taper", "one12")
SCALES = ((1, 0), (1.5, 0.25), (1, -1), (0, 1.5))  # (rscale, radd): as given, grown, a negative radd that clamps thin nodes to 0, radd alone


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    yield c
    c.close()


def options(c, piece=0, box=0, per_launch=0):
    c.set_option("render_piece", piece)
    c.set_option("render_box", box)
    c.set_option("render_items_per_launch", per_launch)


# ---- closed forms: do not depend on the restatement ----
def test_closed_forms(ctx):
    for R, count in BALLS.items():
        L, M = ctx.render_tree([[8, 8, 8]], [R], [-1], (17, 17, 17), mask=True)
        assert L.dtype == np.int32 and M.dtype == np.uint8 and L.shape == M.shape == (17, 17, 17)
        assert int((L == 1).sum()) == count and int((L == 0).sum()) == 17 ** 3 - count and np.array_equal(M, np.where(L > 0, 255, 0))
    L = ctx.render_tree([[3, 4, 5]], [0], [-1], (9, 9, 9))
    assert np.argwhere(L > 0).tolist() == [[5, 4, 3]]  # R = 0: the one voxel, (z, y, x)
    # a ball of radius 4 centred one voxel outside the x = 0 face: the planes dx = 1..4 of the ball
    M = ctx.render_tree([[-1, 8, 8]], [4], [-1], (17, 17, 17), labels=False, mask=True)
    per_plane = [sum(1 for dy in range(-4, 5) for dz in range(-4, 5) if dx * dx + dy * dy + dz * dz <= 16) for dx in range(1, 5)]
    assert [int((M[:, :, x] == 255).sum()) for x in range(5)] == per_plane + [0] and int((M > 0).sum()) == sum(per_plane)
    # an axis-aligned capsule of radius 2 from x = 5 to x = 15: eleven disks and two half balls; the root's ball keeps label 1
    L = ctx.render_tree([[5, 8, 8], [15, 8, 8]], [2, 2], [-1, 0], (17, 17, 21))
    assert int((L > 0).sum()) == 11 * DISK2 + (BALL2 - DISK2) and int((L == 1).sum()) == BALL2
    assert L[8, 8, 10] == 2 and L[8, 8, 3] == 1 and L[8, 8, 17] == 2 and L[8, 8, 18] == 0
    # zscale 2: a ball of radius 2 around plane 4 holds the planes 3..5 only
    L = ctx.render_tree([[8, 8, 4]], [2], [-1], (9, 17, 17), zscale=2)
    assert sorted(set(np.argwhere(L > 0)[:, 0].tolist())) == [3, 4, 5] and int((L > 0).sum()) == DISK2 + 2
    # n = 0: an all-zero label volume
    L, M = ctx.render_tree(np.zeros((0, 3), F), [], [], (3, 5, 7), mask=True)
    assert not L.any() and not M.any() and L.shape == (3, 5, 7)


# ---- fuzz against the restatement ----
def forest(rng, n, shape, zscale):
    """a forest larger than the grid on every side, so that edges cross the faces"""
    l, h, w = shape
    xyz, parent = distance_ref.random_forest(rng, n, roots=min(3, n), extent=float(max(w, h) + 8), step=2.5)
    xyz = xyz - F(4)
    xyz[:, 2] = xyz[:, 2] * F((l + 8) / (max(w, h) + 8))
    xyz[0] = (w // 2, h // 2, min(1, l - 1))  # the first root sits on a voxel: even with radius 0 no case is empty
    return xyz.astype(F), parent


@pytest.mark.parametrize("shape", [(3, 5, 7), (20, 36, 40), (1, 29, 33)])
def test_fuzz_against_restatement(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    for iz, zscale in enumerate((1, 2, 2.5, 4)):
        for jn, n in enumerate((1, 2, 63, 300)):
            xyz, parent = forest(rng, n, shape, zscale)
            if n == 2:  # (a lone edge along x, on voxels)
                xyz[1] = xyz[0] + np.array([1, 0, 0], F)
            radius = render_ref.radius_mix(rng, n, KINDS[(iz + jn) % 4])
            rscale, radd = SCALES[(iz + 2 * jn) % 4]
            want = render_ref.render(xyz, radius, parent, shape, zscale, rscale, radd)
            L, M = ctx.render_tree(xyz, radius, parent, shape, zscale=zscale, rscale=rscale, radd=radd, mask=True)
            case = (shape, zscale, n, KINDS[(iz + jn) % 4], rscale, radd)
            assert np.array_equal(L, want), (case, int((L != want).sum()))
            assert np.array_equal(M, np.where(want > 0, 255, 0).astype(np.uint8)), case
            assert int((L > 0).sum()) > 0, case


# ---- the same bits however the work is cut ----
def test_same_bits_however_cut(ctx):
    rng = np.random.default_rng(11)
    shape = (40, 40, 40)
    fx, fp = forest(rng, 300, shape, 2)
    xyz = np.concatenate([np.array([[1, 1, 0.5], [38, 38, 19]], F), fx])  # one long diagonal edge (z in planes of zscale 2), then the forest
    parent = np.concatenate([np.array([-1, 0], np.int32), np.where(fp < 0, -1, fp + 2).astype(np.int32)])
    radius = np.concatenate([np.array([2.5, 1.5], F), render_ref.radius_mix(rng, 300, "one12")])
    want = render_ref.render(xyz, radius, parent, shape, 2)
    assert int((want == 2).sum()) > 100  # the diagonal edge is there
    seen = set()
    try:
        for piece in (1, 4, 0):
            for box in (37, 0):
                for per_launch in (1, 7, 0):
                    if piece == 1 and box == 37 and per_launch == 1:
                        continue  # (tens of thousands of one-item launches: the other combinations reach every boundary)
                    options(ctx, piece, box, per_launch)
                    L = ctx.render_tree(xyz, radius, parent, shape, zscale=2)
                    assert np.array_equal(L, want), (piece, box, per_launch)
                    seen.add(ctx.get_option("render_items"))
    finally:
        options(ctx)
    assert len(seen) >= 4  # the cuts really differed


def test_smaller_index_wins(ctx):
    shape = (13, 13, 13)
    L = ctx.render_tree([[6, 6, 6], [6, 6, 6]], [3, 3], [-1, -1], shape)  # two identical segments
    assert set(np.unique(L)) == {0, 1} and int((L == 1).sum()) == 123
    thick_first = ctx.render_tree([[2, 6, 6], [10, 6, 6], [3, 6, 6], [9, 6, 6]], [3, 3, 1, 1], [-1, 0, -1, 2], shape)
    assert not (thick_first >= 3).any()  # the thin capsule lies inside the thick one, which came first
    thin_first = ctx.render_tree([[3, 6, 6], [9, 6, 6], [2, 6, 6], [10, 6, 6]], [1, 1, 3, 3], [-1, 0, -1, 2], shape)
    assert np.array_equal(thin_first > 0, thick_first > 0)
    # the thin capsule keeps its voxels: the ball of its root (7), and seven disks of radius 1 (5 each) plus the two end voxels in all
    assert int((thin_first == 1).sum()) == 7 and int(((thin_first == 1) | (thin_first == 2)).sum()) == 7 * 5 + 2 and (thin_first[6, 6, 3:10] <= 2).all()


# ---- coverage ----
def volumes():
    rng = np.random.default_rng(5)
    return {"noise": rng.integers(0, 256, (24, 40, 48), dtype=np.uint8), "synth": synth.synth(48, 40, 24, seed=3), "zero": np.zeros((24, 40, 48), np.uint8),
            "full": np.full((24, 40, 48), 255, np.uint8), "odd": rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)}


@pytest.fixture(scope="module")
def cover_case():
    rng = np.random.default_rng(6)
    shape = (24, 40, 48)
    xyz, parent = forest(rng, 63, shape, 2)
    radius = render_ref.radius_mix(rng, 63, "one12")
    return xyz, radius, parent


def check_coverage(ctx, V, xyz, radius, parent, thr, zscale=2):
    L = render_ref.render(xyz, radius, parent, V.shape, zscale)
    want, seg_vox, seg_fg, seg_sum, residual = render_ref.coverage(V, L, len(xyz), thr)
    got = ctx.tree_coverage(xyz, radius, parent, zscale=zscale, thr=thr, per_node=True, mask=True, residual=True)
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v, thr)
    assert np.array_equal(got["seg_vox"], seg_vox) and np.array_equal(got["seg_fg"], seg_fg) and np.array_equal(got["seg_sum"], seg_sum), thr
    assert got["seg_vox"].dtype == np.int64 and int(got["seg_vox"].sum()) == want["n_tree"]
    assert np.array_equal(got["mask"], np.where(L > 0, 255, 0)) and np.array_equal(got["residual"], residual)
    assert np.array_equal(np.where(got["mask"] > 0, 0, V), got["residual"])  # residual + mask are consistent
    plain = ctx.tree_coverage(xyz, radius, parent, zscale=zscale, thr=thr)
    assert plain == {k: got[k] for k in plain}
    return got


@pytest.mark.parametrize("name", ["noise", "synth", "zero", "full", "odd"])
def test_coverage_counts(ctx, cover_case, name):
    V = volumes()[name]
    xyz, radius, parent = cover_case
    if name == "odd":
        xyz = xyz * F(0.15)
    ctx.set_volume(V)
    for thr in (-1, 0, 1, 37, 255):
        got = check_coverage(ctx, V, xyz, radius, parent, thr)
        assert got["n_tree"] > 0 and got["n_vox"] == V.size
        if name == "zero" and thr != 0:
            assert got["covered"] == got["on_signal"] == got["covered_intensity"] == 0.0 and got["n_fg"] == 0
        if name == "full":
            assert got["n_fg"] == V.size and got["on_signal"] == 1.0 and got["covered"] == got["n_tree"] / V.size
    assert ctx.tree_coverage(xyz, radius, parent, zscale=2, thr=-1)["thr_used"] == max(1, int(V.astype(np.int64).sum()) // V.size)
    empty = ctx.tree_coverage(np.zeros((0, 3), F), [], [], thr=37, per_node=True, mask=True, residual=True)  # n = 0
    assert empty["n_tree"] == 0 and empty["covered"] == 0.0 and empty["on_signal"] == 0.0 and empty["n_fg"] == int((V >= 37).sum())
    assert len(empty["seg_vox"]) == 0 and not empty["mask"].any() and np.array_equal(empty["residual"], V)
    assert np.array_equal(ctx.get_volume(), V)  # V is never written


def test_coverage_on_a_borrowed_unaligned_volume(ctx, cover_case):
    import torch
    V = volumes()["noise"]
    xyz, radius, parent = cover_case
    for shift in (0, 1, 6):  # a borrowed volume off a 4- and 16-byte boundary: the byte path of the finish pass and of the sum
        flat = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), V.ravel()])).cuda()
        torch.cuda.synchronize()
        ctx.set_volume_device(flat.data_ptr() + shift, V.shape, keepalive=flat)
        check_coverage(ctx, V, xyz, radius, parent, -1)
        check_coverage(ctx, V, xyz, radius, parent, 37)
        torch.cuda.synchronize()
        assert np.array_equal(flat.cpu().numpy()[shift:], V.ravel())  # the borrowed volume is unchanged
    ctx.set_volume(V)


# ---- errors and resources ----
def test_argument_errors(ctx):
    ok = dict(xyz=[[2, 2, 2], [4, 4, 4]], radius=[1, 1], parent=[-1, 0], shape=(6, 6, 6))
    bad = [dict(shape=(0, 6, 6)), dict(shape=(6, 0, 6)), dict(shape=(6, 6, 0)), dict(xyz=[[2, np.nan, 2], [4, 4, 4]]), dict(xyz=[[2, 2, np.inf], [4, 4, 4]]),
           dict(radius=[1, -0.5]), dict(radius=[np.inf, 1]), dict(radius=[np.nan, 1]), dict(rscale=-1), dict(radd=np.inf), dict(radd=np.nan),
           dict(radius=[1, 1025]), dict(radius=[1, 600], rscale=2), dict(radius=[1, 1], radd=1024), dict(parent=[-1, 2]), dict(zscale=0), dict(zscale=-1),
           dict(xyz=[[2, 2, 3e38], [4, 4, 4]], zscale=4)]
    for b in bad:
        kw = {**ok, **b}
        with pytest.raises(pnr_amd.PnrError, match="error -1"):
            ctx.render_tree(**kw)
    big = lib.PNR_RENDER_MAX_N + 1
    with pytest.raises(pnr_amd.PnrError, match="error -1"):
        ctx.render_tree(np.zeros((big, 3), F), np.zeros(big, F), np.full(big, -1, np.int32), (2, 2, 2))
    ctx.set_volume(np.zeros((6, 6, 6), np.uint8))
    for thr in (-2, 256):
        with pytest.raises(pnr_amd.PnrError, match="error -1"):
            ctx.tree_coverage(ok["xyz"], ok["radius"], ok["parent"], thr=thr)
    with pytest.raises(pnr_amd.PnrError, match="error -1"):
        ctx.tree_coverage(ok["xyz"], [1, -1], ok["parent"])
    with pytest.raises(pnr_amd.PnrError, match="error -1"):
        ctx.set_option("render_piece", -1)
    L = ctx.render_tree(ok["xyz"], [1024, 1024], ok["parent"], ok["shape"])  # the largest radius is legal
    assert (L > 0).all()


def test_coverage_needs_a_volume():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    with pytest.raises(pnr_amd.PnrError, match="error -4"):
        c.tree_coverage([[1, 1, 1]], [1], [-1])
    assert int((c.render_tree([[1, 1, 1]], [1], [-1], (3, 3, 3)) > 0).sum()) == 7  # the render itself needs none
    c.close()


def test_buffers_are_freed_and_the_timer_counts(ctx, cover_case):
    xyz, radius, parent = cover_case
    V = volumes()["synth"]
    ctx.set_volume(V)
    ctx.tree_coverage(xyz, radius, parent, zscale=2)
    before = lib.live_bytes()
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    ctx.tree_coverage(xyz, radius, parent, zscale=2, per_node=True, mask=True, residual=True)
    ctx.render_tree(xyz, radius, parent, V.shape, zscale=2, mask=True)
    with pytest.raises(pnr_amd.PnrError):
        ctx.render_tree(xyz, -radius - 1, parent, V.shape)
    ms, launches = ctx.kernel_ms("render")
    (ms_s, n_s), (ms_f, n_f) = ctx.kernel_ms("render_scatter"), ctx.kernel_ms("render_finish")
    ctx.set_profiling(False)
    assert lib.live_bytes() == before
    assert launches == n_s + n_f and n_s == 2 and n_f == 3 and ms > 0 and ms == ms_s + ms_f  # the sum and the finish of the coverage, the finish of the render
    assert ctx.get_option("render_items") > 0 and ctx.get_option("render_pairs") >= ctx.get_option("render_items")


# ---- CLI ----
SWC = """# a hand-written tree: a trunk along x with a tapering branch, an isolated thick node, a thin tail that leaves the stack
1 2 6 20 12 2.5 -1
2 2 20.5 20 12 2 1
3 2 34 21.25 12.5 1.5 2
4 3 20 30 14 1 2
5 3 21 38.5 16 0.25 4
7 1 40 8 6 4 -1
9 6 52 8 6 0 7
"""
ZS = 2


def read_tiff(path):
    from PIL import Image
    with Image.open(path) as im:
        pages = []
        for z in range(im.n_frames):
            im.seek(z)
            pages.append(np.array(im))
    return np.stack(pages)


def test_cli_render_swc(tmp_path):
    V = synth.synth(48, 40, 24, seed=3)
    swc, tif = tmp_path / "t.swc", tmp_path / "stack.tif"
    swc.write_text(SWC)
    lib.write_tiff(tif, V)
    xyz, radius, typ, parent, ids = pnr_amd.read_swc_nodes(swc)
    for thr, rscale, radd in ((37, 1, 0), (-1, 1.5, 0.5)):
        L = render_ref.render(xyz, radius, parent, V.shape, ZS, rscale, radd)
        want, seg_vox, seg_fg, seg_sum, residual = render_ref.coverage(V, L, len(xyz), thr)
        flags = ["--coverage-threshold", str(thr)] if thr >= 0 else []
        r = subprocess.run([CLI, "--render-swc", str(swc), "-i", str(tif), "--mask", str(tmp_path / "m.tif"), "--residual", str(tmp_path / "r.raw"), "--per-node",
                            str(tmp_path / "n.csv"), "--zscale", str(ZS), "--radius-scale", str(rscale), "--radius-add", str(radd), *flags],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1500:]
        got = json.loads(r.stdout)
        assert list(got)[-2:] == ["nodes", "items"] and got["nodes"] == len(xyz) and got["items"] > 0
        assert {k: got[k] for k in want} == want and want["n_tree"] > 0
        assert np.array_equal(read_tiff(tmp_path / "m.tif"), np.where(L > 0, 255, 0))
        assert open(tmp_path / "r.raw", "rb").read() == residual.tobytes()
        rows = open(tmp_path / "n.csv").read().split("\n")
        assert rows[0] == "id,vox,fg,sum" and rows[-1] == ""
        assert [[int(v) for v in ln.split(",")] for ln in rows[1:-1]] == [[int(ids[i]), int(seg_vox[i]), int(seg_fg[i]), int(seg_sum[i])] for i in range(len(ids))]
    # the pre-filters apply as in tracing: the tree is measured on what would be traced
    r = subprocess.run([CLI, "--render-swc", str(swc), "-i", str(tif), "--median", "3d", "--zscale", str(ZS), "--residual", str(tmp_path / "rf.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)
    c.set_volume(V)
    c.filter_volume(median=3)
    Vf = c.get_volume()
    c.close()
    L = render_ref.render(xyz, radius, parent, V.shape, ZS)
    want = render_ref.coverage(Vf, L, len(xyz), -1)
    got = json.loads(r.stdout)
    assert {k: got[k] for k in want[0]} == want[0] and open(tmp_path / "rf.raw", "rb").read() == want[4].tobytes()


def test_cli_render_swc_mask_only(tmp_path):
    swc = tmp_path / "t.swc"
    swc.write_text(SWC)
    xyz, radius, typ, parent, ids = pnr_amd.read_swc_nodes(swc)
    L = render_ref.render(xyz, radius, parent, (24, 40, 48), ZS)
    r = subprocess.run([CLI, "--render-swc", str(swc), "-d", "48,40,24", "--zscale", str(ZS), "--mask", str(tmp_path / "m.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    got = json.loads(r.stdout)
    assert got["n_vox"] == L.size and got["n_tree"] == int((L > 0).sum()) > 0 and got["nodes"] == len(xyz) and got["items"] > 0
    assert open(tmp_path / "m.raw", "rb").read() == np.where(L > 0, 255, 0).astype(np.uint8).tobytes()
    for extra in (["--residual", str(tmp_path / "r.raw")], ["--per-node", str(tmp_path / "n.csv")], ["--coverage-threshold", "5"]):  # need a stack
        r = subprocess.run([CLI, "--render-swc", str(swc), "-d", "48,40,24", "--mask", str(tmp_path / "m2.raw"), *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "only --mask" in r.stderr and not os.path.exists(tmp_path / "m2.raw")
    r = subprocess.run([CLI, "--radius-scale", "2", "-f", "advantra_func", "-i", "x.tif", "-p", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "need --render-swc" in r.stderr


PARAS = "2,3 0 5 0.3 3 2 40 50 2 4 5".split()


def test_cli_mask_and_coverage_while_tracing(tmp_path):
    img = synth.synth(48, 40, 24, seed=1)
    out = {}
    for name, flags in (("plain", []), ("render", ["--mask", str(tmp_path / "mask.tif"), "--coverage"])):
        d = tmp_path / name
        d.mkdir()
        lib.write_tiff(d / "stack.tif", img)
        r = subprocess.run([CLI, *flags, "-f", "advantra_func", "-i", str(d / "stack.tif"), "-p", *PARAS], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        out[name] = open(str(d / "stack.tif") + "_Advantra.swc").read().split("\n")
    cov = [ln for ln in out["render"] if ln.startswith("#coverage=")]
    assert len(cov) == 1 and not [ln for ln in out["plain"] if "coverage" in ln]
    fields = dict(kv.split(":") for kv in cov[0][len("#coverage="):].split(","))
    assert list(fields) == ["thr", "covered", "on_signal", "intensity", "tree_voxels"]
    mask = read_tiff(tmp_path / "mask.tif")
    assert mask.shape == img.shape and set(np.unique(mask)) <= {0, 255}
    assert int((mask == 255).sum()) == int(fields["tree_voxels"]) > 0
    assert [ln for ln in out["render"] if ln is not cov[0]] == out["plain"]  # the one comment line apart, the same file
    # the mask is the render of the file's own tree: the radius column as written (three decimals) may differ from the f32 rendered, so
    # the check is on the nodes: every node inside the stack lies under the mask
    xyz, radius, typ, parent, ids = pnr_amd.read_swc_nodes(str(tmp_path / "render" / "stack.tif") + "_Advantra.swc")
    vox = np.round(xyz).astype(int)
    inside = ((vox >= 0) & (vox < np.array(img.shape[::-1]))).all(1) & (np.abs(xyz - vox).max(1) < 0.25) & (radius >= 1)
    assert inside.sum() > 0 and (mask[vox[inside, 2], vox[inside, 1], vox[inside, 0]] == 255).all()
    assert float(fields["thr"]) == max(1, int(img.astype(np.int64).sum()) // img.size)


# ---- voxel indices above 2^31 ----
def _two_blocks(shape):
    """a six-node tree with mixed radii (one of 12) in each block of a stack that is background elsewhere (bigvol.render_case), borrowed from the
    device -> the coverage.  A voxel's label depends on its absolute coordinates and the segments alone (render_ref takes the crop's
    origin), so the per-node triples and the counts are the sums over two crops that hold every voxel a segment can reach and every
    foreground voxel: the box of a tree's nodes widened by the largest radius + 2 and the tree's block, cut where the stack cuts them."""
    import bigvol
    case = bigvol.render_case(shape)
    bigvol.check_placement(case["blocks"], shape, (1, 1, 1))  # (no tiles in this tool: the other placement rules)
    wcov, wvox, wfg, wsum = bigvol.render_want(case)
    t, c = bigvol.open_stack(case["blocks"], shape)
    try:
        cov = c.tree_coverage(case["xyz"], case["radius"], case["parent"], zscale=bigvol.REN_ZS, thr=case["thr"], per_node=True)
    finally:
        c.close()
    assert {k: cov[k] for k in wcov} == wcov, (cov, wcov)
    for k, v in (("seg_vox", wvox), ("seg_fg", wfg), ("seg_sum", wsum)):
        assert cov[k].dtype == np.int64 and np.array_equal(cov[k], v), (k, cov[k], v)
    assert (wvox > 0).sum() >= 8 and wcov["n_both"] > 100 and wcov["n_vox"] == int(np.prod(shape, dtype=np.int64))
    assert bigvol.untouched(t, case["blocks"])
    return case, cov


def test_two_blocks_on_a_small_stack():
    """the placement of the case below at 96 x 64 x 41, where test_bigvol_host.py restates the whole stack"""
    import bigvol
    _two_blocks(bigvol.SMALL)


def test_indices_beyond_2_to_31():
    """2048 x 2048 x 513 voxels (N > 2^31): rn_scatter's atomics at lab + ((z h + y) w + x), rn_finish over (N + 3) >> 2 groups; the far tree ends
    beside the stack's last voxel with a radius of 12: its capsule is cut by z = l - 1, y = h - 1 and x = w - 1"""
    import bigvol
    l, h, w = bigvol.SHAPE
    case, cov = _two_blocks(bigvol.SHAPE)
    assert bigvol.check_placement(case["blocks"], bigvol.SHAPE, (1, 1, 1)) > 2**31 and cov["n_vox"] == l * h * w
    thick = len(case["xyz"]) - 2
    (x, y, z), r = case["xyz"][thick], case["radius"][thick]
    assert x + r > w - 1 and y + r > h - 1 and z * bigvol.REN_ZS + r > (l - 1) * bigvol.REN_ZS and cov["seg_vox"][thick] > 100
