"""Pruning on the GPU (pnr_prune_tree, Context.prune_tree, advantra_cli --prune-swc / --prune): the pointer jumping of prune.hip against
the sequential host pass (pnr_prune_tree_host, which test_prune_host.py holds against the numpy restatement prune_ref.py) at the
smallest sizes at which the kernels can go wrong, the bound on the launches, the contract of the call, and the CLI.  Every comparison
is exact."""
import ctypes as C
import json
import math
import os
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import prune_ref as ref
from test_prune_host import FORESTS, OPTIONS, ARRAYS, RANGE_TEXT, generated, reference, range_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
CLOSED = {"y_tie": (ref.y_tie, ((4.5, 0, 0), (4, 0, 0))), "star": (ref.star, ((2, 0, 0), (2.01, 0, 0))), "chain": (ref.chain, ((100, 50, 0), (0, 0, 5000))),
          "radius_1": (lambda: ref.radius_case(1), ((0, 2, 0),)), "radius_2": (lambda: ref.radius_case(2), ((0, 2, 0),))}


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)  # no volume: the pruning needs none
    yield c
    c.close()


def depth_of(parent):
    d, up = 0, np.asarray(parent).copy()
    while (up >= 0).any():
        up = np.where(up >= 0, parent[np.maximum(up, 0)], -1)
        d += 1
    return d


def same(got, want, what, depth=None):
    assert {k: got[0][k] for k in ref.INFO_KEYS} == {k: want[0][k] for k in ref.INFO_KEYS}, what
    for name, g, w in zip(ARRAYS, got[1:6], want[1:6]):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)
    if depth is not None:  # nothing climbs node by node
        bound = math.ceil(math.log2(depth + 1)) + 2
        assert 1 <= got[0]["rounds_up"] <= bound and 1 <= got[0]["rounds_down"] <= bound, (what, depth, got[0])


@pytest.mark.parametrize("case", FORESTS)
def test_gpu_equals_the_host_pass(ctx, case):
    xyz, radius, parent = generated(*case)  # (permuted indices: a parent is processed after its child as often as before)
    depth = reference(case, 1, OPTIONS[0])[6]
    for zscale in (1, 2):
        for opts in OPTIONS + ((0, 0, 0),):
            same(ctx.prune_tree(xyz, radius, parent, zscale, *opts), pnr_amd.prune_tree_host(xyz, radius, parent, zscale, *opts), (case, zscale, opts), depth)
    same(ctx.prune_tree(xyz, None, parent, 1, 10, 2, 0), pnr_amd.prune_tree_host(xyz, None, parent, 1, 10, 2, 0), (case, "no radius"), depth)


@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_forms(ctx, name):
    make, options = CLOSED[name]
    xyz, radius, parent = make()
    depth = depth_of(parent)
    for opts in options:
        got = ctx.prune_tree(xyz, radius, parent, 1, *opts)
        same(got, pnr_amd.prune_tree_host(xyz, radius, parent, 1, *opts), (name, opts), depth)
    if name == "chain":  # depth 4999: 14 rounds, not 4999
        assert depth == 4999 and got[0]["rounds_up"] == 14 and got[0]["rounds_down"] == 14, got[0]
    if name == "star":   # every atomic of a round on one address, and the tie rule under contention: leaf 1 continues
        assert got[5][1] == 0 and got[0]["n_removed"] == 2999 and got[0]["rounds_up"] == 1


def test_chain_written_leaf_first(ctx):
    xyz, radius, parent = ref.chain(5000)
    xyz, parent = xyz[::-1].copy(), np.where(parent[::-1] >= 0, 4999 - parent[::-1], -1).astype(np.int32)
    same(ctx.prune_tree(xyz, radius, parent, 1, 0, 0, 5000), pnr_amd.prune_tree_host(xyz, radius, parent, 1, 0, 0, 5000), "leaf first", 4999)


def test_two_calls_give_identical_bytes_and_null_outputs_the_same_info(ctx):
    xyz, radius, parent = generated(4099, 7, .95)
    before = lib.live_bytes()[0]  # (what the context holds between calls)
    a, b = ctx.prune_tree(xyz, radius, parent, 1, 40, 0, 30), ctx.prune_tree(xyz, radius, parent, 1, 40, 0, 30)
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    o, info = lib.PruneOpts(1, 40, 0, 30), lib.PruneInfo()
    lib.check(ctx.L.pnr_prune_tree(ctx.h, xyz.ctypes.data, radius.ctypes.data, parent.ctypes.data, len(parent), C.byref(o), C.byref(info), None, None, None, None, None))
    assert info.as_dict() == a[0]
    lib.check(ctx.L.pnr_prune_tree(ctx.h, xyz.ctypes.data, radius.ctypes.data, parent.ctypes.data, len(parent), C.byref(o), None, None, None, None, None, None))
    assert lib.live_bytes()[0] == before  # nothing stays allocated after the call


def test_range_error_and_the_context_afterwards(ctx):
    with pytest.raises(pnr_amd.PnrError) as e:
        ctx.prune_tree(*range_case())
    assert "pnr_prune_tree: " + RANGE_TEXT in str(e.value) and "error -1" in str(e.value)
    xyz = np.array([[0, 0, 0], [1.7e7, 0, 0]], np.float32)  # a single edge beyond the limit: the edge kernel's own flag
    with pytest.raises(pnr_amd.PnrError, match="2\\^24 xy voxels"):
        ctx.prune_tree(xyz, None, [-1, 0])
    xyz = np.zeros((40, 3), np.float32)  # the limit is reached by a path only: 40 edges of 2^19 voxels, each sum below it for 5 rounds
    xyz[:, 0] = np.arange(40) * 2.0 ** 19
    with pytest.raises(pnr_amd.PnrError, match="2\\^24 xy voxels"):
        ctx.prune_tree(xyz, None, np.arange(-1, 39))
    with pytest.raises(pnr_amd.PnrError, match="2\\^24 xy voxels"):
        pnr_amd.prune_tree_host(xyz, None, np.arange(-1, 39))
    got = ctx.prune_tree(xyz[:32], None, np.arange(-1, 31))  # 31 edges: 2^32 - 2^27 units
    assert got[0]["h_max"] == 31 * 2 ** 27 and got[3][31] == 31 * 2 ** 27
    xyz, radius, parent = ref.y_tie()
    same(ctx.prune_tree(xyz, radius, parent, 1, 4.5), pnr_amd.prune_tree_host(xyz, radius, parent, 1, 4.5), "after the error")
    for bad, text in (((xyz, radius, np.array([-1, 0, 1, 2, 7, 4, 5, 6, 3, 8, 9, 10])), "pnr_prune_tree: the parent chain of node 7 does not end (a cycle)"),
                      ((xyz, radius, parent, 1, -1), "pnr_prune_tree: min_length = -1 must not be negative")):
        with pytest.raises(pnr_amd.PnrError) as e:
            ctx.prune_tree(*bad)
        assert text in str(e.value)


def test_kernel_time_group(ctx):
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    info = ctx.prune_tree(*generated(1000, 4, .9))[0]
    ms, launches = ctx.kernel_ms("prune")
    ctx.set_profiling(False)
    assert ms > 0 and launches == 4 + info["rounds_up"] + info["rounds_down"]


# ---- the CLI ----
def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)


def write_swc(path, xyz, radius, parent, types):
    with open(path, "w") as f:
        f.write("# a generated forest\n")
        for i in range(len(parent)):
            f.write("%d %d %s %s %s %s %d\n" % (i + 1, types[i], *(repr(float(v)) for v in xyz[i]), repr(float(radius[i])), parent[i] + 1 if parent[i] >= 0 else -1))


def rows_of(path):
    lines = open(path).read().splitlines()
    return [ln for ln in lines if ln.startswith("#") and not ln.startswith("##")], [ln.split() for ln in lines if ln and not ln.startswith("#")]  # (## heads the columns)


def pruned_by_the_tool(swc, out, length, factor, tree, zscale):
    r = run("--prune-swc", swc, out, "--prune-length", str(length), "--prune-radius", str(factor), "--prune-min-tree", str(tree), "--zscale", str(zscale))
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return rows_of(out)


def test_cli_prune_swc(tmp_path):
    xyz, radius, parent = generated(1000, 4, .9)
    types = 2 + np.arange(len(parent)) % 3
    swc, out, csv = (str(tmp_path / n) for n in ("in.swc", "out.swc", "nodes.csv"))
    write_swc(swc, xyz, radius, parent, types)
    want = reference((1000, 4, .9), 2, (10, 2, 0))
    info, keep, height, path, order, seg = want[:6]
    r = run("--prune-swc", swc, out, "--prune-length", "10", "--prune-radius", "2", "--zscale", "2", "--per-node", csv)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    line = json.loads(r.stdout)
    idx, par = ref.apply(parent, keep)
    assert line.pop("rounds_up") >= 1 and line.pop("rounds_down") >= 1
    assert line == {"nodes": 1000, "nodes_out": len(par), "zscale": 2, "min_length": 10, "radius_factor": 2, "min_tree": 0, **{k: info[k] for k in ref.INFO_KEYS if k[0] == "n" and k != "n"},
                    "length_in": info["length_in"] / 256, "length_out": info["length_out"] / 256, "h_max": info["h_max"] / 256, "order_max": info["order_max"]}
    comments, rows = rows_of(out)
    assert comments[-1] == f"#prune=length:10,radius:2,min_tree:0,removed:{info['n_removed']},segments:{info['n_removed_segments']}" and 0 < info["n_removed"] < 1000
    k = np.flatnonzero(keep)
    assert [int(f[0]) for f in rows] == list(range(1, len(k) + 1)) and [int(f[6]) for f in rows] == [p + 1 if p >= 0 else -1 for p in par]
    assert [int(f[1]) for f in rows] == list(types[k])  # types and radii are carried over, the nodes keep their order
    assert np.array_equal(np.array([f[2:6] for f in rows], np.float32), np.column_stack([xyz[k], radius[k]]))
    table = [ln.split(",") for ln in open(csv).read().splitlines()]
    assert table[0] == ["id", "keep", "height", "path", "order", "seg_id"] and len(table) == 1001
    got = np.array(table[1:], np.float64)
    assert np.array_equal(got, np.column_stack([np.arange(1, 1001), keep, height / 256, path / 256, order, seg + 1]))
    # no threshold and no OUT: the morphometry of the file
    r = run("--prune-swc", swc)
    assert r.returncode == 0 and json.loads(r.stdout)["n_removed"] == 0 and json.loads(r.stdout)["n_segments"] == info["n_segments"]


def test_cli_skeleton_prune(tmp_path):
    """--skeleton --swc --prune L,K writes what --prune-swc makes of the unpruned file with the same numbers"""
    import thin_ref
    shape = (24, 48, 64)
    V = thin_ref.volume(shape, "tubes")
    V[8:15, 18:25, 6:58] = 255  # a bar 7 x 7 across ...
    for x in range(10, 56, 6):  # ... with bumps on two of its faces: the thinning leaves a spur for each
        V[15:18, 20:23, x:x + 2] = 255
        V[10:13, 25:28, x + 3:x + 5] = 255
    raw, plain, pruned, again = (str(tmp_path / n) for n in ("t.raw", "plain.swc", "pruned.swc", "again.swc"))
    V.tofile(raw)
    args = ("--skeleton", "-i", raw, "-d", "64,48,24", "--threshold", str(thin_ref.THR), "--zscale", "2")
    for swc, flags in ((plain, ()), (pruned, ("--prune", "3,1.5"))):
        r = run(*args, "--swc", swc, *flags)
        assert r.returncode == 0 and r.stderr == "", r.stderr
    c0, rows0 = rows_of(plain)
    c1, rows1 = rows_of(pruned)
    c2, rows2 = pruned_by_the_tool(plain, again, 3, 1.5, 0, 2)
    assert rows1 == rows2 and 20 < len(rows1) < len(rows0)  # some spurs went
    assert c1[:-1] == c0 and c0[-1].startswith("#skeleton=") and c1[-1] == c2[-1] and c1[-1].startswith("#prune=length:3,radius:1.5,min_tree:0,removed:")
    print(len(rows0), "->", len(rows1), c1[-1])


def test_cli_prune_while_tracing(tmp_path):
    """--join 0 --prune 5 writes the nodes --prune-swc makes of the --join 0 file; without --prune that file is what it always was"""
    from PIL import Image
    from test_gpu_join import PARAS, PLAIN_COMMENT, two_fragment_stack
    img = two_fragment_stack()
    files = {}
    for name, flags in (("joined", ("--join", "0")), ("pruned", ("--join", "0", "--prune", "5"))):
        tif = str(tmp_path / f"{name}.tif")
        pages = [Image.fromarray(z) for z in img]
        pages[0].save(tif, save_all=True, append_images=pages[1:], compression=None)
        r = run(*flags, "-f", "advantra_func", "-i", tif, "-p", *PARAS)
        assert r.returncode == 0, r.stderr[-1500:]
        files[name] = tif + "_Advantra.swc"
    c0, rows0 = rows_of(files["joined"])
    c1, rows1 = rows_of(files["pruned"])
    join_line = [ln for ln in c0 if ln.startswith("#join=")]
    assert "\n".join(c0[:-1]).endswith(PLAIN_COMMENT) and c0[-1:] == join_line and not [ln for ln in c0 if "prune" in ln]  # nothing of the pruning shows
    c2, rows2 = pruned_by_the_tool(files["joined"], str(tmp_path / "again.swc"), 5, 0, 0, 2)
    # (the tracer writes three decimals, the tool the shortest text of the same f32: the rows are compared as numbers)
    assert np.array_equal(np.array(rows1, np.float32), np.array(rows2, np.float32)) and 0 < len(rows1) < len(rows0)
    assert c1[:-1] == c0 and c1[-1] == c2[-1] and c1[-1].startswith("#prune=length:5,radius:0,min_tree:0,removed:%d," % (len(rows0) - len(rows1)))
