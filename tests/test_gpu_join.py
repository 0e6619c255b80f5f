"""The join on the GPU (pnr_nearest_other, pnr_join_trees, Context.join_trees, advantra_cli --join / --join-swc): closed forms, the tie
rule, a fuzz of the search and of the whole join against the rule of include/pnr_hip.h restated in numpy (join_ref.py) with automatic
and with forced slices and launches, the contract of the call, the pipeline and the CLI.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest
import synth
import pnr_amd
from pnr_amd import lib
import join_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
F = np.float32
SIZES = [(1, 1), (2, 2), (65, 3), (1000, 40), (4099, 300)]


@pytest.fixture(scope="module")
def ctx():
    c = pnr_amd.Context(pnr_amd.make_params(sigmas=(2,)), 0)  # no volume: the join needs none
    yield c
    c.close()


def forced(c, on):
    c.set_option("join_split", 64 if on else 0)
    c.set_option("join_pairs_per_launch", 100000 if on else 0)


def triples(bridges):
    return [(int(b["lo"]), int(b["hi"]), float(b["d"])) for b in bridges]


# ---- closed forms: do not depend on the restatement ----
def test_closed_forms(ctx):
    chain = np.array([-1, 0, 1, 2, 3], np.int32)
    xyz = np.zeros((10, 3), F)
    xyz[:5, 0], xyz[5:, 0] = np.arange(5), 7 + np.arange(5)  # two 5-node chains, 3 apart along x
    parent = np.concatenate([chain, np.where(chain < 0, -1, chain + 5)]).astype(np.int32)
    for gap in (3, 0):
        po, order, comp, br, cnt = ctx.join_trees(xyz, parent, gap=gap, counts=True)
        assert triples(br) == [(4, 5, 3.0)] and cnt == {"trees_in": 2, "trees_out": 1, "rounds": 1}
        assert np.array_equal(po, [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8]) and np.array_equal(order, np.arange(10)) and not comp.any()
        assert po.dtype == order.dtype == comp.dtype == np.int32 and br.dtype == lib.BRIDGE
    po, order, comp, br, cnt = ctx.join_trees(xyz, parent, gap=2.5, counts=True)
    assert len(br) == 0 and cnt["trees_out"] == 2 and np.array_equal(po, parent) and np.array_equal(comp, [0] * 5 + [1] * 5)
    # zscale: node 0 alone; the tree {1, 2} has node 2 two planes above node 0 and node 1 three voxels beside it
    xyz = np.array([[0, 0, 0], [3, 0, 0], [0, 0, 2]], F)
    assert triples(ctx.join_trees(xyz, [-1, -1, 1])[3]) == [(0, 2, 2.0)]
    po, order, _, br = ctx.join_trees(xyz, [-1, -1, 1], zscale=2)
    assert triples(br) == [(0, 1, 3.0)] and np.array_equal(po, [1, -1, 1]) and np.array_equal(order, [1, 0, 2])  # (the larger tree keeps its root)
    # three collinear fragments at x = 0, 5, 2: two bridges in ascending key order
    xyz = np.array([[0, 1, 1], [5, 1, 1], [2, 1, 1]], F)
    po, order, comp, br = ctx.join_trees(xyz, [-1, -1, -1])
    assert triples(br) == [(0, 2, 2.0), (1, 2, 3.0)] and np.array_equal(po, [-1, 2, 0]) and np.array_equal(order, [0, 2, 1])
    assert triples(ctx.join_trees(xyz, [-1, -1, -1], gap=2)[3]) == [(0, 2, 2.0)]
    # one tree alone, and a single node: no bridge, identity
    po, order, comp, br, cnt = ctx.join_trees(np.arange(15, dtype=F).reshape(5, 3), chain, counts=True)
    assert len(br) == 0 and np.array_equal(po, chain) and np.array_equal(order, np.arange(5)) and cnt == {"trees_in": 1, "trees_out": 1, "rounds": 0}
    po, order, comp, br = ctx.join_trees([[1, 2, 3]], [-1])
    assert len(br) == 0 and po.tolist() == [-1] and order.tolist() == [0] and comp.tolist() == [0]
    d, j = ctx.nearest_other([[0, 0, 0], [3, 4, 0], [0, 0, 1]], [0, 1, 0])
    assert d.dtype == F and j.dtype == np.int32 and np.array_equal(d, [5, 5, np.sqrt(F(26))]) and np.array_equal(j, [1, 0, 1])


def test_tie_rule(ctx):
    """four fragments on the corners of a square of side 4, 75 coincident nodes each (node i belongs to fragment i % 4): every pair
    across a side has d2 = 16, so only (lo, hi) decides -- the bridges are (0, 1), (0, 3), (1, 2); the equal targets of a point sit in
    all five slices when join_split = 64 is forced"""
    n = 300
    corner = np.array([[0, 0, 7], [4, 0, 7], [4, 4, 7], [0, 4, 7]], F)
    xyz = corner[np.arange(n) % 4]
    parent = np.arange(n, dtype=np.int32) - 4
    parent[:4] = -1
    out = []
    for on in (False, True):
        forced(ctx, on)
        d, j = ctx.nearest_other(xyz, np.arange(n) % 4)
        assert (d == 4).all() and np.array_equal(j, np.where(np.arange(n) % 2 == 0, 1, 0))  # the smallest index on the two adjacent corners
        out.append(ctx.join_trees(xyz, parent, counts=True))
        assert triples(out[-1][3]) == [(0, 1, 4.0), (0, 3, 4.0), (1, 2, 4.0)], (on, out[-1][3])
    forced(ctx, False)
    for a, b in zip(*out):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    po = out[0][0]
    assert po[0] == -1 and po[1] == 0 and po[3] == 0 and po[2] == 1 and np.array_equal(po[4:], parent[4:])


# ---- fuzz of the search against the restatement ----
def labelled_points(n, labels, integer):
    rng = np.random.default_rng(1000 * n + labels + (1 if integer else 0))
    xyz = (np.floor(rng.random((n, 3)) * 16) if integer else rng.random((n, 3)) * 64).astype(F)
    label = rng.integers(0, labels, n).astype(np.int32)
    if n >= labels:
        label[rng.permutation(n)[:labels]] = np.arange(labels)  # every label occurs
    label[6::7] = -1 - rng.integers(0, 5, len(label[6::7]))  # every seventh point takes no part
    if n > 2:
        label[n // 2] = labels  # a label that holds a single point
    return xyz, label


SEARCH_REF = {}


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("n,labels", SIZES)
def test_fuzz_nearest_other(ctx, n, labels, integer):
    xyz, label = labelled_points(n, labels, integer)
    if (n, integer) not in SEARCH_REF:
        SEARCH_REF[(n, integer)] = join_ref.nearest_other(xyz, label)
    want_d, want_j = SEARCH_REF[(n, integer)]
    forced(ctx, False)
    d0, j0 = ctx.nearest_other(xyz, label)
    forced(ctx, True)
    d1, j1 = ctx.nearest_other(xyz, label)
    forced(ctx, False)
    print(f"n={n} labels={labels} integer={integer}: d mismatches auto {int((d0 != want_d).sum())} forced {int((d1 != want_d).sum())}, j mismatches auto "
          f"{int((j0 != want_j).sum())} forced {int((j1 != want_j).sum())}, zeros {int((want_d == 0).sum())}, without a partner {int((want_j < 0).sum())}")
    assert np.array_equal(d0, d1) and np.array_equal(j0, j1)
    assert np.array_equal(d0, want_d), np.flatnonzero(d0 != want_d)[:5]
    assert np.array_equal(j0, want_j), np.flatnonzero(j0 != want_j)[:5]
    assert (want_j[label < 0] == -1).all() and np.isinf(want_d[label < 0]).all() and (n < 7 or (label < 0).any())
    assert not np.isin(want_j[want_j >= 0], np.flatnonzero(label < 0)).any()


# ---- fuzz of the whole join ----
EXTENT = {1: 8, 2: 8, 65: 12, 1000: 40, 4099: 64}  # sparse enough that the three gaps give three different forests


def forest_case(n, trees):
    """integer coordinates: massive ties, coincident nodes of different trees (d2 = 0) included"""
    return join_ref.random_forest(np.random.default_rng(77 * n + trees), n, trees, extent=EXTENT[n])


JOIN_REF = {}


def join_want(n, trees, gap, root):
    key = (n, trees, gap)
    xyz, parent = forest_case(n, trees)
    if key not in JOIN_REF:
        JOIN_REF[key] = join_ref.bridges_kruskal(xyz, parent, 1, gap)
    return join_ref.join(xyz, parent, 1, gap, root, bridges=JOIN_REF[key])


@pytest.mark.parametrize("gap", [0, 1.5, 4])
@pytest.mark.parametrize("n,trees", SIZES)
def test_fuzz_join_trees(ctx, n, trees, gap):
    xyz, parent = forest_case(n, trees)
    for root in (-1, (2 * n) // 3):
        want = join_want(n, trees, gap, root)
        forced(ctx, root >= 0 and n <= 1000)  # (forced launches of 100 000 pairs: kept to the small cases)
        got = ctx.join_trees(xyz, parent, gap=gap, root=root, counts=True)
        forced(ctx, False)
        print(f"n={n} trees={trees} gap={gap} root={root}: {len(got[3])} bridges (want {len(want[3])}), {got[4]}")
        assert np.array_equal(got[3], want[3]), (root, got[3][:5], want[3][:5])
        for k, name in enumerate(("parent", "order", "comp")):
            assert np.array_equal(got[k], want[k]), (root, name, np.flatnonzero(got[k] != want[k])[:5])
        assert {k: got[4][k] for k in ("trees_in", "trees_out")} == want[4] and want[4]["trees_in"] == trees
        if gap == 0:
            assert want[4]["trees_out"] == 1 and len(got[3]) == trees - 1
        if (n, trees, gap) == (4099, 300, 0):  # the multi-round path cannot go untested
            assert got[4]["rounds"] >= 3 and ctx.get_option("join_rounds") == got[4]["rounds"], got[4]


# ---- the contract of the call ----
def test_contract(ctx):
    L = lib.load()
    xyz, parent = forest_case(65, 3)
    xyz = np.ascontiguousarray(xyz)
    want = join_want(65, 3, 0, -1)
    nb, t0, t1 = C.c_int64(), C.c_int64(), C.c_int64()

    def call(x=xyz, par=parent, n=65, opts=(1, 0, -1), br=None, cap=0, nbp=nb):
        o = lib.JoinOpts(*opts) if opts is not None else None
        ptr = lambda v: v.ctypes.data if v is not None else None
        return L.pnr_join_trees(ctx.h, ptr(x), ptr(par), n, C.byref(o) if o is not None else None, None, None, None, ptr(br), cap, C.byref(nbp) if nbp is not None else None,
                                C.byref(t0), C.byref(t1))

    live = lib.live_bytes()
    # a capacity that is too small: the count and the first `cap` bridges; then call again
    assert call(opts=None) == 0 and nb.value == 2 and (t0.value, t1.value) == (3, 1)  # NULL options = {1, 0, -1}; every output is nullable
    br = np.zeros(3, lib.BRIDGE)
    br["lo"] = 77
    assert call(br=br, cap=1) == 0 and nb.value == 2 and br[0] == want[3][0] and (br["lo"][1:] == 77).all()
    assert call(br=br, cap=2) == 0 and np.array_equal(br[:2], want[3]) and br["lo"][2] == 77
    for opts in ((0, 0, -1), (-1, 0, -1), (np.nan, 0, -1), (1, -0.5, -1), (1, np.nan, -1), (1, np.inf, -1), (1, 0, 65)):
        assert call(opts=opts) == -1, opts
    assert call(n=0) == -1 and call(n=-1) == -1 and call(n=lib.PNR_JOIN_MAX_N + 1) == -1 and call(x=None) == -1 and call(par=None) == -1 and call(nbp=None) == -1
    assert call(cap=2) == -1 and call(cap=-1, br=br) == -1
    assert L.pnr_join_trees(None, xyz.ctypes.data, parent.ctypes.data, 65, None, None, None, None, None, 0, C.byref(nb), None, None) == -1
    for v in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[9, 1] = v
        assert call(x=bad) == -1 and b"node 9" in L.pnr_last_error()
    big = xyz.copy()
    big[3, 2] = 3e38
    assert call(x=big, opts=(2, 0, -1)) == -1  # z * zscale is not finite
    cyc = parent.copy()
    cyc[0], cyc[np.flatnonzero(parent == 0)[0]] = np.flatnonzero(parent == 0)[0], 0
    assert call(par=cyc) == -1 and b"cycle" in L.pnr_last_error()
    high = parent.copy()
    high[7] = 65
    assert call(par=high) == -1 and b"parent[7]" in L.pnr_last_error()
    # pnr_nearest_other
    lab = np.arange(65, dtype=np.int32) % 3
    d, j = np.full(65, 77, F), np.full(65, 77, np.int32)
    near = lambda x=xyz, la=lab, n=65, dd=d, jj=j: L.pnr_nearest_other(ctx.h, *(v.ctypes.data if v is not None else None for v in (x, la)), n, *(v.ctypes.data if v is not None else None for v in (dd, jj)))
    assert near(n=0) == -1 and near(n=lib.PNR_JOIN_MAX_N + 1) == -1 and near(x=None) == -1 and near(la=None) == -1 and near(dd=None) == -1 and near(jj=None) == -1
    assert near(x=bad) == -1 and (d == 77).all() and (j == 77).all()
    with pytest.raises(pnr_amd.PnrError):
        ctx.join_trees(xyz, parent, gap=-1)
    assert lib.live_bytes() == live  # every device buffer of a call is freed before it returns, failed calls included
    # the timer group "join": (0, 0) before a call; prep + one launch + finish per pass
    ctx.set_profiling(True)
    ctx.reset_kernel_ms()
    assert ctx.kernel_ms("join") == (0.0, 0)
    ctx.nearest_other(xyz, lab)
    ms, launches = ctx.kernel_ms("join")
    assert ms > 0 and launches == 3, (ms, launches)
    rounds = ctx.join_trees(xyz, parent, counts=True)[4]["rounds"]
    assert rounds >= 1 and ctx.kernel_ms("join")[1] == 3 + 3 * rounds and ctx.kernel_ms("join")[0] > ms
    ctx.set_profiling(False)
    # a foreign stream gives the same result
    import torch
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    got = ctx.join_trees(xyz, parent)
    ctx.set_stream(None)
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:4]))
    assert lib.live_bytes() == live


# ---- the pipeline and the CLI ----
# two 48 x 40 x 24 synth stacks (seeds 1 and 2) side by side with 12 dark columns between them: the CPU oracle's pipeline traces this
# to 526 tree nodes in two trees with the parameters below
def two_fragment_stack():
    return np.concatenate([synth.synth(48, 40, 24, seed=1), np.zeros((24, 40, 12), np.uint8), synth.synth(48, 40, 24, seed=2)], axis=2)


PARAS = "2,3 0 5 0.3 3 2 40 50 2 4 5".split()
# the comment block advantra_cli writes for PARAS on an 8-bit stack with no other flag (the first line gets the `#comment ` prefix)
PLAIN_COMMENT = ("email: miro@braincadet.com\n#params:\n#channel=1\n#neuritesigmas=2,3\n#somaradius=0\n#tolerance=5\n#znccth=0.3\n#kappa=3\n#step=2\n#ni=40\n#np=50\n"
                 "#zdist=2\n#nodepervol=4\n#vol=5\n#------------------------\n#Kc=20\n#neff_ratio=0.8\n#frangi_alfa=0.5\n#frangi_beta=0.5\n#frangi_C=500\n"
                 "#MAX_TRACE_COUNT=5000\n#EPSILON2=0.0001\n#REFINE_ITER=4\n#SIG2RADIUS=1.5\n#TRACE_RSMPL=1\n#GROUP_RADIUS=2\n#ENFORCE_SINGLE_TREE=0\n"
                 "#TREE_SIZE_MIN=10\n#TAIL_SIZE_MIN=2")


def read_lines(path):
    """-> (comment lines, rows [id, type, x, y, z, r, parent] as text)"""
    lines = open(path).read().splitlines()
    return [ln for ln in lines if ln.startswith("#")], [ln.split() for ln in lines if ln and not ln.startswith("#")]


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    """the stack traced by the CLI without and with --join 0 -> (plain file, joined file, stdout of the joined run)"""
    from PIL import Image
    d = tmp_path_factory.mktemp("join_cli")
    img = two_fragment_stack()
    out = []
    for name, flags in (("plain", ()), ("joined", ("--join", "0"))):
        tif = str(d / f"{name}.tif")
        pages = [Image.fromarray(z) for z in img]
        pages[0].save(tif, save_all=True, append_images=pages[1:], compression=None)
        r = subprocess.run([CLI, *flags, "-f", "advantra_func", "-i", tif, "-p", *PARAS], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        out.append(tif + "_Advantra.swc")
    return out[0], out[1], r.stdout, img


def test_cli_join_while_tracing(ctx, traced):
    plain, joined, stdout, img = traced
    c0, rows0 = read_lines(plain)
    c1, rows1 = read_lines(joined)
    xyz, parent, ids = lib.read_swc(plain)
    trees_in = int((parent < 0).sum())
    print(f"{len(rows0)} nodes in {trees_in} trees; {[ln for ln in c1 if ln.startswith('#join')]}")
    assert trees_in > 1 and np.array_equal(ids, np.arange(len(ids)) + 1)  # the case is a forest
    # without the flag nothing of the join shows; with it the comment block gains one line, after the parameters
    assert not [ln for ln in c0 if "join" in ln]
    extra = [ln for ln in c1 if ln not in c0]
    assert extra == [f"#join=gap:0,bridges:{trees_in - 1},trees:{trees_in}->1"] and [ln for ln in c1 if ln in c0] == c0
    # one component, ids 1..n, every parent id below its child's id; the same nodes up to order
    pid = np.array([int(r[6]) for r in rows1])
    nid = np.array([int(r[0]) for r in rows1])
    assert np.array_equal(nid, np.arange(len(rows1)) + 1) and (pid == -1).sum() == 1 and pid[0] == -1 and (pid[1:] < nid[1:]).all() and (pid[1:] >= 1).all()
    assert sorted(tuple(r[1:6]) for r in rows0) == sorted(tuple(r[1:6]) for r in rows1)
    # the joined file is the plain file's tree under Context.join_trees with zscale = zdist
    po, order, comp, br = ctx.join_trees(xyz, parent, zscale=2)
    assert [tuple(r[1:6]) for r in rows1] == [tuple(rows0[v][1:6]) for v in order]
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order)) + 1
    assert np.array_equal(pid, np.where(po[order] < 0, -1, pos[po[order]]))
    assert "join... gap 0" in stdout
    # the Python pipeline's tree is the plain file's; a context with Frangi state joins and goes on
    p = pnr_amd.make_params(sigmas=[2, 3], tolerance=5, znccth=0.3, kappa=3, step=2, ni=40, np_=50, zdist=2, nodepervol=4, vol=5)
    c = pnr_amd.Context(p, 0)
    res = pnr_amd.advantra.run_pipeline(c, img)
    tx = np.stack([res["tree"]["x"], res["tree"]["y"], res["tree"]["z"]], 1)[1:]
    tp = np.where(res["parent"][1:] > 0, res["parent"][1:] - 1, -1).astype(np.int32)
    assert len(tx) == len(xyz) and np.array_equal(tp, parent)
    # without the flag the file is today's, byte for byte: the name line, the comment block of the C++ host as it was before the join
    # (written out here), the header, and every row as write_swc_tree puts the Python pipeline's tree, which knows nothing of the join
    ref = plain + ".ref"
    pnr_amd.write_swc_tree(ref, res["tree"], res["parent"], comment=PLAIN_COMMENT)
    got_b, want_b = open(plain, "rb").read(), open(ref, "rb").read()
    diff = [(a, b) for a, b in zip(got_b.splitlines(), want_b.splitlines()) if a != b][:3]
    print(f"plain file {len(got_b)} bytes, reference {len(want_b)} bytes, first differing lines {diff}")
    assert got_b == want_b
    seeds = c.extract_seeds()
    got = c.join_trees(tx, tp, zscale=2)
    want = join_ref.join(tx, tp, 2, 0)
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:4])) and len(got[3]) == trees_in - 1
    assert np.array_equal(c.extract_seeds(), seeds) and len(c.score_filter_sort(seeds)) > 0
    c.close()


def test_cli_join_swc(ctx, traced, tmp_path):
    plain = traced[0]
    xyz, parent, ids = lib.read_swc(plain)
    _, rows0 = read_lines(plain)
    root = len(ids) // 2
    for flags, kw in ((("--join", "0"), {}), (("--join", "40", "--zscale", "2", "--join-root", str(ids[root])), dict(gap=40, zscale=2, root=root)),
                      (("--join", "3", "--join-keep-largest"), dict(gap=3))):
        out = str(tmp_path / f"out{len(flags)}.swc")
        r = subprocess.run([CLI, "--join-swc", plain, out, *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and len(r.stdout.splitlines()) == 1, r.stderr[-1500:]
        info = json.loads(r.stdout)
        po, order, comp, br, cnt = ctx.join_trees(xyz, parent, counts=True, **kw)
        print(r.stdout.strip())
        if "--join-keep-largest" in flags:
            order = order[comp[order] == 0]
        assert F(info.pop("longest_bridge")) == (br["d"].max() if len(br) else 0)  # (nine digits: the f32 exactly)
        assert info == {"nodes": len(order), "trees_in": cnt["trees_in"], "trees_out": cnt["trees_out"], "bridges": len(br), "rounds": cnt["rounds"]}
        comments, rows = read_lines(out)
        assert comments[0] == f"#join=gap:{kw.get('gap', 0)},bridges:{len(br)},trees:{cnt['trees_in']}->{cnt['trees_out']}"
        x2, p2, i2 = lib.read_swc(out)
        pos = np.full(len(xyz), -1, np.int64)
        pos[order] = np.arange(len(order))
        assert np.array_equal(i2, np.arange(len(order)) + 1) and np.array_equal(x2, xyz[order]) and np.array_equal(p2, np.where(po[order] < 0, -1, pos[po[order]]))
        assert [(r[1], float(r[5])) for r in rows] == [(rows0[v][1], float(rows0[v][5])) for v in order]  # type and radius carried over
