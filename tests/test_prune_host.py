"""CPU (no GPU needed): the pruning rule of include/pnr_hip.h -- pnr_prune_tree_host (prune_rule.cpp, one sequential pass) against its
numpy restatement (prune_ref.py) on generated forests, the closed forms that need no restatement, the rule's consequences, the range
and argument errors with their texts, pnr_prune_apply, and the stand-alone sanitizer run of the rule (make prune_check).  Every
comparison is exact."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import prune_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORESTS = ((1, 1, 0), (2, 1, 0), (65, 3, .7), (1000, 4, .9), (4099, 7, .95))
OPTIONS = ((5, 0, 0), (10, 2, 0), (40, 0, 30))
ARRAYS = ("keep", "height", "path", "order", "seg")
_cache = {}


def generated(n, trees, chain):
    if (n, trees, chain) not in _cache:
        _cache[n, trees, chain] = ref.forest(n, trees, chain, seed=n)
    return _cache[n, trees, chain]


def reference(case, zscale, opts):
    """the restatement's answer, computed once per case and shared (test_gpu_prune.py reads it too)"""
    key = ("ref", case, zscale, opts)
    if key not in _cache:
        _cache[key] = ref.prune(*generated(*case), zscale, *opts)
    return _cache[key]


def same(got, want, what):
    assert {k: got[0][k] for k in ref.INFO_KEYS} == want[0], what
    for name, g, w in zip(ARRAYS, got[1:6], want[1:6]):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("case", FORESTS)
@pytest.mark.parametrize("zscale", (1, 2))
def test_host_equals_the_restatement(case, zscale):
    xyz, radius, parent = generated(*case)
    for opts in OPTIONS + ((0, 0, 0),):
        got = pnr_amd.prune_tree_host(xyz, radius, parent, zscale, *opts)
        same(got, reference(case, zscale, opts), (case, zscale, opts))
        assert got[0]["rounds_up"] == 0 and got[0]["rounds_down"] == 0
    same(pnr_amd.prune_tree_host(xyz, None, parent, zscale, 10, 2, 0), ref.prune(xyz, None, parent, zscale, 10, 2, 0), (case, "no radius"))


@pytest.mark.parametrize("case", FORESTS[3:])
def test_the_fuzz_removes_some_and_not_all(case):
    info = reference(case, 1, (40, 0, 30))[0]
    assert 0.10 * info["n"] <= info["n_removed"] <= 0.70 * info["n"], info


def test_y_with_a_tie():
    xyz, radius, parent = ref.y_tie()
    info, keep, height, path, order, seg = pnr_amd.prune_tree_host(xyz, radius, parent, min_length=4.5)
    assert list(keep) == [1] * 8 + [0] * 4 and list(seg) == [0] * 8 + [8] * 4 and list(order) == [0] * 8 + [1] * 4
    assert list(height[:4]) == [7 * 256, 6 * 256, 5 * 256, 4 * 256] and info["n_removed_segments"] == 1 and info["n_segments"] == 2
    assert list(path[8:]) == [4 * 256, 5 * 256, 6 * 256, 7 * 256]
    info, keep, *_ = pnr_amd.prune_tree_host(xyz, radius, parent, min_length=4)  # S = 4 * 256 < 4 * 256 is false
    assert keep.all() and info["n_removed"] == 0
    # the other numbering: the arm whose first node has the smaller index continues
    swap = np.array([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7])
    xyz2, parent2 = xyz[swap], np.array([-1, 0, 1, 2, 3, 4, 5, 6, 3, 8, 9, 10], np.int32)
    _, keep2, *_ = pnr_amd.prune_tree_host(xyz2, radius, parent2, min_length=4.5)
    assert list(keep2) == [1] * 8 + [0] * 4


def test_star():
    xyz, radius, parent = ref.star(3000, 2.0)
    info, keep, height, path, order, seg = pnr_amd.prune_tree_host(xyz, radius, parent, min_length=2)
    assert keep.all() and info["n_segments"] == 3000 and info["n_leaves"] == 3000 and info["n_branch"] == 1 and info["order_max"] == 1
    assert seg[1] == 0 and np.array_equal(seg[2:], np.arange(2, 3001)) and order[1] == 0 and (order[2:] == 1).all()
    info, keep, *_ = pnr_amd.prune_tree_host(xyz, radius, parent, min_length=2.01)
    assert list(keep[:2]) == [1, 1] and not keep[2:].any() and info["n_removed"] == 2999 == info["n_removed_segments"]
    assert info["length_in"] == 3000 * 512 and info["length_out"] == 512


def test_single_chain():
    xyz, radius, parent = ref.chain(5000)
    for L in (0, 1, 100, 4998.5, 1e5):
        info, keep, height, path, order, seg = pnr_amd.prune_tree_host(xyz, radius, parent, min_length=L, radius_factor=50)
        assert keep.all() and info["n_segments"] == 1 and not order.any() and not seg.any()
        assert np.array_equal(path, 256 * np.arange(5000)) and np.array_equal(height, path[::-1])


def test_radius_rule():
    for r, stays in ((1, 1), (2, 0)):  # a side branch of 3 voxels: 3 >= 2 * 1 stays, 3 < 2 * 2 goes
        xyz, radius, parent = ref.radius_case(r)
        _, keep, *_ = pnr_amd.prune_tree_host(xyz, radius, parent, radius_factor=2)
        assert list(keep) == [1] * 8 + [stays]


def test_min_tree_drops_whole_trees_and_nothing_else():
    xyz, radius, parent = generated(1000, 4, .9)
    extra = np.array([[90, 90, 90], [91, 90, 90], [92, 90, 90], [92, 91, 90]], np.float32)  # a tree of height 2: two leaves, one a side branch of 1
    xyz = np.concatenate([xyz, extra])
    radius = np.concatenate([radius, np.ones(4, np.float32)])
    parent = np.concatenate([parent, np.array([-1, 1000, 1001, 1001], np.int32)])
    info0, _, height, _, _, _ = pnr_amd.prune_tree_host(xyz, radius, parent)
    info, keep, *_ = pnr_amd.prune_tree_host(xyz, radius, parent, min_tree=2.5)
    roots = np.flatnonzero(parent < 0)
    low = {int(r) for r in roots if height[r] < 640}
    assert 1000 in low and info["n_removed_trees"] == len(low) < len(roots)
    root_of = np.arange(len(parent))
    for _ in range(len(parent)):
        up = np.where(parent[root_of] >= 0, parent[root_of], root_of)
        if np.array_equal(up, root_of):
            break
        root_of = up
    assert np.array_equal(keep == 0, np.isin(root_of, list(low)))
    assert info0["n_removed"] == 0


def test_all_options_zero_keep_everything():
    for case in FORESTS:
        info, keep, *_ = pnr_amd.prune_tree_host(*generated(*case))
        assert keep.all() and info["n_removed"] == 0 and info["length_in"] == info["length_out"]


@pytest.mark.parametrize("case", FORESTS[2:])
def test_pruning_the_pruned_tree_removes_nothing(case):
    xyz, radius, parent = generated(*case)
    for opts in OPTIONS:
        info, keep, height, *_ = pnr_amd.prune_tree_host(xyz, radius, parent, 1, *opts)
        idx, parent2 = pnr_amd.prune_apply(parent, keep)
        want_idx, want_parent = ref.apply(parent, keep)
        assert np.array_equal(idx, want_idx) and np.array_equal(parent2, want_parent)
        if not len(parent2):
            continue
        k = keep != 0
        info2, keep2, height2, *_ = pnr_amd.prune_tree_host(xyz[k], radius[k], parent2, 1, *opts)
        assert keep2.all() and info2["n_removed"] == 0 and np.array_equal(height2, height[k])
        assert info2["length_in"] == info["length_out"]


def test_keep_is_monotone_in_min_length():
    xyz, radius, parent = generated(4099, 7, .95)
    last = np.ones(len(parent), np.uint8)
    for L in (0, 1, 2, 3.5, 5, 10, 20, 40, 80, 1000):
        _, keep, *_ = pnr_amd.prune_tree_host(xyz, radius, parent, min_length=L)
        assert not (keep & ~last & 1).any(), L
        last = keep
    assert not last[parent >= 0].all()


def test_renumbering_that_keeps_the_order_of_siblings():
    """a breadth-first renumbering visits the children of a node in ascending old index, so every tie falls the same way"""
    xyz, radius, parent = generated(1000, 4, .9)
    n = len(parent)
    children = [[] for _ in range(n)]
    for i, p in enumerate(parent):
        if p >= 0:
            children[p].append(i)
    bfs = [int(i) for i in np.flatnonzero(parent < 0)][::-1]  # (roots in any order: they are no siblings)
    for v in bfs:
        bfs.extend(children[v])
    bfs = np.array(bfs)
    new = np.empty(n, np.int64)
    new[bfs] = np.arange(n)
    parent2 = np.where(parent[bfs] >= 0, new[np.maximum(parent[bfs], 0)], -1).astype(np.int32)
    for opts in OPTIONS:
        a = pnr_amd.prune_tree_host(xyz, radius, parent, 1, *opts)
        b = pnr_amd.prune_tree_host(xyz[bfs], radius[bfs], parent2, 1, *opts)
        assert {k: a[0][k] for k in ref.INFO_KEYS} == {k: b[0][k] for k in ref.INFO_KEYS}
        for x, y in zip(a[1:5], b[1:5]):
            assert np.array_equal(x[bfs], y)
        assert np.array_equal(new[a[5][bfs]], b[5])


RANGE_TEXT = "a path reaches 2^32 units of 1/256 voxel: the limit is 2^24 xy voxels of path"


def range_case():
    return np.array([[0, 0, 0], [1e7, 0, 0], [2e7, 0, 0]], np.float32), None, np.array([-1, 0, 1], np.int32)


def _fails(text, fn, *args, **kw):
    with pytest.raises(pnr_amd.PnrError) as e:
        fn(*args, **kw)
    assert text in str(e.value) and "error -1" in str(e.value), str(e.value)


def test_range():
    _fails("pnr_prune_tree_host: " + RANGE_TEXT, pnr_amd.prune_tree_host, *range_case())
    with pytest.raises(ref.RangeError):
        ref.prune(*range_case())
    xyz, _, parent = range_case()
    info, *_ = pnr_amd.prune_tree_host(xyz[:2], None, parent[:2])  # one edge of 1e7 voxels stays below the limit
    assert info["h_max"] == 2560000000
    _fails(RANGE_TEXT, pnr_amd.prune_tree_host, np.array([[0, 0, 0], [1.7e7, 0, 0]], np.float32), None, parent[:2])  # a single edge beyond it


def test_argument_errors_and_their_texts():
    who = "pnr_prune_tree_host: "
    xyz, radius, parent = ref.y_tie()
    cyc = parent.copy()
    cyc[4] = 7
    _fails(who + "the parent chain of node 7 does not end (a cycle)", pnr_amd.prune_tree_host, xyz, radius, cyc)
    big = parent.copy()
    big[5] = 12
    _fails(who + "parent[5] = 12 outside [-1, 12)", pnr_amd.prune_tree_host, xyz, radius, big)
    _fails(who + "min_length = -1 must not be negative", pnr_amd.prune_tree_host, xyz, radius, parent, min_length=-1)
    _fails(who + "radius_factor = -0.5 must not be negative", pnr_amd.prune_tree_host, xyz, radius, parent, radius_factor=-.5)
    _fails(who + "min_tree = -2 must not be negative", pnr_amd.prune_tree_host, xyz, radius, parent, min_tree=-2)
    _fails(who + "min_length = nan must not be negative", pnr_amd.prune_tree_host, xyz, radius, parent, min_length=float("nan"))
    _fails(who + "zscale = 0 must be positive", pnr_amd.prune_tree_host, xyz, radius, parent, zscale=0)
    _fails(who + "n = 0 nodes (1 to 2^31 - 1) need xyz and parent", pnr_amd.prune_tree_host, np.zeros((0, 3), np.float32), None, np.zeros(0, np.int32))
    bad = xyz.copy()
    bad[3, 1] = np.inf
    _fails(who + "a coordinate is not finite", pnr_amd.prune_tree_host, bad, radius, parent)
    _fails(who + "a radius is not finite", pnr_amd.prune_tree_host, xyz, radius * np.float32("nan"), parent)
    L = lib.load()
    for a in ((None, None, parent.ctypes.data, 12), (xyz.ctypes.data, None, None, 12)):
        assert L.pnr_prune_tree_host(*a, None, None, None, None, None, None, None) == -1
        assert L.pnr_last_error() == b"pnr_prune_tree_host: n = 12 nodes (1 to 2^31 - 1) need xyz and parent"
    info = lib.PruneInfo()  # every per-node output may be NULL
    assert L.pnr_prune_tree_host(xyz.ctypes.data, None, parent.ctypes.data, 12, None, C.byref(info), None, None, None, None, None) == 0 and info.n_segments == 2
    with pytest.raises(pnr_amd.PnrError, match="one radius and one parent per node"):
        pnr_amd.prune_tree_host(xyz, radius[:5], parent)


def test_prune_apply():
    parent = np.array([-1, 0, 1, 1, -1, 4], np.int32)
    idx, par = pnr_amd.prune_apply(parent, [1, 1, 0, 1, 0, 0])
    assert list(idx) == [0, 1, -1, 2, -1, -1] and list(par) == [-1, 0, 1]
    idx, par = pnr_amd.prune_apply(parent, [0] * 6)
    assert list(idx) == [-1] * 6 and len(par) == 0
    _fails("pnr_prune_apply: node 3 is kept, its parent 1 is removed", pnr_amd.prune_apply, parent, [1, 0, 0, 1, 1, 1])
    _fails("pnr_prune_apply: parent[2] = 6 outside [-1, 6)", pnr_amd.prune_apply, np.array([-1, 0, 6, 1, -1, 4], np.int32), [1] * 6)
    _fails("pnr_prune_apply: n = 0 nodes (1 to 2^31 - 1) need parent, keep and m", pnr_amd.prune_apply, np.zeros(0, np.int32), [])
    # a file in tree order stays in tree order
    xyz, radius, parent = ref.forest(500, 3, .8, seed=3, permute=False)
    _, keep, *_ = pnr_amd.prune_tree_host(xyz, radius, parent, min_length=6)
    _, par = pnr_amd.prune_apply(parent, keep)
    assert 0 < len(par) < 500 and (par < np.arange(len(par))).all()


def test_exports():
    hdr = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    for name in ("pnr_prune_tree", "pnr_prune_tree_host", "pnr_prune_apply"):
        assert name in lib.PRODUCT_EXPORTS and ("int %s(" % name) in hdr and hasattr(lib.load(), name)


def test_make_prune_check():
    """the host rule under -fsanitize=address,undefined as a stand-alone program: builds, runs, exits 0"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pnr_amd", "csrc"), "prune_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "prune rule check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
