"""CPU (no GPU needed): the host side of the join (include/pnr_hip.h) -- the two numpy restatements of the bridges (Kruskal over the sorted
cross pairs, Boruvka's rounds) agree on forests with heavy ties; pnr_join_reroot against the restated re-rooting and ordering, its
closed forms and its argument errors; advantra_cli's usage errors around --join / --join-swc."""
import os
import subprocess
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import join_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
F = np.float32


@pytest.mark.parametrize("n,trees,extent", [(2, 2, 4), (40, 7, 6), (150, 30, 8), (300, 60, 16)])
def test_kruskal_and_boruvka_restatements_agree(n, trees, extent):
    """integer coordinates in a small box: most pair weights repeat many times, so only the (lo, hi) part of the key decides"""
    rng = np.random.default_rng(100 * n + trees)
    xyz, parent = join_ref.random_forest(rng, n, trees, extent=extent)
    for zscale, gap in ((1, 0), (1, 1.5), (2, 3), (1, 0.5)):
        k = join_ref.bridges_kruskal(xyz, parent, zscale, gap)
        b, rounds = join_ref.bridges_boruvka(xyz, parent, zscale, gap)
        assert np.array_equal(k, b), (zscale, gap)
        if gap == 0:
            assert len(k) == trees - 1 and rounds >= 1
        assert (np.diff(k["d"]) >= 0).all() and (gap == 0 or (k["d"] <= gap).all())
    ties = np.unique(join_ref.bridges_kruskal(xyz, parent)["d"], return_counts=True)[1].max()
    assert n < 100 or ties > 3, ties


def check_order(parent_out, order, comp):
    """order is a permutation, components come in their numbering, every parent before its child, children in ascending index"""
    n = len(order)
    assert np.array_equal(np.sort(order), np.arange(n))
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    kids = parent_out >= 0
    assert (pos[parent_out[kids]] < pos[kids]).all()
    assert (np.diff(comp[order]) >= 0).all() and comp[order][0] == 0
    for p in np.unique(parent_out[kids]):
        c = np.flatnonzero(parent_out == p)  # ascending index
        assert (np.diff(pos[c]) > 0).all()
        assert pos[c[0]] == pos[p] + 1  # pre-order: the first child follows its parent directly


def test_reroot_closed_forms():
    # a 5-chain 0 <- 1 <- 2 <- 3 <- 4 and a 3-chain 5 <- 6 <- 7; the bridge (6, 2) enters both in the middle: the larger tree keeps its
    # root and its parents, the smaller one is reversed on the root's side of the bridge only (5 now hangs off 6; 7 still does)
    parent = np.array([-1, 0, 1, 2, 3, -1, 5, 6], np.int32)
    po, order, comp = lib.join_reroot(parent, [(2, 6)])
    assert np.array_equal(po, [-1, 0, 1, 2, 3, 6, 2, 6])
    assert np.array_equal(order, [0, 1, 2, 3, 4, 6, 5, 7]) and np.array_equal(comp, np.zeros(8))
    # root given: everything hangs off node 7
    po, order, comp = lib.join_reroot(parent, [(2, 6)], root=7)
    assert np.array_equal(po, [1, 2, 6, 2, 3, 6, 7, -1]) and np.array_equal(order, [7, 6, 2, 1, 0, 3, 4, 5])
    # no bridge: two components, the larger first; root in the smaller one puts that first and re-roots it alone
    po, order, comp = lib.join_reroot(parent)
    assert np.array_equal(po, parent) and np.array_equal(order, np.arange(8)) and np.array_equal(comp, [0] * 5 + [1] * 3)
    po, order, comp = lib.join_reroot(parent, root=6)
    assert np.array_equal(po, [-1, 0, 1, 2, 3, 6, -1, 6]) and np.array_equal(order, [6, 5, 7, 0, 1, 2, 3, 4]) and np.array_equal(comp, [1] * 5 + [0] * 3)
    # equal sizes: the smaller root index wins, as root of a joined component and in the numbering of separate ones
    two = np.array([2, -1, -1, 1], np.int32)  # trees {1, 3} and {2, 0}
    po, order, comp = lib.join_reroot(two, [(0, 3)])
    assert np.array_equal(po, [3, -1, 0, 1]) and np.array_equal(order, [1, 3, 0, 2])
    po, order, comp = lib.join_reroot(two)
    assert np.array_equal(comp, [1, 0, 1, 0]) and np.array_equal(order, [1, 3, 2, 0])
    # a single node
    po, order, comp = lib.join_reroot([-1])
    assert po.tolist() == [-1] and order.tolist() == [0] and comp.tolist() == [0]


@pytest.mark.parametrize("n,trees", [(1, 1), (9, 9), (60, 5), (257, 31)])
def test_reroot_matches_the_restatement(n, trees):
    rng = np.random.default_rng(7 * n + trees)
    xyz, parent = join_ref.random_forest(rng, n, trees, extent=8)
    perm = rng.permutation(n)  # parents after their children, roots anywhere
    inv = np.argsort(perm)
    parent = np.where(parent[perm] >= 0, inv[parent[perm]], -1 - rng.integers(0, 3, n)).astype(np.int32)  # (any negative value = none)
    xyz = xyz[perm]
    for gap in (0, 1.5):
        bridges = join_ref.bridges_kruskal(xyz, parent, 1, gap)
        for root in (-1, n // 2, n - 1):
            got = lib.join_reroot(parent, bridges, root)
            want = join_ref.reroot(parent, bridges, root)
            for g, w in zip(got, want):
                assert g.dtype == np.int32 and np.array_equal(g, w), (gap, root)
            check_order(*got)
            if root >= 0:
                assert got[0][root] == -1 and got[1][0] == root and got[2][root] == 0
            edges = lambda p: {(min(i, int(q)), max(i, int(q))) for i, q in enumerate(p) if q >= 0}
            assert edges(got[0]) == edges(parent) | {(int(b["lo"]), int(b["hi"])) for b in bridges}  # the same edges, re-oriented
            assert (got[0] < 0).sum() == want[3] == trees - len(bridges)


def test_reroot_validation():
    """cycle, parent >= n, bad bridges, bad root, null and oversized arguments.  The third validation case of the rule, a coordinate
    that is not finite, cannot be reached here: pnr_join_reroot takes no coordinates, and pnr_join_trees / pnr_nearest_other check
    their context before anything else (as pnr_point_segment_distance does), which no machine without a GPU can create.  It is
    exercised on the GPU: test_gpu_join.py, test_contract (nan, +inf and -inf in a coordinate, and a z that overflows under zscale)."""
    L = lib.load()
    ok = np.array([-1, 0, 1, -1], np.int32)
    for bad, what in (([1, 2, 0, -1], b"cycle"), ([0, -1, -1, -1], b"cycle"), ([-1, 0, 3, 2], b"cycle"), ([-1, 4, 1, -1], b"parent[1]"), ([-1, 0, 99, -1], b"parent[2]")):
        with pytest.raises(pnr_amd.PnrError):
            lib.join_reroot(np.array(bad, np.int32))
        assert what in L.pnr_last_error(), (bad, L.pnr_last_error())
        with pytest.raises(ValueError):
            join_ref.input_trees(bad)
    for bridges in ([(0, 4)], [(-1, 3)], [(0, 2)], [(3, 3)], [(0, 3), (3, 2)]):  # outside [0, n); inside one tree; closing a cycle
        with pytest.raises(pnr_amd.PnrError):
            lib.join_reroot(ok, bridges)
    with pytest.raises(pnr_amd.PnrError):
        lib.join_reroot(ok, root=4)
    out = np.full(4, 77, np.int32)
    assert L.pnr_join_reroot(ok.ctypes.data, 0, None, 0, -1, out.ctypes.data, None, None) == -1
    assert L.pnr_join_reroot(None, 4, None, 0, -1, out.ctypes.data, None, None) == -1
    assert L.pnr_join_reroot(ok.ctypes.data, 4, None, 1, -1, out.ctypes.data, None, None) == -1
    assert L.pnr_join_reroot(ok.ctypes.data, lib.PNR_JOIN_MAX_N + 1, None, 0, -1, out.ctypes.data, None, None) == -1
    assert (out == 77).all()
    assert L.pnr_join_reroot(ok.ctypes.data, 4, None, 0, -1, None, out.ctypes.data, None) == 0 and np.array_equal(out, [0, 1, 2, 3])  # outputs are nullable


GOOD = "1 2 0 0 0 1 -1\n2 2 1 0 0 1 1\n3 2 5 0 0 1 -1\n"


def test_cli_usage_errors(tmp_path):
    good = tmp_path / "good.swc"
    good.write_text(GOOD)
    out = tmp_path / "out.swc"

    def cli(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)

    trace = ("-f", "advantra_func", "-i", str(tmp_path / "none.tif"), "-p", "2", "0", "10", "0.5", "3", "3", "10", "20", "2", "5", "5")
    for args in (("--join", "-1", *trace), ("--join", "x", *trace), ("--join", *trace[:0]), ("--join-root", "soma", *trace), ("--join-root", "3", *trace),
                 ("--join-keep-largest", *trace), ("--join", "2", "--join-root", "0", *trace), ("--join", "2", "--join-root", "tree", *trace),
                 ("--join-swc", str(good)), ("--join-swc",), ("--join-swc", str(good), str(out), "--join", "-1"),
                 ("--join-swc", str(good), str(out), "--zscale", "0"), ("--join-swc", str(good), str(out), "--join-root", "soma"),
                 ("--join-swc", str(good), str(out), "--join-root", "9"), ("--join-swc", str(tmp_path / "missing.swc"), str(out)),
                 ("--zscale", "2")):
        r = cli(*args)
        assert r.returncode != 0 and r.stdout == "" and r.stderr, args
        assert not out.exists(), args
    h = cli("--help")
    assert h.returncode == 0
    for flag in ("--join GAP", "--join-root", "--join-keep-largest", "--join-swc IN.swc OUT.swc"):
        assert flag in h.stdout, flag
