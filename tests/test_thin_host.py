"""CPU: the thinning rule's numpy restatement (thin_ref.py) is held to the topology it must keep, against scipy.ndimage.label; the pure
host pnr_skeleton_forest equals its restatement; the C ABI has pnr_skeletonize; and advantra_cli --skeleton lists its flags and fails in
the order of the other tool modes on a machine without a GPU."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import synth
import thin_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
SHAPES = ((3, 7, 9), (12, 24, 40))  # (l, h, w); the second has tile corners, edges and faces of thin.h's 32 x 8 x 8 inside


@functools.lru_cache(maxsize=None)
def thinned(shape, kind):
    obj = ref.objects(shape, kind)
    skel, rounds = ref.thin(obj)
    obj.setflags(write=False), skel.setflags(write=False)
    return obj, skel, rounds


def test_simple_point_test_against_labels():
    """conditions (a) and (b) on random, sparse and dense neighbourhood words: the flood over adjacency masks equals scipy's labels"""
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1 << 27, 1500, dtype=np.uint32) & np.uint32(ref.N26)
    w = np.concatenate([w, w[:500] & np.roll(w, 1)[:500], w[:500] | np.roll(w, 1)[:500], np.array([0, 1, 1 << 26, ref.N6, ref.N18, ref.N26, ref.N26 & ~ref.N6], np.uint32)])
    assert np.array_equal(ref.is_simple(w), np.array([ref.simple_by_labels(int(v)) for v in w]))
    assert ref.is_end(np.array([0, 1, 3, 1 << 26], np.uint32)).tolist() == [False, True, False, True]


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_keeps_the_topology(shape, kind):
    obj, skel, rounds = thinned(shape, kind)
    assert not (skel & ~obj).any()
    want = ref.topology(obj)  # 26-components, 6-components of the padded background, Euler number
    assert ref.topology(skel) == want
    first, r1 = ref.thin(obj, max_rounds=1)
    assert r1 == 1 and ref.topology(first) == want and not (first & ~obj).any() and not (skel & ~first).any()
    again, r2 = ref.thin(skel)
    assert r2 == 1 and np.array_equal(again, skel)
    assert rounds >= 1 and (rounds > 1) == bool((obj & ~skel).any())


@pytest.mark.parametrize("shape, left, rounds", [((2, 2, 2), 2, 2), ((3, 3, 3), 3, 2), ((33, 65, 129), 473, 25)])
def test_calibration_counts_of_a_full_block(shape, left, rounds):
    skel, r = ref.thin(np.ones(shape, bool))
    assert (int(skel.sum()), r) == (left, rounds)


def components(skel):
    from scipy import ndimage
    return ndimage.label(skel, np.ones((3, 3, 3), int))[1]


def check_forest(vox, shape, n_comp):
    want = ref.forest(vox, shape)
    got = pnr_amd.skeleton_forest(vox, shape)
    assert got.dtype == lib.BRIDGE
    assert [(int(e["lo"]), int(e["hi"])) for e in got] == [(lo, hi) for lo, hi, _ in want]
    assert np.array_equal(got["d"], np.sqrt(np.array([len2 for _, _, len2 in want], np.float32)))
    assert len(got) == len(vox) - n_comp
    if len(vox):
        parent, order, comp = pnr_amd.join_reroot(np.full(len(vox), -1, np.int32), got)
        assert int((parent < 0).sum()) == n_comp == len(set(comp.tolist()))
        place = np.empty(len(vox), np.int64)
        place[order] = np.arange(len(vox))
        assert all(p < 0 or place[p] < place[i] for i, p in enumerate(parent.tolist()))  # every parent before its children


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forest_equals_the_restatement(shape, kind):
    _, skel, _ = thinned(shape, kind)
    check_forest(np.flatnonzero(skel).astype(np.int64), shape, components(skel))


def test_forest_edge_cases():
    check_forest(np.zeros(0, np.int64), (2, 3, 4), 0)
    check_forest(np.array([7], np.int64), (2, 3, 4), 1)
    # a junction triangle opens at its diagonal; any order of the voxels is taken as given
    tri = np.array([1 + 4 * 1, 0, 1], np.int64)  # (1, 1, 0), (0, 0, 0), (1, 0, 0) of a 4 x 3 x 2 grid
    got = pnr_amd.skeleton_forest(tri, (2, 3, 4))
    assert [(int(e["lo"]), int(e["hi"]), float(e["d"])) for e in got] == [(0, 2, 1.0), (1, 2, 1.0)]
    full = np.arange(24, dtype=np.int64)
    check_forest(full, (2, 3, 4), 1)
    assert set(pnr_amd.skeleton_forest(full, (2, 3, 4))["d"].tolist()) == {1.0}
    L = lib.load()
    n = C.c_int64()
    two = np.array([3, 3], np.int64)
    assert L.pnr_skeleton_forest(two.ctypes.data, 2, 4, 3, 2, None, 0, C.byref(n)) == -1  # listed twice
    out = np.array([24], np.int64)
    assert L.pnr_skeleton_forest(out.ctypes.data, 1, 4, 3, 2, None, 0, C.byref(n)) == -1  # outside the grid
    assert L.pnr_skeleton_forest(full.ctypes.data, 24, 4, 3, 0, None, 0, C.byref(n)) == -1
    assert L.pnr_skeleton_forest(full.ctypes.data, 24, 4, 3, 2, None, -1, C.byref(n)) == -1
    part = np.zeros(5, lib.BRIDGE)
    assert L.pnr_skeleton_forest(full.ctypes.data, 24, 4, 3, 2, part.ctypes.data, 5, C.byref(n)) == 0 and n.value == 23  # the full count
    assert np.array_equal(part, pnr_amd.skeleton_forest(full, (2, 3, 4))[:5])


def test_c_abi_has_the_entry_points():
    L = lib.load()
    assert L.pnr_skeletonize and L.pnr_skeleton_forest
    assert "pnr_skeletonize" in lib.PRODUCT_EXPORTS and "pnr_skeleton_forest" in lib.PRODUCT_EXPORTS
    assert L.pnr_skeletonize(None, None, None, None, None, None, 0) == -1  # a null context is an argument error, GPU or not
    assert C.sizeof(lib.ThinInfo) == 72 and C.sizeof(lib.ThinOpts) == 8
    txt = open(os.path.join(ROOT, "include", "pnr_hip.h")).read()
    for word in ("Malandain-Bertrand", "int pnr_skeletonize(", "int pnr_skeleton_forest(", "never 26-adjacent", "Device memory of a call"):
        assert word in txt, word


# ---- advantra_cli --skeleton ----
def run(*args):
    if not os.path.exists(CLI):
        subprocess.run(["make", "-s", "-C", os.path.dirname(CLI)], check=True)
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_the_flags():
    r = run("--help")
    assert r.returncode == 0
    for flag in ("--skeleton -i stack", "--skeleton-rounds R", "--skeleton-out OUT", "--swc OUT.swc", "#skeleton=thr:T,rounds:R,voxels:K,trees:C"):
        assert flag in r.stdout, flag


def test_usage_errors_come_before_any_file_is_read(tmp_path):
    missing = str(tmp_path / "none.raw")
    for bad in ("300", "-2", "x", ""):
        r = run("--skeleton", "-i", missing, "--threshold", bad)
        assert (r.returncode, r.stderr) == (1, "--threshold T: an integer from 0 to 255, or -1 for the stack's mean\n")
    r = run("--skeleton", "-i", missing, "--skeleton-rounds", "-1")
    assert r.returncode == 1 and r.stderr.startswith("--skeleton-rounds R:") and r.stderr.count("\n") == 1
    for args, line in ((("--skeleton-rounds", "3", "-i", missing), "--skeleton-rounds / --skeleton-out / --swc need --skeleton -i stack"),
                       (("--swc", "o.swc", "-i", missing), "--skeleton-rounds / --skeleton-out / --swc need --skeleton -i stack"),
                       (("--skeleton",), "--skeleton needs -i <stack>"),
                       (("--skeleton", "-i", missing, "--zscale", "0.5"), "--skeleton: --zscale Z: a number, 1 or more"),
                       (("--skeleton", "-i", missing, "--swc"), "--swc OUT.swc"),
                       (("--skeleton", "-i", missing, "--skeleton-out"), "--skeleton-out OUT: a .tif or .raw file name")):
        r = run(*args)
        assert (r.returncode, r.stderr) == (1, line + "\n"), (args, r.stderr)
    for other in (("--components",), ("--edt",), ("--min-size", "3"), ("--distance", "a.swc", "b.swc"), ("--info",), ("--despeckle", "3"), ("--per-node", "x.csv")):
        r = run("--skeleton", "-i", missing, *other)
        assert r.returncode == 1 and r.stderr.count("\n") == 1 and any(s in r.stderr for s in ("--skeleton: not with", "need --components", "need --distance")), (other, r.stderr)


def test_failure_order_of_the_skeleton_mode(tmp_path):
    """the stack's loader, then the refusal of --window on an 8-bit stack, then pnr_create: status 1, one line each, no output file --
    the order and the texts of test_cli_tool_order.py"""
    import torch
    import test_cli_tool_order as order
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    raw, missing, swc, vol = (str(tmp_path / n) for n in ("s.raw", "none.raw", "o.swc", "o.raw"))
    synth.synth(32, 24, 8, seed=1).tofile(raw)
    tail = ("-d", order.DIMS, "--threshold", "100", "--skeleton-rounds", "2", "--zscale", "2", "--swc", swc, "--skeleton-out", vol)
    for r, line in ((run("--skeleton", "-i", missing, *tail), "cannot open " + missing), (run("--window", "0,100", "--skeleton", "-i", missing, *tail), "cannot open " + missing),
                    (run("--window", "0,100", "--skeleton", "-i", raw, *tail), order.WINDOW), (run("--skeleton", "-i", raw, *tail), "pnr_create: " + order.NO_GPU)):
        assert (r.returncode, r.stderr, r.stdout) == (1, line + "\n", "")
        assert not os.path.exists(swc) and not os.path.exists(vol)
