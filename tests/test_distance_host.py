"""CPU (no GPU needed): the host side of the tree distance (include/pnr_hip.h) -- pnr_tree_sample against the rule restated in numpy
(distance_ref.py), its "count returned, call again" protocol and its argument errors, lib.read_swc, and advantra_cli --swc-info on
good and on malformed SWC files."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest
import pnr_amd
from pnr_amd import lib
import distance_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
F = np.float32


def trees():
    rng = np.random.default_rng(3)
    chain = (np.stack([np.arange(12) * 2.3, np.arange(12) * 0.4, np.arange(12) * 0.9], 1), np.arange(-1, 11))
    star = (np.concatenate([[[20, 20, 10]], 20 + rng.normal(0, 6, (9, 3))]), np.array([-1] + [0] * 9))
    forest = distance_ref.random_forest(rng, 60, roots=4)
    isolated = (rng.random((5, 3)) * 30, np.full(5, -1))
    # a segment of length exactly 5 (3-4-5: q = 5 / step without a remainder for step 0.5 and 1), one of length 0, a node that is
    # its own parent, parents after their children, and a parent below -1
    special = (np.array([[0, 0, 0], [3, 4, 0], [3, 4, 0], [7, 7, 7], [1, 1, 1], [10, 0, 0]]), np.array([-1, 0, 1, 3, 5, -7]))
    return {"chain": chain, "star": star, "forest": forest, "isolated": isolated, "special": special}


@pytest.mark.parametrize("step", [0, 0.5, 1, 3.7])
@pytest.mark.parametrize("zscale", [1, 2.5])
def test_tree_sample_matches_the_restatement(step, zscale):
    for name, (xyz, parent) in trees().items():
        pts, owner = lib.tree_sample(xyz, parent, zscale, step)
        want_p, want_o = distance_ref.tree_sample(xyz, parent, zscale, step)
        assert pts.dtype == F and owner.dtype == np.int32
        assert np.array_equal(owner, want_o), (name, step, zscale)
        assert np.array_equal(pts, want_p), (name, step, zscale, np.flatnonzero((pts != want_p).any(1))[:5])
        assert lib.tree_sample(xyz, parent, zscale, step, count_only=True) == len(want_p)
        if step == 0:
            assert np.array_equal(pts, distance_ref.scaled(xyz, zscale)) and np.array_equal(owner, np.arange(len(xyz)))


def test_tree_sample_closed_forms():
    """3-4-5: five steps of 1 give the four interior points k / 5 of the way from the node to its parent; step 0.5 gives nine; a
    step longer than the segment and a zero-length segment give none; zscale multiplies z before anything is measured"""
    xyz = np.array([[0, 0, 0], [3, 4, 0]], F)
    pts, owner = lib.tree_sample(xyz, [-1, 0], 1, 1)
    k = np.arange(1, 5, dtype=np.float64)[:, None] / 5
    assert np.array_equal(owner, [0, 1, 1, 1, 1, 1])
    assert np.array_equal(pts, np.concatenate([xyz, (np.array([3.0, 4, 0]) + np.array([-3.0, -4, 0]) * k).astype(F)]))
    assert lib.tree_sample(xyz, [-1, 0], 1, 0.5, count_only=True) == 2 + 9
    assert lib.tree_sample(xyz, [-1, 0], 1, 5, count_only=True) == 2 and lib.tree_sample(xyz, [-1, 0], 1, 7.5, count_only=True) == 2
    assert lib.tree_sample([[1, 2, 3], [1, 2, 3]], [-1, 0], 1, 0.25, count_only=True) == 2
    up = np.array([[0, 0, 0], [0, 0, 2]], F)
    pts, _ = lib.tree_sample(up, [-1, 0], 2.5, 1)  # length 5 after the scaling
    assert np.array_equal(pts, np.array([[0, 0, 0], [0, 0, 5], [0, 0, 4], [0, 0, 3], [0, 0, 2], [0, 0, 1]], F))


def test_tree_sample_capacity_protocol_and_errors():
    L = lib.load()
    xyz, parent = trees()["forest"]
    xyz = np.ascontiguousarray(xyz, F)
    parent = np.ascontiguousarray(parent, np.int32)
    want_p, want_o = distance_ref.tree_sample(xyz, parent, 1, 1)
    n = C.c_int64()

    def call(cap, pts=None, owner=None, x=xyz, par=parent, nn=None, zscale=1.0, step=1.0):
        return L.pnr_tree_sample(x.ctypes.data if x is not None else None, par.ctypes.data if par is not None else None, len(par) if nn is None else nn,
                                 zscale, step, pts.ctypes.data if pts is not None else None, owner.ctypes.data if owner is not None else None, cap, C.byref(n))

    assert call(0) == 0 and n.value == len(want_p) > len(xyz)
    for cap in (1, 7, len(want_p) - 1, len(want_p), len(want_p) + 3):  # too small: the count and the first cap points; then call again
        pts = np.full((cap + 1, 3), 77, F)
        owner = np.full(cap + 1, 77, np.int32)
        assert call(cap, pts, owner) == 0 and n.value == len(want_p)
        k = min(cap, len(want_p))
        assert np.array_equal(pts[:k], want_p[:k]) and np.array_equal(owner[:k], want_o[:k])
        assert (pts[k:] == 77).all() and (owner[k:] == 77).all()
    pts = np.zeros((len(want_p), 3), F)
    assert call(len(want_p), pts, None) == 0 and np.array_equal(pts, want_p)  # either output may be NULL
    assert call(0, nn=0, x=None, par=None) == 0 and n.value == 0              # an empty tree has no points
    for kw in (dict(zscale=0.0), dict(zscale=-1.0), dict(zscale=float("nan")), dict(zscale=float("inf")), dict(step=-0.5), dict(step=float("nan")),
               dict(nn=-1), dict(nn=lib.PNR_DISTANCE_MAX_N + 1), dict(x=None), dict(par=None, nn=len(parent)), dict(cap=-1)):
        cap = kw.pop("cap", 0)
        assert call(cap, **kw) == -1, kw
        assert L.pnr_last_error()
    bad_parent = parent.copy()
    bad_parent[5] = len(parent)
    assert call(0, par=bad_parent) == -1 and b"parent[5]" in L.pnr_last_error()
    for v in (np.nan, np.inf, -np.inf):
        bad = xyz.copy()
        bad[9, 1] = v
        assert call(0, x=bad) == -1 and b"node 9" in L.pnr_last_error()
    far = np.array([[0, 0, 0], [3e9, 0, 0]], F)
    assert call(0, x=far, par=np.array([-1, 0], np.int32), step=1.0) == -1  # more than 2^31 steps on one segment
    assert call(0, x=far, par=np.array([-1, 0], np.int32), step=0.0) == 0 and n.value == 2
    assert L.pnr_tree_sample(xyz.ctypes.data, parent.ctypes.data, len(parent), 1.0, 1.0, None, None, 0, None) == -1


# ---- SWC files: lib.read_swc and advantra_cli --swc-info ----
GOOD = """# a comment
#another
1 2 0 0 0 1.5 -1
2 2 3.0 4.0 0 1.5 1

3 2 3 4 12 0.5 2
4 6 10 10 10 1 -1
"""


def _info(path):
    r = subprocess.run([CLI, "--swc-info", str(path)], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout, r.stderr


def test_swc_info_and_read_swc(tmp_path):
    good = tmp_path / "good.swc"
    good.write_text(GOOD)
    rc, out, err = _info(good)
    assert rc == 0 and len(out.splitlines()) == 1, err
    assert json.loads(out) == {"nodes": 4, "roots": 2, "segments": 2, "length": 17.0, "bbox": [0, 0, 0, 10, 10, 12]}
    xyz, parent, ids = lib.read_swc(str(good))
    assert xyz.dtype == F and np.array_equal(xyz, [[0, 0, 0], [3, 4, 0], [3, 4, 12], [10, 10, 10]])
    assert np.array_equal(parent, [-1, 0, 1, -1]) and np.array_equal(ids, [1, 2, 3, 4])
    # ids written as floats, lines in another order, a parent that is not in the file: the same tree
    lines = ["3.0 2 3 4 12 0.5 2.0", "1.0 2 0 0 0 1.5 -1.0", "4 6 10 10 10 1 99", "2.0 2 3.0 4.0 0 1.5 1.0"]
    other = tmp_path / "other.swc"
    other.write_text("\n".join(lines) + "\n")
    rc, out2, err = _info(other)
    assert rc == 0 and json.loads(out2) == json.loads(out), err
    xyz2, parent2, ids2 = lib.read_swc(str(other))
    assert np.array_equal(ids2, [3, 1, 4, 2]) and np.array_equal(parent2, [3, -1, -1, 1])
    assert np.array_equal(xyz2[np.argsort(ids2)], xyz)
    # decimal coordinates: the f32 nearest to the double the text denotes, in both readers; the length is a sequential f64 sum
    rng = np.random.default_rng(1)
    pos = rng.random((40, 3)) * 100
    dec = tmp_path / "dec.swc"
    dec.write_text("".join(f"{i + 1} 2 {p[0]:.3f} {p[1]:.3f} {p[2]:.3f} 1.000 {i if i else -1}\n" for i, p in enumerate(pos)))
    x, par, _ = lib.read_swc(str(dec))
    assert np.array_equal(x, np.array([[float(f"{v:.3f}") for v in p] for p in pos]).astype(F)) and np.array_equal(par, np.arange(-1, 39))
    d = x[1:].astype(np.float64) - x[:-1].astype(np.float64)
    length = np.cumsum(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))[-1]
    rc, out, err = _info(dec)
    info = json.loads(out)
    assert rc == 0 and info["nodes"] == 40 and info["roots"] == 1 and info["segments"] == 39 and info["length"] == length
    assert np.array_equal(np.array(info["bbox"], F), np.concatenate([x.min(0), x.max(0)]))
    empty = tmp_path / "empty.swc"
    empty.write_text("# nothing\n")
    rc, out, err = _info(empty)
    assert rc == 0 and json.loads(out) == {"nodes": 0, "roots": 0, "segments": 0, "length": 0, "bbox": None}


@pytest.mark.parametrize("text,line,what", [
    (GOOD + "2 2 1 1 1 1 1\n", 8, "duplicate node id 2"),
    (GOOD + "# fine\n5 2 1 1 1 1\n", 9, "not an SWC line"),
    ("1 2 0 0 0 1 -1\n2 2 x 0 0 1 1\n", 2, "not a number"),
    ("1.5 2 0 0 0 1 -1\n", 1, "whole numbers"),
])
def test_malformed_swc_files_name_the_file_and_the_line(tmp_path, text, line, what):
    bad = tmp_path / "bad.swc"
    bad.write_text(text)
    rc, out, err = _info(bad)
    assert rc != 0 and out == "" and f"{bad}:{line}: " in err and what in err, err
    with pytest.raises(pnr_amd.PnrError, match=f"bad.swc:{line}: "):
        lib.read_swc(str(bad))
    # --distance fails the same way, before any GPU work
    good = tmp_path / "good.swc"
    good.write_text(GOOD)
    r = subprocess.run([CLI, "--distance", str(good), str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == "" and f"{bad}:{line}: " in r.stderr


def test_unreadable_swc_file_and_usage_errors(tmp_path):
    missing = tmp_path / "missing.swc"
    rc, out, err = _info(missing)
    assert rc != 0 and out == "" and str(missing) in err
    with pytest.raises(OSError):
        lib.read_swc(str(missing))
    good = tmp_path / "good.swc"
    good.write_text(GOOD)
    empty = tmp_path / "empty.swc"
    empty.write_text("")

    def cli(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)

    for args in (("--swc-info",), ("--distance", str(good)), ("--distance", str(good), str(good), "--zscale", "0"),
                 ("--distance", str(good), str(good), "--distance-step", "-1"), ("--distance", str(good), str(good), "--distance-threshold", "x"),
                 ("--distance-step", "1"), ("--per-node", "p"), ("--distance", str(good), str(missing)),
                 ("--distance", str(good), str(empty))):  # (an empty tree: refused by the library before a context exists)
        r = cli(*args)
        assert r.returncode != 0 and r.stdout == "" and r.stderr, args
    h = cli("--help")
    assert h.returncode == 0
    for flag in ("--swc-info", "--distance A.swc B.swc", "--distance-step", "--distance-threshold", "--zscale", "--per-node"):
        assert flag in h.stdout, flag
